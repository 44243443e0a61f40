"""-m gpu: csrc/kernels_track.hip and tracking.label_pairs / track_lesions / track_series against tests/track_oracle.py.  Every device result is an integer and every
float is computed on the host by the stated formula: every comparison is an equality (a NaN matches a NaN).  Every output is pre-filled with garbage and lies between
sentinels that must survive; a refused call must leave it untouched."""
import numpy as np
import pytest

import track_oracle as TO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
SHAPES = [(1, 1, 1), (2, 2, 2), (5, 3, 2), (64, 2, 2), (67, 5, 3), (130, 9, 7)]
GUARD = 8                                                           # sentinel elements either side of every output
FILL = -0x0123456789ABCDEF                                          # the garbage an output starts with
AFFINE = np.array([[-0.8, 0.0, 0.0, 90.0], [0.0, 0.75, 0.0, -60.0], [0.0, 0.0, 2.5, -30.0], [0.0, 0.0, 0.0, 1.0]])
CHUNK, LDS_SLOTS = 4096, 1024                                       # UNET_VOL_PAIRS_CHUNK, UNET_VOL_PAIRS_LDS_SLOTS (pinned by test_track_host.py)


def _flat(a):
    return np.asarray(a).reshape(-1, order="F")


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


class _In:
    """a label volume on the device, `offset` elements into its buffer (offset 1: off the 16-byte alignment of the vector path)"""

    def __init__(self, labels, offset=0):
        import torch
        flat = _flat(labels).astype(np.int32)
        self.t = torch.zeros(len(flat) + offset + 4, dtype=torch.int32, device="cuda")
        self.t[offset:offset + len(flat)] = torch.from_numpy(flat).cuda()
        self.ptr = self.t.data_ptr() + 4 * offset


class _Out:
    """n elements of garbage between two runs of sentinels; offset: elements the payload is shifted by (alignment)"""

    def __init__(self, n, dtype, offset=0):
        import torch
        self.n, self.lo = n, GUARD + offset
        fill = {torch.int64: FILL, torch.int32: -0x1234567, torch.uint8: 0x5A}[dtype]
        self.fill = fill
        self.t = torch.full((self.lo + n + GUARD,), fill, dtype=dtype, device="cuda")
        self.ptr = self.t.data_ptr() + self.lo * self.t.element_size()

    def get(self):
        a = self.t.cpu().numpy()
        assert (a[:self.lo] == self.fill).all() and (a[self.lo + self.n:] == self.fill).all(), "a sentinel beside an output was overwritten"
        return a[self.lo:self.lo + self.n]

    def untouched(self):
        return bool((self.t.cpu().numpy() == self.fill).all())


def _run_pairs(o, la, n_a, lb, n_b, shape, capacity, offset=0, rc=0):
    """-> (sorted keys, their counts, info, raw keys); refused calls (rc != 0) must leave all three outputs as they were"""
    a, b = _In(la, offset), _In(lb, offset)
    keys, counts, info = _Out(capacity, _i64()), _Out(capacity, _i64()), _Out(3, _i64())
    got = o.lib.unet_vol_label_pairs(o.h, a.ptr, n_a, b.ptr, n_b, *shape, keys.ptr, counts.ptr, capacity, info.ptr, o.s)
    if rc != 0:
        assert got == rc and keys.untouched() and counts.untouched() and info.untouched()
        return None
    o.ck(got, "label_pairs")
    k, c, i = keys.get().view(np.uint64), counts.get(), info.get()
    used = np.flatnonzero(k)
    assert (c[k == 0] == 0).all() and i[0] == len(used) and len(np.unique(k[used])) == len(used)          # empty slots hold no count; no pair sits in two slots
    assert int(c.sum()) + int(i[1]) == int(i[2])
    order = used[np.argsort(k[used])]
    return k[order], c[order], i


def _i64():
    import torch
    return torch.int64


def _random_labels(shape, n_a, n_b, rng, background=0.7, wild=False):
    la = rng.integers(1, n_a + 1, shape) if n_a else np.zeros(shape, np.int64)
    lb = rng.integers(1, n_b + 1, shape) if n_b else np.zeros(shape, np.int64)
    la, lb = la * (rng.random(shape) > background), lb * (rng.random(shape) > background)
    if wild:                                                        # values outside 0..n, negative and above: they count as 0
        for l, n in ((la, n_a), (lb, n_b)):
            l[rng.random(shape) < 0.1] = -3
            l[rng.random(shape) < 0.1] = n + 1
            l[rng.random(shape) < 0.05] = 2 ** 31 - 1
            l[rng.random(shape) < 0.05] = -2 ** 31
    return np.asfortranarray(la), np.asfortranarray(lb)


def _check_pairs(o, la, n_a, lb, n_b, shape, capacity, offset=0):
    wk, wc = TO.pair_table(la, n_a, lb, n_b)
    k, c, info = _run_pairs(o, la, n_a, lb, n_b, shape, capacity, offset)
    assert np.array_equal(k, wk) and np.array_equal(c, wc), (shape, offset)
    assert info.tolist() == [len(wk), 0, int(np.count_nonzero(TO.packed_keys(la, n_a, lb, n_b)))]
    return k, c


# ---- unet_vol_label_pairs -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_label_pairs_equal_the_oracle(shape):
    o = Ops()
    rng = np.random.default_rng(sum(shape))
    la, lb = _random_labels(shape, 5, 7, rng)
    first = _check_pairs(o, la, 5, lb, 7, shape, 64)
    again = _check_pairs(o, la, 5, lb, 7, shape, 64)                 # the same sorted table on every run
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    _check_pairs(o, la, 5, lb, 7, shape, 64, offset=1)               # both pointers off their 16-byte alignment: the scalar path
    wa, wb = _random_labels(shape, 5, 7, rng, wild=True)
    _check_pairs(o, wa, 5, wb, 7, shape, 64)
    _check_pairs(o, wa, 5, wb, 7, shape, 64, offset=1)
    _check_pairs(o, la, 0, lb, 7, shape, 16)                         # n_a = 0: every label of a counts as 0
    _check_pairs(o, la, 5, lb, 0, shape, 16)
    _check_pairs(o, la, 0, lb, 0, shape, 16)                         # nothing to count: an empty table


def test_label_pairs_hold_the_largest_labels():
    o = Ops()
    big = 2 ** 31 - 1
    rng = np.random.default_rng(5)
    shape = (67, 5, 3)
    la = np.asfortranarray(rng.choice([0, 1, big - 1, big], shape, p=[0.5, 0.2, 0.1, 0.2]))
    lb = np.asfortranarray(rng.choice([0, 2, big, -1], shape, p=[0.5, 0.2, 0.2, 0.1]))
    k, _ = _check_pairs(o, la, big, lb, big, shape, 32)
    assert int(k.max()) == (big << 32) | big


@pytest.fixture(scope="module")
def one_chunk():
    """one chunk of UNET_VOL_PAIRS_CHUNK voxels: (every voxel a pair of its own; the same volume in long runs of one pair)"""
    shape = (64, 8, CHUNK // 512)
    i = np.arange(CHUNK)
    distinct = ((i + 1).reshape(shape, order="F"), (i * 7 % 5).reshape(shape, order="F"))
    runs = ((1 + i // 512).reshape(shape, order="F"), (1 + i // 768).reshape(shape, order="F"))
    return shape, distinct, runs


def test_a_chunk_of_distinct_pairs_overfills_the_lds_stage(one_chunk):
    o = Ops()
    shape, (la, lb), _ = one_chunk
    assert CHUNK > LDS_SLOTS
    k, c = _check_pairs(o, la, CHUNK, lb, 4, shape, 4 * CHUNK)
    assert len(k) == CHUNK and (c == 1).all()
    _check_pairs(o, la, CHUNK, lb, 4, shape, 4 * CHUNK, offset=1)
    k, _ = _check_pairs(o, la, CHUNK, lb, 4, shape, CHUNK)           # a table loaded to exactly 1.0 completes
    assert len(k) == CHUNK


def test_long_runs_of_one_pair_are_summed_per_wave(one_chunk):
    o = Ops()
    shape, _, (la, lb) = one_chunk
    k, c = _check_pairs(o, la, 8, lb, 6, shape, 16)
    assert len(k) == 11 and int(c.sum()) == CHUNK and int(c.max()) == 512          # 11 runs of 256 or 512 voxels: whole waves hold one pair
    _check_pairs(o, la, 8, lb, 6, shape, 16, offset=1)


def test_a_workgroup_walks_several_chunks():
    """more than 1024 chunks, so every workgroup takes two; lesions as blocks, the way label volumes look"""
    o = Ops()
    shape = (250, 131, 131)
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    la = np.asfortranarray(((x // 25 + 10 * (y // 27) + 50 * (z // 30) + 1) * ((x % 25 < 17) & (y % 27 < 20) & (z % 30 < 19))).astype(np.int32))
    lb = np.asfortranarray(((x // 31 + 9 * (y // 22) + 54 * (z // 33) + 1) * ((x % 31 < 24) & (y % 22 < 15) & (z % 33 < 25))).astype(np.int32))
    n_a, n_b = int(la.max()), int(lb.max())
    assert (int(np.prod(shape)) + CHUNK - 1) // CHUNK > 1024
    k, _ = _check_pairs(o, la, n_a, lb, n_b, shape, 4096)
    assert len(k) > 256                                             # hundreds of lesions and their borders


def test_a_full_table_returns_and_says_what_it_dropped():
    o = Ops()
    shape = (40, 8, 4)
    la = np.asfortranarray((1 + np.arange(1280) // 32).reshape(shape, order="F"))          # 40 pairs (a, a % 7) of 32 voxels each
    lb = np.asfortranarray(la % 7)
    wk, wc = TO.pair_table(la, 40, lb, 6)
    assert len(wk) == 40
    k, c, info = _run_pairs(o, la, 40, lb, 6, shape, 16)
    assert info[0] == 16 and len(k) == 16 and info[1] > 0 and int(c.sum()) + int(info[1]) == int(info[2]) == 1280
    truth = dict(zip(wk.tolist(), wc.tolist()))
    assert all(truth.get(kk) == cc for kk, cc in zip(k.tolist(), c.tolist()))          # every stored key a true pair, every stored count that pair's true count


def test_label_pairs_refusals_and_empty_volumes():
    o = Ops()
    la = np.ones((2, 2, 2), np.int32)
    a, keys, counts, info = _In(la), _Out(32, _i64()), _Out(32, _i64()), _Out(3, _i64())
    call = lambda X=2, Y=2, Z=2, cap=32, na=1, nb=1, ap=a.ptr, bp=a.ptr, kp=keys.ptr, cp=counts.ptr, ip=info.ptr: \
        o.lib.unet_vol_label_pairs(o.h, ap, na, bp, nb, X, Y, Z, kp, cp, cap, ip, o.s)
    for kw in (dict(cap=24), dict(cap=8), dict(cap=0), dict(cap=-16), dict(cap=2 ** 31), dict(cap=2 ** 30 + 1), dict(X=2048, Y=1024, Z=1024), dict(X=65536, Y=65536, Z=0),
               dict(X=-1), dict(na=-1), dict(nb=-1), dict(ap=None), dict(bp=None), dict(kp=None), dict(cp=None), dict(ip=None), dict(kp=keys.ptr + 4), dict(ap=a.ptr + 2)):
        assert call(**kw) == E_ARG, kw
    import torch
    torch.cuda.synchronize()
    assert keys.untouched() and counts.untouched() and info.untouched()
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):                   # a zero dimension: UNET_OK, the outputs in their empty state
        keys, counts, info = _Out(32, _i64()), _Out(32, _i64()), _Out(3, _i64())
        o.ck(o.lib.unet_vol_label_pairs(o.h, None, 1, None, 1, *dims, keys.ptr, counts.ptr, 32, info.ptr, o.s), "empty")
        assert not keys.get().any() and not counts.get().any() and not info.get().any()


# ---- unet_vol_track_map ---------------------------------------------------------------------------------------------------------------------------------------
def _tables(n_a, n_b, rng):
    """random lookup and class tables whose entry 0 is NOT zero: it must read as 0"""
    lut_a, lut_b = rng.integers(1, 50, n_a + 1).astype(np.int32), rng.integers(1, 50, n_b + 1).astype(np.int32)
    cls_a, cls_b = rng.integers(0, 6, n_a + 1).astype(np.uint8), rng.integers(0, 6, n_b + 1).astype(np.uint8)
    lut_a[0], lut_b[0], cls_a[0], cls_b[0] = 99, -7, 5, 200
    return lut_a, lut_b, cls_a, cls_b


def _run_map(o, la, n_a, lb, n_b, shape, tables, offset=0, want=(True, True, True, True), rc=0):
    import torch
    N, Z = int(np.prod(shape)), shape[2]
    a, b = _In(la, offset), _In(lb, offset)
    tabs = [o.d(t, t.dtype) for t in tables]
    cls, ta, tb, ps = _Out(N, torch.uint8, offset), _Out(N, torch.int32, offset), _Out(N, torch.int32, offset), _Out(6 * Z, torch.int64)
    outs = [cls, ta, tb, ps]
    got = o.lib.unet_vol_track_map(o.h, a.ptr, n_a, b.ptr, n_b, *shape, *(t.data_ptr() for t in tabs), *(x.ptr if w else None for x, w in zip(outs, want)), o.s)
    if rc != 0:
        torch.cuda.synchronize()
        assert got == rc and all(x.untouched() for x in outs)
        return None
    o.ck(got, "track_map")
    for x, w in zip(outs, want):
        assert w or x.untouched()                                   # a null output is simply not written
    return [x.get() if w else None for x, w in zip(outs, want)]


def _check_map(o, la, n_a, lb, n_b, shape, tables, offset=0, want=(True, True, True, True)):
    wcls, wta, wtb, wps = TO.track_map(la, n_a, lb, n_b, *tables)
    cls, ta, tb, ps = _run_map(o, la, n_a, lb, n_b, shape, tables, offset, want)
    for got, w in ((cls, _flat(wcls)), (ta, _flat(wta)), (tb, _flat(wtb)), (ps, wps.reshape(-1))):
        assert got is None or np.array_equal(got, w), (shape, offset, want)
    if ps is not None:
        assert int(ps.sum()) == int(np.prod(shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_track_map_equals_the_oracle(shape):
    o = Ops()
    rng = np.random.default_rng(100 + sum(shape))
    la, lb = _random_labels(shape, 5, 7, rng, background=0.6, wild=True)
    tables = _tables(5, 7, rng)
    _check_map(o, la, 5, lb, 7, shape, tables)
    _check_map(o, la, 5, lb, 7, shape, tables, offset=1)             # inputs and outputs off their alignment
    for k in range(4):                                              # each output null in turn, then alone
        _check_map(o, la, 5, lb, 7, shape, tables, want=tuple(i != k for i in range(4)))
        _check_map(o, la, 5, lb, 7, shape, tables, offset=1, want=tuple(i == k for i in range(4)))
    _run_map(o, la, 5, lb, 7, shape, tables, want=(False, False, False, False), rc=E_ARG)
    for t in (2, 3):                                                # a class of 6 in either table
        bad = [x.copy() for x in tables]
        bad[t][-1] = 6
        _run_map(o, la, 5, lb, 7, shape, bad, rc=E_ARG)
        _check_map(o, la, 5, lb, 7, shape, bad, want=(False, True, True, False))          # ... is not read when no class is asked for
    _check_map(o, la, 0, lb, 7, shape, (tables[0][:1], tables[1], tables[2][:1], tables[3]))
    _check_map(o, la, 5, lb, 0, shape, (tables[0], tables[1][:1], tables[2], tables[3][:1]))


def test_track_map_over_whole_waves_slice_borders_and_several_chunks_per_workgroup():
    o = Ops()
    shape = (250, 131, 131)                                         # a slice is no multiple of a wave's 256 voxels; more than 1024 chunks
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    la = np.asfortranarray(((x // 25 + 10 * (y // 27) + 50 * (z // 30) + 1) * ((x % 25 < 17) & (y % 27 < 20) & (z % 30 < 19))).astype(np.int32))
    lb = np.asfortranarray(((x // 31 + 9 * (y // 22) + 54 * (z // 33) + 1) * ((x % 31 < 24) & (y % 22 < 15) & (z % 33 < 25))).astype(np.int32))
    n_a, n_b = int(la.max()), int(lb.max())
    _check_map(o, la, n_a, lb, n_b, shape, _tables(n_a, n_b, np.random.default_rng(9)))


def test_track_map_refusals_and_empty_volumes():
    import torch
    o = Ops()
    la = np.ones((2, 2, 2), np.int32)
    tables = _tables(1, 1, np.random.default_rng(1))
    a = _In(la)
    tabs = [o.d(t, t.dtype) for t in tables]
    cls, ta, tb, ps = _Out(8, torch.uint8), _Out(8, torch.int32), _Out(8, torch.int32), _Out(12, torch.int64)
    call = lambda X=2, Y=2, Z=2, na=1, nb=1, ap=a.ptr, bp=a.ptr, la_=tabs[0].data_ptr(), ca=tabs[2].data_ptr(), cp=cls.ptr, tp=ta.ptr, pp=ps.ptr: \
        o.lib.unet_vol_track_map(o.h, ap, na, bp, nb, X, Y, Z, la_, tabs[1].data_ptr(), ca, tabs[3].data_ptr(), cp, tp, tb.ptr, pp, o.s)
    for kw in (dict(X=-1), dict(X=2048, Y=1024, Z=1024), dict(na=-1), dict(nb=-1), dict(ap=None), dict(bp=None), dict(la_=None), dict(ca=None), dict(tp=ta.ptr + 2),
               dict(pp=ps.ptr + 4), dict(cp=a.ptr)):
        assert call(**kw) == E_ARG, kw
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        o.ck(call(*dims), "empty")
    torch.cuda.synchronize()
    assert cls.untouched() and ta.untouched() and tb.untouched()
    assert not ps.get().any()                                       # (a volume of empty slices zeroes their counts and nothing else)


# ---- label_pairs, track_lesions, track_series ----------------------------------------------------------------------------------------------------------------------
def test_label_pairs_grows_its_table_until_everything_fits(monkeypatch):
    from covidseg_amd import tracking as T
    shape = (64, 8, CHUNK // 512)
    i = np.arange(CHUNK)
    la, lb = (i + 1).reshape(shape, order="F"), (i * 7 % 5).reshape(shape, order="F")
    want = TO.pairs(la, CHUNK, lb, 4)
    monkeypatch.setattr(T, "first_capacity", lambda n_a, n_b: 16)    # 16 -> 64 -> 256 -> 1024 -> 4096
    seen = []
    real = T.label_pairs_device
    monkeypatch.setattr(T, "label_pairs_device", lambda *a: seen.append(a[-1]) or real(*a))
    got = T.label_pairs(la, CHUNK, lb, 4)
    assert got.dtype == T.PAIR_DTYPE and got.tolist() == want.tolist() and seen == [16, 64, 256, 1024, 4096]
    import torch
    dev = [torch.from_numpy(_flat(l).astype(np.int32)).cuda() for l in (la, lb)]
    assert T.label_pairs(dev[0], CHUNK, dev[1], 4, shape=shape).tolist() == want.tolist()


@pytest.fixture(scope="module")
def scene():
    ma, mb = TO.scene()
    return ma, mb


def _check_tracking(res, mask_a, b_on_a, change, kw):
    from covidseg_amd import tracking as T
    la, n_a = TO.label(mask_a, kw.get("connectivity", 1))
    lb, n_b = TO.label(b_on_a, kw.get("connectivity", 1))
    want = TO.track(la, n_a, lb, n_b, AFFINE, kw.get("min_overlap_voxels", 1), kw.get("min_fraction", 0.0), kw.get("interval_days"))
    assert (res.n_a, res.n_b) == (n_a, n_b) and res.pairs.tolist() == want["pairs"].tolist()
    m = want["match"]
    assert np.array_equal(res.match.lut_a, m["lut_a"]) and np.array_equal(res.match.lut_b, m["lut_b"]) and res.match.events == m["events"]
    assert [x.tolist() for x in res.labels_a] == m["members_a"] and [x.tolist() for x in res.labels_b] == m["members_b"]
    assert len(res.tracks) == len(want["rows"]) and res.tracks.dtype == T.TRACK_DTYPE
    for got, w in zip(res.tracks, want["rows"]):
        for k in T.TRACK_DTYPE.names:
            assert (got[k] == w[k]) if k == "event" else _same(got[k], w[k]), (k, got[k], w[k])
    assert np.array_equal(res.class_map, want["cls"]) and np.array_equal(res.track_a, want["track_a"]) and np.array_equal(res.track_b, want["track_b"])
    assert res.class_map.dtype == np.uint8 and res.track_a.dtype == np.int32 and np.array_equal(res.per_slice, want["per_slice"])
    assert (res.persistent, res.new, res.resolved) == (want["persistent"], want["new"], want["resolved"]) == (change.persistent, change.new, change.resolved)
    assert (res.persistent_ml, res.new_ml, res.resolved_ml) == (change.persistent_ml, change.new_ml, change.resolved_ml) and _same(res.dice, change.dice)
    assert np.array_equal(res.b_on_a, change.b_on_a) and np.array_equal(res.b_on_a != 0, np.asarray(b_on_a) != 0)
    assert sum(v["count"] for v in res.events.values()) == len(res.tracks)
    assert int(res.tracks["voxels_a"].sum()) == int((mask_a != 0).sum()) and int(res.tracks["voxels_b"].sum()) == int((np.asarray(b_on_a) != 0).sum())
    return want


def test_track_lesions_on_identical_grids(scene):
    from covidseg_amd import tracking as T, volume as V
    ma, mb = scene
    g = V.Grid(ma.shape, AFFINE)
    kw = dict(interval_days=90)
    res = T.track_lesions(ma, g, mb, g, **kw)
    want = _check_tracking(res, ma, mb, V.change_between(ma, g, mb, g), kw)
    assert sorted(res.tracks["event"].tolist()) == sorted(["persistent", "persistent", "merged", "split", "complex", "resolved", "new"])
    assert int(res.tracks["overlap"].sum()) == res.persistent
    grown = res.tracks[(res.tracks["event"] == "persistent") & (res.tracks["voxels_b"] > res.tracks["voxels_a"])][0]
    assert grown["doubling_time_days"] > 0 and grown["change_pct"] > 100
    assert set(np.unique(res.class_map)) == {0, 1, 2, 3, 4, 5}
    # the thresholds reach the match; the maps may stay on the device; the class map is an overlay of render_planes
    cut = T.track_lesions(ma, g, mb, g, min_fraction=0.9, connectivity=3)
    _check_tracking(cut, ma, mb, V.change_between(ma, g, mb, g), dict(min_fraction=0.9, connectivity=3))
    assert len(cut.tracks) > len(res.tracks)
    import torch
    dev = T.track_lesions(torch.from_numpy(_flat(ma)).cuda(), g, torch.from_numpy(_flat(mb)).cuda(), g, return_device=True, **kw)
    assert dev.class_map.is_cuda and np.array_equal(dev.class_map.cpu().numpy(), _flat(want["cls"])) and np.array_equal(dev.track_b.cpu().numpy(), _flat(want["track_b"]))
    ct = np.asfortranarray(np.where(ma | mb, 40, -800).astype(np.int16))
    z = int(np.argmax(res.per_slice[:, 1:].sum(axis=1)))
    sheet = V.render_planes(ct, [("axial", z), ("coronal", 6)], layers=[res.layer()], window=(-1000.0, 400.0))
    colours = {tuple(c) for c in sheet.image.reshape(-1, 3)}
    assert sheet.image.ndim == 3 and len(colours) > 4                # grey levels and several class colours
    assert V.render_planes(ct, [("axial", z)], layers=[dev.layer()], window=(-1000.0, 400.0), shape=ma.shape).image.shape[2] == 3


def test_track_lesions_with_a_follow_up_on_a_coarser_grid(scene):
    from covidseg_amd import tracking as T, volume as V
    ma, mb = scene
    ga = V.Grid(ma.shape, AFFINE)
    coarse = np.asfortranarray(mb[::2, ::2, ::2])
    gb = V.Grid(coarse.shape, AFFINE @ np.diag([2.0, 2.0, 2.0, 1.0]))
    change = V.change_between(ma, ga, coarse, gb)
    res = T.track_lesions(ma, ga, coarse, gb)
    assert res.b_on_a.shape == ma.shape and not np.array_equal(res.b_on_a, mb) and res.persistent > 0
    _check_tracking(res, ma, change.b_on_a, change, {})


def test_track_lesions_through_a_rigid_transform(scene):
    from covidseg_amd import tracking as T, volume as V
    ma, mb = scene
    g = V.Grid(ma.shape, AFFINE)
    rigid = V.RigidTransform((1.7, -0.8, 2.6) + tuple(np.deg2rad([1.0, -2.0, 3.0])), (72.0, -46.0, -2.0))
    change = V.change_between(ma, g, mb, g, transform=rigid)
    res = T.track_lesions(ma, g, mb, g, transform=rigid, interval_days=30.5)
    assert not np.array_equal(res.b_on_a, mb) and res.persistent > 0
    _check_tracking(res, ma, change.b_on_a, change, dict(interval_days=30.5))
    as_matrix = T.track_lesions(ma, g, mb, g, transform=rigid.matrix, interval_days=30.5)
    assert np.array_equal(as_matrix.class_map, res.class_map) and as_matrix.match.events == res.match.events and _same(as_matrix.tracks["shift_mm"], res.tracks["shift_mm"])


def test_track_lesions_through_a_displacement_field(scene):
    import torch
    from covidseg_amd import tracking as T, volume as V
    ma, mb = scene
    g = V.Grid(ma.shape, AFFINE)
    N = int(np.prod(ma.shape))
    u = np.zeros((3, N), np.float32)
    u[0], u[2] = 1.6, -2.5                                          # two voxels along x (the affine's -0.8 mm), one slice down
    u[1, :N // 2] = 0.75
    field = V.DisplacementField(torch.from_numpy(u.reshape(-1)).cuda(), g, np.eye(4), g, g)
    deform = V.DeformableRegistration(field=field)
    change = V.change_between(ma, g, mb, g, transform=deform)
    res = T.track_lesions(ma, g, mb, g, transform=deform)
    assert not np.array_equal(res.b_on_a, mb) and res.persistent > 0
    _check_tracking(res, ma, change.b_on_a, change, {})


def test_track_series_over_three_time_points(scene):
    from covidseg_amd import tracking as T, volume as V
    ma, mb = scene
    g = V.Grid(ma.shape, AFFINE)
    mc = np.asfortranarray(mb.copy())
    mc[:24] = 0                                                     # the third time point: half of the follow-up is gone
    coarse = np.asfortranarray(mc[::2, ::2, ::2])
    gc = V.Grid(coarse.shape, AFFINE @ np.diag([2.0, 2.0, 2.0, 1.0]))
    res = T.track_series([ma, mb, coarse], [g, g, gc])
    c_on_a = V.change_between(ma, g, coarse, gc).b_on_a
    labelled = [TO.label(m) for m in (ma, mb, c_on_a)]
    sizes = [np.bincount(l.reshape(-1), minlength=n + 1).astype(np.int64) for l, n in labelled]
    matches = [TO.match(TO.pairs(labelled[s][0], labelled[s][1], labelled[s + 1][0], labelled[s + 1][1]), labelled[s][1], labelled[s + 1][1]) for s in range(2)]
    lineage_of, voxels, first, last, events = TO.chain(matches, sizes)
    assert res.n_times == 3 and res.n_lineages == len(voxels) and res.counts == [n for _, n in labelled]
    assert np.array_equal(res.voxels, voxels) and np.array_equal(res.ml, voxels * g.voxel_ml) and res.ml.shape == (len(voxels), 3)
    assert np.array_equal(res.first, first) and np.array_equal(res.last, last) and res.events == events
    assert all(np.array_equal(a, b) for a, b in zip(res.lineage_of, lineage_of))
    assert any("resolved" in e for e in res.events) and int(res.voxels[:, 0].sum()) == int(ma.sum())

"""-m gpu: csrc/kernels_mesh.hip and volume.extract_surface / lesion_shapes / segment_volume(mesh=) against tests/mesh_oracle.py.  Every comparison is an equality of the
stored bits (a NaN matches a NaN): the totals, the flag and count bytes of the workspace, vertices, triangles, groups, per-triangle area and signed volume.  Every output is
pre-filled with garbage and lies between sentinels that must survive, and a refused call must leave it untouched.  Only counts of differences are printed."""
import numpy as np
import pytest

import mesh_oracle as MO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
CHUNK = 2048                                                        # lattice points per workgroup of the scans (csrc/kernels_mesh.hip: TPB * PER)
SMALL = [(1, 1, 1), (2, 2, 2), (5, 3, 2), (64, 2, 2), (67, 5, 3), (130, 9, 7)]          # x: one voxel .. on a wave, past a wave, past two waves
INPUTS = ["mask_u1_off1", "labels_any", "labels_one", "f4_nonfinite", "i2_scaled", "f8"]
SENTINEL = 0x5A
GUARD = 64
MASK, LABELS, SCALAR = 0, 1, 2


def _oblique():
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
    return np.hstack([R * np.array([0.7, 0.8, 2.5]), [[-31.5], [12.25], [100.0]]])


MATRICES = [MO.default_matrix(), MO.default_matrix((0.7, 0.8, 2.5)), _oblique()]


class Case:
    """an input as the entry points take it (raw, kind, code, scaling, element offset of the upload, iso, select, pad_value) and as the oracle takes it"""

    def __init__(self, raw, kind, code, scaling=None, offset=0, iso=0.5, select=0, pad=0.0):
        self.raw, self.kind, self.code, self.scaling, self.offset, self.iso, self.select, self.pad = np.asfortranarray(raw), kind, code, scaling, offset, iso, select, pad

    def vargs(self):
        return (self.code,) + tuple(int(v) for v in self.raw.shape) + ((1, float(self.scaling[0]), float(self.scaling[1])) if self.scaling else (0, 1.0, 0.0))

    def oracle(self, closed, M):
        if self.kind == MASK:
            return MO.extract(mask=self.raw, closed=closed, matrix=M)
        if self.kind == LABELS:
            return MO.extract(labels=self.raw, select=self.select, closed=closed, matrix=M)
        v = self.raw.astype(np.float64)
        if self.scaling:
            v = v * np.float64(self.scaling[0]) + np.float64(self.scaling[1])          # get_fdata's two rounded operations
        return MO.extract(values=v, iso=self.iso, closed=closed, pad_value=self.pad, matrix=M)


def _case(shape, name, seed):
    rng = np.random.default_rng(seed)
    if name == "mask_u1_off1":
        return Case((rng.random(shape) < 0.5).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8), MASK, 2, offset=1)          # any non-zero byte is inside
    if name.startswith("labels"):
        lab = np.where(rng.random(shape) < 0.5, rng.integers(1, 4, shape), 0).astype(np.int32)
        if min(shape) >= 2:
            lab[0, 0, 0], lab[1, 1, 0] = 1, 2                       # two labels that touch along a face diagonal
        return Case(lab, LABELS, 8, select=0 if name == "labels_any" else 2)
    if name == "f4_nonfinite":
        raw = np.round(rng.normal(size=shape) * 3).astype(np.float32)          # many values equal iso = 0
        bad = rng.random(shape)
        raw[bad < 0.08] = np.nan; raw[(bad >= 0.08) & (bad < 0.12)] = np.inf; raw[(bad >= 0.12) & (bad < 0.16)] = -np.inf
        return Case(raw, SCALAR, 16, iso=0.0, pad=-2.5)
    if name == "i2_scaled":
        return Case(rng.integers(-1200, 600, shape).astype(np.int16), SCALAR, 4, scaling=(0.5, -100.0), iso=-300.0, pad=-300.0)          # values equal iso too (raw -400)
    return Case(rng.normal(size=shape) * 400 - 300, SCALAR, 64, iso=-250.0, pad=-1e4)


def _up(a, offset=0):
    """the bytes of `a` in Fortran order on the device, `offset` elements into a larger buffer -> (tensor kept alive, pointer)"""
    import torch
    a = np.asarray(a)
    flat = np.asfortranarray(a).reshape(-1, order="F").view(np.uint8)
    buf = torch.zeros(flat.size + 64 + offset * a.itemsize, dtype=torch.uint8, device="cuda")
    buf[offset * a.itemsize:offset * a.itemsize + flat.size] = torch.from_numpy(flat.copy()).cuda()
    return buf, buf.data_ptr() + offset * a.itemsize


def _out(nbytes):
    import torch
    return torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")          # garbage where the output goes


def _take(buf, dtype=np.uint8):
    """the output between its sentinels"""
    h = buf.cpu().numpy()
    n = h.size - 2 * GUARD
    assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + n:] == SENTINEL).all(), "a sentinel around the output was overwritten"
    return h[GUARD:GUARD + n].copy().view(dtype)


def _untouched(buf):
    return bool((buf.cpu().numpy() == SENTINEL).all())


def _count(o, case, ptr, closed):
    """unet_vol_mesh_count -> (nv, nt, ws buffer between sentinels, its size)"""
    X, Y, Z = case.raw.shape
    n = int(o.lib.unet_vol_mesh_ws_bytes(X, Y, Z, int(closed)))
    ws, totals = _out(max(n, 16)), _out(16)
    o.ck(o.lib.unet_vol_mesh_count(o.h, ptr, case.kind, *case.vargs(), float(case.iso), case.select, int(closed), float(case.pad), ws.data_ptr() + GUARD, n,
                                   totals.data_ptr() + GUARD, o.s), "vol_mesh_count")
    nv, nt = (int(v) for v in _take(totals, np.int64))
    return nv, nt, ws, n


def _emit(o, case, ptr, closed, M, ws, n_ws, cap_v, cap_t, groups=True):
    v, t, g = _out(12 * cap_v), _out(12 * cap_t), _out(4 * cap_t)
    o.ck(o.lib.unet_vol_mesh_emit(o.h, ptr, case.kind, *case.vargs(), float(case.iso), case.select, int(closed), float(case.pad), np.ascontiguousarray(M, np.float64).ctypes.data,
                                  ws.data_ptr() + GUARD, n_ws, v.data_ptr() + GUARD if cap_v else None, cap_v, t.data_ptr() + GUARD if cap_t else None,
                                  (g.data_ptr() + GUARD) if (groups and cap_t) else None, cap_t, o.s), "vol_mesh_emit")
    return _take(v, np.float32).reshape(-1, 3), _take(t, np.int32).reshape(-1, 3), (_take(g, np.int32) if groups else g)


def _measure(o, v, t):
    import torch
    nt = len(t)
    dv, dt = torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(t)).cuda()
    a, s = _out(8 * nt), _out(8 * nt)
    o.ck(o.lib.unet_vol_mesh_measure(o.h, dv.data_ptr() if len(v) else None, len(v), dt.data_ptr() if nt else None, nt, a.data_ptr() + GUARD, s.data_ptr() + GUARD, o.s),
         "vol_mesh_measure")
    return _take(a, np.float64), _take(s, np.float64)


def _differ(got, want):
    """the number of elements whose bits differ (-1: another shape)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return -1
    if got.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        both = np.isnan(got) & np.isnan(want)
        return int((np.where(both, 0, np.ascontiguousarray(got).view(u)) != np.where(both, 0, np.ascontiguousarray(want).view(u))).sum())
    return int((got != want).sum())


def _check_all(o, case, closed_list=(True, False), matrices=MATRICES, measure=True):
    buf, ptr = _up(case.raw, case.offset)
    for closed in closed_list:
        nv, nt, ws, n_ws = _count(o, case, ptr, closed)
        want = case.oracle(closed, matrices[0])
        assert (nv, nt) == (len(want.vertices), len(want.triangles)), f"totals {(nv, nt)} != {(len(want.vertices), len(want.triangles))} closed={closed}"
        npts = int(np.prod(want.lattice))
        if n_ws:
            w = _take(ws)
            npad = (npts + 15) // 16 * 16
            assert _differ(w[:npts], want.flags) == 0, f"{_differ(w[:npts], want.flags)} flag bytes differ, closed={closed}"
            assert _differ(w[npad:npad + npts], want.counts) == 0, f"{_differ(w[npad:npad + npts], want.counts)} count bytes differ, closed={closed}"
        else:
            assert (nv, nt) == (0, 0) and _untouched(ws)
        for k, M in enumerate(matrices):
            if k:
                want = case.oracle(closed, M)
            v, t, g = _emit(o, case, ptr, closed, M, ws, n_ws, nv, nt)
            assert _differ(v, want.vertices) == 0, f"{_differ(v, want.vertices)} of {v.size} vertex coordinates differ, closed={closed} matrix {k}"
            assert _differ(t, want.triangles) == 0, f"{_differ(t, want.triangles)} of {t.size} triangle indices differ, closed={closed} matrix {k}"
            assert _differ(g, want.groups) == 0, f"{_differ(g, want.groups)} of {g.size} groups differ, closed={closed} matrix {k}"
            if measure and nt:
                a, s = _measure(o, v, t)
                wa, ws_ = MO.measure(want.vertices, want.triangles)
                assert _differ(a, wa) == 0 and _differ(s, ws_) == 0, f"{_differ(a, wa)} areas, {_differ(s, ws_)} signed volumes of {nt} differ, closed={closed} matrix {k}"
    del buf


# ---- every input on the small shapes, closed and open, three matrices -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes_match_the_oracle(shape, name):
    _check_all(Ops(), _case(shape, name, seed=sum(shape) + len(name)))


@pytest.mark.parametrize("X", [2045, 2050])
def test_rows_at_the_staging_limit(X):
    """closed, a row of the lattice holds X + 2 points: 2047 is the longest row whose halo (a row + 1) fits beside the CHUNK = 2048 points the count kernel stages in LDS,
    2052 takes its other path, the overlapping loads"""
    _check_all(Ops(), _case((X, 3, 2), "mask_u1_off1", X), closed_list=(True,), matrices=MATRICES[2:])
    _check_all(Ops(), _case((X, 2, 2), "f4_nonfinite", X), matrices=MATRICES[:1], measure=False)


def test_the_256_corner_patterns():
    o = Ops()
    case = Case(MO.pattern_volume(), MASK, 2)
    _check_all(o, case, matrices=MATRICES[:1])
    buf, ptr = _up(case.raw)
    nv, nt, _, _ = _count(o, case, ptr, True)
    assert (nv, nt) == (11904, 22656)


def test_chunk_boundaries_inside_rows():
    """(131, 33, 17) padded is 133 x 35 x 19 = 88 445 lattice points = 44 chunks of CHUNK = 2048 points; 2048 is no multiple of 133, so every chunk boundary lies inside a
    row, and the four owner rows of a chunk's cells reach into the next chunks"""
    assert (133 * 35 * 19 + CHUNK - 1) // CHUNK == 44 and CHUNK % 133 != 0
    o = Ops()
    _check_all(o, _case((131, 33, 17), "mask_u1_off1", 5), matrices=MATRICES[2:])
    _check_all(o, _case((131, 33, 17), "labels_any", 6), closed_list=(True,), matrices=MATRICES[:1], measure=False)


def test_two_small_balls_in_emptiness_take_the_skip_path():
    shape = (96, 64, 40)
    f = np.maximum(MO.ball_field(shape, (20.3, 30.1, 12.2), 5.0), MO.ball_field(shape, (70.6, 21.4, 29.7), 3.5)).astype(np.float32)
    case = Case(f, SCALAR, 16, iso=0.0, pad=-100.0)
    o = Ops()
    _check_all(o, case, matrices=MATRICES[1:2])
    want = case.oracle(True, MATRICES[0])
    assert MO.is_closed_manifold(want.triangles) and MO.euler(len(want.vertices), want.triangles) == 4 and np.count_nonzero(want.counts) * 50 < want.counts.size


@pytest.mark.parametrize("fill", [0, 1])
def test_all_zero_and_all_one_volumes(fill):
    o = Ops()
    case = Case(np.full((67, 5, 3), fill, np.uint8), MASK, 2)
    _check_all(o, case, matrices=MATRICES[:1])
    buf, ptr = _up(case.raw)
    assert _count(o, case, ptr, False)[:2] == (0, 0)                 # open: nothing is crossed either way
    nv, nt = _count(o, case, ptr, True)[:2]
    assert (nv, nt) == ((0, 0) if fill == 0 else (len(case.oracle(True, MATRICES[0]).vertices), len(case.oracle(True, MATRICES[0]).triangles))) and (fill == 0 or nv - nt // 2 == 2)


# ---- capacities -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_capacity_below_the_total_writes_exactly_that_many_items():
    o = Ops()
    case = _case((67, 5, 3), "labels_any", 3)
    buf, ptr = _up(case.raw)
    nv, nt, ws, n_ws = _count(o, case, ptr, True)
    want = case.oracle(True, MATRICES[2])
    assert nv > 40 and nt > 40
    for cap_v, cap_t in ((nv - 7, nt), (nv, nt - 5), (13, 29), (0, nt), (nv, 0), (0, 0)):
        v, t, g = _emit(o, case, ptr, True, MATRICES[2], ws, n_ws, cap_v, cap_t)          # _out: each buffer is exactly `capacity` items between its sentinels
        assert _differ(v, want.vertices[:cap_v]) == 0 and _differ(t, want.triangles[:cap_t]) == 0 and _differ(g, want.groups[:cap_t]) == 0, (cap_v, cap_t)
    v, t, g = _emit(o, case, ptr, True, MATRICES[2], ws, n_ws, nv, nt, groups=False)     # groups is nullable
    assert _differ(t, want.triangles) == 0 and _untouched(g)
    import torch
    big_v, big_t = _out(12 * (nv + 10)), _out(12 * (nt + 10))                             # a capacity above the total: nothing past the total is written
    o.ck(o.lib.unet_vol_mesh_emit(o.h, ptr, case.kind, *case.vargs(), float(case.iso), case.select, 1, float(case.pad), MATRICES[2].ctypes.data, ws.data_ptr() + GUARD, n_ws,
                                  big_v.data_ptr() + GUARD, nv + 10, big_t.data_ptr() + GUARD, None, nt + 10, o.s), "vol_mesh_emit")
    assert (_take(big_v)[12 * nv:] == SENTINEL).all() and (_take(big_t)[12 * nt:] == SENTINEL).all()
    assert _differ(_take(big_v, np.float32)[:3 * nv].reshape(-1, 3), want.vertices) == 0
    del torch


# ---- determinism and the sums ---------------------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes_and_the_sums_have_a_fixed_shape():
    import torch
    from covidseg_amd import volume as V
    o = Ops()
    case = _case((130, 9, 7), "labels_any", 9)
    buf, ptr = _up(case.raw)
    runs = []
    for _ in range(2):
        nv, nt, ws, n_ws = _count(o, case, ptr, True)
        v, t, g = _emit(o, case, ptr, True, MATRICES[2], ws, n_ws, nv, nt)
        a, s = _measure(o, v, t)
        runs.append((_take(ws).tobytes(), v.tobytes(), t.tobytes(), g.tobytes(), a.tobytes(), s.tobytes()))
    assert runs[0] == runs[1]
    assert nt > 2 * MO.CHUNK                                          # more than one partial sum per group
    per = torch.from_numpy(np.stack([a, s])).cuda()
    want_a, want_s = MO.measure(v, t)
    sums = [V.mesh_group_sums(per, torch.from_numpy(g).cuda()) for _ in range(2)]
    totals, ids, counts, gs = sums[0]
    assert all(np.array_equal(x, y) for x, y in zip(sums[0], sums[1]))
    assert ids.tolist() == [1, 2, 3] and counts.tolist() == [int((g == i).sum()) for i in ids]
    assert _differ(totals, np.array([MO.two_level_sum(want_a), MO.two_level_sum(want_s)])) == 0
    assert _differ(gs, np.stack([MO.group_sums(want_a, g, ids), MO.group_sums(want_s, g, ids)])) == 0
    t1, i1, c1, g1 = V.mesh_group_sums(per, None)
    assert i1.tolist() == [1] and c1.tolist() == [nt] and _differ(g1[:, 0], totals) == 0


def test_measure_never_takes_a_bad_index_for_an_address():
    o = Ops()
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    t = np.array([[0, 2, 1], [0, 1, 4], [-1, 1, 2], [1, 2, 3]], np.int32)
    a, s = _measure(o, v, t)
    assert a[0] == 0.5 and s[0] == 0.0 and np.isnan(a[1:3]).all() and np.isnan(s[1:3]).all() and s[3] == 1.0 / 6.0


# ---- refusals: UNET_E_ARG before any launch, every output untouched -----------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_their_outputs_untouched():
    import torch
    o = Ops()
    lab = _case((5, 3, 2), "labels_any", 1)
    f4 = _case((5, 3, 2), "f4_nonfinite", 2)
    bufs = {c: _up(c.raw) for c in (lab, f4)}
    n_ws = int(o.lib.unet_vol_mesh_ws_bytes(5, 3, 2, 1))
    ws, totals, v, t, g = _out(n_ws), _out(16), _out(12 * 400), _out(12 * 400), _out(4 * 400)
    M = MATRICES[2].copy()

    def count(case, ptr=None, kind=None, code=None, dims=None, iso=None, select=None, pad=None, wsp=None, wsn=None, tot=None):
        va = list(case.vargs())
        if code is not None:
            va[0] = code
        if dims is not None:
            va[1:4] = dims
        return o.lib.unet_vol_mesh_count(o.h, bufs[case][1] if ptr is None else ptr[0], case.kind if kind is None else kind, *va, float(case.iso if iso is None else iso),
                                         case.select if select is None else select, 1, float(case.pad if pad is None else pad), (ws.data_ptr() + GUARD) if wsp is None else wsp[0],
                                         n_ws if wsn is None else wsn, (totals.data_ptr() + GUARD) if tot is None else tot[0], o.s)

    def emit(case, mat=M, cap_v=400, cap_t=400, vp=None, iso=None, pad=None, select=None, code=None, wsn=None):
        va = list(case.vargs())
        if code is not None:
            va[0] = code
        return o.lib.unet_vol_mesh_emit(o.h, bufs[case][1], case.kind, *va, float(case.iso if iso is None else iso), case.select if select is None else select, 1,
                                        float(case.pad if pad is None else pad), mat.ctypes.data if mat is not None else None, ws.data_ptr() + GUARD, n_ws if wsn is None else wsn,
                                        (v.data_ptr() + GUARD) if vp is None else vp[0], cap_v, t.data_ptr() + GUARD, g.data_ptr() + GUARD, cap_t, o.s)
    bad_m = M.copy(); bad_m[1, 2] = np.nan
    inf_m = M.copy(); inf_m[2, 3] = np.inf
    refused = [
        count(lab, ptr=(None,)), count(lab, ptr=(bufs[lab][1] + 1,)), count(f4, ptr=(bufs[f4][1] + 2,)),          # null, misaligned to the element size
        count(lab, kind=3), count(lab, kind=-1), count(lab, code=16), count(lab, kind=MASK), count(f4, code=3), count(f4, code=0),          # kind / datatype
        count(lab, dims=(-1, 3, 2)), count(lab, dims=(2047, 1023, 1023)), count(lab, dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)),          # a lattice of 2^31 points or more
        count(f4, iso=np.nan), count(f4, iso=np.inf), count(f4, pad=np.nan), count(f4, pad=-np.inf), count(f4, pad=0.5),          # non-finite; pad_value > iso
        count(lab, select=-1),
        count(lab, wsp=(None,)), count(lab, wsp=(ws.data_ptr() + GUARD + 8,)), count(lab, wsn=n_ws - 1), count(lab, tot=(None,)), count(lab, tot=(totals.data_ptr() + GUARD + 4,)),
        emit(lab, mat=bad_m), emit(lab, mat=inf_m), emit(lab, mat=None), emit(lab, cap_v=-1), emit(lab, cap_t=-1), emit(lab, cap_v=2 ** 31), emit(lab, vp=(None,)),
        emit(lab, vp=(v.data_ptr() + GUARD + 2,)), emit(f4, iso=np.nan), emit(f4, pad=1.0), emit(lab, select=-2), emit(f4, code=5), emit(lab, wsn=n_ws - 16),
        o.lib.unet_vol_mesh_measure(o.h, v.data_ptr() + GUARD, -1, t.data_ptr() + GUARD, 4, ws.data_ptr() + GUARD, None, o.s),
        o.lib.unet_vol_mesh_measure(o.h, v.data_ptr() + GUARD, 4, None, 4, ws.data_ptr() + GUARD, None, o.s),
        o.lib.unet_vol_mesh_measure(o.h, v.data_ptr() + GUARD, 4, t.data_ptr() + GUARD, 4, ws.data_ptr() + GUARD + 4, None, o.s),
    ]
    torch.cuda.synchronize()
    assert all(rc == E_ARG for rc in refused), [i for i, rc in enumerate(refused) if rc != E_ARG]
    assert all(_untouched(b) for b in (ws, totals, v, t, g))
    # a volume with a zero dimension, an unpadded extent of 1: totals (0, 0), nothing else touched, and nothing is read (null volume, null workspace)
    for dims, closed in (((0, 3, 2), 1), ((5, 0, 2), 0), ((5, 3, 0), 1), ((5, 1, 2), 0), ((1, 1, 1), 0)):
        tot = _out(16)
        o.ck(o.lib.unet_vol_mesh_count(o.h, None, MASK, 2, *dims, 0, 1.0, 0.0, 0.5, 0, closed, 0.0, None, 0, tot.data_ptr() + GUARD, o.s), "vol_mesh_count")
        assert _take(tot, np.int64).tolist() == [0, 0]
        o.ck(o.lib.unet_vol_mesh_emit(o.h, None, MASK, 2, *dims, 0, 1.0, 0.0, 0.5, 0, closed, 0.0, M.ctypes.data, None, 0, v.data_ptr() + GUARD, 400, t.data_ptr() + GUARD,
                                      g.data_ptr() + GUARD, 400, o.s), "vol_mesh_emit")
    assert all(_untouched(b) for b in (ws, v, t, g))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _same_mesh(got, want, M=None):
    assert _differ(np.asarray(got.vertices), want.vertices) == 0 and _differ(np.asarray(got.triangles), want.triangles) == 0
    wa, wv = MO.measure(want.vertices, want.triangles)
    assert got.area_mm2 == float(MO.two_level_sum(wa)) and got.volume_ml == float(MO.two_level_sum(wv)) / 1000.0


def test_extract_surface_end_to_end(tmp_path):
    import torch
    from covidseg_amd import mesh_min as MM, nifti_min, volume as V
    shape = (23, 19, 14)
    f = MO.ball_field(shape, (11.2, 9.1, 6.8), 5.0).astype(np.float32)
    aff = np.vstack([_oblique(), [0, 0, 0, 1]])
    # a scalar volume with an affine: world frame
    got = V.extract_surface(f, iso=0.0, affine=aff)
    want = MO.extract(values=f.astype(np.float64), iso=0.0, matrix=aff[:3])
    _same_mesh(got, want)
    assert got.frame == "world" and got.closed and got.euler == 2 and got.kind == "scalar" and got.groups is None and got.launches[:2] == ["vol_mesh_count", "vol_mesh_emit"]
    assert got.area_mm2 > 0 and got.volume_ml > 0                   # (the closed forms are the host tests')
    row = got.measure()
    assert len(row) == 1 and row["label"][0] == 1 and row["triangles"][0] == len(want.triangles) and row["area_mm2"][0] == got.area_mm2 and row["mesh_ml"][0] == got.volume_ml
    # a mask with a pixdim: scaled voxel frame, open and closed; the STL read back equals the mesh
    m = f > 0
    got = V.extract_surface(m, pixdim=(0.7, 0.8, 2.5))
    want = MO.extract(mask=m, matrix=MO.default_matrix((0.7, 0.8, 2.5)))
    _same_mesh(got, want)
    assert got.frame == "scaled voxel" and got.kind == "mask" and got.euler == 2
    sph, s2v = MO.shape_fields(MO.two_level_sum(MO.measure(want.vertices, want.triangles)[0]), MO.two_level_sum(MO.measure(want.vertices, want.triangles)[1]))
    assert got.measure()["sphericity"][0] == float(sph) and got.measure()["surface_to_volume"][0] == float(s2v) and 0.5 < float(sph) < 0.8          # an ellipsoid's staircase
    got.write(tmp_path / "ball.stl")
    corners, _ = MM.read_stl(tmp_path / "ball.stl")
    assert _differ(corners, got.vertices[got.triangles]) == 0
    opened = V.extract_surface(m[:, :, 7:], closed=False)
    _same_mesh(opened, MO.extract(mask=m[:, :, 7:], closed=False))
    assert opened.euler is None and not opened.closed and not MO.is_closed_manifold(opened.triangles)
    # a device tensor with shape=, kept on the device
    dev = torch.from_numpy(np.asfortranarray(m.astype(np.uint8)).reshape(-1, order="F")).cuda()
    on = V.extract_surface(dev, shape=shape, return_device=True)
    assert isinstance(on.vertices, torch.Tensor) and on.vertices.is_cuda and _differ(on.vertices.cpu().numpy(), MO.extract(mask=m).vertices) == 0
    on.write(tmp_path / "ball.ply")
    assert np.array_equal(MM.read_ply(tmp_path / "ball.ply")[1], MO.extract(mask=m).triangles)
    # a file: int16 with slope and inter, its own pixdim, no orientation; an empty surface
    raw = np.asfortranarray(np.round(f * 100).astype(np.int16))
    hdr = nifti_min.default_header(shape, (0.9, 0.9, 3.0))
    vol = nifti_min.NiftiVolume(raw, 0.01, -0.5, (0.9, 0.9, 3.0), hdr, "<")
    got = V.extract_surface(vol, iso=0.25)
    want = MO.extract(values=raw.astype(np.float64) * 0.01 + (-0.5), iso=0.25, matrix=MO.default_matrix(vol.pixdim) if vol.affine is None else vol.affine[:3])
    _same_mesh(got, want)
    none = V.extract_surface(np.zeros(shape, np.uint8))
    assert len(none.vertices) == 0 and len(none.triangles) == 0 and none.area_mm2 == 0.0 and none.euler == 0 and len(none.measure()) == 0


def test_lesion_shapes_against_the_oracle():
    from covidseg_amd import volume as V
    shape = (40, 30, 20)
    lab = np.zeros(shape, np.int32)
    lab[MO.ball_field(shape, (10.3, 10.1, 9.8), 5.0) > 0] = 1
    lab[MO.ball_field(shape, (28.6, 18.4, 9.7), 6.5) > 0] = 2
    lab[20:22, 3:5, 3:5] = 3
    lab[22, 5, 3:5] = 4                                              # touches lesion 3 along a face diagonal: they share a surface, never a triangle
    pix = (0.8, 0.8, 2.0)
    table, mesh = V.lesion_shapes(lab, 5, pixdim=pix, return_mesh=True)
    want = MO.extract(labels=lab, matrix=MO.default_matrix(pix))
    assert _differ(mesh.vertices, want.vertices) == 0 and _differ(mesh.triangles, want.triangles) == 0 and _differ(mesh.groups, want.groups) == 0
    wa, wv = MO.measure(want.vertices, want.triangles)
    ids = [1, 2, 3, 4]
    assert table["label"].tolist() == [1, 2, 3, 4, 5] and table["triangles"][:4].tolist() == [int((want.groups == i).sum()) for i in ids] and table["triangles"][4] == 0
    assert _differ(table["area_mm2"][:4], MO.group_sums(wa, want.groups, ids)) == 0 and _differ(table["mesh_ml"][:4], MO.group_sums(wv, want.groups, ids) / 1000.0) == 0
    sph, s2v = MO.shape_fields(MO.group_sums(wa, want.groups, ids), MO.group_sums(wv, want.groups, ids))
    assert _differ(table["sphericity"][:4], sph) == 0 and _differ(table["surface_to_volume"][:4], s2v) == 0
    assert np.isnan(table["sphericity"][4]) and table["area_mm2"][4] == 0 and (table["mesh_ml"][:2] > 0).all()
    vox_ml = np.array([(lab == i).sum() for i in ids]) * 0.8 * 0.8 * 2.0 / 1000.0
    assert (np.abs(table["mesh_ml"][:2] / vox_ml[:2] - 1) < 0.03).all()          # the binary ball's volume error (host tests: -1.3 % at r = 5)
    assert mesh.euler == 2 * 3                                        # three surfaces: lesions 3 and 4 share one
    with pytest.raises(ValueError):
        V.lesion_shapes(lab, 3)                                       # label 4 is outside 1..3


def test_segment_volume_fills_the_meshes(tmp_path):
    from covidseg_amd import mesh_min as MM, nifti_min, volume as V
    from covidseg_amd.keras_like import UNetModel
    from test_gpu_volume import NEW_DIM, SIZE, _patient
    paths, (ct, lung, inf) = _patient(tmp_path)
    model = UNetModel(NEW_DIM, 1, seed=1)
    model.verbose = 0
    t = float(np.median(model.predict(V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM))))
    plain = V.segment_volume(paths[0], model, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    assert plain.mesh is None and plain.lung_mesh is None and "mesh" not in plain.seconds
    out = tmp_path / "inf.stl"
    res = V.segment_volume(paths[0], model, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE, lesions=True, mesh={"what": "both", "out_path": out, "lesions": True})
    assert np.array_equal(res.mask, plain.mask) and "mesh" in res.seconds
    vol = nifti_min.read(paths[0])
    M = MO.default_matrix(vol.pixdim) if vol.affine is None else vol.affine[:3]
    labels, n = V.label_volume(res.mask, connectivity=1)
    want = MO.extract(labels=labels, matrix=M)
    assert n == res.n_lesions and _differ(res.mesh.vertices, want.vertices) == 0 and _differ(res.mesh.triangles, want.triangles) == 0 and _differ(res.mesh.groups, want.groups) == 0
    assert res.mesh.frame == ("scaled voxel" if vol.affine is None else "world") and res.mesh.closed
    wa, wv = MO.measure(want.vertices, want.triangles)
    ids = list(range(1, n + 1))
    assert len(res.mesh.lesions) == n and _differ(res.mesh.lesions["area_mm2"], MO.group_sums(wa, want.groups, ids)) == 0
    assert _differ(res.mesh.lesions["mesh_ml"], MO.group_sums(wv, want.groups, ids) / 1000.0) == 0 and np.array_equal(res.mesh.lesions["label"], res.lesions["label"])
    lw = MO.extract(mask=lung, matrix=M)
    assert _differ(res.lung_mesh.vertices, lw.vertices) == 0 and _differ(res.lung_mesh.triangles, lw.triangles) == 0 and res.lung_mesh.groups is None
    corners, _ = MM.read_stl(out)
    assert _differ(corners, want.vertices[want.triangles]) == 0
    assert _differ(MM.read_stl(tmp_path / "inf_lung.stl")[0], lw.vertices[lw.triangles]) == 0
    ens = V.segment_volume_ensemble(paths[0], [model], threshold=t, batch_size=8, img_size=SIZE, lung_mask=paths[1], mesh=True)
    assert np.array_equal(ens.mask, plain.mask) and ens.lung_mesh is None
    assert _differ(ens.mesh.vertices, MO.extract(mask=ens.mask, matrix=M).vertices) == 0 and _differ(ens.mesh.triangles, want.triangles) == 0

"""-m gpu: csrc/kernels_texture.hip and texture.py against tests/texture_oracle.py.  The device's results are integer counts: every comparison of counts is array_equal.
Every output of a direct entry-point call lies between two guard bands of a sentinel that must be untouched afterwards.  The features of texture_stats are held to the
host bound of tests/test_texture_host.py (the oracle computes it per feature), on counts that must be equal first.

The GLCM launch has three persistent workgroups per CU, so the 45 bricks of the (70, 40, 20) cases get a workgroup each; the case in which a workgroup walks
several bricks is test_glcm_many_bricks_per_workgroup (1052 bricks).

A volume with a zero dimension returns UNET_OK, its counts are zeroed (a memset, no kernel) and nothing else is touched; a UNET_E_ARG call launches nothing and leaves
every output byte as it was."""
import math

import numpy as np
import pytest

import texture_oracle as TO

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
ALL = 0x1FFF
# around the brick (32 x 8 x 8) and the wave: one voxel, a sliver, one short of a brick, exactly one, one past it in every axis, three bricks along x, odd sizes, long y
SHAPES = [(1, 1, 1), (3, 2, 1), (31, 7, 7), (32, 8, 8), (33, 9, 9), (65, 3, 2), (37, 11, 9), (7, 70, 5)]
SLOPE, INTER = 0.5, -1024.0
GUARD = 64
SENT64, SENT8 = 0x5A5A5A5A5A5A5A5A, 0xA5


def _vol(raw, scaled):
    from covidseg_amd import nifti_min
    raw = np.asfortranarray(raw)
    return nifti_min.NiftiVolume(raw, SLOPE if scaled else 0.0, INTER if scaled else 0.0, (1.0, 1.0, 1.0), nifti_min.default_header(raw.shape, (1.0, 1.0, 1.0)), "<")


def _dev(a, dtype):
    import torch
    t = torch.from_numpy(np.asfortranarray(np.asarray(a).astype(dtype)).reshape(-1, order="F")).cuda()
    return t if t.numel() else torch.zeros(16, dtype=t.dtype, device="cuda")


class Guarded:
    """n elements of an output between two guard bands"""

    def __init__(self, n, dtype):
        import torch
        self.n, self.sent = int(n), SENT64 if dtype == "int64" else SENT8
        self.full = torch.full((self.n + 2 * GUARD,), self.sent, dtype=getattr(torch, dtype), device="cuda")
        self.view = self.full[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.full.data_ptr() + GUARD * self.full.element_size()

    def get(self, what=""):
        import torch
        torch.cuda.synchronize()
        a = self.full.cpu().numpy()
        assert (a[:GUARD] == self.sent).all() and (a[GUARD + self.n:] == self.sent).all(), f"guard band written: {what}"
        return a[GUARD:GUARD + self.n].copy()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.full == self.sent).all().item())


def _api():
    import torch
    from covidseg_amd import _lib
    return _lib.load(), _lib.Context.get(torch.cuda.current_device()), torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def dev_quantize(vol, ld, md, n, rd, lo, width, Ng, outside, what=""):
    """-> (levels uint8 [X, Y, Z], level_counts [n, Ng], the guarded device level buffer)"""
    from covidseg_amd import volume as V
    lib, ctx, s = _api()
    shape = tuple(int(v) for v in vol.raw.shape)
    N = int(np.prod(shape))
    lv, lc = Guarded(N, "uint8"), Guarded(n * Ng, "int64")
    dev = V.upload(vol)
    dev = dev if dev.numel() else _dev(np.zeros(16), np.uint8)
    ctx.check(lib.unet_vol_texture_quantize(ctx.handle, dev.data_ptr(), *V._vox_args(vol), _ptr(ld), _ptr(md), n, _ptr(rd), lo, width, Ng, outside, lv.ptr, lc.ptr, s), what)
    return lv.get(what).reshape(shape, order="F"), lc.get(what).reshape(n, Ng), lv


def dev_glcm(levels_dev, ld, n, shape, Ng, distance, bits, merge=False, what=""):
    lib, ctx, s = _api()
    K = 1 if merge else bin(bits).count("1")
    out = Guarded(n * K * Ng * Ng, "int64")
    ctx.check(lib.unet_vol_texture_glcm(ctx.handle, levels_dev.data_ptr(), _ptr(ld), n, *shape, Ng, distance, bits, 1 if merge else 0, out.ptr, s), what)
    return out.get(what).reshape(n, K, Ng, Ng)


def dev_runs(levels_dev, ld, n, shape, Ng, bits, max_run, what=""):
    lib, ctx, s = _api()
    K = bin(bits).count("1")
    out, cl = Guarded(n * K * Ng * max_run, "int64"), Guarded(n * K, "int64")
    ctx.check(lib.unet_vol_texture_runs(ctx.handle, levels_dev.data_ptr(), _ptr(ld), n, *shape, Ng, bits, max_run, out.ptr, cl.ptr, s), what)
    return out.get(what).reshape(n, K, Ng, max_run), cl.get(what).reshape(n, K)


def _raw(shape, kind, rng):
    """voxels of one NIfTI dtype over a narrow range (many voxels share a value and sit on a bin edge); the float kinds carry NaN, both infinities and both zeros"""
    dt = np.dtype(kind)
    N = int(np.prod(shape))
    if dt.kind == "f":
        a = (rng.normal(0.0, 40.0, N).round() * 0.5).astype(dt)
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, np.nan)):
            if N > 3 * k + 2:
                a[3 * k + 1] = v
    else:
        lo, hi = (0, 120) if kind == "u1" else (-60, 60) if kind == "i1" else (0, 300) if dt.kind == "u" else (-150, 150)
        a = rng.integers(lo, hi, N).astype(dt)
    return a.reshape(shape, order="F")


def _layouts(shape, rng):
    """(name, labels, mask, n, region) over one shape: test_gpu_intensity.py's"""
    N = int(np.prod(shape))
    f = np.arange(N).reshape(shape, order="F")
    region = (rng.random(shape) < 0.6).astype(np.uint8) * 3
    sparse = rng.integers(-2, 10, shape)
    sparse[sparse == 3] = 0                                         # label 3 has no voxel; -2, -1, 0 and 7..9 lie outside 1..6
    yield "one group over everything", None, np.full(shape, 2, np.uint8), 1, None
    yield "64 groups share a wave", (f % 64 + 1), None, 64, None
    yield "64 groups share a wave, region", (f % 64 + 1), None, 64, region
    yield "missing and outside labels", sparse, None, 6, None
    yield "missing and outside labels, region", sparse, None, 6, region
    yield "n = 0", sparse, None, 0, None
    yield "mask", None, (rng.random(shape) < 0.3).astype(np.uint8) * 7, 1, None
    yield "mask, region", None, (rng.random(shape) < 0.5).astype(np.uint8), 1, region
    yield "nothing takes part", None, np.zeros(shape, np.uint8), 1, None


def _levels_case(shape, Ng, rng, blobs=True):
    """a level volume with spatial structure (runs and co-occurrences of every kind): smooth blobs plus noise, about a tenth of the voxels at level 0"""
    x, y, z = np.indices(shape)
    lev = ((x // 3 + y // 2 + z) % Ng + 1) if blobs else rng.integers(1, Ng + 1, shape)
    lev = np.where(rng.random(shape) < 0.3, rng.integers(1, Ng + 1, shape), lev)
    return np.where(rng.random(shape) < 0.1, 0, lev).astype(np.uint8)


# ---- quantize ----------------------------------------------------------------------------------------------------------------------------------------------
QUANT = [(Ng, outside) for Ng in (1, 2, 32, 64) for outside in (0, 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_quantize_equals_the_oracle(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    turn = 0
    for kind in TO.DTYPES.values():
        raw = _raw(shape, kind, rng)
        for scaled in (False, True):
            vol = _vol(raw, scaled)
            fdata = TO.decode(raw, scaled, SLOPE, INTER)
            assert np.array_equal(vol.get_fdata(), fdata, equal_nan=True)
            fin = np.unique(fdata[np.isfinite(fdata)])
            lo = float(fin[len(fin) // 4])                          # a value that occurs: with widths of 0.5 and 2 the bin edges fall on values of the volume
            for name, labels, mask, n, region in _layouts(shape, rng):
                Ng, outside = QUANT[turn % len(QUANT)]
                width = (0.5, 2.0, 7.0)[turn % 3]
                turn += 1
                what = (shape, kind, scaled, name, Ng, outside, width)
                g = TO.group_of(shape, labels=labels, mask=mask, n=n, region=region)
                want_lv, want_lc = TO.quantize(fdata, g, n, lo, width, Ng, outside)
                ld, md = (_dev(labels, np.int32) if labels is not None else None), (_dev(mask, np.uint8) if mask is not None else None)
                rd = _dev(region, np.uint8) if region is not None else None
                got_lv, got_lc, _ = dev_quantize(vol, ld, md, n, rd, lo, width, Ng, outside, str(what))
                assert np.array_equal(got_lv, want_lv), what
                assert np.array_equal(got_lc, want_lc), what
    assert turn >= 8 * 2 * 9 and turn % len(QUANT) == 0              # every (Ng, mode) pair met every layout


@pytest.mark.parametrize("kind", ["f4", "f8"])
def test_quantize_bin_edges_infinities_zeros_and_nan(kind):
    vals = np.array([-np.inf, -1000.5, -1000.0, -975.5, -975.0, -0.0, 0.0, 574.5, 575.0, 600.0, np.inf, np.nan])          # all exact in float32
    vol = _vol(vals.astype(kind).reshape(12, 1, 1), False)
    md = _dev(np.ones(12), np.uint8)
    lv, lc, _ = dev_quantize(vol, None, md, 1, None, -1000.0, 25.0, 63, 0)
    assert lv.ravel().tolist() == [1, 1, 1, 1, 2, 41, 41, 63, 63, 63, 63, 0] and lc.sum() == 11 and lc[0, 62] == 4
    lv, lc, _ = dev_quantize(vol, None, md, 1, None, -1000.0, 25.0, 63, 1)
    assert lv.ravel().tolist() == [0, 0, 1, 1, 2, 41, 41, 63, 0, 0, 0, 0] and lc.sum() == 6
    vol = _vol(np.array([-0.0, 0.0, -1e-30], kind).reshape(3, 1, 1), False)          # the drop test is on q: q = -0.0 is not below 0
    lv, _, _ = dev_quantize(vol, None, _dev(np.ones(3), np.uint8), 1, None, 0.0, 1.0, 4, 1)
    assert lv.ravel().tolist() == [1, 1, 0]


def test_quantize_more_groups_than_its_lds_table_holds():
    shape, n = (64, 16, 3), 700                                     # n Ng = 700 * 8 > 4096
    rng = np.random.default_rng(700)
    labels = np.arange(int(np.prod(shape))).reshape(shape, order="F") % (n + 5) + 1
    raw = _raw(shape, "i2", rng)
    fdata = TO.decode(raw, True, SLOPE, INTER)
    g = TO.group_of(shape, labels=labels, n=n)
    for Ng in (5, 8):                                               # 3500 <= 4096 < 5600
        want = TO.quantize(fdata, g, n, -1090.0, 9.0, Ng, 0)
        got_lv, got_lc, _ = dev_quantize(_vol(raw, True), _dev(labels, np.int32), None, n, None, -1090.0, 9.0, Ng, 0)
        assert np.array_equal(got_lv, want[0]) and np.array_equal(got_lc, want[1])


# ---- GLCM ----------------------------------------------------------------------------------------------------------------------------------------------------
def _check_glcm(lev, lev_dev, labels, mask, n, region, Ng, distance, bits, merge, what):
    shape = lev.shape
    g = TO.group_of(shape, labels=labels, mask=mask, n=n, region=None)          # the counting kernels see levels and labels; the region acted in quantize
    ld = _dev(labels, np.int32) if labels is not None else None
    want = TO.glcm(lev, g, n, Ng, distance, bits, merge)
    got = dev_glcm(lev_dev, ld, n, shape, Ng, distance, bits, merge, str(what))
    assert got.shape == want.shape and np.array_equal(got, want), what
    return got


@pytest.mark.parametrize("shape", SHAPES + [(70, 40, 20)])
def test_glcm_equals_the_oracle(shape):
    """every layout, distances 1 to 4 (at and above a dimension: that direction counts nothing), unmerged and merged; Ng = 8 puts the 64-group layouts beyond the LDS table
    (64 * 13 * 64 counters) and the others inside it"""
    rng = np.random.default_rng(shape[0] * 100 + shape[2])
    Ng, big = 8, int(np.prod(shape)) > 10000
    for li, (name, labels, mask, n, region) in enumerate(_layouts(shape, rng)):
        if big and li not in (0, 2, 4, 7):                          # the large volume: one group, 64 groups, sparse labels and a mask, the last three under a region
            continue
        lev = _levels_case(shape, Ng, rng)
        take = TO.group_of(shape, labels=labels, mask=mask, n=n, region=region) > 0
        lev = np.where(take, lev, 0).astype(np.uint8)               # what quantize would have written
        lev_dev = _dev(lev, np.uint8)
        for distance in ((1, 3) if big else (1, 2, 3, 4)):
            got = _check_glcm(lev, lev_dev, labels, mask, n, region, Ng, distance, ALL, False, (shape, name, distance))
            for k, d in enumerate(TO.DIRECTIONS):
                if any(abs(o) * distance >= dim for o, dim in zip(d, shape)):
                    assert not got[:, k].any(), (shape, name, distance, d)
            _check_glcm(lev, lev_dev, labels, mask, n, region, Ng, distance, ALL, True, (shape, name, distance, "merged"))


def test_glcm_direction_sets():
    from covidseg_amd import texture as T
    shape, Ng, n = (37, 11, 9), 6, 5
    rng = np.random.default_rng(37)
    lev = _levels_case(shape, Ng, rng, blobs=False)
    labels = rng.integers(0, n + 1, shape)
    lev = np.where(labels > 0, lev, 0).astype(np.uint8)
    lev_dev = _dev(lev, np.uint8)
    full = _check_glcm(lev, lev_dev, labels, None, n, None, Ng, 1, ALL, False, "3d")
    for k in range(13):                                             # every single direction alone is its slice of the full launch
        one = _check_glcm(lev, lev_dev, labels, None, n, None, Ng, 1, 1 << k, False, ("single", k))
        assert np.array_equal(one[:, 0], full[:, k])
        assert np.array_equal(_check_glcm(lev, lev_dev, labels, None, n, None, Ng, 1, 1 << k, True, ("single merged", k)), one)
    for sel in (T.DIRECTIONS_2D, (2, 5, 6, 12), (0, 12), tuple(range(1, 13))):
        bits = T.direction_bits(sel)
        got = _check_glcm(lev, lev_dev, labels, None, n, None, Ng, 2, bits, False, sel)
        assert got.shape[1] == len(sel)
        merged = _check_glcm(lev, lev_dev, labels, None, n, None, Ng, 2, bits, True, (sel, "merged"))
        assert np.array_equal(merged[:, 0], got.sum(axis=1))
    again = dev_glcm(lev_dev, _dev(labels, np.int32), n, shape, Ng, 1, ALL)          # a repeated launch: identical bits
    assert np.array_equal(again, full)


@pytest.mark.parametrize("Ng,bits,merge", [(8, 1 << 9, False), (8, ALL, True), (4, 0b11011, False)])
def test_glcm_table_sizes_around_the_lds_limit(Ng, bits, merge):
    """n K Ng^2 just below, exactly at and just above TEXTURE_LDS_COUNTERS: the same data counted by the LDS-table kernel and by the global-atomic kernel"""
    from covidseg_amd import _lib
    K = 1 if merge else bin(bits).count("1")
    n_at = _lib.TEXTURE_LDS_COUNTERS // (K * Ng * Ng)
    assert n_at * K * Ng * Ng == _lib.TEXTURE_LDS_COUNTERS
    shape = (70, 40, 20)                                            # 3 x 5 x 3 bricks, partial ones on every axis
    rng = np.random.default_rng(Ng)
    lev = _levels_case(shape, Ng, rng)
    x, y, z = np.indices(shape)
    labels = (x // 4 + 18 * (y // 4 + 10 * (z // 4))) % (n_at + 1) + 1          # groups 1 .. n_at + 1 in blocks of 4 x 4 x 4: in-group pairs along every direction
    lev_dev = _dev(lev, np.uint8)
    got = {n: _check_glcm(lev, lev_dev, labels, None, n, None, Ng, 1, bits, merge, ("table", n)) for n in (n_at - 1, n_at, n_at + 1)}
    assert got[n_at].any() and np.array_equal(got[n_at + 1][:n_at], got[n_at]) and np.array_equal(got[n_at][:n_at - 1], got[n_at - 1])


def test_glcm_many_bricks_per_workgroup():
    """1052 bricks for the 768 persistent workgroups of 256 CUs: some walk two, and a slab of bricks in which nothing takes part is left early"""
    shape, Ng, n = (34, 9, 2100), 4, 3
    rng = np.random.default_rng(64)
    lev = _levels_case(shape, Ng, rng)
    lev[:, :, 800:1000] = 0
    labels = rng.integers(0, n + 1, (3, 2, 210)).repeat(12, axis=0).repeat(5, axis=1).repeat(10, axis=2)[:34, :9]
    lev = np.where(labels > 0, lev, 0).astype(np.uint8)
    lev_dev = _dev(lev, np.uint8)
    _check_glcm(lev, lev_dev, labels, None, n, None, Ng, 3, ALL, False, "two bricks per workgroup, LDS table")
    many = np.where(labels > 0, labels + 3 * ((np.indices(shape)[2] // 4) % 32), 0)          # 96 groups: 99 * 13 * 16 counters
    _check_glcm(lev, lev_dev, many, None, 99, None, Ng, 2, ALL, False, "two bricks per workgroup, global atomics")


def test_levels_above_ng_and_labels_outside_take_no_part():
    shape, Ng, n = (33, 9, 9), 8, 4
    rng = np.random.default_rng(5)
    lev = np.where(rng.random(shape) < 0.5, rng.integers(1, Ng + 1, shape), rng.integers(0, 256, shape)).astype(np.uint8)          # half of the levels: mostly above Ng
    labels = np.where(rng.random(shape) < 0.7, rng.integers(1, n + 1, shape), rng.integers(-2 ** 31, 2 ** 31 - 1, shape))
    lev_dev, ld = _dev(lev, np.uint8), _dev(labels, np.int32)
    g = TO.group_of(shape, labels=labels, n=n)
    for merge in (False, True):
        assert np.array_equal(dev_glcm(lev_dev, ld, n, shape, Ng, 2, ALL, merge), TO.glcm(lev, g, n, Ng, 2, ALL, merge))
    got, cl = dev_runs(lev_dev, ld, n, shape, Ng, ALL, 5)
    want, wcl = TO.runs(lev, g, n, Ng, ALL, 5)
    assert np.array_equal(got, want) and np.array_equal(cl, wcl)


# ---- runs ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(70, 40, 20)])
def test_runs_equal_the_oracle(shape):
    rng = np.random.default_rng(shape[1] * 100 + shape[2])
    Ng, big = 3, int(np.prod(shape)) > 10000
    for li, (name, labels, mask, n, region) in enumerate(_layouts(shape, rng)):
        if big and li not in (0, 2, 4):
            continue
        lev = _levels_case(shape, Ng, rng)
        take = TO.group_of(shape, labels=labels, mask=mask, n=n, region=region) > 0
        lev = np.where(take, lev, 0).astype(np.uint8)
        g = TO.group_of(shape, labels=labels, mask=mask, n=n)
        lev_dev, ld = _dev(lev, np.uint8), (_dev(labels, np.int32) if labels is not None else None)
        for bits, max_run in ((ALL, max(shape)), (ALL, 2), (0b11011, 3)):
            want, wcl = TO.runs(lev, g, n, Ng, bits, max_run)
            got, cl = dev_runs(lev_dev, ld, n, shape, Ng, bits, max_run, str((shape, name, bits, max_run)))
            assert np.array_equal(got, want) and np.array_equal(cl, wcl), (shape, name, bits, max_run)
            if max_run == max(shape):
                assert not cl.any()


def test_runs_spanning_the_whole_extent_and_clamped_columns():
    from covidseg_amd import texture as T
    shape, Ng = (70, 40, 20), 4                                     # a constant volume: every run spans the volume along its direction and crosses every brick seam
    lev = np.full(shape, 3, np.uint8)
    g = np.ones(shape, np.int64)
    lev_dev = _dev(lev, np.uint8)
    got, cl = dev_runs(lev_dev, None, 1, shape, Ng, ALL, 70)
    want, wcl = TO.runs(lev, g, 1, Ng, ALL, 70)
    assert np.array_equal(got, want) and not cl.any()
    assert got[0, 0, 2, 69] == 40 * 20 and got[0, 1, 2, 39] == 70 * 20 and got[0, 2, 2, 19] == 70 * 40 and got[0, 3, 2, 39] == 31 * 20          # x, y, z, and the full (1, 1, 0) diagonals
    assert ((got[0] * np.arange(1, 71)).sum(axis=(1, 2)) == 70 * 40 * 20).all()
    short, cl = dev_runs(lev_dev, None, 1, shape, Ng, ALL, 16)      # max_run below the longest run: the last column and clamped are exact
    want, wcl = TO.runs(lev, g, 1, Ng, ALL, 16)
    assert np.array_equal(short, want) and np.array_equal(cl, wcl) and cl[0, 0] == 40 * 20 and short[0, 0, 2, 15] == 40 * 20
    ct = np.full(shape, -940, np.int16)                              # the wrapper doubles max_run until nothing is clamped: 16 -> 32 -> 64 -> 70
    counts, clamped = T.run_lengths(ct, mask=np.ones(shape, np.uint8), levels=Ng, width=25.0, max_run=16, return_clamped=True)
    assert counts.shape == (1, 13, Ng, 70) and not clamped.any() and np.array_equal(counts, got)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------
def _assert_rows(groups, prefix, per_group, names, what):
    for gi, want in enumerate(per_group):
        for f in names:
            w, bound = want[f]
            v = float(groups[gi][prefix + f])
            if math.isnan(w):
                assert math.isnan(v), (what, gi, f)
            else:
                assert abs(v - w) <= bound, (what, gi, f, v, w, bound)


def test_texture_stats_and_lesion_texture():
    from covidseg_amd import texture as T, volume as V
    import covidseg_amd
    shape, n, Ng = (37, 11, 9), 5, 8
    rng = np.random.default_rng(11)
    x, y, z = np.indices(shape)
    raw = (-900 + 60 * ((x // 2 + y + z) % 7) + rng.integers(-40, 40, shape)).astype(np.int16)
    labels = rng.integers(0, n, (13, 4, 3)).repeat(3, axis=0).repeat(3, axis=1).repeat(3, axis=2)[:37, :11, :9]          # label 5 has no voxel: a NaN row
    fdata = raw.astype(np.float64)
    g = TO.group_of(shape, labels=labels, n=n)
    lev, lc = TO.quantize(fdata, g, n, -1000.0, 75.0, Ng, False)
    C, (R, _) = TO.glcm(lev, g, n, Ng, 1, ALL), TO.runs(lev, g, n, Ng, ALL, 64)
    ts = covidseg_amd.lesion_texture(raw, labels, n, width=75.0, levels=Ng)
    assert np.array_equal(ts.level_counts, lc) and np.array_equal(ts.glcm, C) and np.array_equal(ts.runs, R[..., :ts.runs.shape[-1]]) and not R[..., ts.runs.shape[-1]:].any()
    assert ts.groups["label"].tolist() == [1, 2, 3, 4, 5] and np.array_equal(ts.groups["voxels"], lc.sum(axis=1)) and ts.groups["voxels"][4] == 0
    table = V.component_table(labels.astype(np.int32), n)           # the rows line up with component_table's
    assert np.array_equal(table["label"][:4], ts.groups["label"][:4]) and np.array_equal(table["voxels"][:4], ts.groups["voxels"][:4])
    vox = lc.sum(axis=1)
    _assert_rows(ts.groups, "glcm_", [TO.mean_over_directions([TO.glcm_features_exact(C[gi, k]) for k in range(13)], T.GLCM_FEATURES) for gi in range(n)], T.GLCM_FEATURES, "lesions")
    _assert_rows(ts.groups, "glrlm_", [TO.mean_over_directions([TO.run_features_exact(R[gi, k], int(vox[gi])) for k in range(13)], T.RUN_FEATURES) for gi in range(n)],
                 T.RUN_FEATURES, "lesions")
    assert np.isnan(ts.groups["glcm_contrast"][4]) and np.isnan(ts.groups["glrlm_run_entropy"][4]) and not np.isnan(ts.groups["glcm_contrast"][:4]).any()
    # one mask under a region, in-plane directions, merged, distance 2, values dropped outside the bins, device inputs
    mask, region = (labels > 0).astype(np.uint8), (rng.random(shape) < 0.8).astype(np.uint8)
    g = TO.group_of(shape, mask=mask, n=1, region=region)
    lev, lc = TO.quantize(fdata, g, 1, -880.0, 50.0, Ng, True)
    bits = T.direction_bits(T.DIRECTIONS_2D)
    C, (R, _) = TO.glcm(lev, g, 1, Ng, 2, bits, merge=True), TO.runs(lev, g, 1, Ng, bits, 64)
    ts = T.texture_stats(raw, mask=_dev(mask, np.uint8), region=_dev(region, np.uint8), shape=shape, lo=-880.0, width=50.0, levels=Ng, outside="drop", distance=2,
                         directions="2d", merge=True)
    assert np.array_equal(ts.level_counts, lc) and np.array_equal(ts.glcm, C) and np.array_equal(ts.runs, R[..., :ts.runs.shape[-1]]) and ts.directions == (0, 1, 3, 4)
    _assert_rows(ts.groups, "glcm_", [TO.mean_over_directions([TO.glcm_features_exact(C[0, 0])], T.GLCM_FEATURES)], T.GLCM_FEATURES, "mask")
    _assert_rows(ts.groups, "glrlm_", [TO.mean_over_directions([TO.run_features_exact(R[0, k], int(lc.sum())) for k in range(4)], T.RUN_FEATURES)], T.RUN_FEATURES, "mask")
    lv, hist = T.quantize_volume(raw, mask=mask, region=region, lo=-880.0, width=50.0, levels=Ng, outside="drop")
    assert lv.shape == shape and lv.dtype == np.uint8 and np.array_equal(lv, lev) and np.array_equal(hist, lc)
    assert np.array_equal(T.glcm(raw, mask=mask, region=region, lo=-880.0, width=50.0, levels=Ng, outside="drop", distance=2, directions="2d", merge=True), C)


# ---- nothing to do, and refusals ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(0, 5, 5), (4, 0, 3), (6, 2, 0)])
def test_a_zero_dimension_counts_nothing(shape):
    from covidseg_amd import volume as V
    lib, ctx, s = _api()
    vol = _vol(np.zeros(shape, np.int16), False)
    buf = _dev(np.zeros(16), np.uint8)
    lv, lc = Guarded(32, "uint8"), Guarded(3 * 8, "int64")
    ctx.check(lib.unet_vol_texture_quantize(ctx.handle, buf.data_ptr(), *V._vox_args(vol), None, buf.data_ptr(), 3, None, 0.0, 1.0, 8, 0, lv.ptr, lc.ptr, s))
    assert not lc.get().any() and lv.untouched()
    out = Guarded(3 * 13 * 64, "int64")
    ctx.check(lib.unet_vol_texture_glcm(ctx.handle, buf.data_ptr(), None, 3, *shape, 8, 1, ALL, 0, out.ptr, s))
    assert not out.get().any()
    out, cl = Guarded(3 * 13 * 8 * 4, "int64"), Guarded(3 * 13, "int64")
    ctx.check(lib.unet_vol_texture_runs(ctx.handle, buf.data_ptr(), None, 3, *shape, 8, ALL, 4, out.ptr, cl.ptr, s))
    assert not out.get().any() and not cl.get().any()


def test_refused_arguments_launch_nothing():
    from covidseg_amd import volume as V
    lib, ctx, s = _api()
    shape = (5, 4, 3)
    vol = _vol(np.zeros(shape, np.int16), False)
    vox, lab, msk = _dev(np.zeros(shape), np.int16), _dev(np.ones(shape), np.int32), _dev(np.ones(shape), np.uint8)
    lv, lc = Guarded(60, "uint8"), Guarded(2 * 8, "int64")
    good = dict(dtype=4, X=5, Y=4, Z=3, labels=lab.data_ptr(), mask=None, n=2, lo=0.0, width=1.0, Ng=8, outside=0)

    def quantize(**kw):
        a = {**good, **kw}
        return lib.unet_vol_texture_quantize(ctx.handle, vox.data_ptr(), a["dtype"], a["X"], a["Y"], a["Z"], 0, 1.0, 0.0, a["labels"], a["mask"], a["n"], None, a["lo"], a["width"],
                                             a["Ng"], a["outside"], lv.ptr, lc.ptr, s)

    for kw in (dict(Ng=0), dict(Ng=65), dict(width=0.0), dict(width=-2.0), dict(width=float("inf")), dict(width=float("nan")), dict(lo=float("nan")), dict(lo=float("-inf")),
               dict(mask=msk.data_ptr()), dict(labels=None), dict(n=-1), dict(dtype=3), dict(outside=2), dict(X=-1), dict(X=2 ** 16, Y=2 ** 15, Z=1)):
        assert quantize(**kw) == E_ARG, kw
        assert ctx.last_error().startswith("vol_texture_quantize"), kw
    assert lv.untouched() and lc.untouched()
    lev = _dev(np.ones(shape), np.uint8)
    out = Guarded(2 * 13 * 64, "int64")
    for n, dims, Ng, distance, bits in ((2, shape, 8, 0, ALL), (2, shape, 8, 5, ALL), (2, shape, 8, 1, 0), (2, shape, 8, 1, 1 << 13), (2, shape, 8, 1, -1), (2, shape, 0, 1, ALL),
                                        (2, shape, 65, 1, ALL), (-1, shape, 8, 1, ALL), (2, (5, -4, 3), 8, 1, ALL), (2, (2 ** 11, 2 ** 10, 2 ** 10), 8, 1, ALL)):
        assert lib.unet_vol_texture_glcm(ctx.handle, lev.data_ptr(), lab.data_ptr(), n, *dims, Ng, distance, bits, 0, out.ptr, s) == E_ARG, (n, dims, Ng, distance, bits)
    assert out.untouched()
    cl = Guarded(2 * 13, "int64")
    for n, dims, Ng, bits, max_run in ((2, shape, 8, ALL, 0), (2, shape, 8, ALL, 2 ** 15 + 1), (2, shape, 8, 0, 4), (2, shape, 8, 1 << 13, 4), (2, shape, 65, ALL, 4),
                                       (-1, shape, 8, ALL, 4), (2, (5, 4, -3), 8, ALL, 4)):
        assert lib.unet_vol_texture_runs(ctx.handle, lev.data_ptr(), lab.data_ptr(), n, *dims, Ng, bits, max_run, out.ptr, cl.ptr, s) == E_ARG, (n, dims, Ng, bits, max_run)
    assert out.untouched() and cl.untouched()
    got, _ = dev_runs(lev, lab, 2, shape, 8, 1, 2 ** 15)            # the largest max_run is taken: 5 x 4 x 3 of level 1 in group 1 -> 12 runs of 5 along x
    assert got[0, 0, 0, 4] == 12 and got.sum() == 12

"""-m gpu: csrc/kernels_intensity.hip and volume.intensity_stats / segment_volume(density=) against tests/intensity_oracle.py.  Integer counts, exact min / max, values
that are copied, and sums whose order and tree are stated: every comparison is array_equal."""
import numpy as np
import pytest

import intensity_oracle as IO
import volume_oracle as VO

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
SHAPES = [(1, 1, 1), (63, 5, 3), (65, 3, 2), (128, 2, 2), (7, 70, 5), (130, 9, 4)]          # x short of a wave, exactly on it (128 = two), one past it, two waves + 2
SLOPE, INTER = 0.5, -1024.0                                         # stored even values land on whole numbers: on the edges below


def _vol(raw, scaled, pixdim=(1.0, 1.0, 1.0)):
    from covidseg_amd import nifti_min
    raw = np.asfortranarray(raw)
    return nifti_min.NiftiVolume(raw, SLOPE if scaled else 0.0, INTER if scaled else 0.0, pixdim, nifti_min.default_header(raw.shape, pixdim), "<")


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.asfortranarray(np.asarray(a).astype(dtype)).reshape(-1, order="F")).cuda()


def _raw(shape, kind, rng):
    """voxels of one NIfTI dtype over a narrow range (many voxels share a value and sit on an edge); the float kinds carry NaN, both infinities and both zeros"""
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


def _edges(fdata):
    """four ascending edges: three values that occur in the volume (as many as it has) and one that does not"""
    u = np.unique(fdata[np.isfinite(fdata)])
    picks = sorted({float(u[0]), float(u[len(u) // 2]), float(u[-1]), 0.0})
    picks.append(picks[-1] + 0.25)
    return np.array(sorted(set(picks)), np.float64)


def _layouts(shape, rng):
    """(name, labels, mask, n, region) over one shape"""
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
    yield "n = 1", sparse, None, 1, region
    yield "mask", None, (rng.random(shape) < 0.3).astype(np.uint8) * 7, 1, None
    yield "mask, region", None, (rng.random(shape) < 0.5).astype(np.uint8), 1, region
    yield "nothing takes part", None, np.zeros(shape, np.uint8), 1, None


def _check_bands(vol, fdata, labels, mask, n, region, edges, what):
    from covidseg_amd import volume as V
    dev = V.upload(vol)
    ld = _dev(labels, np.int32) if labels is not None else None
    md = _dev(mask, np.uint8) if mask is not None else None
    rd = _dev(region, np.uint8) if region is not None else None
    g = IO.group_of(fdata.shape, labels=labels, mask=mask, n=n, region=region)
    want = IO.bands(fdata, g, n, edges)
    got = V.intensity_bands_device(vol, dev, ld, md, n, rd, edges)
    for name, a, b in zip(("band_counts", "slice_counts", "minmax"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (what, name)
    bc, sc, mm = V.intensity_bands_device(vol, dev, ld, md, n, rd, edges, per_slice=False, minmax=False)          # the optional outputs left out
    assert sc is None and mm is None and np.array_equal(bc, want[0]), what
    return dev, ld, md, rd, g


# ---- bands, min / max, slice counts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_bands_minmax_and_slice_counts_equal_the_oracle(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for kind in IO.DTYPES.values():
        raw = _raw(shape, kind, rng)
        for scaled in (False, True):
            vol = _vol(raw, scaled)
            fdata = vol.get_fdata()
            assert np.array_equal(fdata, IO.decode(raw, scaled, SLOPE, INTER), equal_nan=True)
            edges = _edges(fdata)
            for name, labels, mask, n, region in _layouts(shape, rng):
                _check_bands(vol, fdata, labels, mask, n, region, edges, (shape, kind, scaled, name))


def test_values_on_the_default_edges_go_to_the_band_above():
    """int16 with slope 0.5, inter -1024: the stored values 148, 548, 1448, 2148 decode to -950, -750, -300, 50 exactly"""
    from covidseg_amd import volume as V
    raw = np.array([146, 148, 150, 546, 548, 1446, 1448, 2146, 2148, 2150, -32768, 32767], np.int16).reshape(12, 1, 1)
    vol = _vol(raw, True)
    bc, sc, mm = V.intensity_bands_device(vol, V.upload(vol), None, _dev(np.ones((12, 1, 1)), np.uint8), 1, None, np.array(IO.HU_EDGES))
    assert bc.tolist() == [[2, 3, 2, 2, 3, 0]] and sc.tolist() == bc.tolist() and mm.tolist() == [[-32768 * 0.5 - 1024, 32767 * 0.5 - 1024]]


def test_more_groups_than_an_lds_table_holds():
    shape, n = (64, 64, 2), 3000
    rng = np.random.default_rng(3000)
    labels = np.arange(64 * 64 * 2).reshape(shape, order="F") % n + 1
    for kind, scaled in (("i2", True), ("f4", False)):
        vol = _vol(_raw(shape, kind, rng), scaled)
        fdata = vol.get_fdata()
        for region in (None, (rng.random(shape) < 0.5).astype(np.uint8)):
            _check_bands(vol, fdata, labels, None, n, region, _edges(fdata), (kind, "n = 3000", region is not None))
    vol = _vol(_raw(shape, "i2", rng), True)                          # 63 edges: the widest table row; n (B + 1) passes the LDS table from n = 64 on
    fdata = vol.get_fdata()
    edges = np.arange(63) * 2.0 - 1090.0
    for n_groups in (63, 64, 1024, 1025):
        _check_bands(vol, fdata, labels, None, n_groups, None, edges, ("63 edges", n_groups))
    for n_groups in (1024, 1025):                                    # one edge: the table has room, the min / max keys decide
        _check_bands(vol, fdata, labels, None, n_groups, None, np.array([-1000.0]), ("1 edge", n_groups))


# ---- gather ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(65, 3, 2), (130, 9, 4)])
def test_gather_returns_the_taking_part_values(shape):
    import torch
    from covidseg_amd import volume as V
    rng = np.random.default_rng(shape[0])
    for kind, scaled in (("i2", True), ("f8", False), ("u1", False)):
        vol = _vol(_raw(shape, kind, rng), scaled)
        fdata = vol.get_fdata()
        for name, labels, mask, n, region in _layouts(shape, rng):
            dev, ld, md, rd, g = _check_bands(vol, fdata, labels, mask, n, region, _edges(fdata), (shape, kind, name))
            wv, wg, off = IO.ordered(fdata, g, n)
            count, vals, grps = V.intensity_gather_device(vol, dev, ld, md, n, rd, len(wv))
            assert count == len(wv) == vals.numel() == grps.numel(), name
            v, k = vals.cpu().numpy(), grps.cpu().numpy()
            order = np.lexsort((v, k))
            assert np.array_equal(v[order], wv) and np.array_equal(k[order], wg), name
            sv, gv = V.sort_by_group_value(vals, grps)               # the device's own ordering
            assert np.array_equal(gv.cpu().numpy(), wv) and np.array_equal(sv.cpu().numpy(), np.sort(wv)), name
            if count < 4:
                continue
            cap = count // 2                                         # a short buffer: the count is still the true one and nothing is written past the capacity
            vb = torch.full((count + 8,), -777.25, dtype=torch.float64, device="cuda"); gb = torch.full((count + 8,), -7, dtype=torch.int32, device="cuda")
            c2, v2, g2 = V.intensity_gather_device(vol, dev, ld, md, n, rd, cap, values=vb, groups=gb)
            assert c2 == count and v2.numel() == cap == g2.numel(), name
            assert (vb[cap:].cpu().numpy() == -777.25).all() and (gb[cap:].cpu().numpy() == -7).all(), name
            pairs = set(zip(wg.tolist(), (wv + 0.0).view(np.uint64).tolist()))          # (+ 0.0: -0.0 and 0.0 are one value here)
            assert set(zip(g2.cpu().numpy().tolist(), (v2.cpu().numpy() + 0.0).view(np.uint64).tolist())) <= pairs, name
            c3, v3, g3 = V.intensity_gather_device(vol, dev, ld, md, n, rd, 0, want_groups=False)
            assert c3 == count and v3.numel() == 0 and g3 is None


# ---- moments ---------------------------------------------------------------------------------------------------------------------------------------------
def test_moments_of_runs_around_the_chunk_size_equal_the_oracle_bit_for_bit():
    from covidseg_amd import volume as V
    shape = (100, 100, 7)
    rng = np.random.default_rng(7)
    raw = rng.normal(-420.0, 310.0, shape)
    sizes = (1, 255, 256, 257, 65537, 0, 300)                        # group 6 has no voxel
    labels = np.zeros(int(np.prod(shape)), np.int32)
    perm = rng.permutation(labels.size)
    at = 0
    for k, m in enumerate(sizes):
        labels[perm[at:at + m]] = k + 1
        at += m
    labels = labels.reshape(shape, order="F")
    vol = _vol(raw, False)
    dev, ld = V.upload(vol), _dev(labels, np.int32)
    n = len(sizes)
    wv, wg, off = IO.ordered(raw, IO.group_of(shape, labels=labels, n=n), n)
    assert np.diff(off).tolist() == list(sizes)
    count, vals, grps = V.intensity_gather_device(vol, dev, ld, None, n, None, int(off[-1]))
    sv, gv = V.sort_by_group_value(vals, grps)
    assert np.array_equal(gv.cpu().numpy(), wv)
    want = IO.moments(wv, off)
    got = V.group_moments_device(gv, off, n)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert got[5].tolist() == [0.0, 0.0] and got[0, 0] == wv[0] and got[0, 1] == 0.0
    assert np.array_equal(V.group_moments_device(gv, off, n).view(np.uint64), got.view(np.uint64))          # a second run: the same bits
    union = V.group_moments_device(sv, np.array([0, off[-1]]), 1)                                             # one run of 66 606 values
    assert np.array_equal(union.view(np.uint64), IO.moments(np.sort(wv), [0, off[-1]]).view(np.uint64))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_and_take_empty_volumes():
    import torch
    from covidseg_amd import volume as V
    lib, ctx = V._ctx()
    s = V._stream()
    vox = torch.zeros(64, dtype=torch.int16, device="cuda"); lab = torch.ones(64, dtype=torch.int32, device="cuda"); msk = torch.ones(64, dtype=torch.uint8, device="cuda")
    bc = torch.full((4, 6), 99, dtype=torch.int64, device="cuda"); sc = torch.full((4, 6), 99, dtype=torch.int64, device="cuda")
    mm = torch.full((4, 2), 99.0, dtype=torch.float64, device="cuda")
    val = torch.zeros(64, dtype=torch.float64, device="cuda"); grp = torch.zeros(64, dtype=torch.int32, device="cuda"); cnt = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    edges = np.array(IO.HU_EDGES)

    def bands(dtype=4, X=4, Y=4, Z=4, labels=lab, mask=None, n=4, e=edges, ne=None):
        return lib.unet_vol_intensity_bands(ctx.handle, vox.data_ptr(), dtype, X, Y, Z, 0, 1.0, 0.0, labels.data_ptr() if labels is not None else None,
                                            mask.data_ptr() if mask is not None else None, n, None, e.ctypes.data, len(e) if ne is None else ne, bc.data_ptr(), sc.data_ptr(),
                                            mm.data_ptr(), s)

    def gather(dtype=4, X=4, Y=4, Z=4, labels=lab, mask=None, n=4, cap=64):
        return lib.unet_vol_intensity_gather(ctx.handle, vox.data_ptr(), dtype, X, Y, Z, 0, 1.0, 0.0, labels.data_ptr() if labels is not None else None,
                                             mask.data_ptr() if mask is not None else None, n, None, val.data_ptr(), grp.data_ptr(), cap, cnt.data_ptr(), s)

    for call in (bands, gather):
        assert call(X=2048, Y=2048, Z=512) == E_ARG and "2^31" in ctx.last_error()
        assert call(dtype=3) == E_ARG and call(dtype=1024) == E_ARG and "datatype" in ctx.last_error()
        assert call(mask=msk) == E_ARG and call(labels=None) == E_ARG and "exactly one" in ctx.last_error()
        assert call(n=-1) == E_ARG and call(X=-1) == E_ARG
    assert gather(cap=-1) == E_ARG
    many = np.arange(64, dtype=np.float64)
    assert bands(ne=0) == E_ARG and bands(e=many) == E_ARG and "edges" in ctx.last_error()
    assert bands(e=np.array([1.0, 1.0])) == E_ARG and bands(e=np.array([2.0, 1.0])) == E_ARG and bands(e=np.array([0.0, np.inf])) == E_ARG and bands(e=np.array([np.nan])) == E_ARG
    torch.cuda.synchronize()
    assert (bc == 99).all() and (sc == 99).all() and (mm == 99.0).all() and int(cnt.item()) == 99          # nothing was launched
    assert lib.unet_vol_group_moments(ctx.handle, val.data_ptr(), cnt.data_ptr(), -1, mm.data_ptr(), bc.data_ptr(), 64, s) == E_ARG
    assert lib.unet_vol_group_moments(ctx.handle, val.data_ptr(), cnt.data_ptr(), 2, mm.data_ptr(), bc.data_ptr(), 8, s) == E_ARG and "workspace" in ctx.last_error()
    assert lib.unet_vol_group_moments(ctx.handle, None, None, 0, None, None, 0, s) == 0
    assert lib.unet_vol_group_moments_ws_bytes(65537, 3) >= 8 * (3 + 65537 // 256 + 3)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):                   # a zero dimension: status 0, the outputs in their empty state
        bc.fill_(99); sc.fill_(99); mm.fill_(99.0); cnt.fill_(99)
        assert bands(X=dims[0], Y=dims[1], Z=dims[2], mask=msk, labels=None) == 0 and gather(X=dims[0], Y=dims[1], Z=dims[2]) == 0
        torch.cuda.synchronize()
        assert not bc.any() and int(cnt.item()) == 0 and not sc[:dims[2]].any()
        assert mm.cpu().numpy().tolist() == [[np.inf, -np.inf]] * 4
    vol = _vol(np.zeros((0, 3, 2), np.int16), False)
    st = V.intensity_stats(vol, mask=np.zeros((0, 3, 2), np.uint8))
    assert st.voxels == 0 and np.isnan(st.mean) and st.slice_band_voxels.shape == (2, 5) and not st.slice_band_voxels.any()


# ---- intensity_stats ---------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(b).dtype.kind == "f")


def _check_stats(got, want, moments=True, per_slice=True):
    for k in ("voxels", "nan_voxels", "ml", "min", "max", "band_voxels", "band_ml", "band_share"):
        assert _same(getattr(got, k), want[k]), k
    for k in ("slice_band_voxels", "slice_nan_voxels"):
        assert _same(getattr(got, k), want[k]) if per_slice else getattr(got, k) is None, k
    if moments:
        assert _same(got.mean, want["mean"]) and _same(got.std, want["std"]) and got.percentiles.keys() == want["percentiles"].keys()
        assert all(_same(got.percentiles[q], want["percentiles"][q]) for q in got.percentiles)
    else:
        assert got.mean is None and got.std is None and got.percentiles is None
    gw = want["groups"]
    assert len(got.groups) == len(gw["label"]) == got.n
    for k in got.groups.dtype.names:
        if k in ("mean", "std", "percentiles") and not moments:
            assert np.isnan(got.groups[k]).all(), k
        else:
            assert _same(got.groups[k], gw[k]), k


def _lesion_volume():
    """(40, 36, 10) int16 with slope 0.5 / inter -1024 and three lesions: a ball, a slab that a wave crosses, a single voxel; one label outside 1..3"""
    shape = (40, 36, 10)
    rng = np.random.default_rng(40)
    x, y, z = np.mgrid[0:40, 0:36, 0:10]
    raw = (rng.normal(600.0, 500.0, shape)).round().astype(np.int16)
    raw[::7, ::5, ::3] = 148                                        # -950 exactly
    labels = np.zeros(shape, np.int32)
    labels[(x - 12) ** 2 + (y - 14) ** 2 + 4 * (z - 4) ** 2 < 60] = 1
    labels[25:39, 3:30, 6:9] = 2
    labels[39, 35, 9] = 3
    labels[0, 0, 0] = 9
    return shape, raw, labels


def test_intensity_stats_end_to_end():
    from covidseg_amd import volume as V
    shape, raw, labels = _lesion_volume()
    pixdim = (0.8, 0.8, 5.0)
    vol = _vol(raw, True, pixdim)
    fdata = vol.get_fdata()
    g = IO.group_of(shape, labels=labels, n=3)
    got = V.intensity_stats(vol, labels=labels, n=3)
    _check_stats(got, IO.stats(fdata, g, 3, pixdim=pixdim))
    assert got.names == IO.HU_NAMES and got.voxels == (g > 0).sum() and got.groups["voxels"][2] == 1 and got.band("ggo") == got.band_voxels[2]
    assert got.groups["mean"][2] == got.groups["min"][2] == fdata[39, 35, 9] and got.groups["std"][2] == 0.0
    _check_stats(V.intensity_stats(vol, labels=labels, n=3, moments=False), IO.stats(fdata, g, 3, pixdim=pixdim), moments=False)
    qs, edges = (0, 50, 100, 12.5), (-1000.0, -500.0)
    region = (np.random.default_rng(1).random(shape) < 0.7)
    want = IO.stats(fdata, IO.group_of(shape, labels=labels, n=4, region=region), 4, edges=edges, qs=qs, pixdim=pixdim)          # group 4 is empty
    got = V.intensity_stats(vol, labels=labels, n=4, region=region, edges=edges, names=("a", "b", "c"), percentiles=qs, per_slice=False)
    _check_stats(got, want, per_slice=False)
    assert got.groups["dominant_band"][3] == -1 and np.isnan(got.groups["mean"][3])
    m = labels > 0                                                  # a mask, as numpy and as the device buffers the volume path hands on
    want = IO.stats(fdata, IO.group_of(shape, mask=m, region=region), 1, pixdim=pixdim)
    _check_stats(V.intensity_stats(vol, mask=m, region=region), want)
    _check_stats(V.intensity_stats(vol, mask=_dev(m, np.uint8), region=_dev(region, np.uint8), shape=shape), want)
    _check_stats(V.intensity_stats(vol, labels=_dev(labels, np.int32), n=3, shape=shape), IO.stats(fdata, g, 3, pixdim=pixdim))
    plain = V.intensity_stats(raw.astype(np.float32), mask=m)       # a bare array: not scaled, 1 mm voxels
    _check_stats(plain, IO.stats(raw.astype(np.float64), IO.group_of(shape, mask=m), 1))


# ---- segment_volume(density=) --------------------------------------------------------------------------------------------------------------------------------
SIZE, Z, NEW_DIM = 128, 20, 64
F = np.float32


def _patient(tmp_path):
    """CT: int16 with slope 0.5 / inter -1000; lung mask: two blobs per slice, empty on a few slices"""
    import gzip, struct
    from covidseg_amd import nifti_min
    from covidseg_amd.data import synthetic_ct
    x, _ = synthetic_ct(Z, SIZE, seed=11)
    ct = np.empty((SIZE, SIZE, Z), np.int16, order="F"); lung = np.zeros((SIZE, SIZE, Z), np.uint8, order="F")
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    z0, _ = VO.trim_range(Z)
    for z in range(Z):
        ct[:, :, z] = np.round(x[z, :, :, 0] * 2800).astype(np.int16)
        if z not in (0, 1, z0 + 2, Z - 1):
            r = 1.0 + 0.02 * (z - Z / 2)
            lung[:, :, z] = (((xx - 38) / (22 * r)) ** 2 + ((yy - 64) / (40 * r)) ** 2 < 1) | (((xx - 90) / (24 * r)) ** 2 + ((yy - 66) / (38 * r)) ** 2 < 1)
    hdr = nifti_min.default_header(ct.shape, (0.8, 0.8, 5.0))
    paths = [tmp_path / "ct.nii.gz", tmp_path / "lung.nii.gz"]
    nifti_min.write(paths[1], lung, hdr)
    h = bytearray(hdr)
    struct.pack_into("<2h", h, 70, 4, 16); struct.pack_into("<3f", h, 108, 352.0, 0.5, -1000.0)
    paths[0].write_bytes(gzip.compress(bytes(h) + b"\0\0\0\0" + ct.tobytes(order="F"), 1))
    return paths, lung


class _Stub:
    """clip(a x + b ramp, 0, 1): a model that needs no training to mark part of every slice"""

    def __init__(self, a, b, d=NEW_DIM):
        self.h, self.a, self.b = d, F(a), F(b)
        i, j = np.mgrid[0:d, 0:d].astype(F)
        self.ramp = ((F(1.7) * i + F(0.6) * j + i * j / F(d)) / F(3.3 * d)).astype(F)[None, :, :, None]

    def __call__(self, x):
        return np.clip((self.a * np.asarray(x, F) + (self.b * self.ramp).astype(F)).astype(F), F(0), F(1)).astype(F)

    def predict(self, x, batch_size=32):
        return self(x.cpu().numpy() if hasattr(x, "cpu") else x)


def _threshold(paths, stub):
    from covidseg_amd import volume as V
    r1, r2, kept = V.load_volume(paths[1], "lungs", img_size=SIZE)
    x = V.load_volume(paths[0], "cts", img_size=SIZE, rects=(r1, r2, kept), box_indexing="slice", new_dim=NEW_DIM).cpu().numpy()
    return float(np.quantile(stub(x), 0.9))


def _check_density(res, fdata, lung, **kw):
    from covidseg_amd import volume as V
    pixdim = tuple(float(v) for v in res.pixdim)
    if res.lesions is not None:
        labels, n = V.label_volume(res.mask)
        assert n == res.n_lesions == res.density.n and np.array_equal(res.density.groups["voxels"], res.lesions["voxels"])
        g = IO.group_of(fdata.shape, labels=labels, n=n)
    else:
        n, g = 1, IO.group_of(fdata.shape, mask=res.mask)
    _check_stats(res.density, IO.stats(fdata, g, n, pixdim=pixdim, **kw))
    assert res.density.voxels == res.counts.sum() and res.seconds["density"] > 0.0
    _check_stats(res.lung_density, IO.stats(fdata, IO.group_of(fdata.shape, mask=lung), 1, pixdim=pixdim, **kw))
    assert res.lung_density.n == 1 and res.lung_density.voxels == np.count_nonzero(lung)


def test_segment_volume_reports_the_density_under_its_mask(tmp_path):
    from covidseg_amd import nifti_min, volume as V
    paths, lung = _patient(tmp_path)
    stub = _Stub(0.9, 0.35)
    t = _threshold(paths, stub)
    fdata = nifti_min.read(paths[0]).get_fdata()
    kw = dict(lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    plain = V.segment_volume(paths[0], stub, min_lesion_ml=0.05, **kw)
    off = V.segment_volume(paths[0], stub, min_lesion_ml=0.05, density=None, **kw)
    assert off.density is None and off.lung_density is None and "density" not in off.seconds and plain.density is None
    for k, v in plain.__dict__.items():
        if k != "seconds":
            assert V._same(v, off.__dict__[k]) or v == off.__dict__[k], k
    res = V.segment_volume(paths[0], stub, min_lesion_ml=0.05, density=True, **kw)          # per lesion, on the labels of the filter
    assert np.array_equal(res.mask, plain.mask) and np.array_equal(res.lesions, plain.lesions) and res.mask.any() and res.n_lesions >= 1
    print(f"{res.n_lesions} lesions, removed {res.removed_ml:.3f} ml, bands {res.density.band_voxels.tolist()}")
    _check_density(res, fdata, lung)
    res = V.segment_volume(paths[0], stub, lesions=True, density={"percentiles": (50,)}, **kw)          # per lesion, nothing filtered
    _check_density(res, fdata, lung, qs=(50,))
    edges = (-900.0, -400.0, 0.0, 200.0, 399.5)
    res = V.segment_volume(paths[0], stub, density={"edges": edges, "names": None, "moments": False}, **kw)          # no lesion table: the mask is one group
    assert res.lesions is None and res.density.n == 1 and res.density.mean is None and res.density.names[5] == "band5"
    want = IO.stats(fdata, IO.group_of(fdata.shape, mask=res.mask), 1, edges=edges, pixdim=tuple(float(v) for v in res.pixdim))
    _check_stats(res.density, want, moments=False)
    with pytest.raises(ValueError):
        V.segment_volume(paths[0], stub, density={"edges": (1.0, 0.0)}, **kw)


def test_segment_volume_ensemble_reports_the_density_under_its_mask(tmp_path):
    from covidseg_amd import nifti_min, volume as V
    paths, lung = _patient(tmp_path)
    stubs = [_Stub(0.9, 0.35), _Stub(0.6, 0.8)]
    t = _threshold(paths, stubs[0])
    fdata = nifti_min.read(paths[0]).get_fdata()
    kw = dict(tta=("id", "hflip"), combine="majority", lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    plain = V.segment_volume_ensemble(paths[0], stubs, lesions=True, **kw)
    assert plain.density is None and plain.lung_density is None
    res = V.segment_volume_ensemble(paths[0], stubs, lesions=True, density={"percentiles": (10, 90)}, **kw)
    assert np.array_equal(res.mask, plain.mask) and np.array_equal(res.votes, plain.votes) and np.array_equal(res.lesions, plain.lesions) and res.mask.any()
    _check_density(res, fdata, lung, qs=(10, 90))

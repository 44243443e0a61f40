"""-m gpu: csrc/kernels_lungside.hip and volume.split_lungs / lung_burden / segment_volume(per_lung=) against tests/lungside_oracle.py.  Sides, counts and tables are
integers, the distances behind them are the exact transform the other oracles define: every comparison is array_equal / ==."""
import gzip
import struct

import numpy as np
import pytest

import intensity_oracle as IO
import lungside_oracle as LO
import volume_oracle as VO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
SHAPES = [(5, 3, 2), (64, 4, 3), (67, 9, 7), (64, 8, 1), (1, 1, 1)]          # x short of a wave, exactly on it, past it; one slice; one voxel
SENTINEL = 0x5A


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.asfortranarray(np.asarray(a).astype(dtype)).reshape(-1, order="F")).cuda()


def _flat(a):
    return np.asarray(a).reshape(-1, order="F")


# ---- unet_vol_side_assign ------------------------------------------------------------------------------------------------------------------------------
def _assign_inputs(shape, rng):
    """a mask with whole background waves, distances with planted ties, +inf on either or both sides, and zeros"""
    N = int(np.prod(shape))
    mask = (rng.random(N) < 0.6).astype(np.uint8) * rng.integers(1, 255, N).astype(np.uint8)
    if N > 600:
        mask[256:512] = 0                                           # waves of the 4-voxel path and of the 1-voxel path that see no mask voxel
    a = (rng.integers(0, 40, N) * 0.5625).astype(np.float64)        # few distinct values: many ties
    b = (rng.integers(0, 40, N) * 0.5625).astype(np.float64)
    b[::7] = a[::7]
    a[3::11] = np.inf
    b[5::13] = np.inf
    b[3::33] = np.inf                                               # inf on both sides
    return mask.reshape(shape, order="F"), a.reshape(shape, order="F"), b.reshape(shape, order="F")


def _run_assign(o, mask_t, a_t, b_t, shape, side_a, side_b, offset=0):
    """-> (sides numpy, counts numpy); the outputs lie inside larger buffers filled with a sentinel, which must survive"""
    import torch
    N = int(np.prod(shape))
    sides = torch.full((offset + N + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    counts = torch.full((3 + 5,), -77, dtype=torch.int64, device="cuda")
    o.ck(o.lib.unet_vol_side_assign(o.h, mask_t.data_ptr(), a_t.data_ptr(), b_t.data_ptr(), *shape, side_a, side_b, sides.data_ptr() + offset, counts.data_ptr(), o.s), "side_assign")
    s, c = sides.cpu().numpy(), counts.cpu().numpy()
    assert (s[:offset] == SENTINEL).all() and (s[offset + N:] == SENTINEL).all() and (c[3:] == -77).all()
    return s[offset:offset + N], c[:3]


@pytest.mark.parametrize("shape", SHAPES)
def test_side_assign_equals_the_oracle(shape):
    o = Ops()
    rng = np.random.default_rng(sum(shape))
    mask, a, b = _assign_inputs(shape, rng)
    mt, at, bt = _dev(mask, np.uint8), _dev(a, np.float64), _dev(b, np.float64)
    for side_a, side_b in ((1, 2), (2, 1)):
        want, wc = LO.side_assign(mask, a, b, side_a, side_b)
        got, gc = _run_assign(o, mt, at, bt, shape, side_a, side_b)
        assert np.array_equal(got, _flat(want)) and np.array_equal(gc, wc), (shape, side_a)
        ties = (_flat(mask) != 0) & (_flat(a) == _flat(b))
        assert (got[ties] == 1).all() and (ties.sum() > 0 or np.prod(shape) < 8)          # the seed whose side is 1 wins, whichever argument it is
    swapped, _ = _run_assign(o, mt, bt, at, shape, 2, 1)             # the same two seeds handed over in the other order: the same volume
    assert np.array_equal(swapped, _flat(LO.side_assign(mask, a, b, 1, 2)[0]))
    got1, gc1 = _run_assign(o, mt, at, bt, shape, 1, 2, offset=1)    # sides off its 4-byte alignment: the one-voxel path
    assert np.array_equal(got1, _flat(LO.side_assign(mask, a, b)[0])) and np.array_equal(gc1, LO.side_assign(mask, a, b)[1])


def test_side_assign_refusals_and_empty_volumes():
    import torch
    o = Ops()
    m, a, b = _dev(np.ones(8), np.uint8), _dev(np.zeros(8), np.float64), _dev(np.zeros(8), np.float64)
    sides = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
    counts = torch.full((3,), -77, dtype=torch.int64, device="cuda")
    call = lambda X, Y, Z, sa, sb, mp=None, sp=None: o.lib.unet_vol_side_assign(o.h, mp or m.data_ptr(), a.data_ptr(), b.data_ptr(), X, Y, Z, sa, sb, sp or sides.data_ptr(), counts.data_ptr(), o.s)
    for args in ((2, 2, 2, 1, 1), (2, 2, 2, 0, 1), (2, 2, 2, 2, 3), (-1, 2, 2, 1, 2), (2048, 1024, 1024, 1, 2), (65536, 65536, 0, 1, 2)):
        assert call(*args) == E_ARG, args
    assert call(2, 2, 2, 1, 2, sp=m.data_ptr()) == E_ARG             # in place
    assert o.lib.unet_vol_side_assign(o.h, m.data_ptr(), a.data_ptr() + 4, b.data_ptr(), 2, 2, 1, 1, 2, sides.data_ptr(), counts.data_ptr(), o.s) == E_ARG
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        o.ck(call(*dims, 1, 2), "empty")
    torch.cuda.synchronize()
    assert (sides.cpu().numpy() == SENTINEL).all() and (counts.cpu().numpy() == -77).all()          # a zero dimension touches nothing


# ---- unet_vol_side_table ---------------------------------------------------------------------------------------------------------------------------------
def _run_table(o, sides, infection, labels, n, shape, per_slice=True):
    import torch
    Z = shape[2]
    st = _dev(sides, np.uint8)
    it = _dev(infection, np.uint8) if infection is not None else None
    lt = _dev(labels, np.int32) if labels is not None else None
    totals = torch.full((6 + 4,), -77, dtype=torch.int64, device="cuda")
    les = torch.full((3 * n + 4,), -77, dtype=torch.int64, device="cuda")
    ps = torch.full((6 * Z + 4,), -77, dtype=torch.int64, device="cuda")
    o.ck(o.lib.unet_vol_side_table(o.h, st.data_ptr(), it.data_ptr() if it is not None else None, lt.data_ptr() if lt is not None else None, n, *shape, totals.data_ptr(),
                                   les.data_ptr(), ps.data_ptr() if per_slice else None, o.s), "side_table")
    t, l, p = totals.cpu().numpy(), les.cpu().numpy(), ps.cpu().numpy()
    assert (t[6:] == -77).all() and (l[3 * n:] == -77).all() and (p[6 * Z:] == -77).all() and (per_slice or (p == -77).all())
    return t[:6].reshape(2, 3), l[:3 * n].reshape(n, 3), p[:6 * Z].reshape(Z, 6)


def _check_table(o, sides, infection, labels, n, what):
    shape = sides.shape
    want = LO.side_table(sides, infection, labels, n)
    got = _run_table(o, sides, infection, labels, n, shape)
    for name, a, b in zip(("totals", "lesion_side", "per_slice"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, shape, name)
    t, l, _ = _run_table(o, sides, infection, labels, n, shape, per_slice=False)
    assert np.array_equal(t, want[0]) and np.array_equal(l, want[1]), (what, "no per_slice")


@pytest.mark.parametrize("shape", SHAPES)
def test_side_table_equals_the_oracle(shape):
    o = Ops()
    rng = np.random.default_rng(10 + sum(shape))
    N = int(np.prod(shape))
    f = np.arange(N).reshape(shape, order="F")
    sides = rng.integers(0, 3, shape).astype(np.uint8)
    inf = (rng.random(shape) < 0.4).astype(np.uint8) * 9
    sparse = rng.integers(-2, 10, shape)
    sparse[sparse == 3] = 0                                         # label 3 has no voxel; -2, -1, 0 and 7..9 lie outside 1..6
    _check_table(o, sides, inf, f % 64 + 1, 64, "64 lesions share a wave")
    _check_table(o, sides, inf, sparse, 6, "missing and outside labels")
    _check_table(o, sides, inf, sparse, 0, "n = 0")
    _check_table(o, sides, inf, sparse, 1, "n = 1")
    _check_table(o, sides, None, sparse, 6, "no infection")
    _check_table(o, sides, inf, None, 6, "no labels")
    _check_table(o, sides, None, None, 0, "sides alone")
    _check_table(o, np.where(rng.random(shape) < 0.1, 200, sides).astype(np.uint8), inf, sparse, 6, "side values above 2")
    _check_table(o, np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), np.zeros(shape, np.int32), 3, "nothing anywhere")


@pytest.mark.parametrize("n", [1365, 1366])
def test_side_table_on_both_sides_of_the_lds_limit(n):
    """3 n = 4095 fits the workgroup's table, 3 n = 4098 goes straight to the output"""
    o = Ops()
    rng = np.random.default_rng(n)
    shape = (67, 9, 7)
    sides = rng.integers(0, 3, shape).astype(np.uint8)
    inf = (rng.random(shape) < 0.5).astype(np.uint8)
    labels = rng.integers(0, n + 3, shape)
    labels.reshape(-1)[:8] = [n, n, n + 1, 1, 1, n - 1, 2 ** 31 - 1, -2 ** 31]
    _check_table(o, sides, inf, labels, n, f"n = {n}")


def test_side_table_slice_change_inside_a_workgroup():
    """more slices than workgroups: every workgroup walks several slices and hands its slice counters over at each change"""
    o = Ops()
    rng = np.random.default_rng(3)
    shape = (5, 1, 2100)
    sides = rng.integers(0, 3, shape).astype(np.uint8)
    inf = (rng.random(shape) < 0.5).astype(np.uint8)
    _check_table(o, sides, inf, rng.integers(0, 5, shape), 4, "2100 slices")


def test_side_table_refusals_and_empty_volumes():
    import torch
    o = Ops()
    s = _dev(np.ones(8), np.uint8)
    out = torch.full((64,), -77, dtype=torch.int64, device="cuda")
    call = lambda X, Y, Z, n, tp=None: o.lib.unet_vol_side_table(o.h, s.data_ptr(), None, None, n, X, Y, Z, tp or out.data_ptr(), out.data_ptr() + 64, out.data_ptr() + 128, o.s)
    for args in ((2, 2, 2, -1), (-1, 2, 2, 0), (2048, 1024, 1024, 0)):
        assert call(*args) == E_ARG, args
    assert call(2, 2, 2, 0, tp=out.data_ptr() + 4) == E_ARG          # misaligned totals
    assert o.lib.unet_vol_side_table(o.h, s.data_ptr(), None, None, 2, 2, 2, 2, out.data_ptr(), None, None, o.s) == E_ARG          # n > 0 without a lesion table
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        o.ck(call(*dims, 2), "empty")
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -77).all()


# ---- split_lungs -------------------------------------------------------------------------------------------------------------------------------------------
PIXDIM = (0.75, 0.75, 2.5)
PHANTOMS = {"separate": lambda: LO.fused_lungs((48, 40, 12), PIXDIM, gap=4.0), "fused": lambda: LO.fused_lungs((48, 40, 12), PIXDIM)}
_WANT = {}


def _want_split(name, codes):
    """the oracle's answer for a phantom stored with axis codes `codes`, computed once"""
    if (name, codes) not in _WANT:
        m = LO.reorient(PHANTOMS[name](), codes)
        pix = LO.reorient_pixdim(PIXDIM, codes)
        _WANT[name, codes] = (m, pix, LO.split(m, LO.affine_of(codes, pix), pix))
    return _WANT[name, codes]


def _oriented_header(shape, pixdim, codes, sform=True):
    from covidseg_amd import nifti_min
    h = bytearray(nifti_min.default_header(shape, pixdim))
    a = LO.affine_of(codes, pixdim)
    if sform:
        struct.pack_into("<h", h, 254, 1)
        struct.pack_into("<12f", h, 280, *a[:3].reshape(-1))
    return bytes(h)


@pytest.mark.parametrize("name", ["separate", "fused"])
@pytest.mark.parametrize("codes", ["LPS", "ASR"])
def test_split_lungs_equals_the_oracle(name, codes, tmp_path):
    from covidseg_amd import nifti_min, volume as V
    m, pix, want = _want_split(name, codes)
    assert (want["radius_mm"] == 0.0) == (name == "separate") and min(want["voxels"]) > 0
    got = V.split_lungs(m, orientation=codes, pixdim=pix)
    assert got.sides.dtype == np.uint8 and got.sides.shape == m.shape and np.array_equal(got.sides, want["sides"])
    assert got.radius_mm == want["radius_mm"] and got.voxels == want["voxels"] and got.seed_voxels == want["seed_voxels"] and got.axcodes == tuple(codes)
    ml = float(np.prod(np.asarray(pix, np.float64))) / 1000.0
    assert got.ml == (want["voxels"][0] * ml, want["voxels"][1] * ml) and got.shape == m.shape
    # the same from a file whose sform says so, from an affine, and from the device
    p = tmp_path / "lung.nii.gz"
    nifti_min.write(p, m, _oriented_header(m.shape, pix, codes))
    out = tmp_path / "sides.nii.gz"
    f = V.split_lungs(p, out_path=out)
    assert np.array_equal(f.sides, want["sides"]) and f.axcodes == tuple(codes) and f.pixdim == tuple(float(np.float32(v)) for v in pix)
    back = nifti_min.read(out)
    assert np.array_equal(back.raw, want["sides"]) and back.axcodes == tuple(codes) and back.header[252:328] == nifti_min.read(p).header[252:328]
    d = V.split_lungs(_dev(m, np.uint8), orientation=LO.affine_of(codes, pix), pixdim=pix, shape=m.shape, return_device=True)
    assert d.sides.is_cuda and np.array_equal(d.sides.cpu().numpy().reshape(m.shape, order="F"), want["sides"])
    flipped = V.split_lungs(m, orientation=LO.affine_of(codes, pix) * np.array([-1.0, 1.0, 1.0, 1.0])[:, None], pixdim=pix)          # world x turned over: the lungs swap
    assert np.array_equal(flipped.sides, np.where(want["sides"] == 0, 0, 3 - want["sides"])) or (want["d2_left"] == want["d2_right"])[m != 0].any()


def test_split_lungs_errors_on_the_device():
    from covidseg_amd import volume as V
    one = LO.boxes((22, 12, 10), ((2, 9), (2, 10), (2, 8)), ((2, 9), (2, 10), (2, 8)))
    with pytest.raises(V.LungSplitError, match="336 and 0"):
        V.split_lungs(one, orientation="LPS")
    two = LO.boxes((22, 12, 10), ((2, 9), (2, 10), (2, 8)), ((13, 20), (2, 10), (2, 8)))
    with pytest.raises(V.LungSplitError, match="same world x"):
        V.split_lungs(two, orientation="ARS")
    with pytest.raises(V.LungSplitError, match="0 and 0"):
        V.split_lungs(np.zeros((6, 5, 4), np.uint8), orientation="LPS")


def _invariance_phantom():
    """12 x 10 x 6 in the canonical frame at pixdim (0.5, 0.75, 2.5): two blocks that reach the x faces (the erosion takes nothing from a face), joined by a bar one
    voxel thick.  r = 1 mm takes two voxels along x and one along y from every open side and the whole bar: the seeds are x = 0..2 and x = 10..11, y = 2..7, z = 1..4,
    and every mask voxel at x = 6 inside that y, z range lies 2 mm from both (planted ties)"""
    m = np.zeros((12, 10, 6), np.uint8)
    m[0:5, 1:9, 1:5] = 1
    m[8:12, 1:9, 1:5] = 1
    m[5:8, 4, 2] = 1                                                 # the bar
    m[6, 2:8, 3] = 1                                                 # more voxels half way
    return m


def test_the_split_is_the_same_in_all_48_storage_orders():
    """pixdim (0.5, 0.75, 2.5): the squares are dyadic, every squared distance is exact in any order of its three terms, so all 48 storage orders give the same volume"""
    from covidseg_amd import volume as V
    base = _invariance_phantom()
    pix_ras = (0.5, 0.75, 2.5)
    ref = LO.split(base, LO.affine_of("RAS", pix_ras), pix_ras)
    ties = (base != 0) & (ref["d2_left"] == ref["d2_right"])
    assert ties.sum() >= 4 and (ref["sides"][ties] == 1).all() and ref["radius_mm"] > 0 and min(ref["voxels"]) > 0
    for codes in LO.all_axcodes():
        stored, pix = LO.reorient(base, codes), LO.reorient_pixdim(pix_ras, codes)
        got = V.split_lungs(stored, orientation="".join(codes), pixdim=pix)
        assert got.axcodes == codes and got.radius_mm == ref["radius_mm"]
        assert np.array_equal(LO.to_canonical(got.sides, codes), ref["sides"]), codes
        assert got.voxels == ref["voxels"] and got.seed_voxels == ref["seed_voxels"]


# ---- lung_burden ----------------------------------------------------------------------------------------------------------------------------------------------
def _check_burden(b, want, n):
    assert b.left.lung_ml == want["left"]["lung_ml"] and b.left.infected_ml == want["left"]["infected_ml"]
    assert b.right.lung_ml == want["right"]["lung_ml"] and b.right.infected_ml == want["right"]["infected_ml"]
    for got, w in ((b.left.fraction, want["left"]["fraction"]), (b.right.fraction, want["right"]["fraction"])):
        assert got == w or (np.isnan(got) and np.isnan(w))
    assert b.outside_ml == want["outside_ml"] and b.bilateral == want["bilateral"]
    assert np.array_equal(b.per_slice, want["per_slice"]) and b.per_slice.dtype == np.int64
    les = want["lesion_side"]
    assert len(b.lesions) == n and np.array_equal(b.lesions["label"], np.arange(1, n + 1))
    assert np.array_equal(b.lesions["voxels_outside"], les[:, 0]) and np.array_equal(b.lesions["voxels_left"], les[:, 1]) and np.array_equal(b.lesions["voxels_right"], les[:, 2])
    assert b.lesions["side"].tolist() == want["side"].tolist()


def test_lung_burden_equals_the_oracle():
    from covidseg_amd import volume as V
    m, pix, want = _want_split("fused", "LPS")
    rng = np.random.default_rng(4)
    inf = np.zeros(m.shape, np.uint8)
    for _ in range(14):                                              # small boxes: inside a lung, across the junction, outside
        c = [int(rng.integers(0, s - 3)) for s in m.shape]
        inf[c[0]:c[0] + int(rng.integers(1, 6)), c[1]:c[1] + int(rng.integers(1, 6)), c[2]:c[2] + int(rng.integers(1, 3))] = 3
    inf[24, 20, 6] = 1
    lab, n = LO.CO.label(inf)
    assert n >= 4
    wb = LO.burden(inf, want["sides"], pixdim=pix)
    assert set(wb["side"].tolist()) == {"left", "right", "none"} and wb["bilateral"]
    _check_burden(V.lung_burden(inf, want["sides"], pixdim=pix), wb, n)
    ls = V.split_lungs(m, orientation="LPS", pixdim=pix, return_device=True)
    _check_burden(V.lung_burden(_dev(inf, np.uint8), ls, pixdim=pix, shape=m.shape), wb, n)          # a LungSides on the device, the infection on the device
    _check_burden(V.lung_burden(inf, want["sides"], labels=lab, n=n, pixdim=pix), wb, n)          # the caller's labels
    _check_burden(V.lung_burden(inf, want["sides"], labels=_dev(lab, np.int32), n=n, pixdim=pix), wb, n)
    lab3, n3 = LO.CO.label(inf, 3)
    _check_burden(V.lung_burden(inf, want["sides"], pixdim=pix, connectivity=3), LO.burden(inf, want["sides"], lab3, n3, pix), n3)
    none = V.lung_burden(np.zeros(m.shape, np.uint8), np.zeros(m.shape, np.uint8))
    assert np.isnan(none.left.fraction) and np.isnan(none.right.fraction) and not none.bilateral and len(none.lesions) == 0 and none.outside_ml == 0.0


# ---- segment_volume(per_lung=) -------------------------------------------------------------------------------------------------------------------------------
SIZE, Z, NEW_DIM = 128, 20, 64
F = np.float32
CODES = ("P", "L", "S")                                             # the lungs of the phantom lie side by side along voxel axis 1, which grows to the patient's left


def _patient(tmp_path, oriented=True):
    """CT: int16 with slope 0.5 / inter -1000; lung mask: two blobs per slice that grow with z and touch on the upper slices, none on a few slices; both files carry the same sform"""
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
    pix = (0.8, 0.8, 5.0)
    hdr = _oriented_header(ct.shape, pix, CODES, sform=oriented)
    paths = [tmp_path / "ct.nii.gz", tmp_path / "lung.nii.gz"]
    nifti_min.write(paths[1], lung, hdr)
    h = bytearray(hdr)
    struct.pack_into("<2h", h, 70, 4, 16); struct.pack_into("<3f", h, 108, 352.0, 0.5, -1000.0)
    paths[0].write_bytes(gzip.compress(bytes(h) + b"\0\0\0\0" + ct.tobytes(order="F"), 1))
    return paths, lung, pix


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


def _check_per_lung(res, lung, pix, connectivity=1):
    """res.per_lung against the oracle applied to the lung mask and to the mask the pipeline returned"""
    from covidseg_amd import volume as V
    pix = tuple(float(np.float32(v)) for v in pix)
    assert res.per_lung_error is None and res.seconds["per_lung"] > 0.0
    if "patient" not in _WANT:                                      # one lung mask serves every pipeline test: its reference is computed once
        _WANT["patient"] = LO.split(lung, LO.affine_of(CODES, pix), pix)
    want = _WANT["patient"]
    b = res.per_lung
    assert np.array_equal(b.sides.sides, want["sides"]) and b.sides.radius_mm == want["radius_mm"] and b.sides.axcodes == CODES
    lab, n = V.label_volume(res.mask, connectivity)
    _check_burden(b, LO.burden(res.mask, want["sides"], lab, n, pix), n)
    if res.lesions is not None:
        assert n == res.n_lesions and np.array_equal(b.lesions["label"], res.lesions["label"])
        assert np.array_equal(b.lesions["voxels_outside"] + b.lesions["voxels_left"] + b.lesions["voxels_right"], res.lesions["voxels"])
    assert b.left.infected_voxels + b.right.infected_voxels + b.outside_voxels == int(res.counts.sum())
    return want


def test_segment_volume_reports_the_burden_per_lung(tmp_path):
    from covidseg_amd import nifti_min, volume as V
    paths, lung, pix = _patient(tmp_path)
    stub = _Stub(0.9, 0.35)
    t = _threshold(paths, stub)
    kw = dict(lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    plain = V.segment_volume(paths[0], stub, min_lesion_ml=0.05, **kw)
    assert plain.per_lung is None and plain.per_lung_error is None and "per_lung" not in plain.seconds
    res = V.segment_volume(paths[0], stub, min_lesion_ml=0.05, per_lung=True, **kw)          # on the labels of the filter
    assert np.array_equal(res.mask, plain.mask) and np.array_equal(res.lesions, plain.lesions) and res.lesions.dtype == V.LESION_DTYPE and res.mask.any()
    for k, v in plain.__dict__.items():
        if k not in ("seconds", "per_lung"):
            assert V._same(v, res.__dict__[k]) or v == res.__dict__[k], k
    want = _check_per_lung(res, lung, pix)
    assert want["radius_mm"] > 0.0 and res.per_lung.density is None          # the lungs of this patient touch on the upper slices
    print(f"{res.n_lesions} lesions; left {res.per_lung.left!r}; right {res.per_lung.right!r}; sides {sorted(set(res.per_lung.lesions['side'].tolist()))}")
    res = V.segment_volume(paths[0], stub, lesions=True, per_lung={"min_ratio": 0.5}, density={"percentiles": (50,)}, **kw)          # nothing filtered; density per lung as well
    _check_per_lung(res, lung, pix)
    fdata = nifti_min.read(paths[0]).get_fdata()
    wd = IO.stats(fdata, IO.group_of(fdata.shape, labels=want["sides"].astype(np.int32), n=2), 2, qs=(50,), pixdim=tuple(float(v) for v in res.pixdim))
    d = res.per_lung.density
    assert d.n == 2 and np.array_equal(d.groups["voxels"], [want["voxels"][0], want["voxels"][1]]) and np.array_equal(d.groups["band_voxels"], wd["groups"]["band_voxels"])
    assert np.array_equal(d.groups["mean"], wd["groups"]["mean"]) and np.array_equal(d.groups["percentiles"], wd["groups"]["percentiles"])
    assert np.array_equal(d.groups["min"], wd["groups"]["min"]) and np.array_equal(d.groups["max"], wd["groups"]["max"])
    res = V.segment_volume(paths[0], stub, per_lung=True, connectivity=2, **kw)          # no lesion table: the mask is labelled for the burden alone
    assert res.lesions is None
    _check_per_lung(res, lung, pix, connectivity=2)


def test_a_failed_split_keeps_the_segmentation(tmp_path):
    from covidseg_amd import volume as V
    paths, lung, pix = _patient(tmp_path, oriented=False)
    stub = _Stub(0.9, 0.35)
    kw = dict(lung_mask=paths[1], threshold=_threshold(paths, stub), batch_size=8, img_size=SIZE)
    plain = V.segment_volume(paths[0], stub, lesions=True, **kw)
    res = V.segment_volume(paths[0], stub, lesions=True, per_lung=True, **kw)          # neither file says where left is
    assert res.per_lung is None and "orientation" in res.per_lung_error and np.array_equal(res.mask, plain.mask) and np.array_equal(res.lesions, plain.lesions)
    assert res.seconds["per_lung"] >= 0.0
    res = V.segment_volume(paths[0], stub, lesions=True, per_lung={"orientation": "PLS", "min_ratio": 1.0, "erode_mm": (1,)}, **kw)          # the lungs differ in size
    assert res.per_lung is None and "largest two counts" in res.per_lung_error and np.array_equal(res.mask, plain.mask)
    res = V.segment_volume(paths[0], stub, lesions=True, per_lung={"orientation": "PLS"}, **kw)          # the orientation as an argument
    _check_per_lung(res, lung, pix)


def test_segment_volume_ensemble_reports_the_burden_per_lung(tmp_path):
    from covidseg_amd import volume as V
    paths, lung, pix = _patient(tmp_path)
    stubs = [_Stub(0.9, 0.35), _Stub(0.6, 0.8)]
    kw = dict(tta=("id", "hflip"), combine="majority", lung_mask=paths[1], threshold=_threshold(paths, stubs[0]), batch_size=8, img_size=SIZE)
    plain = V.segment_volume_ensemble(paths[0], stubs, lesions=True, **kw)
    assert plain.per_lung is None
    res = V.segment_volume_ensemble(paths[0], stubs, lesions=True, per_lung=True, **kw)
    assert np.array_equal(res.mask, plain.mask) and np.array_equal(res.votes, plain.votes) and np.array_equal(res.lesions, plain.lesions) and res.mask.any()
    _check_per_lung(res, lung, pix)

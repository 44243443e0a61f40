"""GPU: unet_vol_rank_filter (csrc/kernels_filter.hip) and filters.* against tests/filter_oracle.py, every comparison for equality (float32: of the raw bits).

Which cases reach which selection path of the kernel.  The host picks the instance from the footprint's n and the rank; the first pass over a voxel's n keys gives the
smallest and the largest key:
  * rank kinds "min" and "max" (ranks 0 and n - 1), and so every rank of the footprints with n = 1 and n = 2, take the instance that counts from the staged brick and
    end after that pass, whatever n is;
  * rank kinds "second", "median" and "second_largest" (ranks 1, n // 2, n - 2) with n >= 3 take the instance that holds the keys in 8 registers for n <= 8 (cross7,
    planar5), in 27 registers for n <= 27 (planar9, s19, box27) and the staged-brick instance beyond (random64, random124, box125);
  * inside each of them a voxel whose footprint holds one value ends after the first pass: the constant block in the corner of every volume with more than 64 voxels;
  * every other voxel is bisected from the highest bit in which its smallest and largest key differ: at most 8 rounds for uint8 / int8, 16 for int16 / uint16 (the
    int16 volumes span -32768 .. 32767, so bit 15 is met) and 32 for int32 / uint32 / float32 (the int32 and float32 volumes hold both signs, so bit 31 is met); the
    narrow-range stripe of every volume starts its bisection at a low bit.
The small shapes take every instance at every key width; test_int16_spans_its_full_range_and_float32_holds_the_specials does so on two bricks and test_larger_shapes_
walk_the_product asserts a bisection at every key width."""
import os
import re

import numpy as np
import pytest
import torch

import filter_oracle as FO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

CODES = {"u1": 2, "i1": 256, "i2": 4, "u2": 512, "i4": 8, "u4": 768, "f4": 16}
MODE = {"nearest": 0, "constant": 1, "reflect": 2}
SMALL = [(1, 1, 1), (2, 1, 3), (1, 5, 2), (3, 2, 2)]                # extents below R: reflect wraps more than once
LARGE = [(31, 7, 9), (32, 8, 8), (33, 9, 17), (65, 5, 3), (129, 6, 4), (200, 7, 3)]          # brick edges: one short of, exactly and one beyond 32 x 8 x 8; up to 7 bricks along x
RANK_KINDS = ("min", "second", "median", "second_largest", "max")
BAND = 96                                                            # sentinel elements either side of dst
SENTINEL = 0xA5


def _footprints():
    fps = [("cross7", FO.structure(1)), ("s19", FO.structure(2)), ("box27", FO.structure(3)), ("planar5", FO.structure(1, True)), ("planar9", FO.structure(2, True)),
           ("box125", np.ones((5, 5, 5), bool))]
    for n in (1, 2, 64, 124):
        fp = FO.random_footprint(2, n, 1000 + n)
        fps.append((f"random{n}", fp))
    return fps


FOOTPRINTS = _footprints()


def _rank(kind, n):
    return {"min": 0, "second": min(1, n - 1), "median": n // 2, "second_largest": max(n - 2, 0), "max": n - 1}[kind]


def _volume(shape, dt, seed):
    rng = np.random.default_rng(seed)
    if dt == "f4":
        a = (rng.standard_normal(shape) * 300).astype(np.float32)
        f = a.reshape(-1)
        special = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001], np.uint32).view(np.float32)
        idx = rng.choice(f.size, max(1, f.size // 6), replace=False)          # NaNs of both signs, +-0, +-inf, denormals
        f[idx] = special[rng.integers(0, special.size, idx.size)]
    else:
        info = np.iinfo(np.dtype(dt))
        a = rng.integers(info.min, int(info.max) + 1, shape, dtype=np.int64).astype(np.dtype(dt))
        f = a.reshape(-1)
        f[rng.choice(f.size, max(1, f.size // 8), replace=False)] = info.min
        f[rng.choice(f.size, max(1, f.size // 8), replace=False)] = info.max
    if a.size > 64:
        a[:6, :5, :3] = a[0, 0, 0]                                    # a constant block: its inner voxels see one value
        stripe = rng.integers(0, 4, a[-8:, :, :].shape)              # a narrow range: the bisection starts at bit 1
        a[-8:, :, :] = stripe.astype(a.dtype) if dt != "f4" else (np.float32(100.0) + stripe.astype(np.float32))
    return np.asfortranarray(a)


def _cval_bits(dt, seed):
    rng = np.random.default_rng(seed)
    if dt == "f4":
        return int(np.array([-7.5, np.nan, 0.0, 1e30][seed % 4], np.float32).view(np.uint32))
    return int(rng.integers(0, 2 ** (8 * np.dtype(dt).itemsize)))


def _cval_of(bits, dt):
    return np.array([bits], np.uint64).astype(np.dtype("u" + dt[1])).view(np.dtype(dt))[0]


def _words(fp):
    from covidseg_amd import filters as F
    return F.footprint_bits(fp)


def _call(ops, a, fp, rank, mode, cval_bits=0, src_offset=0):
    """-> (rc, the filtered volume, whether the sentinel bands survived); src may start src_offset elements into its buffer"""
    dt = a.dtype
    eb, N = dt.itemsize, a.size
    flat = np.ascontiguousarray(a.reshape(-1, order="F")).view(np.uint8)
    src = torch.empty((N + src_offset) * eb + 8, dtype=torch.uint8, device="cuda")
    src[src_offset * eb:(src_offset + N) * eb] = torch.from_numpy(flat).cuda()
    dst = torch.full(((N + 2 * BAND) * eb,), SENTINEL, dtype=torch.uint8, device="cuda")
    R, lo, hi = _words(fp)
    rc = ops.lib.unet_vol_rank_filter(ops.h, src.data_ptr() + src_offset * eb, CODES[dt.str[1:]], *a.shape, R, lo, hi, rank, mode, cval_bits, dst.data_ptr() + BAND * eb, ops.s)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    bands = bool((host[:BAND * eb] == SENTINEL).all() and (host[(BAND + N) * eb:] == SENTINEL).all())
    return rc, np.asfortranarray(host[BAND * eb:(BAND + N) * eb].view(dt).reshape(a.shape, order="F")), bands


def _check(ops, a, name, fp, kind, mode, cval_bits):
    dt = a.dtype.str[1:]
    n = int(fp.sum())
    rank = _rank(kind, n)
    rc, got, bands = _call(ops, a, fp, rank, MODE[mode], cval_bits)
    want = FO.rank_filter(a, rank, fp, mode, _cval_of(cval_bits, dt))
    assert rc == 0 and bands, (dt, name, kind, mode)
    assert np.array_equal(FO.bits(got), FO.bits(want)), (a.shape, dt, name, kind, mode, rank, int(np.count_nonzero(FO.bits(got) != FO.bits(want))))


def _combos():
    return [(dt, f, mode, kind) for dt in CODES for f in range(len(FOOTPRINTS)) for mode in FO.MODES for kind in RANK_KINDS]


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes_take_the_full_product(shape):
    """all seven dtypes x every footprint x all three modes x the five ranks, on extents below the radius"""
    ops = Ops()
    vols = {dt: _volume(shape, dt, 7 + sum(shape)) for dt in CODES}
    for i, (dt, f, mode, kind) in enumerate(_combos()):
        _check(ops, vols[dt], *FOOTPRINTS[f], kind, mode, _cval_bits(dt, i))


@pytest.mark.parametrize("shape", LARGE)
def test_larger_shapes_walk_the_product(shape):
    """the product is walked with a stride that still meets every value of every factor"""
    ops = Ops()
    combos = _combos()[(shape[0] % 13)::13]
    assert {c[0] for c in combos} == set(CODES) and {c[1] for c in combos} == set(range(len(FOOTPRINTS))) and {c[2] for c in combos} == set(FO.MODES)
    assert {c[3] for c in combos} == set(RANK_KINDS)
    assert {(c[0], c[3]) for c in combos} >= {(dt, "median") for dt in ("u1", "i2", "f4")}          # a bisection at every key width
    vols = {dt: _volume(shape, dt, 11 + sum(shape)) for dt in CODES}
    for i, (dt, f, mode, kind) in enumerate(combos):
        _check(ops, vols[dt], *FOOTPRINTS[f], kind, mode, _cval_bits(dt, i))


def test_int16_spans_its_full_range_and_float32_holds_the_specials():
    a = _volume((33, 9, 17), "i2", 1)
    assert a.min() == -32768 and a.max() == 32767
    f = _volume((33, 9, 17), "f4", 1)
    u = f.view(np.uint32)
    assert np.isnan(f).any() and ((u >> 31 == 1) & np.isnan(f)).any() and ((u >> 31 == 0) & np.isnan(f)).any()
    assert (u == 0x80000000).any() and (u == 0).any() and np.isposinf(f).any() and np.isneginf(f).any()
    b = _volume((33, 9, 17), "u1", 1)
    ops = Ops()
    picked = (FOOTPRINTS[0], FOOTPRINTS[2], FOOTPRINTS[5], FOOTPRINTS[8])
    assert [int(fp.sum()) for _, fp in picked] == [7, 27, 125, 64]   # registers (8), registers (27), the staged brick twice: every selection at every key width
    for name, fp in picked:
        for kind in RANK_KINDS:
            for mode in FO.MODES:
                _check(ops, a, name, fp, kind, mode, 0x8000)         # the constant is -32768
                _check(ops, f, name, fp, kind, mode, 0xFFC00000)     # the constant is a NaN with the sign bit: the lowest key
                _check(ops, b, name, fp, kind, mode, 0xFF)


@pytest.mark.parametrize("dt", ["i2", "u1", "f4"])
def test_two_runs_give_the_same_bits_and_a_source_offset_by_one_element(dt):
    """src starts one element into its buffer (2-byte alignment for int16); the kernel runs twice"""
    ops = Ops()
    a = _volume((65, 9, 10), dt, 5)
    for name, fp in (FOOTPRINTS[0], FOOTPRINTS[5]):
        n = int(fp.sum())
        for mode in FO.MODES:
            rc1, g1, b1 = _call(ops, a, fp, n // 2, MODE[mode], 0, src_offset=1)
            rc2, g2, b2 = _call(ops, a, fp, n // 2, MODE[mode], 0, src_offset=1)
            assert rc1 == rc2 == 0 and b1 and b2 and np.array_equal(FO.bits(g1), FO.bits(g2))
            assert np.array_equal(FO.bits(g1), FO.bits(FO.rank_filter(a, n // 2, fp, mode, _cval_of(0, dt)))), (name, mode)


# ---- later trips of the persistent workgroups ------------------------------------------------------------------------------------------------------------------------
def _grid_cap():
    from covidseg_amd import _lib
    import later_trips as LT
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "kernels_filter.hip")).read()
    cap = LT.constant_value(re.search(r"constexpr long long GRID_CAP = ([^;]+);", src).group(1))
    brick = tuple(int(v) for v in re.search(r"constexpr int BX = (\d+), BY = (\d+), BZ = (\d+),", src).groups())
    return cap, brick


def test_every_workgroup_takes_more_than_two_bricks():
    """an int16 volume of more than twice as many bricks as the launch has workgroups, plus a ragged remainder: 2 x 2 bricks a slab (the second of each pair one voxel
    wide), the last slab 3 voxels deep.  The cross-7 median, the box-27 maximum and the box-27 median (outside reads 0); the later bricks' results are not constant."""
    cap, (BX, BY, BZ) = _grid_cap()
    assert (BX, BY, BZ) == (32, 8, 8)
    slabs = -(-(2 * cap + cap // 16 + 3) // 4)
    shape = (BX + 1, BY + 1, BZ * (slabs - 1) + 3)
    nbricks = 2 * 2 * slabs
    assert nbricks > 2 * cap and nbricks % cap != 0 and np.prod(shape) < 2 ** 23
    rng = np.random.default_rng(cap)
    a = np.asfortranarray(rng.integers(-1200, 600, shape, dtype=np.int16))
    x, y, z = np.indices(shape, dtype=np.int32)
    trip = ((x // BX) + 2 * ((y // BY) + 2 * (z // BZ))) // cap
    assert trip.max() == 2 and (trip == 2).any()
    ops = Ops()
    for fp, rank, mode in ((FO.structure(1), 3, "reflect"), (FO.structure(3), 26, "nearest"), (FO.structure(3), 13, "constant")):          # the three instances at R = 1
        rc, got, bands = _call(ops, a, fp, rank, MODE[mode])
        want = FO.rank_filter(a, rank, fp, mode)
        assert rc == 0 and bands and np.array_equal(got, want)
        for t in (1, 2):                                             # the content rule of later_trips.py: what a later trip writes carries information
            later = want[trip == t]
            assert later.size > 0 and np.unique(later).size > 16 and (later != later[0]).mean() > 0.5


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_dst_untouched():
    ops = Ops()
    lib, h, s = ops.lib, ops.h, ops.s
    X, Y, Z = 9, 5, 4
    N = X * Y * Z
    src = torch.zeros(4 * N + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((4 * N + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    sp, dp = src.data_ptr(), dst.data_ptr() + BAND
    box, full = 2 ** 27 - 1, (2 ** 64 - 1, 2 ** 61 - 1)
    ok = dict(src=sp, dtype=4, X=X, Y=Y, Z=Z, R=1, lo=box, hi=0, rank=13, mode=2, cval=0, dst=dp)

    def call(**kw):
        a = {**ok, **kw}
        rc = lib.unet_vol_rank_filter(h, a["src"], a["dtype"], a["X"], a["Y"], a["Z"], a["R"], a["lo"], a["hi"], a["rank"], a["mode"], a["cval"], a["dst"], s)
        torch.cuda.synchronize()
        return rc

    bad = [dict(src=None), dict(dst=None), dict(src=sp + 1), dict(dst=dp + 1), dict(dtype=16, src=sp + 2), dict(dtype=8, dst=dp + 2),
           dict(dst=sp), dict(dst=sp + 2 * N - 2), dict(src=dp + 2 * N - 2), dict(dst=sp + 2),
           dict(X=-1), dict(Y=-1), dict(Z=-1), dict(X=2048, Y=2048, Z=512), dict(X=65536, Y=65536, Z=0),
           dict(dtype=64), dict(dtype=3), dict(dtype=0), dict(dtype=1024),
           dict(R=0), dict(R=3), dict(R=-1),
           dict(lo=0), dict(lo=box | (1 << 27)), dict(lo=1, hi=1), dict(R=2, lo=0, hi=0), dict(R=2, lo=1, hi=1 << 61), dict(R=2, lo=full[0], hi=full[1] | (1 << 63), rank=0),
           dict(rank=-1), dict(rank=27), dict(lo=0b101, rank=2), dict(R=2, lo=full[0], hi=full[1], rank=125),
           dict(mode=3), dict(mode=-1),
           dict(mode=1, cval=0x10000), dict(mode=0, cval=0x10000), dict(dtype=2, mode=1, cval=0x100), dict(dtype=16, mode=1, cval=2 ** 32), dict(mode=1, cval=2 ** 63)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.unet_last_error(h), kw
    assert (dst.cpu().numpy() == SENTINEL).all()
    for kw in (dict(X=0), dict(Y=0), dict(Z=0), dict(X=0, src=None, dst=None)):          # a zero dimension touches nothing
        assert call(**kw) == 0, kw
    assert (dst.cpu().numpy() == SENTINEL).all()
    assert call() == 0 and call(R=2, lo=full[0], hi=full[1], rank=0, mode=1, cval=0xFFFF) == 0          # the accepted twins of the refusals above
    host = dst.cpu().numpy()          # the minimum of zeros and the constant -1, which every voxel of 9 x 5 x 4 meets under the 5-box
    assert (host[:BAND] == SENTINEL).all() and (host[BAND + 2 * N:] == SENTINEL).all() and (host[BAND:BAND + 2 * N] == 0xFF).all()


# ---- through filters.* ------------------------------------------------------------------------------------------------------------------------------------------------
ASYM = np.zeros((3, 3, 3), bool)
ASYM[1, 1, 1] = ASYM[2, 1, 1] = ASYM[1, 0, 2] = ASYM[0, 0, 1] = True


@pytest.mark.parametrize("shape", [(33, 9, 17), (65, 5, 3)])
def test_every_public_function_against_the_oracle(shape):
    from covidseg_amd import filters as F
    for dt in ("i2", "u2", "f4"):
        a = _volume(shape, dt, 21)
        eq = lambda got, want: np.array_equal(FO.bits(got.data), FO.bits(want)) and got.data.dtype == a.dtype and got.data.flags.f_contiguous and got.shape == shape
        assert eq(F.rank_filter(a, 5), FO.rank_filter(a, 5, np.ones((3, 3, 3), bool)))                      # the default: a 3-box, reflect
        assert eq(F.rank_filter(a, 2, footprint=ASYM, mode="nearest"), FO.rank_filter(a, 2, ASYM, "nearest"))
        assert eq(F.median_filter(a), FO.rank_filter(a, 13, np.ones((3, 3, 3), bool)))
        assert eq(F.median_filter(a, connectivity=1), FO.rank_filter(a, 3, FO.structure(1)))
        assert eq(F.median_filter(a, connectivity=2, per_slice=True), FO.rank_filter(a, 4, FO.structure(2, True)))
        assert eq(F.median_filter(a, size=5, mode="nearest"), FO.rank_filter(a, 62, np.ones((5, 5, 5), bool), "nearest"))
        assert eq(F.median_filter(a, size=(5, 3, 1)), FO.rank_filter(a, 7, np.ones((5, 3, 1), bool)))
        assert eq(F.minimum_filter(a, size=5), FO.rank_filter(a, 0, np.ones((5, 5, 5), bool)))
        assert eq(F.maximum_filter(a, footprint=ASYM), FO.rank_filter(a, 3, ASYM))
        assert eq(F.percentile_filter(a, 25, connectivity=2), FO.rank_filter(a, FO.percentile_rank(25, 19), FO.structure(2)))
        assert eq(F.percentile_filter(a, -10, size=5), FO.rank_filter(a, FO.percentile_rank(-10, 125), np.ones((5, 5, 5), bool)))
        cmin = a[~np.isnan(a)].min() if dt == "f4" else a.min()
        assert eq(F.median_filter(a, mode="constant"), FO.rank_filter(a, 13, np.ones((3, 3, 3), bool), "constant", cmin))          # the default constant: the minimum
        c = {"i2": -1000, "u2": 65535, "f4": -0.0}[dt]
        for mode in FO.MODES:
            kw = dict(footprint=ASYM, mode=mode, cval=c)
            assert eq(F.grey_erosion(a, **kw), FO.grey_erosion(a, ASYM, mode, c))
            assert eq(F.grey_dilation(a, **kw), FO.grey_dilation(a, ASYM, mode, c))
            assert eq(F.grey_opening(a, **kw), FO.grey_opening(a, ASYM, mode, c))
            assert eq(F.grey_closing(a, **kw), FO.grey_closing(a, ASYM, mode, c))
        assert not np.array_equal(F.grey_dilation(a, footprint=ASYM).data, F.maximum_filter(a, footprint=ASYM).data)          # the mirrored footprint is another one
        r = F.median_filter(a)
        with np.errstate(invalid="ignore"):                          # (a signalling NaN raises the flag when it is widened)
            assert (r.slope, r.inter) == (0.0, 0.0) and np.array_equal(r.decoded(), r.data.astype(np.float64), equal_nan=True)


def test_a_device_tensor_source_and_a_device_result():
    from covidseg_amd import filters as F
    shape = (33, 9, 17)
    for dt, tdt in (("i2", torch.int16), ("f4", torch.float32), ("u1", torch.uint8)):
        a = _volume(shape, dt, 31)
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(-1, order="F"))).cuda()
        before = t.clone()
        r = F.grey_closing(t, footprint=ASYM, mode="nearest", return_device=True, src_shape=shape)
        assert isinstance(r.data, torch.Tensor) and r.data.is_cuda and r.data.dtype == tdt and r.data.numel() == a.size and r.shape == shape
        want = FO.grey_closing(a, ASYM, "nearest")
        assert np.array_equal(FO.bits(r.data.cpu().numpy().reshape(shape, order="F")), FO.bits(want)) and torch.equal(t.view(torch.uint8), before.view(torch.uint8))
        with np.errstate(invalid="ignore"):                          # (a signalling NaN raises the flag when it is widened)
            assert np.array_equal(r.decoded(), want.astype(np.float64), equal_nan=True)
        m =F.median_filter(t, src_shape=shape, mode="constant")     # the default constant of a device tensor: its minimum, NaNs aside
        cmin = a[~np.isnan(a)].min() if dt == "f4" else a.min()
        assert np.array_equal(FO.bits(m.data), FO.bits(FO.rank_filter(a, 13, np.ones((3, 3, 3), bool), "constant", cmin)))


def test_a_scaled_volume_with_a_negative_slope_is_ranked_in_decoded_order():
    from covidseg_amd import filters as F
    from covidseg_amd import nifti_min
    shape = (33, 9, 17)
    raw = np.asfortranarray(np.random.default_rng(9).integers(-1200, 600, shape, dtype=np.int16))
    vol = nifti_min.NiftiVolume(raw, -0.5, 100.0, (1.0, 1.0, 1.0), nifti_min.default_header(shape), "<")
    fp = FO.random_footprint(2, 30, 77)
    for rank in (0, 4, 15, 29):
        r = F.rank_filter(vol, rank, footprint=fp, mode="nearest")
        stored = -FO.rank_filter(np.asfortranarray(-raw), rank, fp, "nearest")          # decoded order is the order of -raw
        assert r.data.dtype == np.int16 and (r.slope, r.inter) == (-0.5, 100.0) and np.array_equal(r.data, stored)
        assert np.array_equal(r.decoded(), stored.astype(np.float64) * -0.5 + 100.0)
    ero = F.grey_erosion(vol, connectivity=1, mode="constant")       # decoded minimum = stored maximum; the default constant decodes to the minimum: the stored maximum
    assert np.array_equal(ero.data, FO.rank_filter(raw, 6, FO.structure(1), "constant", raw.max()))
    assert ero.decoded().min() == vol.get_fdata().min()


def test_gaussian_filter_is_bit_equal_to_its_oracle():
    from covidseg_amd import filters as F
    from covidseg_amd import nifti_min
    for shape in ((65, 5, 3), (33, 9, 17)):
        raw = np.asfortranarray(np.random.default_rng(12).integers(-1024, 400, shape, dtype=np.int16))
        a32 = raw.astype(np.float32)
        for sigma in (1.0, (1.0, 0.0, 1.5), (0.0, 0.0, 0.0), (0.4, 2.0, 0.0)):          # an axis with sigma = 0 is skipped
            got = F.gaussian_filter(raw, sigma=sigma)
            want = FO.gaussian_filter(a32, np.broadcast_to(np.asarray(sigma, np.float64), (3,)))
            assert got.dtype == np.float32 and got.shape == shape and got.flags.f_contiguous and np.array_equal(FO.bits(got), FO.bits(want)), (shape, sigma)
    pix = (0.75, 0.75, 2.5)
    vol = nifti_min.NiftiVolume(raw, 0.5, -100.25, pix, nifti_min.default_header(shape, pix), "<")
    dec32 = vol.get_fdata().astype(np.float32)
    want = FO.gaussian_filter(dec32, tuple(1.5 / p for p in pix))
    assert np.array_equal(FO.bits(F.gaussian_filter(vol, sigma_mm=1.5)), FO.bits(want))                      # an anisotropic sigma_mm: the file's own pixdim
    assert np.array_equal(FO.bits(F.gaussian_filter(dec32, sigma_mm=1.5, pixdim=pix)), FO.bits(want))
    t = torch.from_numpy(np.ascontiguousarray(raw.reshape(-1, order="F"))).cuda()
    dev = F.gaussian_filter(t, sigma=(1.0, 0.0, 1.5), return_device=True, src_shape=shape)
    assert dev.is_cuda and dev.dtype == torch.float32 and dev.numel() == raw.size
    assert np.array_equal(FO.bits(dev.cpu().numpy().reshape(shape, order="F")), FO.bits(FO.gaussian_filter(a32, (1.0, 0.0, 1.5))))
    same = F.gaussian_filter(t, sigma=0.0, return_device=True, src_shape=shape)
    assert same.data_ptr() != t.data_ptr() and torch.equal(same, t.to(torch.float32))

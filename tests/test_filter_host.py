"""CPU: tests/filter_oracle.py against scipy.ndimage (rank, percentile, flat grey morphology, the Gaussian), the float32 key order, footprint words, the rank mirror
of a negative slope, the new entry's declaration and binding, the exports, and every argument error of filters.*, which must be raised before a device is needed."""
import math
import os
import re

import numpy as np
import pytest

import filter_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 1, 3), (1, 5, 2), (3, 2, 2), (7, 6, 5), (33, 9, 8)]          # extents below R (reflect wraps more than once) up to two bricks along x
CVAL = {"i2": -7, "u1": 7, "f4": -7.5}


def _volume(shape, dt, rng):
    if dt == "i2":
        return rng.integers(-1200, 600, shape).astype(np.int16)
    if dt == "u1":
        return rng.integers(0, 256, shape).astype(np.uint8)
    return (rng.standard_normal(shape) * 300).astype(np.float32)


# ---- the oracle against scipy ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_the_oracle_equals_scipys_rank_filter(shape):
    """int16, uint8 and float32 without NaN; R 1 and 2; random footprints at three densities; all three modes; ranks 0, n // 2, n - 1.  By value (np.array_equal):
    scipy orders +-0 differently."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(sum(shape))
    cases = 0
    for dt in ("i2", "u1", "f4"):
        a = _volume(shape, dt, rng)
        for R in (1, 2):
            for di, density in enumerate((0.1, 0.5, 0.9)):
                n = max(1, int(round(density * (2 * R + 1) ** 3)))
                fp = FO.random_footprint(R, n, 100 * R + di)
                for mode in FO.MODES:
                    for rank in sorted({0, n // 2, n - 1}):
                        want = ndi.rank_filter(a, rank, footprint=fp, mode=mode, cval=CVAL[dt])
                        got = FO.rank_filter(a, rank, fp, mode, CVAL[dt])
                        assert got.dtype == want.dtype and np.array_equal(got, want), (dt, R, n, mode, rank)
                        cases += 1
    assert cases == 3 * 2 * 3 * 3 * 3


def test_percentile_ranks_are_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    from covidseg_amd import filters as F
    rng = np.random.default_rng(3)
    a = _volume((9, 8, 7), "i2", rng)
    for R, n in ((1, 7), (2, 37), (2, 125), (1, 1)):
        fp = FO.random_footprint(R, n, n)
        for p in (-100, -50, -1, -0.5, 0, 1, 33.3, 50, 50.0, 99, 99.9, 100, np.float64(25), np.int64(75)):
            rank = F.percentile_rank(p, n)
            assert rank == FO.percentile_rank(p, n) and 0 <= rank < n
            assert np.array_equal(ndi.percentile_filter(a, p, footprint=fp), FO.rank_filter(a, rank, fp)), (n, p)
    for bad in (101, -100.5, "50", True, None, float("nan")):
        with pytest.raises(ValueError):
            F.percentile_rank(bad, 27)


def test_grey_morphology_is_scipys_and_dilation_mirrors_the_footprint():
    ndi = pytest.importorskip("scipy.ndimage")
    from covidseg_amd import filters as F
    rng = np.random.default_rng(4)
    a = _volume((9, 8, 7), "i2", rng)
    asym = np.zeros((3, 3, 3), bool)
    asym[1, 1, 1] = asym[2, 1, 1] = asym[1, 0, 2] = True
    assert np.array_equal(F._mirrored(asym), FO.mirrored(asym)) and not np.array_equal(F._mirrored(asym), asym)
    for fp in (asym, FO.random_footprint(2, 40, 9), FO.structure(1)):
        n = int(fp.sum())
        for mode in FO.MODES:
            dil = ndi.grey_dilation(a, footprint=fp, mode=mode, cval=-5)
            assert np.array_equal(dil, FO.grey_dilation(a, fp, mode, -5))
            assert np.array_equal(dil, ndi.maximum_filter(a, footprint=FO.mirrored(fp), mode=mode, cval=-5))
            if not np.array_equal(FO.mirrored(fp), fp):
                assert not np.array_equal(dil, FO.rank_filter(a, n - 1, fp, mode, -5))          # the unmirrored maximum is another volume
            assert np.array_equal(ndi.grey_erosion(a, footprint=fp, mode=mode, cval=-5), FO.grey_erosion(a, fp, mode, -5))
            assert np.array_equal(ndi.grey_opening(a, footprint=fp, mode=mode, cval=-5), FO.grey_opening(a, fp, mode, -5))
            assert np.array_equal(ndi.grey_closing(a, footprint=fp, mode=mode, cval=-5), FO.grey_closing(a, fp, mode, -5))


def test_structures_are_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    from covidseg_amd import filters as F
    for c, n, planar in ((1, 7, 5), (2, 19, 9), (3, 27, 9)):
        want = ndi.generate_binary_structure(3, c)
        assert np.array_equal(F.structure(c), want) and np.array_equal(FO.structure(c), want) and F.structure(c).sum() == n
        p = F.structure(c, per_slice=True)
        assert p.sum() == planar and not p[:, :, 0].any() and not p[:, :, 2].any() and np.array_equal(p[:, :, 1], want[:, :, 1]) and np.array_equal(p, FO.structure(c, True))
    for bad in (0, 4, 1.0, True, "1", None):
        with pytest.raises(ValueError):
            F.structure(bad)
    with pytest.raises(ValueError):
        F.structure(1, per_slice=1)


# ---- the order of float32 -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_float_key_orders_nan_zero_and_inf():
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    pos_nan = np.array([0x7FC00001], np.uint32).view(np.float32)[0]
    vals = np.array([neg_nan, -np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf, pos_nan], np.float32)
    k = FO.key32(vals)
    assert (np.diff(k.astype(np.int64)) > 0).all()                   # strictly ascending: -nan < -inf < .. < -0 < +0 < .. < +inf < nan
    assert np.array_equal(FO.unkey32(k).view(np.uint32), vals.view(np.uint32))
    # a line of these values under a 3-voxel footprint along x, every rank: the sorted window, bit for bit
    a = np.asfortranarray(vals[[5, 9, 4, 0, 8, 1, 2, 7]].reshape(8, 1, 1))
    fp = np.zeros((3, 3, 3), bool)
    fp[:, 1, 1] = True
    pad = np.concatenate([a[:1, 0, 0], a[:, 0, 0], a[-1:, 0, 0]])    # nearest
    for rank in range(3):
        got = FO.rank_filter(a, rank, fp, "nearest")
        want = np.array([sorted(pad[i:i + 3], key=lambda v: int(FO.key32(np.array([v]))[0]))[rank] for i in range(8)], np.float32)
        assert np.array_equal(FO.bits(got).reshape(-1), want.view(np.uint32))
    assert FO.bits(FO.rank_filter(a, 0, fp, "nearest"))[3, 0, 0] == 0xFFC00000 and FO.bits(FO.rank_filter(a, 2, fp, "nearest"))[1, 0, 0] == 0x7FC00001
    assert FO.bits(FO.rank_filter(a, 0, fp, "nearest"))[1, 0, 0] == 0x80000000          # -0 is below +0


# ---- footprints -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_footprint_bits_round_trip_and_refusals():
    from covidseg_amd import filters as F
    for R, n, seed in ((1, 1, 0), (1, 13, 1), (1, 27, 2), (2, 1, 3), (2, 64, 4), (2, 124, 5), (2, 125, 6)):
        fp = FO.random_footprint(R, n, seed)
        if R == 2:
            fp[0, 0, 0] = True                                       # keep the extent at 5
            n = int(fp.sum())
        r, lo, hi = F.footprint_bits(fp)
        assert r == R and bin(lo).count("1") + bin(hi).count("1") == n and 0 <= lo < 2 ** 64 and 0 <= hi < 2 ** 61 and (R == 2 or (hi == 0 and lo < 2 ** 27))
        assert np.array_equal(F.footprint_of_bits(r, lo, hi), fp)
        for (dx, dy, dz) in FO.offsets(fp):
            b = (dx + R) + (2 * R + 1) * ((dy + R) + (2 * R + 1) * (dz + R))
            assert ((lo | (hi << 64)) >> b) & 1
    assert F.footprint_bits(np.ones((3, 3, 3), bool)) == (1, 2 ** 27 - 1, 0) and F.footprint_bits(np.ones((5, 5, 5), bool)) == (2, 2 ** 64 - 1, 2 ** 61 - 1)
    assert F.footprint_bits(np.ones((1, 1, 1), bool)) == (1, 1 << 13, 0)          # the centre of the 3-cube
    r, lo, hi = F.footprint_bits(np.ones((5, 1, 3), bool))             # embedded centrally
    cube = F.footprint_of_bits(r, lo, hi)
    assert r == 2 and cube.sum() == 15 and cube[:, 2, 1:4].all()
    for bad in (np.ones((2, 3, 3), bool), np.ones((3, 3, 4), bool), np.ones((7, 3, 3), bool), np.ones((3, 3), bool), np.zeros((3, 3, 3), bool), np.ones((3, 3, 3), np.float32)):
        with pytest.raises(ValueError):
            F.footprint_bits(bad)
    for bad in ((0, 1, 0), (3, 1, 0), (1, 1 << 27, 0), (1, 1, 1), (2, 0, 1 << 61)):
        with pytest.raises(ValueError):
            F.footprint_of_bits(*bad)


# ---- a negative slope ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_negative_slope_mirrors_the_rank():
    from covidseg_amd import filters as F
    from covidseg_amd import nifti_min, volume as V
    rng = np.random.default_rng(6)
    raw = np.asfortranarray(rng.integers(-1200, 600, (7, 6, 5)).astype(np.int16))
    fp = FO.random_footprint(2, 20, 8)
    n = 20
    hdr = nifti_min.default_header(raw.shape)
    neg = V._resample_source(nifti_min.NiftiVolume(raw, -0.5, 10.0, (1.0, 1.0, 1.0), hdr, "<"))
    pos = V._resample_source(nifti_min.NiftiVolume(raw, 0.5, 10.0, (1.0, 1.0, 1.0), hdr, "<"))
    plain = V._resample_source(raw)
    for rank in (0, 1, 7, 10, 18, 19):
        assert F.launch_rank(rank, n, neg) == n - 1 - rank and F.launch_rank(rank, n, pos) == rank and F.launch_rank(rank, n, plain) == rank
        # the decoded volume -0.5 v + 10 is ordered as -v: the stored element of stored rank n - 1 - rank decodes to the value of decoded rank `rank`
        decoded_order = FO.rank_filter(np.asfortranarray(-raw), rank, fp)
        assert np.array_equal(-FO.rank_filter(raw, F.launch_rank(rank, n, neg), fp), decoded_order)


# ---- declarations, bindings, exports ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_bound_and_built():
    import covidseg_amd
    from covidseg_amd import _lib, filters as F
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    m = re.search(r"int32_t\s+unet_vol_rank_filter\s*\(([^;{]*?)\)\s*;", hdr)
    assert m and m.group(1).count(",") + 1 == 14
    assert "uint64_t fp_lo, uint64_t fp_hi, int32_t rank" in m.group(1) and "uint64_t cval_bits" in m.group(1)
    proto = _lib._PROTOS["unet_vol_rank_filter"]
    assert proto[0] is _lib.i32 and len(proto[1]) == 14 and proto[1][7] is _lib.u64 and proto[1][8] is _lib.u64 and proto[1][11] is _lib.u64
    assert "unet_vol_rank_filter" in _lib.EXPORTED_SYMBOLS and _lib.ABI_VERSION == 16 and re.search(r"#define UNET_ABI_VERSION 16\b", text)
    assert re.search(r"#define UNET_VOL_RANK_MAX_RADIUS 2\b", text) and _lib.RANK_MAX_RADIUS == 2 == F.MAX_RADIUS
    assert re.search(r"enum \{ UNET_FILTER_NEAREST = 0, UNET_FILTER_CONSTANT = 1, UNET_FILTER_REFLECT = 2 \};", text)
    assert _lib.FILTER_MODES == {"nearest": 0, "constant": 1, "reflect": 2} and F.MODES is _lib.FILTER_MODES
    assert "DESIGN.md section 4ad" in text
    mk = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    first = [line for line in mk.splitlines() if line.startswith("SRCS =")]
    assert len(first) == 1 and re.search(r"\bkernels_filter\.hip\b", first[0])
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "kernels_filter.hip")).read()
    assert re.search(r"constexpr long long GRID_CAP = ([^;]+);", src) and "atomic" not in src.split("#include")[1]          # a bounded grid with its cap stated; no atomics
    names = ("rank_filter", "median_filter", "minimum_filter", "maximum_filter", "percentile_filter", "grey_erosion", "grey_dilation", "grey_opening", "grey_closing",
             "gaussian_filter", "footprint_bits", "structure", "FilteredVolume")
    for name in names:
        assert getattr(covidseg_amd, name) is getattr(F, name) and name in covidseg_amd.__all__
    assert "filters" in covidseg_amd.__all__
    assert "spacing=" in F.gaussian_filter.__doc__ and "resample_volume(" in F.gaussian_filter.__doc__ and "return_device=True" in F.gaussian_filter.__doc__
    import inspect
    from covidseg_amd import volume as V
    assert "antialias" not in inspect.signature(V.resample_volume).parameters


# ---- every argument error comes before a device is needed ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from covidseg_amd import volume as V

    def boom(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(V, "_ctx", boom)
    monkeypatch.setattr(V, "upload", boom)
    monkeypatch.setattr(V, "smooth_axis_device", boom)
    return V


RANKED = ("median_filter", "minimum_filter", "maximum_filter", "grey_erosion", "grey_dilation", "grey_opening", "grey_closing")


def test_the_rank_filters_refuse_their_arguments_before_any_device_work(no_device):
    from covidseg_amd import filters as F
    ct = np.zeros((4, 4, 4), np.int16)
    off_plane = np.zeros((3, 3, 3), bool)
    off_plane[1, 1, 0] = off_plane[0, 2, 2] = True                   # no voxel in the plane dz = 0
    common = (dict(size=2), dict(size=7), dict(size=0), dict(size=(3, 3)), dict(size=(3, 3, 4)), dict(size=3.0), dict(size=True), dict(size=3, connectivity=1),
              dict(footprint=np.ones((3, 3, 3), bool), connectivity=1), dict(footprint=np.ones((3, 3, 3), bool), size=3), dict(footprint=np.ones((2, 3, 3), bool)),
              dict(footprint=np.ones((7, 7, 7), bool)), dict(footprint=np.zeros((3, 3, 3), bool)), dict(footprint=np.ones((3, 3), bool)), dict(connectivity=0),
              dict(connectivity=4), dict(connectivity=1.0), dict(per_slice=1), dict(footprint=off_plane, per_slice=True),
              dict(mode="mirror"), dict(mode="wrap"), dict(mode=2), dict(mode="constant", cval=1.5), dict(mode="constant", cval=40000), dict(mode="constant", cval="0"),
              dict(mode="constant", cval=True), dict(cval=float("nan")), dict(cval=-32769), dict(return_device=1), dict(src_shape=(4, 4, 4)))
    for name in RANKED:
        for bad in common:
            with pytest.raises(ValueError):
                getattr(F, name)(ct, **bad)
    for bad in common:
        with pytest.raises(ValueError):
            F.rank_filter(ct, 0, **bad)
        with pytest.raises(ValueError):
            F.percentile_filter(ct, 50, **bad)
    for rank, kw in ((-1, {}), (27, {}), (7, dict(connectivity=1)), (5, dict(connectivity=1, per_slice=True)), (1.0, {}), (True, {}), ("0", {}), (1, dict(size=1))):
        with pytest.raises(ValueError, match="rank"):
            F.rank_filter(ct, rank, **kw)
    for p in (101, -101, "50", None):
        with pytest.raises(ValueError, match="percentile"):
            F.percentile_filter(ct, p)
    for name in RANKED + ("gaussian_filter",):
        kw = dict(sigma=1.0) if name == "gaussian_filter" else {}
        with pytest.raises(ValueError, match="float32"):
            getattr(F, name)(np.zeros((4, 4, 4), np.float64), **kw)
        with pytest.raises(ValueError, match="float32"):
            getattr(F, name)(np.zeros((4, 4, 4), np.int64), **kw)      # (taken as float64, like every bare array of another dtype)
        with pytest.raises(ValueError):
            getattr(F, name)(np.zeros((4, 4), np.int16), **kw)
    with pytest.raises(ValueError, match="stored dtype"):
        F.median_filter(np.zeros((4, 4, 4), np.uint8), mode="constant", cval=-1)
    with pytest.raises(ValueError, match="stored dtype"):
        F.median_filter(np.zeros((4, 4, 4), np.float32), mode="constant", cval=0.1)          # not a float32
    assert F._check_cval(0.5, np.dtype(np.float32)) == np.float32(0.5) and math.isnan(F._check_cval(float("nan"), np.dtype(np.float32)))
    assert F._check_cval(-32768, np.dtype(np.int16)) == -32768 and F._check_cval(np.int64(255), np.dtype(np.uint8)).dtype == np.uint8


def test_gaussian_filter_refuses_its_arguments_before_any_device_work(no_device):
    from covidseg_amd import filters as F
    from covidseg_amd import nifti_min
    ct = np.zeros((4, 4, 4), np.int16)
    for bad in (dict(), dict(sigma=1.0, sigma_mm=1.0), dict(sigma=-1.0), dict(sigma=(1.0, 1.0)), dict(sigma=(1.0, 1.0, 1.0, 1.0)), dict(sigma="1"), dict(sigma=float("inf")),
                dict(sigma=float("nan")), dict(sigma=True), dict(sigma=11.0), dict(sigma_mm=1.0), dict(sigma_mm=1.0, pixdim=(1.0, 0.0, 1.0)), dict(sigma_mm=1.0, pixdim=(1.0, 1.0)),
                dict(sigma_mm=40.0, pixdim=(1.0, 1.0, 1.0)), dict(sigma=1.0, return_device=1), dict(sigma=1.0, src_shape=(4, 4, 4))):
        with pytest.raises(ValueError):
            F.gaussian_filter(ct, **bad)
    # a NiftiVolume carries its pixdim: sigma_mm passes the checks and only then asks for the device
    vol = nifti_min.NiftiVolume(np.asfortranarray(ct), 0.0, 0.0, (0.7, 0.7, 2.5), nifti_min.default_header(ct.shape, (0.7, 0.7, 2.5)), "<")
    with pytest.raises((AssertionError, RuntimeError, ImportError)):
        F.gaussian_filter(vol, sigma_mm=1.0)
    assert F._check_sigma(None, 2.0, (0.5, 1.0, 4.0)) == (4.0, 2.0, 0.5) and F._check_sigma((1, 0, 2.5), None, None) == (1.0, 0.0, 2.5)


# ---- the Gaussian against scipy -----------------------------------------------------------------------------------------------------------------------------------
GAUSS_SHAPE, GAUSS_SIGMA = (41, 30, 23), (1.0, 1.5, 0.7)
GAUSS_MEASURED = 0.0


def test_the_gaussian_oracle_against_scipy():
    """filter_oracle.gaussian_filter (the float64 sum of a pass in ascending tap order, rounded to float32 per pass, as unet_vol_smooth_axis) against
    scipy.ndimage.gaussian_filter(a32, sigma, mode="nearest", radius=ceil(3 sigma)) on a CT-ranged volume of -1024 .. 400.  scipy also sums a pass in float64 and rounds
    it to float32, but it adds the symmetric taps in pairs.  Measured on the CPU, oracle against scipy 1.15.3, never the device: the largest absolute difference on
    this case is GAUSS_MEASURED = 0.0 -- the two float64 sums differ by about 1e-13 relative and did not fall on different sides of a float32 rounding boundary
    anywhere.  The assertion is twice the measured value."""
    ndi = pytest.importorskip("scipy.ndimage")
    from covidseg_amd import volume as V
    a = np.random.default_rng(41).uniform(-1024.0, 400.0, GAUSS_SHAPE).astype(np.float32)
    got = FO.gaussian_filter(a, GAUSS_SIGMA)
    want = ndi.gaussian_filter(a, GAUSS_SIGMA, mode="nearest", radius=[int(np.ceil(3 * s)) for s in GAUSS_SIGMA])
    diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"gaussian oracle against scipy: largest absolute difference {diff!r}")
    assert got.dtype == np.float32 and diff <= 2.0 * GAUSS_MEASURED
    for s in GAUSS_SIGMA + (0.0, 3.3):
        w, wo = V.gaussian_weights(s), FO.gaussian_weights(s)
        assert (w is None and wo is None) or np.array_equal(w, wo)
    skipped = FO.gaussian_filter(a, (0.0, 1.5, 0.0))                  # an axis with sigma = 0 is skipped: one pass along y
    assert np.array_equal(skipped, ndi.gaussian_filter1d(a, 1.5, axis=1, mode="nearest", radius=5)) and np.array_equal(FO.gaussian_filter(a, (0, 0, 0)), a)

"""CPU: tests/texture_oracle.py against itself and against closed forms, texture.py's host features against the exact rational values, the argument refusals (all raised
before a device is needed), and the declarations of csrc/kernels_texture.hip's three entries.

The feature bound.  texture.glcm_features / run_features form every feature that is a ratio of integers from exact integers (int64 histograms, Python integers where a
product may pass 2^63) and divide once: Python's int / int is correctly rounded, so the error is at most 2^-53 |value|.  The others (energy, the two inverse differences,
the short-run and low-grey-level emphases) are float64 sums of m non-zero terms, each formed with at most three roundings (relative error <= 3 u, u = 2^-53), added by
numpy's pairwise sum (relative error of the sum of the absolute terms <= (m - 1) u to first order): |err| <= (m + 2) u sum |term|.  The oracle sums per matrix entry, the
host per histogram bin, so the oracle's m is never smaller.  The entropies are sum (S / T) (log2 T - log2 S) over integers S, that is log2 T - sum S log2 S / T:
besides the same summation error, a logarithm may be off by up to 2 ulp (numpy promises no correct rounding), which is 2 u of (S / T) log2 T and of (S / T) log2 S; summed
over the entries these are the terms log2 T and S log2 S / T.  The asserted bound is therefore (m + 8) u sum |term| + 2 u sum |log term| with the terms log2 T and
S log2 S / T for an entropy; the 6 u of slack cover the second-order terms and the oracle's own math.fsum of rounded products."""
import math
import os
import re

import numpy as np
import pytest

import texture_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd")


def _random_case(shape, n, Ng, seed):
    rng = np.random.default_rng(seed)
    val = rng.normal(-600.0, 300.0, shape).round()
    labels = rng.integers(-1, n + 2, shape)
    g = TO.group_of(shape, labels=labels, n=n)
    lev, lc = TO.quantize(val, g, n, -1000.0, 1000.0 / Ng, Ng, False)
    return val, labels, g, lev, lc


# ---- the oracle against itself ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 11, 9), (5, 1, 7), (1, 1, 1)])
def test_oracle_sums(shape):
    n, Ng = 3, 6
    val, labels, g, lev, lc = _random_case(shape, n, Ng, 7)
    assert np.array_equal(lc, np.stack([np.bincount(lev[g == k + 1], minlength=Ng + 1)[1:] for k in range(n)]))          # the first-order histogram
    for distance in (1, 2):
        C = TO.glcm(lev, g, n, Ng, distance, 0x1FFF)
        for kk, d in enumerate(TO.DIRECTIONS):                      # sum C[g][k] = the in-group pairs, counted one pair at a time
            pairs = np.zeros(n, np.int64)
            for x in range(shape[0]):
                for y in range(shape[1]):
                    for z in range(shape[2]):
                        qx, qy, qz = x + distance * d[0], y + distance * d[1], z + distance * d[2]
                        if 0 <= qx < shape[0] and 0 <= qy < shape[1] and 0 <= qz < shape[2] and lev[x, y, z] and lev[qx, qy, qz] and g[x, y, z] == g[qx, qy, qz]:
                            pairs[g[x, y, z] - 1] += 1
            assert np.array_equal(C[:, kk].sum(axis=(1, 2)), pairs), (distance, d)
        assert np.array_equal(TO.glcm(lev, g, n, Ng, distance, 0x1FFF, merge=True)[:, 0], C.sum(axis=1))
    R, clamped = TO.runs(lev, g, n, Ng, 0x1FFF, max(shape))
    assert not clamped.any()
    lengths = np.arange(1, max(shape) + 1)
    assert np.array_equal((R * lengths).sum(axis=(2, 3)), np.repeat(lc.sum(axis=1)[:, None], 13, axis=1))          # every taking-part voxel lies in one run per direction
    R2, c2 = TO.runs(lev, g, n, Ng, 0x1FFF, 2)                      # clamped: the last column takes the longer runs
    assert np.array_equal(R2[..., 0], R[..., 0]) and np.array_equal(R2[..., 1], R[..., 1:].sum(axis=-1)) and np.array_equal(c2, R[..., 2:].sum(axis=(2, 3)))


def test_quantize_edges_clip_and_drop():
    val = np.array([-np.inf, -1000.5, -1000.0, -975.0001, -975.0, -0.0, 0.0, 574.9, 575.0, 600.0, np.inf, np.nan]).reshape(12, 1, 1)
    g = np.ones((12, 1, 1), np.int64)
    clip, lc = TO.quantize(val, g, 1, -1000.0, 25.0, 63, False)
    assert clip.ravel().tolist() == [1, 1, 1, 1, 2, 41, 41, 63, 63, 63, 63, 0] and lc.sum() == 11
    drop, lc = TO.quantize(val, g, 1, -1000.0, 25.0, 63, True)
    assert drop.ravel().tolist() == [0, 0, 1, 1, 2, 41, 41, 63, 0, 0, 0, 0] and lc.sum() == 6
    zero, _ = TO.quantize(np.array([-0.0, 0.0, -1e-300]).reshape(3, 1, 1), g[:3], 1, 0.0, 1.0, 4, True)          # q = -0.0 is not below 0
    assert zero.ravel().tolist() == [1, 1, 0]


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------------------------
def test_checkerboard_and_constant_volume():
    from covidseg_amd import texture as T
    shape = (6, 5, 4)
    x, y, z = np.indices(shape)
    lev = np.where((x + y + z) % 2 == 0, 3, 8).astype(np.uint8)
    g = np.ones(shape, np.int64)
    C = TO.glcm(lev, g, 1, 8, 1, 1)
    assert C[0, 0].sum() == 5 * 5 * 4 and C[0, 0, 2, 7] + C[0, 0, 7, 2] == 100
    f = T.glcm_features(C)[0, 0]
    assert f["contrast"] == 25.0 and f["joint_energy"] == 0.5 and f["inverse_difference_moment"] == 1.0 / 26.0 and f["joint_entropy"] == 1.0
    lev[:] = 5
    C = TO.glcm(lev, g, 1, 8, 1, 0x1FFF)
    f = T.glcm_features(C)[0]
    assert (f["joint_energy"] == 1.0).all() and (f["contrast"] == 0.0).all() and (f["joint_entropy"] == 0.0).all() and (f["correlation"] == 1.0).all()
    R, clamped = TO.runs(lev, g, 1, 8, 1, 6)
    assert R[0, 0, 4].tolist() == [0, 0, 0, 0, 0, 20] and R.sum() == 20 and not clamped.any()
    rf = T.run_features(R, 120)[0, 0]
    assert rf["run_percentage"] == 1.0 / 6.0 and rf["long_run_emphasis"] == 36.0 and rf["run_entropy"] == 0.0 and rf["run_variance"] == 0.0
    assert abs(rf["short_run_emphasis"] - 1.0 / 36.0) <= 3 * 2.0 ** -53 / 36.0          # (c / j^2) / Nr: two roundings


# ---- the host features against the exact values ------------------------------------------------------------------------------------------------------------------
def _assert_features(got, exact, names, what):
    for f in names:
        if exact is None:
            assert math.isnan(got[f]), (what, f)
            continue
        want, bound = exact[f]
        if math.isnan(want):
            assert math.isnan(got[f]), (what, f)
        else:
            assert abs(float(got[f]) - want) <= bound, (what, f, float(got[f]), want, bound)


@pytest.mark.parametrize("Ng,scale", [(1, 5), (2, 3), (8, 40), (16, 2 ** 20), (64, 9)])
def test_glcm_features_within_the_summation_bound(Ng, scale):
    from covidseg_amd import texture as T
    rng = np.random.default_rng(Ng)
    C = rng.integers(0, scale, (3, 2, Ng, Ng))
    C[rng.random(C.shape) < 0.5] = 0
    C[1, 0] = 0                                                     # an empty matrix: NaN everywhere
    C[2, 1] = 0
    C[2, 1, Ng // 2, Ng // 2] = 7                                    # one level: the marginal's variance is 0, the correlation 1
    got = T.glcm_features(C)
    assert got.shape == (3, 2) and got.dtype == T.GLCM_FEATURE_DTYPE
    for i in np.ndindex(3, 2):
        _assert_features(got[i], TO.glcm_features_exact(C[i]), T.GLCM_FEATURES, (Ng, i))
    assert got[2, 1]["correlation"] == 1.0 and np.isnan(got[1, 0]["contrast"])
    one = T.glcm_features(C[2, 1])                                  # one matrix: a record
    assert one.shape == () and one["autocorrelation"] == got[2, 1]["autocorrelation"] == float((Ng // 2 + 1) ** 2)


def test_glcm_features_with_counts_beyond_2_to_the_31():
    from covidseg_amd import texture as T
    C = np.zeros((4, 4), np.int64)
    C[0, 3], C[1, 1], C[2, 3], C[3, 3] = 2 ** 33 + 1, 2 ** 35 + 3, 2 ** 31 + 5, 2 ** 34 + 7
    _assert_features(T.glcm_features(C), TO.glcm_features_exact(C), T.GLCM_FEATURES, "large counts")


@pytest.mark.parametrize("Ng,R,scale", [(1, 1, 5), (4, 7, 30), (64, 64, 3), (8, 300, 2 ** 25)])
def test_run_features_within_the_summation_bound(Ng, R, scale):
    from covidseg_amd import texture as T
    rng = np.random.default_rng(R)
    C = rng.integers(0, scale, (2, 3, Ng, R))
    C[rng.random(C.shape) < 0.6] = 0
    C[0, 1] = 0
    voxels = (C * np.arange(1, R + 1)).sum(axis=(2, 3)).max(axis=1)
    got = T.run_features(C, voxels[:, None])
    assert got.shape == (2, 3) and got.dtype == T.RUN_FEATURE_DTYPE
    for i in np.ndindex(2, 3):
        _assert_features(got[i], TO.run_features_exact(C[i], int(voxels[i[0]])), T.RUN_FEATURES, (Ng, R, i))
    mean = T.mean_over_directions(got)
    for gi in range(2):
        want = TO.mean_over_directions([TO.run_features_exact(C[gi, k], int(voxels[gi])) for k in range(3)], T.RUN_FEATURES)
        _assert_features(mean[gi], want, T.RUN_FEATURES, ("mean", gi))
    assert np.isnan(T.mean_over_directions(T.run_features(np.zeros((1, 2, Ng, R), np.int64), [[0]]))["run_entropy"]).all()


# ---- refusals: all before a device is needed ------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals():
    from covidseg_amd import texture as T
    ct = np.zeros((4, 3, 2), np.int16)
    m = np.ones((4, 3, 2), np.uint8)
    for fn in (T.quantize_volume, T.glcm, T.run_lengths, T.texture_stats):
        for kw in (dict(levels=0), dict(levels=65), dict(levels=8.0), dict(levels=True), dict(width=0.0), dict(width=-1.0), dict(width=np.inf), dict(width=np.nan),
                   dict(lo=np.nan), dict(lo=-np.inf), dict(outside="wrap")):
            with pytest.raises(ValueError):
                fn(ct, mask=m, **kw)
        with pytest.raises(ValueError, match="exactly one of mask, labels"):
            fn(ct)
        with pytest.raises(ValueError, match="exactly one of mask, labels"):
            fn(ct, mask=m, labels=m.astype(np.int32), n=1)
        with pytest.raises(ValueError, match="labels need n"):
            fn(ct, labels=m.astype(np.int32))
        with pytest.raises(ValueError):
            fn(ct, labels=m.astype(np.int32), n=-1)
        with pytest.raises(ValueError):
            fn(ct, mask=np.ones((4, 3, 3), np.uint8))
        with pytest.raises(ValueError):
            fn(ct, mask=m, region=np.ones((4, 3, 2), np.float32))
    for fn in (T.glcm, T.run_lengths, T.texture_stats):
        for d in ("4d", [], [13], [-1], [(2, 0, 0)], [(0, 0, 0)], [(1, 0)], [1.5], 3, None):
            with pytest.raises(ValueError):
                fn(ct, mask=m, directions=d)
    for fn in (T.glcm, T.texture_stats):
        for d in (0, 5, 1.0, True, None):
            with pytest.raises(ValueError, match="distance"):
                fn(ct, mask=m, distance=d)
    for fn in (T.run_lengths, T.texture_stats):
        for r in (0, 2 ** 15 + 1, 2.0):
            with pytest.raises(ValueError, match="max_run"):
                fn(ct, mask=m, max_run=r)
    lab = np.ones((4, 3, 2), np.int32)
    with pytest.raises(ValueError, match=r"n = 300000 groups, K = 13 directions and Ng = 64 levels"):
        T.glcm(ct, labels=lab, n=300000)
    with pytest.raises(ValueError, match=r"n = 5 groups, K = 1 directions and Ng = 64 levels"):
        T.glcm(ct, labels=lab, n=5, merge=True, table_budget=1000)
    with pytest.raises(ValueError, match=r"n = 70000 groups, K = 4 directions and Ng = 64 levels"):
        T.run_lengths(ct, labels=lab, n=70000, directions="2d")
    with pytest.raises(ValueError, match="n = 300000"):
        T.texture_stats(ct, labels=lab, n=300000)
    assert T.check_table_budget(10, 13, 64, 64, "x") == 8 * 10 * 13 * 64 * 64


def test_directions():
    from covidseg_amd import texture as T
    assert T.DIRECTIONS == TO.DIRECTIONS and len(set(T.DIRECTIONS)) == 13
    assert T.check_directions("3d") == tuple(range(13)) and T.check_directions("2d") == (0, 1, 3, 4)
    assert T.check_directions([4, 0, (0, 1, 0), (-1, -1, 0), 4]) == (0, 1, 3, 4)
    assert T.check_directions([(1, -1, -1), np.int64(2)]) == (2, 12) and T.direction_bits((0, 1, 3, 4)) == 0b11011
    for k, d in enumerate(T.DIRECTIONS):                            # every direction or its negation, never both: dx > 0, or dx = 0 and dy > 0, or (0, 0, 1)
        assert d > (0, 0, 0) and tuple(-v for v in d) not in T.DIRECTIONS and T.check_directions([tuple(-v for v in d)]) == (k,)


# ---- declarations ---------------------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_built():
    import covidseg_amd
    from covidseg_amd import _lib, texture as T
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("unet_vol_texture_quantize", 20), ("unet_vol_texture_glcm", 13), ("unet_vol_texture_runs", 13)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", code)
        assert m and m.group(1).count(",") + 1 == nargs, name
        assert name in _lib._PROTOS and len(_lib._PROTOS[name][1]) == nargs and _lib._PROTOS[name][0] is _lib.i32 and name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 16
    for macro, value in (("UNET_VOL_TEXTURE_MAX_LEVELS", _lib.TEXTURE_MAX_LEVELS), ("UNET_VOL_TEXTURE_MAX_DISTANCE", _lib.TEXTURE_MAX_DISTANCE),
                         ("UNET_VOL_TEXTURE_LDS_COUNTERS", _lib.TEXTURE_LDS_COUNTERS)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", hdr), macro
    assert (T.MAX_LEVELS, T.MAX_DISTANCE, T.LDS_COUNTERS) == (64, 4, 8192)
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernels_texture\.hip\b", mk, flags=re.M)
    lists = [line for line in mk.splitlines() if line.endswith("EXTRA = -ffp-contract=off")]
    assert len(lists) == 3 and all("kernels_texture.o" in line for line in lists)          # the product, asan and ubsan rules
    assert re.search(r"^# kernels_texture\.hip:", mk, flags=re.M)
    assert re.search(r"^texture_loads:", mk, flags=re.M) and "-DTEXTURE_GLCM_LDS=0" in mk          # the measurement build: never the product library
    for name in ("texture_stats", "lesion_texture", "glcm", "run_lengths", "quantize_volume", "glcm_features", "run_features", "TextureStats"):
        assert getattr(covidseg_amd, name) is getattr(T, name) and name in covidseg_amd.__all__
    assert "texture" in covidseg_amd.__all__

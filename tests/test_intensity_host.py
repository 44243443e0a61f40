"""CPU: tests/intensity_oracle.py against numpy's own digitize / percentile / mean / var, the new entries' declarations and bindings, and every argument error of
volume.intensity_stats, which must be raised before a device is needed."""
import os
import re

import numpy as np
import pytest

import intensity_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unet_vol_intensity_bands": 19, "unet_vol_intensity_gather": 18, "unet_vol_group_moments_ws_bytes": 2, "unet_vol_group_moments": 8}
SIZES = (0, 1, 255, 256, 257, 65537)
U = 2.0 ** -53


def _values(m, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.normal(-400.0, 350.0, m))


def test_bands_are_digitize():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.uniform(-1100, 200, 5000), np.array(IO.HU_EDGES), np.nextafter(IO.HU_EDGES, -np.inf), np.nextafter(IO.HU_EDGES, np.inf), [-np.inf, np.inf, -0.0]])
    assert np.array_equal(IO.band_of(v, IO.HU_EDGES), np.digitize(v, IO.HU_EDGES))
    assert IO.band_of(np.array(IO.HU_EDGES), IO.HU_EDGES).tolist() == [1, 2, 3, 4]          # a value on an edge belongs to the band above it
    assert IO.band_of(np.array([np.nan, -2000.0, 1e9]), IO.HU_EDGES).tolist() == [5, 0, 4]
    one = IO.band_of(np.array([-1.0, 0.0, 1.0]), [0.0])
    assert one.tolist() == [0, 1, 1]


@pytest.mark.parametrize("m", SIZES)
def test_percentiles_are_numpys_bit_for_bit(m):
    run = _values(m, m)
    for q in (0, 5, 25, 50, 75, 95, 100, 33.3, 99.9):
        got = IO.percentile(run, q)
        if m == 0:
            assert np.isnan(got)
        else:
            want = np.percentile(run, q)
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (m, q)


@pytest.mark.parametrize("m", SIZES)
def test_two_level_moments_stay_within_the_reordering_bound(m):
    """Any two summation orders of m doubles differ by at most 2 (m - 1) u sum|v| (each within (m - 1) u sum|v| of the true sum, u = 2^-53): divided by m, the means
    differ by at most 2 m u mean|v|; the same for the squared deviations against np.var."""
    run = _values(m, 1000 + m)
    s, ssd = IO.moments_of_run(run)
    if m == 0:
        assert s == 0.0 and ssd == 0.0
        return
    mean = s / m
    assert abs(mean - np.mean(run)) <= 2 * m * U * np.mean(np.abs(run))
    d2 = (run - np.mean(run)) ** 2
    assert abs(ssd - np.var(run) * m) <= 2 * m * U * np.mean(d2) * m
    if m == 1:
        assert s == run[0] and ssd == 0.0
    if m <= 256:                                                    # one chunk: the plain left-to-right chain
        acc = run[0]
        for v in run[1:]:
            acc = acc + v
        assert s == acc


def test_grouping_ordering_and_counts():
    rng = np.random.default_rng(5)
    shape = (9, 7, 4)
    val = rng.uniform(-1000, 100, shape)
    val[0, 0, 0] = np.nan
    labels = rng.integers(-1, 6, shape)
    region = rng.integers(0, 2, shape).astype(np.uint8)
    g = IO.group_of(shape, labels=labels, n=3, region=region)
    assert set(np.unique(g)) <= {0, 1, 2, 3} and not g[region == 0].any() and not g[(labels < 1) | (labels > 3)].any()
    bc, sc, mm = IO.bands(val, g, 3, IO.HU_EDGES)
    assert bc.sum() == (g > 0).sum() == sc.sum() and np.array_equal(bc.sum(axis=0), sc.sum(axis=0))
    vals, grp, off = IO.ordered(val, g, 3)
    assert off[0] == 0 and off[-1] == len(vals) == bc[:, :5].sum()
    for k in range(3):
        run = vals[off[k]:off[k + 1]]
        assert (grp[off[k]:off[k + 1]] == k + 1).all() and (np.diff(run) >= 0).all()
        sel = val[(g == k + 1) & ~np.isnan(val)]
        assert mm[k, 0] == sel.min() and mm[k, 1] == sel.max()
    st = IO.stats(val, g, 3)
    assert st["voxels"] == (g > 0).sum() and np.array_equal(st["band_voxels"], st["groups"]["band_voxels"].sum(axis=0))
    assert st["min"] == np.nanmin(st["groups"]["min"]) and st["max"] == np.nanmax(st["groups"]["max"])
    none = IO.stats(val, np.zeros(shape, np.int64), 2)
    assert none["voxels"] == 0 and np.isnan(none["mean"]) and (none["groups"]["dominant_band"] == -1).all()


def test_the_new_entries_are_declared_and_bound():
    from covidseg_amd import _lib, volume as V
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/unet_hip.h"
        assert m.group(1).count(",") + 1 == nargs
        assert name in _lib._PROTOS, f"{name} is not bound in _lib._PROTOS"
        assert len(_lib._PROTOS[name][1]) == nargs
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 16 and "#define UNET_ABI_VERSION 16" in text
    m = re.search(r"#define UNET_VOL_INTENSITY_MAX_EDGES (\d+)", text)
    assert m and int(m.group(1)) == _lib.INTENSITY_MAX_EDGES == V.INTENSITY_MAX_EDGES == 63
    assert V.HU_BANDS == (IO.HU_NAMES, IO.HU_EDGES)
    mk = open(os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc", "Makefile")).read()
    assert "kernels_intensity.hip" in mk
    assert len(re.findall(r"kernels_intensity\.o: EXTRA = -ffp-contract=off", mk)) == 3          # the product, asan and ubsan rules
    for name in ("intensity_stats", "intensity_bands_device", "intensity_gather_device", "group_moments_device", "IntensityStats"):
        assert callable(getattr(V, name))


def test_lerp_is_shared_and_unchanged():
    from covidseg_amd import volume as V
    rng = np.random.default_rng(2)
    for _ in range(200):
        a, b = sorted(rng.normal(size=2)); t = float(rng.random())
        want = a + (b - a) * t
        if t >= 0.5:
            want = b - (b - a) * (1.0 - t)
        assert float(V._lerp(a, b, t)) == want
    arr = V._lerp(np.array([1.0, 2.0]), np.array([3.0, 2.0]), np.array([0.25, 0.75]))
    assert arr.tolist() == [1.5, 2.0]


def test_argument_errors_need_no_device():
    from covidseg_amd import volume as V
    ct = np.zeros((6, 5, 4), np.int16)
    mask = np.ones((6, 5, 4), np.uint8)
    labels = np.ones((6, 5, 4), np.int32)
    bad = [
        dict(mask=np.ones((6, 5, 3), np.uint8)),                                              # shapes that differ
        dict(mask=mask, region=np.ones((5, 6, 4), np.uint8)),
        dict(labels=np.ones((6, 4, 4), np.int32), n=1),
        dict(mask=mask.astype(np.float32)),                                                   # a float mask
        dict(mask=mask, region=mask.astype(np.float64)),
        dict(labels=labels.astype(np.float32), n=1),
        dict(labels=labels),                                                                  # labels without n
        dict(mask=mask, labels=labels, n=1),                                                  # both
        dict(),                                                                               # neither
        dict(labels=labels, n=-1),
        dict(mask=mask, edges=(0.0, 0.0)),                                                    # not ascending
        dict(mask=mask, edges=(1.0, 0.0), names=("a", "b", "c")),
        dict(mask=mask, edges=(0.0, np.inf), names=("a", "b", "c")),                          # not finite
        dict(mask=mask, edges=(np.nan,), names=("a", "b")),
        dict(mask=mask, edges=tuple(range(64)), names=None),                                  # too many
        dict(mask=mask, edges=(), names=("a",)),
        dict(mask=mask, names=("a", "b")),                                                    # names of the wrong length
        dict(mask=mask, percentiles=(50, 101)),                                               # a percentile outside [0, 100]
        dict(mask=mask, percentiles=(-1,)),
        dict(mask=mask, percentiles=(float("nan"),)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            V.intensity_stats(ct, **kw)
    with pytest.raises(ValueError):
        V.intensity_stats(np.zeros((6, 5), np.int16), mask=mask)
    for density in ({"edges": (1.0, 0.0)}, {"percentiles": (200,)}, {"shape": (1, 2, 3)}, {"names": ("a",)}):
        with pytest.raises(ValueError):
            V._check_density(density)
    assert V._check_density(None) is None and V._check_density(True) == {} and V._check_density({"moments": False}) == {"moments": False}

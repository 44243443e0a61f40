"""No GPU: the conditions the cases of tests/test_gpu_front_edges.py rest on, evaluated from the oracles and the case lists of tests/front_edges.py alone -- every "second
trip" shape exceeds the cap it is meant to exceed, the full-range volumes hold their type's extremes, few enough voxels lie near an unslice threshold for the rule taken
over from test_gpu_volume.py, the CLAHE shapes pad by less than the image (and the refused ones do not), and the NaN / infinity / uniform volumes give the values the GPU
test expects the device to reproduce."""
import warnings

import numpy as np
import pytest

import front_edges as FE
import volume_oracle as VO
from oracle import preprocess_oracle as P


def test_every_second_trip_shape_exceeds_its_cap():
    by = {name: (shape, S) for name, shape, S in FE.STRIDE_CASES}
    (X, Y, _), S = by["outputs<4> and resize"]
    assert S * S % 4 == 0 and S * S > FE.VOL_OUTPUTS4_TRIP and S * S > FE.VOL_RESIZE_TRIP and S > X and S > Y            # vectorised outputs, both axes up-scaled
    (X, Y, _), S = by["outputs<1> and resize"]
    assert S * S % 4 != 0 and S * S > FE.VOL_OUTPUTS1_TRIP and S * S > FE.VOL_RESIZE_TRIP
    (X, Y, _), S = by["uniform scan, area tables"]
    assert X * Y > FE.VOL_RESIZE_TRIP and S * S <= FE.VOL_RESIZE_TRIP
    sx, sy = 1.0 / (S / X), 1.0 / (S / Y)
    assert sx >= 1 and sy >= 1 and not (abs(sx - np.rint(sx)) < VO._EPS and abs(sy - np.rint(sy)) < VO._EPS)              # ResizeArea_'s tables, not the integer-scale sum
    assert 512 * 512 <= min(FE.VOL_RESIZE_TRIP, FE.VOL_OUTPUTS4_TRIP)                                                      # what the suite ran before: one trip exactly
    cases = {c[0]: c for c in FE.UNSLICE_CASES}
    _, (X, Y, Z), z0, z1, _, skew = cases["X % 4 == 0, unslice<4> strides, the whole range"]
    assert X % 4 == 0 and skew == 0 and X * Y > FE.VOL_UNSLICE4_TRIP and (z0, z1) == (0, Z)
    _, (X, Y, Z), z0, z1, _, skew = cases["the scalar loop strides, a single slice"]
    assert X % 4 != 0 and X * Y > FE.VOL_UNSLICE1_TRIP and z1 - z0 == 1
    _, (X, Y, Z), z0, z1, _, skew = cases["X % 4 == 0 behind a mask pointer off by one byte"]
    assert X % 4 == 0 and skew % 4 != 0
    assert FE.UNIT_COUNTS[-1] > FE.PRE_UNIT_TRIP >= FE.UNIT_COUNTS[-2]
    assert 256 * 256 + 1 > FE.PRE_MINMAX_TRIP >= 37 * 91 and 65 > FE.PRE_MINMAX_INIT_TPB


@pytest.mark.parametrize("kind", FE.INT_KINDS)
def test_full_range_volumes_hold_their_types_extremes(kind):
    raw = FE.full_range_volume(kind)
    info = np.iinfo(kind)
    assert raw.dtype == np.dtype(kind) and raw.shape == FE.RANGE_SHAPE and raw.min() == info.min and raw.max() == info.max
    for z in (0, FE.RANGE_SHAPE[2] - 1):
        assert raw[:, :, z].min() == info.min and raw[:, :, z].max() == info.max
    top = raw.astype(np.float64) > (info.max / 2)                    # a decode through the signed type of the same width would turn these negative
    assert 0.2 < top.mean() < 0.3 if info.min < 0 else 0.45 < top.mean() < 0.55
    for S in (31, 16, 48):                                          # the oracle answers at every resize path: nothing but finite values
        for slope, inter in ((0.0, 0.0), FE.SCALE):
            got = VO.slices_f64(raw, slope, inter, 0, 2, S)
            assert np.isfinite(got["img64"]).all() and np.isfinite(got["f32"]).all() and not got["uniform"].any()


@pytest.mark.parametrize("case", FE.UNSLICE_CASES, ids=[c[0] for c in FE.UNSLICE_CASES])
def test_few_voxels_lie_near_an_unslice_threshold(case):
    name, shape, z0, z1, t, _ = case
    c, wmask, near = FE.unslice_case(case)
    print(f"{name}: {int(near.sum())} of {near.size} voxels within {FE.NEAR} of {t}")
    assert near.mean() <= FE.NEAR_SHARE_CAP
    kept = wmask[:, :, z0:z1]
    if t > c.max():
        assert not wmask.any()
    elif t < c.min():
        assert kept.all() and not wmask[:, :, :z0].any() and not wmask[:, :, z1:].any()
    elif kept.size >= 1000:
        assert kept.any() and not kept.all()                         # the threshold cuts through the maps


def test_clahe_shapes_pad_by_less_than_the_image_and_the_refused_ones_do_not():
    tile_areas = set()
    for shape, tiles, clips in FE.CLAHE_CASES:
        ph, pw = FE.clahe_padding(shape, tiles)
        assert ph < shape[0] and pw < shape[1], (shape, tiles)
        tile_areas.add(((shape[0] + ph) // tiles[1]) * ((shape[1] + pw) // tiles[0]))
        for im in FE.clahe_batch(shape):                             # the oracle answers all of them
            for clip in clips:
                assert P.clahe_u8(im, clip, tiles).shape == shape
    assert {1, 4} <= tile_areas                                      # tiles of 1 x 1 and 2 x 2 pixels: lut_scale 255 and 63.75, the clip limit clamped up to 1
    assert FE.clahe_padding((16, 9), (8, 8)) == (8, 7) and FE.clahe_padding((17, 16), (8, 8)) == (7, 8)          # the divisible axis is padded by a whole tile
    for shape, tiles in FE.CLAHE_REFUSED:
        ph, pw = FE.clahe_padding(shape, tiles)
        assert ph >= shape[0] or pw >= shape[1], (shape, tiles)


@pytest.mark.parametrize("kind", ["f4", "f8"])
def test_nan_and_infinity_slices_give_what_numpy_gives(kind):
    raw = FE.nan_inf_volume(kind)
    Z = raw.shape[2]
    for S in FE.NAN_SIZES:
        with np.errstate(invalid="ignore"):
            got = VO.slices_f64(raw, 0.0, 0.0, 0, Z, S)
        assert got["uniform"].tolist() == [1, 0, 0, 0]              # np.unique collapses the NaNs of the all-NaN slice into one value
        assert np.isnan(got["minmax"][:2]).all() and np.isnan(got["img64"][0]).all() and np.isnan(got["f32"][:2]).all()
        assert not got["u8"].any()                                   # NaN, and x / inf = 0, all truncate to 0
        assert not got["lung"][:2].any()
        if S == 48:                                                  # up-scaling: inf * 0 sits in the bilinear blend
            assert np.isnan(got["minmax"][2:]).all() and np.isnan(got["f32"][2:]).all() and not got["lung"][2:].any()
        else:
            (mn2, mx2), (mn3, mx3) = got["minmax"][2], got["minmax"][3]
            assert np.isfinite(mn2) and mx2 == np.inf and mn3 == -np.inf and np.isfinite(mx3)
            hit = np.isinf(got["img64"][2])                          # the destination pixels whose cells hold the +inf: (inf - mn) / inf = NaN, the others 0
            assert 1 <= hit.sum() <= 9 and np.isnan(got["f32"][2][hit]).all() and (got["f32"][2][~hit] == 0).all()
            assert np.isnan(got["f32"][3]).all()                     # (v + inf) / inf


def test_uniform_volumes_give_the_flags_the_gpu_test_expects():
    i2, f4, flags = FE.uniform_volumes()
    Z = i2.shape[2]
    assert VO.slices_f64(i2, 0.0, 0.0, 0, Z, 32)["uniform"].tolist() == [0, 1, 0, 0, 0, 0]
    assert VO.slices_f64(f4, 0.0, 0.0, 0, Z, 32)["uniform"].tolist() == [0] + flags + [0]
    assert np.signbit(f4[:, :, 4]).any() and not np.signbit(f4[:, :, 4]).all() and not f4[:, :, 4].any()
    X, Y, _ = i2.shape
    lone = np.argwhere(i2[:, :, 2] != i2[0, 0, 2])
    assert lone.tolist() == [[X - 1, Y - 1]]                         # the last voxel of the slice in memory (Fortran order): the last thread of the strided scan sees it


def test_minmax_expected_is_the_oracle_and_a_nan_zeroes_the_slice():
    x = FE.minmax_batch()
    assert np.array_equal(FE.minmax_expected(x[0]), P.minmax_to_u8(x[0])) and FE.minmax_expected(x[0]).max() == 255
    for i in (1, 2, 3, 4):                                           # NaN, +inf, -inf, constant: all zero
        assert not FE.minmax_expected(x[i]).any(), i
    small = np.random.default_rng(1).normal(0, 1, (5, 7)).astype(np.float32)
    small[2, 3] = np.nan
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore")
        assert not P.minmax_to_u8(small).any()                       # the oracle's own np.uint8 cast agrees on this platform
    assert not FE.minmax_expected(small).any()


def test_unit_edges_sit_on_both_sides_of_every_truncation():
    e = FE.unit_edges()
    assert e.dtype == np.float32 and e.size == 511 and e.min() == 0 and e.max() == 1
    got = P.to_u8(e)
    assert set(got.tolist()) == set(range(256)) and (got[256:] == np.arange(255)).all()          # just below k / 255: the byte below
    assert (got[:256] == np.arange(256)).all()                       # float32(k / 255) never lies below k / 255 (1 / 255 repeats 00000001: the cut-off tail starts with a 1)
    assert (np.rint(e[256:].astype(np.float64) * 255) == np.arange(1, 256)).all()          # ... and a rounding conversion gets every value just below wrong
    assert np.array_equal(P.u8_to_unit(np.arange(256, dtype=np.uint8)), e[:256])


def test_resize_rectangles_touch_the_edges_and_the_oracle_answers_them():
    sh, sw = FE.RESIZE_SRC
    r = FE.RESIZE_RECTS
    assert (r[:, 0] + r[:, 2] <= sw).all() and (r[:, 1] + r[:, 3] <= sh).all()
    assert (r[:, 0] + r[:, 2] == sw).sum() >= 2 and (r[:, 1] + r[:, 3] == sh).sum() >= 3
    assert [1, 1] in r[:, 2:].tolist() and any(w == 1 and h > 1 for w, h in r[:, 2:].tolist())
    d = FE.RESIZE_DST
    assert d["dst_x0"] > 0 and d["dst_ld"] > d["dst_x0"] + d["dw"]
    for im, (x, y, w, h) in zip(FE.resize_sources(), r):
        for interp in (P.INTER_LINEAR, P.INTER_AREA):
            assert P.resize_u8(im[y:y + h, x:x + w], (d["dw"], d["dh"]), interp).shape == (d["dh"], d["dw"])

"""CPU: tests/volume_oracle.py against facts that do not depend on it, and the host logic of covidseg_amd.volume (slice trim, box indexing, the
empty-mask filter)."""
import math

import numpy as np
import pytest

import volume_oracle as VO
from oracle import preprocess_oracle as P


def _ramp(shape):
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape, order="F")


@pytest.mark.parametrize("Z", [5, 7, 10, 13, 45, 301])
def test_rot90_and_trim_against_numpy(Z):
    from covidseg_amd import volume as V
    vol = _ramp((4, 3, Z))
    z0, z1 = VO.trim_range(Z)
    assert (z0, z1) == (round(Z * 0.2), round(Z * 0.8)) == V.trim_range(Z)
    want = np.rollaxis(np.rot90(vol)[:, :, z0:z1], 2)                 # T1:287-290
    assert np.array_equal(VO.rot90_slices(vol, z0, z1), want)
    assert want.shape == (z1 - z0, 3, 4)


def test_get_fdata_is_two_rounded_operations():
    raw = np.array([[[3]]], np.int32)
    s = float(np.float32(1 / 3))
    assert VO.get_fdata(raw, s, -1.0)[0, 0, 0] == np.float64(3.0 * s) - 1.0
    assert VO.get_fdata(raw, 0.0, 9.0)[0, 0, 0] == 3.0 and VO.get_fdata(raw, float("nan"), 9.0)[0, 0, 0] == 3.0
    assert VO.get_fdata(raw, 2.0, float("nan"))[0, 0, 0] == 6.0


def test_equal_size_resize_is_the_identity():
    a = np.random.default_rng(0).normal(-500, 300, (32, 32))
    assert np.array_equal(VO.resize_area_f64(a, 32), a)


@pytest.mark.parametrize("shape", [(32, 32), (64, 64), (128, 64), (64, 96), (40, 63), (20, 50), (63, 20), (630, 630)])
def test_area_resize_of_a_constant_is_that_constant(shape):
    """Exactly that constant wherever OpenCV's arithmetic can give it: the copy, and integer scales whose float32 1 / area is a power of two (2 x 2, 4 x 2).
    Elsewhere the weights are float32 roundings of 1 / area or of the table's cell fractions and sum to one only up to float32 rounding (1.f / 6 is not 1 / 6):
    the constant comes back within the float32 epsilon times the number of weights per pixel (<= (scale + 2)^2) -- a bound from the number format, not a
    measured figure."""
    c = -731.25
    out = VO.resize_area_f64(np.full(shape, c), 32 if shape[0] < 600 else 512)
    S = out.shape[0]
    sy, sx = shape[0] / S, shape[1] / S
    area = sy * sx
    if sy == int(sy) and sx == int(sx) and sy >= 1 and sx >= 1 and math.log2(area) == int(math.log2(area)):
        assert np.all(out == c)
    else:
        terms = (max(sx, 1) + 2) * (max(sy, 1) + 2)
        assert np.abs(out - c).max() <= abs(c) * np.finfo(np.float32).eps * terms


def test_integer_scale_area_resize_is_the_block_mean():
    rng = np.random.default_rng(3)
    a = rng.normal(-400, 350, (64, 96))                              # 2 x 3 blocks -> 32 x 32
    out = VO.resize_area_f64(a, 32)
    inv = float(np.float32(1) / np.float32(6))                       # the float32 constant OpenCV multiplies by
    for dy, dx in ((0, 0), (31, 31), (7, 19), (16, 2)):
        blk = [float(v) for v in a[2 * dy:2 * dy + 2, 3 * dx:3 * dx + 3].ravel()]
        exact = math.fsum(blk)
        # the running float64 sum of 6 terms is within 5 roundings of the exact sum; the product adds one more
        assert abs(out[dy, dx] - exact * inv) <= 6 * np.spacing(abs(exact) + sum(abs(b) for b in blk)) * inv + np.spacing(abs(exact * inv))
    a2 = rng.normal(0, 1, (64, 64))                                  # 2 x 2: mean to 1 ulp of float64 (1/4 is exact in float32)
    o2 = VO.resize_area_f64(a2, 32)
    for dy, dx in ((0, 0), (5, 9), (31, 30)):
        blk = [float(v) for v in a2[2 * dy:2 * dy + 2, 2 * dx:2 * dx + 2].ravel()]
        m = math.fsum(blk) / 4
        assert abs(o2[dy, dx] - m) <= np.spacing(max(abs(b) for b in blk))


def test_normalise_and_uint8_forms():
    raw = np.zeros((4, 4, 5), np.int16)
    raw[:, :, 1] = np.arange(16).reshape(4, 4)
    raw[:, :, 2] = 7                                                 # a constant slice
    r = VO.slices_f64(raw, 0.0, 0.0, 1, 4, 4)
    assert list(r["uniform"]) == [0, 1, 1]
    assert r["f32"][0].min() == 0 and r["f32"][0].max() == 1 and r["u8"][0].max() == 255
    assert np.array_equal(r["lung"][0] > 0, r["f32"][0] > 0) and set(np.unique(r["lung"][0])) == {0, 255}
    assert np.isnan(r["f32"][1]).all() and not r["u8"][1].any() and not r["lung"][1].any()          # numpy's 0/0


RECTS = np.array([[[30, 40, 90, 200], [150, 30, 80, 190]]], np.int32)


def test_paste_back_of_a_constant_map():
    prob = np.full((1, 64, 64), 0.625, np.float32)
    c = VO.paste_back(prob, RECTS, 256)
    inside = np.zeros((256, 256), bool)
    for x, y, w, h in RECTS[0]:
        inside[y:y + h, x:x + w] = True
    assert np.all(c[0][inside] == np.float32(0.625)) and np.all(c[0][~inside] == 0)
    whole = VO.paste_back(prob, None, 256)
    assert np.all(whole == np.float32(0.625))


def test_paste_back_then_forward_crop_returns_a_smooth_map():
    """p(u, v) = 0.5 + 0.4 sin(2 pi u / 90) cos(2 pi v / 120) on a 224 x 224 model grid -> paste-back to a 512 canvas -> uint8 -> crop / INTER_AREA / fuse /
    INTER_LINEAR back to 224.  Per model pixel |dp/du| <= Lu = 0.4 * 2 pi / 90, |dp/dv| <= Lv = 0.4 * 2 pi / 120.  A sample can move, per axis, by at most
    1 model pixel in the paste-back's bilinear blend, by half a fused pixel (d / 250 model pixels) plus one canvas pixel (d / (2 w) resp. d / h model pixels) in the
    area average, and by one fused pixel in the last bilinear resize; three uint8 roundings add 1 / 255 each at most."""
    d, S = 224, 512
    rects = np.array([[[60, 90, 170, 330], [280, 95, 180, 320]]], np.int32)
    v, u = np.mgrid[0:d, 0:d].astype(np.float64)
    p = (0.5 + 0.4 * np.sin(2 * np.pi * u / 90) * np.cos(2 * np.pi * v / 120)).astype(np.float32)
    canvas = VO.paste_back(p[None], rects, S)[0]
    u8 = np.uint8(np.rint(canvas.astype(np.float64) * 255))
    back = P.resize_u8(P.crop_resize_fuse(u8, tuple(rects[0, 0]), tuple(rects[0, 1])), (d, d), P.INTER_LINEAR).astype(np.float64) / 255
    Lu, Lv = 0.4 * 2 * np.pi / 90, 0.4 * 2 * np.pi / 120
    wmin, hmin = rects[0, :, 2].min(), rects[0, :, 3].min()
    bound = Lu * (1 + 1.5 * d / 250 + d / (2 * wmin)) + Lv * (1 + 1.5 * d / 250 + d / hmin) + 3 / 255
    err = np.abs(back - p).max()
    print(f"paste-back -> forward round trip: max error {err:.4f}, bound {bound:.4f}")
    assert err <= bound


def test_unslice_identity_geometry_and_counts():
    rng = np.random.default_rng(5)
    canvas = rng.random((3, 8, 8)).astype(np.float32)
    mask, counts, ps = VO.unslice(canvas, 0.5, (8, 8, 7), 2, 5)
    assert np.array_equal(ps, canvas)                                # S == X == Y: the sampler lands on the pixel centres
    assert not mask[:, :, :2].any() and not mask[:, :, 5:].any()
    for k in range(3):
        want = np.rot90(mask[:, :, 2 + k])                           # back to the image orientation
        assert np.array_equal(want, (canvas[k] > np.float32(0.5)).astype(np.uint8))
        assert counts[k] == mask[:, :, 2 + k].sum()


def test_box_indexing_modes_on_a_volume_whose_third_kept_slice_is_uniform():
    from covidseg_amd import volume as V
    Z = 10
    z0, z1 = V.trim_range(Z)                                         # slices 2..7: six kept
    n = z1 - z0
    lung = np.zeros((16, 16, Z), np.uint8)
    for z in range(Z):
        if z != z0 + 2:
            lung[2:6, 3:12, z] = 1; lung[9:14, 3:12, z] = 1
    uniform = [int(np.unique(lung[:, :, z]).size == 1) for z in range(z0, z1)]
    kept = [i for i in range(n) if not uniform[i]]
    assert kept == [0, 1, 3, 4, 5]
    ref = V.box_plan(n, kept, "reference")
    assert list(ref) == [0, 1, 2, 3, 4, -1]                          # slice 2 takes slice 3's boxes, ..., the last slice finds none (T1:347)
    assert [kept[k] for k in ref[:5]] == [0, 1, 3, 4, 5]             # ... i.e. every box after the skipped slice is shifted by one
    sl = V.box_plan(n, kept, "slice")
    assert list(sl) == [0, 1, -1, 2, 3, 4]                           # only the uniform slice falls through
    with pytest.raises(ValueError, match="box_indexing"):
        V.box_plan(n, kept, "other")


def test_drop_constant_removes_exactly_the_all_constant_infection_slices():
    from covidseg_amd import volume as V
    inf = [np.zeros((4, 4)), np.eye(4), np.full((4, 4), 3.0), np.arange(16.).reshape(4, 4), np.zeros((4, 4))]
    cts = [np.full((4, 4), float(i)) for i in range(5)]
    c, m, dropped = V.drop_constant(cts, inf)
    assert dropped == [0, 2, 4] and [int(a[0, 0]) for a in c] == [1, 3] and len(m) == 2


def test_whole_frame_rects_cover_the_frame_once():
    from covidseg_amd import volume as V
    r1, r2 = V.whole_frame_rects(2, 511)
    cover = np.zeros((511, 511), int)
    for x, y, w, h in (r1[0], r2[0]):
        cover[y:y + h, x:x + w] += 1
    assert np.all(cover == 1)


def test_probability_maps_of_the_gpu_tests_stay_clear_of_the_threshold():
    """the synthetic maps tests/test_gpu_volume.py thresholds: the share of voxels whose float64 probability lies within 1e-6 of t is far under the 0.1 % cap
    for the oracle itself (float32 vs float64 blend)"""
    from test_gpu_volume import synthetic_prob, PASTE_RECTS
    prob = synthetic_prob(3, 64, 1)
    c32 = VO.paste_back(prob, PASTE_RECTS, 128)
    c64 = VO.paste_back(prob, PASTE_RECTS, 128, np.float64)
    m32, _, _ = VO.unslice(c32, 0.547, (120, 100, 5), 1, 4)
    m64, _, p64 = VO.unslice(c64, 0.547, (120, 100, 5), 1, 4, np.float64)
    near = np.abs(p64 - 0.547) <= 1e-6
    assert near.mean() <= 0.001
    diff = (m32 != m64)[:, :, 1:4]
    assert diff.sum() <= near.sum()

"""CPU: tests/render_oracle.py against statements written another way, the committed BONE table against matplotlib, key_slices / the sheet layout of volume.py against the
oracle's, and every argument error of render_planes / project_volume / segment_volume(render=) -- raised before any device is looked for."""
import numpy as np
import pytest

import render_oracle as RO
from covidseg_amd import volume as V


# ---- the oracle against independent statements ------------------------------------------------------------------------------------------------------------
def test_grey_is_clip_and_round_away_from_ties():
    rng = np.random.default_rng(0)
    lo, hi = -1350.0, 150.0
    v = rng.uniform(-3000, 2000, 5000)
    t = (v - lo) / (hi - lo) * 255.0
    v = v[np.abs(t - np.floor(t) - 0.5) > 1e-6]                      # away from the .5 ties
    want = np.clip(np.rint(np.clip((v - lo) / (hi - lo), 0.0, 1.0) * 255.0), 0, 255).astype(np.uint8)
    assert np.array_equal(RO.grey(v, lo, hi), want)
    edge = np.array([lo, hi, np.nan, np.inf, -np.inf, lo + (hi - lo) * 0.5 / 255.0, lo + (hi - lo) * 1.5 / 255.0])
    assert RO.grey(edge, lo, hi).tolist()[:5] == [0, 255, 0, 255, 0]
    assert RO.grey(np.array([0.5, 1.5, 2.5, 254.5]), 0.0, 255.0).tolist() == [1, 2, 3, 255]          # ties go up: floor(t 255 + 0.5)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_nearest_at_an_integer_zoom_is_repeat(k):
    img = np.random.default_rng(1).integers(0, 99, (5, 7))
    assert np.array_equal(RO.sample_nearest(img, 7 * k, 5 * k), np.repeat(np.repeat(img, k, 0), k, 1))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_identity_size_nearest_is_rot90_of_the_plane(axis):
    vol = np.random.default_rng(2).normal(size=(6, 5, 4))
    roi = RO.whole(vol.shape)
    idx = 2
    want = np.rot90(np.take(vol, idx, axis=axis))
    img = RO.plane_image(vol, axis, idx, roi)
    assert np.array_equal(img, want)
    assert np.array_equal(RO.sample_nearest(img, img.shape[1], img.shape[0]), want)
    assert np.array_equal(RO.sample_linear(img, img.shape[1], img.shape[0]), want)          # fx = fy = 0 at identity size
    # the table of the definition: row i, column j of the axial view is voxel (x = j, y = n_y - 1 - i)
    i, j = 1, 3
    u, v = RO.IN_PLANE[axis]
    pos = [idx, idx, idx]; pos[u] = j; pos[v] = vol.shape[v] - 1 - i
    assert img[i, j] == vol[tuple(pos)]


def test_linear_sampling_of_a_ramp_and_of_a_constant():
    img = np.add.outer(np.arange(4) * 10.0, np.arange(6) * 1.0)
    up = RO.sample_linear(img, 12, 8)
    assert up[0, 0] == img[0, 0] and up[-1, -1] == img[-1, -1]          # clamped at the edge
    assert np.allclose(up[2:-2, 2:-2], np.add.outer(((np.arange(8) + 0.5) / 2 - 0.5) * 10.0, (np.arange(12) + 0.5) / 2 - 0.5)[2:-2, 2:-2])
    assert (RO.sample_linear(np.full((3, 5), 7.25), 11, 4) == 7.25).all()


def test_blend_full_and_zero_alpha():
    rgb = np.random.default_rng(3).integers(0, 256, (4, 5, 3)).astype(np.uint8)
    colour = np.random.default_rng(4).integers(0, 256, (4, 5, 3)).astype(np.uint8)
    assert np.array_equal(RO.blend(rgb, colour, np.full((4, 5), 255)), colour)
    assert np.array_equal(RO.blend(rgb, colour, np.full((4, 5), 0)), rgb)
    half = RO.blend(np.full((1, 1, 3), 100, np.uint8), np.full((1, 1, 3), 200, np.uint8), np.full((1, 1), 128))
    assert half.tolist() == [[[150, 150, 150]]]                     # (200 128 + 100 127 + 127) // 255


def test_the_outline_of_a_rectangle_is_its_border():
    L = np.zeros((9, 11), np.int64)
    L[2:7, 3:9] = 4
    want = np.zeros_like(L, bool)
    want[2:7, 3:9] = True; want[3:6, 4:8] = False
    on = L > 0
    assert np.array_equal(RO.outline(L) & on, want)
    L = np.zeros((6, 6), np.int64); L[0:4, 2:6] = 1                  # touches the top and the right edge of the tile: the edge pixels are outline
    want = np.zeros_like(L, bool); want[0:4, 2:6] = True; want[1:3, 3:5] = False
    assert np.array_equal(RO.outline(L) & (L > 0), want)
    pal = np.array([(9, 9, 9), (255, 0, 0)], np.uint8)
    rgb = np.full((6, 6, 3), 50, np.uint8)
    out = RO.apply_layer(rgb, L, pal, 0, 255)
    assert (out[want] == (255, 0, 0)).all() and (out[~want] == 50).all()          # fill alpha 0 leaves the inside


def test_labels_cycle_through_the_palette():
    pal = np.array([(0, 0, 0), (10, 0, 0), (20, 0, 0), (30, 0, 0)], np.uint8)
    L = np.array([[1, 2, 3, 4, 5, 7, -3, 0, 2 ** 31 - 1]])
    out = RO.apply_layer(np.zeros((1, 9, 3), np.uint8), L, pal, 255, 255)
    assert out[0, :, 0].tolist() == [10, 20, 30, 10, 20, 10, 0, 0, 10 * (1 + (2 ** 31 - 2) % 3)]


def test_projection_skips_nans():
    fd = np.array([[[1.0, np.nan], [np.nan, np.nan]], [[-2.0, 5.0], [np.nan, 0.0]]])
    assert np.array_equal(RO.project(fd, 0, 0, 2, 0)[0], [[1.0, 5.0], [np.nan, 0.0]], equal_nan=True)
    assert np.array_equal(RO.project(fd, 0, 0, 2, 1)[0], [[-2.0, 5.0], [np.nan, 0.0]], equal_nan=True)
    assert RO.project(fd, 2, 1, 2, 0).shape == (2, 2, 1)


# ---- the committed table and the host side of render_planes ----------------------------------------------------------------------------------------
def test_bone_is_matplotlibs_table():
    mpl = pytest.importorskip("matplotlib")
    want = mpl.colormaps["bone"](np.arange(256), bytes=True)[:, :3]
    assert V.BONE.dtype == np.uint8 and np.array_equal(V.BONE, want)


def test_tables_and_constants():
    assert V.BONE.shape == (256, 3) and V.GRAY.shape == (256, 3) and (V.GRAY[:, 0] == np.arange(256)).all() and V.GRAY.dtype == np.uint8
    assert V.WINDOWS == {"lung": (-1350.0, 150.0), "mediastinum": (-160.0, 240.0)}
    for p in (V.PALETTE_INFECTION, V.PALETTE_LUNG, V.PALETTE_LESIONS):
        assert p.dtype == np.uint8 and p.ndim == 2 and p.shape[1] == 3 and p.shape[0] >= 2
    l = V.Layer(np.zeros((2, 2, 2), np.uint8))
    assert (l.fill_alpha, l.outline_alpha) == (128, 255)
    import covidseg_amd
    assert covidseg_amd.render_planes is V.render_planes and covidseg_amd.Layer is V.Layer


def test_key_slices():
    c = [0, 5, 9, 5, 0, 9, 1, 5]
    for n in range(0, 10):
        assert V.key_slices(c, n) == RO.key_slices(c, n), n
    assert V.key_slices(c, 2) == [2, 5] and V.key_slices(c, 3) == [1, 2, 5]          # the tie among the three 5s goes to the lowest z
    assert V.key_slices(c, 4) == [1, 2, 3, 5] and V.key_slices(c, 50) == [1, 2, 3, 5, 6, 7]          # fewer than n hold infection
    assert V.key_slices(np.zeros(7, np.int64), 6) == [] and V.key_slices([], 3) == []
    with pytest.raises(ValueError):
        V.key_slices(c, -1)


def test_layout_and_tile_sizes():
    rng = np.random.default_rng(6)
    for k in (1, 2, 5, 7, 65):
        sizes = [(int(rng.integers(1, 40)), int(rng.integers(1, 40))) for _ in range(k)]
        for cols in (None, 1, 3, 100):
            for gap in (0, 2):
                pos, H, W = V.sheet_layout(sizes, cols, gap)
                assert (pos, H, W) == RO.layout(sizes, cols, gap)
                occ = np.zeros((H, W), np.int32)
                for (x0, y0), (w, h) in zip(pos, sizes):
                    assert x0 >= gap and y0 >= gap and x0 + w <= W - gap and y0 + h <= H - gap
                    occ[y0:y0 + h, x0:x0 + w] += 1
                assert occ.max() == 1                               # no two tiles overlap
    assert V.tile_pixels(67, 0.7, 0.7) == 67 and V.tile_pixels(7, 2.5, 0.7) == 25 and V.tile_pixels(1, 0.1, 5.0) == 1


def test_minmax_window_minds_the_slope():
    from covidseg_amd import nifti_min
    raw = np.asfortranarray(np.arange(24, dtype=np.int16).reshape(2, 3, 4) - 5)
    vol = nifti_min.NiftiVolume(raw, -2.0, 100.0, (1.0, 1.0, 1.0), nifti_min.default_header(raw.shape), "<")
    assert V._check_window("minmax", vol) == RO.minmax_window(vol.get_fdata()) == (100.0 - 2.0 * 18, 110.0)
    f = np.asfortranarray(np.array([[[np.nan, 3.0], [np.inf, -1.5]]], np.float32))
    assert V._check_window("minmax", V._source(f)) == (-1.5, 3.0)
    with pytest.raises(ValueError, match="constant"):
        V._check_window("minmax", V._source(np.full((2, 2, 2), 7, np.int16)))


# ---- argument errors: ValueError, with or without a device --------------------------------------------------------------------------------------------
CT = np.zeros((6, 5, 4), np.int16)
MASK = np.zeros((6, 5, 4), np.uint8)


def _bad_render_calls():
    P = [("axial", 1)]
    yield "unknown view", lambda: V.render_planes(CT, [("oblique", 1)])
    yield "unknown projection view", lambda: V.render_planes(CT, [("mip", "frontal", 0, 2)])
    yield "malformed plane", lambda: V.render_planes(CT, [("axial", 1, 2)])
    yield "no planes", lambda: V.render_planes(CT, [])
    yield "unknown window", lambda: V.render_planes(CT, P, window="bone")
    yield "inverted window", lambda: V.render_planes(CT, P, window=(5.0, 5.0))
    yield "NaN window", lambda: V.render_planes(CT, P, window=(float("nan"), 5.0))
    yield "constant minmax", lambda: V.render_planes(CT, P, window="minmax")
    yield "unknown cmap", lambda: V.render_planes(CT, P, cmap="viridis")
    yield "cmap shape", lambda: V.render_planes(CT, P, cmap=np.zeros((255, 3), np.uint8))
    yield "unknown interp", lambda: V.render_planes(CT, P, interp="cubic")
    yield "index above", lambda: V.render_planes(CT, [("axial", 4)])
    yield "index below", lambda: V.render_planes(CT, [("sagittal", -1)])
    yield "coronal index", lambda: V.render_planes(CT, [("coronal", 5)])
    yield "slab", lambda: V.render_planes(CT, [("mip", "coronal", 2, 2)])
    yield "slab past the axis", lambda: V.render_planes(CT, [("minip", "axial", 0, 5)])
    yield "five layers", lambda: V.render_planes(CT, P, layers=[MASK] * 5)
    yield "layer shape", lambda: V.render_planes(CT, P, layers=[np.zeros((6, 5, 3), np.uint8)])
    yield "float layer", lambda: V.render_planes(CT, P, layers=[np.zeros((6, 5, 4), np.float32)])
    yield "alpha above", lambda: V.render_planes(CT, P, layers=[V.Layer(MASK, fill_alpha=256)])
    yield "alpha below", lambda: V.render_planes(CT, P, layers=[V.Layer(MASK, outline_alpha=-1)])
    yield "alpha float", lambda: V.Layer(MASK, fill_alpha=0.5)
    yield "palette dtype", lambda: V.Layer(MASK, palette=np.zeros((3, 3), np.float32))
    yield "palette shape", lambda: V.Layer(MASK, palette=np.zeros((3, 4), np.uint8))
    yield "palette of one", lambda: V.Layer(MASK, palette=np.zeros((1, 3), np.uint8))
    yield "background", lambda: V.render_planes(CT, P, background=(0, 0, 256))
    yield "gap", lambda: V.render_planes(CT, P, gap=-1)
    yield "cols", lambda: V.render_planes(CT, P, cols=0)
    yield "tile_size", lambda: V.render_planes(CT, P, tile_size=(0, 4))
    yield "mm_per_px", lambda: V.render_planes(CT, P, mm_per_px=0.0)
    yield "roi name", lambda: V.render_planes(CT, P, roi="lungs")
    yield "roi empty", lambda: V.render_planes(CT, P, roi=((0, 6), (2, 2), (0, 4)))
    yield "roi outside", lambda: V.render_planes(CT, P, roi=((0, 7), (0, 5), (0, 4)))
    yield "plane outside the roi", lambda: V.render_planes(CT, P, roi=((0, 6), (0, 5), (2, 4)))
    yield "project axis", lambda: V.project_volume(CT, 3)
    yield "project view", lambda: V.project_volume(CT, "top")
    yield "project mode", lambda: V.project_volume(CT, 0, mode="mean")
    yield "project slab", lambda: V.project_volume(CT, 2, slab=(3, 3))
    yield "project slab outside", lambda: V.project_volume(CT, 1, slab=(0, 6))
    yield "project five layers", lambda: V.project_volume(CT, 0, layers=[MASK] * 5)
    yield "project layer shape", lambda: V.project_volume(CT, 0, layers=[MASK[:, :, :2]])
    yield "render key", lambda: V.segment_volume(CT, None, render={"zoom": 2})
    yield "render n", lambda: V.segment_volume(CT, None, render={"n": 0})
    yield "render window", lambda: V.segment_volume(CT, None, render={"window": "abdomen"})
    yield "render interp", lambda: V.segment_volume(CT, None, render={"interp": 2})
    yield "ensemble render", lambda: V._check_render({"cmap": "jet"})


@pytest.mark.parametrize("what,call", list(_bad_render_calls()), ids=[w for w, _ in _bad_render_calls()])
def test_argument_errors_need_no_device(what, call, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # were any device work attempted, the error would be a UNetHipError (or a torch one)
    with pytest.raises(ValueError):
        call()


def test_render_none_is_off():
    assert V._check_render(None) is None and V._check_render(False) is None and V._check_render(True) == {}
    assert V._check_render({"n": 3, "out_path": "x.png", "window": (0.0, 1.0)}) == {"n": 3, "out_path": "x.png", "window": (0.0, 1.0)}

"""-m gpu: csrc/kernels_render.hip and volume.project_volume / render_planes / segment_volume(render=) against tests/render_oracle.py.  Planes, label planes and canvases
are defined operation by operation, so every comparison is array_equal (NaN planes: equal_nan)."""
import ctypes as C

import numpy as np
import pytest

import render_oracle as RO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
SHAPES = [(5, 3, 2), (64, 4, 3), (67, 9, 7), (130, 5, 4), (1, 1, 1)]          # x short of a wave, on it, past it, past two waves; one voxel
STORAGE = ["i2", "i2neg", "u1", "f4nan", "f8"]
CODES = {"u1": 2, "i2": 4, "f4": 16, "f8": 64}
SENTINEL = 0x5A
PAL2 = np.array([(0, 0, 0), (255, 40, 0)], np.uint8)
PAL4 = np.array([(1, 2, 3), (0, 255, 255), (10, 200, 30), (250, 250, 5)], np.uint8)


def _volume(shape, kind, seed):
    """-> (raw [X, Y, Z] Fortran order, NIfTI code, scaling or None, element offset of the upload)"""
    rng = np.random.default_rng(seed)
    if kind in ("i2", "i2neg"):
        raw = rng.integers(-1200, 600, shape).astype(np.int16)
        return np.asfortranarray(raw), 4, ((0.5, -100.0) if kind == "i2" else (-1.5, 20.25)), 0
    if kind == "u1":
        return np.asfortranarray(rng.integers(0, 256, shape).astype(np.uint8)), 2, None, 1          # the byte type: off its alignment by one element
    if kind == "f4nan":
        raw = (rng.normal(size=shape) * 500).astype(np.float32)
        raw[rng.random(shape) < 0.15] = np.nan
        raw[:, 0, 0] = np.nan; raw[0, :, -1] = np.nan; raw[-1, -1, :] = np.nan          # a whole NaN column along every axis
        return np.asfortranarray(raw), 16, None, 0
    return np.asfortranarray(rng.normal(size=shape) * 400 - 300), 64, None, 0


def _up(a, offset=0):
    """the bytes of `a` on the device -- a volume [X, Y, Z] in Fortran order, a table or palette [n, 3] row by row --, `offset` elements into a larger buffer
    -> (tensor kept alive, pointer)"""
    import torch
    a = np.asarray(a)
    flat = (np.asfortranarray(a).reshape(-1, order="F") if a.ndim == 3 else np.ascontiguousarray(a).reshape(-1)).view(np.uint8)
    buf = torch.zeros(flat.size + 64 + offset * a.itemsize, dtype=torch.uint8, device="cuda")
    buf[offset * a.itemsize:offset * a.itemsize + flat.size] = torch.from_numpy(flat.copy()).cuda()
    return buf, buf.data_ptr() + offset * a.itemsize


def _labels(shape, seed):
    """a uint8 mask that touches the volume's border and an int32 label volume with labels above the palettes' sizes, negative labels and zeros"""
    rng = np.random.default_rng(100 + seed)
    mask = (rng.random(shape) < 0.45).astype(np.uint8) * rng.integers(1, 250, shape).astype(np.uint8)
    mask[0] = 7; mask[:, -1] = 1
    lab = rng.integers(-3, 14, shape).astype(np.int32)
    lab[rng.random(shape) < 0.3] = 0
    if np.prod(shape) > 8:
        lab[-1, 0, 0] = 2 ** 31 - 1
    return np.asfortranarray(mask), np.asfortranarray(lab)


def _vargs(raw, code, scaling):
    return (code,) + tuple(int(v) for v in raw.shape) + ((1, float(scaling[0]), float(scaling[1])) if scaling else (0, 1.0, 0.0))


# ---- unet_vol_project ----------------------------------------------------------------------------------------------------------------------------------
def _project(o, ptr, vargs, axis, a, b, mode, labels):
    """labels: [(device pointer or None, numpy dtype)] -> (rc, plane, [label planes or None]); every output lies inside a sentinel-filled buffer that must survive"""
    import torch
    dims = list(vargs[1:4]); dims[axis] = 1
    n = int(np.prod(dims))
    plane = torch.full((n + 16,), -77.0, dtype=torch.float64, device="cuda")
    outs = [None if p is None else torch.full((n + 32,), SENTINEL if dt == np.uint8 else -77, dtype=torch.uint8 if dt == np.uint8 else torch.int32, device="cuda") for p, dt in labels]
    k = len(labels)
    lp = (C.c_void_p * max(k, 1))(*[p for p, _ in labels])
    ld = (C.c_int32 * max(k, 1))(*[2 if dt == np.uint8 else 8 for _, dt in labels])
    lo = (C.c_void_p * max(k, 1))(*[None if t is None else t.data_ptr() + 8 * t.element_size() for t in outs])
    rc = o.lib.unet_vol_project(o.h, ptr, *vargs, axis, a, b, mode, lp, ld, lo, k, plane.data_ptr() + 64, o.s)
    torch.cuda.synchronize()
    p = plane.cpu().numpy()
    assert (p[:8] == -77.0).all() and (p[8 + n:] == -77.0).all()
    got = []
    for t, (_, dt) in zip(outs, labels):
        if t is None:
            got.append(None); continue
        h = t.cpu().numpy()
        s = SENTINEL if dt == np.uint8 else -77
        assert (h[:8] == s).all() and (h[8 + n:] == s).all()
        got.append(h[8:8 + n].reshape(dims, order="F"))
    return rc, p[8:8 + n].reshape(dims, order="F"), got


@pytest.mark.parametrize("kind", STORAGE)
@pytest.mark.parametrize("shape", SHAPES)
def test_project_equals_the_oracle(shape, kind):
    o = Ops()
    raw, code, scaling, off = _volume(shape, kind, sum(shape))
    fd = RO.fdata(raw, scaling)
    mask, lab = _labels(shape, sum(shape))
    keep, ptr = _up(raw, off)
    km, mp = _up(mask, 1)
    kl, lp = _up(lab)
    vargs = _vargs(raw, code, scaling)
    for axis in range(3):
        n = shape[axis]
        for a, b in {(0, n), (n // 2, n // 2 + 1), (n - 1, n), (0, max(1, n - 1))}:
            for mode in (0, 1):
                rc, plane, (pm, none, pl) = _project(o, ptr, vargs, axis, a, b, mode, [(mp, np.uint8), (None, np.int32), (lp, np.int32)])
                assert rc == 0, o.ctx.last_error()
                sl = [slice(None)] * 3; sl[axis] = slice(a, b)
                direct = (np.fmin if mode else np.fmax).reduce(fd[tuple(sl)], axis=axis, keepdims=True)
                assert np.array_equal(plane, direct, equal_nan=True), (axis, a, b, mode)
                assert np.array_equal(plane, RO.project(fd, axis, a, b, mode), equal_nan=True)
                assert none is None and pm.dtype == np.uint8 and pl.dtype == np.int32
                assert np.array_equal(pm, RO.project_labels(mask, axis, a, b)) and np.array_equal(pl, RO.project_labels(lab, axis, a, b)), (axis, a, b)
    if kind == "f4nan" and min(shape) > 1:
        assert np.isnan(_project(o, ptr, vargs, 0, 0, shape[0], 0, [])[1][0, 0, 0])          # the column of NaNs only
    rc, plane, _ = _project(o, ptr, vargs, 2, 0, shape[2], 0, [])                                  # no label volume at all
    assert rc == 0 and np.array_equal(plane, RO.project(fd, 2, 0, shape[2], 0), equal_nan=True)


def test_project_refusals_leave_the_outputs():
    o = Ops()
    raw, code, scaling, _ = _volume((6, 5, 4), "i2", 1)
    keep, ptr = _up(raw)
    km, mp = _up(np.ones((6, 5, 4), np.uint8))
    good = _vargs(raw, code, scaling)
    five = [(mp, np.uint8)] * 5
    cases = [(good, 3, 0, 1, 0, []), (good, -1, 0, 1, 0, []), (good, 0, 2, 2, 0, []), (good, 0, 3, 2, 0, []), (good, 1, 0, 6, 0, []), (good, 2, -1, 2, 0, []),
             (good, 0, 0, 6, 2, []), (good, 0, 0, 6, -1, []), (good, 0, 0, 6, 0, five), ((3,) + good[1:], 0, 0, 6, 0, []), ((code, 6, 0, 4, 0, 1.0, 0.0), 1, 0, 1, 0, [])]
    import torch
    plane = torch.full((64,), -77.0, dtype=torch.float64, device="cuda")
    lab_out = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    for vargs, axis, a, b, mode, labels in cases:
        k = len(labels)
        lp = (C.c_void_p * max(k, 1))(*[p for p, _ in labels])
        ld = (C.c_int32 * max(k, 1))(*[2] * k)
        lo = (C.c_void_p * max(k, 1))(*[lab_out.data_ptr()] * k)
        assert o.lib.unet_vol_project(o.h, ptr, *vargs, axis, a, b, mode, lp, ld, lo, k, plane.data_ptr(), o.s) == E_ARG, (vargs, axis, a, b, mode, k)
    lp, ld, lo = (C.c_void_p * 1)(mp), (C.c_int32 * 1)(4), (C.c_void_p * 1)(lab_out.data_ptr())
    assert o.lib.unet_vol_project(o.h, ptr, *good, 0, 0, 6, 0, lp, ld, lo, 1, plane.data_ptr(), o.s) == E_ARG          # an int16 label volume
    torch.cuda.synchronize()
    assert (plane.cpu().numpy() == -77.0).all() and (lab_out.cpu().numpy() == SENTINEL).all()


# ---- unet_vol_render ------------------------------------------------------------------------------------------------------------------------------------
class _Scene:
    """one volume with three layers on the device, and the same for the oracle"""

    def __init__(self, shape, kind, seed=None):
        from covidseg_amd import volume as V
        seed = sum(shape) if seed is None else seed
        self.raw, self.code, self.scaling, off = _volume(shape, kind, seed)
        self.fd = RO.fdata(self.raw, self.scaling)
        self.mask, self.lab = _labels(shape, seed)
        self.keep = [_up(self.raw, off), _up(self.mask, 1), _up(self.lab), _up(PAL2), _up(PAL4), _up(V.PALETTE_LESIONS), _up(V.BONE)]
        self.ptr, self.table = self.keep[0][1], self.keep[6][1]
        self.vargs = _vargs(self.raw, self.code, self.scaling)
        # a uint8 mask at half opacity with a solid edge, int32 labels as an outline only, the same labels again through a long palette: the layers overlap
        self.dev_layers = [(self.keep[1][1], self.keep[3][1], 2, 2, 128, 255), (self.keep[2][1], self.keep[4][1], 8, 4, 0, 255), (self.keep[2][1], self.keep[5][1], 8, 9, 200, 77)]          # unet_render_layer: labels, palette, dtype, P, alphas
        self.layers = [(self.mask, PAL2, 128, 255), (self.lab, PAL4, 0, 255), (self.lab, V.PALETTE_LESIONS, 200, 77)]
        f = self.fd[np.isfinite(self.fd)]
        if f.size > 1 and f.min() < f.max():
            self.window = (float(np.quantile(f, 0.2)), float(np.quantile(f, 0.8)))          # clips at both ends
        else:
            self.window = (float(f.min()) - 1.0, float(f.min()) + 1.0) if f.size else (0.0, 1.0)
        self.table_np = V.BONE


def _render(o, ptr, vargs, roi, window, table, interp, bg, fill, layers, tiles, H, W, pad=64, start=None):
    """-> (rc, canvas [H, W, 3], the bytes around it); the canvas sits `pad` bytes into a buffer filled with the sentinel (or with `start`)"""
    import torch
    from covidseg_amd import _lib
    n = H * W * 3
    buf = torch.full((pad + n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    if start is not None:
        buf[pad:pad + n] = torch.from_numpy(np.ascontiguousarray(start).reshape(-1)).cuda()
    L = (_lib.RenderLayer * max(len(layers), 1))(*[_lib.RenderLayer(*l) for l in layers])
    T = (_lib.RenderTile * max(len(tiles), 1))(*[_lib.RenderTile(*t) for t in tiles])
    r = (C.c_int32 * 6)(*[int(v) for ab in roi for v in ab])
    rc = o.lib.unet_vol_render(o.h, ptr, *vargs, r, float(window[0]), float(window[1]), table, interp, (bg[0] << 16) | (bg[1] << 8) | bg[2], fill, L, len(layers), T, len(tiles),
                               buf.data_ptr() + pad, H, W, o.s)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return rc, h[pad:pad + n].reshape(H, W, 3), np.concatenate([h[:pad], h[pad + n:]])


def _zooms(nu, nv):
    """identity, 2x and 3x up, a non-integer zoom down and up (7 -> 5 and 7 -> 11), one pixel"""
    return [(nu, nv), (2 * nu, 2 * nv), (3 * nu, 3 * nv), (max(1, nu * 5 // 7), nv * 11 // 7 + 1), (nu * 11 // 7 + 1, max(1, nv * 5 // 7)), (1, 1)]


def _row_of_tiles(axis, index, sizes, gaps=(1, 3, 2, 5, 1, 2, 4)):
    """the tiles side by side with uneven gaps, so that their row starts fall on every byte offset modulo 4 -> (tiles, H, W)"""
    x, tiles = gaps[0], []
    for k, (w, h) in enumerate(sizes):
        tiles.append((axis, index, x, 1 + k % 3, w, h))
        x += w + gaps[(k + 1) % len(gaps)]
    return tiles, max(t[3] + t[5] for t in tiles) + 2, x + 1


@pytest.mark.parametrize("kind", STORAGE)
@pytest.mark.parametrize("shape", SHAPES)
def test_render_every_view_zoom_and_sampler(shape, kind):
    o = Ops()
    S = _Scene(shape, kind)
    rois = [RO.whole(shape)]
    if shape == (67, 9, 7):
        rois.append(((3, 60), (1, 8), (2, 6)))                       # a region smaller than the volume
    for roi in rois:
        for axis in range(3):
            u, v = RO.IN_PLANE[axis]
            index = (roi[axis][0] + roi[axis][1]) // 2
            tiles, H, W = _row_of_tiles(axis, index, _zooms(roi[u][1] - roi[u][0], roi[v][1] - roi[v][0]))
            for interp in (0, 1):
                for pad in (64, 3):                                 # the canvas on and off a 4-byte boundary
                    rc, got, around = _render(o, S.ptr, S.vargs, roi, S.window, S.table, interp, (9, 80, 200), 1, S.dev_layers, tiles, H, W, pad)
                    assert rc == 0, o.ctx.last_error()
                    want = RO.draw_canvas(np.zeros((H, W, 3), np.uint8), S.fd, S.layers, tiles, roi, *S.window, S.table_np, interp, (9, 80, 200))
                    assert (around == SENTINEL).all(), (axis, interp, pad)
                    assert np.array_equal(got, want), (axis, interp, pad, roi, np.argwhere((got != want).any(-1))[:5])


def test_render_window_edges_and_grey_ties():
    from covidseg_amd import volume as V
    o = Ops()
    import math
    vals = np.array([0.0, 255.0, 0.5, 1.5, 100.5, -0.0, 254.5, np.nan, -7.0, 300.0, 254.49999999999997, 0.49999999999999994, 63.5, 127.5, 31.5], np.float64)
    n = vals.size
    raw = np.asfortranarray(vals.reshape(n, 1, 1))
    keep, ptr = _up(raw)
    kt, table = _up(V.GRAY)
    rc, got, _ = _render(o, ptr, (64, n, 1, 1, 0, 1.0, 0.0), RO.whole(raw.shape), (0.0, 255.0), table, 0, (0, 0, 0), 1, [], [(2, 0, 0, 0, n, 1)], 1, n)
    assert rc == 0
    t255 = [((v - 0.0) / (255.0 - 0.0)) * 255.0 for v in vals]      # the definition in scalar arithmetic: the same IEEE operations
    ties = [v for v, t in zip(vals, t255) if t == t and t == math.floor(t) + 0.5]
    assert len(ties) >= 3, "no value sits exactly on a .5 tie: the test would not see the rounding rule"
    want = [0 if not t > 0.0 else 255 if t >= 255.0 else int(math.floor(t + 0.5)) for t in t255]
    assert want[:2] == [0, 255] and want[5] == 0 and want[7:10] == [0, 0, 255]          # lo, hi, -0.0, NaN, both ends clip
    assert all(got[0, list(vals).index(v), 0] == math.floor(v) + 1 for v in ties)          # ties go up
    assert got[0, :, 0].tolist() == want
    assert np.array_equal(got, RO.draw_canvas(got, raw, [], [(2, 0, 0, 0, n, 1)], RO.whole(raw.shape), 0.0, 255.0, V.GRAY, 0, (0, 0, 0)))


def test_render_layer_rules():
    """fill alpha 0 with a solid outline, a mask touching the tile border, labels above P - 1 and below 0, alpha 0 leaves the bits, two layers on one pixel"""
    from covidseg_amd import volume as V
    o = Ops()
    shape = (9, 8, 1)
    raw = np.asfortranarray(np.random.default_rng(3).integers(0, 256, shape).astype(np.uint8))
    m = np.zeros(shape, np.uint8); m[0:5, 2:8] = 200                 # touches x = 0 and y = 7: two tile edges
    lab = np.zeros(shape, np.int32); lab[3:9, 0:4] = 5; lab[6, 6] = -4; lab[7, 7] = 2 ** 31 - 1; lab[8, 7] = 9
    keep = [_up(raw), _up(m), _up(lab), _up(PAL2), _up(PAL4), _up(V.GRAY)]
    roi, tiles = RO.whole(shape), [(2, 0, 2, 1, 9, 8), (2, 0, 14, 0, 27, 24)]
    for fa, oa in ((0, 255), (255, 0), (0, 0), (128, 255)):
        dl = [(keep[1][1], keep[3][1], 2, 2, fa, oa), (keep[2][1], keep[4][1], 8, 4, 255 - fa, oa)]
        rc, got, around = _render(o, keep[0][1], (2,) + shape + (0, 1.0, 0.0), roi, (0.0, 255.0), keep[5][1], 0, (1, 2, 3), 1, dl, tiles, 26, 43)
        want = RO.draw_canvas(got, raw.astype(np.float64), [(m, PAL2, fa, oa), (lab, PAL4, 255 - fa, oa)], tiles, roi, 0.0, 255.0, V.GRAY, 0, (1, 2, 3))
        assert rc == 0 and (around == SENTINEL).all() and np.array_equal(got, want), (fa, oa)
        if (fa, oa) == (0, 0):
            plain = RO.draw_canvas(got, raw.astype(np.float64), [], tiles, roi, 0.0, 255.0, V.GRAY, 0, (1, 2, 3))
            only_first = np.rot90((m[:, :, 0] > 0) & (lab[:, :, 0] <= 0))
            assert np.array_equal(got[1:9, 2:11][only_first], plain[1:9, 2:11][only_first])          # alpha 0: the grey's bits are untouched


def test_render_mixed_views_on_one_canvas_and_a_second_call():
    o = Ops()
    S = _Scene((67, 9, 7), "i2", 5)
    roi = RO.whole((67, 9, 7))
    tiles = [(2, 3, 1, 1, 67, 9), (1, 4, 70, 2, 67, 25), (0, 30, 139, 0, 9, 25), (2, 0, 3, 30, 33, 5), (0, 66, 40, 29, 18, 14), (1, 0, 61, 28, 90, 10)]
    H, W = 45, 153
    rc, got, around = _render(o, S.ptr, S.vargs, roi, S.window, S.table, 1, (20, 0, 40), 1, S.dev_layers, tiles, H, W, 1)
    want = RO.draw_canvas(np.zeros((H, W, 3), np.uint8), S.fd, S.layers, tiles, roi, *S.window, S.table_np, 1, (20, 0, 40))
    assert rc == 0 and (around == SENTINEL).all() and np.array_equal(got, want)
    assert (got[:, 151:] == (20, 0, 40)).all() and (got[44] == (20, 0, 40)).all()          # the gaps are written by the kernel: no sentinel is left
    # fill_background = 0: what no tile covers stays as it was
    more = [(2, 6, 100, 30, 40, 12)]
    rc, got2, around = _render(o, S.ptr, S.vargs, roi, S.window, S.table, 0, (1, 1, 1), 0, S.dev_layers[:1], more, H, W, 2, start=got)
    want2 = RO.draw_canvas(want, S.fd, S.layers[:1], more, roi, *S.window, S.table_np, 0, None)
    assert rc == 0 and (around == SENTINEL).all() and np.array_equal(got2, want2)
    rc, got3, _ = _render(o, S.ptr, S.vargs, roi, S.window, S.table, 0, (7, 8, 9), 1, [], [], 5, 6)          # no tile: the background alone
    assert rc == 0 and (got3 == (7, 8, 9)).all()


def test_render_refusals_leave_the_canvas():
    o = Ops()
    S = _Scene((6, 5, 4), "i2", 2)
    roi, win, H, W = RO.whole((6, 5, 4)), (-500.0, 100.0), 20, 30
    t0 = (2, 1, 0, 0, 6, 5)
    L = S.dev_layers
    nan = float("nan")

    def call(roi=roi, win=win, interp=1, bg=(0, 0, 0), layers=L, tiles=(t0,), H=H, W=W, vargs=S.vargs):
        rc, got, around = _render(o, S.ptr, vargs, roi, win, S.table, interp, bg, 1, list(layers), list(tiles), H, W)
        assert (got == SENTINEL).all() and (around == SENTINEL).all()
        return rc
    many = [(2, k % 4, (k % 10) * 3, (k // 10) * 2, 2, 1) for k in range(65)]
    bad = {"65 tiles": dict(tiles=many), "5 layers": dict(layers=L + L[:2]), "axis": dict(tiles=[(3, 1, 0, 0, 6, 5)]), "negative axis": dict(tiles=[(-1, 1, 0, 0, 6, 5)]),
           "index": dict(tiles=[(2, 4, 0, 0, 6, 5)]), "index below": dict(tiles=[(0, -1, 0, 0, 6, 5)]), "index outside the region": dict(roi=((0, 6), (0, 5), (2, 4)), tiles=[(2, 1, 0, 0, 6, 5)]),
           "w": dict(tiles=[(2, 1, 0, 0, 0, 5)]), "h": dict(tiles=[(2, 1, 0, 0, 6, 0)]), "right edge": dict(tiles=[(2, 1, 25, 0, 6, 5)]), "bottom edge": dict(tiles=[(2, 1, 0, 16, 6, 5)]),
           "negative corner": dict(tiles=[(2, 1, -1, 0, 6, 5)]), "overlap": dict(tiles=[t0, (1, 2, 5, 4, 6, 5)]), "empty region": dict(roi=((2, 2), (0, 5), (0, 4))),
           "inverted region": dict(roi=((0, 6), (3, 1), (0, 4))), "region past the volume": dict(roi=((0, 6), (0, 5), (0, 5))), "hi == lo": dict(win=(5.0, 5.0)),
           "hi < lo": dict(win=(5.0, 1.0)), "NaN lo": dict(win=(nan, 1.0)), "NaN hi": dict(win=(0.0, nan)), "interp": dict(interp=2),
           "P < 2": dict(layers=[L[0][:3] + (1,) + L[0][4:]]), "alpha": dict(layers=[L[0][:4] + (256, 0)]), "negative alpha": dict(layers=[L[0][:5] + (-1,)]),
           "layer dtype": dict(layers=[L[0][:2] + (4,) + L[0][3:]]), "null layer": dict(layers=[(None,) + L[0][1:]]), "datatype": dict(vargs=(3,) + S.vargs[1:])}
    for what, kw in bad.items():
        assert call(**kw) == E_ARG, what
    rc, got, around = _render(o, S.ptr, S.vargs, roi, win, S.table, 1, (0, 0, 0), 1, L, many[:64], H, W)          # 64 tiles that touch but do not overlap are taken
    assert rc == 0 and (around == SENTINEL).all()
    assert np.array_equal(got, RO.draw_canvas(got, S.fd, S.layers, many[:64], roi, *win, S.table_np, 1, (0, 0, 0)))


# ---- render_planes / project_volume ------------------------------------------------------------------------------------------------------------------------
PIX = (0.7, 0.7, 2.5)


def _nifti(raw, scaling, pix=PIX):
    from covidseg_amd import nifti_min
    return nifti_min.NiftiVolume(raw, scaling[0] if scaling else 0.0, scaling[1] if scaling else 0.0, pix, nifti_min.default_header(raw.shape, pix), "<")


def _sheet_case():
    raw, code, scaling, _ = _volume((67, 9, 7), "i2neg", 8)
    mask = np.zeros((67, 9, 7), np.uint8); mask[20:41, 2:6, 1:5] = 1; mask[25:30, 3, 2] = 0
    lab = np.zeros((67, 9, 7), np.int32); lab[10:30, 1:8, 0:7] = 3; lab[28:50, 4:9, 3:6] = 12
    return raw, scaling, RO.fdata(raw, scaling), np.asfortranarray(mask), np.asfortranarray(lab)


def test_render_planes_end_to_end(tmp_path):
    import torch
    from covidseg_amd import png_min, volume as V
    raw, scaling, fd, mask, lab = _sheet_case()
    vol = _nifti(raw, scaling)
    planes = [("axial", 3), ("coronal", 4), ("mip", "coronal", 2, 7), ("sagittal", 30), ("minip", "axial", 0, 7), ("axial", 0), ("mip", "sagittal", 66, 67)]
    mask_dev = torch.from_numpy(mask.reshape(-1, order="F")).cuda()
    layers = [V.Layer(mask_dev), V.Layer(lab, V.PALETTE_LESIONS, 60, 255)]
    olayers = [(mask, V.PALETTE_INFECTION, 128, 255), (lab, V.PALETTE_LESIONS, 60, 255)]
    out = tmp_path / "sheet.png"
    s = V.render_planes(vol, planes, layers, shape=(67, 9, 7), out_path=out)
    want, rects = RO.sheet(fd, PIX, planes, olayers, V.WINDOWS["lung"], V.BONE)
    assert [(t.x0, t.y0, t.w, t.h) for t in s.tiles] == rects and [t.plane for t in s.tiles] == planes
    assert (s.tiles[0].w, s.tiles[0].h) == (67, 9) and (s.tiles[1].w, s.tiles[1].h) == (67, 25) and (s.tiles[3].w, s.tiles[3].h) == (9, 25)          # 7 x 2.5 / 0.7 = 25: the physical aspect
    assert s.mm_per_px == 0.7 and s.tiles[1].mm_per_px == pytest.approx((0.7, 0.7)) and s.window == V.WINDOWS["lung"] and s.launches == 4          # one call for the plain planes, one per projection
    assert s.image.dtype == np.uint8 and s.image.shape == want.shape and np.array_equal(s.image, want)
    assert np.array_equal(png_min.read(out), want)
    # roi="layers", "minmax", nearest, another table, more columns, a device result
    s2 = V.render_planes(vol, planes[:5], layers, window="minmax", cmap="gray", roi="layers", cols=5, gap=0, background=(3, 2, 1), interp="nearest", mm_per_px=0.35,
                         shape=(67, 9, 7), return_device=True)
    roi = RO.layers_roi(mask, mask.shape, planes[:5])
    assert s2.roi == roi == ((12, 49), (0, 9), (0, 7)) and s2.window == RO.minmax_window(fd)
    want2, rects2 = RO.sheet(fd, PIX, planes[:5], olayers, RO.minmax_window(fd), V.GRAY, mm_per_px=0.35, roi=roi, cols=5, gap=0, background=(3, 2, 1), interp=0)
    assert s2.image.is_cuda and [(t.x0, t.y0, t.w, t.h) for t in s2.tiles] == rects2 and np.array_equal(s2.image.cpu().numpy(), want2)
    s3 = V.render_planes(fd.astype(np.float32), [("axial", 2)], tile_size=(11, 5), window=(-800.0, 200.5))          # a bare array: 1 mm voxels, no layers
    want3, _ = RO.sheet(fd.astype(np.float32).astype(np.float64), (1.0, 1.0, 1.0), [("axial", 2)], (), (-800.0, 200.5), V.BONE, tile_size=(11, 5))
    assert np.array_equal(s3.image, want3)


def test_render_planes_splits_65_tiles_into_two_launches():
    from covidseg_amd import volume as V
    raw, scaling, fd, mask, lab = _sheet_case()
    planes = [("axial", k % 7) for k in range(60)] + [("coronal", k) for k in range(5)]
    s = V.render_planes(_nifti(raw, scaling), planes, [mask], tile_size=(5, 3), cols=9, gap=1)
    want, rects = RO.sheet(fd, PIX, planes, [(mask, V.PALETTE_INFECTION, 128, 255)], V.WINDOWS["lung"], V.BONE, tile_size=(5, 3), cols=9, gap=1)
    assert s.launches == 2 and len(s.tiles) == 65 and np.array_equal(s.image, want)


def test_project_volume_end_to_end():
    import torch
    from covidseg_amd import volume as V
    raw, scaling, fd, mask, lab = _sheet_case()
    vol = _nifti(raw, scaling)
    lab_dev = torch.from_numpy(lab.reshape(-1, order="F")).cuda()
    for axis, slab, mode in ((0, None, "max"), ("coronal", (2, 7), "min"), (2, (6, 7), "max")):
        ax = V.VIEWS[axis] if isinstance(axis, str) else axis
        a, b = slab or (0, fd.shape[ax])
        plane, (pm, none, pl) = V.project_volume(vol, axis, slab, mode, [mask, None, V.Layer(lab_dev)], shape=(67, 9, 7))
        assert plane.dtype == np.float64 and np.array_equal(plane, RO.project(fd, ax, a, b, mode == "min")) and none is None
        assert pm.dtype == np.uint8 and pl.dtype == np.int32 and np.array_equal(pm, RO.project_labels(mask, ax, a, b)) and np.array_equal(pl, RO.project_labels(lab, ax, a, b))


# ---- segment_volume(render=) ---------------------------------------------------------------------------------------------------------------------------------
def _want_sheet(res, ct_path, lung, n=6, **kw):
    from covidseg_amd import nifti_min, volume as V
    fd = nifti_min.read(ct_path).get_fdata()
    keys = RO.key_slices(res.counts, n) or [fd.shape[2] // 2]
    planes = [("axial", z) for z in keys] + [("mip", "coronal", 0, fd.shape[1])]
    layers = [(res.mask, V.PALETTE_INFECTION, 128, 255)] + ([((lung != 0).astype(np.uint8), V.PALETTE_LUNG, 0, 255)] if lung is not None else [])
    return planes, RO.sheet(fd, tuple(float(v) for v in res.pixdim), planes, layers, kw.pop("window", V.WINDOWS["lung"]), kw.pop("table", V.BONE), **kw)


def test_segment_volume_draws_the_sheet(tmp_path):
    from test_gpu_lungside import SIZE, _patient, _Stub, _threshold
    from covidseg_amd import png_min, volume as V
    paths, lung, pix = _patient(tmp_path)
    stub = _Stub(0.9, 0.35)
    kw = dict(lung_mask=paths[1], threshold=_threshold(paths, stub), batch_size=8, img_size=SIZE, min_lesion_ml=0.05)
    plain = V.segment_volume(paths[0], stub, **kw)
    assert plain.sheet is None and "render" not in plain.seconds
    out = tmp_path / "sheet.png"
    res = V.segment_volume(paths[0], stub, render={"out_path": out}, **kw)
    for k, v in plain.__dict__.items():                             # render= changes nothing else
        if k not in ("seconds", "sheet"):
            assert V._same(v, res.__dict__[k]) or v == res.__dict__[k], k
    planes, (want, rects) = _want_sheet(res, paths[0], lung)
    assert res.mask.any() and len(planes) == 7 and [t.plane for t in res.sheet.tiles] == planes and res.seconds["render"] > 0.0
    assert [(t.x0, t.y0, t.w, t.h) for t in res.sheet.tiles] == rects and np.array_equal(res.sheet.image, want)
    assert np.array_equal(png_min.read(out), want)
    assert (want == (255, 0, 0)).all(-1).any() and (want == (0, 255, 255)).all(-1).any()          # the solid edge of the infection, the lungs' outline
    res = V.segment_volume(paths[0], stub, render={"n": 2, "window": "mediastinum", "interp": "nearest", "cols": 3}, **{**kw, "lung_mask": None, "min_lesion_ml": None})
    planes, (want, rects) = _want_sheet(res, paths[0], None, 2, window=V.WINDOWS["mediastinum"], interp=0, cols=3)
    assert len(planes) == 3 and np.array_equal(res.sheet.image, want)
    res = V.segment_volume(paths[0], stub, render=True, **{**kw, "threshold": 2.0, "min_lesion_ml": None})          # nothing is infected: the middle slice
    assert not res.mask.any() and [t.plane for t in res.sheet.tiles] == [("axial", 10), ("mip", "coronal", 0, SIZE)]
    assert np.array_equal(res.sheet.image, _want_sheet(res, paths[0], lung)[1][0])


def test_segment_volume_ensemble_draws_the_sheet(tmp_path):
    from test_gpu_lungside import SIZE, _patient, _Stub, _threshold
    from covidseg_amd import volume as V
    paths, lung, pix = _patient(tmp_path)
    stubs = [_Stub(0.9, 0.35), _Stub(0.6, 0.8)]
    kw = dict(tta=("id", "hflip"), combine="majority", lung_mask=paths[1], threshold=_threshold(paths, stubs[0]), batch_size=8, img_size=SIZE)
    plain = V.segment_volume_ensemble(paths[0], stubs, **kw)
    res = V.segment_volume_ensemble(paths[0], stubs, render={"n": 3}, **kw)
    assert plain.sheet is None and np.array_equal(res.mask, plain.mask) and np.array_equal(res.votes, plain.votes) and res.mask.any()
    assert np.array_equal(res.sheet.image, _want_sheet(res, paths[0], lung, 3)[1][0])

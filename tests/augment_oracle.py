"""Float64 numpy restatement of the augmentation (augment.py's module docstring states the semantics): the composed inverse map of one sample built with
explicit 3x3 products, the bilinear warp with zero taps outside the source (scipy's mode="grid-constant"), and the nearest-neighbour warp
(floor(s + 0.5), 0 outside).  The warps read the float32 table the kernel reads, so the kernel's only error source is its own arithmetic."""
import math

import numpy as np


def step_matrix(step, h, w, sx=1.0, sy=1.0, tx=0.0, ty=0.0, rot=0.0, shear=0.0):
    """Forward 3x3 map of one step: "fliplr", "flipud" or "affine" (tx, ty as fractions of W, H; rot, shear in degrees)."""
    if step == "fliplr":
        return np.array([[-1.0, 0.0, w - 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    if step == "flipud":
        return np.array([[1.0, 0.0, 0.0], [0.0, -1.0, h - 1.0], [0.0, 0.0, 1.0]])
    r, s = math.radians(rot), math.radians(shear)
    a = np.array([[sx * math.cos(r), -sy * math.sin(r + s), tx * w], [sx * math.sin(r), sy * math.cos(r + s), ty * h], [0.0, 0.0, 1.0]])
    cx, cy = w / 2.0 - 0.5, h / 2.0 - 0.5
    t_c = np.array([[1.0, 0.0, cx], [0.0, 1.0, cy], [0.0, 0.0, 1.0]])
    t_mc = np.array([[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, 1.0]])
    return t_c @ a @ t_mc


def sample_inverse(draws, k, h, w):
    """float64 [2, 3] inverse map of sample k of a policy.sample() record: steps in the sample's order, forward map F3 . F2 . F1, then inverted."""
    names = ("fliplr", "flipud", "affine")
    on = (bool(draws.fliplr[k]), bool(draws.flipud[k]), bool(draws.affine[k]))
    fwd = np.eye(3)
    for j in range(3):
        st = int(draws.order[k, j])
        if on[st]:
            m = step_matrix(names[st], h, w, draws.scale_x[k], draws.scale_y[k], draws.translate_x[k], draws.translate_y[k], draws.rotate[k], draws.shear[k])
            fwd = m @ fwd
    return np.linalg.inv(fwd)[:2]


def _coords(row, h, w):
    m = np.asarray(row, np.float32).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return m[0] * xx + m[1] * yy + m[2], m[3] * xx + m[4] * yy + m[5]


def warp_bilinear(img, row):
    """img [h, w, c] (any float), row = the float32 [6] inverse map -> float64 [h, w, c]; taps outside the source read 0."""
    img = np.asarray(img, np.float64)
    if img.ndim == 2:
        img = img[..., None]
    h, w = img.shape[:2]
    xs, ys = _coords(row, h, w)
    x0, y0 = np.floor(xs), np.floor(ys)
    ax, ay = (xs - x0)[..., None], (ys - y0)[..., None]
    out = np.zeros(img.shape, np.float64)
    for dy, wy in ((0, 1 - ay), (1, ay)):
        for dx, wx in ((0, 1 - ax), (1, ax)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            v = np.zeros(img.shape, np.float64)
            v[ok] = img[yi[ok].astype(np.int64), xi[ok].astype(np.int64)]
            out += wx * wy * v
    return out


def warp_nearest(mask, row):
    """mask [h, w] or [h, w, 1] -> float64 of the same shape: floor(s + 0.5), 0 outside the source."""
    m2 = np.asarray(mask, np.float64).reshape(mask.shape[0], mask.shape[1])
    h, w = m2.shape
    xs, ys = _coords(row, h, w)
    rx, ry = np.floor(xs + 0.5), np.floor(ys + 0.5)
    ok = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
    out = np.zeros((h, w), np.float64)
    out[ok] = m2[ry[ok].astype(np.int64), rx[ok].astype(np.int64)]
    return out.reshape(np.shape(mask))


def near_rounding_boundary(row, h, w, tol=1e-3):
    """[h, w] bool: pixels whose float64 source coordinate lies within `tol` px of a nearest-neighbour rounding boundary (a half-integer)."""
    xs, ys = _coords(row, h, w)
    fx, fy = xs + 0.5 - np.floor(xs + 0.5), ys + 0.5 - np.floor(ys + 0.5)
    return (np.minimum(fx, 1 - fx) < tol) | (np.minimum(fy, 1 - fy) < tol)

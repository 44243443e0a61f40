"""CPU restatement of csrc/kernels_volume.hip in numpy float64 (TEST INFRASTRUCTURE ONLY): the first half of read_nii / read_nii_demo (T1:285-297,
317-337), the paste-back of a predicted map onto the slice canvas and the way back into the patient's volume.  Every floating-point operation is
written out on its own line of arithmetic, in the order the kernels perform it; vectorised over pixels only (never over a sum's terms).

PARITY UNPINNED for cv2.resize on 64-bit float images (cv2 is absent): restates opencv/modules/imgproc/src/resize.cpp as remembered --
  * dsize == ssize: a copy;
  * INTER_AREA, both scales >= 1 and integer: resizeAreaFast_<double, double>: float64 sum over the block in source order (rows outer), times the
    float32 constant 1.f / area;
  * INTER_AREA, both scales >= 1: ResizeArea_<double, double> over the computeResizeAreaTab tables (float32 alphas, taken from
    oracle.preprocess_oracle._area_tab): per source row buf[dx] += S[sx] * alpha in table order, then per destination row sum = beta * buf for the
    first table entry and sum += beta * buf for the others;
  * otherwise: the bilinear code with INTER_AREA's coefficients: sx = floor(dx * scale), fx = float32((dx + 1) - (sx + 1) * inv_scale),
    fx = fx <= 0 ? 0 : fx - floor(fx), x clamped at both ends with fx = 0, rows clipped when read; float32 coefficients (1 - fx, fx), float64 buffers:
    D = S[sx] * a0 + S[sx + 1] * a1 horizontally, then S0 * b0 + S1 * b1.
"""
import numpy as np

from oracle import preprocess_oracle as P

F = np.float32
D = np.float64
_EPS = np.finfo(np.float64).eps


def get_fdata(raw, slope, inter):
    """nibabel's get_fdata restated: float64; slope 0 or not finite: no scaling; a non-finite inter counts as 0; else (float64(v) * slope) + inter."""
    a = np.asarray(raw).astype(D)
    slope, inter = float(slope), float(inter)
    if slope == 0.0 or not np.isfinite(slope):
        return a
    if not np.isfinite(inter):
        inter = 0.0
    a = a * D(slope)
    a = a + D(inter)
    return a


def trim_range(Z, trim=(0.2, 0.8)):
    return round(Z * trim[0]), round(Z * trim[1])


def rot90_slices(vol, z0, z1):
    """np.rot90 of [X, Y, Z] (first two axes) then slices z0..z1-1 as images [n, Y, X]: out[z, i, j] = vol[j, Y - 1 - i, z]."""
    X, Y, Z = vol.shape
    out = np.empty((z1 - z0, Y, X), vol.dtype)
    for z in range(z0, z1):
        for i in range(Y):
            out[z - z0, i, :] = vol[:, Y - 1 - i, z]
    return out


def _linear_coef(ssize, dsize, scale, inv_scale, clamp):
    ofs = np.zeros(dsize, np.int64); c0 = np.zeros(dsize, F); c1 = np.zeros(dsize, F)
    for d in range(dsize):
        s = int(np.floor(d * scale))
        f = F((d + 1) - (s + 1) * inv_scale)
        f = F(0) if f <= 0 else F(f - F(np.floor(f)))
        if clamp:
            if s < 0:
                f, s = F(0), 0
            if s >= ssize - 1:
                f, s = F(0), ssize - 1
        ofs[d] = s; c0[d] = F(F(1) - f); c1[d] = f
    return ofs, c0, c1


def resize_area_f64(img, S):
    """cv2.resize(img, (S, S), interpolation=cv2.INTER_AREA) for a 2-D float64 image."""
    src = np.ascontiguousarray(img, D)
    sh, sw = src.shape
    if sh == S and sw == S:
        return src.copy()
    inv_x, inv_y = S / sw, S / sh
    scale_x, scale_y = 1.0 / inv_x, 1.0 / inv_y
    if scale_x >= 1 and scale_y >= 1:
        isx, isy = int(np.rint(scale_x)), int(np.rint(scale_y))
        if abs(scale_x - isx) < _EPS and abs(scale_y - isy) < _EPS:
            s = np.zeros((S, S), D)
            for ky in range(isy):
                for kx in range(isx):
                    s = s + src[ky:ky + S * isy:isy, kx:kx + S * isx:isx]
            return s * D(F(F(1) / F(isx * isy)))
        xtab, ytab = P._area_tab(sw, S, scale_x), P._area_tab(sh, S, scale_y)
        buf = np.zeros((sh, S), D)
        for di, si, a in xtab:
            buf[:, di] = buf[:, di] + src[:, si] * D(a)
        out = np.zeros((S, S), D)
        prev = -1
        for di, si, b in ytab:
            if di != prev:
                out[di] = D(b) * buf[si]; prev = di
            else:
                out[di] = out[di] + D(b) * buf[si]
        return out
    xo, a0, a1 = _linear_coef(sw, S, scale_x, inv_x, True)
    yo, b0, b1 = _linear_coef(sh, S, scale_y, inv_y, False)
    x1 = np.minimum(xo + 1, sw - 1)
    rows = src[:, xo] * a0.astype(D)[None, :] + src[:, x1] * a1.astype(D)[None, :]
    r0 = np.clip(yo, 0, sh - 1); r1 = np.clip(yo + 1, 0, sh - 1)
    return rows[r0] * b0.astype(D)[:, None] + rows[r1] * b1.astype(D)[:, None]


def _u8_trunc(a):
    """np.uint8(a) on float64 as x86 numpy does it: truncation toward zero, NaN -> 0 (written out so that no platform warning decides it)."""
    a = np.asarray(a, D)
    return np.where(np.isnan(a), 0, np.trunc(np.nan_to_num(a, nan=0.0))).astype(np.int64).astype(np.uint8)


def normalise(img):
    """T1:336-337: (img - xmin)/(xmax - xmin) in float64; max == min gives numpy's 0/0 = NaN."""
    mn, mx = img.min(), img.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return (img - mn) / (mx - mn), mn, mx


def slices_f64(raw, slope, inter, z0, z1, S):
    """-> dict(img64 [n,S,S] the resized float64 slices, f32, u8, lung, uniform [n] int32, minmax [n,2]) for slices z0..z1-1 of the raw [X, Y, Z] volume."""
    vol = get_fdata(raw, slope, inter)
    sl = rot90_slices(vol, z0, z1)
    n = z1 - z0
    out = {"img64": np.zeros((n, S, S), D), "f32": np.zeros((n, S, S), F), "u8": np.zeros((n, S, S), np.uint8), "lung": np.zeros((n, S, S), np.uint8),
           "uniform": np.zeros(n, np.int32), "minmax": np.zeros((n, 2), D)}
    for i in range(n):
        out["uniform"][i] = int(np.unique(sl[i]).size == 1)
        img = resize_area_f64(sl[i], S)
        out["img64"][i] = img
        nrm, mn, mx = normalise(img)
        out["minmax"][i] = (mn, mx)
        out["f32"][i] = nrm.astype(F)
        out["u8"][i] = _u8_trunc(nrm * 255)
        lung = nrm.copy()
        lung[lung > 0] = 1                                          # T1:341
        out["lung"][i] = _u8_trunc(lung * 255)
    return out


def bilerp(p, u, v, dtype=F):
    """Bilinear sample of p [h, w] at float64 coordinates (u along x, v along y), half-pixel centres already applied by the caller, clamped to the
    edge.  The blend in `dtype` arithmetic in this order: fx = dtype(u - floor(u)); top = p00 + (p01 - p00) * fx; bot = p10 + (p11 - p10) * fx;
    value = top + (bot - top) * fy (each difference, product and sum rounded on its own; a constant map stays that constant exactly)."""
    h, w = p.shape
    u = np.asarray(u, D); v = np.asarray(v, D)
    fu, fv = np.floor(u), np.floor(v)
    fx, fy = (u - fu).astype(dtype), (v - fv).astype(dtype)
    xi, yi = fu.astype(np.int64), fv.astype(np.int64)
    x0, x1 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    y0, y1 = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    q = p.astype(dtype)
    p00, p01, p10, p11 = q[y0, x0], q[y0, x1], q[y1, x0], q[y1, x1]
    top = (p00 + ((p01 - p00).astype(dtype) * fx).astype(dtype)).astype(dtype)
    bot = (p10 + ((p11 - p10).astype(dtype) * fx).astype(dtype)).astype(dtype)
    return (top + ((bot - top).astype(dtype) * fy).astype(dtype)).astype(dtype)


def paste_back(prob, rects, S, dtype=F):
    """prob [n, d, d] -> canvas [n, S, S]: rects [n, 2, 4] = (x, y, w, h) of the two lungs (w <= 0 or h <= 0: absent; None or both absent: the whole canvas)."""
    prob = np.asarray(prob, F)
    n, d, _ = prob.shape
    out = np.zeros((n, S, S), dtype)
    r, c = np.mgrid[0:S, 0:S]
    for i in range(n):
        R = np.zeros((2, 4), np.int64) if rects is None else np.asarray(rects[i], np.int64).reshape(2, 4)
        present = [k for k in range(2) if R[k, 2] > 0 and R[k, 3] > 0]
        if not present:
            out[i] = bilerp(prob[i], (c + 0.5) * d / S - 0.5, (r + 0.5) * d / S - 0.5, dtype)
            continue
        for k in present:
            x, y, w, h = (int(t) for t in R[k])
            inside = (c >= x) & (c < x + w) & (r >= y) & (r < y + h)
            u = (c - x + 0.5) * 125.0 / w - 0.5 + 125.0 * k
            v = (r - y + 0.5) * 250.0 / h - 0.5
            val = bilerp(prob[i], (u + 0.5) * d / 250.0 - 0.5, (v + 0.5) * d / 250.0 - 0.5, dtype)
            out[i] = np.where(inside, np.fmax(out[i], val), out[i])
    return out


def unslice(canvas, t, shape, z0, z1, dtype=F):
    """canvas [z1 - z0, S, S] -> (mask uint8 [X, Y, Z] with (p > t), counts int64 [z1 - z0], p [n, Y, X] the resampled probabilities)."""
    X, Y, Z = shape
    canvas = np.asarray(canvas)
    n, S, _ = canvas.shape
    assert n == z1 - z0
    i, j = np.mgrid[0:Y, 0:X]
    v = (i + 0.5) * S / Y - 0.5
    u = (j + 0.5) * S / X - 0.5
    mask = np.zeros((X, Y, Z), np.uint8)
    counts = np.zeros(n, np.int64)
    ps = np.zeros((n, Y, X), dtype)
    for k in range(n):
        p = bilerp(canvas[k], u, v, dtype)
        ps[k] = p
        m = (p > dtype(t)).astype(np.uint8)                          # image [Y, X]: m[i, j] -> vol[x = j, y = Y - 1 - i]
        mask[:, :, z0 + k] = m[::-1, :].T
        counts[k] = int(m.sum())
    return mask, counts, ps

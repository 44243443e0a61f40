"""numpy restatement of csrc/kernels_render.hip and of volume.render_planes' sheet: every definition as whole-array operations on the decoded
volume, so that the device's canvas can be compared with array_equal.  Nothing here follows the kernels' loops: a tile is sampled with index vectors, the outline is
a comparison of shifted arrays, the blend one integer expression.

    fdata(raw, scaling)                      get_fdata(): (float64(v) * slope) + inter
    project(fd, axis, a, b, mode)            np.fmax.reduce / np.fmin.reduce over the slab, the collapsed axis kept with extent 1
    project_labels(lab, axis, a, b)          the largest label of every column
    plane_image(vol, axis, index, roi)       np.rot90 of the plane inside the region: the image a tile samples
    draw_tile / draw_canvas                  unet_vol_render
    key_slices, tile_pixels, layout, sheet   the host side of render_planes
"""
import numpy as np

IN_PLANE = ((1, 2), (0, 2), (0, 1))
VIEWS = {"sagittal": 0, "coronal": 1, "axial": 2}


def fdata(raw, scaling=None):
    a = np.asarray(raw).astype(np.float64)
    if scaling is not None:
        a = a * np.float64(scaling[0])
        a = a + np.float64(scaling[1])
    return a


def project(fd, axis, a, b, mode):
    slab = np.take(fd, np.arange(a, b), axis=axis)
    return (np.fmin if mode else np.fmax).reduce(slab, axis=axis, keepdims=True)


def project_labels(lab, axis, a, b):
    return np.take(lab, np.arange(a, b), axis=axis).max(axis=axis, keepdims=True)


def whole(shape):
    return tuple((0, int(n)) for n in shape)


def plane_image(vol, axis, index, roi):
    """row i runs against the second in-plane axis, column j along the first"""
    sl = [slice(lo, hi) for lo, hi in roi]
    sl[axis] = index
    return np.rot90(vol[tuple(sl)])


def near_index(w, n):
    j = np.arange(w)
    return np.minimum(np.floor((j + 0.5) * n / w).astype(np.int64), n - 1)


def sample_nearest(img, w, h):
    return img[np.ix_(near_index(h, img.shape[0]), near_index(w, img.shape[1]))]


def _taps(w, n):
    u = (np.arange(w) + 0.5) * n / w - 0.5
    f = np.floor(u)
    k = f.astype(np.int64)
    return np.clip(k, 0, n - 1), np.clip(k + 1, 0, n - 1), u - f


def sample_linear(img, w, h):
    r0, r1, fy = _taps(h, img.shape[0])
    c0, c1, fx = _taps(w, img.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        p00, p01, p10, p11 = img[np.ix_(r0, c0)], img[np.ix_(r0, c1)], img[np.ix_(r1, c0)], img[np.ix_(r1, c1)]
        top = p00 + (p01 - p00) * fx[None, :]
        bot = p10 + (p11 - p10) * fx[None, :]
        return top + (bot - top) * fy[:, None]


def grey(val, lo, hi):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = (val - np.float64(lo)) / (np.float64(hi) - np.float64(lo))
        g = np.floor(t * 255.0 + 0.5)
    g = np.where(t >= 1.0, 255.0, g)
    g = np.where(t > 0.0, g, 0.0)                                   # t <= 0, and NaN
    return g.astype(np.uint8)


def outline(L):
    """a pixel whose left, right, upper or lower neighbour in the tile holds another label; outside the tile: 0"""
    P = np.pad(L, 1)
    return (P[1:-1, :-2] != L) | (P[1:-1, 2:] != L) | (P[:-2, 1:-1] != L) | (P[2:, 1:-1] != L)


def blend(rgb, colour, a):
    a = np.asarray(a, np.int64)[..., None]
    return ((colour.astype(np.int64) * a + rgb.astype(np.int64) * (255 - a) + 127) // 255).astype(np.uint8)


def apply_layer(rgb, L, palette, fill_alpha, outline_alpha):
    L = L.astype(np.int64)
    P = palette.shape[0]
    on = L > 0
    colour = palette[np.where(on, 1 + (L - 1) % (P - 1), 0)]
    a = np.where(outline(L), outline_alpha, fill_alpha)
    return np.where(on[..., None], blend(rgb, colour, a), rgb)


def draw_tile(fd, layers, axis, index, w, h, roi, lo, hi, table, interp):
    """layers: (label volume, palette, fill_alpha, outline_alpha) -> uint8 [h, w, 3]"""
    img = plane_image(fd, axis, index, roi)
    val = sample_linear(img, w, h) if interp else sample_nearest(img, w, h)
    rgb = table[grey(val, lo, hi)]
    for lab, palette, fa, oa in layers:
        rgb = apply_layer(rgb, sample_nearest(plane_image(lab, axis, index, roi), w, h), palette, fa, oa)
    return rgb


def draw_canvas(canvas, fd, layers, tiles, roi, lo, hi, table, interp, background=None):
    """unet_vol_render on a copy of `canvas`: background (r, g, b) fills what no tile covers, None leaves it; tiles: (axis, index, x0, y0, w, h)"""
    out = canvas.copy()
    if background is not None:
        out[:] = np.asarray(background, np.uint8)
    for axis, index, x0, y0, w, h in tiles:
        out[y0:y0 + h, x0:x0 + w] = draw_tile(fd, layers, axis, index, w, h, roi, lo, hi, table, interp)
    return out


# ---- the host side of render_planes ------------------------------------------------------------------------------------------------------------------
def key_slices(counts, n=6):
    c = np.asarray(counts)
    order = sorted(range(c.size), key=lambda z: (-int(c[z]), z))
    return sorted([z for z in order if c[z] > 0][:n])


def tile_pixels(extent, spacing, mm):
    return max(1, round(extent * spacing / mm))


def layout(sizes, cols=None, gap=2):
    k = len(sizes)
    cols = int(np.ceil(np.sqrt(k))) if cols is None else cols
    cols = max(1, min(cols, k))
    rows = -(-k // cols)
    grid = [[sizes[r * cols + c] if r * cols + c < k else (0, 0) for c in range(cols)] for r in range(rows)]
    colw = [max(grid[r][c][0] for r in range(rows)) for c in range(cols)]
    rowh = [max(grid[r][c][1] for c in range(cols)) for r in range(rows)]
    xs = gap + np.concatenate([[0], np.cumsum(np.asarray(colw) + gap)])
    ys = gap + np.concatenate([[0], np.cumsum(np.asarray(rowh) + gap)])
    return [(int(xs[i % cols]), int(ys[i // cols])) for i in range(k)], int(ys[-1]), int(xs[-1])


def minmax_window(fd):
    f = fd[np.isfinite(fd)]
    return float(f.min()), float(f.max())


def layers_roi(first_layer, shape, planes, margin=8):
    nz = np.nonzero(first_layer)
    box = [(0, n) for n in shape] if nz[0].size == 0 else [(max(0, int(i.min()) - margin), min(n, int(i.max()) + 1 + margin)) for i, n in zip(nz, shape)]
    for p in planes:
        if len(p) == 2:
            ax = VIEWS[p[0]]
            box[ax] = (min(box[ax][0], p[1]), max(box[ax][1], p[1] + 1))
    return tuple(box)


def sheet(fd, pixdim, planes, layers=(), window=(-1350.0, 150.0), table=None, mm_per_px=None, tile_size=None, roi=None, cols=None, gap=2, background=(0, 0, 0), interp=1):
    """render_planes -> (image uint8 [H, W, 3], [(x0, y0, w, h)]); planes and layers as render_planes takes them, roi: three ranges or None"""
    roi = whole(fd.shape) if roi is None else roi
    axes = [VIEWS[p[0]] if len(p) == 2 else VIEWS[p[1]] for p in planes]
    mm = min(pixdim[d] for ax in axes for d in IN_PLANE[ax]) if mm_per_px is None else mm_per_px
    sizes = []
    for ax in axes:
        au, av = IN_PLANE[ax]
        sizes.append(tuple(tile_size) if tile_size is not None else
                     (tile_pixels(roi[au][1] - roi[au][0], pixdim[au], mm), tile_pixels(roi[av][1] - roi[av][0], pixdim[av], mm)))
    pos, H, W = layout(sizes, cols, gap)
    img = np.empty((H, W, 3), np.uint8)
    img[:] = np.asarray(background, np.uint8)
    for p, ax, (x0, y0), (w, h) in zip(planes, axes, pos, sizes):
        if len(p) == 2:
            tile = draw_tile(fd, layers, ax, p[1], w, h, roi, window[0], window[1], table, interp)
        else:
            mode = {"mip": 0, "minip": 1}[p[0]]
            pfd = project(fd, ax, p[2], p[3], mode)
            pl = [(project_labels(lab, ax, p[2], p[3]), pal, fa, oa) for lab, pal, fa, oa in layers]
            proi = tuple((0, 1) if d == ax else r for d, r in enumerate(roi))
            tile = draw_tile(pfd, pl, ax, 0, w, h, proi, window[0], window[1], table, interp)
        img[y0:y0 + h, x0:x0 + w] = tile
    return img, [(x0, y0, w, h) for (x0, y0), (w, h) in zip(pos, sizes)]

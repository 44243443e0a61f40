"""CPU restatement of the binary morphology (csrc/kernels_morph.hip, covidseg_amd.volume.binary_dilation ... fill_holes, label_volume(per_slice=True)) in numpy only:
padded shifted ORs and ANDs, no scipy (tests/test_morph_host.py pins it against scipy.ndimage where that imports).

Structuring element: generate_binary_structure(3, c) = the offsets (dx, dy, dz) in {-1, 0, 1}^3 that move along at most c axes, centre included; planar: those with
dz = 0 (c = 1, 2).  One step: dilate out[v] = OR over offsets of m[v + o], erode out[v] = AND, where m outside the volume holds border_value at every step."""
import numpy as np

import components_oracle as CO
import volscore_oracle as SO


def offsets(connectivity, planar=False):
    if connectivity not in ((1, 2) if planar else (1, 2, 3)):
        raise ValueError("connectivity is 1, 2 or 3 (planar: 1 or 2)")
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in ((0,) if planar else (-1, 0, 1))
            if (dx != 0) + (dy != 0) + (dz != 0) <= connectivity]


def structure(connectivity, planar=False):
    """the 3 x 3 x 3 bool footprint scipy takes as `structure`"""
    s = np.zeros((3, 3, 3), bool)
    for dx, dy, dz in offsets(connectivity, planar):
        s[1 + dx, 1 + dy, 1 + dz] = True
    return s


def step(m, offs, border_value, dilate):
    X, Y, Z = m.shape
    p = np.full((X + 2, Y + 2, Z + 2), bool(border_value))
    p[1:-1, 1:-1, 1:-1] = m
    out = np.zeros(m.shape, bool) if dilate else np.ones(m.shape, bool)
    for dx, dy, dz in offs:
        v = p[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
        out = (out | v) if dilate else (out & v)
    return out


def _iterate(mask, connectivity, iterations, border_value, planar, dilate):
    if not 1 <= iterations:
        raise ValueError("iterations >= 1")
    m = np.asarray(mask) != 0
    offs = offsets(connectivity, planar)
    for _ in range(iterations):
        m = step(m, offs, border_value, dilate)
    return m


def dilation(mask, connectivity=1, iterations=1, border_value=0, planar=False):
    return _iterate(mask, connectivity, iterations, border_value, planar, True).astype(np.uint8)


def erosion(mask, connectivity=1, iterations=1, border_value=0, planar=False):
    return _iterate(mask, connectivity, iterations, border_value, planar, False).astype(np.uint8)


def opening(mask, connectivity=1, iterations=1, border_value=0, planar=False):
    return dilation(erosion(mask, connectivity, iterations, border_value, planar), connectivity, iterations, border_value, planar)


def closing(mask, connectivity=1, iterations=1, border_value=0, planar=False):
    return erosion(dilation(mask, connectivity, iterations, border_value, planar), connectivity, iterations, border_value, planar)


OPS = {"dilate": dilation, "erode": erosion, "open": opening, "close": closing}


def dilate_mm(mask, radius_mm, pixdim=(1, 1, 1)):
    """squared distance to the foreground (volscore_oracle.edt_sq_lines: the definition of unet_vol_edt_sq) <= fl(r r)"""
    r = float(radius_mm)
    return (SO.edt_sq_lines(mask, True, pixdim) <= r * r).astype(np.uint8)


def erode_mm(mask, radius_mm, pixdim=(1, 1, 1)):
    """squared distance to the background > fl(r r); no background anywhere: +inf, everything stays (the outside is foreground)"""
    r = float(radius_mm)
    return (SO.edt_sq_lines(mask, False, pixdim) > r * r).astype(np.uint8)


def open_mm(mask, radius_mm, pixdim=(1, 1, 1)):
    return dilate_mm(erode_mm(mask, radius_mm, pixdim), radius_mm, pixdim)


def close_mm(mask, radius_mm, pixdim=(1, 1, 1)):
    return erode_mm(dilate_mm(mask, radius_mm, pixdim), radius_mm, pixdim)


def ball_footprint(radius, pixdim=(1, 1, 1)):
    """the closed ball as a footprint array (odd sizes, centred) for scipy's structure="""
    w = SO.weights(pixdim)
    n = [int(np.floor(radius / np.sqrt(w[a]))) for a in range(3)]
    g = np.ogrid[-n[0]:n[0] + 1, -n[1]:n[1] + 1, -n[2]:n[2] + 1]
    return (w[0] * (g[0] * g[0]).astype(np.float64) + w[1] * (g[1] * g[1]).astype(np.float64)) + w[2] * (g[2] * g[2]).astype(np.float64) <= float(radius) * float(radius)


def label_planar(mask, connectivity=1):
    """-> (labels int32 [X, Y, Z], n): components inside every axial slice (connectivity 1, 2 = 4, 8 neighbours), numbered over the whole volume in ascending order of the
    C-order index (x Y + y) Z + z of their first voxel.  Every slice is labelled by components_oracle.label as a one-slice volume (no dz neighbour exists there)."""
    if connectivity not in (1, 2):
        raise ValueError("planar connectivity is 1 or 2")
    fg = np.asarray(mask) != 0
    X, Y, Z = fg.shape
    out = np.zeros(fg.shape, np.int64)
    keys = []
    base = 0
    for z in range(Z):
        lab, n = CO.label(fg[:, :, z:z + 1], connectivity)
        if n == 0:
            continue
        lab = lab[:, :, 0].astype(np.int64)
        flat = lab.reshape(-1)                                        # C order over (x, y): index x Y + y
        pos = np.nonzero(flat)[0]
        first = np.full(n + 1, X * Y, np.int64)
        np.minimum.at(first, flat[pos], pos)
        keys.append(first[1:] * Z + z)
        out[:, :, z] = np.where(lab > 0, lab + base, 0)
        base += n
    if base == 0:
        return np.zeros(fg.shape, np.int32), 0
    keys = np.concatenate(keys)
    rank = np.empty(base + 1, np.int64)
    rank[0] = 0
    rank[1 + np.argsort(keys, kind="stable")] = np.arange(1, base + 1)
    return rank[out].astype(np.int32), int(base)


def fill_holes(mask, connectivity=1, planar=False):
    """the mask plus the components of its complement (under the structure's connectivity) that hold no border voxel: the six faces, planar: the four edges of a slice"""
    m = np.asarray(mask) != 0
    if m.size == 0:
        return m.astype(np.uint8)
    lab, n = label_planar(~m, connectivity) if planar else CO.label(~m, connectivity)
    touch = np.zeros(n + 1, bool)
    faces = [lab[0], lab[-1], lab[:, 0], lab[:, -1]] + ([] if planar else [lab[:, :, 0], lab[:, :, -1]])
    for f in faces:
        touch[f.reshape(-1)] = True
    touch[0] = False
    return (m | ((lab > 0) & ~touch[lab])).astype(np.uint8)


# ---- test volumes -----------------------------------------------------------------------------------------------------------------------------
def hollow_shell(shape, lo, hi):
    """a closed box shell: walls one voxel thick between the corners lo and hi (inclusive), empty inside"""
    m = np.zeros(shape, np.uint8)
    m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = 1
    m[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = 0
    return m


def open_tube(shape, lo, hi):
    """a tube along z with a square wall, closed at its far z end by a cap and OPEN at z = lo[2]: every slice through the wall holds a closed ring"""
    m = hollow_shell(shape, lo, hi)
    m[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2]] = 0
    return m

"""CPU restatement of the component step (csrc/kernels_components.hip, covidseg_amd.volume.label_volume / component_table / remove_small / keep_largest)
in numpy only: a union-find over the foreground voxels' C-order indices, written out -- no scipy, no scikit-image (tests/golden/component_goldens.npz pins it
against the real skimage.measure.label).

Numbering rule: components 1..n in ascending order of the C-order index (x Y + y) Z + z of their first voxel, which is what scikit-image and scipy return.
"""
import numpy as np


def offsets(connectivity):
    """the forward half of the neighbourhood: offsets after (0, 0, 0) in (dx, dy, dz) order that move along at most `connectivity` axes"""
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity is 1, 2 or 3")
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) > (0, 0, 0) and (dx != 0) + (dy != 0) + (dz != 0) <= connectivity:
                    out.append((dx, dy, dz))
    return out


def _edges(fg, connectivity):
    """pairs (a, b) of C-order indices of adjacent foreground voxels"""
    X, Y, Z = fg.shape
    idx = np.arange(fg.size, dtype=np.int64).reshape(fg.shape)
    ea, eb = [], []
    for dx, dy, dz in offsets(connectivity):
        def sl(d, n):
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n + min(0, d)))
        (ax, bx), (ay, by), (az, bz) = sl(dx, X), sl(dy, Y), sl(dz, Z)
        both = fg[ax, ay, az] & fg[bx, by, bz]
        ea.append(idx[ax, ay, az][both]); eb.append(idx[bx, by, bz][both])
    return np.concatenate(ea), np.concatenate(eb)


def label(mask, connectivity=1):
    """-> (labels int32 [X, Y, Z], n).  Union-find: every round hooks the larger of two adjacent roots under the smaller one (np.minimum.at), then halves every
    path until all voxels point at their root; an edge inside one tree is dropped.  A tree's root is its smallest index, so ranking the roots numbers the
    components by their first voxel."""
    fg = np.asarray(mask) != 0
    if fg.ndim != 3:
        raise ValueError("a volume is [X, Y, Z]")
    if fg.size == 0:
        return np.zeros(fg.shape, np.int32), 0
    parent = np.arange(fg.size, dtype=np.int64)
    ea, eb = _edges(fg, connectivity)
    while ea.size:
        pa, pb = parent[ea], parent[eb]
        live = pa != pb
        if not live.any():
            break
        ea, eb, pa, pb = ea[live], eb[live], pa[live], pb[live]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    flat = fg.reshape(-1)
    roots = parent[flat]
    uniq = np.unique(roots)                                           # sorted: the rank of a root is its component's number
    out = np.zeros(fg.size, np.int32)
    out[flat] = (np.searchsorted(uniq, roots) + 1).astype(np.int32)
    return out.reshape(fg.shape), int(uniq.size)


STAT_FIELDS = ("voxels", "sx", "sy", "sz", "x0", "x1", "y0", "y1", "z0", "z1")


def stats(labels, n):
    """dict of int64 arrays [n] (row i: label i + 1): voxels, coordinate sums sx sy sz, inclusive bounding box x0 x1 y0 y1 z0 z1"""
    labels = np.asarray(labels)
    x, y, z = np.nonzero(labels)
    lab = labels[x, y, z].astype(np.int64) - 1
    out = {"voxels": np.bincount(lab, minlength=n).astype(np.int64)}
    order = np.argsort(lab, kind="stable")
    starts = np.concatenate([[0], np.cumsum(out["voxels"])[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    for name, c in (("x", x), ("y", y), ("z", z)):
        c = c.astype(np.int64)[order]
        if n and (out["voxels"] == 0).any():
            raise ValueError("labels are not 1..n without gaps")
        out["s" + name] = np.add.reduceat(c, starts) if n else np.zeros(0, np.int64)
        out[name + "0"] = np.minimum.reduceat(c, starts) if n else np.zeros(0, np.int64)
        out[name + "1"] = np.maximum.reduceat(c, starts) if n else np.zeros(0, np.int64)
    return out


def min_voxels_from_ml(min_ml, pixdim):
    """the smallest voxel count whose volume reaches min_ml: ceil(min_ml * 1000 / prod(pixdim))"""
    return int(np.ceil(float(min_ml) * 1000.0 / float(np.prod(np.asarray(pixdim, np.float64)))))


def remove_small(mask, min_voxels, connectivity=1):
    """skimage.morphology.remove_small_objects(mask != 0, min_size=min_voxels, connectivity=c): components with fewer than min_voxels voxels go"""
    lab, n = label(mask, connectivity)
    keep = np.zeros(n + 1, bool)
    keep[1:] = np.bincount(lab.reshape(-1), minlength=n + 1)[1:] >= min_voxels
    return keep[lab].astype(np.uint8)


def largest(counts, k):
    """labels (1-based) of the k largest components, ties to the lower label"""
    counts = np.asarray(counts, np.int64)
    order = np.lexsort((np.arange(counts.size), -counts))
    return np.sort(order[:max(0, int(k))] + 1)


def keep_largest(mask, k=2, connectivity=1):
    lab, n = label(mask, connectivity)
    keep = np.zeros(n + 1, bool)
    keep[largest(np.bincount(lab.reshape(-1), minlength=n + 1)[1:], k)] = True
    return keep[lab].astype(np.uint8)


# ---- test volumes -----------------------------------------------------------------------------------------------------------------------------
def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def serpentine(shape):
    """a one-voxel-wide path that visits every second row of every second plane: ONE component at every connectivity, as long and winding as the volume allows"""
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8)
    flip = False                                                      # which end of the row the path is at
    for zi, z in enumerate(range(0, Z, 2)):
        ys = list(range(0, Y, 2))
        if zi % 2:
            ys = ys[::-1]
        for i, y in enumerate(ys):
            m[:, y, z] = 1
            if i + 1 < len(ys):
                lo, hi = sorted((y, ys[i + 1]))
                m[0 if flip else X - 1, lo:hi + 1, z] = 1
                flip = not flip
        if z + 2 < Z:
            m[0 if flip else X - 1, ys[-1], z:z + 3] = 1             # the end of this plane's path climbs to the next plane; the same row starts there
            flip = not flip
    return m


def spiral(shape):
    """a square spiral in every second plane, two voxels between its arms, joined to the next plane alternately at the outer end and at the centre"""
    X, Y, Z = shape
    plane = np.zeros((X, Y), np.uint8)
    x, y, dx, dy = 0, 0, 1, 0
    lo_x, hi_x, lo_y, hi_y = 0, X - 1, 0, Y - 1
    plane[0, 0] = 1
    end = (0, 0)
    while True:
        moved = False
        while lo_x <= x + dx <= hi_x and lo_y <= y + dy <= hi_y:
            x, y = x + dx, y + dy
            plane[x, y] = 1; moved = True
        end = (x, y)
        if not moved:
            break
        if (dx, dy) == (1, 0): lo_y += 2
        elif (dx, dy) == (0, 1): hi_x -= 2
        elif (dx, dy) == (-1, 0): hi_y -= 2
        else: lo_x += 2
        dx, dy = -dy, dx
        if lo_x > hi_x or lo_y > hi_y:
            break
    m = np.zeros(shape, np.uint8)
    for zi, z in enumerate(range(0, Z, 2)):
        m[:, :, z] = plane
        if z + 2 < Z:
            cx, cy = end if zi % 2 == 0 else (0, 0)
            m[cx, cy, z + 1] = 1
    return m


def checkerboard(shape):
    x, y, z = np.indices(shape)
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def ellipsoids(shape, count, noise, seed):
    """`count` random ellipsoids + salt noise of the given density (the full-size test volume)"""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8)
    for _ in range(count):
        c = rng.uniform(0, 1, 3) * (X, Y, Z)
        r = rng.uniform(3, 24, 3) * (1, 1, min(1.0, Z / max(X, 1) * 2))
        r = np.maximum(r, 1.5)
        lo = np.maximum(np.floor(c - r).astype(int), 0); hi = np.minimum(np.ceil(c + r).astype(int) + 1, (X, Y, Z))
        if (hi <= lo).any():
            continue
        gx, gy, gz = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        inside = ((gx - c[0]) / r[0]) ** 2 + ((gy - c[1]) / r[1]) ** 2 + ((gz - c[2]) / r[2]) ** 2 <= 1
        m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= inside.astype(np.uint8)
    if noise:
        m |= (rng.random(shape, dtype=np.float32) < noise).astype(np.uint8)
    return m

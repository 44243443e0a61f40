"""The thinning, the skeleton table and the label spread of csrc/kernels_skeleton.hip restated in numpy, and the slow per-voxel form that
pins the restatement (scipy.ndimage.label on every 3 x 3 x 3).

Neighbour i = (dx + 1) + 3 (dy + 1) + 9 (dz + 1) without the centre 13 is bit i (i < 13) or i - 1 (i > 13) of a uint32 code.
simple(v): the set neighbours form exactly one 26-connected component, and the clear voxels of the 18-neighbourhood that are 6-adjacent to v are not empty and lie
in one 6-connected component of the clear voxels of the 18-neighbourhood.  Here both are flood fills over tables of 26 adjacency constants.
An iteration: passes +z, -z, +y, -y, +x, -x; the candidates of a pass (set, v + d clear or outside, n26 >= 2 with endpoints / 1 without, simple) are all judged on the
image as the pass finds it; then eight sub-passes k = (x & 1) | (y & 1) << 1 | (z & 1) << 2 clear the candidates that are still simple in the current image."""
import numpy as np

OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]          # bit b <-> OFFSETS[b]
DIRECTIONS = ((0, 0, 1), (0, 0, -1), (0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0))
SIMPLE_COUNT = 25985144                                              # of the 2^26 neighbourhoods


def _adjacency():
    a26 = np.zeros(26, np.uint32); a6 = np.zeros(26, np.uint32)
    n6 = n18 = 0
    for b, p in enumerate(OFFSETS):
        k = sum(1 for v in p if v)
        n6 |= (1 << b) if k == 1 else 0
        n18 |= (1 << b) if k <= 2 else 0
        for c, q in enumerate(OFFSETS):
            if c == b:
                continue
            if max(abs(p[i] - q[i]) for i in range(3)) <= 1:
                a26[b] |= np.uint32(1 << c)
            if sum(abs(p[i] - q[i]) for i in range(3)) == 1 and sum(1 for v in q if v) <= 2 and k <= 2:
                a6[b] |= np.uint32(1 << c)
    return a26, a6, np.uint32(n6), np.uint32(n18)


ADJ26, ADJ6, N6, N18 = _adjacency()


def popcount(codes):
    c = np.asarray(codes, np.uint32)
    return np.unpackbits(c.view(np.uint8).reshape(-1, 4), axis=1).sum(1).reshape(c.shape).astype(np.int64)


def _fill(seed, inside, adj):
    """the flood fill of `seed` inside `inside`, every element on its own"""
    f = seed.copy()
    while True:
        g = np.zeros_like(f)
        for b in range(26):
            g |= np.where((f >> np.uint32(b)) & np.uint32(1), adj[b], np.uint32(0))
        g = (f | g) & inside
        if np.array_equal(g, f):
            return f
        f = g


def simple(codes):
    """codes: uint32 array -> bool array"""
    n = np.asarray(codes, np.uint32).reshape(-1) & np.uint32(0x3FFFFFF)
    low = n & (~n + np.uint32(1))
    one = (n != 0) & (_fill(low, n, ADJ26) == n)
    c = ~n & N18
    c6 = c & N6
    f = _fill(c6 & (~c6 + np.uint32(1)), c, ADJ6)
    return (one & (c6 != 0) & ((c6 & ~f) == 0)).reshape(np.shape(codes))


def codes_at(pad, coords):
    """the neighbour codes of the voxels coords [M, 3] of the image whose zero-padded copy is pad"""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    code = np.zeros(len(coords), np.uint32)
    for b, (dx, dy, dz) in enumerate(OFFSETS):
        code |= pad[coords[:, 0] + 1 + dx, coords[:, 1] + 1 + dy, coords[:, 2] + 1 + dz].astype(np.uint32) << np.uint32(b)
    return code


def thin(vol, endpoints=True, max_iterations=None):
    """-> (mask uint8 [X, Y, Z], iterations, removed int64 [iterations]); the iteration count includes the last, empty one"""
    vol = np.asarray(vol)
    X, Y, Z = vol.shape
    pad = np.zeros((X + 2, Y + 2, Z + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = vol != 0
    img = pad[1:-1, 1:-1, 1:-1]
    need = 2 if endpoints else 1
    removed = []
    while max_iterations is None or len(removed) < max_iterations:
        cleared = 0
        for dx, dy, dz in DIRECTIONS:
            border = np.argwhere(img & ~pad[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z])
            codes = codes_at(pad, border)
            cand = border[(popcount(codes) >= need) & simple(codes)]
            sub = (cand[:, 0] & 1) | ((cand[:, 1] & 1) << 1) | ((cand[:, 2] & 1) << 2)
            for k in range(8):
                c = cand[sub == k]
                if len(c) == 0:
                    continue
                c = c[simple(codes_at(pad, c))]
                pad[c[:, 0] + 1, c[:, 1] + 1, c[:, 2] + 1] = False
                cleared += len(c)
        removed.append(cleared)
        if cleared == 0:
            break
    return np.asfortranarray(img.astype(np.uint8)), len(removed), np.asarray(removed, np.int64)


# ---- the slow form: scipy.ndimage.label on every 3 x 3 x 3 --------------------------------------------------------------------------------------------
def cube_of(code):
    """a code -> bool [3, 3, 3] indexed [dx + 1, dy + 1, dz + 1], the centre clear"""
    c = np.zeros((3, 3, 3), bool)
    for b, (dx, dy, dz) in enumerate(OFFSETS):
        c[dx + 1, dy + 1, dz + 1] = (int(code) >> b) & 1
    return c


def simple_slow(cube):
    from scipy import ndimage
    cube = np.array(cube, bool)
    cube[1, 1, 1] = False
    if ndimage.label(cube, np.ones((3, 3, 3), bool))[1] != 1:
        return False
    n18 = ndimage.generate_binary_structure(3, 2)
    clear = ~cube & n18
    clear[1, 1, 1] = False
    lab = ndimage.label(clear, ndimage.generate_binary_structure(3, 1))[0]
    faces = [lab[p] for p in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)) if clear[p]]
    return len(faces) > 0 and len(set(faces)) == 1


def thin_slow(vol, endpoints=True, max_iterations=None):
    vol = np.asarray(vol)
    X, Y, Z = vol.shape
    pad = np.zeros((X + 2, Y + 2, Z + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = vol != 0
    removed = []
    while max_iterations is None or len(removed) < max_iterations:
        cleared = 0
        for dx, dy, dz in DIRECTIONS:
            cand = []
            for x, y, z in np.argwhere(pad[1:-1, 1:-1, 1:-1]):
                if pad[x + 1 + dx, y + 1 + dy, z + 1 + dz]:
                    continue
                cube = pad[x:x + 3, y:y + 3, z:z + 3]
                if int(cube.sum()) - 1 >= (2 if endpoints else 1) and simple_slow(cube):
                    cand.append((x, y, z))
            for k in range(8):
                for x, y, z in cand:
                    if ((x & 1) | ((y & 1) << 1) | ((z & 1) << 2)) == k and simple_slow(pad[x:x + 3, y:y + 3, z:z + 3]):
                        pad[x + 1, y + 1, z + 1] = False
                        cleared += 1
        removed.append(cleared)
        if cleared == 0:
            break
    return np.asfortranarray(pad[1:-1, 1:-1, 1:-1].astype(np.uint8)), len(removed), np.asarray(removed, np.int64)


# ---- the table and the label spread -----------------------------------------------------------------------------------------------------------------
def table(vol, d2=None):
    """-> (index int32 [n] ascending, neighbour codes uint32 [n], d2 at those voxels or None)"""
    vol = np.asarray(vol)
    pad = np.zeros(tuple(s + 2 for s in vol.shape), bool)
    pad[1:-1, 1:-1, 1:-1] = vol != 0
    idx = np.flatnonzero((vol != 0).reshape(-1, order="F"))
    coords = np.stack(np.unravel_index(idx, vol.shape, order="F"), 1)
    vals = None if d2 is None else np.asarray(d2, np.float64).reshape(-1, order="F")[idx]
    return idx.astype(np.int32), codes_at(pad, coords), vals


def label_spread(arrival, labels, connectivity=3, first=1, n=None):
    """a voxel with arrival == s takes the smallest non-zero label among its neighbours (moving along at most `connectivity` axes) whose arrival == s - 1"""
    arrival = np.asarray(arrival).astype(np.int64)
    out = np.array(labels, np.int32, order="F")
    X, Y, Z = arrival.shape
    reached = arrival[arrival != 0xFFFF]
    last = int(reached.max()) if reached.size else 0
    if n is not None:
        last = min(last, first + n - 1)
    big = np.iinfo(np.int32).max
    pa = np.full((X + 2, Y + 2, Z + 2), -5, np.int64)
    pa[1:-1, 1:-1, 1:-1] = arrival
    for s in range(first, last + 1):
        pl = np.zeros((X + 2, Y + 2, Z + 2), np.int32)
        pl[1:-1, 1:-1, 1:-1] = out
        best = np.full((X, Y, Z), big, np.int32)
        for dx, dy, dz in OFFSETS:
            if (dx != 0) + (dy != 0) + (dz != 0) > connectivity:
                continue
            a = pa[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
            l = pl[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
            best = np.minimum(best, np.where((a == s - 1) & (l != 0), l, big))
        take = (arrival == s) & (best != big)
        out[take] = best[take]
    return out


# ---- phantoms: a voxel belongs when its centre lies within the stated distance ----------------------------------------------------------------------------
def _segment_distance(shape, a, b):
    g = np.stack(np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij"), -1)
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    t = np.clip(((g - a) @ (b - a)) / float((b - a) @ (b - a)), 0.0, 1.0)
    return np.sqrt((((g - a) - t[..., None] * (b - a)) ** 2).sum(-1))


def tubes(shape, segments):
    """segments: (a, b, radius)"""
    m = np.zeros(shape, bool)
    for a, b, r in segments:
        m |= _segment_distance(shape, a, b) <= r
    return np.asfortranarray(m.astype(np.uint8))


def three_armed_tube():
    return tubes((40, 36, 44), (((20, 18, 4), (20, 18, 22), 3.5), ((20, 18, 22), (8, 14, 38), 2.5), ((20, 18, 22), (32, 22, 38), 2.5)))


def torus():
    x, y, z = np.meshgrid(np.arange(33) - 16.0, np.arange(33) - 16.0, np.arange(13) - 6.0, indexing="ij")
    return np.asfortranarray(((np.sqrt(x * x + y * y) - 10.0) ** 2 + z * z <= 9.0).astype(np.uint8))


def ball():
    x, y, z = np.meshgrid(*(np.arange(15) - 7.0,) * 3, indexing="ij")
    return np.asfortranarray((x * x + y * y + z * z <= 25.0).astype(np.uint8))


def blobs(shape, seed, fill=0.33):
    """smoothed-noise blobs at about `fill`"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal(shape), 1.2, mode="constant")
    return np.asfortranarray((f > np.quantile(f, 1.0 - fill)).astype(np.uint8))


def degrees(vol):
    vol = np.asarray(vol)
    _, codes, _ = table(vol)
    return popcount(codes)

"""Two statements of the watershed definition of DESIGN.md section 4ah (include/unet_hip.h, csrc/kernels_watershed.hip), without a device:
  fixed_point(...)   the synchronous whole-volume numpy iteration to its fixed point (every voxel from the previous state, until nothing changes)
  by_heap(...)       an independent priority-queue restatement: Dijkstra on H, then Dijkstra on (steps, label) over the tight edges; one Dijkstra on (dist, label) for "sum"
and the one-phase prototype packed_one_phase(...) (height << 24 | label in one key) whose disagreement with the heap is why the ABI has phases; the contents of the tests;
and split_lesions restated over scipy.  Volumes are [X, Y, Z]; costs uint32 (as int64 / uint64 arrays here), markers int32, mask bool or None."""
import heapq

import numpy as np
from scipy import ndimage

UNREACHED = np.uint64(0xFFFFFFFFFFFFFFFF)
H_UNREACHED = 0xFFFFFFFF
DIST_MAX = (1 << 40) - 2
LABEL_MAX = (1 << 24) - 1
OFFSETS = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))


def offsets(conn):
    return tuple(o for o in OFFSETS if sum(v != 0 for v in o) <= conn)


def _shifted(a, off, fill):
    """b[v] = a[v + off], fill outside the volume"""
    out = np.full_like(a, fill)
    src, dst = [], []
    for n, o in zip(a.shape, off):
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n - max(o, 0)))
    if all(s.stop > s.start for s in src):
        out[tuple(dst)] = a[tuple(src)]
    return out


def _inputs(cost, markers, mask):
    cost = np.asarray(cost).astype(np.uint64)
    markers = np.asarray(markers).astype(np.int64)
    inmask = np.ones(cost.shape, bool) if mask is None else np.asarray(mask) != 0
    valid = (markers >= 1) & (markers <= LABEL_MAX)
    invalid = int(((markers != 0) & ~valid).sum())
    seeds = valid & inmask
    return cost, markers, inmask, seeds, invalid


def _iterate(key, live, candidate, conn):
    """key <- min(key, candidates) on the live voxels until nothing changes -> (key, sweeps including the one that changed nothing)"""
    sweeps = 0
    while True:
        best = key.copy()
        for off in offsets(conn):
            cand = candidate(_shifted(key, off, UNREACHED), off)
            best = np.where(live & (cand < best), cand, best)
        sweeps += 1
        if np.array_equal(best, key):
            return key, sweeps
        key = best


def fixed_point(cost, markers, mask=None, conn=1, rule="max"):
    """-> dict(labels int32, counts (reached, unreached in mask, overflowed, invalid), sweeps tuple, and height / steps uint32 ("max") or distance uint64 ("sum"))"""
    cost, markers, inmask, seeds, invalid = _inputs(cost, markers, mask)
    live = inmask & ~seeds
    seed_label = np.where(seeds, markers, 0).astype(np.uint64)
    if rule == "sum":
        key = np.where(seeds, seed_label, UNREACHED)

        def cand(kn, off):
            ok = kn != UNREACHED
            dist = np.where(ok, kn >> np.uint64(24), np.uint64(0)) + cost
            ok &= dist <= np.uint64(DIST_MAX)
            return np.where(ok, (dist << np.uint64(24)) | (kn & np.uint64(0xFFFFFF)), UNREACHED)
        key, sweeps = _iterate(key, live, cand, conn)
        got = key != UNREACHED
        beside = np.zeros(cost.shape, bool)
        for off in offsets(conn):
            beside |= _shifted(got, off, False)
        return dict(labels=np.where(got, key & np.uint64(0xFFFFFF), 0).astype(np.int32), distance=key >> np.uint64(24), sweeps=(sweeps,),
                    counts=(int(got.sum()), int((inmask & ~got).sum()), int((inmask & ~got & beside).sum()), invalid))
    H = np.where(seeds, cost, UNREACHED)
    H, s1 = _iterate(H, live, lambda hn, off: np.where(hn != UNREACHED, np.maximum(hn, cost), UNREACHED), conn)
    key = np.where(seeds, seed_label, UNREACHED)
    finite = H != UNREACHED

    def cand(kn, off):
        hn = _shifted(H, off, UNREACHED)
        tight = finite & (kn != UNREACHED) & (np.maximum(hn, cost) == H)
        return np.where(tight, kn + np.uint64(1 << 32), UNREACHED)
    key, s2 = _iterate(key, live, cand, conn)
    got = key != UNREACHED
    assert np.array_equal(got, finite)                                   # every voxel with a finite H receives a label
    return dict(labels=np.where(got, key & np.uint64(0xFFFFFFFF), 0).astype(np.int32), height=np.where(finite, H, H_UNREACHED).astype(np.uint32),
                steps=np.where(got, key >> np.uint64(32), H_UNREACHED).astype(np.uint32), sweeps=(s1, s2),
                counts=(int(got.sum()), int((inmask & ~got).sum()), 0, invalid))


def _dijkstra(shape, start, inmask, seeds, edge, conn):
    """start: {voxel: key}; edge(u, v, key_u) -> the key v gets through u, or None; seeds keep their start -> {voxel: key}"""
    done, heap = {}, [(k, v) for v, k in start.items()]
    heapq.heapify(heap)
    offs = offsets(conn)
    while heap:
        k, u = heapq.heappop(heap)
        if u in done:
            continue
        done[u] = k
        for o in offs:
            v = (u[0] + o[0], u[1] + o[1], u[2] + o[2])
            if min(v) < 0 or any(v[i] >= shape[i] for i in range(3)) or v in done or not inmask[v] or seeds[v]:
                continue
            c = edge(u, v, k)
            if c is not None:
                heapq.heappush(heap, (c, v))
    return done


def by_heap(cost, markers, mask=None, conn=1, rule="max"):
    """the same fields as fixed_point (without sweeps), voxel by voxel from priority queues"""
    cost, markers, inmask, seeds, invalid = _inputs(cost, markers, mask)
    shape = cost.shape
    sv = [tuple(int(i) for i in v) for v in np.argwhere(seeds)]
    labels = np.zeros(shape, np.int32)
    if rule == "sum":
        def edge(u, v, k):
            d = k[0] + int(cost[v])
            return (d, k[1]) if d <= DIST_MAX else None
        done = _dijkstra(shape, {v: (0, int(markers[v])) for v in sv}, inmask, seeds, edge, conn)
        dist = np.full(shape, (1 << 40) - 1, np.uint64)
        for v, (d, l) in done.items():
            dist[v], labels[v] = d, l
        got = labels != 0
        beside = np.zeros(shape, bool)
        for off in offsets(conn):
            beside |= _shifted(got, off, False)
        return dict(labels=labels, distance=dist, counts=(int(got.sum()), int((inmask & ~got).sum()), int((inmask & ~got & beside).sum()), invalid))
    hd = _dijkstra(shape, {v: int(cost[v]) for v in sv}, inmask, seeds, lambda u, v, k: max(k, int(cost[v])), conn)
    H = np.full(shape, H_UNREACHED, np.uint32)
    for v, h in hd.items():
        H[v] = h
    def tight(u, v, k):
        return (k[0] + 1, k[1]) if max(int(H[u]), int(cost[v])) == int(H[v]) and H[v] != H_UNREACHED else None
    done = _dijkstra(shape, {v: (0, int(markers[v])) for v in sv}, inmask, seeds, tight, conn)
    steps = np.full(shape, H_UNREACHED, np.uint32)
    for v, (s, l) in done.items():
        steps[v], labels[v] = s, l
    got = labels != 0
    return dict(labels=labels, height=H, steps=steps, counts=(int(got.sum()), int((inmask & ~got).sum()), 0, invalid))


def packed_one_phase(cost, markers, mask=None, conn=1):
    """the prototype the definition warns against: one key height << 24 | label, relaxed in raster order (Gauss-Seidel, forwards then backwards) until nothing changes
    -> labels.  The operator is not monotone, so what it converges to depends on the order."""
    cost, markers, inmask, seeds, _ = _inputs(cost, markers, mask)
    shape = cost.shape
    INF = (1 << 63)
    key = {}
    order = [tuple(int(i) for i in v) for v in np.argwhere(inmask)]
    for v in order:
        key[v] = (int(cost[v]) << 24) | int(markers[v]) if seeds[v] else INF
    offs = offsets(conn)
    changed = True
    while changed:
        changed = False
        for seq in (order, order[::-1]):
            for v in seq:
                if seeds[v]:
                    continue
                best = key[v]
                for o in offs:
                    kn = key.get((v[0] + o[0], v[1] + o[1], v[2] + o[2]), INF)
                    if kn == INF:
                        continue
                    c = (max(kn >> 24, int(cost[v])) << 24) | (kn & 0xFFFFFF)
                    if c < best:
                        best = c
                if best != key[v]:
                    key[v], changed = best, True
    labels = np.zeros(shape, np.int32)
    for v, k in key.items():
        if k != INF:
            labels[v] = k & 0xFFFFFF
    return labels


# ---- the contents of the tests -----------------------------------------------------------------------------------------------------------------------------------------
def content(shape, seed):
    """smoothed noise quantised to multiples of 8 (plateaus), a mask about 85 % set, about 3 % markers from five labels, voxels and markers on every face, one mask voxel no marker can reach"""
    rng = np.random.default_rng(seed)
    noise = ndimage.gaussian_filter(rng.random(shape), 1.2, mode="nearest")
    lo, hi = float(noise.min()), float(noise.max())
    cost = (np.floor((noise - lo) / max(hi - lo, 1e-9) * 12.0) * 8).astype(np.uint32)
    mask = rng.random(shape) < 0.85
    markers = np.where(rng.random(shape) < 0.03, rng.integers(1, 6, shape), 0).astype(np.int32)
    for ax in range(3):
        for side in (0, -1):
            face = [slice(None)] * 3
            face[ax] = side
            face = tuple(face)
            mask[face] |= rng.random(mask[face].shape) < 0.5
            markers[face] = np.where(rng.random(mask[face].shape) < 0.04, rng.integers(1, 6, mask[face].shape), markers[face])
    if min(shape) >= 5:                                                  # a mask voxel alone in a cleared 3 x 3 x 3: unreached under every connectivity
        cx, cy, cz = (n // 2 for n in shape)
        mask[cx - 1:cx + 2, cy - 1:cy + 2, cz - 1:cz + 2] = False
        mask[cx, cy, cz], markers[cx, cy, cz] = True, 0
    return np.asfortranarray(cost), np.asfortranarray(markers), np.asfortranarray(mask.astype(np.uint8))


def tie_decided(cost, markers, mask, conn, rule, res):
    """voxels whose label the tie rule decides: with the labels reversed (l -> 6 - l) the voxel goes to another marker set"""
    flipped = np.where(np.asarray(markers) > 0, 6 - np.asarray(markers), 0).astype(np.int32)
    other = fixed_point(cost, flipped, mask, conn, rule)["labels"]
    back = np.where(other > 0, 6 - other, 0)
    return int((back != res["labels"]).sum())


def asserted_content(shape, conn, rule):
    """the first seed for which the ORACLE shows at least two labels reached, an unreached mask voxel, a voxel decided by the label tie and at least two sweeps"""
    for seed in range(60):
        cost, markers, mask = content(shape, seed)
        res = fixed_point(cost, markers, mask, conn, rule)
        if len(np.unique(res["labels"][res["labels"] > 0])) >= 2 and res["counts"][1] >= 1 and min(res["sweeps"]) >= 2 and tie_decided(cost, markers, mask, conn, rule, res) >= 1:
            return cost, markers, mask, res
    raise AssertionError(f"no seed gives {shape} conn {conn} rule {rule} the asserted content")


def serpentine(shape=(33, 17, 9)):
    """a one-voxel corridor that runs along x in the rows y = 1, 3, 5, ... of every second z plane, joined at alternating ends: it crosses the brick faces at x = 32, at
    y = 8 | 16 and at z = 8 many times.  One marker at each end.  -> cost, markers, mask"""
    X, Y, Z = shape
    mask = np.zeros(shape, np.uint8, order="F")
    rows = []
    for i, z in enumerate(range(0, Z, 2)):
        ys = list(range(1, Y, 2))
        rows += [(y, z) for y in (ys if i % 2 == 0 else ys[::-1])]
    path = [(0, rows[0][0], rows[0][1])]
    for i, (y, z) in enumerate(rows):
        px, py, pz = path[-1]
        while py != y:                                                   # the joint to this row: along y, then along z, at the end the last row stopped at
            py += 1 if y > py else -1
            path.append((px, py, pz))
        while pz != z:
            pz += 1
            path.append((px, py, pz))
        step = 1 if px == 0 else -1
        while 0 <= px + step < X:
            px += step
            path.append((px, py, pz))
    for v in path:
        mask[v] = 1
    rng = np.random.default_rng(5)
    cost = np.asfortranarray((rng.integers(0, 4, shape) * 8).astype(np.uint32))
    markers = np.zeros(shape, np.int32, order="F")
    markers[path[0]], markers[path[-1]] = 2, 1
    return cost, markers, mask


def two_balls():
    """48 x 24 x 24: balls of radius 9 about (15, 12, 12) and (31, 12, 12), a ball of radius 2 about (44, 4, 4)"""
    g = np.indices((48, 24, 24))
    ball = lambda c, r: ((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) <= r * r
    return np.asfortranarray((ball((15, 12, 12), 9) | ball((31, 12, 12), 9) | ball((44, 4, 4), 2)).astype(np.uint8))


# ---- split_lesions over scipy ------------------------------------------------------------------------------------------------------------------------------------------
def depth_cost(d2, mask, d2max, quantum):
    q = np.floor((np.float64(d2max) - np.asarray(d2, np.float64)) / np.float64(quantum))
    q = np.where(np.isnan(q), 0.0, np.clip(q, 0.0, 4294967294.0))
    return np.where(np.asarray(mask) != 0, q, 0.0).astype(np.uint32)


def numbered_markers(comp, n_comp, cores, n_cores, min_seed_voxels=1):
    """comp / cores: label volumes (components of the mask, components of the deep voxels), both numbered in the order of their first voxel -> (markers int32, n parts,
    parent int32 [n parts]): the kept cores first in label order, then the components without a core in component order, each wholly its own marker"""
    comp, cores = np.asarray(comp), np.asarray(cores)
    size = np.bincount(cores.reshape(-1), minlength=n_cores + 1)
    owner = np.zeros(n_cores + 1, np.int64)
    owner[cores[cores > 0]] = comp[cores > 0]
    per_comp = np.bincount(owner[1:], minlength=n_comp + 1)
    keep = np.zeros(n_cores + 1, bool)
    keep[1:] = (size[1:] >= min_seed_voxels) | (per_comp[owner[1:]] == 1)
    number = np.zeros(n_cores + 1, np.int32)
    number[keep] = np.arange(1, int(keep.sum()) + 1)
    markers = number[cores].astype(np.int32)
    parent = [int(owner[c]) for c in range(1, n_cores + 1) if keep[c]]
    has = np.zeros(n_comp + 1, bool)
    has[owner[keep]] = True
    nxt = int(keep.sum())
    for c in range(1, n_comp + 1):
        if not has[c]:
            nxt += 1
            markers[comp == c] = nxt
            parent.append(c)
    return markers, nxt, np.asarray(parent, np.int32)


def split_lesions(mask, pixdim=(1.0, 1.0, 1.0), seed_depth_mm=6.0, conn=1, min_seed_voxels=1, quantum_mm2=None):
    """-> dict(labels, n, n_components, parent, d2max, cores): the definition of watershed.split_lesions over scipy.ndimage (label in C order of the first voxel, exact
    squared distances via distance_transform_edt, squared and rounded to the integer they are where the squared spacings are integers)"""
    m = np.asarray(mask) != 0
    s = ndimage.generate_binary_structure(3, conn)
    comp, n_comp = ndimage.label(m, s)
    p = np.asarray(pixdim, np.float64)
    d2 = ndimage.distance_transform_edt(m, sampling=p) ** 2
    if np.all(p * p == np.rint(p * p)):                                 # integer squared spacings: every exact squared distance is an integer
        d2 = np.rint(d2)
    d2 = np.where(m, d2, 0.0)
    cores, n_cores = ndimage.label(m & (d2 >= float(seed_depth_mm) ** 2), s)
    markers, n, parent = numbered_markers(comp, n_comp, cores, n_cores, min_seed_voxels)
    quantum = float((p * p).min()) / 4.0 if quantum_mm2 is None else float(quantum_mm2)
    d2max = float(d2.max()) if m.any() else 0.0
    cost = depth_cost(d2, m, d2max, quantum)
    res = fixed_point(cost, markers, m, conn, "max")
    return dict(labels=res["labels"], n=n, n_components=n_comp, parent=parent, d2max=d2max, cores=int(np.count_nonzero(np.bincount(cores.reshape(-1))[1:])) if n_cores else 0,
                sweeps=res["sweeps"], markers=markers, cost=cost)

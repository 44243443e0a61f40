"""Airway and vessel centerlines on the device: thinning, the branch graph, branch territories (csrc/kernels_skeleton.hip).

    thin_volume(mask, endpoints=, max_iterations=, chunk=)      -> Skeleton: the topology-preserving thinning of a mask (unet_vol_thin_begin / _iterations / _end)
    skeleton_table(skel, radius_of=, pixdim=)                   -> one row per voxel of a thin mask: index, x, y, z, degree, neighbour mask (+ radius_mm)
                                                                   (unet_vol_skeleton_count / _emit)
    skeleton_graph(skel, pixdim, radius_of=, affine=)           -> SkeletonGraph: nodes, branches with length, chord, tortuosity and calibre, components with their cycles
    prune(graph, min_length_mm=, min_ratio=)                    -> the graph without short terminal branches
    root_tree(graph, root=)                                     -> RootedTree: parent, children and generation of every branch
    branch_territories(mask, skel, graph, connectivity=)        -> BranchTerritories: the branch id of every mask voxel (geodesic growth + unet_vol_label_spread)
    airway_tree / vessel_tree                                   -> CenterlineTree: thin -> graph -> prune -> root -> territories, with a table per generation
    thin_device / table_device / label_spread_device            -> the entries on device buffers
    graph_from_table / table_from_indices                       -> the host half on its own: a graph from any table of voxels

Sources are what lungs and filters take: a path, a NiftiVolume, an [X, Y, Z] array, or a flat uint8 device tensor with shape=.  The thinning is defined in DESIGN.md section
4ag (directional passes +z, -z, +y, -y, +x, -x; candidates judged on the image as a pass finds it; eight subfield sub-passes that test simplicity again) and every device
result equals tests/skeleton_oracle.py element for element.  The graph is built on the host from the table: a skeleton is sparse.  Every argument error is a ValueError
raised before any device work; there is no CPU fallback for the device steps.  The pruning thresholds are conventional and configurable, NOT clinically validated here.
World coordinates are given only with an affine; left and right are never guessed.  Lobes, artery / vein separation, surface skeletons, sub-voxel centerlines and sharding
across ranks are out of scope.
"""
from __future__ import annotations

import time

import numpy as np

from . import lungs as L
from . import volume as V

OFFSETS = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))          # bit b of a neighbour mask <-> OFFSETS[b]
TABLE_FIELDS = [("index", np.int32), ("x", np.int32), ("y", np.int32), ("z", np.int32), ("degree", np.int32), ("neighbours", np.uint32)]
NODE_DTYPE = np.dtype([("id", np.int32), ("kind", "U8"), ("voxels", np.int32), ("x", np.float64), ("y", np.float64), ("z", np.float64), ("wx", np.float64), ("wy", np.float64),
                       ("wz", np.float64), ("branches", np.int32), ("component", np.int32), ("radius_mm", np.float64)])
COMPONENT_DTYPE = np.dtype([("component", np.int32), ("nodes", np.int32), ("branches", np.int32), ("cycles", np.int32), ("length_mm", np.float64)])
GENERATION_DTYPE = np.dtype([("generation", np.int32), ("branches", np.int32), ("length_mm", np.float64), ("voxels", np.int64), ("ml", np.float64), ("radius_mm", np.float64)])
MIN_LENGTH_MM, MIN_RATIO = 3.0, 1.5                                  # conventional, configurable, not validated here
_TREE_KEYS = {"endpoints", "max_iterations", "min_length_mm", "min_ratio", "connectivity", "pixdim", "orientation", "affine", "root", "territories", "shape", "close", "fill"}


class Skeleton:
    """thin_volume's result.  mask: uint8 [X, Y, Z] (return_device=True: the flat device tensor); shape; iterations: the iterations run, the last, empty one included;
    removed: int64 [iterations], the voxels every iteration cleared; voxels: the voxels left; endpoints; seconds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"Skeleton(shape={self.shape}, voxels={self.voxels}, iterations={self.iterations})"


class Branch:
    """id; a, b: the node ids of its ends; path: int64 flat indices from the node voxel it touches at a to the one at b; length_mm: summed over consecutive voxel centres;
    chord_mm: between the two end voxels; tortuosity = length / chord (inf for a closed branch); radius_min / _mean / _max (NaN without radii); component."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"Branch({self.id}: {self.a} -> {self.b}, voxels={len(self.path)}, length_mm={self.length_mm:.2f})"


class SkeletonGraph:
    """shape; pixdim; affine (or None); table: the voxel table it was built from; nodes: NODE_DTYPE records (kind: end, isolated, junction, loop; x, y, z: the centroid in
    voxel coordinates; wx, wy, wz: in world millimetres, NaN without an affine; branches: the branch ends that meet there); node_voxels: per node the flat indices of its
    voxels; branches: a list of Branch; components: COMPONENT_DTYPE records, cycles = E - V + 1."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"SkeletonGraph(nodes={len(self.nodes)}, branches={len(self.branches)}, components={len(self.components)})"


class RootedTree:
    """root_tree's result, arrays over the graph's branches.  parent: the parent branch or -1; generation: 0 for a root branch, -1 for a branch that closes a cycle;
    closes_cycle: bool; towards: the node id at the branch's far end (away from the root); children: per branch the list of its children; roots: the root node of every
    component."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"RootedTree(branches={len(self.parent)}, generations={int(self.generation.max()) + 1 if len(self.generation) else 0}, cycles={int(self.closes_cycle.sum())})"


class BranchTerritories:
    """labels: int32 [X, Y, Z], 1 + the id of the branch whose centerline a mask voxel is nearest to along the mask (0: outside the mask, or not reachable from the
    centerline); voxels, ml: per branch; steps: the growth steps."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class CenterlineTree:
    """airway_tree's / vessel_tree's result.  mask: the prepared mask (closed, holes filled) that was thinned, uint8 [X, Y, Z]; skeleton; graph (pruned); tree: the RootedTree; territories (or None); generations: GENERATION_DTYPE records -- branches,
    total length, territory volume and mean calibre per generation; cycles: the sum of the components' cyclomatic numbers (in an airway tree a cycle marks a leak);
    seconds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"CenterlineTree(branches={len(self.graph.branches)}, generations={len(self.generations)}, cycles={self.cycles})"


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_thin_args(endpoints=True, max_iterations=None, chunk=8):
    L._check_bool(endpoints, "endpoints")
    if max_iterations is not None and (not L._is_int(max_iterations) or not 0 <= int(max_iterations) < 2 ** 31):
        raise ValueError(f"max_iterations is None or an integer >= 0, not {max_iterations!r}")
    if not L._is_int(chunk) or not 1 <= int(chunk) <= 4096:
        raise ValueError(f"chunk is an integer in 1..4096, not {chunk!r}")
    return bool(endpoints), (None if max_iterations is None else int(max_iterations)), int(chunk)


def _mask_source(mask, shape, what="mask"):
    """a path, a NiftiVolume, an array or a device tensor with shape= -> (upload: a function that gives the flat device bytes, (X, Y, Z)); no device work here"""
    torch = V._torch()
    if isinstance(mask, Skeleton):
        mask, shape = mask.mask, (mask.shape if isinstance(mask.mask, torch.Tensor) else None)
    if isinstance(mask, torch.Tensor):
        L._mask_arg(mask, shape, None, what)
        if shape is None:
            raise ValueError(f"a device {what} is a flat Fortran-order byte buffer: pass shape=(X, Y, Z)")
    elif isinstance(mask, np.ndarray) or isinstance(mask, (list, tuple)):
        L._mask_arg(mask, shape, None, what)
    src = V._resample_source(mask, src_shape=shape if isinstance(mask, torch.Tensor) else None, kind="mask")
    return (lambda: src.tensor if src.tensor is not None else V.upload(src.vol)), tuple(int(v) for v in src.shape)


def _check_positive_or_none(v, what):
    if v is not None and (not L._is_number(v) or not (np.isfinite(float(v)) and float(v) >= 0.0)):
        raise ValueError(f"{what} is None or a finite number >= 0, not {v!r}")
    return None if v is None else float(v)


# ---- the entries ------------------------------------------------------------------------------------------------------------------------------------------------------
def thin_device(mask_dev, shape, endpoints=True, max_iterations=None, chunk=8):
    """unet_vol_thin_begin, then unet_vol_thin_iterations in calls of `chunk` iterations until one clears nothing or max_iterations have run, then unet_vol_thin_end ->
    (the thinned mask as a flat uint8 device tensor, removed: int64 numpy [iterations]).  The counts come to the host between the calls, nothing else does."""
    endpoints, limit, chunk = _check_thin_args(endpoints, max_iterations, chunk)
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    N = X * Y * Z
    out = torch.empty(N, dtype=torch.uint8, device="cuda")
    if N == 0:
        return out, np.zeros(0, np.int64)
    ws = torch.empty(max(int(lib.unet_vol_thin_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_thin_begin(ctx.handle, V._ptr(mask_dev), X, Y, Z, V._ptr(ws), ws.numel(), V._stream()), "vol_thin_begin")
    removed, first = [], 0
    while limit is None or first < limit:
        n = chunk if limit is None else min(chunk, limit - first)
        counts = torch.zeros(first + n, dtype=torch.int64, device="cuda")          # (the entry writes removed[first .. first + n - 1]; a thinning runs tens of iterations)
        ctx.check(lib.unet_vol_thin_iterations(ctx.handle, X, Y, Z, first, n, 1 if endpoints else 0, V._ptr(counts), V._ptr(ws), ws.numel(), V._stream()),
                  "vol_thin_iterations")
        got = counts[first:first + n].cpu().numpy()
        empty = np.flatnonzero(got == 0)
        if empty.size:
            removed.extend(int(v) for v in got[:int(empty[0]) + 1])
            break
        removed.extend(int(v) for v in got)
        first += n
    ctx.check(lib.unet_vol_thin_end(ctx.handle, X, Y, Z, V._ptr(out), V._ptr(ws), ws.numel(), V._stream()), "vol_thin_end")
    return out, np.asarray(removed, np.int64)


def table_device(mask_dev, shape, d2_dev=None):
    """unet_vol_skeleton_count, the total to the host, unet_vol_skeleton_emit -> (index int32 [n], neighbour masks uint32 [n], d2 at those voxels float64 [n] or None), numpy"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    if X * Y * Z == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.uint32), (None if d2_dev is None else np.zeros(0, np.float64))
    ws = torch.empty(max(int(lib.unet_vol_skeleton_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_skeleton_count(ctx.handle, V._ptr(mask_dev), X, Y, Z, V._ptr(total), V._ptr(ws), ws.numel(), V._stream()), "vol_skeleton_count")
    n = int(total.item())
    index = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    nbr = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    vals = None if d2_dev is None else torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    ctx.check(lib.unet_vol_skeleton_emit(ctx.handle, V._ptr(mask_dev), X, Y, Z, V._ptr(d2_dev), n, n, V._ptr(index), V._ptr(nbr), V._ptr(vals), V._ptr(ws), ws.numel(),
                                         V._stream()), "vol_skeleton_emit")
    return index[:n].cpu().numpy(), nbr[:n].cpu().numpy().view(np.uint32), (None if vals is None else vals[:n].cpu().numpy())


def label_spread_device(arrival_dev, labels_dev, shape, steps, connectivity=3, chunk=64):
    """unet_vol_label_spread over the steps 1 .. steps, in place on labels_dev (int32); arrival_dev: geodesic_device's bytes of the uint16 volume"""
    lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    connectivity = V._check_connectivity(connectivity)
    first = 1
    while first <= steps:
        n = min(int(chunk), steps - first + 1)
        ctx.check(lib.unet_vol_label_spread(ctx.handle, V._ptr(arrival_dev), V._ptr(labels_dev), X, Y, Z, first, n, connectivity, V._stream()), "vol_label_spread")
        first += n
    return labels_dev


# ---- thinning and the table ---------------------------------------------------------------------------------------------------------------------------------------------
def thin_volume(mask, endpoints=True, max_iterations=None, chunk=8, return_device=False, shape=None):
    """The centerline of mask != 0 -> Skeleton.  26-connected objects in a 6-connected background; the components, the cavities and the tunnels of the mask survive, every
    voxel cleared was a simple point when it went.  endpoints=True keeps the ends of curves (a voxel with one neighbour is never cleared), so tubes thin to curves and a
    ball to a short segment; endpoints=False thins everything without a tunnel or a cavity to one voxel.  max_iterations=None: until an iteration clears nothing; the
    launches go in calls of `chunk` iterations and the counts come to the host between them."""
    _check_thin_args(endpoints, max_iterations, chunk)
    L._check_bool(return_device, "return_device")
    upload, shp = _mask_source(mask, shape)
    t0 = time.perf_counter()
    out, removed = thin_device(upload(), shp, endpoints, max_iterations, chunk)
    voxels = int(V._torch().count_nonzero(out).item()) if out.numel() else 0
    sec = {"thin": time.perf_counter() - t0}
    return Skeleton(mask=V._result(out, shp, bool(return_device)), shape=shp, iterations=len(removed), removed=removed, voxels=voxels, endpoints=bool(endpoints), seconds=sec)


def _finish_table(index, nbr, shape, radius=None):
    X, Y, Z = (int(v) for v in shape)
    t = np.zeros(len(index), np.dtype(TABLE_FIELDS + ([("radius_mm", np.float64)] if radius is not None else [])))
    f = np.asarray(index, np.int64)
    t["index"], t["x"], t["y"], t["z"] = index, f % max(X, 1), (f // max(X, 1)) % max(Y, 1), f // max(X * Y, 1)
    t["neighbours"] = nbr
    t["degree"] = np.unpackbits(np.ascontiguousarray(nbr, np.uint32).view(np.uint8).reshape(-1, 4), axis=1).sum(1) if len(index) else 0
    if radius is not None:
        t["radius_mm"] = radius
    return t


def table_from_indices(index, shape, radius=None):
    """the table of the voxels with the flat indices `index` (any order, distinct) of a volume of `shape`, on the host: the neighbour masks by search among the indices"""
    X, Y, Z = (int(v) for v in shape)
    order = np.argsort(np.asarray(index, np.int64), kind="stable")
    f = np.asarray(index, np.int64)[order]
    x, y, z = f % max(X, 1), (f // max(X, 1)) % max(Y, 1), f // max(X * Y, 1)
    nbr = np.zeros(len(f), np.uint32)
    for b, (dx, dy, dz) in enumerate(OFFSETS):
        xx, yy, zz = x + dx, y + dy, z + dz
        ok = (xx >= 0) & (xx < X) & (yy >= 0) & (yy < Y) & (zz >= 0) & (zz < Z)
        g = xx + X * (yy + Y * zz)
        pos = np.clip(np.searchsorted(f, g), 0, max(len(f) - 1, 0))
        nbr |= (ok & (f[pos] == g)).astype(np.uint32) << np.uint32(b) if len(f) else np.uint32(0)
    return _finish_table(f.astype(np.int32), nbr, shape, None if radius is None else np.asarray(radius, np.float64)[order])


def skeleton_table(skel, radius_of=None, pixdim=None, shape=None):
    """One row per set voxel of a (thin) mask, sorted by flat index: index, x, y, z, degree = the set voxels among the 26 neighbours, neighbours = which (bit b <-> OFFSETS[b]).
    skel: a Skeleton, or a mask source.  radius_of: a mask in the same shape -- adds radius_mm = sqrt(d2), d2 the exact squared distance (pixdim, default 1 mm) of the voxel
    to the nearest background voxel of that mask (unet_vol_edt_sq); outside the volume counts as far away, as distance_transform defines it."""
    p = V._check_pixdim((1.0, 1.0, 1.0) if pixdim is None else pixdim)
    upload, shp = _mask_source(skel, shape, "skel")
    up_r = None
    if radius_of is not None:
        up_r, rshape = _mask_source(radius_of, shp if isinstance(radius_of, V._torch().Tensor) else None, "radius_of")
        if rshape != shp:
            raise ValueError(f"radius_of is {rshape}, the skeleton {shp}")
    d2 = None if up_r is None or int(np.prod(shp)) == 0 else V.edt_sq_device(up_r(), shp, p, features_nonzero=False)
    index, nbr, vals = table_device(upload(), shp, d2)
    return _finish_table(index, nbr, shp, None if radius_of is None else np.sqrt(vals if vals is not None else np.zeros(0)))


# ---- the graph (host) -------------------------------------------------------------------------------------------------------------------------------------------------
def _neighbour_rows(table, shape):
    """per row the rows of its set neighbours, ascending"""
    X, Y, Z = (int(v) for v in shape)
    f = table["index"].astype(np.int64)
    out = [[] for _ in range(len(f))]
    for b, (dx, dy, dz) in enumerate(OFFSETS):
        rows = np.flatnonzero((table["neighbours"] >> np.uint32(b)) & np.uint32(1))
        if rows.size == 0:
            continue
        g = f[rows] + dx + X * (dy + Y * dz)
        pos = np.searchsorted(f, g)
        if (pos >= len(f)).any() or not np.array_equal(f[np.minimum(pos, len(f) - 1)], g):
            raise ValueError("the table's neighbour masks name voxels that are not in the table")
        for r, q in zip(rows.tolist(), pos.tolist()):
            out[r].append(q)
    return [sorted(v) for v in out]


def _path_length(path, shape, p):
    X, Y, Z = (int(v) for v in shape)
    f = np.asarray(path, np.int64)
    c = np.stack([f % X, (f // X) % Y, f // (X * Y)], 1).astype(np.float64) * p
    seg = np.sqrt(((c[1:] - c[:-1]) ** 2).sum(1))
    return float(seg.sum()), float(np.sqrt(((c[-1] - c[0]) ** 2).sum()))


def graph_from_table(table, shape, pixdim=(1.0, 1.0, 1.0), affine=None):
    """The branch graph of the voxels of a table (skeleton_table's, or table_from_indices') -> SkeletonGraph.  Nodes: voxels of degree 1 (end) and 0 (isolated), the
    26-connected clusters of voxels of degree >= 3 (junction; position: the centroid), and for a closed curve without one its voxel of smallest flat index (loop).
    Branches: the maximal chains of degree-2 voxels between nodes, with the node voxel they touch at either end; a chain from a junction back to itself is a branch with
    both ends there; two touching node voxels of different nodes are a branch without interior."""
    p = V._check_pixdim(pixdim)
    shape = tuple(int(v) for v in shape)
    A = None
    if affine is not None:
        A = np.asarray(affine, np.float64)
        if A.shape != (4, 4) or not np.isfinite(A).all():
            raise ValueError("affine is a finite 4 x 4 matrix")
    n = len(table)
    nb = _neighbour_rows(table, shape)
    deg = table["degree"].astype(np.int64)
    has_r = "radius_mm" in (table.dtype.names or ())
    node_of = np.full(n, -1, np.int64)
    node_rows, kinds = [], []
    for r in range(n):                                               # ascending flat index: node ids follow the smallest index of a node's voxels
        if node_of[r] >= 0 or deg[r] == 2:
            continue
        if deg[r] <= 1:
            node_of[r] = len(node_rows); node_rows.append([r]); kinds.append("end" if deg[r] == 1 else "isolated")
            continue
        cluster, stack = [], [r]
        node_of[r] = len(node_rows)
        while stack:
            c = stack.pop(); cluster.append(c)
            for q in nb[c]:
                if deg[q] >= 3 and node_of[q] < 0:
                    node_of[q] = len(node_rows); stack.append(q)
        node_rows.append(sorted(cluster)); kinds.append("junction")
    visited = np.zeros(n, bool)
    paths = []

    def walk(v, u):
        path, prev, cur = [v, u], v, u
        while node_of[cur] < 0:
            visited[cur] = True
            nxt = [q for q in nb[cur] if q != prev]
            if len(nxt) != 1:                                        # (a degree-2 voxel whose two neighbours are one voxel cannot be)
                raise ValueError("the table is not consistent: a degree-2 voxel without a way on")
            prev, cur = cur, nxt[0]
            path.append(cur)
        return path

    for v in range(n):
        if node_of[v] < 0:
            continue
        for u in nb[v]:
            if node_of[u] == node_of[v]:
                continue
            path = walk(v, u)
            if (path[0], path[1]) <= (path[-1], path[-2]):           # every branch is met from both ends: the walk from the smaller end is kept
                paths.append(path)
    for v in range(n):                                               # closed curves without a node
        if node_of[v] >= 0 or visited[v]:
            continue
        node_of[v] = len(node_rows); node_rows.append([v]); kinds.append("loop")
        paths.append(walk(v, nb[v][0]))
    index = table["index"].astype(np.int64)
    nodes = np.zeros(len(node_rows), NODE_DTYPE)
    for i, rows in enumerate(node_rows):
        c = np.stack([table["x"][rows], table["y"][rows], table["z"][rows]], 1).astype(np.float64).mean(0)
        w = (A @ np.append(c, 1.0))[:3] if A is not None else np.full(3, np.nan)
        nodes[i] = (i, kinds[i], len(rows), c[0], c[1], c[2], w[0], w[1], w[2], 0, -1, float(np.max(table["radius_mm"][rows])) if has_r else np.nan)
    parent = list(range(len(node_rows)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]; a = parent[a]
        return a

    branches = []
    for i, path in enumerate(paths):
        a, b = int(node_of[path[0]]), int(node_of[path[-1]])
        length, chord = _path_length(index[path], shape, p)
        rr = table["radius_mm"][path].astype(np.float64) if has_r else None
        branches.append(Branch(id=i, a=a, b=b, path=index[path].copy(), length_mm=length, chord_mm=chord, tortuosity=(length / chord if chord > 0 else float("inf")),
                               radius_min=float(rr.min()) if has_r else np.nan, radius_mean=float(rr.mean()) if has_r else np.nan,
                               radius_max=float(rr.max()) if has_r else np.nan, radius_a=float(rr[0]) if has_r else np.nan, radius_b=float(rr[-1]) if has_r else np.nan,
                               component=-1))
        nodes["branches"][a] += 1; nodes["branches"][b] += 1
        parent[find(a)] = find(b)
    first = {}
    for i in range(len(node_rows)):                                  # components in the order of their first node
        first.setdefault(find(i), i)
    roots = sorted(first, key=first.get)
    comp_of = {r: c for c, r in enumerate(roots)}
    comps = np.zeros(len(roots), COMPONENT_DTYPE)
    comps["component"] = np.arange(len(roots))
    for i in range(len(node_rows)):
        c = comp_of[find(i)]
        nodes["component"][i] = c; comps["nodes"][c] += 1
    for br in branches:
        br.component = int(nodes["component"][br.a]); comps["branches"][br.component] += 1; comps["length_mm"][br.component] += br.length_mm
    comps["cycles"] = comps["branches"] - comps["nodes"] + 1
    return SkeletonGraph(shape=shape, pixdim=tuple(float(v) for v in p), affine=A, table=table, nodes=nodes, node_voxels=[index[rows].copy() for rows in node_rows],
                         branches=branches, components=comps)


def skeleton_graph(skel, pixdim, radius_of=None, affine=None, shape=None):
    """skeleton_table (on the device), then graph_from_table (on the host) -> SkeletonGraph.  pixdim: the voxel size the lengths and radii are measured with."""
    p = V._check_pixdim(pixdim)
    upload, shp = _mask_source(skel, shape, "skel")
    if affine is not None and (np.shape(affine) != (4, 4) or not np.isfinite(np.asarray(affine, np.float64)).all()):
        raise ValueError("affine is a finite 4 x 4 matrix")
    return graph_from_table(skeleton_table(skel, radius_of, p, shape), shp, p, affine)


# ---- pruning ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _terminal(graph):
    """(branch, which end is the free one) of every branch from an end node to a junction"""
    out = []
    for br in graph.branches:
        ka, kb = graph.nodes["kind"][br.a], graph.nodes["kind"][br.b]
        if ka == "end" and kb == "junction":
            out.append((br, 0))
        elif kb == "end" and ka == "junction":
            out.append((br, 1))
    return out


def _branch_measures(graph, path):
    table = graph.table
    length, chord = _path_length(path, graph.shape, np.asarray(graph.pixdim, np.float64))
    has_r = "radius_mm" in (table.dtype.names or ())
    rr = table["radius_mm"][np.searchsorted(table["index"].astype(np.int64), path)].astype(np.float64) if has_r else None
    return dict(path=path, length_mm=length, chord_mm=chord, tortuosity=(length / chord if chord > 0 else float("inf")),
                radius_min=float(rr.min()) if has_r else np.nan, radius_mean=float(rr.mean()) if has_r else np.nan, radius_max=float(rr.max()) if has_r else np.nan,
                radius_a=float(rr[0]) if has_r else np.nan, radius_b=float(rr[-1]) if has_r else np.nan)


def _merge_through(graph, node, nb):
    """a junction left with two branch ends -> one branch through it: the two paths joined by the shortest way inside the cluster (breadth first, neighbours in index
    order); a single branch from the junction back to itself is left alone"""
    inc = [br for br in graph.branches if br.a == node or br.b == node]
    if len(inc) != 2:
        return
    index = graph.table["index"].astype(np.int64)
    p1 = inc[0].path if inc[0].b == node else inc[0].path[::-1]      # ... -> the cluster
    p2 = inc[1].path if inc[1].a == node else inc[1].path[::-1]      # the cluster -> ...
    t1, t2 = int(p1[-1]), int(p2[0])
    if t1 == t2:
        joined = np.concatenate([p1, p2[1:]])
    else:
        inside = set(np.searchsorted(index, graph.node_voxels[node]).tolist())
        s, e = int(np.searchsorted(index, t1)), int(np.searchsorted(index, t2))
        prev, queue = {s: None}, [s]
        while queue and e not in prev:
            c = queue.pop(0)
            for q in nb[c]:
                if q in inside and q not in prev:
                    prev[q] = c; queue.append(q)
        mid, c = [], prev[e]
        while c is not None and c != s:
            mid.append(int(index[c])); c = prev[c]
        joined = np.concatenate([p1, np.asarray(mid[::-1], np.int64), p2])
    a = inc[0].a if inc[0].b == node else inc[0].b
    b = inc[1].b if inc[1].a == node else inc[1].a
    inc[0].__dict__.update(a=int(a), b=int(b), **_branch_measures(graph, joined))
    graph.branches.remove(inc[1])
    graph.nodes["branches"][node] = 0
    graph.nodes["kind"][node] = "through"


def prune(graph, min_length_mm=MIN_LENGTH_MM, min_ratio=None):
    """The graph without its short terminal branches -> a new SkeletonGraph over the same table.  A terminal branch runs from an end to a junction; it goes when its
    length is below min_length_mm, or (min_ratio, with radii in the table) below min_ratio x the radius at its junction end -- a spur no longer than the tube is wide
    there.  The shortest goes first (ties: the lower id); a junction left with two branches at once becomes part of one branch through it, one left with a single
    branch becomes an end; that repeats until no branch qualifies.  A branch between two ends is a whole component and stays.  Nodes and branches are renumbered in their
    old order; the table keeps the pruned voxels, which no branch runs over any more.  The thresholds are conventional and configurable, not clinically validated here."""
    if not isinstance(graph, SkeletonGraph):
        raise ValueError(f"graph is a SkeletonGraph, not {graph!r}")
    ml, mr = _check_positive_or_none(min_length_mm, "min_length_mm"), _check_positive_or_none(min_ratio, "min_ratio")
    if mr is not None and "radius_mm" not in (graph.table.dtype.names or ()):
        raise ValueError("min_ratio compares a branch with the radius at its junction: build the graph with radius_of=")
    g = SkeletonGraph(shape=graph.shape, pixdim=graph.pixdim, affine=graph.affine, table=graph.table, nodes=graph.nodes.copy(), node_voxels=list(graph.node_voxels),
                      branches=[Branch(**br.__dict__) for br in graph.branches], components=graph.components.copy())
    nb = None
    while True:
        worst = None
        for br, free in _terminal(g):
            r_j = br.radius_b if free == 0 else br.radius_a
            if (ml is not None and br.length_mm < ml) or (mr is not None and br.length_mm < mr * r_j):
                if worst is None or (br.length_mm, br.id) < (worst[0].length_mm, worst[0].id):
                    worst = (br, free)
        if worst is None:
            break
        br, free = worst
        end, junction = (br.a, br.b) if free == 0 else (br.b, br.a)
        g.branches.remove(br)
        g.nodes["kind"][end] = "through"; g.nodes["branches"][end] = 0
        g.nodes["branches"][junction] -= 1
        if g.nodes["branches"][junction] == 2:
            if nb is None:
                nb = _neighbour_rows(g.table, g.shape)
            _merge_through(g, junction, nb)
        elif g.nodes["branches"][junction] == 1:
            g.nodes["kind"][junction] = "end"
        elif g.nodes["branches"][junction] == 0:
            g.nodes["kind"][junction] = "isolated"
    alive = np.flatnonzero(g.nodes["kind"] != "through")             # the ends of pruned branches and the merged-away junctions leave; ids stay dense
    remap = np.full(len(g.nodes), -1, np.int64)
    remap[alive] = np.arange(len(alive))
    g.node_voxels = [g.node_voxels[i] for i in alive.tolist()]
    g.nodes = g.nodes[alive].copy()
    g.nodes["id"] = np.arange(len(alive))
    for i, br in enumerate(g.branches):
        br.id, br.a, br.b = i, int(remap[br.a]), int(remap[br.b])
    g.components["nodes"] = np.bincount(g.nodes["component"].astype(np.int64), minlength=len(g.components))
    g.components["branches"] = np.bincount(np.asarray([br.component for br in g.branches], np.int64), minlength=len(g.components))
    g.components["length_mm"] = np.bincount(np.asarray([br.component for br in g.branches], np.int64), [br.length_mm for br in g.branches], minlength=len(g.components))
    g.components["cycles"] = g.components["branches"] - g.components["nodes"] + 1
    return g


# ---- rooting ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _superior_axis(orientation):
    """-> (axis, sign) of the superior direction, from a code or an affine; ValueError without one"""
    if orientation is None:
        raise ValueError('root="superior" needs the orientation: the graph carries no affine; pass orientation= (a code such as "LPS", or an affine) -- superior is not guessed')
    _, codes = V._check_orientation(orientation)
    for ax, c in enumerate(codes):
        if str(c) in ("S", "I"):
            return ax, (1.0 if str(c) == "S" else -1.0)
    raise ValueError(f"the axis codes {codes} hold no S / I axis")


def root_tree(graph, root="thickest", orientation=None):
    """Parent, children and generation of every branch -> RootedTree.  root: "thickest" -- per component the end with the largest radius (ties: the smallest index; needs
    radii); "superior" -- per component the end furthest towards S (orientation=, or the graph's affine; ValueError without: it is not guessed); a voxel (three
    integers) or, with an affine, a world point (three floats): the node nearest to it roots its component, the others take their end of smallest index.  A component
    without an end is rooted at its first node.  The branches at the root are generation 0, their children 1, and so on, breadth first in id order; a branch whose far
    node was reached before closes a cycle: it is flagged, has generation -1 and is not forced into the tree."""
    if not isinstance(graph, SkeletonGraph):
        raise ValueError(f"graph is a SkeletonGraph, not {graph!r}")
    nodes, nb = graph.nodes, len(graph.branches)
    score, chosen = None, None
    if isinstance(root, str):
        if root == "thickest":
            if "radius_mm" not in (graph.table.dtype.names or ()):
                raise ValueError('root="thickest" needs radii: build the graph with radius_of=')
            score = nodes["radius_mm"].astype(np.float64)
        elif root == "superior":
            ax, sign = _superior_axis(orientation if orientation is not None else graph.affine)
            score = sign * nodes[("x", "y", "z")[ax]].astype(np.float64)
        else:
            raise ValueError(f'root is "thickest", "superior", a voxel or a world point, not {root!r}')
    else:
        try:
            pt = np.asarray(root, np.float64).reshape(-1)
        except (TypeError, ValueError):
            pt = np.zeros(0)
        if pt.shape != (3,) or not np.isfinite(pt).all():
            raise ValueError(f'root is "thickest", "superior", a voxel or a world point, not {root!r}')
        is_voxel = all(L._is_int(v) for v in (list(root) if not isinstance(root, np.ndarray) else root.tolist()))
        if not is_voxel and graph.affine is None:
            raise ValueError("a world point needs the graph's affine: pass a voxel (three integers) instead")
        if len(nodes):
            c = np.stack([nodes["x"], nodes["y"], nodes["z"]] if is_voxel else [nodes["wx"], nodes["wy"], nodes["wz"]], 1)
            chosen = int(np.argmin(((c - pt) ** 2).sum(1)))
    roots = []
    for comp in range(len(graph.components)):
        members = np.flatnonzero(nodes["component"] == comp)
        if chosen is not None and nodes["component"][chosen] == comp:
            roots.append(chosen); continue
        ends = members[nodes["kind"][members] == "end"]
        if ends.size == 0:
            roots.append(int(members[0]))
        elif score is None:
            roots.append(int(ends[0]))
        else:
            roots.append(int(ends[np.argmax(score[ends])]))          # argmax: the first of equal scores, the smallest index
    at = [[] for _ in range(len(nodes))]
    for br in graph.branches:
        at[br.a].append(br.id)
        if br.b != br.a:
            at[br.b].append(br.id)
    parent = np.full(nb, -1, np.int64); gen = np.full(nb, -1, np.int64); cyc = np.zeros(nb, bool); towards = np.full(nb, -1, np.int64)
    seen_b = np.zeros(nb, bool); seen_n = np.zeros(len(nodes), bool)
    children = [[] for _ in range(nb)]
    for r in roots:
        seen_n[r] = True
        queue = [(r, -1, 0)]
        while queue:
            node, par, g = queue.pop(0)
            for bid in at[node]:
                if seen_b[bid]:
                    continue
                seen_b[bid] = True
                br = graph.branches[bid]
                far = br.b if br.a == node else br.a
                if seen_n[far]:                                      # (a branch back to its own node included)
                    cyc[bid] = True
                    continue
                seen_n[far] = True
                parent[bid], gen[bid], towards[bid] = par, g, far
                if par >= 0:
                    children[par].append(bid)
                queue.append((far, bid, g + 1))
    return RootedTree(parent=parent, generation=gen, closes_cycle=cyc, towards=towards, children=children, roots=np.asarray(roots, np.int64))


# ---- territories ------------------------------------------------------------------------------------------------------------------------------------------------------
def branch_seed_labels(graph):
    """-> (flat indices int64, labels int32): 1 + the branch id on every voxel of the graph; a node voxel takes the lowest id among the branches that meet at its node"""
    lab = {}
    for br in graph.branches:
        for f in br.path[1:-1].tolist():
            lab[f] = br.id + 1
    for br in graph.branches:                                        # ascending id: setdefault keeps the lowest
        for node in (br.a, br.b):
            for f in graph.node_voxels[node].tolist():
                lab.setdefault(f, br.id + 1)
        for f in (int(br.path[0]), int(br.path[-1])):
            lab.setdefault(f, br.id + 1)
    idx = np.asarray(sorted(lab), np.int64)
    return idx, np.asarray([lab[f] for f in idx.tolist()], np.int32)


def branch_territories(mask, skel, graph, connectivity=3, return_device=False, shape=None):
    """The branch every mask voxel belongs to -> BranchTerritories.  The centerline voxels of the graph carry 1 + their branch's id (branch_seed_labels); the growth of
    lungs.geodesic_distance from them inside the mask records the step every voxel was reached at, and unet_vol_label_spread hands the labels on step by step: a voxel
    takes the smallest label among the neighbours (`connectivity`, as in the growth) reached one step before it.  skel is accepted for its shape only: the seeds are the
    graph's voxels, so a pruned graph leaves the pruned voxels to the branches that remain.  voxels and ml per branch come from volume.component_stats_device."""
    connectivity = V._check_connectivity(connectivity)
    L._check_bool(return_device, "return_device")
    if not isinstance(graph, SkeletonGraph):
        raise ValueError(f"graph is a SkeletonGraph, not {graph!r}")
    upload, shp = _mask_source(mask, shape)
    if skel is not None and tuple(int(v) for v in skel.shape) != shp:
        raise ValueError(f"the skeleton is {tuple(skel.shape)}, the mask {shp}")
    if tuple(graph.shape) != shp:
        raise ValueError(f"the graph is {tuple(graph.shape)}, the mask {shp}")
    torch = V._torch()
    N, nb = int(np.prod(shp)), len(graph.branches)
    idx, lab = branch_seed_labels(graph)
    labels = torch.zeros(N, dtype=torch.int32, device="cuda")
    steps = 0
    if N and len(idx):
        labels[torch.from_numpy(idx).cuda()] = torch.from_numpy(lab).cuda()
        mask_dev = upload()
        labels *= (mask_dev != 0).to(torch.int32)                    # (seeds outside the mask are ignored, as the growth ignores them)
        arrival, counts = L.geodesic_device((labels != 0).to(torch.uint8), mask_dev, shp, connectivity)
        steps = len(counts) - 1
        label_spread_device(arrival, labels, shp, steps, connectivity)
    vox = np.zeros(nb, np.int64)
    if nb and N:
        vox[:] = np.asarray(V.component_stats_device(labels, shp, nb)["voxels"], np.int64)
    return BranchTerritories(labels=labels if return_device else V._host_of(labels, np.int32, shp), shape=shp, voxels=vox,
                             ml=vox.astype(np.float64) * float(np.prod(np.asarray(graph.pixdim, np.float64))) / 1000.0, steps=steps)


# ---- the chains -------------------------------------------------------------------------------------------------------------------------------------------------------
def generation_table(graph, tree, territories=None):
    """branches, total length, territory voxels / ml and the mean calibre (the branches' mean radii weighted by their voxel count) per generation"""
    gens = sorted({int(g) for g in tree.generation.tolist() if g >= 0})
    t = np.zeros(len(gens), GENERATION_DTYPE)
    for i, g in enumerate(gens):
        ids = np.flatnonzero(tree.generation == g).tolist()
        w = np.asarray([len(graph.branches[b].path) for b in ids], np.float64)
        r = np.asarray([graph.branches[b].radius_mean for b in ids], np.float64)
        vox = int(territories.voxels[ids].sum()) if territories is not None else 0
        t[i] = (g, len(ids), float(sum(graph.branches[b].length_mm for b in ids)), vox, float(territories.ml[ids].sum()) if territories is not None else 0.0,
                float((r * w).sum() / w.sum()) if len(ids) and not np.isnan(r).any() else np.nan)
    return t


def _check_tree_args(kw, what, close=1):
    bad = set(kw) - _TREE_KEYS
    if bad:
        raise ValueError(f"{what} takes {sorted(_TREE_KEYS)}, not {sorted(bad)}")
    a = dict(endpoints=True, max_iterations=None, min_length_mm=MIN_LENGTH_MM, min_ratio=MIN_RATIO, connectivity=3, pixdim=None, orientation=None, affine=None, root=None,
             territories=True, shape=None, close=close, fill=True)
    a.update(kw)
    if not L._is_int(a["close"]) or not 0 <= int(a["close"]) <= 8:
        raise ValueError(f"close is an integer in 0..8 (iterations of the 26-neighbourhood closing), not {a['close']!r}")
    L._check_bool(a["fill"], "fill")
    _check_thin_args(a["endpoints"], a["max_iterations"])
    _check_positive_or_none(a["min_length_mm"], "min_length_mm"); _check_positive_or_none(a["min_ratio"], "min_ratio")
    V._check_connectivity(a["connectivity"])
    L._check_bool(a["territories"], "territories")
    if a["pixdim"] is not None:
        V._check_pixdim(a["pixdim"])
    if a["orientation"] is not None:
        V._check_orientation(a["orientation"])
    if a["affine"] is not None and (np.shape(a["affine"]) != (4, 4) or not np.isfinite(np.asarray(a["affine"], np.float64)).all()):
        raise ValueError("affine is a finite 4 x 4 matrix")
    return a


def _tree(mask, a, root):
    sec = {}
    p = V._check_pixdim((1.0, 1.0, 1.0) if a["pixdim"] is None else a["pixdim"])
    orientation = a["orientation"] if a["orientation"] is not None else a["affine"]
    if root == "superior":
        _superior_axis(orientation)                                  # refused before any device work
    upload, shp = _mask_source(mask, a["shape"])
    if max(shp) > V.EDT_MAX_DIM:
        raise ValueError(f"the calibre comes from the distance transform, which takes at most {V.EDT_MAX_DIM} voxels per axis, not {shp}")
    torch = V._torch()
    t_all = t0 = time.perf_counter()
    mask_dev = upload()
    if int(a["close"]) > 0 and mask_dev.numel():                     # a noisy mask is full of one-voxel cavities and tunnels, and thinning keeps every one of them
        wide = V.morph_device(mask_dev, shp, "dilate", 3, int(a["close"]), 0)[0]
        mask_dev = V.morph_device(wide, shp, "erode", 3, int(a["close"]), 1)[0]          # (border 1: the erosion does not eat into what touches a face)
    if a["fill"] and mask_dev.numel():
        mask_dev = V.fill_holes_device(mask_dev, shp, 1)[0]
    torch.cuda.synchronize(); sec["prepare"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    thin, removed = thin_device(mask_dev, shp, a["endpoints"], a["max_iterations"])
    skel = Skeleton(mask=thin, shape=shp, iterations=len(removed), removed=removed, voxels=int(torch.count_nonzero(thin).item()) if thin.numel() else 0,
                    endpoints=bool(a["endpoints"]), seconds={})
    torch.cuda.synchronize(); sec["thin"] = skel.seconds["thin"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    d2 = V.edt_sq_device(mask_dev, shp, p, features_nonzero=False) if int(np.prod(shp)) else None
    index, nbr, vals = table_device(thin, shp, d2)
    del d2
    table = _finish_table(index, nbr, shp, np.sqrt(vals) if vals is not None else np.zeros(0))
    torch.cuda.synchronize(); sec["table"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    graph = prune(graph_from_table(table, shp, p, a["affine"]), a["min_length_mm"], a["min_ratio"])
    tree = root_tree(graph, root, orientation)
    sec["graph"] = time.perf_counter() - t0
    terr = None
    if a["territories"]:
        t0 = time.perf_counter()
        terr = branch_territories(mask_dev, skel, graph, a["connectivity"], shape=shp)
        torch.cuda.synchronize(); sec["territories"] = time.perf_counter() - t0
    skel.mask = V._host_of(thin, np.uint8, shp)
    sec["total"] = time.perf_counter() - t_all
    return CenterlineTree(mask=V._host_of(mask_dev, np.uint8, shp), skeleton=skel, graph=graph, tree=tree, territories=terr, generations=generation_table(graph, tree, terr),
                          cycles=int(graph.components["cycles"].sum()) if len(graph.components) else 0, seconds=sec)


def airway_tree(airways, **kw):
    """The airway tree of an airway mask -> CenterlineTree: thin_volume, skeleton_graph with the mask's own distance transform as the calibre, prune, root_tree at the
    superior end, branch_territories.  airways: a lungs.LungMask whose airway step ran (its AirwayGrowth's mask and its pixdim are taken), an AirwayGrowth, or a mask
    source (with pixdim=).  The superior end comes from orientation= (a code such as "LPS", or an affine) or affine= (which also gives the nodes world coordinates);
    without either it is a ValueError: superior is not guessed.  The mask is prepared first: close iterations (default 1) of closing with the 26-neighbourhood -- the
    dilations see background outside the volume, the erosions foreground, so nothing is eaten at a face -- and, with fill (default True), fill_holes: a thresholded mask
    is full of one-voxel cavities and tunnels, and a topology-preserving thinning keeps a shell around each.  The calibre and the territories refer to the prepared mask
    (res.mask).  Keywords: close, fill, endpoints, max_iterations, min_length_mm, min_ratio, connectivity, pixdim, orientation, affine,
    root (default "superior"), territories, shape.  A cycle in an airway tree marks a leak: the growth left the tree and came back."""
    a = _check_tree_args(kw, "airway_tree")
    if isinstance(airways, L.LungMask):
        if airways.airways is None:
            raise ValueError(f"the lung mask's airway step did not run ({airways.airway_error}): there is no airway to thin")
        if a["pixdim"] is None:
            a["pixdim"] = airways.pixdim
        if a["shape"] is None and isinstance(airways.airways.mask, V._torch().Tensor):
            a["shape"] = airways.shape
        airways = airways.airways.mask
    elif isinstance(airways, L.AirwayGrowth):
        airways = airways.mask
    return _tree(airways, a, "superior" if a["root"] is None else a["root"])


def vessel_tree(vessel_mask, **kw):
    """The vessel trees of a vessel mask -> CenterlineTree, as airway_tree, rooted per component at its thickest end.  vessel_mask: a vessels.VesselMask (its mask and
    its vesselness' pixdim are taken) or a mask source (with pixdim=).  The same keywords; root defaults to "thickest" and close to 0: a closing with the
    26-neighbourhood would join vessels that run two voxels apart into cycles that are not there, so only the holes are filled (fill=True).  As in airway_tree the
    calibre and the territories refer to the prepared mask (res.mask), which differs from the caller's by the filled holes."""
    a = _check_tree_args(kw, "vessel_tree", close=0)
    from . import vessels as VS
    if isinstance(vessel_mask, VS.VesselMask):
        if a["pixdim"] is None:
            a["pixdim"] = vessel_mask.vesselness.pixdim
        if a["shape"] is None and isinstance(vessel_mask.mask, V._torch().Tensor):
            a["shape"] = vessel_mask.vesselness.shape
        vessel_mask = vessel_mask.mask
    return _tree(vessel_mask, a, "thickest" if a["root"] is None else a["root"])

"""The definition of volume.extract_surface in numpy: marching tetrahedra on the Freudenthal split of every lattice cell.  A cell, the cube between
lattice points p and p + (1, 1, 1), is cut into six tetrahedra, one per axis order; every tetrahedron edge runs from a lattice point q to q + d, d one of seven directions, so
a vertex belongs to (q, edge type) and the mesh is indexed without welding.  Vertex ids, triangle order, winding, the interpolation parameter t and the stored float32 of a
vertex are all part of the contract: the device is compared with this file bit for bit.  Vectorised numpy, one rounded float64 operation at a time."""
import numpy as np

DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))          # edge types 0..6
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))                # T0..T5: xyz, xzy, yxz, yzx, zxy, zyx
CHUNK = 256                                                         # unet_vol_group_moments' partial sums


def tet_corners(n):
    """the four corners of tetrahedron n as offsets from the cell's point p: v0 = p, v1 = v0 + e_first, v2 = v1 + e_second, v3 = p + (1, 1, 1)"""
    a, b, _ = ORDERS[n]
    v0 = np.zeros(3, np.int64)
    v1 = v0.copy(); v1[a] = 1
    v2 = v1.copy(); v2[b] = 1
    return np.stack([v0, v1, v2, np.ones(3, np.int64)])


def edge_type(d):
    return DIRS.index(tuple(int(v) for v in d))


def case_edges(case):
    """the triangles of a case as lists of tetrahedron edges (i, o), i the inside corner, before the winding rule"""
    ins = [k for k in range(4) if (case >> k) & 1]
    out = [k for k in range(4) if not (case >> k) & 1]
    if len(ins) == 1:
        return [[(ins[0], o) for o in out]]
    if len(ins) == 3:
        return [[(i, out[0]) for i in ins]]
    if len(ins) == 2:
        q = [(ins[0], out[0]), (ins[0], out[1]), (ins[1], out[1]), (ins[1], out[0])]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def derive_table():
    """table[n][case] -> list of triangles, each three (inside corner, outside corner) pairs of tetrahedron n, wound so that the normal of the triangle of edge midpoints
    points from the inside corners' centroid to the outside corners'"""
    table = []
    for n in range(6):
        v = tet_corners(n).astype(np.float64)
        row = []
        for case in range(16):
            tris = []
            ins = [k for k in range(4) if (case >> k) & 1]
            out = [k for k in range(4) if not (case >> k) & 1]
            for tri in case_edges(case):
                m = [(v[i] + v[o]) * 0.5 for i, o in tri]
                nrm = np.cross(m[1] - m[0], m[2] - m[0])
                if np.dot(nrm, v[out].mean(0) - v[ins].mean(0)) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                tris.append(tri)
            row.append(tris)
        table.append(row)
    return table


PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))            # a tetrahedron's six edges as (lower corner, upper corner): the code of an edge in the packed table


def packed_table():
    """the kernel's constant: word[n][case] = number of triangles | code of vertex j << (4 + 3 j), vertices 0..2 the first triangle, 3..5 the second; a code indexes PAIRS"""
    t = derive_table()
    words = np.zeros((6, 16), np.uint32)
    for n in range(6):
        for case in range(16):
            w = len(t[n][case])
            for j, (i, o) in enumerate(e for tri in t[n][case] for e in tri):
                w |= PAIRS.index((min(i, o), max(i, o))) << (4 + 3 * j)
            words[n, case] = w
    return words


def same_bits(got, want):
    """equality of the stored bits, NaN-aware: a NaN matches any NaN, everything else bit for bit"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    both = np.isnan(got) & np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.array_equal(np.where(both, 0, np.ascontiguousarray(got).view(u)), np.where(both, 0, np.ascontiguousarray(want).view(u))))


def default_matrix(pixdim=(1.0, 1.0, 1.0)):
    m = np.zeros((3, 4), np.float64)
    m[0, 0], m[1, 1], m[2, 2] = pixdim
    return m


class Mesh:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _pad(a, pad, value):
    return np.pad(a, pad, constant_values=value) if pad else a


def _shift(a, d):
    """a at q + d for every q where q + d exists"""
    return a[d[0]:, d[1]:, d[2]:]


def _low(a, d):
    return a[:a.shape[0] - d[0], :a.shape[1] - d[1], :a.shape[2] - d[2]]


def extract(mask=None, labels=None, values=None, iso=None, select=0, closed=True, pad_value=None, matrix=None):
    """Exactly one of mask (non-zero = inside), labels (int32; select = 0: any non-zero label, else that label) and values (decoded float64; inside = value > iso, a NaN is
    outside) -> Mesh(vertices float32 [nv, 3], triangles int32 [nt, 3], groups int32 [nt], flags uint8 [lattice], counts uint8 [lattice]: the flag byte of every lattice point
    and the triangle count of the cell it starts, in Fortran order)."""
    M = default_matrix() if matrix is None else np.asarray(matrix, np.float64).reshape(3, 4)
    pad = 1 if closed else 0
    lab = None
    if mask is not None:
        ins = np.asarray(mask) != 0
    elif labels is not None:
        lab = np.asarray(labels).astype(np.int32)
        ins = (lab != 0) if select == 0 else (lab == select)
    else:
        val = np.asarray(values, np.float64)
        with np.errstate(invalid="ignore"):
            ins = val > np.float64(iso)
        val = _pad(val, pad, np.float64(iso if pad_value is None else pad_value))
    ins = _pad(ins, pad, False)
    if lab is not None:
        lab = _pad(lab, pad, 0)
    P = ins.shape
    npts = int(np.prod(P))
    empty = Mesh(vertices=np.zeros((0, 3), np.float32), triangles=np.zeros((0, 3), np.int32), groups=np.zeros(0, np.int32), flags=np.zeros(npts, np.uint8),
                 counts=np.zeros(npts, np.uint8), lattice=P)
    if npts == 0 or min(P) < 2:                                       # no voxels, or an unpadded extent of 1: no cells, an empty mesh
        return empty
    # ---- vertices: one per crossed edge, owned by its lower endpoint; id = rank of (point in Fortran order, edge type)
    cross = np.zeros((7,) + P, bool)
    for e, d in enumerate(DIRS):
        if all(P[r] > d[r] for r in range(3)):
            cross[e][:P[0] - d[0], :P[1] - d[1], :P[2] - d[2]] = _low(ins, d) != _shift(ins, d)
    flat = cross.reshape(-1, order="F")                               # e fastest, then x, y, z
    vid = (np.cumsum(flat, dtype=np.int64) - 1).reshape(cross.shape, order="F")
    flags = (cross * (1 << np.arange(7)).reshape(7, 1, 1, 1)).sum(0).astype(np.uint8).reshape(-1, order="F")
    e_i, x_i, y_i, z_i = np.unravel_index(np.flatnonzero(flat), cross.shape, order="F")
    d_i = np.asarray(DIRS, np.int64)[e_i]
    q = np.stack([x_i, y_i, z_i], 1)
    t = np.full(e_i.size, 0.5, np.float64)
    if values is not None and e_i.size:
        a = val[x_i, y_i, z_i]
        b = val[x_i + d_i[:, 0], y_i + d_i[:, 1], z_i + d_i[:, 2]]
        fin = np.isfinite(a) & np.isfinite(b)
        with np.errstate(all="ignore"):
            t = np.where(fin, (np.float64(iso) - a) / (b - a), 0.5)
    with np.errstate(invalid="ignore"):
        c = (q - pad).astype(np.float64) + t[:, None] * d_i.astype(np.float64)
        vertices = np.stack([((M[r, 0] * c[:, 0] + M[r, 1] * c[:, 1]) + M[r, 2] * c[:, 2]) + M[r, 3] for r in range(3)], 1).astype(np.float32)
    # ---- triangles: (cell in Fortran order, tetrahedron, table order)
    counts = np.zeros(P, np.uint8)
    table = derive_table()
    C = tuple(p - 1 for p in P)
    cell_f = (np.arange(C[0])[:, None, None] + P[0] * (np.arange(C[1])[None, :, None] + P[1] * np.arange(C[2])[None, None, :])).astype(np.int64)
    keys, tris, grps = [], [], []
    for n in range(6):
        v = tet_corners(n)
        corner = [_low(_shift(ins, v[k]), 1 - v[k]) for k in range(4)]          # ins at p + v_k for every cell p
        case = sum(corner[k].astype(np.int64) << k for k in range(4))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)
            if sel[0].size == 0:
                continue
            p = np.stack(sel, 1)
            counts[sel] += len(table[n][cs])
            for j, tri in enumerate(table[n][cs]):
                ids = []
                for i, o in tri:
                    lo, hi = min(i, o), max(i, o)
                    own = p + v[lo]
                    ids.append(vid[edge_type(v[hi] - v[lo]), own[:, 0], own[:, 1], own[:, 2]])
                keys.append(cell_f[sel] * 12 + n * 2 + j)
                tris.append(np.stack(ids, 1))
                src = p + v[tri[0][0]]
                grps.append(lab[src[:, 0], src[:, 1], src[:, 2]] if lab is not None else np.ones(p.shape[0], np.int32))
    if not keys:
        return Mesh(vertices=vertices, triangles=empty.triangles, groups=empty.groups, flags=flags, counts=counts.reshape(-1, order="F"), lattice=P)
    order = np.argsort(np.concatenate(keys), kind="stable")
    return Mesh(vertices=vertices, triangles=np.concatenate(tris)[order].astype(np.int32), groups=np.concatenate(grps)[order].astype(np.int32), flags=flags,
                counts=counts.reshape(-1, order="F"), lattice=P)


def measure(vertices, triangles):
    """per triangle, float64 from the stored float32 vertices: area = fl(0.5 sqrt((c_x^2 + c_y^2) + c_z^2)), c = (b - a) x (c - a); signed volume = fl(((a_x n_x + a_y n_y) +
    a_z n_z) / 6), n = b x c; every operation rounded on its own"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    tr = np.asarray(triangles, np.int64).reshape(-1, 3)
    a, b, c = v[tr[:, 0]], v[tr[:, 1]], v[tr[:, 2]]

    def cross(u, w):
        return u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    with np.errstate(all="ignore"):
        cx, cy, cz = cross(b - a, c - a)
        area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
        nx, ny, nz = cross(b, c)
        vol = ((a[:, 0] * nx + a[:, 1] * ny) + a[:, 2] * nz) / 6.0
    return area, vol


def two_level_sum(run):
    """unet_vol_group_moments' sum: partials of 256 elements left to right from their first element, then the partials left to right"""
    run = np.asarray(run, np.float64)
    if run.size == 0:
        return np.float64(0.0)
    partials = np.array([np.cumsum(run[c:c + CHUNK])[-1] for c in range(0, run.size, CHUNK)], np.float64)
    return np.cumsum(partials)[-1]


def group_sums(per_triangle, groups, ids):
    """the two-level sum of a per-triangle quantity over the triangles of every group of `ids`, in triangle order (a stable sort by group keeps it)"""
    g = np.asarray(groups)
    order = np.argsort(g, kind="stable")
    sg, sv = g[order], np.asarray(per_triangle, np.float64)[order]
    lo, hi = np.searchsorted(sg, ids, side="left"), np.searchsorted(sg, ids, side="right")
    return np.array([two_level_sum(sv[a:b]) for a, b in zip(lo, hi)], np.float64)


def shape_fields(area, vol):
    """sphericity = pi^(1/3) (6 V)^(2/3) / A and A / V, nan where undefined"""
    area, vol = np.asarray(area, np.float64), np.asarray(vol, np.float64)
    with np.errstate(all="ignore"):
        sph = np.where((area > 0) & (vol > 0), np.pi ** (1.0 / 3.0) * np.power(6.0 * np.abs(vol), 2.0 / 3.0) / area, np.nan)
        s2v = np.where(vol > 0, area / vol, np.nan)
    return sph, s2v


# ---- topology ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def directed_edges(triangles):
    tr = np.asarray(triangles, np.int64).reshape(-1, 3)
    return np.concatenate([tr[:, [0, 1]], tr[:, [1, 2]], tr[:, [2, 0]]])


def is_closed_manifold(triangles):
    """every directed edge occurs once and its reverse once"""
    e = directed_edges(triangles)
    if e.size == 0:
        return True
    n = int(e.max()) + 1
    k = e[:, 0] * n + e[:, 1]
    u, c = np.unique(k, return_counts=True)
    return bool((c == 1).all() and np.array_equal(u, np.unique(e[:, 1] * n + e[:, 0])))


def euler(nv, triangles):
    """V - E + F with E = 3 F / 2 on a closed mesh"""
    nt = int(np.asarray(triangles).reshape(-1, 3).shape[0])
    return int(nv) - nt // 2


# ---- shapes the tests share -----------------------------------------------------------------------------------------------------------------------------------------------
def pattern_volume():
    """(48, 48, 2): each of the 256 corner patterns as a 2 x 2 x 2 block, a one-voxel gap of background between blocks"""
    m = np.zeros((48, 48, 2), np.uint8)
    for pat in range(256):
        bx, by = 3 * (pat % 16), 3 * (pat // 16)
        for c in range(8):
            if (pat >> c) & 1:
                m[bx + (c & 1), by + ((c >> 1) & 1), (c >> 2) & 1] = 1
    return m


def ball_field(shape, centre, r):
    """r - |x - c| on the voxel grid, float64"""
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return r - np.sqrt(sum((g[a] - centre[a]) ** 2 for a in range(3)))


def torus_field(shape, centre, R, r):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    rho = np.sqrt((g[0] - centre[0]) ** 2 + (g[1] - centre[1]) ** 2)
    return r - np.sqrt((rho - R) ** 2 + (g[2] - centre[2]) ** 2)

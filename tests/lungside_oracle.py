"""CPU restatement of the left / right lung split and the per-lung burden (csrc/kernels_lungside.hip, covidseg_amd.volume.split_lungs / lung_burden; DESIGN.md section
4u) in numpy, on the definitions the other oracles already state: components_oracle.label / stats (the labelling and its numbering), morph_oracle.erode_mm and
volscore_oracle.edt_sq_lines (the exact squared distance transform as a sequence of IEEE double operations).  tests/test_lungside_host.py pins the pieces against
scipy.ndimage.  Every device test against this file is an equality."""
import itertools

import numpy as np

import components_oracle as CO
import morph_oracle as MO
import volscore_oracle as SO

MIN_RATIO = 0.25
ERODE_MM = (1, 2, 3, 4, 5, 6, 8, 10)
LETTERS = (("L", "R"), ("P", "A"), ("I", "S"))                       # per world axis of RAS+: (negative, positive)


class SplitError(ValueError):
    pass


def all_axcodes():
    """the 48 signed axis permutations as letter triples"""
    return [tuple(LETTERS[w][s] for w, s in zip(perm, signs)) for perm in itertools.permutations(range(3)) for signs in itertools.product((0, 1), repeat=3)]


def affine_of(codes, pixdim=(1.0, 1.0, 1.0)):
    """axis-aligned: voxel axis j grows by pixdim[j] along the world direction of its letter"""
    m = np.zeros((4, 4)); m[3, 3] = 1.0
    for j, c in enumerate(codes):
        w = [k for k, pair in enumerate(LETTERS) if c in pair][0]
        m[w, j] = pixdim[j] if LETTERS[w][1] == c else -pixdim[j]
    return m


def two_largest(counts):
    """indices (0-based) of the two components with the most voxels, ties to the lower label"""
    counts = np.asarray(counts, np.int64)
    return np.lexsort((np.arange(counts.size), -counts))[:2]


def seeds(mask, pixdim=(1, 1, 1), connectivity=1, min_ratio=MIN_RATIO, erode_mm=ERODE_MM):
    """-> (radius, labels of the candidate, the 0-based indices of A and B, component statistics); SplitError when no radius qualifies"""
    m = np.asarray(mask) != 0
    best = (0, 0)
    for r in (0,) + tuple(erode_mm):
        cand = m if r == 0 else MO.erode_mm(m, r, pixdim) != 0
        lab, n = CO.label(cand, connectivity)
        st = CO.stats(lab, n)
        ab = two_largest(st["voxels"])
        counts = tuple(int(st["voxels"][k]) for k in ab) + (0,) * (2 - len(ab))
        best = max(best, counts)
        if n >= 2 and float(counts[1]) >= min_ratio * float(counts[0]):
            return r, lab, ab, st
    raise SplitError(f"no radius separates two lungs; the largest two counts seen were {best[0]} and {best[1]}")


def world_x(affine, st, k):
    cnt = float(st["voxels"][k])
    c = (float(st["sx"][k]) / cnt, float(st["sy"][k]) / cnt, float(st["sz"][k]) / cnt)
    a = np.asarray(affine, np.float64)
    return float(a[0, 0]) * c[0] + float(a[0, 1]) * c[1] + float(a[0, 2]) * c[2]


def side_assign(mask, d2_a, d2_b, side_a=1, side_b=2):
    """-> (sides uint8, counts int64 [3]): the nearer seed's side on the mask, a tie to the seed whose side is 1"""
    m = np.asarray(mask) != 0
    if side_a == 1:
        s = np.where(d2_a <= d2_b, side_a, side_b)
    else:
        s = np.where(d2_b <= d2_a, side_b, side_a)
    sides = np.where(m, s, 0).astype(np.uint8)
    return sides, np.bincount(sides.reshape(-1), minlength=3).astype(np.int64)


def split(mask, affine, pixdim=(1, 1, 1), connectivity=1, min_ratio=MIN_RATIO, erode_mm=ERODE_MM):
    """-> dict: sides (0 / 1 = the patient's left / 2 = right), radius_mm, voxels (left, right), seed_voxels (left, right), d2_left, d2_right"""
    m = np.asarray(mask) != 0
    r, lab, ab, st = seeds(m, pixdim, connectivity, min_ratio, erode_mm)
    xa, xb = world_x(affine, st, ab[0]), world_x(affine, st, ab[1])
    if xa == xb:
        raise SplitError("the two seeds have the same world x")
    left, right = (ab[0], ab[1]) if xa < xb else (ab[1], ab[0])      # RAS+: +x is the patient's right
    d2l, d2r = SO.edt_sq_lines(lab == left + 1, True, pixdim), SO.edt_sq_lines(lab == right + 1, True, pixdim)
    sides, counts = side_assign(m, d2l, d2r)
    return {"sides": sides, "radius_mm": float(r), "voxels": (int(counts[1]), int(counts[2])), "seed_voxels": (int(st["voxels"][left]), int(st["voxels"][right])),
            "d2_left": d2l, "d2_right": d2r}


def side_table(sides, infection=None, labels=None, n=0):
    """-> (totals int64 [2, 3], lesion_side int64 [n, 3], per_slice int64 [Z, 6]); a side value above 2 counts as 0, a label outside 1..n is ignored"""
    s = np.asarray(sides).astype(np.int64)
    s = np.where(s > 2, 0, s)
    Z = s.shape[2]
    inf = np.zeros(s.shape, bool) if infection is None else np.asarray(infection) != 0
    totals = np.zeros((2, 3), np.int64)
    totals[0] = np.bincount(s.reshape(-1), minlength=3)
    totals[1] = np.bincount(s[inf], minlength=3)
    les = np.zeros((n, 3), np.int64)
    if labels is not None and n > 0:
        l = np.asarray(labels).astype(np.int64)
        ok = (l >= 1) & (l <= n)
        np.add.at(les, (l[ok] - 1, s[ok]), 1)
    ps = np.zeros((Z, 6), np.int64)
    for z in range(Z):
        sz, iz = s[:, :, z], inf[:, :, z]
        ps[z, :5] = [(sz == 1).sum(), (sz == 2).sum(), (iz & (sz == 0)).sum(), (iz & (sz == 1)).sum(), (iz & (sz == 2)).sum()]
    return totals, les, ps


def burden(infection, sides, labels=None, n=None, pixdim=(1, 1, 1), connectivity=1):
    """what volume.lung_burden reports, from side_table"""
    if labels is None:
        labels, n = CO.label(np.asarray(infection) != 0, connectivity)
    totals, les, ps = side_table(sides, infection, labels, n)
    ml = float(np.prod(np.asarray(pixdim, np.float64))) / 1000.0
    out = {"outside_ml": int(totals[1, 0]) * ml, "per_slice": ps, "lesion_side": les}
    for name, k in (("left", 1), ("right", 2)):
        lung, infd = int(totals[0, k]) * ml, int(totals[1, k]) * ml
        out[name] = {"lung_ml": lung, "infected_ml": infd, "fraction": infd / lung if totals[0, k] else float("nan")}
    inlung = les[:, 1] + les[:, 2]
    out["side"] = np.where(inlung == 0, "none", np.where(les[:, 1] >= les[:, 2], "left", "right"))
    out["bilateral"] = bool(out["left"]["fraction"] > 0 and out["right"]["fraction"] > 0)
    return out


# ---- phantoms: built in a canonical frame whose voxel axes grow to the patient's Right, Anterior, Superior, then stored in any orientation ----------------------------
def reorient(vol_ras, codes):
    """the canonical-frame volume as a file with axis codes `codes` would store it: stored axis j runs along the world axis of its letter, backwards for L / P / I"""
    perm = [[k for k, pair in enumerate(LETTERS) if c in pair][0] for c in codes]
    out = np.transpose(vol_ras, perm)
    for j, c in enumerate(codes):
        if c in "LPI":
            out = np.flip(out, axis=j)
    return np.ascontiguousarray(out)


def to_canonical(vol, codes):
    """the inverse of reorient"""
    perm = [[k for k, pair in enumerate(LETTERS) if c in pair][0] for c in codes]
    out = vol
    for j, c in enumerate(codes):
        if c in "LPI":
            out = np.flip(out, axis=j)
    return np.ascontiguousarray(np.transpose(out, np.argsort(perm)))


def reorient_pixdim(pixdim_ras, codes):
    return tuple(pixdim_ras[[k for k, pair in enumerate(LETTERS) if c in pair][0]] for c in codes)


def boxes(shape, a, b, bridge=None):
    """two boxes a, b = ((x0, x1), (y0, y1), (z0, z1)) (half-open) and an optional bridge box"""
    m = np.zeros(shape, np.uint8)
    for box in (a, b) + ((bridge,) if bridge else ()):
        m[tuple(slice(lo, hi) for lo, hi in box)] = 1
    return m


def fused_lungs(shape, pixdim, gap=0.0):
    """two ellipsoids side by side along axis 0 (in mm), overlapping in a narrow junction when gap <= 0; the one at low x is smaller"""
    X, Y, Z = shape
    g = np.meshgrid(*(np.arange(n) * p for n, p in zip(shape, pixdim)), indexing="ij")
    ext = [n * p for n, p in zip(shape, pixdim)]
    ra, rb = 0.235 * ext[0] - gap / 2, 0.265 * ext[0] - gap / 2
    ca, cb = (0.26 * ext[0], 0.5 * ext[1], 0.5 * ext[2]), (0.735 * ext[0], 0.52 * ext[1], 0.5 * ext[2])
    ea = ((g[0] - ca[0]) / ra) ** 2 + ((g[1] - ca[1]) / (0.38 * ext[1])) ** 2 + ((g[2] - ca[2]) / (0.45 * ext[2])) ** 2 <= 1.0
    eb = ((g[0] - cb[0]) / rb) ** 2 + ((g[1] - cb[1]) / (0.40 * ext[1])) ** 2 + ((g[2] - cb[2]) / (0.45 * ext[2])) ** 2 <= 1.0
    return (ea | eb).astype(np.uint8)

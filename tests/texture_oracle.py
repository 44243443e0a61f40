"""numpy restatement of csrc/kernels_texture.hip (include/unet_hip.h states the same rule by rule): the grey levels, the co-occurrence counts by shifted-view
comparison, the run-length counts by walking every run one step at a time -- everything the device counts is compared with this for equality -- and an independent
computation of texture.py's features: the non-logarithmic ones exactly, from the integer counts with fractions.Fraction, the entropies with math.fsum."""
import math
from fractions import Fraction

import numpy as np

from intensity_oracle import DTYPES, decode, group_of          # noqa: F401  (the decode and the groups are those of the intensity kernels)

DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))
U = 2.0 ** -53                                                       # the float64 unit round-off


def indices_of(bits):
    return [k for k in range(13) if (bits >> k) & 1]


# ---- the counts -------------------------------------------------------------------------------------------------------------------------------------------
def quantize(val, g, n, lo, width, Ng, drop):
    """-> (levels uint8 [X, Y, Z]: 0 = takes no part, level_counts int64 [n, Ng]); q = floor((v - lo) / width), two rounded operations"""
    val = np.asarray(val, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((val - np.float64(lo)) / np.float64(width))
    take = (g > 0) & ~np.isnan(val)
    if drop:
        take &= (q >= 0) & (q < Ng)
    lev = np.where(take, np.clip(np.where(take, q, 0.0), 0, Ng - 1) + 1, 0).astype(np.uint8)
    lc = np.zeros((n, Ng), np.int64)
    if take.any():
        np.add.at(lc, (g[take] - 1, lev[take].astype(np.int64) - 1), 1)
    return lev, lc


def _views(shape, off):
    """the slices of p and of q = p + off with both inside the volume (empty when an offset reaches the dimension)"""
    sp, sq = [], []
    for dim, o in zip(shape, off):
        if abs(o) >= dim:
            return None, None
        sp.append(slice(0, dim - o) if o >= 0 else slice(-o, dim))
        sq.append(slice(o, dim) if o >= 0 else slice(0, dim + o))
    return tuple(sp), tuple(sq)


def glcm(levels, g, n, Ng, distance, bits, merge=False):
    """-> int64 [n, K, Ng, Ng]: C[g - 1, k, a - 1, b - 1] over the pairs (p, p + distance dir_k); g: int64 group volume (0 = none)"""
    idx = indices_of(bits)
    K = 1 if merge else len(idx)
    C = np.zeros((n, K, Ng, Ng), np.int64)
    lv = np.asarray(levels).astype(np.int64)
    lv = np.where(lv <= Ng, lv, 0)
    for kk, k in enumerate(idx):
        sp, sq = _views(lv.shape, tuple(distance * d for d in DIRECTIONS[k]))
        if sp is None:
            continue
        a, b, gp, gq = lv[sp], lv[sq], g[sp], g[sq]
        ok = (a > 0) & (b > 0) & (gp > 0) & (gp == gq)
        flat = (((gp[ok] - 1) * K + (0 if merge else kk)) * Ng + (a[ok] - 1)) * Ng + (b[ok] - 1)
        C += np.bincount(flat, minlength=C.size).reshape(C.shape)
    return C


def runs(levels, g, n, Ng, bits, max_run):
    """-> (int64 [n, K, Ng, max_run], clamped int64 [n, K]): every maximal run of one level and one group along dir_k, walked from its first voxel one step at a time"""
    idx = indices_of(bits)
    R, clamped = np.zeros((n, len(idx), Ng, max_run), np.int64), np.zeros((n, len(idx)), np.int64)
    lv = np.asarray(levels).astype(np.int64)
    lv = np.where((lv <= Ng) & (g > 0), lv, 0)
    key = np.where(lv > 0, g * 256 + lv, 0)                          # what a run holds constant
    shape = np.array(lv.shape)
    for kk, k in enumerate(idx):
        d = np.array(DIRECTIONS[k])
        pos = np.argwhere(key > 0)
        if not len(pos):
            continue
        prev = pos - d
        inside = ((prev >= 0) & (prev < shape)).all(axis=1)
        same = np.zeros(len(pos), bool)
        same[inside] = key[tuple(prev[inside].T)] == key[tuple(pos[inside].T)]
        start = pos[~same]
        k0 = key[tuple(start.T)]
        length = np.ones(len(start), np.int64)
        alive, cur = np.arange(len(start)), start.copy()
        while len(alive):                                           # one step per round: the runs that go on stay alive
            cur = cur + d
            inside = ((cur >= 0) & (cur < shape)).all(axis=1)
            on = np.zeros(len(alive), bool)
            on[inside] = key[tuple(cur[inside].T)] == k0[alive[inside]]
            alive, cur = alive[on], cur[on]
            length[alive] += 1
        gi, ai = k0 // 256 - 1, k0 % 256 - 1
        np.add.at(R, (gi, kk, ai, np.minimum(length, max_run) - 1), 1)
        np.add.at(clamped, (gi[length > max_run], kk), 1)
    return R, clamped


# ---- the features ------------------------------------------------------------------------------------------------------------------------------------------
# name -> (value, bound).  The value of a non-logarithmic feature is the exact rational number, rounded once by float().  bound = (terms + 8) 2^-53 sum |term| over
# the terms the feature is the sum of (a feature formed as one ratio of integers has one term, itself); an entropy adds 2 ulp of every logarithm term.
def _bound(terms, log_terms=()):
    t = [abs(float(v)) for v in terms]
    return (len(t) + 8) * U * math.fsum(t) + 2 * U * math.fsum(abs(float(v)) for v in log_terms)


def glcm_features_exact(C):
    """one count matrix [Ng, Ng] -> {feature: (value, bound)}, or None for an empty matrix"""
    C = np.asarray(C)
    Ng = C.shape[0]
    S = [[int(C[a, b]) + int(C[b, a]) for b in range(Ng)] for a in range(Ng)]
    T = sum(sum(r) for r in S)
    if T == 0:
        return None
    ent = [(a + 1, b + 1, Fraction(S[a][b], T)) for a in range(Ng) for b in range(Ng) if S[a][b]]
    mu = sum(i * p for i, j, p in ent)
    var = sum((i - mu) ** 2 * p for i, j, p in ent)
    out = {}

    def put(name, terms):
        out[name] = (float(sum(terms)), _bound(terms))

    put("joint_energy", [p * p for i, j, p in ent])
    put("contrast", [(i - j) ** 2 * p for i, j, p in ent])
    put("dissimilarity", [abs(i - j) * p for i, j, p in ent])
    put("inverse_difference", [p / (1 + abs(i - j)) for i, j, p in ent])
    put("inverse_difference_moment", [p / (1 + (i - j) ** 2) for i, j, p in ent])
    put("autocorrelation", [i * j * p for i, j, p in ent])
    put("maximum_probability", [max(p for i, j, p in ent)])
    put("sum_of_squares", [var])
    put("correlation", [(sum(i * j * p for i, j, p in ent) - mu * mu) / var if var else Fraction(1)])
    put("cluster_shade", [sum((i + j - 2 * mu) ** 3 * p for i, j, p in ent)])
    put("cluster_prominence", [sum((i + j - 2 * mu) ** 4 * p for i, j, p in ent)])
    logs = [math.log2(T)] + [S[i - 1][j - 1] * math.log2(S[i - 1][j - 1]) / T for i, j, p in ent]          # the terms of log2 T - sum S log2 S / T
    out["joint_entropy"] = (math.fsum(float(p) * (math.log2(T) - math.log2(S[i - 1][j - 1])) for i, j, p in ent), _bound(logs, logs))
    return out


def run_features_exact(R, voxels):
    """one run matrix [Ng, max_run] and the group's taking-part voxels -> {feature: (value, bound)}, or None for an empty matrix"""
    R = np.asarray(R)
    ent = [(a + 1, l + 1, int(R[a, l])) for a in range(R.shape[0]) for l in range(R.shape[1]) if R[a, l]]
    Nr = sum(c for i, j, c in ent)
    if Nr == 0:
        return None
    ri, cj = {}, {}
    for i, j, c in ent:
        ri[i] = ri.get(i, 0) + c
        cj[j] = cj.get(j, 0) + c
    out = {}

    def put(name, terms):
        out[name] = (float(sum(terms)), _bound(terms))

    put("short_run_emphasis", [Fraction(c, j * j * Nr) for j, c in cj.items()])
    put("low_gray_level_run_emphasis", [Fraction(c, i * i * Nr) for i, c in ri.items()])
    put("long_run_emphasis", [Fraction(sum(c * j * j for j, c in cj.items()), Nr)])
    put("high_gray_level_run_emphasis", [Fraction(sum(c * i * i for i, c in ri.items()), Nr)])
    put("gray_level_non_uniformity", [Fraction(sum(c * c for c in ri.values()), Nr)])
    put("gray_level_non_uniformity_normalized", [Fraction(sum(c * c for c in ri.values()), Nr * Nr)])
    put("run_length_non_uniformity", [Fraction(sum(c * c for c in cj.values()), Nr)])
    put("run_length_non_uniformity_normalized", [Fraction(sum(c * c for c in cj.values()), Nr * Nr)])
    out["run_percentage"] = (float(Fraction(Nr, voxels)), _bound([Fraction(Nr, voxels)])) if voxels else (float("nan"), 0.0)
    mj, mi = Fraction(sum(c * j for j, c in cj.items()), Nr), Fraction(sum(c * i for i, c in ri.items()), Nr)
    put("run_variance", [sum(Fraction(c, Nr) * (j - mj) ** 2 for j, c in cj.items())])
    put("gray_level_variance", [sum(Fraction(c, Nr) * (i - mi) ** 2 for i, c in ri.items())])
    logs = [math.log2(Nr)] + [c * math.log2(c) / Nr for i, j, c in ent]
    out["run_entropy"] = (math.fsum(c / Nr * (math.log2(Nr) - math.log2(c)) for i, j, c in ent), _bound(logs, logs))
    return out


def mean_over_directions(per_direction, names):
    """[{feature: (value, bound)} or None per direction] -> {feature: (value, bound)}: the mean over the non-empty directions (NaN without one).  The mean of m values in
    float64 adds at most (m + 1) 2^-53 of their mean absolute value to the mean of their bounds."""
    have = [d for d in per_direction if d is not None]
    if not have:
        return {f: (float("nan"), 0.0) for f in names}
    m = len(have)
    return {f: (math.fsum(d[f][0] for d in have) / m, math.fsum(d[f][1] for d in have) / m + (m + 2) * U * math.fsum(abs(d[f][0]) + d[f][1] for d in have) / m) for f in names}

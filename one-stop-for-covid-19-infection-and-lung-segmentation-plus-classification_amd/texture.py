"""Second-order texture of the CT under a mask (csrc/kernels_texture.hip).

    quantize_volume(ct, mask= | labels=, n=)      -> the uint8 grey-level volume (0 = takes no part, 1..levels) and its histogram per group (unet_vol_texture_quantize)
    glcm(ct, ..., distance=, directions=, merge=) -> the grey-level co-occurrence counts int64 [n, K, Ng, Ng] per group and direction (unet_vol_texture_glcm)
    run_lengths(ct, ..., directions=, max_run=)   -> the grey-level run-length counts int64 [n, K, Ng, max_run] (unet_vol_texture_runs), repeated with a doubled max_run
                                                  while a run was clamped
    glcm_features(counts) / run_features(counts, voxels)     -> the conventional features of the matrices, float64 records per group and direction.  Pure numpy.
    texture_stats(ct, mask= | labels=, n=, region=)          -> TextureStats: one row per group with the mean of every feature over the directions
    lesion_texture(ct, labels, n)                 -> the same per lesion; its rows line up with component_table's

The device counts; the host turns the integer matrices (a few MB at most) into features.  The features are the conventional definitions of the radiomics literature (as
pyradiomics states them), on a configurable binning (lo, width, levels), and -- like the other tables of this package -- NOT clinically validated.  There is no CPU
fallback for the device steps.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from . import volume as V

MAX_LEVELS, MAX_DISTANCE, LDS_COUNTERS, MAX_RUN = _lib.TEXTURE_MAX_LEVELS, _lib.TEXTURE_MAX_DISTANCE, _lib.TEXTURE_LDS_COUNTERS, _lib.TEXTURE_MAX_RUN
# the 13 directions, bit k of unet_vol_texture_glcm's `directions`; the other 13 neighbours are their negations, which the symmetric matrix C + C^T covers
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))
DIRECTIONS_2D = (0, 1, 3, 4)                                         # the four in-plane directions
OUTSIDE = {"clip": 0, "drop": 1}
TABLE_BYTE_BUDGET = 2 ** 30                                          # the count tables of one launch (int64 [n, K, Ng, Ng] or [n, K, Ng, max_run]) may take this many bytes
GLCM_FEATURES = ("joint_energy", "contrast", "dissimilarity", "inverse_difference", "inverse_difference_moment", "joint_entropy", "correlation", "autocorrelation",
                 "cluster_shade", "cluster_prominence", "maximum_probability", "sum_of_squares")
RUN_FEATURES = ("short_run_emphasis", "long_run_emphasis", "gray_level_non_uniformity", "gray_level_non_uniformity_normalized", "run_length_non_uniformity",
                "run_length_non_uniformity_normalized", "run_percentage", "low_gray_level_run_emphasis", "high_gray_level_run_emphasis", "run_entropy", "run_variance",
                "gray_level_variance")
GLCM_FEATURE_DTYPE = np.dtype([(f, np.float64) for f in GLCM_FEATURES])
RUN_FEATURE_DTYPE = np.dtype([(f, np.float64) for f in RUN_FEATURES])
TEXTURE_DTYPE = np.dtype([("label", np.int32), ("voxels", np.int64), ("ml", np.float64)] + [("glcm_" + f, np.float64) for f in GLCM_FEATURES] +
                         [("glrlm_" + f, np.float64) for f in RUN_FEATURES])


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_directions(directions):
    """"3d" (all 13), "2d" (the four in-plane ones: bits 0, 1, 3, 4), or a list of indices 0..12 and / or offset triples (a triple or its negation names one direction)
    -> the ascending tuple of distinct indices, which is the order of the K matrices"""
    if isinstance(directions, str):
        if directions not in ("3d", "2d"):
            raise ValueError(f'directions is "3d", "2d" or a list of indices / offset triples, not {directions!r}')
        return tuple(range(13)) if directions == "3d" else DIRECTIONS_2D
    try:
        items = list(directions)
    except TypeError:
        raise ValueError(f'directions is "3d", "2d" or a list of indices / offset triples, not {directions!r}') from None
    out = set()
    for d in items:
        if _is_int(d):
            if not 0 <= int(d) < 13:
                raise ValueError(f"a direction index lies in 0 .. 12, not {d!r}")
            out.add(int(d))
            continue
        try:
            t = tuple(int(v) for v in d)
            ok = len(t) == 3 and all(_is_int(v) for v in d)
        except (TypeError, ValueError):
            ok = False
        neg = tuple(-v for v in t) if ok else None
        if not ok or (t not in DIRECTIONS and neg not in DIRECTIONS):
            raise ValueError(f"a direction is an index 0 .. 12 or one of the 13 offset triples (or its negation), not {d!r}")
        out.add(DIRECTIONS.index(t) if t in DIRECTIONS else DIRECTIONS.index(neg))
    if not out:
        raise ValueError("directions names at least one direction")
    return tuple(sorted(out))


def direction_bits(indices):
    return sum(1 << k for k in indices)


def check_binning(lo=-1000.0, width=25.0, levels=64, outside="clip"):
    """-> (lo, width, Ng, outside code), or ValueError: no device is needed"""
    if not _is_int(levels) or not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"levels is an integer in 1 .. {MAX_LEVELS}, not {levels!r}")
    for v, what in ((lo, "lo"), (width, "width")):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{what} is a finite number, not {v!r}")
    if not float(width) > 0.0:
        raise ValueError(f"width is greater than 0, not {width!r}")
    if outside not in OUTSIDE:
        raise ValueError(f'outside is "clip" or "drop", not {outside!r}')
    return float(lo), float(width), int(levels), OUTSIDE[outside]


def check_distance(distance):
    if not _is_int(distance) or not 1 <= int(distance) <= MAX_DISTANCE:
        raise ValueError(f"distance is an integer in 1 .. {MAX_DISTANCE}, not {distance!r}")
    return int(distance)


def check_max_run(max_run):
    if not _is_int(max_run) or not 1 <= int(max_run) <= MAX_RUN:
        raise ValueError(f"max_run is an integer in 1 .. {MAX_RUN}, not {max_run!r}")
    return int(max_run)


def check_table_budget(n, K, Ng, columns, what, budget=None):
    """refuses a count table int64 [n, K, Ng, columns] beyond the byte budget before anything is allocated"""
    budget = TABLE_BYTE_BUDGET if budget is None else int(budget)
    need = 8 * int(n) * int(K) * int(Ng) * int(columns)
    if need > budget:
        raise ValueError(f"{what}: the count table of n = {n} groups, K = {K} directions and Ng = {Ng} levels ({columns} columns) takes {need} bytes, more than the budget "
                         f"of {budget} (fewer levels, merge=True, fewer directions, or table_budget=)")
    return need


class _Groups:
    """the checked inputs of one call on the device: vol (NiftiVolume), dev (its raw bytes), labels / mask / region (flat device tensors or None), n, shape"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _check_groups(ct, mask, labels, n, region, shape):
    """intensity_stats' input rules -> (vol, n, vshape); every argument error is a ValueError before anything is uploaded"""
    torch = V._torch()
    if (mask is None) == (labels is None):
        raise ValueError("pass exactly one of mask, labels")
    if labels is not None and n is None:
        raise ValueError("labels need n, the number of groups (what label_volume returned)")
    n = 1 if labels is None else n
    if not _is_int(n) or not 0 <= int(n) < 2 ** 31:
        raise ValueError(f"n is the number of groups, not {n!r}")
    vol = V._source(ct)
    vshape = tuple(int(v) for v in vol.raw.shape)
    V._check_volume_dims(vshape)
    for a, what, dt in ((mask, "the mask", torch.uint8), (labels, "the label volume", torch.int32), (region, "the region", torch.uint8)):
        if a is not None:
            V._check_group_volume(a, what, vshape, shape, dt)
    return vol, int(n), vshape


def _upload_groups(vol, n, vshape, mask, labels, region):
    torch = V._torch()

    def flat(a):                                                    # (a volume without voxels still hands the entry points a buffer: null means "not given" there)
        a = torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F")).cuda() if not isinstance(a, torch.Tensor) else a.contiguous().reshape(-1)
        return a if a.numel() else torch.zeros(16, dtype=a.dtype, device="cuda")

    as_bytes = lambda a: flat(a if isinstance(a, torch.Tensor) else (np.asarray(a) != 0).astype(np.uint8))
    labels_dev = None
    if labels is not None:
        if isinstance(labels, torch.Tensor):
            labels_dev = flat(labels)
        else:
            a = np.asarray(labels)
            labels_dev = flat(np.where((a >= 1) & (a <= n), a, 0).astype(np.int32))          # a label outside 1..n takes no part: it must not wrap into the range
    return _Groups(vol=vol, dev=flat(V.upload(vol)), labels=labels_dev, mask=as_bytes(mask) if mask is not None else None,
                   region=as_bytes(region) if region is not None else None, n=n, shape=vshape)


# ---- the device wrappers ------------------------------------------------------------------------------------------------------------------------------------
def quantize_device(vol, dev, labels_dev, mask_dev, n, region_dev, lo, width, levels, outside):
    """unet_vol_texture_quantize on an uploaded volume (dev = upload(vol)) -> (the flat uint8 level tensor on the device, level_counts int64 [n, Ng] numpy);
    outside: 0 clip, 1 drop"""
    torch = V._torch(); lib, ctx = V._ctx()
    N = int(np.prod(vol.raw.shape))
    lv = torch.empty(max(N, 16), dtype=torch.uint8, device="cuda")
    lc = torch.empty((max(n, 1), levels), dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_texture_quantize(ctx.handle, dev.data_ptr(), *V._vox_args(vol), V._ptr(labels_dev), V._ptr(mask_dev), int(n), V._ptr(region_dev), float(lo), float(width),
                                            int(levels), int(outside), lv.data_ptr(), lc.data_ptr(), V._stream()), "vol_texture_quantize")
    return lv[:N], lc[:n].cpu().numpy()


def glcm_device(levels_dev, labels_dev, n, shape, levels, distance, bits, merge=False):
    """unet_vol_texture_glcm -> int64 [n, K, Ng, Ng] numpy, K = 1 with merge, else the number of set bits; labels_dev None: one group"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = shape
    K = 1 if merge else bin(int(bits)).count("1")
    out = torch.empty((max(n, 1), max(K, 1), levels, levels), dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_texture_glcm(ctx.handle, levels_dev.data_ptr(), V._ptr(labels_dev), int(n), X, Y, Z, int(levels), int(distance), int(bits), 1 if merge else 0,
                                        out.data_ptr(), V._stream()), "vol_texture_glcm")
    return out[:n].cpu().numpy()


def runs_device(levels_dev, labels_dev, n, shape, levels, bits, max_run):
    """unet_vol_texture_runs -> (int64 [n, K, Ng, max_run], clamped int64 [n, K]) numpy"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = shape
    K = bin(int(bits)).count("1")
    out = torch.empty((max(n, 1), max(K, 1), levels, max_run), dtype=torch.int64, device="cuda")
    cl = torch.empty((max(n, 1), max(K, 1)), dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_texture_runs(ctx.handle, levels_dev.data_ptr(), V._ptr(labels_dev), int(n), X, Y, Z, int(levels), int(bits), int(max_run), out.data_ptr(),
                                        cl.data_ptr(), V._stream()), "vol_texture_runs")
    return out[:n].cpu().numpy(), cl[:n].cpu().numpy()


def _quantized(ct, mask, labels, n, region, lo, width, levels, outside, shape):
    lo, width, Ng, code = check_binning(lo, width, levels, outside)
    vol, n, vshape = _check_groups(ct, mask, labels, n, region, shape)
    return vol, n, vshape, (lo, width, Ng, code)


def _run_quantize(vol, n, vshape, mask, labels, region, binning):
    g = _upload_groups(vol, n, vshape, mask, labels, region)
    g.levels, g.level_counts = quantize_device(vol, g.dev, g.labels, g.mask, n, g.region, *binning)
    return g


def _runs_with_retry(g, Ng, idx, max_run, budget):
    """the run counts with max_run doubled while a run was clamped, up to the longest axis (no run is longer) or the entry point's limit"""
    longest = min(max(max(g.shape), 1), MAX_RUN)
    bits = direction_bits(idx)
    while True:
        check_table_budget(g.n, len(idx), Ng, max_run, "run_lengths", budget)
        counts, clamped = runs_device(g.levels, g.labels, g.n, g.shape, Ng, bits, max_run)
        if not clamped.any() or max_run >= longest:
            return counts, clamped
        max_run = min(max_run * 2, longest)


# ---- the matrices ------------------------------------------------------------------------------------------------------------------------------------------------
def quantize_volume(ct, mask=None, labels=None, n=None, region=None, lo=-1000.0, width=25.0, levels=64, outside="clip", return_device=False, shape=None):
    """The CT under a mask as grey levels -> (the uint8 level volume [X, Y, Z] -- with return_device=True the flat device tensor in Fortran order --, level_counts int64
    [n, levels]).  ct, mask / labels / n, region, shape: as intensity_stats takes them.  The level of a non-NaN value v is floor((v - lo) / width) + 1 in float64;
    outside="clip" puts values below lo into level 1 and values from lo + levels width on into the last level, outside="drop" leaves them out.  0 = the voxel takes no
    part (outside every group or the region, NaN, or dropped).  The defaults are 25 HU bins from -1000 HU: conventional, configurable, not clinically validated."""
    vol, n, vshape, binning = _quantized(ct, mask, labels, n, region, lo, width, levels, outside, shape)
    g = _run_quantize(vol, n, vshape, mask, labels, region, binning)
    return (g.levels if return_device else V._host_of(g.levels, np.uint8, vshape)), g.level_counts


def glcm(ct, mask=None, labels=None, n=None, region=None, lo=-1000.0, width=25.0, levels=64, outside="clip", distance=1, directions="3d", merge=False, shape=None,
         table_budget=None):
    """The grey-level co-occurrence counts -> int64 [n, K, levels, levels]: C[g - 1, k, a - 1, b - 1] = the voxel pairs (p, p + distance dir_k) inside the volume with
    levels a and b that both lie in group g.  Not symmetrised (glcm_features forms C + C^T).  directions: "3d" (all 13 of DIRECTIONS), "2d" (the four in-plane ones --
    the right choice for thick-slice CT, where a step along z is several times a step in the plane), or a list of indices / offset triples; K matrices in ascending
    index order, or one with merge=True (their sum).  A request whose table would pass table_budget bytes (default TABLE_BYTE_BUDGET) is refused before anything is
    allocated."""
    idx, distance = check_directions(directions), check_distance(distance)
    vol, n, vshape, binning = _quantized(ct, mask, labels, n, region, lo, width, levels, outside, shape)
    check_table_budget(n, 1 if merge else len(idx), binning[2], binning[2], "glcm", table_budget)
    g = _run_quantize(vol, n, vshape, mask, labels, region, binning)
    return glcm_device(g.levels, g.labels, n, vshape, binning[2], distance, direction_bits(idx), merge)


def run_lengths(ct, mask=None, labels=None, n=None, region=None, lo=-1000.0, width=25.0, levels=64, outside="clip", directions="3d", max_run=64, shape=None,
                table_budget=None, return_clamped=False):
    """The grey-level run-length counts -> int64 [n, K, levels, R]: the maximal runs of one level inside one group along every direction (step 1), by level and length;
    column R - 1 would also hold longer runs, so the launch is repeated with max_run doubled while any run was clamped, up to the longest axis: R is the max_run that
    sufficed.  return_clamped=True: -> (counts, clamped int64 [n, K]), the clamped runs of the last launch (zero unless an axis passes 2^15).  directions: as for glcm."""
    idx, max_run = check_directions(directions), check_max_run(max_run)
    vol, n, vshape, binning = _quantized(ct, mask, labels, n, region, lo, width, levels, outside, shape)
    check_table_budget(n, len(idx), binning[2], max_run, "run_lengths", table_budget)
    g = _run_quantize(vol, n, vshape, mask, labels, region, binning)
    counts, clamped = _runs_with_retry(g, binning[2], idx, max_run, table_budget)
    return (counts, clamped) if return_clamped else counts


# ---- the features (host, float64) ---------------------------------------------------------------------------------------------------------------------------------
# Wherever a feature is a ratio of integers -- every one but the energy, the inverse differences, the short-run and low-grey-level emphases and the entropies -- its
# numerator and denominator are formed exactly (int64 histograms, Python integers where a product may pass 2^63) and divided once: Python's int / int is correctly
# rounded.  The others are float64 sums of terms that carry at most three roundings each.  tests/test_texture_host.py holds all of them to the exact rational values.
def _obj(a):
    return np.asarray(a).astype(object)


def _ratio(num, den):
    """elementwise Python-integer num / den as float64, NaN where den == 0"""
    num, den = np.asarray(num, object), np.asarray(den, object)
    out = np.full(num.shape, np.nan)
    for i in np.ndindex(num.shape):
        if den[i] != 0:
            out[i] = int(num[i]) / int(den[i])
    return out


def _entropy(c, total):
    """the terms of -sum p log2 p, p = c / total, as p (log2 total - log2 c): logarithms of integers (a p next to 1 loses nothing), 0 where c = 0, exactly 0 where c = total"""
    c = np.asarray(c, np.float64)
    return c / total * (np.log2(total) - np.log2(np.where(c > 0, c, total)))


def glcm_features(counts):
    """Co-occurrence counts int64 [..., Ng, Ng] (glcm's result, or one matrix) -> GLCM_FEATURE_DTYPE records of shape [...]: the features of P = (C + C^T) / sum, with
    grey values i, j = 1..Ng, px its marginal, mu = sum i px(i):
      joint_energy sum P^2 (the angular second moment); contrast sum (i - j)^2 P; dissimilarity sum |i - j| P; inverse_difference sum P / (1 + |i - j|);
      inverse_difference_moment sum P / (1 + (i - j)^2) (homogeneity); joint_entropy -sum P log2 P; correlation (sum i j P - mu^2) / var, defined as 1 where the
      marginal's variance is 0; autocorrelation sum i j P; cluster_shade sum (i + j - 2 mu)^3 P; cluster_prominence sum (i + j - 2 mu)^4 P; maximum_probability max P;
      sum_of_squares sum (i - mu)^2 P (the marginal's variance).
    An empty matrix gives NaN in every field.  Conventional definitions; not clinically validated."""
    C = np.asarray(counts)
    if C.ndim < 2 or C.shape[-1] != C.shape[-2] or C.dtype.kind not in "iu":
        raise ValueError("counts are integer matrices [..., Ng, Ng]")
    if C.size and C.min() < 0:
        raise ValueError("counts are not negative")
    C = C.astype(np.int64)
    Ng = C.shape[-1]
    S = C + np.swapaxes(C, -1, -2)
    lead = S.shape[:-2]
    out = np.zeros(lead, GLCM_FEATURE_DTYPE)
    for f in GLCM_FEATURES:
        out[f] = np.nan
    if Ng == 0 or S.size == 0:
        return out
    i = np.arange(1, Ng + 1, dtype=np.int64)
    T = S.sum(axis=(-1, -2))                                        # int64: at most 2 * 13 * 2^31
    ok = T > 0
    Tf = np.where(ok, T, 1).astype(np.float64)
    hd = np.stack([np.trace(S, offset=o, axis1=-2, axis2=-1) * (2 if o else 1) for o in range(Ng)], axis=-1)          # the difference histogram [..., Ng]: S is symmetric
    k = np.arange(Ng, dtype=np.int64)
    hs = np.zeros(lead + (2 * Ng + 1,), np.int64)                   # the sum histogram: hs[..., s] over i + j = s
    for a in range(Ng):
        hs[..., a + 2:a + 2 + Ng] += S[..., a, :]
    s = np.arange(2 * Ng + 1, dtype=np.int64)
    r = S.sum(axis=-1)                                              # the marginal's counts [..., Ng]
    M, A2, B = (r * i).sum(axis=-1), (r * i * i).sum(axis=-1), (S * (i[:, None] * i[None, :])).sum(axis=(-1, -2))          # < 2^49: exact in int64
    with np.errstate(invalid="ignore", divide="ignore"):
        P = S / Tf[..., None, None]
        out["joint_energy"] = np.where(ok, (P * P).sum(axis=(-1, -2)), np.nan)
        out["contrast"] = np.where(ok, (hd * k * k).sum(axis=-1) / Tf, np.nan)          # integer numerators below 2^53: one rounding
        out["dissimilarity"] = np.where(ok, (hd * k).sum(axis=-1) / Tf, np.nan)
        out["autocorrelation"] = np.where(ok, B / Tf, np.nan)
        out["inverse_difference"] = np.where(ok, (hd / (Tf[..., None] * (1 + k))).sum(axis=-1), np.nan)          # T (1 + d) < 2^53: one rounding per term
        out["inverse_difference_moment"] = np.where(ok, (hd / (Tf[..., None] * (1 + k * k))).sum(axis=-1), np.nan)
        out["joint_entropy"] = np.where(ok, _entropy(S, Tf[..., None, None]).sum(axis=(-1, -2)), np.nan)
        out["maximum_probability"] = np.where(ok, S.max(axis=(-1, -2)) / Tf, np.nan)
    To, Mo = _obj(T), _obj(M)
    var_num = To * _obj(A2) - Mo * Mo                               # T^2 var
    out["sum_of_squares"] = _ratio(var_num, To * To)
    corr = _ratio(To * _obj(B) - Mo * Mo, var_num)
    out["correlation"] = np.where(ok & (var_num == 0), 1.0, corr)
    m = [(_obj(hs) * _obj(s ** p)).sum(axis=-1) for p in range(5)]   # raw moments of i + j, Python integers
    c = 2 * Mo                                                      # sum (T s - 2 M)^p hs = T^p sum (s - 2 mu)^p hs
    out["cluster_shade"] = _ratio(To ** 3 * m[3] - 3 * To ** 2 * c * m[2] + 3 * To * c ** 2 * m[1] - c ** 3 * m[0], To ** 4)
    out["cluster_prominence"] = _ratio(To ** 4 * m[4] - 4 * To ** 3 * c * m[3] + 6 * To ** 2 * c ** 2 * m[2] - 4 * To * c ** 3 * m[1] + c ** 4 * m[0], To ** 5)
    return out


def run_features(counts, voxels):
    """Run-length counts int64 [..., Ng, R] (run_lengths' result, or one matrix) and the taking-part voxels of every matrix (broadcast against [...]; for run_lengths'
    result level_counts.sum(axis=1)[:, None]) -> RUN_FEATURE_DTYPE records of shape [...].  With Nr = sum R, grey values i = 1..Ng, lengths j = 1..R, p = R / Nr:
      short_run_emphasis sum p / j^2; long_run_emphasis sum p j^2; gray_level_non_uniformity sum_i (sum_j R)^2 / Nr, _normalized / Nr^2; run_length_non_uniformity
      sum_j (sum_i R)^2 / Nr, _normalized / Nr^2; run_percentage Nr / voxels; low_gray_level_run_emphasis sum p / i^2; high_gray_level_run_emphasis sum p i^2;
      run_entropy -sum p log2 p; run_variance sum p (j - mu_j)^2; gray_level_variance sum p (i - mu_i)^2.
    An empty matrix gives NaN in every field.  Conventional definitions; not clinically validated."""
    R = np.asarray(counts)
    if R.ndim < 2 or R.dtype.kind not in "iu":
        raise ValueError("counts are integer matrices [..., Ng, R]")
    if R.size and R.min() < 0:
        raise ValueError("counts are not negative")
    R = R.astype(np.int64)
    lead = R.shape[:-2]
    Np = np.broadcast_to(np.asarray(voxels, np.int64), lead)
    out = np.zeros(lead, RUN_FEATURE_DTYPE)
    for f in RUN_FEATURES:
        out[f] = np.nan
    if R.size == 0:
        return out
    i = np.arange(1, R.shape[-2] + 1, dtype=np.int64)
    j = np.arange(1, R.shape[-1] + 1, dtype=np.int64)
    ri, cj = R.sum(axis=-1), R.sum(axis=-2)                         # runs per level [..., Ng], per length [..., R]
    Nr = ri.sum(axis=-1)
    ok = Nr > 0
    Nf = np.where(ok, Nr, 1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["short_run_emphasis"] = np.where(ok, (cj / (j * j).astype(np.float64) / Nf[..., None]).sum(axis=-1), np.nan)
        out["low_gray_level_run_emphasis"] = np.where(ok, (ri / (i * i).astype(np.float64) / Nf[..., None]).sum(axis=-1), np.nan)
        out["run_entropy"] = np.where(ok, _entropy(R, Nf[..., None, None]).sum(axis=(-1, -2)), np.nan)
    No = _obj(Nr)
    J1, J2 = _obj((cj * j).sum(axis=-1)), _obj((cj * j * j).sum(axis=-1))          # sum j cj <= the voxels, sum j^2 cj <= 2^15 times that: exact in int64
    I1, I2 = _obj((ri * i).sum(axis=-1)), _obj((ri * i * i).sum(axis=-1))
    out["long_run_emphasis"] = _ratio(J2, No)
    out["high_gray_level_run_emphasis"] = _ratio(I2, No)
    g2, r2 = (_obj(ri) ** 2).sum(axis=-1), (_obj(cj) ** 2).sum(axis=-1)
    out["gray_level_non_uniformity"] = _ratio(g2, No)
    out["gray_level_non_uniformity_normalized"] = _ratio(g2, No * No)
    out["run_length_non_uniformity"] = _ratio(r2, No)
    out["run_length_non_uniformity_normalized"] = _ratio(r2, No * No)
    out["run_percentage"] = np.where(ok, _ratio(No, np.where(ok, _obj(Np), 0)), np.nan)
    out["run_variance"] = _ratio(No * J2 - J1 * J1, No * No)
    out["gray_level_variance"] = _ratio(No * I2 - I1 * I1, No * No)
    return out


def mean_over_directions(features):
    """records [n, K] -> records [n]: the mean of every field over the directions whose matrix is not empty (NaN where all are), as pyradiomics averages its angles"""
    f = np.asarray(features)
    out = np.zeros(f.shape[:-1], f.dtype)
    for name in f.dtype.names:
        v = f[name]
        have = ~np.isnan(v)
        cnt = have.sum(axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[name] = np.where(cnt > 0, np.where(have, v, 0.0).sum(axis=-1) / np.maximum(cnt, 1), np.nan)
    return out


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------------------
class TextureStats:
    """What texture_stats returns.  groups: TEXTURE_DTYPE records, one per label 1..n -- label, voxels (taking-part voxels), ml, glcm_<feature> for GLCM_FEATURES and
    glrlm_<feature> for RUN_FEATURES: the mean over the directions (the features of the one merged co-occurrence matrix with merge=True), NaN for a group whose matrices
    are empty.  glcm: the counts int64 [n, K, Ng, Ng]; runs: int64 [n, K', Ng, R]; glcm_by_direction / runs_by_direction: the feature records [n, K] / [n, K'];
    level_counts int64 [n, Ng]; directions: the indices into DIRECTIONS; lo, width, levels, outside, distance, merge, max_run (the R that sufficed), voxel_ml, n."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"TextureStats({self.n} groups, {self.levels} levels of {self.width} from {self.lo}, {len(self.directions)} directions, distance {self.distance})"


def texture_stats(ct, mask=None, labels=None, n=None, region=None, lo=-1000.0, width=25.0, levels=64, outside="clip", distance=1, directions="3d", merge=False,
                  max_run=64, shape=None, table_budget=None):
    """The texture of the CT where a mask is set -> TextureStats.  ct: a path, a NiftiVolume or an [X, Y, Z] array; exactly one of mask (non-zero = the one group) and
    labels (int, groups 1..n, n given; other labels take no part); region: only voxels where it is non-zero take part; mask / labels / region: numpy [X, Y, Z] arrays or
    flat device tensors in Fortran order with shape= -- all as intensity_stats takes them, so a lung side of split_lungs or the label volume of label_volume goes in as
    it is.  The CT is quantised once (quantize_volume's lo, width, levels, outside), its co-occurrence (distance, directions, merge) and run-length (directions, max_run)
    matrices are counted on the device, and the features are the host's (glcm_features, run_features), averaged over the directions.  Anisotropic grids are accepted as
    they are: a step along an axis is one voxel whatever its size, so for the 3-D directions resample_volume the CT (and resample_labels the groups) to an isotropic grid
    first, or use directions="2d" on thick slices.  Conventional definitions on a configurable binning; not clinically validated.  Every argument error is a ValueError
    raised before anything is uploaded or launched."""
    idx, distance, max_run = check_directions(directions), check_distance(distance), check_max_run(max_run)
    vol, n, vshape, binning = _quantized(ct, mask, labels, n, region, lo, width, levels, outside, shape)
    Ng = binning[2]
    check_table_budget(n, 1 if merge else len(idx), Ng, Ng, "texture_stats (glcm)", table_budget)
    check_table_budget(n, len(idx), Ng, max_run, "texture_stats (run_lengths)", table_budget)
    g = _run_quantize(vol, n, vshape, mask, labels, region, binning)
    C = glcm_device(g.levels, g.labels, n, vshape, Ng, distance, direction_bits(idx), merge)
    R, clamped = _runs_with_retry(g, Ng, idx, max_run, table_budget)
    voxels = g.level_counts.sum(axis=1)
    gf, rf = glcm_features(C), run_features(R, voxels[:, None])
    gm, rm = mean_over_directions(gf), mean_over_directions(rf)
    voxel_ml = float(np.prod(np.asarray(vol.pixdim, np.float64))) / 1000.0
    t = np.zeros(n, TEXTURE_DTYPE)
    t["label"], t["voxels"], t["ml"] = np.arange(1, n + 1), voxels, voxels * voxel_ml
    for f in GLCM_FEATURES:
        t["glcm_" + f] = gm[f]
    for f in RUN_FEATURES:
        t["glrlm_" + f] = rm[f]
    return TextureStats(groups=t, glcm=C, runs=R, clamped=clamped, glcm_by_direction=gf, runs_by_direction=rf, level_counts=g.level_counts, directions=idx, lo=binning[0],
                        width=binning[1], levels=Ng, outside=outside, distance=distance, merge=bool(merge), max_run=R.shape[-1], voxel_ml=voxel_ml, n=n, shape=vshape)


def lesion_texture(ct, labels, n, region=None, **kw):
    """texture_stats per lesion of a label volume (label_volume's labels and n; host array or device tensor with shape=): row i of .groups is lesion i + 1, as in
    component_table."""
    return texture_stats(ct, labels=labels, n=n, region=region, **kw)

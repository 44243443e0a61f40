"""numpy restatement of csrc/kernels_intensity.hip and volume.intensity_stats (include/unet_hip.h states the same operation by operation): decode, groups, bands,
min / max, the (group, value) order, the 256-chunk two-level sums and numpy's linear percentile.  Everything the device computes is compared with this for equality."""
import numpy as np

CHUNK = 256
HU_NAMES = ("below", "aerated", "ggo", "consolidation", "above")
HU_EDGES = (-950.0, -750.0, -300.0, 50.0)
DTYPES = {2: "u1", 256: "i1", 4: "i2", 512: "u2", 8: "i4", 768: "u4", 16: "f4", 64: "f8"}


def decode(raw, scaled=False, slope=1.0, inter=0.0):
    """get_fdata(): float64(raw), then (. * slope) + inter as two rounded operations"""
    a = np.asarray(raw).astype(np.float64)
    if scaled:
        a = a * np.float64(slope)
        a = a + np.float64(inter)
    return a


def group_of(shape, labels=None, mask=None, n=1, region=None):
    """int64 [X, Y, Z]: the group 1..n of every taking-part voxel, 0 elsewhere"""
    assert (labels is None) != (mask is None)
    g = np.asarray(labels).astype(np.int64) if labels is not None else (np.asarray(mask) != 0).astype(np.int64)
    assert g.shape == tuple(shape)
    g = np.where((g >= 1) & (g <= n), g, 0)
    if region is not None:
        g = np.where(np.asarray(region) != 0, g, 0)
    return g


def band_of(values, edges):
    """the number of edges <= v; a NaN goes to column B = len(edges) + 1"""
    v = np.asarray(values, np.float64)
    e = np.asarray(edges, np.float64)
    b = np.searchsorted(e, v, side="right")
    return np.where(np.isnan(v), e.size + 1, b)


def bands(val, g, n, edges):
    """-> band_counts int64 [n, B + 1], slice_counts int64 [Z, B + 1], minmax float64 [n, 2] ((+inf, -inf) for a group without a non-NaN value)"""
    W = len(edges) + 2
    b = band_of(val, edges)
    bc, sc, mm = np.zeros((n, W), np.int64), np.zeros((val.shape[2], W), np.int64), np.empty((n, 2), np.float64)
    mm[:, 0], mm[:, 1] = np.inf, -np.inf
    take = g > 0
    if take.any():
        np.add.at(bc, (g[take] - 1, b[take]), 1)
        z = np.broadcast_to(np.arange(val.shape[2])[None, None, :], val.shape)
        np.add.at(sc, (z[take], b[take]), 1)
        ok = take & ~np.isnan(val)
        np.minimum.at(mm[:, 0], g[ok] - 1, val[ok])
        np.maximum.at(mm[:, 1], g[ok] - 1, val[ok])
    return bc, sc, mm


def ordered(val, g, n):
    """the taking-part non-NaN values ordered by (group, value ascending) -> (values, groups, offsets int64 [n + 1])"""
    ok = (g > 0) & ~np.isnan(val)
    v, k = val[ok], g[ok]
    order = np.lexsort((v, k))
    sizes = np.bincount(k, minlength=n + 1)[1:n + 1]
    return v[order], k[order].astype(np.int32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def two_level_sum(run):
    """partials of 256 elements summed left to right from their first element, then the partials left to right: np.cumsum is that chain"""
    run = np.asarray(run, np.float64)
    if run.size == 0:
        return np.float64(0.0)
    partials = np.array([np.cumsum(run[c:c + CHUNK])[-1] for c in range(0, run.size, CHUNK)], np.float64)
    return np.cumsum(partials)[-1]


def moments_of_run(run):
    """(sum, ssd): ssd over q = fl(d d), d = fl(v - mean), mean = sum / m; an empty run: (0, 0)"""
    run = np.asarray(run, np.float64)
    if run.size == 0:
        return np.float64(0.0), np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        s = two_level_sum(run)
        d = run - s / np.float64(run.size)
        return s, two_level_sum(d * d)


def moments(values, offsets):
    """float64 [n, 2] for the runs values[offsets[g] : offsets[g + 1]]"""
    n = len(offsets) - 1
    out = np.zeros((n, 2), np.float64)
    for g in range(n):
        out[g] = moments_of_run(values[offsets[g]:offsets[g + 1]])
    return out


def percentile(run, q):
    """np.percentile(run, q) on an ascending run, from its two order statistics (numpy's linear rule and its _lerp); nan for an empty run"""
    m = len(run)
    if m == 0:
        return np.float64(np.nan)
    pos = (float(q) / 100.0) * (m - 1)
    lo = min(int(np.floor(pos)), m - 1)
    hi = min(lo + 1, m - 1)
    a, b, t = np.float64(run[lo]), np.float64(run[hi]), pos - lo
    with np.errstate(invalid="ignore"):
        return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t


def _run_fields(run, qs):
    m = len(run)
    if m == 0:
        return np.nan, np.nan, [np.nan] * len(qs)
    with np.errstate(invalid="ignore"):
        s, ssd = moments_of_run(run)
        return s / np.float64(m), np.sqrt(ssd / np.float64(m)), [percentile(run, q) for q in qs]


def stats(fdata, g, n, edges=HU_EDGES, qs=(5, 25, 50, 75, 95), pixdim=(1.0, 1.0, 1.0)):
    """what volume.intensity_stats returns, as a dict: the union's fields and `groups`, a dict of per-group arrays"""
    B = len(edges) + 1
    voxel_ml = float(np.prod(np.asarray(pixdim, np.float64))) / 1000.0
    bc, sc, mm = bands(fdata, g, n, edges)
    vals, _, off = ordered(fdata, g, n)
    sizes, nans = bc[:, :B].sum(axis=1), bc[:, B]
    total = int(sizes.sum())
    rows = [_run_fields(vals[off[k]:off[k + 1]], qs) for k in range(n)]
    with np.errstate(invalid="ignore", divide="ignore"):
        groups = dict(label=np.arange(1, n + 1), voxels=sizes + nans, nan_voxels=nans, ml=(sizes + nans) * voxel_ml,
                      min=np.where(sizes > 0, mm[:, 0], np.nan), max=np.where(sizes > 0, mm[:, 1], np.nan),
                      mean=np.array([r[0] for r in rows], np.float64), std=np.array([r[1] for r in rows], np.float64),
                      percentiles=np.array([r[2] for r in rows], np.float64).reshape(n, len(qs)), band_voxels=bc[:, :B], band_ml=bc[:, :B] * voxel_ml,
                      band_share=np.where(sizes[:, None] > 0, bc[:, :B] / sizes[:, None].astype(np.float64), np.nan),
                      dominant_band=np.where(sizes > 0, np.argmax(bc[:, :B], axis=1), -1))
    union = np.sort(vals, kind="stable")
    mean, std, pct = _run_fields(union, qs)
    band = bc[:, :B].sum(axis=0)
    return dict(voxels=total + int(nans.sum()), nan_voxels=int(nans.sum()), ml=(total + int(nans.sum())) * voxel_ml, min=float(mm[:, 0].min()) if total else np.nan,
                max=float(mm[:, 1].max()) if total else np.nan, mean=float(mean), std=float(std), percentiles={float(q): float(v) for q, v in zip(qs, pct)},
                band_voxels=band, band_ml=band * voxel_ml, band_share=band / float(total) if total else np.full(B, np.nan), slice_band_voxels=sc[:, :B],
                slice_nan_voxels=sc[:, B], groups=groups)

"""CPU restatement of the volume score (csrc/kernels_volscore.hip, covidseg_amd.volume.surface / distance_transform / score_volume) in numpy only -- no scipy
(tests/test_volscore_host.py pins it against scipy.ndimage where that imports).

The squared distance transform is DEFINED as a sequence of IEEE double operations (include/unet_hip.h):
    d2[v] = min over features f of fl( fl( fl(wx i^2) + fl(wy j^2) ) + fl(wz k^2) ),   (i, j, k) = v - f,   w = pixdim ** 2 in float64
and is computed here two ways: `edt_sq_brute` takes that minimum over all features, `edt_sq_lines` makes three passes (x, y, z) that each scan their whole line.
fl(a + c) is monotone in a, so the two agree bit for bit; numpy never fuses a multiply into an add."""
import math

import numpy as np

import components_oracle as CO


def weights(pixdim):
    p = np.asarray(pixdim, np.float64)
    return p * p


def _features(vol, nonzero):
    v = np.asarray(vol) != 0
    return v if nonzero else ~v


def edt_sq_at(points, feats, pixdim, chunk=1 << 22):
    """the definition at the voxels `points` [n, 3] over the feature coordinates `feats` [m, 3] (integer arrays) -> float64 [n]; +inf without features"""
    w = weights(pixdim)
    points = np.asarray(points, np.int64).reshape(-1, 3); feats = np.asarray(feats, np.int64).reshape(-1, 3)
    out = np.full(len(points), np.inf)
    if len(feats) == 0 or len(points) == 0:
        return out
    step = max(1, chunk // len(points))
    for s in range(0, len(feats), step):
        f = feats[s:s + step]
        d = (points[:, None, :] - f[None, :, :]).astype(np.float64)
        d *= d                                                        # exact integers
        t = w[0] * d[:, :, 0]
        t += w[1] * d[:, :, 1]
        t += w[2] * d[:, :, 2]
        np.minimum(out, t.min(axis=1), out=out)
    return out


def edt_sq_brute(vol, nonzero, pixdim):
    f = _features(vol, nonzero)
    pts = np.argwhere(np.ones(f.shape, bool))
    return edt_sq_at(pts, np.argwhere(f), pixdim).reshape(f.shape)


def _line_pass(g, axis, w):
    """out[l] = min over ALL l' of fl(g[l'] + fl(w (l - l')^2)) along `axis`"""
    L = g.shape[axis]
    g = np.ascontiguousarray(np.moveaxis(g, axis, 0))                # (a copy in line order: the long lines of the regime tests scan twice as fast)
    k = np.arange(L, dtype=np.float64)
    t = w * (k * k)
    out = np.full(g.shape, np.inf)
    idx = np.arange(L)
    shape = (L,) + (1,) * (g.ndim - 1)
    cand = np.empty(g.shape)
    for l2 in range(L):
        if np.isinf(g[l2]).all():
            continue                                                  # fl(inf + c) = inf lowers no minimum
        np.add(g[l2][None], t[np.abs(idx - l2)].reshape(shape), out=cand)
        np.minimum(out, cand, out=out)
    return np.moveaxis(out, 0, axis)


def edt_sq_lines(vol, nonzero, pixdim):
    f = _features(vol, nonzero)
    w = weights(pixdim)
    g = np.where(f, 0.0, np.inf)
    for axis in range(3):
        if g.shape[axis]:
            g = _line_pass(g, axis, w[axis])
    return g


def neighbour_offsets(connectivity):
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity is 1, 2 or 3")
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and (dx != 0) + (dy != 0) + (dz != 0) <= connectivity]


def surface(mask, connectivity=1):
    """mask != 0 and some neighbour within the structuring element is background (outside the volume: background) -> uint8"""
    m = np.asarray(mask) != 0
    X, Y, Z = m.shape
    p = np.zeros((X + 2, Y + 2, Z + 2), bool)
    p[1:-1, 1:-1, 1:-1] = m
    inner = m.copy()
    for dx, dy, dz in neighbour_offsets(connectivity):
        inner &= p[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
    return (m & ~inner).astype(np.uint8)


def confusion(pred, truth):
    """int64 [Z, 3]: tp, fp, fn per slice"""
    p, t = np.asarray(pred) != 0, np.asarray(truth) != 0
    return np.stack([(p & t).sum(axis=(0, 1)), (p & ~t).sum(axis=(0, 1)), (t & ~p).sum(axis=(0, 1))], axis=1).astype(np.int64)


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def overlap_metrics(counts, pixdim):
    counts = np.asarray(counts, np.int64)
    tp, fp, fn = (int(v) for v in counts.sum(axis=0)) if len(counts) else (0, 0, 0)
    vox = float(np.prod(np.asarray(pixdim, np.float64)))
    empty = tp + fp + fn == 0
    den = (2 * counts[:, 0] + counts[:, 1] + counts[:, 2]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_slice = np.where(den > 0, 2.0 * counts[:, 0] / den, np.nan)
    pred_ml, truth_ml = float(tp + fp) * vox / 1000.0, float(tp + fn) * vox / 1000.0
    return {"tp": tp, "fp": fp, "fn": fn, "dice": 1.0 if empty else 2.0 * tp / (2 * tp + fp + fn), "iou": 1.0 if empty else tp / (tp + fp + fn),
            "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn), "pred_ml": pred_ml, "truth_ml": truth_ml, "volume_error_ml": pred_ml - truth_ml,
            "per_slice_dice": per_slice, "tp_per_slice": counts[:, 0].copy(), "fp_per_slice": counts[:, 1].copy(), "fn_per_slice": counts[:, 2].copy()}


def surface_metrics(sa, sb, d2_a_to_b, d2_b_to_a, percentile=95.0):
    """sa, sb: surfaces of pred and truth; d2_a_to_b: squared distance of every voxel to the nearest voxel of sb (and the other way round).  Sums by math.fsum."""
    na, nb = int(np.count_nonzero(sa)), int(np.count_nonzero(sb))
    out = {"n_surface_pred": na, "n_surface_truth": nb}
    names = ("hd_pred_to_truth", "hd_truth_to_pred", "hd", "asd_pred_to_truth", "asd_truth_to_pred", "assd", "hd95")
    if na == 0 or nb == 0:
        out.update({k: 0.0 if na == nb else float("inf") for k in names})
        return out
    da, db = np.sqrt(d2_a_to_b[sa != 0]), np.sqrt(d2_b_to_a[sb != 0])
    out["hd_pred_to_truth"], out["hd_truth_to_pred"] = float(da.max()), float(db.max())
    out["hd"] = max(out["hd_pred_to_truth"], out["hd_truth_to_pred"])
    out["asd_pred_to_truth"], out["asd_truth_to_pred"] = math.fsum(da) / na, math.fsum(db) / nb
    out["assd"] = (out["asd_pred_to_truth"] + out["asd_truth_to_pred"]) / 2.0
    out["hd95"] = float(np.percentile(np.concatenate([da, db]), percentile))
    return out


def lesion_cover(pred, truth, connectivity=1, min_overlap_voxels=1):
    """-> dict: labels / n of both masks, covered voxels per truth lesion (by the prediction) and per predicted lesion (by the truth), detected / matched flags"""
    lt, nt = CO.label(truth, connectivity)
    lp, npred = CO.label(pred, connectivity)
    both = (lt != 0) & (lp != 0)
    cover_t = np.bincount(lt[both].astype(np.int64), minlength=nt + 1)[1:].astype(np.int64)
    cover_p = np.bincount(lp[both].astype(np.int64), minlength=npred + 1)[1:].astype(np.int64)
    det, mat = cover_t >= min_overlap_voxels, cover_p >= min_overlap_voxels
    return {"labels_t": lt, "n_t": nt, "labels_p": lp, "n_p": npred, "cover_t": cover_t, "cover_p": cover_p, "detected": det, "matched": mat,
            "lesion_recall": _ratio(int(det.sum()), nt), "lesion_precision": _ratio(int(mat.sum()), npred),
            "missed_lesions": int(nt - det.sum()), "false_positive_lesions": int(npred - mat.sum())}


def cover_tables(lt, nt, lp, np_):
    """unet_vol_lesion_overlap on ANY two int32 volumes: a voxel counts for its own label when that lies in 1..n and the partner is non-zero there (whatever its value)
    -> (cover_t int64 [nt], cover_p int64 [np_])"""
    lt, lp = np.asarray(lt).astype(np.int64), np.asarray(lp).astype(np.int64)
    ct = np.bincount(lt[(lp != 0) & (lt >= 1) & (lt <= nt)], minlength=nt + 1)[1:]
    cp = np.bincount(lp[(lt != 0) & (lp >= 1) & (lp <= np_)], minlength=np_ + 1)[1:]
    return ct.astype(np.int64), cp.astype(np.int64)


def _distinct_nonzero(rows):
    s = np.sort(rows, axis=1)
    return ((s[:, 1:] != s[:, :-1]) & (s[:, 1:] != 0)).sum(axis=1) + (s[:, 0] != 0)


def fallback_counts(own, other, n):
    """How often the coverage kernel's two fallbacks run for the table of `own` (labels 1..n count where `other` is non-zero), over the Fortran-order flat index:
    -> (groups of four consecutive indices, aligned to 4, that hold two or more distinct counted labels -- a voxel leaves cover_quad as its own atomic;
        runs of 256 consecutive indices, aligned to 256, that hold three or more distinct counted labels;
        the same runs counted by what wave_count sees, the FIRST counted label of each of the 64 groups of four: three or more distinct ones leave a lane to itself).
    The third implies the second."""
    o = np.asarray(own).reshape(-1, order="F").astype(np.int64); t = np.asarray(other).reshape(-1, order="F")
    v = np.where((t != 0) & (o >= 1) & (o <= n), o, 0)
    quads = np.concatenate([v, np.zeros(-v.size % 4, np.int64)]).reshape(-1, 4)
    runs = np.concatenate([v, np.zeros(-v.size % 256, np.int64)]).reshape(-1, 256)
    first = np.zeros(len(quads), np.int64)
    for i in (3, 2, 1, 0):
        first = np.where(quads[:, i] != 0, quads[:, i], first)
    waves = np.concatenate([first, np.zeros(-first.size % 64, np.int64)]).reshape(-1, 64)
    return int((_distinct_nonzero(quads) >= 2).sum()), int((_distinct_nonzero(runs) >= 3).sum()), int((_distinct_nonzero(waves) >= 3).sum())


def score(pred, truth, pixdim=(1, 1, 1), connectivity=1, lesion_connectivity=1, percentile=95.0, min_overlap_voxels=1):
    """everything score_volume returns, from the definitions above (d2 by the line scan)"""
    out = overlap_metrics(confusion(pred, truth), pixdim)
    sa, sb = surface(pred, connectivity), surface(truth, connectivity)
    out.update(surface_metrics(sa, sb, edt_sq_lines(sb, True, pixdim), edt_sq_lines(sa, True, pixdim), percentile))
    out.update(lesion_cover(pred, truth, lesion_connectivity, min_overlap_voxels))
    return out


def sum_chain(n_voxels):
    """the longest chain of additions behind unet_vol_surface_distances' sum for a volume of n_voxels, from the reduction shape include/unet_hip.h documents:
    per-lane chain 16 ceil(items / (256 G)), two 6-level butterflies, two times 3 additions across the waves, ceil(G / 256) partial sums per lane"""
    items = -(-n_voxels // 16)
    G = max(1, min(-(-items // 256), 32768 // 8))
    return 16 * -(-items // (256 * G)) + -(-G // 256) + 18

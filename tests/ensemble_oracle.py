"""CPU restatement of csrc/kernels_ensemble.hip and volume.segment_volume_ensemble in numpy (TEST INFRASTRUCTURE ONLY): the eight symmetries of a slice batch, the
members' weighted mean canvas with every float32 product, sum and the one division rounded on its own and in member order, the vote words and everything
unet_vol_vote_reduce derives from them, and the whole ensemble composed from volume_oracle's paste_back / unslice."""
import numpy as np

import volume_oracle as VO

F = np.float32
TTA = ("id", "rot90", "rot180", "rot270", "hflip", "vflip", "transpose", "antitranspose")
INVERSE = {"id": "id", "rot90": "rot270", "rot180": "rot180", "rot270": "rot90", "hflip": "hflip", "vflip": "vflip", "transpose": "transpose",
           "antitranspose": "antitranspose"}


def dihedral(a, code):
    """a [n, d, d] (or [n, d, d, 1]) under the symmetry `code` (a name of TTA or its index), by its numpy meaning on axes (1, 2); a contiguous copy"""
    name = code if isinstance(code, str) else TTA[code]
    a = np.asarray(a)
    if name == "id":
        out = a
    elif name in ("rot90", "rot180", "rot270"):
        out = np.rot90(a, {"rot90": 1, "rot180": 2, "rot270": 3}[name], (1, 2))
    elif name == "hflip":
        out = a[:, :, ::-1]
    elif name == "vflip":
        out = a[:, ::-1]
    elif name == "transpose":
        out = np.swapaxes(a, 1, 2)
    else:
        out = np.rot90(np.swapaxes(a, 1, 2), 2, (1, 2))
    return np.ascontiguousarray(out)


def weighted_mean(canvases, weights):
    """acc = w0 c0; acc = acc + wm cm for m = 1..; acc / wsum with wsum = ((w0 + w1) + ...): every operation one float32 operation, in member order"""
    w = [F(v) for v in weights]
    acc = (w[0] * np.asarray(canvases[0], F)).astype(F)
    wsum = F(F(0.0) + w[0])
    for c, wm in zip(canvases[1:], w[1:]):
        prod = (wm * np.asarray(c, F)).astype(F)
        acc = (acc + prod).astype(F)
        wsum = F(wsum + wm)
    return (acc / wsum).astype(F), wsum


def axpy(acc, canvas, w, first):
    prod = (F(w) * np.asarray(canvas, F)).astype(F)
    return prod if first else (np.asarray(acc, F) + prod).astype(F)


def pack(masks):
    """masks: list of arrays of one shape -> uint32 words, bit m = masks[m] != 0"""
    words = np.zeros(np.shape(masks[0]), np.uint32)
    for m, a in enumerate(masks):
        words |= (np.asarray(a) != 0).astype(np.uint32) << np.uint32(m)
    return words


def popcount(words):
    w = np.asarray(words, np.uint32)
    out = np.zeros(w.shape, np.uint8)
    for b in range(32):
        out += ((w >> np.uint32(b)) & np.uint32(1)).astype(np.uint8)
    return out


def min_votes(rule, M):
    return {"majority": M // 2 + 1, "any": 1, "all": M}[rule] if isinstance(rule, str) else int(rule)


def reduce(words, M, k):
    """words uint32 [X, Y, Z] -> dict(mask, votes, counts [Z], member_voxels [M], pair [M, M], hist [M + 1]) with mask = votes >= k"""
    words = np.asarray(words, np.uint32)
    votes = popcount(words)
    mask = (votes >= k).astype(np.uint8)
    bits = [((words >> np.uint32(m)) & np.uint32(1)).astype(bool) for m in range(M)]
    pair = np.zeros((M, M), np.int64)
    for a in range(M):
        for b in range(M):
            pair[a, b] = int(np.count_nonzero(bits[a] & bits[b]))
    hist = np.bincount(votes.reshape(-1), minlength=M + 1).astype(np.int64)
    return dict(mask=mask, votes=votes, counts=mask.sum(axis=(0, 1)).astype(np.int64), member_voxels=np.diag(pair).copy(), pair=pair, hist=hist)


def pairwise_dice(pair):
    v = np.diag(pair).astype(np.float64)
    den = v[:, None] + v[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, 2.0 * np.asarray(pair, np.float64) / den, np.nan)


def unslice_prob(canvas, shape, z0, z1):
    """float32 [X, Y, Z]: the probabilities volume_oracle.unslice thresholds (its sampler, its geometry), 0 outside [z0, z1)"""
    X, Y, Z = shape
    _, _, ps = VO.unslice(canvas, 0.0, shape, z0, z1)               # ps [n, Y, X]: image (i, j) -> vol[x = j, y = Y - 1 - i]
    prob = np.zeros((X, Y, Z), F)
    for k in range(z1 - z0):
        prob[:, :, z0 + k] = ps[k][::-1, :].T
    return prob


def ensemble(x, predicts, tta, weights, rects, S, shape, z0, z1, threshold, combine="mean"):
    """x [n, d, d, 1] float32 (the prepared batch); predicts: one function [n, d, d, 1] -> [n, d, d, 1] per model; members = (model, tta) in model-major order.
    -> dict(mask, counts [Z], votes, prob, pair, hist, member_voxels)"""
    X, Y, Z = shape
    canvases, masks, ws = [], [], []
    for mi, f in enumerate(predicts):
        for name in tta:
            p = np.asarray(f(dihedral(x, name)), F)
            p = dihedral(p, INVERSE[name])
            c = VO.paste_back(p[..., 0], rects, S)
            m, _, _ = VO.unslice(c, threshold, shape, z0, z1)
            canvases.append(c); masks.append(m); ws.append(F(weights[mi]))
    mean, _ = weighted_mean(canvases, ws)
    M = len(masks)
    k = min_votes("majority" if combine == "mean" else combine, M)
    r = reduce(pack(masks), M, k)
    if combine == "mean":
        mask, cnt, _ = VO.unslice(mean, threshold, shape, z0, z1)
        counts = np.zeros(Z, np.int64); counts[z0:z1] = cnt
    else:
        mask, counts = r["mask"], r["counts"]
    return dict(mask=mask, counts=counts, votes=r["votes"], prob=unslice_prob(mean, shape, z0, z1), pair=r["pair"], hist=r["hist"], member_voxels=r["member_voxels"])

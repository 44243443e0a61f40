"""numpy restatement of csrc/kernels_filter.hip and filters.py (TEST INFRASTRUCTURE ONLY): the element of a rank under a footprint, with the kernel's borders and its
order of float32 elements, and the Gaussian of filters.gaussian_filter.  tests/test_filter_host.py holds it to scipy.ndimage on the CPU; tests/test_gpu_filter.py holds
the device to it for equality.

    rank_filter(a, rank, fp, mode, cval)     a: [X, Y, Z] of a stored dtype; fp: bool [2 R + 1] * 3 (any odd extents); mode "reflect" / "nearest" / "constant"
The n shifted copies a[v + o], o in the footprint, are gathered through one index map per axis (index_map); float32 is compared as its 32-bit key (key32), integers
by value; ranks 0 and n - 1 are a running minimum / maximum, every other rank is np.partition's column `rank`."""
import numpy as np

import deform_oracle as DO

MODES = ("reflect", "nearest", "constant")


def key32(a):
    """float32 -> uint32, ascending in the filter's total order: bits ^ (sign ? 0xFFFFFFFF : 0x80000000)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey32(k):
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def index_map(n, R, mode):
    """for i = -R .. n - 1 + R: the index read there, -1 for the constant"""
    i = np.arange(-R, n + R)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode == "constant":
        return np.where((i >= 0) & (i < n), i, -1)
    assert mode == "reflect"
    p = np.mod(i, 2 * n)
    return np.where(p >= n, 2 * n - 1 - p, p)


def padded(a, R, mode, cval):
    """a with a halo of R on every side, the border applied"""
    out = a
    for ax in range(3):
        idx = index_map(a.shape[ax], R, mode)
        out = np.take(out, np.maximum(idx, 0), axis=ax)
    if mode == "constant":
        outside = np.zeros(out.shape, bool)
        for ax in range(3):
            sel = [slice(None)] * 3
            sel[ax] = index_map(a.shape[ax], R, mode) < 0
            outside[tuple(sel)] = True
        out = np.where(outside, np.asarray(cval, a.dtype), out)
    return out


def offsets(fp):
    """the footprint's offsets (dx, dy, dz) in ascending bit order (x fastest)"""
    fp = np.asarray(fp) != 0
    c = [e // 2 for e in fp.shape]
    return [(int(x) - c[0], int(y) - c[1], int(z) - c[2]) for z, y, x in np.argwhere(fp.transpose(2, 1, 0))]


def shifted(a, fp, mode, cval):
    """yields a[v + o] for every offset o of the footprint, each of a's shape"""
    R = max(1, max(np.asarray(fp).shape) // 2)
    P = padded(a, R, mode, cval)
    X, Y, Z = a.shape
    for dx, dy, dz in offsets(fp):
        yield P[R + dx:R + dx + X, R + dy:R + dy + Y, R + dz:R + dz + Z]


def rank_filter(a, rank, fp, mode="reflect", cval=0):
    a = np.asarray(a)
    assert a.ndim == 3 and a.dtype.str[1:] in ("u1", "i1", "i2", "u2", "i4", "u4", "f4") and mode in MODES
    n = int(np.count_nonzero(fp))
    assert 0 <= rank < n
    is_float = a.dtype.kind == "f"
    if is_float:
        k = key32(a).reshape(a.shape)
        ck = key32(np.array([cval], np.float32))[0]
    else:
        k, ck = a, cval
    if rank in (0, n - 1):
        pick = np.minimum if rank == 0 else np.maximum
        res = None
        for s in shifted(k, fp, mode, ck):
            res = s.copy() if res is None else pick(res, s)
    else:
        res = np.partition(np.stack(list(shifted(k, fp, mode, ck)), axis=-1), rank, axis=-1)[..., rank]
    res = unkey32(res).reshape(a.shape) if is_float else res
    return np.asfortranarray(res)


def bits(a):
    """the stored bits, for a comparison that tells -0 from +0 and one NaN from another"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.kind == "f" else a


def structure(connectivity, per_slice=False):
    d = np.abs(np.arange(-1, 2))
    fp = (d[:, None, None] + d[None, :, None] + d[None, None, :]) <= connectivity
    if per_slice:
        fp[:, :, 0] = fp[:, :, 2] = False
    return fp


def random_footprint(R, n, seed):
    """n of the (2 R + 1)^3 voxels"""
    side = 2 * R + 1
    fp = np.zeros(side ** 3, bool)
    fp[np.random.default_rng(seed).choice(side ** 3, n, replace=False)] = True
    return fp.reshape((side,) * 3)


def mirrored(fp):
    return np.asarray(fp)[::-1, ::-1, ::-1]


def percentile_rank(p, n):
    """scipy.ndimage.percentile_filter's rule (1.15)"""
    if p < 0:
        p += 100.0
    return n - 1 if p == 100 else int(float(n) * p / 100.0)


def grey_erosion(a, fp, mode="reflect", cval=0):
    return rank_filter(a, 0, fp, mode, cval)


def grey_dilation(a, fp, mode="reflect", cval=0):
    return rank_filter(a, int(np.count_nonzero(fp)) - 1, mirrored(fp), mode, cval)


def grey_opening(a, fp, mode="reflect", cval=0):
    return grey_dilation(grey_erosion(a, fp, mode, cval), fp, mode, cval)


def grey_closing(a, fp, mode="reflect", cval=0):
    return grey_erosion(grey_dilation(a, fp, mode, cval), fp, mode, cval)


# ---- the Gaussian ----------------------------------------------------------------------------------------------------------------------------------------------------
def gaussian_weights(sigma):
    """volume.gaussian_weights restated: 2 ceil(3 sigma) + 1 normalised float64 weights, None for sigma = 0"""
    if sigma == 0:
        return None
    R = int(np.ceil(3.0 * float(sigma)))
    t = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(t * t) / (2.0 * float(sigma) * float(sigma)))
    return w / w.sum()


def gaussian_filter(a32, sigmas):
    """a32: the volume decoded to float32; one pass of deform_oracle.smooth_axis along x, y, z, an axis with sigma = 0 skipped"""
    out = np.asarray(a32, np.float32)
    for axis, s in enumerate(sigmas):
        w = gaussian_weights(s)
        if w is not None:
            out = DO.smooth_axis(out, axis, w)
    return np.asfortranarray(out)

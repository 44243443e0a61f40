"""CPU restatement of csrc/kernels_resample.hip as whole-array numpy float64, operation by operation: the source coordinate
((M[r][0] i + M[r][1] j) + M[r][2] k) + M[r][3], np.floor, and the blend a + (b - a) * w along x, then y, then z -- no einsum, no dot, nothing that may fuse or reorder.
tests/test_resample_host.py pins it against scipy.ndimage.affine_transform; every device test against this file is an equality."""
import numpy as np

MODES = {"nearest": 0, "constant": 1}


def decode(raw, scaling=None):
    """get_fdata(): (float64(v) * slope) + inter when scaled"""
    a = np.asarray(raw).astype(np.float64)
    if scaling is not None:
        a = a * np.float64(scaling[0])
        a = a + np.float64(scaling[1])
    return a


def coords(M, out_shape):
    """s_r [X2, Y2, Z2] for r = 0, 1, 2"""
    M = np.asarray(M, np.float64).reshape(3, 4)
    i = np.arange(out_shape[0], dtype=np.float64)[:, None, None]
    j = np.arange(out_shape[1], dtype=np.float64)[None, :, None]
    k = np.arange(out_shape[2], dtype=np.float64)[None, None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        return [np.broadcast_to(((M[r, 0] * i + M[r, 1] * j) + M[r, 2] * k) + M[r, 3], tuple(out_shape)) for r in range(3)]


def nearest(src, M, out_shape, mode=0, cval=0):
    """elements moved untouched: q = floor(s + 0.5); mode 0: q clamped into the volume (a NaN coordinate: 0); mode 1: cval where any q is outside (or a NaN)"""
    src = np.asarray(src)
    out = np.full(tuple(out_shape), cval, src.dtype)
    if src.size == 0:
        assert mode == 1
        return out
    q, inside = [], np.ones(tuple(out_shape), bool)
    with np.errstate(invalid="ignore"):
        for s, n in zip(coords(M, out_shape), src.shape):
            v, top = np.floor(s + 0.5), float(n - 1)
            if mode == 0:
                q.append(np.where(~(v >= 0.0), 0.0, np.where(v > top, top, v)).astype(np.int64))
            else:
                ok = (v >= 0.0) & (v <= top)
                inside &= ok
                q.append(np.where(ok, v, 0.0).astype(np.int64))
    got = src[q[0], q[1], q[2]]
    return got if mode == 0 else np.where(inside, got, out)


def lerp(a, b, w):
    return a + (b - a) * w


def linear(fd, M, out_shape, mode=0, cval=0.0, dst=64):
    """fd: the decoded source, float64.  Mode 1: an axis whose two neighbours both lie outside (a coordinate below -1, at n or beyond, inf or NaN) takes the weight
    0 instead of s - floor(s): all eight neighbours are cval there, and the result is cval.  dst 64: the float64 result; 16: rounded once to float32; 2: uint8 (result >= 0.5)"""
    fd = np.asarray(fd, np.float64)
    cval = np.float64(cval)
    lo, hi, in_lo, in_hi, t = [], [], [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for s, n in zip(coords(M, out_shape), fd.shape):
            top = float(n - 1)
            if mode == 0:
                s = np.where(~(s >= 0.0), 0.0, np.where(s > top, top, s))
            f = np.floor(s)
            if mode == 0:
                t.append(s - f)
                a0 = f.astype(np.int64)
                lo.append(a0); hi.append(np.minimum(a0 + 1, n - 1))
                in_lo.append(np.ones(f.shape, bool)); in_hi.append(np.ones(f.shape, bool))
            else:
                ok0, ok1 = (f >= 0.0) & (f <= top), (f >= -1.0) & (f <= top - 1.0)
                fi = np.where((f >= -1.0) & (f <= top), f, 0.0).astype(np.int64)
                lo.append(np.where(ok0, fi, 0)); hi.append(np.where(ok1, fi + 1, 0))
                in_lo.append(ok0); in_hi.append(ok1)
                t.append(np.where(ok0 | ok1, s - f, 0.0))            # both neighbours outside: weight 0, so that an inf or NaN coordinate still reads cval
        p = {}
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    ok = (in_hi[0] if dx else in_lo[0]) & (in_hi[1] if dy else in_lo[1]) & (in_hi[2] if dz else in_lo[2])
                    if fd.size == 0:
                        p[dx, dy, dz] = np.full(tuple(out_shape), cval)
                        continue
                    v = fd[hi[0] if dx else lo[0], hi[1] if dy else lo[1], hi[2] if dz else lo[2]]
                    p[dx, dy, dz] = np.where(ok, v, cval)
        c00, c10 = lerp(p[0, 0, 0], p[1, 0, 0], t[0]), lerp(p[0, 1, 0], p[1, 1, 0], t[0])
        c01, c11 = lerp(p[0, 0, 1], p[1, 0, 1], t[0]), lerp(p[0, 1, 1], p[1, 1, 1], t[0])
        res = lerp(lerp(c00, c10, t[1]), lerp(c01, c11, t[1]), t[2])
        if dst == 64:
            return res
        if dst == 16:
            return res.astype(np.float32)
        return (res >= 0.5).astype(np.uint8)


def anisotropic_matrix():
    """a diagonal M with three different zooms and fractional offsets"""
    return np.array([[0.61, 0.0, 0.0, 0.13], [0.0, 0.83, 0.0, -0.21], [0.0, 0.0, 0.37, 0.4]])


def oblique_matrix(deg=10.0):
    """a rotation by `deg` about z times a shear times an anisotropic zoom, with a fractional offset"""
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    S = np.array([[1.0, 0.1, 0.0], [0.0, 1.0, 0.05], [0.0, 0.0, 1.0]])
    M = np.zeros((3, 4))
    M[:, :3] = R @ S @ np.diag([0.6, 0.8, 0.4])
    M[:, 3] = [0.37, -0.45, 0.21]
    return M


def oblique_affine(pixdim, deg=10.0, offset=(-12.5, 7.25, -30.0)):
    """a 4 x 4 voxel -> world affine: a rotation by `deg` about z of diag(pixdim), translated"""
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    A = np.eye(4)
    A[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.diag(np.asarray(pixdim, np.float64))
    A[:3, 3] = offset
    return A

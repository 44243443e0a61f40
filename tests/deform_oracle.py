"""CPU restatement of csrc/kernels_deform.hip as whole-array numpy float64, operation by operation, on top of resample_oracle: the Gaussian pass
acc + w v in ascending tap order, the displaced coordinate ((c + L0 u0) + L1 u1) + L2 u2, the demons force d g / (|g|^2 + d^2 / delta^2) with its one-sided differences
and its refusals, the warp (resample_oracle's own samplers, evaluated at the displaced coordinate) and the 3 x 3 determinant by its first row.  A field is float32
[3, X, Y, Z], rounded once where the kernels store it.  Every device test against this file is an equality of the stored bits.  OracleOps runs the loop of
volume.refine_registration over these functions: the host test and the device test run the same loop."""
import numpy as np

import resample_oracle as RS

DEN_MIN = 1e-9                                                      # kernels_deform.hip's DEN_MIN


def smooth_axis(a, axis, weights):
    """a: float32 [..., X, Y, Z]; one pass along axis (0 = x) of the last three: float32(sum_t w[t] a[clamp(p + t - R)]), from 0, t ascending"""
    a = np.asarray(a, np.float32)
    w = np.asarray(weights, np.float64)
    R, ax = (w.size - 1) // 2, a.ndim - 3 + axis
    n = a.shape[ax]
    a64 = a.astype(np.float64)
    acc = np.zeros(a.shape, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(-R, R + 1):
            acc = acc + w[t + R] * np.take(a64, np.clip(np.arange(n) + t, 0, n - 1), axis=ax)
        return acc.astype(np.float32)


def index_diff(a, axis):
    """the index-space difference of a float64 [X, Y, Z]: (a[p + 1] - a[p - 1]) * 0.5 inside, a[1] - a[0] and a[n - 1] - a[n - 2] at the borders, 0 on an axis of one"""
    a = np.asarray(a, np.float64)
    n = a.shape[axis]
    out = np.zeros(a.shape, np.float64)
    if n == 1:
        return out
    a = np.moveaxis(a, axis, 0)
    o = np.moveaxis(out, axis, 0)                                   # (a view)
    with np.errstate(invalid="ignore", over="ignore"):
        o[1:-1] = (a[2:] - a[:-2]) * 0.5
        o[0] = a[1] - a[0]
        o[-1] = a[-1] - a[-2]
    return out


def field_at(field, F, out_shape):
    """u_c on the output grid, float64: the stored elements (F None), or each component blended at F x clamped into the field (resample_oracle.linear, mode 0)"""
    field = np.asarray(field, np.float32)
    if F is None:
        assert tuple(field.shape[1:]) == tuple(out_shape)
        return [field[c].astype(np.float64) for c in range(3)]
    return [RS.linear(field[c].astype(np.float64), F, out_shape, 0, 0.0, 64) for c in range(3)]


def coords(W, L, u, out_shape):
    """s_r = ((c_r + L[r][0] u_0) + L[r][1] u_1) + L[r][2] u_2, c = resample_oracle.coords(W)"""
    L = np.asarray(L, np.float64).reshape(3, 3)
    c = RS.coords(W, out_shape)
    with np.errstate(invalid="ignore", over="ignore"):
        return [((c[r] + L[r, 0] * u[0]) + L[r, 1] * u[1]) + L[r, 2] * u[2] for r in range(3)]


def _at(fn, s, *args):
    """resample_oracle.linear / nearest evaluated at the coordinates s instead of those of a matrix: their own code, with RS.coords answering s"""
    keep = RS.coords
    RS.coords = lambda M, out_shape: s
    try:
        return fn(*args)
    finally:
        RS.coords = keep


def demons_force(f, m, W, L, Ginv, delta, field, mask=None):
    """-> (v: three float64 [X, Y, Z], where it is non-zero by rule: bool, the moving sample).  f, m: the decoded level volumes, float64"""
    f, m = np.asarray(f, np.float64), np.asarray(m, np.float64)
    G = np.asarray(Ginv, np.float64).reshape(3, 3)
    u = field_at(field, None, f.shape)
    s = coords(W, L, u, f.shape)
    ok = ~np.isnan(f)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for sr, n in zip(s, m.shape):
            ok &= (sr >= 0.0) & (sr <= float(n - 1))
        mw = _at(RS.linear, s, m, None, f.shape, 0, 0.0, 64)
        ok &= ~np.isnan(mw)
        d = f - mw
        gi = [index_diff(f, a) for a in range(3)]
        g = [(G[r, 0] * gi[0] + G[r, 1] * gi[1]) + G[r, 2] * gi[2] for r in range(3)]
        gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        den = gg + (d * d) / (np.float64(delta) * np.float64(delta))
        ok &= den > DEN_MIN
        v = [np.where(ok, (d * g[r]) / den, 0.0) for r in range(3)]
    return v, ok, mw


def demons_step(f, m, W, L, Ginv, delta, field, mask=None):
    """one iteration's u + v -> float32 [3, X, Y, Z]"""
    v, _, _ = demons_force(f, m, W, L, Ginv, delta, field, mask)
    u = field_at(field, None, np.asarray(f).shape)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(u[c] + v[c]).astype(np.float32) for c in range(3)])


def warp(src, scaling, W, L, field, F, out_shape, order, mode=0, cval=0, dst=64):
    """src: the stored volume [X, Y, Z].  order 1: resample_oracle.linear of the decoded source at the displaced coordinate (cval decoded; dst 64, 16 or 2); order 0:
    resample_oracle.nearest of the stored elements (cval stored)"""
    s = coords(W, L, field_at(field, F, out_shape), out_shape)
    if order == 1:
        return _at(RS.linear, s, RS.decode(src, scaling), None, out_shape, mode, cval, dst)
    return _at(RS.nearest, s, np.asarray(src), None, out_shape, mode, cval)


def jacobian(field, Ainv):
    """-> (float32 [X, Y, Z]: det(I + D Ainv) by the first row, how many float64 determinants are <= 0)"""
    field = np.asarray(field, np.float32)
    Ai = np.asarray(Ainv, np.float64).reshape(3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        J = [[None] * 3 for _ in range(3)]
        for c in range(3):
            D = [index_diff(field[c].astype(np.float64), a) for a in range(3)]
            for r in range(3):
                mcr = (D[0] * Ai[0, r] + D[1] * Ai[1, r]) + D[2] * Ai[2, r]
                J[c][r] = 1.0 + mcr if c == r else mcr
        m0 = J[1][1] * J[2][2] - J[1][2] * J[2][1]
        m1 = J[1][0] * J[2][2] - J[1][2] * J[2][0]
        m2 = J[1][0] * J[2][1] - J[1][1] * J[2][0]
        det = (J[0][0] * m0 - J[0][1] * m1) + J[0][2] * m2
        return det.astype(np.float32), int(np.count_nonzero(det <= 0.0))


def same_bits(got, want):
    """equality of the stored bits, NaN-aware: a NaN matches any NaN (the payload and sign of an invalid operation's NaN are the processor's), everything else bit for bit"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    both = np.isnan(got) & np.isnan(want)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.all(both | (np.ascontiguousarray(got).view(u) == np.ascontiguousarray(want).view(u))))


class OracleOps:
    """volume.DeformOps over numpy: volumes and fields are flat arrays in Fortran order, as the device holds them"""

    @staticmethod
    def _vol(flat, vargs):
        raw = np.asarray(flat).reshape(tuple(vargs[1:4]), order="F")
        return raw, ((vargs[5], vargs[6]) if vargs[4] else None)

    @staticmethod
    def _field(flat, shape):
        return np.stack([c.reshape(tuple(shape), order="F") for c in np.asarray(flat, np.float32).reshape(3, -1)])

    @staticmethod
    def _flat(a):
        return np.ascontiguousarray(np.asarray(a).reshape(-1, order="F"))

    def upload(self, src):
        return self._flat(src.vol.raw)

    def upload_mask(self, mask, shape):
        return None if mask is None else self._flat((np.asarray(mask) != 0).astype(np.uint8))

    def linear(self, flat, vargs, M, out_shape):
        raw, sc = self._vol(flat, vargs)
        return self._flat(RS.linear(RS.decode(raw, sc), M, out_shape, 0, 0.0, 16))

    def nearest_mask(self, flat, shape, M, out_shape):
        return self._flat(RS.nearest(flat.reshape(tuple(shape), order="F"), M, out_shape, 0, 0))

    def zeros(self, n):
        return np.zeros(int(n), np.float32)

    def stack(self, parts):
        return np.concatenate(list(parts))

    def smooth_axis(self, x, C, shape, axis, weights):
        a = np.stack([c.reshape(tuple(shape), order="F") for c in np.asarray(x, np.float32).reshape(C, -1)])
        return np.concatenate([self._flat(c) for c in smooth_axis(a, axis, weights)])

    def demons_step(self, f, fvargs, mask, m, mvargs, W, L, Ginv, delta, field):
        (fr, fs), (mr, ms) = self._vol(f, fvargs), self._vol(m, mvargs)
        mk = None if mask is None else mask.reshape(fr.shape, order="F")
        out = demons_step(RS.decode(fr, fs), RS.decode(mr, ms), W, L, Ginv, delta, self._field(field, fr.shape), mk)
        return np.concatenate([self._flat(c) for c in out])

    def warp_field(self, src, vargs, W, L, field, field_shape, F, order, mode, cval, cval_bits, out_shape, dst_dtype):
        raw, sc = self._vol(src, vargs)
        assert order == 1
        return self._flat(warp(raw, sc, W, L, self._field(field, field_shape), F, out_shape, 1, mode, cval, dst_dtype))

    def jacobian(self, field, shape, Ainv):
        det, folded = jacobian(self._field(field, shape), Ainv)
        return self._flat(det), folded

    def rms(self, f, warped, mask):
        d = np.asarray(f, np.float32).astype(np.float64) - warped
        ok = ~np.isnan(d) if mask is None else (~np.isnan(d) & (mask != 0))
        n = int(ok.sum())
        return (float(np.sqrt((d[ok] * d[ok]).sum()) / np.sqrt(n)) if n else float("nan")), n

    def minmax(self, det):
        return float(det.min()), float(det.max())

    def sync(self):
        pass


# ---- the phantom case of the end-to-end tests: register_oracle's chest, the follow-up breathed in by a smooth bump and moved rigidly ----------------------------------------
def bump(p, centre=(-17.0, 5.0, 4.0), amplitude=(0.0, 1.5, 4.0), width=14.0):
    """a smooth true displacement in mm at world points p [..., 3]: a Gaussian bump of `amplitude` around `centre` (the left lesion of register_oracle.phantom)"""
    p = np.asarray(p, np.float64)
    r2 = ((p - np.asarray(centre)) ** 2).sum(axis=-1)
    return np.exp(-r2 / (2.0 * width * width))[..., None] * np.asarray(amplitude)


def world_points(shape, affine):
    idx = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"), axis=-1)
    A = np.asarray(affine, np.float64)
    return idx @ A[:3, :3].T + A[:3, 3]


class PhantomCase:
    """fixed, moving: int16 [X, Y, Z]; fixed_affine, moving_affine; rigid: the true 4 x 4, fixed world -> moving world; u_true: float64 [X, Y, Z, 3] on the fixed grid"""


def _centred(shape, pix, centre=(0.0, 0.0, 0.0)):
    A = np.diag([pix[0], pix[1], pix[2], 1.0])
    A[:3, 3] = np.asarray(centre) - A[:3, :3] @ ((np.asarray(shape) - 1) / 2.0)
    return A


def phantom_case():
    """An 80 x 72 x 72 mm field of view at 2 mm.  The follow-up (moving) is register_oracle.phantom's anatomy moved by a known, non-identity rigid T; the baseline (fixed)
    is the same anatomy displaced by bump(): f(p) = anatomy(p + u_true(p)), blended from a noise-free 1 mm rendering, plus its own noise.  So m(T (p + u_true(p))) = f(p):
    u_true is the field refine_registration looks for when it is handed T."""
    import register_oracle as RO
    case = PhantomCase()
    fshape, mshape, fine_shape = (40, 36, 36), (42, 38, 30), (88, 80, 80)
    case.fixed_affine, case.moving_affine = _centred(fshape, (2.0, 2.0, 2.0)), _centred(mshape, (2.0, 2.0, 2.5), (1.0, -1.0, 0.5))
    rx, ry, rz = np.deg2rad([2.0, -1.5, 3.0])
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, (2.3, -1.7, 1.9)
    case.rigid = T
    case.moving = np.asfortranarray(np.rint(RO.phantom(mshape, np.linalg.inv(T) @ case.moving_affine, 2)).astype(np.int16))
    A_fine = _centred(fine_shape, (1.0, 1.0, 1.0))
    fine = RO.phantom(fine_shape, A_fine, 0, sigma=0.0)
    field = np.moveaxis(bump(world_points(fshape, case.fixed_affine)), -1, 0).astype(np.float32)
    inv_fine = np.linalg.inv(A_fine)
    f = warp(fine, None, (inv_fine @ case.fixed_affine)[:3], inv_fine[:3, :3], field, None, fshape, 1, 0, 0.0, 64)
    case.fixed = np.asfortranarray(np.rint(f + np.random.default_rng(1).normal(0.0, 15.0, fshape)).astype(np.int16))
    case.u_true = np.moveaxis(field.astype(np.float64), 0, -1)
    return case


def lesion_masks(case, centre=(-17.0, 5.0, 4.0), radii=(4.0, 5.0, 6.0)):
    """the phantom's displaced lesion drawn on both scans -> (mask_a on the fixed grid, mask_b on the moving grid), uint8: anatomy point a lies in the lesion iff
    |(a - centre) / radii| < 1; the fixed voxel p shows anatomy point p + u_true(p), the moving world point q shows inv(T) q"""
    def inside(a):
        return ((((a - np.asarray(centre)) / np.asarray(radii)) ** 2).sum(axis=-1) < 1.0).astype(np.uint8)
    pa = world_points(case.fixed.shape, case.fixed_affine) + case.u_true
    pb = world_points(case.moving.shape, np.linalg.inv(case.rigid) @ case.moving_affine)
    return np.asfortranarray(inside(pa)), np.asfortranarray(inside(pb))

"""CPU restatement of csrc/kernels_register.hip as whole-array numpy float64, operation by operation, on top of resample_oracle: which fixed
voxels are counted, the moving sample (resample_oracle.linear in mode 0: inside the volume its clamp is the identity), the bin floor((v - lo) * scale) with the
subtraction and the product rounded on their own, and the integer counts.  Every device test against this file is an equality."""
import numpy as np

import resample_oracle as RS


def scale_of(bins, window):
    """B / (hi - lo), once, in float64"""
    return np.float64(bins) / (np.float64(window[1]) - np.float64(window[0]))


def bin_of(v, bins, window):
    """floor((v - lo) * scale), compared as a double first: below 0 (or a NaN) -> 0, >= B -> B - 1; +-inf clamp"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = (np.asarray(v, np.float64) - np.float64(window[0])) * scale_of(bins, window)
        b = np.where(~(q >= 0.0), 0.0, np.where(q >= float(bins), float(bins - 1), np.floor(q)))
    return b.astype(np.int64)


def counted(fixed_fd, moving_fd, M, mask=None):
    """-> (which fixed voxels are counted under M, bool [X, Y, Z]; the moving sample there, float64)"""
    fixed_fd, moving_fd = np.asarray(fixed_fd, np.float64), np.asarray(moving_fd, np.float64)
    ok = ~np.isnan(fixed_fd)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        for s, n in zip(RS.coords(M, fixed_fd.shape), moving_fd.shape):
            ok &= (s >= 0.0) & (s <= float(n - 1))                   # (a NaN or inf coordinate fails one of the two)
    sample = RS.linear(moving_fd, M, fixed_fd.shape, 0, 0.0, 64)
    ok &= ~np.isnan(sample)
    return ok, sample


def joint_hist(fixed_fd, moving_fd, Ms, bins, f_window, m_window=None, mask=None):
    """fixed_fd, moving_fd: the decoded volumes [X, Y, Z]; Ms: [K, 3, 4] (or [K, 12]) -> uint32 [K, B, B], fixed bin major"""
    Ms = np.asarray(Ms, np.float64).reshape(-1, 3, 4)
    m_window = f_window if m_window is None else m_window
    bf = bin_of(fixed_fd, bins, f_window)
    out = np.zeros((len(Ms), bins, bins), np.uint32)
    for c, M in enumerate(Ms):
        ok, sample = counted(fixed_fd, moving_fd, M, mask)
        cell = bf * bins + bin_of(sample, bins, m_window)
        out[c] = np.bincount(cell[ok], minlength=bins * bins).reshape(bins, bins).astype(np.uint32)
    return out


def phantom(shape, affine, noise_seed, sigma=15.0):
    """An analytic chest in WORLD millimetres, sampled at the voxel centres of (shape, affine) -> float64 [X, Y, Z] in HU: a soft-edged body ellipsoid in air, two lung
    ellipsoids, a lesion in each and a spine, plus Gaussian noise.  The anatomy sits around the origin of the frame `affine` maps into: pass inv(T) @ A for the scan of a
    patient moved by T."""
    idx = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    A = np.asarray(affine, np.float64)
    w = [A[r, 0] * idx[0] + A[r, 1] * idx[1] + A[r, 2] * idx[2] + A[r, 3] for r in range(3)]

    def ell(c, r):
        return np.sqrt(((w[0] - c[0]) / r[0]) ** 2 + ((w[1] - c[1]) / r[1]) ** 2 + ((w[2] - c[2]) / r[2]) ** 2)

    body = np.clip((1.0 - ell((0, 0, 0), (34, 27, 30))) * 6.0, 0.0, 1.0)          # a soft edge about a sixth of the radius wide
    v = -1000.0 + body * 1040.0
    for c, r in (((-15, 0, 0), (10, 16, 20)), ((15, 2, -2), (11, 15, 19))):
        lung = np.clip((1.0 - ell(c, r)) * 5.0, 0.0, 1.0)
        v = v - lung * 880.0
    for c, r in (((-17, 5, 4), (4, 5, 6)), ((13, -6, -7), (5, 4, 5))):
        v = v + np.clip((1.0 - ell(c, r)) * 4.0, 0.0, 1.0) * 600.0
    v = v + np.clip((1.0 - ell((0, 18, 0), (5, 5, 40))) * 4.0, 0.0, 1.0) * 500.0
    return v + np.random.default_rng(noise_seed).normal(0.0, sigma, shape)


def corner_error(T_found, T_true, shape, affine):
    """the largest distance, in mm, between where two 4 x 4 world transforms put the eight corners of the field of view of (shape, affine)"""
    n = np.asarray(shape, np.float64) - 1.0
    worst = 0.0
    for c in range(8):
        p = np.asarray(affine, np.float64) @ np.array([n[0] * (c & 1), n[1] * ((c >> 1) & 1), n[2] * ((c >> 2) & 1), 1.0])
        worst = max(worst, float(np.linalg.norm((np.asarray(T_found) @ p - np.asarray(T_true) @ p)[:3])))
    return worst

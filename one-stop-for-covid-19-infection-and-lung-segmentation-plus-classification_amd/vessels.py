"""Vesselness of a CT on the device: Hessian eigenvalues, Frangi's tube measure, a vessel mask inside the lungs (csrc/kernels_vessel.hip).

    hessian_eigenvalues(ct, sigma_mm, region=)                  -> float32 [3, X, Y, Z]: the eigenvalues of the scale-normalised Hessian of the CT smoothed at sigma_mm,
                                                                   |l1| <= |l2| <= |l3| (unet_vol_hessian_eig); plates and blobs can be told from them as well
    vesselness(ct, sigmas_mm=, alpha=, beta=, c=, bright=)      -> Vesselness: Frangi's measure, the maximum over the scales and the scale that gave it (unet_vol_vesselness)
    vessel_mask(ct, lungs, threshold=, dense_hu=, ...)          -> VesselMask: the dense tubes inside the eroded lungs, without what a ball of max_radius_mm fits into
    hessian_factors / denominators                              -> the host doubles the entries take
    hessian_eig_device / vesselness_device                      -> the entries on device buffers

Sources are what filters.gaussian_filter takes: a path, a NiftiVolume, an [X, Y, Z] array with pixdim=, or a flat device tensor with src_shape= and pixdim=.  The voxel
size is needed: the scales are millimetres and the Hessian is scale-normalised (gamma = 1) with sigma^2 / h^2.  The smoothing is filters.gaussian_filter(sigma_mm=)
unchanged, so a scale whose radius ceil(3 sigma / h) exceeds the smoother's 32 taps on some axis is refused.  Every device result equals tests/vessel_oracle.py bit for
bit: the arithmetic is float64 with one rounding per operation, the eigenvalues come from cyclic Jacobi and exp(-u) is the library's own.  Every argument error is a
ValueError raised before any device work; there is no CPU fallback.  alpha = beta = 0.5, c = 100 HU, threshold, dense_hu, max_radius_mm, min_ml and erode_mm are
conventional starting values, configurable and NOT clinically validated here.  Vessel trees and hilum connectivity, artery / vein separation, lobes and fissures, plate and
blob measures, float32 or closed-form eigen-solvers, scales beyond the smoother's radius and sharding across ranks are out of scope (section 4af).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from . import filters as F
from . import lungs as L
from . import volume as V

MAX_SCALES = _lib.VESSEL_MAX_SCALES
SIGMAS_MM, ALPHA, BETA, C_HU = (1.0, 2.0, 3.0), 0.5, 0.5, 100.0      # conventional, configurable, not validated here
_VESSELNESS_KEYS = ("sigmas_mm", "alpha", "beta", "c", "bright")
_VESSEL_MASK_KEYS = {"threshold", "dense_hu", "max_radius_mm", "min_ml", "connectivity", "erode_mm"} | set(_VESSELNESS_KEYS)


class Vesselness:
    """vesselness' result.  response: float32 [X, Y, Z], the maximum of the measure over the scales (return_device=True: the flat device tensor); scale: uint8, 0 where
    response == 0, else 1 + the index of the first scale that reached the maximum; sigmas_mm; shape; pixdim."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"Vesselness(shape={self.shape}, sigmas_mm={self.sigmas_mm})"


class VesselMask:
    """vessel_mask's result.  mask: uint8 [X, Y, Z] (return_device=True: the flat device tensor); ml; n_components; vesselness: the Vesselness under the eroded lungs."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"VesselMask(ml={self.ml:.2f}, n_components={self.n_components})"


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_positive(v, what):
    if not L._is_number(v) or not (np.isfinite(float(v)) and float(v) > 0.0 and np.isfinite(float(v) * float(v))):
        raise ValueError(f"{what} is a finite positive number (with a finite square), not {v!r}")
    return float(v)


def _check_sigma(sigma_mm, pixdim):
    """one scale against the voxel size: positive, and within the smoother's radius on every axis"""
    s = _check_positive(sigma_mm, "sigma_mm")
    for h in pixdim:
        R = int(np.ceil(3.0 * (s / float(h))))
        if R > V.SMOOTH_MAX_RADIUS:
            raise ValueError(f"sigma_mm = {s} needs {R} taps either side on an axis of {float(h)} mm voxels; a Gaussian pass takes {V.SMOOTH_MAX_RADIUS}")
    return s


def _check_sigmas(sigmas_mm, pixdim):
    try:
        ss = tuple(sigmas_mm)
    except TypeError:
        ss = ()
    if not 1 <= len(ss) <= MAX_SCALES:
        raise ValueError(f"sigmas_mm holds 1..{MAX_SCALES} scales in millimetres, not {sigmas_mm!r}")
    ss = tuple(_check_sigma(s, pixdim) for s in ss)
    if any(b <= a for a, b in zip(ss, ss[1:])):
        raise ValueError(f"sigmas_mm is strictly ascending, not {sigmas_mm!r}")
    return ss


def _check_vesselness_args(sigmas_mm=SIGMAS_MM, alpha=ALPHA, beta=BETA, c=C_HU, bright=True, pixdim=(1.0, 1.0, 1.0)):
    """-> (sigmas, the three denominators, bright); pixdim: the one the scales are checked against"""
    ss = _check_sigmas(sigmas_mm, pixdim)
    dens = denominators(_check_positive(alpha, "alpha"), _check_positive(beta, "beta"), _check_positive(c, "c"))
    if not all(np.isfinite(d) and d > 0.0 for d in dens):
        raise ValueError(f"2 alpha^2, 2 beta^2 and 2 c^2 must be finite and positive, not {dens!r}")
    return ss, dens, L._check_bool(bright, "bright")


def _check_vessel_mask_args(threshold=0.3, dense_hu=-500.0, max_radius_mm=3.0, min_ml=0.01, connectivity=3, erode_mm=2.0, pixdim=None, **vkw):
    """every check of vessel_mask that needs no volume -> the checked values as a dict"""
    bad = set(vkw) - set(_VESSELNESS_KEYS)
    if bad:
        raise ValueError(f"vessel_mask takes {sorted(_VESSEL_MASK_KEYS)}, not {sorted(bad)}")
    if not L._is_number(threshold) or not 0.0 < float(threshold) <= 1.0:
        raise ValueError(f"threshold is a response in (0, 1], not {threshold!r}")
    if not L._is_number(min_ml) or not (np.isfinite(float(min_ml)) and float(min_ml) >= 0.0):
        raise ValueError(f"min_ml is a finite number >= 0, not {min_ml!r}")
    p = None if pixdim is None else V._check_pixdim(pixdim)
    _check_vesselness_args(pixdim=(1.0, 1.0, 1.0) if p is None else p, **vkw)
    return dict(threshold=float(threshold), dense_hu=L._check_hu(dense_hu, "dense_hu"), max_radius=V._check_radius(max_radius_mm), min_ml=float(min_ml),
                connectivity=V._check_connectivity(connectivity), erode=V._check_radius(erode_mm), pixdim=p, vkw=vkw)


def hessian_factors(sigma_mm, pixdim):
    """the six host doubles of a scale: kxx, kyy, kzz = sigma^2 / h^2 and kxy, kxz, kyz = sigma^2 / ((4 h_a) h_b), each operation rounded once in float64"""
    s = np.float64(sigma_mm)
    hx, hy, hz = (np.float64(v) for v in pixdim)
    s2 = s * s
    return np.array([s2 / (hx * hx), s2 / (hy * hy), s2 / (hz * hz), s2 / ((4.0 * hx) * hy), s2 / ((4.0 * hx) * hz), s2 / ((4.0 * hy) * hz)], np.float64)


def denominators(alpha=ALPHA, beta=BETA, c=C_HU):
    """2 alpha^2, 2 beta^2, 2 c^2 as 2 (v v) in float64"""
    return tuple(float(2.0 * (np.float64(v) * np.float64(v))) for v in (alpha, beta, c))


def _source(ct, src_shape, pixdim):
    """-> (the filter source, its voxel size); an array or a device tensor carries none: pixdim= is needed"""
    src = F._filter_source(ct, src_shape, pixdim)
    p = pixdim if pixdim is not None else (src.vol.pixdim if src.header is not None else None)
    if p is None:
        raise ValueError("the scales are millimetres and need the voxel size: pass pixdim= (an array or a device tensor carries none)")
    return src, V._check_pixdim(p)


def _region_arg(region, shape):
    if region is not None:
        L._mask_arg(region, shape, shape, "region")


def _decoded_device(src):
    """the volume as the float32 device tensor filters.gaussian_filter smooths: get_fdata rounded once (a device tensor: tensor.to(float32))"""
    torch = V._torch()
    if src.tensor is not None:
        return src.tensor.to(torch.float32)
    return torch.from_numpy(np.asfortranarray(src.vol.get_fdata().astype(np.float32)).reshape(-1, order="F")).cuda()


def _smoothed(x32, shape, pixdim, sigma_mm):
    return F.gaussian_filter(x32, sigma_mm=sigma_mm, pixdim=pixdim, return_device=True, src_shape=shape)


# ---- the entries ------------------------------------------------------------------------------------------------------------------------------------------------------
def hessian_eig_device(smooth_dev, shape, k, region_dev=None):
    """unet_vol_hessian_eig on a smoothed float32 device volume; k: hessian_factors -> a float32 device tensor of 3 X Y Z elements, l1 | l2 | l3"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    k = np.ascontiguousarray(k, np.float64)
    out = torch.empty(3 * X * Y * Z, dtype=torch.float32, device="cuda")
    ctx.check(lib.unet_vol_hessian_eig(ctx.handle, V._ptr(smooth_dev), X, Y, Z, k.ctypes.data, V._ptr(region_dev), V._ptr(out), V._stream()), "vol_hessian_eig")
    return out


def vesselness_device(smooth_dev, shape, k, dens, bright, index, best, scale, region_dev=None):
    """unet_vol_vesselness: the scale of index `index` into best (float32) / scale (uint8), updated in place; index 0 initialises them"""
    lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    k = np.ascontiguousarray(k, np.float64)
    ctx.check(lib.unet_vol_vesselness(ctx.handle, V._ptr(smooth_dev), X, Y, Z, k.ctypes.data, V._ptr(region_dev), float(dens[0]), float(dens[1]), float(dens[2]),
                                      1 if bright else 0, int(index), V._ptr(best), V._ptr(scale), V._stream()), "vol_vesselness")


def _vesselness_device(x32, shape, pixdim, sigmas, dens, bright, region_dev):
    """one Gaussian and one launch per scale; the smoothed volume of a scale is freed before the next -> (best, scale) on the device"""
    torch = V._torch()
    N = int(np.prod(shape))
    best = torch.empty(N, dtype=torch.float32, device="cuda")
    scale = torch.empty(N, dtype=torch.uint8, device="cuda")
    for i, s in enumerate(sigmas):
        sm = _smoothed(x32, shape, pixdim, s)
        vesselness_device(sm, shape, hessian_factors(s, pixdim), dens, bright, i, best, scale, region_dev)
        del sm
    return best, scale


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------------------------------
def hessian_eigenvalues(ct, sigma_mm, pixdim=None, region=None, return_device=False, src_shape=None):
    """The eigenvalues of the scale-normalised Hessian (gamma = 1: second differences times sigma^2 / h^2) of the CT smoothed by filters.gaussian_filter(sigma_mm=) ->
    float32 [3, X, Y, Z], sorted by magnitude |l1| <= |l2| <= |l3|, ties in diagonal order (return_device=True: the flat device tensor, l1 | l2 | l3).  A tube brighter
    than its surroundings has l1 near 0 and l2, l3 < 0; a plate only l3; a blob all three.  Outside the volume the edge voxel repeats.  A voxel whose Hessian is not
    finite (a NaN or an infinity within its 19 samples) gives three NaNs; region (a mask in the CT's shape): voxels outside it give +0.0.  sigma_mm = 0 is refused."""
    L._check_bool(return_device, "return_device")
    src, p = _source(ct, src_shape, pixdim)
    s = _check_sigma(sigma_mm, p)
    _region_arg(region, src.shape)
    if int(np.prod(src.shape)) == 0:
        raise ValueError("the volume has no voxel")
    region_dev = None if region is None else V._mask_to_device(region, src.shape)[0]
    out = hessian_eig_device(_smoothed(_decoded_device(src), src.shape, p, s), src.shape, hessian_factors(s, p), region_dev)
    return out if return_device else np.stack([V._host_of(out[i * int(np.prod(src.shape)):(i + 1) * int(np.prod(src.shape))], np.float32, src.shape) for i in range(3)])


def vesselness(ct, sigmas_mm=SIGMAS_MM, alpha=ALPHA, beta=BETA, c=C_HU, bright=True, region=None, pixdim=None, return_device=False, src_shape=None):
    """Frangi's tube measure over the Hessian eigenvalues at the scales sigmas_mm (strictly ascending, positive, at most 254) -> Vesselness.  At a scale the response is
    0 unless l2 < 0 and l3 < 0 (bright=False, darker tubes such as airways: l2 > 0 and l3 > 0); otherwise with RA = |l2| / |l3|, RB = |l1| / sqrt(|l2| |l3|) and
    S^2 = l1^2 + l2^2 + l3^2 it is (1 - exp(-RA^2 / 2 alpha^2)) exp(-RB^2 / 2 beta^2) (1 - exp(-S^2 / 2 c^2)), rounded once to float32.  response is the maximum over the
    scales, scale 1 + the index of the first scale that reached it (0 where the response is 0).  c is in the CT's units (HU).  region: only its voxels are computed, the
    others keep response 0 and scale 0.  One Gaussian and one launch per scale.  The defaults are conventional starting values, not clinically validated."""
    L._check_bool(return_device, "return_device")
    src, p = _source(ct, src_shape, pixdim)
    sigmas, dens, bright = _check_vesselness_args(sigmas_mm, alpha, beta, c, bright, p)
    _region_arg(region, src.shape)
    if int(np.prod(src.shape)) == 0:
        raise ValueError("the volume has no voxel")
    region_dev = None if region is None else V._mask_to_device(region, src.shape)[0]
    best, scale = _vesselness_device(_decoded_device(src), src.shape, p, sigmas, dens, bright, region_dev)
    if not return_device:
        best, scale = V._host_of(best, np.float32, src.shape), V._host_of(scale, np.uint8, src.shape)
    return Vesselness(response=best, scale=scale, sigmas_mm=sigmas, shape=tuple(src.shape), pixdim=tuple(float(v) for v in p))


def vessel_mask(ct, lungs, threshold=0.3, dense_hu=-500.0, max_radius_mm=3.0, min_ml=0.01, connectivity=3, erode_mm=2.0, pixdim=None, return_device=False, src_shape=None,
                **vesselness_kw):
    """The vessels inside the lungs -> VesselMask.  lungs: the lung mask in the CT's shape (an array, or a device uint8 tensor).  All steps run on the device:
      1. region = erode_mm(lungs != 0, erode_mm): keeps off the pleura, whose edge answers like a plate's rim;
      2. the vesselness under that region (vesselness_kw: sigmas_mm, alpha, beta, c, bright);
      3. dense = the CT >= dense_hu; candidates = (response >= threshold) & dense & region;
      4. thick = open_mm(dense, max_radius_mm), removed from the candidates: the rim of a dense blob -- a nodule, a consolidation -- answers as strongly as a thin tube,
         so no threshold separates them; the opening removes what a ball of max_radius_mm fits into.  Vessels thicker than that, at the hilum, are lost with it;
      5. remove_small(min_ml=, connectivity=).
    ml and n_components describe the final mask; vesselness is the Vesselness of step 2 (host arrays, or device tensors with return_device).  The thresholds are
    conventional defaults, configurable and not clinically validated here."""
    a = _check_vessel_mask_args(threshold, dense_hu, max_radius_mm, min_ml, connectivity, erode_mm, pixdim, **vesselness_kw)
    L._check_bool(return_device, "return_device")
    torch = V._torch()
    src, p = _source(ct, src_shape, pixdim)
    sigmas, dens, bright = _check_vesselness_args(pixdim=p, **a["vkw"])
    shape = src.shape
    L._mask_arg(lungs, shape, shape, "lungs")
    if int(np.prod(shape)) == 0:
        raise ValueError("the volume has no voxel")
    lungs_dev = V._mask_to_device(lungs, shape)[0]
    if isinstance(lungs, torch.Tensor):
        lungs_dev = (lungs_dev != 0).to(torch.uint8)
    region = V.ball_device(lungs_dev, shape, a["erode"], p, False)[0]
    best, scale = _vesselness_device(_decoded_device(src), shape, p, sigmas, dens, bright, region)
    dev = L._ct_device(src)
    dense = L.threshold_device(dev, src.vargs, a["dense_hu"], np.inf)[0]
    inside = L.threshold_device(dev, src.vargs, a["dense_hu"], np.inf, region)[0]
    cand = L.threshold_device(best, (16,) + tuple(shape) + (0, 1.0, 0.0), a["threshold"], np.inf, inside)[0]
    thick = dense
    for dilate in (False, True):
        thick = V.ball_device(thick, shape, a["max_radius"], p, dilate)[0]
    cand = L._and_not(cand, thick, shape)
    labels, n = V.label_device(cand, shape, a["connectivity"])
    vox = np.asarray(V.component_stats_device(labels, shape, n)["voxels"], np.int64)
    keep = np.zeros(n + 1, bool)
    keep[1:] = vox >= V.min_voxels_from_ml(a["min_ml"], p)
    mask = V.filter_components(labels, keep, n, shape, 0, 0)[0]
    voxels = int(vox[keep[1:]].sum())
    if not return_device:
        mask, best, scale = V._host_of(mask, np.uint8, shape), V._host_of(best, np.float32, shape), V._host_of(scale, np.uint8, shape)
    return VesselMask(mask=mask, ml=voxels * float(np.prod(p)) / 1000.0, n_components=int(keep.sum()),
                      vesselness=Vesselness(response=best, scale=scale, sigmas_mm=sigmas, shape=tuple(shape), pixdim=tuple(float(v) for v in p)))

"""Filter a CT's own voxels on the device (csrc/kernels_filter.hip).

    rank_filter(vol, rank, size= | footprint= | connectivity=, mode=, cval=)   -> FilteredVolume: the element of that rank under a footprint of radius <= 2
    median_filter / minimum_filter / maximum_filter / percentile_filter         -> the same selection at rank n // 2, 0, n - 1 and scipy's percentile rank
    grey_erosion / grey_dilation / grey_opening / grey_closing                  -> flat grey-scale morphology: minimum, maximum over the mirrored footprint, and both
    gaussian_filter(vol, sigma= | sigma_mm=)                                    -> float32 [X, Y, Z]: the low-pass resample_volume lacks before it coarsens
    footprint_bits / footprint_of_bits / structure                              -> a footprint as the 128-bit word of unet_vol_rank_filter; scipy's structures
    rank_filter_device                                                          -> the entry (unet_vol_rank_filter) on a device buffer

A rank filter selects and never computes: the result holds STORED elements of the source, bit for bit, and equals scipy.ndimage.rank_filter element for element.  The
order is the decoded one: for a scaled source with a negative slope the stored order is the reverse, so the launch is made with rank n - 1 - rank.  float32 is ordered by
a total order in which NaNs with the sign bit set sort lowest and the other NaNs highest (scipy leaves the place of a NaN to its sort).  Sources are what resample_volume
takes: a path, a NiftiVolume, an [X, Y, Z] array or a flat device tensor with src_shape=; float64 sources are refused (ask for float32).  Every argument error is a
ValueError raised before any device work; there is no CPU fallback for the device steps.  Non-flat structuring elements, morphological gradient and top-hat, footprints
beyond radius 2, "mirror" and "wrap" borders and sharding across ranks are out of scope (section 4ad).
"""
from __future__ import annotations

import numpy as np

from . import _lib, nifti_min
from . import volume as V

MAX_RADIUS = _lib.RANK_MAX_RADIUS
MODES = _lib.FILTER_MODES                                            # "nearest": the edge voxel repeats; "constant": cval; "reflect": scipy's default (d c b a | a b c d | d c b a)


class FilteredVolume:
    """What the rank filters return.  data: the selected STORED elements, in the source's stored dtype -- an [X, Y, Z] Fortran-order array, or with return_device=True the
    flat device tensor (uint16 / uint32, for which torch has no arithmetic type: their bytes as uint8); shape; slope, inter: the source's scaling (0.0, 0.0 when it is
    not scaled).  decoded(): float64, (float64(v) slope) + inter on the host, as get_fdata."""

    def __init__(self, data, shape, slope, inter, dtype):
        self.data, self.shape, self.slope, self.inter, self.dtype = data, tuple(shape), float(slope), float(inter), np.dtype(dtype)

    def decoded(self):
        host = self.data if isinstance(self.data, np.ndarray) else V._host_of(self.data, self.dtype, self.shape)
        return nifti_min.apply_scaling(host, self.slope, self.inter)


# ---- footprints -------------------------------------------------------------------------------------------------------------------------------------------------
def footprint_bits(footprint):
    """A bool [a, b, c] array with odd extents <= 5 and at least one voxel set -> (R, lo, hi): the footprint embedded centrally into the (2 R + 1)^3 cube, R = 1 or 2, as
    the 128-bit word hi:lo of unet_vol_rank_filter -- bit (dx + R) + (2 R + 1) ((dy + R) + (2 R + 1) (dz + R)) for the offset (dx, dy, dz)."""
    fp = np.asarray(footprint)
    if fp.ndim != 3 or fp.dtype.kind not in "biu":
        raise ValueError(f"a footprint is a bool [a, b, c] array, not {fp.dtype} with {fp.ndim} dimensions")
    if any(e % 2 == 0 or e > 2 * MAX_RADIUS + 1 for e in fp.shape):
        raise ValueError(f"a footprint has odd extents of at most {2 * MAX_RADIUS + 1} voxels (radius {MAX_RADIUS}), not {fp.shape}")
    fp = fp != 0
    if not fp.any():
        raise ValueError("a footprint holds at least one voxel")
    R = max(1, max(fp.shape) // 2)
    cube = np.zeros((2 * R + 1,) * 3, bool)
    cube[tuple(slice(R - e // 2, R + e // 2 + 1) for e in fp.shape)] = fp
    word = 0
    for b in np.flatnonzero(cube.reshape(-1, order="F")):
        word |= 1 << int(b)
    return R, word & (2 ** 64 - 1), word >> 64


def footprint_of_bits(R, lo, hi):
    """the inverse of footprint_bits -> bool [2 R + 1] * 3"""
    side = 2 * int(R) + 1
    word = int(lo) | (int(hi) << 64)
    if not 1 <= int(R) <= MAX_RADIUS or word < 0 or word >> side ** 3:
        raise ValueError(f"R lies in 1..{MAX_RADIUS} and the word holds no bit at or above (2 R + 1)^3")
    return np.array([(word >> b) & 1 for b in range(side ** 3)], bool).reshape((side,) * 3, order="F")


def structure(connectivity, per_slice=False):
    """scipy.ndimage.generate_binary_structure(3, connectivity): the 7, 19 or 27 voxels within `connectivity` axis steps of the centre; per_slice=True clears the planes
    with dz != 0 (5 or 9 voxels), for thick-slice scans"""
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (1, 2, 3):
        raise ValueError(f"connectivity is 1, 2 or 3, not {connectivity!r}")
    d = np.abs(np.arange(-1, 2))
    fp = (d[:, None, None] + d[None, :, None] + d[None, None, :]) <= int(connectivity)
    return _planar(fp, per_slice)


def _planar(fp, per_slice):
    if not isinstance(per_slice, (bool, np.bool_)):
        raise ValueError(f"per_slice is True or False, not {per_slice!r}")
    if per_slice:
        fp = fp.copy()
        c = fp.shape[2] // 2
        fp[:, :, :c] = False
        fp[:, :, c + 1:] = False
        if not fp.any():
            raise ValueError("per_slice leaves the footprint no voxel: none lies in the plane dz = 0")
    return fp


def _footprint(size=None, footprint=None, connectivity=None, per_slice=False):
    """exactly one of size (the default: 3), footprint, connectivity -> the bool footprint"""
    if sum(v is not None for v in (size, footprint, connectivity)) > 1:
        raise ValueError("size=, footprint= and connectivity= all describe the footprint: give one")
    if connectivity is not None:
        return structure(connectivity, per_slice)
    if footprint is not None:
        footprint_bits(footprint)                                   # (its checks)
        return _planar(np.asarray(footprint) != 0, per_slice)
    s = (3, 3, 3) if size is None else ((size,) * 3 if isinstance(size, (int, np.integer)) and not isinstance(size, bool) else size)
    try:
        s = tuple(s)
    except TypeError:
        s = ()
    if len(s) != 3 or any(isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < 1 or e % 2 == 0 or e > 2 * MAX_RADIUS + 1 for e in s):
        raise ValueError(f"size is an odd number of voxels up to {2 * MAX_RADIUS + 1}, or three of them, not {size!r}")
    return _planar(np.ones(tuple(int(e) for e in s), bool), per_slice)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------------------------
def _filter_source(vol, src_shape=None, pixdim=None):
    src = V._resample_source(vol, pixdim=pixdim, src_shape=src_shape)
    if src.vargs[0] == 64:
        raise ValueError("a float64 volume is not filtered: ask for float32 (an array of another dtype than the NIfTI element types is taken as float64)")
    return src


def _check_mode(mode):
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode is one of {sorted(MODES)}, not {mode!r}")
    return MODES[mode]


def _check_rank(rank, n):
    if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)) or not 0 <= int(rank) < n:
        raise ValueError(f"rank is an integer in 0..{n - 1} (the footprint holds {n} voxels), not {rank!r}")
    return int(rank)


def percentile_rank(percentile, n):
    """scipy.ndimage.percentile_filter's rank among n elements: p < 0 -> p + 100; n - 1 at p == 100; else int(float(n) p / 100)"""
    if isinstance(percentile, (bool, str)) or not isinstance(percentile, (int, float, np.integer, np.floating)) or not -100 <= percentile <= 100:
        raise ValueError(f"percentile is a number in -100..100, not {percentile!r}")
    p = percentile + 100.0 if percentile < 0 else percentile
    return n - 1 if p == 100 else int(float(n) * p / 100.0)


def _check_cval(cval, npdt):
    """cval is a STORED value: it must be an element of the stored dtype -> the numpy scalar"""
    if isinstance(cval, (bool, str)) or not isinstance(cval, (int, float, np.integer, np.floating)):
        raise ValueError(f"cval is a number, not {cval!r}")
    if npdt.kind in "iu":
        if not (np.isfinite(float(cval)) and float(cval) == int(cval) and np.iinfo(npdt).min <= int(cval) <= np.iinfo(npdt).max):
            raise ValueError(f"cval {cval!r} is not a value of the stored dtype {npdt}")
        return np.array(int(cval), npdt)[()]
    with np.errstate(over="ignore"):
        c = np.float32(cval)
    if not (np.isnan(c) and np.isnan(cval)) and float(c) != float(cval):
        raise ValueError(f"cval {cval!r} is not a value of the stored dtype {npdt}")
    return c


class _Plan:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape):
    """every check of the rank filters, without a device -> _Plan(src, npdt, fp, mode, cval: the stored scalar or None (the default is found at the launch))"""
    fp = _footprint(size, footprint, connectivity, per_slice)
    m = _check_mode(mode)
    if not isinstance(return_device, (bool, np.bool_)):
        raise ValueError(f"return_device is True or False, not {return_device!r}")
    src = _filter_source(vol, src_shape)
    npdt = np.dtype(nifti_min.DTYPES[src.vargs[0]])
    return _Plan(src=src, npdt=npdt, fp=fp, mode=m, cval=None if cval is None else _check_cval(cval, npdt), return_device=bool(return_device))


def launch_rank(rank, n, src):
    """the rank the device is asked for so that `rank` means decoded order: a negative slope reverses the stored order"""
    return n - 1 - rank if src.vargs[4] and src.vargs[5] < 0 else rank


# ---- the entry ----------------------------------------------------------------------------------------------------------------------------------------------------
def rank_filter_device(dev, code, shape, R, lo, hi, rank, mode, cval_bits):
    """unet_vol_rank_filter on a device buffer of prod(shape) elements of NIfTI type `code` -> a new uint8 device tensor holding the selected elements' bytes"""
    torch = V._torch(); lib, ctx = V._ctx()
    V._check_volume_dims(shape)
    out = torch.empty(int(np.prod(shape)) * np.dtype(nifti_min.DTYPES[code]).itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_rank_filter(ctx.handle, V._ptr(dev), int(code), *(int(v) for v in shape), int(R), int(lo), int(hi), int(rank), int(mode), int(cval_bits),
                                       V._ptr(out), V._stream()), "vol_rank_filter")
    return out


def _run(p, steps):
    """steps: (footprint, decoded rank) one after the other, the intermediate volume staying on the device -> FilteredVolume"""
    src = p.src
    code = src.vargs[0]
    cval = p.cval
    if p.mode == MODES["constant"] and cval is None:
        cval = V._stored_extreme(src)                               # the stored element that decodes to the minimum, as resample_volume(dtype="raw")
    bits = V._bits_of(0 if cval is None else cval, p.npdt)
    dev = src.tensor if src.tensor is not None else V.upload(src.vol)
    for fp, rank in steps:
        R, lo, hi = footprint_bits(fp)
        n = int(np.count_nonzero(fp))
        dev = rank_filter_device(dev, code, src.shape, R, lo, hi, launch_rank(rank, n, src), p.mode, bits)
    if p.return_device:
        data = dev.view(getattr(V._torch(), V._TORCH_OF_CODE[code])) if code in V._TORCH_OF_CODE else dev
    else:
        data = V._host_of(dev, p.npdt, src.shape)
    sc = (src.vargs[5], src.vargs[6]) if src.vargs[4] else (0.0, 0.0)
    return FilteredVolume(data, src.shape, sc[0], sc[1], p.npdt)


# ---- the filters --------------------------------------------------------------------------------------------------------------------------------------------------
def rank_filter(vol, rank, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """The element of rank `rank` (0 = the smallest in decoded order, rank < n) among the voxels under the footprint -> FilteredVolume.  The footprint, one of: size= (an
    odd box of 1, 3 or 5 voxels, or three such extents; the default is 3), footprint= (a bool array with odd extents <= 5) or connectivity= (structure(): 7, 19 or 27
    voxels); per_slice=True clears its planes with dz != 0.  mode: "reflect" (the default, scipy's), "nearest" or "constant" -- then outside the volume reads cval, a
    STORED value that must be an element of the stored dtype; its default is the stored element that decodes to the volume's minimum (air, for a CT).  This is
    scipy.ndimage.rank_filter(stored, rank, footprint=fp, mode=mode, cval=cval) element for element (NaNs aside, whose place scipy leaves to its sort)."""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    return _run(p, [(p.fp, _check_rank(rank, int(np.count_nonzero(p.fp))))])


def median_filter(vol, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """rank_filter at rank n // 2: the remedy for voxels that hop across a HU band edge on noise alone"""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    return _run(p, [(p.fp, int(np.count_nonzero(p.fp)) // 2)])


def minimum_filter(vol, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """rank_filter at rank 0"""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    return _run(p, [(p.fp, 0)])


def maximum_filter(vol, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """rank_filter at rank n - 1"""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    return _run(p, [(p.fp, int(np.count_nonzero(p.fp)) - 1)])


def percentile_filter(vol, percentile, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """rank_filter at scipy's rank for a percentile (percentile_rank): p < 0 counts from 100, p == 100 is the maximum, otherwise int(n p / 100)"""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    return _run(p, [(p.fp, percentile_rank(percentile, int(np.count_nonzero(p.fp))))])


def _mirrored(fp):
    return np.ascontiguousarray(fp[::-1, ::-1, ::-1])


def grey_erosion(vol, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """Flat grey-scale erosion: the minimum over the footprint (scipy.ndimage.grey_erosion with a flat footprint)"""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    return _run(p, [(p.fp, 0)])


def grey_dilation(vol, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """Flat grey-scale dilation: the maximum over the MIRRORED footprint fp[::-1, ::-1, ::-1], as scipy.ndimage.grey_dilation does it"""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    return _run(p, [(_mirrored(p.fp), int(np.count_nonzero(p.fp)) - 1)])


def grey_opening(vol, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """Erosion, then dilation, with one footprint and mode: two launches, the eroded volume stays on the device.  It removes bright detail smaller than the footprint."""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    n = int(np.count_nonzero(p.fp))
    return _run(p, [(p.fp, 0), (_mirrored(p.fp), n - 1)])


def grey_closing(vol, size=None, footprint=None, connectivity=None, mode="reflect", cval=None, per_slice=False, return_device=False, src_shape=None):
    """Dilation, then erosion, with one footprint and mode: two launches, the dilated volume stays on the device.  It removes dark detail smaller than the footprint."""
    p = _plan(vol, size, footprint, connectivity, per_slice, mode, cval, return_device, src_shape)
    n = int(np.count_nonzero(p.fp))
    return _run(p, [(_mirrored(p.fp), n - 1), (p.fp, 0)])


# ---- the Gaussian ---------------------------------------------------------------------------------------------------------------------------------------------------
def _check_sigma(sigma, sigma_mm, pixdim):
    """-> the three widths in voxels; pixdim: the source's, needed by sigma_mm"""
    if (sigma is None) == (sigma_mm is None):
        raise ValueError("give one of sigma= (voxels) and sigma_mm= (millimetres)")
    given = sigma if sigma is not None else sigma_mm
    try:
        s = np.asarray(given, np.float64).reshape(-1)
    except (TypeError, ValueError):
        s = np.zeros(0)
    if isinstance(given, (bool, str)) or s.size not in (1, 3) or not np.isfinite(s).all() or (s < 0).any():
        raise ValueError(f"a Gaussian width is a finite number >= 0, or three of them, not {given!r}")
    s = np.broadcast_to(s, (3,)).astype(np.float64)
    if sigma_mm is not None:
        if pixdim is None:
            raise ValueError("sigma_mm needs the voxel size: pass pixdim= (an array or a device tensor carries none)")
        s = s / V._check_pixdim(pixdim)
    return tuple(float(v) for v in s)


def gaussian_filter(vol, sigma=None, sigma_mm=None, pixdim=None, return_device=False, src_shape=None):
    """A separable Gaussian low-pass of the DECODED volume -> float32 [X, Y, Z] (Fortran order; return_device=True: the flat device tensor).  sigma: the width in voxels,
    a scalar or one per axis; sigma_mm: in millimetres, divided by the source's pixdim (a file's own, or pixdim=).  The volume is decoded to float32 once (get_fdata
    rounded once; an unscaled device tensor: tensor.to(float32)); then one pass of volume.gaussian_weights(sigma) -- 2 ceil(3 sigma) + 1 taps, float64 weights, float64
    sum rounded to float32 per pass -- runs along x, y and z (unet_vol_smooth_axis).  An axis with sigma = 0 is skipped; outside the volume the edge voxel repeats, the
    only mode.  The use the resampler lacks -- it does not filter before it coarsens --, with sigma about half the coarsening factor:
        low = gaussian_filter(ct, sigma_mm=2.0, return_device=True)
        coarse = resample_volume(low, src_shape=ct_shape, pixdim=ct_pixdim, spacing=(4.0, 4.0, 4.0))"""
    if not isinstance(return_device, (bool, np.bool_)):
        raise ValueError(f"return_device is True or False, not {return_device!r}")
    torch = V._torch()
    src = _filter_source(vol, src_shape, pixdim)
    widths = _check_sigma(sigma, sigma_mm, pixdim if pixdim is not None else (src.vol.pixdim if src.header is not None else None))          # (a file's own pixdim)
    weights = [V.gaussian_weights(s) for s in widths]
    if src.tensor is not None:
        x = src.tensor.to(torch.float32)
        if x is src.tensor:
            x = x.clone()
    else:
        x = torch.from_numpy(np.asfortranarray(src.vol.get_fdata().astype(np.float32)).reshape(-1, order="F")).cuda()
    if x.numel() > 0:
        for axis, w in enumerate(weights):
            if w is not None:
                x = V.smooth_axis_device(x, 1, src.shape, axis, w)
    return x if return_device else V._host_of(x, np.float32, src.shape)

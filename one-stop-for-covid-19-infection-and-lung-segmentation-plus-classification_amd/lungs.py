"""A lung mask from the CT itself on the device: air, body, airways (csrc/kernels_lungmask.hip).

    threshold_volume(ct, lo=, hi=, region=)                     -> uint8 [X, Y, Z]: lo <= value < hi on the values get_fdata gives (unet_vol_threshold)
    geodesic_distance(seeds, constraint, connectivity=)         -> (arrival uint16, counts): breadth-first growth of the seeds inside the constraint, the step at which every
                                                                   voxel was reached and the voxels reached per step (unet_vol_geodesic_begin / _steps)
    reconstruct(mask, marker)                                   -> the components of the mask that hold a marker voxel
    body_mask(ct, body_hu=)                                     -> the patient: the largest component of value >= body_hu, holes filled slice by slice
    find_trachea(air_in_body, pixdim, superior)                 -> TracheaSeed or None: a small round air component that continues over a few slices from the superior end
    grow_airways(ct, seed, within)                              -> AirwayGrowth: trachea and main bronchi by explosion-controlled region growing
    lung_mask(ct, model=None, ...)                              -> LungMask: the procedure on top of them, from nothing but the CT (or from a lung U-Net's prediction)
    threshold_device / geodesic_device                          -> the entries on device buffers

Sources are what filters / resample_volume take: a path, a NiftiVolume, an [X, Y, Z] array, or a flat device tensor with src_shape= (masks: shape=).  Every device
result equals tests/lungmask_oracle.py element for element.  Every argument error is a ValueError raised before any device work; there is no CPU fallback for the device
steps.  The geodesic distance is a count of steps inside the constraint, not millimetres.  The airway growth is explosion-controlled region growing with a front-count
criterion: its thresholds (airway_hu, leak_ratio, min_front, ref_steps), like air_hu, body_hu, min_lung_ml and min_ratio, are conventional defaults, configurable and
NOT clinically validated here.  Lobes and fissures, vessel exclusion inside the mask itself (vessels.vessel_mask finds the vessels afterwards, section 4af), dense
consolidation at the pleura (a threshold misses it unless close_mm bridges it), per-branch leak control (the front count is global), airway walls and sharding across
ranks are out of scope (section 4ae).
"""
from __future__ import annotations

import os
import time

import numpy as np

from . import _lib, nifti_min
from . import volume as V

MAX_STEP = _lib.GEODESIC_MAX_STEP
UNREACHED = 0xFFFF
AIR_HU, BODY_HU, AIRWAY_HU = -320.0, -500.0, -950.0                  # conventional, configurable, not validated here
MIN_LUNG_ML, MIN_RATIO = 50.0, V.LUNG_MIN_RATIO
_TRACHEA_KEYS = ("area_mm2", "max_extent_mm", "seed_slices", "seed_shift_mm")
_GROW_KEYS = ("airway_hu", "leak_ratio", "min_front", "ref_steps", "max_steps", "connectivity")
_LUNG_MASK_KEYS = {"model", "threshold", "air_hu", "body_hu", "airways", "airway_dilate_mm", "min_lung_ml", "min_ratio", "fill", "close_mm", "orientation", "batch_size",
                   "img_size", "pixdim"} | set(_TRACHEA_KEYS) | set(_GROW_KEYS)


class LungMaskError(ValueError):
    """lung_mask found no lung: no component reaches min_lung_ml, or airways=True and no trachea"""


class TracheaSeed:
    """find_trachea's result.  label: of the per-slice labelling; z: its slice; cx, cy: its centroid (float64 voxel coordinates); voxels; area_mm2; mask: the component as
    a flat uint8 device tensor."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"TracheaSeed(z={self.z}, centroid=({self.cx:.1f}, {self.cy:.1f}), area_mm2={self.area_mm2:.0f})"


class AirwayGrowth:
    """grow_airways' result.  mask: arrival <= stop_step, uint8 [X, Y, Z] (return_device=True: the flat device tensor); counts: int64, the front of every step; leak_step:
    the first step whose front exploded, or None; stop_step: the last step kept."""

    def __init__(self, mask, counts, leak_step, stop_step):
        self.mask, self.counts, self.leak_step, self.stop_step = mask, counts, leak_step, stop_step

    def __repr__(self):
        return f"AirwayGrowth(steps={len(self.counts) - 1}, leak_step={self.leak_step}, stop_step={self.stop_step})"


class LungMask:
    """lung_mask's result.  mask: uint8 [X, Y, Z] (return_device=True: the flat device tensor); shape; pixdim; lung_ml; components: the kept rows of the component table of
    the labelling (volume.LESION_DTYPE); airways: the AirwayGrowth, or None when the step did not run; airway_error: why it did not, or None; method: "threshold" or
    "model"; seconds: the time of every step."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"LungMask(shape={self.shape}, lung_ml={self.lung_ml:.1f}, components={len(self.components)}, method={self.method!r}, airway_error={self.airway_error!r})"


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------------------------
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _check_bool(v, what):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{what} is True or False, not {v!r}")
    return bool(v)


def _check_edges(lo, hi):
    """-> (lo, hi) as floats, None = unbounded; a NaN edge or lo >= hi: ValueError"""
    for v, what in ((lo, "lo"), (hi, "hi")):
        if v is not None and not _is_number(v):
            raise ValueError(f"{what} is a number or None, not {v!r}")
    a = -np.inf if lo is None else float(lo)
    b = np.inf if hi is None else float(hi)
    if np.isnan(a) or np.isnan(b) or not a < b:
        raise ValueError(f"the edges must satisfy lo < hi and neither is NaN, not lo={lo!r}, hi={hi!r}")
    return a, b


def _check_hu(v, what):
    if not _is_number(v) or not np.isfinite(float(v)):
        raise ValueError(f"{what} is a finite number, not {v!r}")
    return float(v)


def _check_growth_args(max_steps=None, chunk=32):
    if max_steps is not None and (not _is_int(max_steps) or not 1 <= int(max_steps) <= MAX_STEP):
        raise ValueError(f"max_steps is None or an integer in 1..{MAX_STEP}, not {max_steps!r}")
    if not _is_int(chunk) or not 1 <= int(chunk) <= MAX_STEP:
        raise ValueError(f"chunk is an integer in 1..{MAX_STEP}, not {chunk!r}")
    return (MAX_STEP if max_steps is None else int(max_steps)), int(chunk)


def _check_trachea_args(area_mm2=(50.0, 1200.0), max_extent_mm=35.0, seed_slices=3, seed_shift_mm=10.0):
    try:
        a0, a1 = (float(v) for v in area_mm2)
    except (TypeError, ValueError):
        raise ValueError(f"area_mm2 is a pair of areas, not {area_mm2!r}") from None
    if not (np.isfinite(a0) and np.isfinite(a1) and 0.0 <= a0 <= a1):
        raise ValueError(f"area_mm2 is a pair 0 <= least <= most of finite areas, not {area_mm2!r}")
    for v, what in ((max_extent_mm, "max_extent_mm"), (seed_shift_mm, "seed_shift_mm")):
        if not _is_number(v) or not (np.isfinite(float(v)) and float(v) > 0.0):
            raise ValueError(f"{what} is a positive finite number, not {v!r}")
    if not _is_int(seed_slices) or int(seed_slices) < 1:
        raise ValueError(f"seed_slices is an integer >= 1, not {seed_slices!r}")
    return (a0, a1), float(max_extent_mm), int(seed_slices), float(seed_shift_mm)


def _check_grow_args(airway_hu=AIRWAY_HU, leak_ratio=3.0, min_front=8, ref_steps=4, max_steps=2000, connectivity=1):
    hu = _check_hu(airway_hu, "airway_hu")
    if not _is_number(leak_ratio) or not (np.isfinite(float(leak_ratio)) and float(leak_ratio) > 1.0):
        raise ValueError(f"leak_ratio is a finite number > 1, not {leak_ratio!r}")
    if not _is_int(min_front) or int(min_front) < 1:
        raise ValueError(f"min_front is an integer >= 1, not {min_front!r}")
    if not _is_int(ref_steps) or int(ref_steps) < 1:
        raise ValueError(f"ref_steps is an integer >= 1, not {ref_steps!r}")
    limit, _ = _check_growth_args(max_steps)
    if max_steps is None:
        raise ValueError("max_steps is an integer: the airway growth is bounded")
    return hu, float(leak_ratio), int(min_front), int(ref_steps), limit, V._check_connectivity(connectivity)


def _check_superior(superior):
    if superior not in ("z+", "z-"):
        raise ValueError(f'superior is "z+" (the last slice is the superior end) or "z-", not {superior!r}')
    return superior


def superior_of(codes):
    """axis codes -> "z+" when voxel axis 2 grows towards S, "z-" towards I, None when axis 2 is no S / I axis (or without codes)"""
    if codes is None:
        return None
    return {"S": "z+", "I": "z-"}.get(str(codes[2]))


def _ct_source(ct, src_shape=None, pixdim=None):
    return V._resample_source(ct, pixdim=pixdim, src_shape=src_shape)


def _ct_device(src):
    return src.tensor if src.tensor is not None else V.upload(src.vol)


def _mask_arg(mask, shape, want_shape, what):
    """what _mask_to_device refuses, and the shape, before anything is uploaded"""
    V._check_mask_host(mask, shape)
    got = tuple(int(v) for v in shape) if isinstance(mask, V._torch().Tensor) else tuple(int(v) for v in np.asarray(mask).shape)
    if want_shape is not None and got != tuple(want_shape):
        raise ValueError(f"{what} is {got}, the volume {tuple(want_shape)}")
    return got


# ---- the entries ------------------------------------------------------------------------------------------------------------------------------------------------------
def threshold_device(dev, vargs, lo, hi, region_dev=None, slice_counts=False):
    """unet_vol_threshold on a device buffer; vargs: (dtype code, X, Y, Z, scaled, slope, inter) -> (mask: uint8 device tensor of X*Y*Z bytes in Fortran order, the set
    voxels per slice as an int64 [Z] device tensor or None)"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in vargs[1:4])
    V._check_volume_dims((X, Y, Z))
    mask = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(max(Z, 1), dtype=torch.int64, device="cuda") if slice_counts else None
    ctx.check(lib.unet_vol_threshold(ctx.handle, V._ptr(dev), int(vargs[0]), X, Y, Z, int(vargs[4]), float(vargs[5]), float(vargs[6]), float(lo), float(hi), V._ptr(region_dev),
                                     V._ptr(mask), V._ptr(counts), V._stream()), "vol_threshold")
    return mask, (counts[:Z] if slice_counts else None)


def _mask_vargs(shape):
    return (2,) + tuple(int(v) for v in shape) + (0, 1.0, 0.0)


def _and_not(a_dev, b_dev, shape):
    """a & ~b of two device masks, by the threshold entry: b's bytes below 1, inside the region a"""
    return threshold_device(b_dev, _mask_vargs(shape), -np.inf, 1.0, a_dev)[0]


def geodesic_device(seeds_dev, constraint_dev, shape, connectivity=1, per_slice=False, max_steps=None, chunk=32):
    """unet_vol_geodesic_begin, then unet_vol_geodesic_steps in calls of `chunk` steps until a step reaches nothing or max_steps have run -> (arrival: the uint16 [X Y Z]
    volume as a uint8 device tensor of 2 X Y Z bytes (torch has no arithmetic type for it), counts: int64 numpy [steps reached + 1]).  The counts come to the host between
    the calls, nothing else does."""
    connectivity = V._check_structure(connectivity, per_slice)
    limit, chunk = _check_growth_args(max_steps, chunk)
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    N = X * Y * Z
    arrival = torch.empty(2 * N, dtype=torch.uint8, device="cuda")
    if N == 0:
        return arrival, np.zeros(1, np.int64)
    counts = torch.zeros(limit + 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_geodesic_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_geodesic_begin(ctx.handle, V._ptr(seeds_dev), V._ptr(constraint_dev), X, Y, Z, V._ptr(arrival), V._ptr(counts), V._ptr(ws), ws.numel(), V._stream()),
              "vol_geodesic_begin")
    if int(counts[0].item()) == 0:
        return arrival, np.zeros(1, np.int64)
    first, last = 1, limit
    while first <= limit:
        n = min(chunk, limit - first + 1)
        ctx.check(lib.unet_vol_geodesic_steps(ctx.handle, X, Y, Z, first, n, connectivity, 1 if per_slice else 0, V._ptr(arrival), V._ptr(counts), V._ptr(ws), ws.numel(),
                                              V._stream()), "vol_geodesic_steps")
        empty = np.flatnonzero(counts[first:first + n].cpu().numpy() == 0)
        if empty.size:
            last = first + int(empty[0]) - 1
            break
        first += n
    return arrival, counts[:last + 1].cpu().numpy()


# ---- the two passes ---------------------------------------------------------------------------------------------------------------------------------------------------
def threshold_volume(ct, lo=None, hi=None, region=None, return_device=False, src_shape=None):
    """The voxels whose value v -- what get_fdata gives: float64(raw), then (v * slope) + inter as two rounded operations for a scaled file -- satisfies lo <= v < hi, as
    uint8 0 / 1 in the CT's shape (return_device=True: the flat device tensor).  lo=None / hi=None: unbounded on that side; -inf and +inf are allowed, a NaN edge or
    lo >= hi is a ValueError.  A NaN value gives 0.  region: a mask in the CT's shape (an array, or a device uint8 tensor); only its non-zero voxels can be set."""
    a, b = _check_edges(lo, hi)
    _check_bool(return_device, "return_device")
    src = _ct_source(ct, src_shape)
    if region is not None:
        _mask_arg(region, src.shape, src.shape, "region")
    region_dev = None if region is None else V._mask_to_device(region, src.shape)[0]
    mask, _ = threshold_device(_ct_device(src), src.vargs, a, b, region_dev)
    return V._result(mask, src.shape, bool(return_device))


def geodesic_distance(seeds, constraint, connectivity=1, per_slice=False, max_steps=None, chunk=32, return_device=False, shape=None):
    """Breadth-first growth of `seeds` inside `constraint` (masks: arrays, or device uint8 tensors with shape=) -> (arrival, counts).  arrival: uint16 [X, Y, Z] -- 0 on
    seeds & constraint, s on the voxels step s reached, 0xFFFF elsewhere (return_device=True: its bytes as a flat uint8 device tensor); counts: int64
    [steps reached + 1], the voxels reached at every step.  Step s reaches the unreached constraint voxels with a neighbour, under generate_binary_structure(3,
    connectivity) (per_slice=True: without its dz != 0 planes, connectivity 1 or 2), reached at step s - 1: by definition the geodesic STEP distance inside the constraint,
    a count of steps and not millimetres.  Seeds outside the constraint are ignored.  The launches go in calls of `chunk` steps, the counts coming to the host between
    them; the growth stops at the first step that reaches nothing or after max_steps (None: 65534, the most a uint16 holds beside the mark 0xFFFF)."""
    V._check_structure(connectivity, per_slice)
    _check_bool(per_slice, "per_slice")
    _check_growth_args(max_steps, chunk)
    _check_bool(return_device, "return_device")
    shp = _mask_arg(seeds, shape, None, "seeds")
    _mask_arg(constraint, shape, shp, "constraint")
    sd, shp = V._mask_to_device(seeds, shape)
    cd, _ = V._mask_to_device(constraint, shape)
    arrival, counts = geodesic_device(sd, cd, shp, connectivity, bool(per_slice), max_steps, chunk)
    return (arrival if return_device else V._host_of(arrival, np.uint16, shp)), counts


def _reconstruct_device(mask_dev, marker_dev, shape, connectivity=1):
    torch = V._torch()
    labels, n = V.label_device(mask_dev, shape, connectivity)
    keep = np.zeros(n + 1, bool)
    if n > 0:
        cover, _ = V.lesion_overlap_device(labels, n, (marker_dev != 0).to(torch.int32), 1, shape)
        keep[1:] = cover > 0
    return V.filter_components(labels, keep, n, shape, 0, 0)[0]


def reconstruct(mask, marker, connectivity=1, return_device=False, shape=None):
    """The components of mask != 0 (connectivity 1, 2, 3 = 6, 18, 26 neighbours) that hold a voxel of marker != 0, as uint8 0 / 1: morphological reconstruction of the
    marker under the mask, by labelling (label_device), the overlap of every component with the marker (lesion_overlap_device) and filter_components."""
    V._check_connectivity(connectivity)
    _check_bool(return_device, "return_device")
    shp = _mask_arg(mask, shape, None, "mask")
    _mask_arg(marker, shape, shp, "marker")
    md, shp = V._mask_to_device(mask, shape)
    kd, _ = V._mask_to_device(marker, shape)
    return V._result(_reconstruct_device(md, kd, shp, int(connectivity)), shp, bool(return_device))


# ---- the procedure ----------------------------------------------------------------------------------------------------------------------------------------------------
def _largest_component_device(mask_dev, shape, connectivity=1):
    labels, n = V.label_device(mask_dev, shape, connectivity)
    keep = np.zeros(n + 1, bool)
    if n > 0:
        keep[V.largest_labels(V.component_stats_device(labels, shape, n)["voxels"], 1)] = True
    return V.filter_components(labels, keep, n, shape, 0, 0)[0]


def _body_device(dev, src, body_hu):
    solid, _ = threshold_device(dev, src.vargs, body_hu, np.inf)
    return V.fill_holes_device(_largest_component_device(solid, src.shape, 1), src.shape, 1, per_slice=True)[0]


def body_mask(ct, body_hu=BODY_HU, return_device=False, src_shape=None):
    """The patient without the air around them and without the table: the component of most voxels (connectivity 1, ties to the lower label) of value >= body_hu, its
    holes -- lungs, airways, bowel gas -- filled slice by slice (fill_holes(per_slice=True), connectivity 1).  uint8 0 / 1."""
    hu = _check_hu(body_hu, "body_hu")
    _check_bool(return_device, "return_device")
    src = _ct_source(ct, src_shape)
    return V._result(_body_device(_ct_device(src), src, hu), src.shape, bool(return_device))


def trachea_from_stats(stats, Z, pixdim, superior, area_mm2=(50.0, 1200.0), max_extent_mm=35.0, seed_slices=3, seed_shift_mm=10.0):
    """The search of find_trachea on the records of the per-slice component table (host only) -> the 0-based row of the seed, or None"""
    px, py = float(pixdim[0]), float(pixdim[1])
    vox = np.asarray(stats["voxels"], np.int64)
    if vox.size == 0:
        return None
    area = vox.astype(np.float64) * (px * py)
    ok = (area >= area_mm2[0]) & (area <= area_mm2[1])
    ok &= ((np.asarray(stats["x1"], np.int64) - stats["x0"] + 1).astype(np.float64) * px <= max_extent_mm)
    ok &= ((np.asarray(stats["y1"], np.int64) - stats["y0"] + 1).astype(np.float64) * py <= max_extent_mm)
    cx, cy = np.asarray(stats["sx"], np.float64) / vox, np.asarray(stats["sy"], np.float64) / vox
    by_slice = {}
    for i in np.flatnonzero(ok):
        by_slice.setdefault(int(stats["z0"][i]), []).append(int(i))
    step = -1 if superior == "z+" else 1
    r2 = seed_shift_mm * seed_shift_mm
    for z in (range(Z - 1, -1, -1) if superior == "z+" else range(Z)):
        for i in by_slice.get(z, []):
            cur, good = i, True
            for k in range(1, seed_slices):
                nxt = [j for j in by_slice.get(z + step * k, []) if ((cx[j] - cx[cur]) * px) ** 2 + ((cy[j] - cy[cur]) * py) ** 2 <= r2]
                if not nxt:
                    good = False
                    break
                cur = nxt[0]
            if good:
                return i
    return None


def _find_trachea_device(air_dev, shape, pixdim, superior, targs):
    labels, n = V.label_device(air_dev, shape, 1, per_slice=True)
    if n == 0:
        return None
    st = V.component_stats_device(labels, shape, n)
    i = trachea_from_stats(st, shape[2], pixdim, superior, *targs)
    if i is None:
        return None
    keep = np.zeros(n + 1, bool)
    keep[i + 1] = True
    vox = int(st["voxels"][i])
    return TracheaSeed(label=i + 1, z=int(st["z0"][i]), cx=float(st["sx"][i]) / vox, cy=float(st["sy"][i]) / vox, voxels=vox,
                       area_mm2=vox * float(pixdim[0]) * float(pixdim[1]), mask=V.filter_components(labels, keep, n, shape, 0, 0)[0], shape=tuple(shape))


def find_trachea(air_in_body, pixdim, superior, area_mm2=(50.0, 1200.0), max_extent_mm=35.0, seed_slices=3, seed_shift_mm=10.0, shape=None):
    """The trachea's cross-section near the superior end of a mask of the air inside the body -> TracheaSeed, or None when there is none.  superior: "z+" (the last slice
    is the superior end) or "z-"; it is never guessed.  The mask is labelled slice by slice (label_device(per_slice=True), connectivity 1) and its component table comes
    to the host (component_stats_device); the volume stays on the device.  A candidate is an in-slice component whose area lies in area_mm2 and whose in-plane
    bounding-box extents are both <= max_extent_mm.  Walking from the superior end, slice by slice and candidate by candidate in label order: a candidate is the seed
    when a chain continues it through the next seed_slices - 1 slices, each link the lowest-labelled candidate of the next slice whose centroid lies within seed_shift_mm
    (in the plane, millimetres) of the current link's centroid."""
    p = V._check_pixdim(pixdim)
    _check_superior(superior)
    targs = _check_trachea_args(area_mm2, max_extent_mm, seed_slices, seed_shift_mm)
    _mask_arg(air_in_body, shape, None, "air_in_body")
    dev, shp = V._mask_to_device(air_in_body, shape)
    return _find_trachea_device(dev, shp, p, superior, targs)


def leak_rule(counts, leak_ratio=3.0, min_front=8, ref_steps=4):
    """The front-count criterion on the host -> (leak_step or None, stop_step).  m = min(counts[:ref_steps]); the first step s >= ref_steps with
    counts[s] > leak_ratio * max(m, min_front) (float64) is the leak; m takes counts[s] in after each test.  stop_step: the last step before the leak whose count equals
    the running minimum at that point; without a leak the last step."""
    c = [int(v) for v in counts]
    if not c:
        raise ValueError("leak_rule: no counts")
    head = c[:ref_steps]
    m = min(head)
    stop = max(i for i, v in enumerate(head) if v == m)
    for s in range(ref_steps, len(c)):
        if float(c[s]) > float(leak_ratio) * float(max(m, min_front)):
            return s, stop
        if c[s] <= m:
            m, stop = c[s], s
    return None, len(c) - 1


def _grow_device(dev, src, seed_dev, within_dev, gargs):
    hu, ratio, min_front, ref_steps, limit, conn = gargs
    constraint, _ = threshold_device(dev, src.vargs, -np.inf, hu, within_dev)
    arrival, counts = geodesic_device(seed_dev, constraint, src.shape, conn, False, limit)
    leak, stop = leak_rule(counts, ratio, min_front, ref_steps)
    mask, _ = threshold_device(arrival, (512,) + tuple(src.shape) + (0, 1.0, 0.0), -np.inf, float(stop) + 1.0)          # arrival <= stop_step: 0xFFFF stays out
    return AirwayGrowth(mask, counts, leak, stop)


def grow_airways(ct, seed, within, airway_hu=AIRWAY_HU, leak_ratio=3.0, min_front=8, ref_steps=4, max_steps=2000, connectivity=1, return_device=False, src_shape=None):
    """Trachea and main bronchi from a seed -> AirwayGrowth(mask, counts, leak_step, stop_step).  The growth is geodesic_distance(seed, within & (value < airway_hu)); seed
    and within: masks in the CT's shape (a TracheaSeed's mask, the candidate component that holds it).  An airway that leaks into the lung shows as a front that
    explodes; the rule (leak_rule) runs on the host, on the counts: m = min(counts[:ref_steps]); the first step s >= ref_steps with
    counts[s] > leak_ratio * max(m, min_front) is the leak, m taking counts[s] in after each test; stop_step is the last step before the leak whose count equals the
    running minimum at that point, without a leak the last step.  The airway is arrival <= stop_step.  This is explosion-controlled region growing with a front-count
    criterion over the WHOLE front (no per-branch control); the defaults are conventional, configurable and not clinically validated here."""
    gargs = _check_grow_args(airway_hu, leak_ratio, min_front, ref_steps, max_steps, connectivity)
    _check_bool(return_device, "return_device")
    src = _ct_source(ct, src_shape)
    seed_mask = seed.mask if isinstance(seed, TracheaSeed) else seed
    _mask_arg(seed_mask, src.shape, src.shape, "seed")
    _mask_arg(within, src.shape, src.shape, "within")
    sd, _ = V._mask_to_device(seed_mask, src.shape)
    wd, _ = V._mask_to_device(within, src.shape)
    g = _grow_device(_ct_device(src), src, sd, wd, gargs)
    g.mask = V._result(g.mask, src.shape, bool(return_device))
    return g


def _check_lung_mask_args(model=None, threshold=0.5, air_hu=AIR_HU, body_hu=BODY_HU, airways="auto", airway_dilate_mm=None, min_lung_ml=MIN_LUNG_ML, min_ratio=MIN_RATIO,
                          fill=True, close_mm=None, orientation=None, batch_size=32, img_size=512, pixdim=None, **airway_kw):
    """every check of lung_mask that needs no volume -> the checked values as a dict, or ValueError"""
    if model is not None and not callable(getattr(model, "predict", None)):
        raise ValueError(f"model is None or has a predict method, not {model!r}")
    if not _is_number(threshold) or not 0.0 <= float(threshold) <= 1.0:
        raise ValueError(f"threshold is a probability in 0..1, not {threshold!r}")
    if not (airways is True or airways is False or airways == "auto"):
        raise ValueError(f'airways is "auto", True or False, not {airways!r}')
    bad = set(airway_kw) - set(_TRACHEA_KEYS) - set(_GROW_KEYS)
    if bad:
        raise ValueError(f"lung_mask takes the keywords of find_trachea {_TRACHEA_KEYS} and grow_airways {_GROW_KEYS}, not {sorted(bad)}")
    if not _is_number(min_lung_ml) or not (np.isfinite(float(min_lung_ml)) and float(min_lung_ml) >= 0.0):
        raise ValueError(f"min_lung_ml is a finite number >= 0, not {min_lung_ml!r}")
    if not _is_number(min_ratio) or not 0.0 < float(min_ratio) <= 1.0:
        raise ValueError(f"min_ratio is a number in (0, 1], not {min_ratio!r}")
    for v, what in ((batch_size, "batch_size"), (img_size, "img_size")):
        if not _is_int(v) or int(v) < 1:
            raise ValueError(f"{what} is an integer >= 1, not {v!r}")
    lin, codes = V._check_orientation(orientation)
    return dict(air_hu=_check_hu(air_hu, "air_hu"), body_hu=_check_hu(body_hu, "body_hu"), threshold=float(threshold), fill=_check_bool(fill, "fill"),
                dilate=None if airway_dilate_mm is None else V._check_radius(airway_dilate_mm), close=None if close_mm is None else V._check_radius(close_mm),
                min_lung_ml=float(min_lung_ml), min_ratio=float(min_ratio), codes=codes, pixdim=None if pixdim is None else V._check_pixdim(pixdim),
                targs=_check_trachea_args(**{k: v for k, v in airway_kw.items() if k in _TRACHEA_KEYS}),
                gargs=_check_grow_args(**{k: v for k, v in airway_kw.items() if k in _GROW_KEYS}))


def _model_candidates(ct, model, threshold, batch_size, img_size, sec):
    """a lung U-Net's prediction over all slices through the front and the back of segment_volume: whole-frame boxes, no trim -> the thresholded mask on the device"""
    torch = V._torch()
    vol, _, _, z0, z1, S, x, info, R1, R2, has, s = V._prepare_segmentation(ct, None, None, img_size, (0, 1), lambda: int(getattr(model, "h", None) or model.base.h))
    sec.update(s)
    t0 = time.perf_counter()
    prob = torch.from_numpy(np.ascontiguousarray(model.predict(x, batch_size=batch_size), np.float32)).cuda()
    torch.cuda.synchronize(); sec["predict"] = time.perf_counter() - t0
    return V.unslice(V.paste_back(prob, R1, R2, S), threshold, tuple(vol.raw.shape), z0, z1)[0]


def lung_mask(ct, model=None, threshold=0.5, air_hu=AIR_HU, body_hu=BODY_HU, airways="auto", airway_dilate_mm=None, min_lung_ml=MIN_LUNG_ML, min_ratio=MIN_RATIO, fill=True,
              close_mm=None, orientation=None, out_path=None, return_device=False, batch_size=32, img_size=512, pixdim=None, src_shape=None, **airway_kw):
    """A CT -> LungMask: the lungs, without trachea and main bronchi, from nothing but the CT.  ct: a path, a NiftiVolume, an [X, Y, Z] array (pixdim=: its voxel size, 1 mm
    without) or a flat device tensor with src_shape=.
    Candidates.  model=None: threshold_volume(ct, hi=air_hu) inside body_mask(ct, body_hu) -- the air inside the patient.  model: a lung U-Net (only `predict` is used):
    its prediction over ALL slices through the front and the back of segment_volume (whole-frame boxes, trim (0, 1), img_size, batch_size; paste_back and unslice at
    `threshold`); the CT is then a host volume.  After that, in this order:
      1. Airways.  find_trachea on the candidates; grow_airways inside the candidate component that holds the seed (reconstruct); the airway dilated -- by one voxel of the
         26-neighbourhood, or with airway_dilate_mm by dilate_mm -- and removed from the candidates: an airway left in the mask joins the lungs high up.  airway_kw: the
         keywords of find_trachea and grow_airways.  airways="auto": without an orientation, with voxel axis 2 not an S / I axis, or without a trachea the step is skipped
         and airway_error says why; airways=True: no orientation is a ValueError before any device work and no trachea a LungMaskError; airways=False: the step does not
         run.  Superior and inferior come from the file's axis codes or orientation= (a code such as "LPS", or an affine); they are never guessed.
      2. Labelling (connectivity 1).
      3. Components under min_lung_ml are dropped; none left: LungMaskError.
      4. The largest component A is kept, the second, B, when count(B) >= min_ratio * count(A) in float64 (split_lungs' rule; ties to the lower label).
      5. fill_holes(per_slice=True) when fill: vessels and what the airway step cut out inside a lung.
      6. close_mm(radius) when given: bridges dense consolidation at the pleura, which a threshold misses.
    out_path: the mask as .nii / .nii.gz with the source's geometry.  The thresholds are conventional defaults, configurable and not clinically validated here."""
    a = _check_lung_mask_args(model, threshold, air_hu, body_hu, airways, airway_dilate_mm, min_lung_ml, min_ratio, fill, close_mm, orientation, batch_size, img_size, pixdim,
                              **airway_kw)
    _check_bool(return_device, "return_device")
    torch = V._torch()
    if out_path is not None and not isinstance(out_path, (str, os.PathLike)):
        raise ValueError(f"out_path is a path, not {out_path!r}")
    if model is not None and isinstance(ct, torch.Tensor):
        raise ValueError("model=: the slices are prepared from a host volume (a path, a NiftiVolume or an array), not a device tensor")
    sec = {}
    t_all = t0 = time.perf_counter()
    src = _ct_source(ct, src_shape, pixdim)
    sec["decode"] = time.perf_counter() - t0
    p = a["pixdim"] if a["pixdim"] is not None else V._check_pixdim(src.vol.pixdim if src.vol is not None else (1.0, 1.0, 1.0))
    codes = a["codes"]
    if codes is None and src.header is not None and src.vol.affine is not None:
        try:
            codes = src.vol.axcodes
        except nifti_min.NiftiFormatError:
            codes = None
    superior = superior_of(codes)
    if airways is True and superior is None:
        raise ValueError("airways=True needs to know which end of axis 2 is superior: the volume carries no orientation (or axis 2 is no S / I axis); pass "
                         "orientation='LPS' (or the volume's code) or an affine -- superior and inferior are not guessed")
    shape = src.shape
    if int(np.prod(shape)) == 0:
        raise LungMaskError("lung_mask: the volume has no voxel")
    t0 = time.perf_counter()
    dev = _ct_device(src)
    if model is None:
        cand, _ = threshold_device(dev, src.vargs, -np.inf, a["air_hu"], _body_device(dev, src, a["body_hu"]))
    else:
        cand = _model_candidates(src.vol, model, a["threshold"], int(batch_size), int(img_size), sec)
    torch.cuda.synchronize(); sec["candidates"] = time.perf_counter() - t0
    grown, why = None, None
    t0 = time.perf_counter()
    if airways is not False:
        if superior is None:
            why = ("the volume carries no orientation: superior and inferior are not guessed" if codes is None
                   else f"voxel axis 2 grows towards {codes[2]}, not S or I: the trachea is searched along axis 2 only")
        else:
            seed = _find_trachea_device(cand, shape, p, superior, a["targs"])
            if seed is None:
                if airways is True:
                    raise LungMaskError("lung_mask: no trachea found from the superior end (airways=True)")
                why = "no trachea found from the superior end"
            else:
                grown = _grow_device(dev, src, seed.mask, _reconstruct_device(cand, seed.mask, shape, 1), a["gargs"])
                wide = V.morph_device(grown.mask, shape, "dilate", 3)[0] if a["dilate"] is None else V.ball_device(grown.mask, shape, a["dilate"], p, True)[0]
                cand = _and_not(cand, wide, shape)
        torch.cuda.synchronize(); sec["airways"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    labels, n = V.label_device(cand, shape, 1)
    st = V.component_stats_device(labels, shape, n)
    vox = np.asarray(st["voxels"], np.int64)
    least = V.min_voxels_from_ml(a["min_lung_ml"], p)
    order = sorted((l for l in range(1, n + 1) if vox[l - 1] >= least), key=lambda l: (-int(vox[l - 1]), l))[:2]
    if not order:
        raise LungMaskError(f"lung_mask: none of the {n} components reaches min_lung_ml = {a['min_lung_ml']} ({least} voxels); the largest has {int(vox.max()) if n else 0}")
    kept = sorted(order[:1] + [l for l in order[1:] if float(vox[l - 1]) >= a["min_ratio"] * float(vox[order[0] - 1])])
    keep = np.zeros(n + 1, bool)
    keep[kept] = True
    mask, per_slice = V.filter_components(labels, keep, n, shape)
    table = V.table_from_stats(st, p)[np.asarray(kept) - 1]
    if a["fill"]:
        mask, per_slice = V.fill_holes_device(mask, shape, 1, per_slice=True)
    if a["close"] is not None:
        for dilate in (True, False):
            mask, per_slice = V.ball_device(mask, shape, a["close"], p, dilate)
    voxels = int(per_slice.cpu().numpy().sum())                      # (the slice counts every one of these steps leaves)
    torch.cuda.synchronize(); sec["components"] = time.perf_counter() - t0
    host = None
    if not return_device or out_path is not None:
        host = V._host_of(mask, np.uint8, shape)
    if out_path is not None:
        nifti_min.write(out_path, host, src.header, tuple(float(v) for v in p))
    if grown is not None:
        grown.mask = V._result(grown.mask, shape, bool(return_device))
    sec["total"] = time.perf_counter() - t_all
    return LungMask(mask=mask if return_device else host, shape=tuple(shape), pixdim=tuple(float(v) for v in p), lung_ml=voxels * float(np.prod(p)) / 1000.0, components=table,
                    airways=grown, airway_error=why, method="threshold" if model is None else "model", seconds=sec)

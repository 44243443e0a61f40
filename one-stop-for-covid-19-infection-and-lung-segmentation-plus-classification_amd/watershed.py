"""Marker-controlled watershed on the device (csrc/kernels_watershed.hip) and what it is for first: splitting lesions that touch.

  watershed(cost, markers, mask=None, connectivity=1, rule="max" | "sum")   region growing from labelled markers over a uint32 cost volume -> WatershedResult
  watershed_device / depth_cost_device                                       the same on device buffers
  split_lesions(mask, pixdim, seed_depth_mm=...)                             the parts of a lesion mask: cores of the distance transform grown back over the depth -> SplitLesions

The definition (include/unet_hip.h states it in full): rule "max" gives every voxel to the marker it reaches over the lowest pass -- the pass height H is the fixed
point of H[v] = min_n max(H[n], cost[v]), then the labels spread along the edges that realise H, nearest marker in steps first, lowest label among equally near ones,
so a plateau is divided and not swallowed; rule "sum" is the cost-weighted geodesic distance with the label of the nearest marker.  Both are greatest fixed points of
monotone operators: the result is unique, and the device, which relaxes 32 x 8 x 8 bricks in LDS and ping-pongs two key buffers, reproduces it -- and its sweep counts --
bit for bit on every run.  tests/watershed_oracle.py restates it twice (a whole-volume numpy iteration and priority queues).  No CPU fallback."""
from __future__ import annotations

import time

import numpy as np

from . import lungs as L
from . import volume as V

HEIGHT, LABEL, SUM = 0, 1, 2                                           # UNET_VOL_WATERSHED_HEIGHT / _LABEL / _SUM
COST_MAX = 2 ** 32 - 2
LABEL_MAX = 2 ** 24 - 1
DIST_MAX = 2 ** 40 - 2
SEED_DEPTH_MM = 3.0                                                    # split_lesions' default core depth: a conventional, configurable starting value, not clinically validated


class WatershedError(RuntimeError):
    """the sweeps ran out before the fixed point, or a "sum" distance passed 2^40 - 2"""


class WatershedResult:
    """labels: int32 [X, Y, Z], 0 where no marker reaches (numpy, Fortran order; return_device=True: flat device tensors); rule "max": height (uint32, the pass height,
    0xFFFFFFFF unreached) and steps (uint32, the steps from the marker along pass-height-realising paths); rule "sum": distance (uint64, 2^40 - 1 unreached);
    sweeps: the sweeps of every phase (the last one changed nothing), changed: their per-sweep counts; reached / unreached (mask voxels) / overflowed / invalid: the four
    counts; shape, rule, connectivity, seconds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"WatershedResult(rule={self.rule!r}, sweeps={self.sweeps}, reached={self.reached}, unreached={self.unreached})"


class SplitLesions:
    """labels: int32 [X, Y, Z] part labels 1..n, 0 outside the mask -- what component_table / lesion_shapes / label_pairs take; n; n_components: the connected components
    of the mask; parent: int32 [n], the component (1-based) every part lies in; n_cores: the parts grown from a core; sweeps: of the two watershed phases; table: the
    component_table of the parts (segment_volume fills it; else None); shape, seconds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"SplitLesions(n={self.n}, n_components={self.n_components})"


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_args(connectivity, rule, max_sweeps, chunk):
    connectivity = V._check_connectivity(connectivity)
    if rule not in ("max", "sum"):
        raise ValueError(f'rule is "max" (watershed) or "sum" (cost-weighted distance), not {rule!r}')
    if max_sweeps is not None and (not L._is_int(max_sweeps) or not 1 <= int(max_sweeps) < 2 ** 31):
        raise ValueError(f"max_sweeps is None or an integer >= 1, not {max_sweeps!r}")
    if not L._is_int(chunk) or not 1 <= int(chunk) <= 4096:
        raise ValueError(f"chunk is an integer in 1..4096, not {chunk!r}")
    return connectivity, rule, (None if max_sweeps is None else int(max_sweeps)), int(chunk)


def _host_volume(a, what):
    a = np.asarray(a)
    if a.ndim != 3:
        raise ValueError(f"{what} is a volume [X, Y, Z]; got {a.ndim} dimensions")
    if a.dtype.kind not in "biu":
        raise ValueError(f"{what} has an integer dtype, not {a.dtype}: float costs are not taken (quantise them first)")
    return a


def _to_device(cost, markers, mask, shape):
    """-> (cost int32 bits of the uint32, markers int32, mask uint8 or None, all flat device tensors in Fortran order, (X, Y, Z)); the refusals the host can make"""
    torch = V._torch()
    if isinstance(cost, torch.Tensor) or isinstance(markers, torch.Tensor):
        if not (isinstance(cost, torch.Tensor) and isinstance(markers, torch.Tensor)) or shape is None:
            raise ValueError("device inputs are flat Fortran-order buffers, cost and markers alike: pass shape=(X, Y, Z)")
        shape = tuple(int(v) for v in shape)
        N = int(np.prod(shape))
        if len(shape) != 3 or cost.dtype not in (torch.int32, torch.uint32) or markers.dtype != torch.int32 or not cost.is_cuda or not markers.is_cuda or cost.numel() != N or markers.numel() != N:
            raise ValueError(f"device cost (int32 holding the uint32 bits, or uint32) and markers (int32) are cuda tensors of prod(shape) = {N} elements")
        cost = cost.contiguous().reshape(-1).view(torch.int32)
        if N and bool((cost == -1).any().item()):
            raise ValueError(f"a cost lies outside 0 .. {COST_MAX}")
        mask_dev = None if mask is None else V._mask_to_device(mask, shape)[0]
        if mask_dev is not None and mask_dev.numel() != N:
            raise ValueError(f"the mask has {mask_dev.numel()} voxels, the volume {N}")
        return cost, markers.contiguous().reshape(-1), mask_dev, shape
    c, m = _host_volume(cost, "cost"), _host_volume(markers, "markers")
    if c.shape != m.shape:
        raise ValueError(f"cost is {c.shape}, markers {m.shape}")
    if c.size and (int(c.min()) < 0 or int(c.max()) > COST_MAX):
        raise ValueError(f"a cost lies outside 0 .. {COST_MAX}")
    if m.size and (int(m.min()) < 0 or int(m.max()) > LABEL_MAX):
        raise ValueError(f"a marker lies outside 0 .. {LABEL_MAX}")
    shape = tuple(int(v) for v in c.shape)
    mask_dev = None
    if mask is not None:
        mask_dev, ms = V._mask_to_device(mask, shape if isinstance(mask, torch.Tensor) else None)
        if tuple(ms) != shape:
            raise ValueError(f"the mask is {tuple(ms)}, the volume {shape}")
    flat = lambda a, dt: torch.from_numpy(np.asfortranarray(a.astype(dt, copy=False)).reshape(-1, order="F").view(np.int32)).cuda()
    return flat(c, np.uint32), flat(m, np.int32), mask_dev, shape


# ---- the entries ------------------------------------------------------------------------------------------------------------------------------------------------------
def _run_phase(lib, ctx, cost, markers, mask, dims, phase, done, connectivity, skip, limit, chunk, ws):
    """_begin, then _sweeps in calls of `chunk` until a sweep changes nothing -> changed int64 [sweeps]; WatershedError when `limit` sweeps did not reach the fixed point"""
    torch = V._torch()
    X, Y, Z = dims
    ctx.check(lib.unet_vol_watershed_begin(ctx.handle, V._ptr(cost), V._ptr(markers), V._ptr(mask), X, Y, Z, phase, done, V._ptr(ws), ws.numel(), V._stream()), "vol_watershed_begin")
    changed, first = [], 0
    while limit is None or first < limit:
        n = chunk if limit is None else min(chunk, limit - first)
        counts = torch.zeros(first + n, dtype=torch.int64, device="cuda")          # (the entry writes changed[first .. first + n - 1])
        ctx.check(lib.unet_vol_watershed_sweeps(ctx.handle, V._ptr(cost), V._ptr(markers), V._ptr(mask), X, Y, Z, first, n, phase, connectivity, 1 if skip else 0,
                                                V._ptr(counts), V._ptr(ws), ws.numel(), V._stream()), "vol_watershed_sweeps")
        got = counts[first:first + n].cpu().numpy()
        still = np.flatnonzero(got == 0)
        if still.size:
            changed.extend(int(v) for v in got[:int(still[0]) + 1])
            return np.asarray(changed, np.int64), first + n
        changed.extend(int(v) for v in got)
        first += n
    raise WatershedError(f"max_sweeps = {limit} sweeps of phase {('HEIGHT', 'LABEL', 'SUM')[phase]} did not reach the fixed point (the last one lowered {changed[-1]} voxels)")


def watershed_device(cost_dev, markers_dev, mask_dev, shape, connectivity=1, rule="max", max_sweeps=None, chunk=16, skip=True):
    """The watershed on flat device buffers (cost: int32 holding the uint32 bits; markers: int32; mask_dev: uint8 or None) -> dict of device tensors labels (int32),
    height / steps (int32 holding uint32 bits) or distance (int64 holding uint64 bits), and changed (a tuple of int64 numpy arrays, one per phase), counts (reached,
    unreached, overflowed, invalid).  Only the per-sweep counts come to the host between the calls.  It returns only at the fixed point (WatershedError otherwise)."""
    connectivity, rule, limit, chunk = _check_args(connectivity, rule, max_sweeps, chunk)
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    N = X * Y * Z
    out = dict(labels=torch.zeros(N, dtype=torch.int32, device="cuda"))
    if N == 0:
        out.update(changed=(), counts=(0, 0, 0, 0))
        out.update(dict(height=out["labels"].clone(), steps=out["labels"].clone()) if rule == "max" else dict(distance=torch.zeros(0, dtype=torch.int64, device="cuda")))
        return out
    ws = torch.empty(max(int(lib.unet_vol_watershed_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    dims = (X, Y, Z)
    if rule == "max":
        ch_h, ran_h = _run_phase(lib, ctx, cost_dev, markers_dev, mask_dev, dims, HEIGHT, 0, connectivity, skip, limit, chunk, ws)
        ch_l, ran_l = _run_phase(lib, ctx, cost_dev, markers_dev, mask_dev, dims, LABEL, ran_h, connectivity, skip, limit, chunk, ws)
        out.update(height=torch.empty(N, dtype=torch.int32, device="cuda"), steps=torch.empty(N, dtype=torch.int32, device="cuda"), changed=(ch_h, ch_l))
        ctx.check(lib.unet_vol_watershed_end(ctx.handle, V._ptr(mask_dev), X, Y, Z, LABEL, ran_l, connectivity, V._ptr(out["labels"]), V._ptr(out["height"]), V._ptr(out["steps"]),
                                             None, V._ptr(counts), V._ptr(ws), ws.numel(), V._stream()), "vol_watershed_end")
    else:
        ch_s, ran_s = _run_phase(lib, ctx, cost_dev, markers_dev, mask_dev, dims, SUM, 0, connectivity, skip, limit, chunk, ws)
        out.update(distance=torch.empty(N, dtype=torch.int64, device="cuda"), changed=(ch_s,))
        ctx.check(lib.unet_vol_watershed_end(ctx.handle, V._ptr(mask_dev), X, Y, Z, SUM, ran_s, connectivity, V._ptr(out["labels"]), None, None, V._ptr(out["distance"]),
                                             V._ptr(counts), V._ptr(ws), ws.numel(), V._stream()), "vol_watershed_end")
    out["counts"] = tuple(int(v) for v in counts.cpu().numpy())
    return out


def depth_cost_device(d2_dev, mask_dev, shape, d2max, quantum):
    """unet_vol_depth_cost: cost = uint32(floor((d2max - d2) / quantum)) inside the mask, 0 outside, clipped to 2^32 - 2 -> int32 device tensor holding the uint32 bits"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = (int(v) for v in shape)
    V._check_volume_dims((X, Y, Z))
    cost = torch.empty(X * Y * Z, dtype=torch.int32, device="cuda")
    ctx.check(lib.unet_vol_depth_cost(ctx.handle, V._ptr(d2_dev), V._ptr(mask_dev), X, Y, Z, float(d2max), float(quantum), V._ptr(cost), V._stream()), "vol_depth_cost")
    return cost


def watershed(cost, markers, mask=None, connectivity=1, rule="max", return_device=False, shape=None, max_sweeps=None, chunk=16, allow_overflow=False, skip=True):
    """Region growing from the labelled `markers` (int, 1 .. 2^24 - 1; 0 none) over `cost` (an integer volume, 0 .. 2^32 - 2) inside `mask` (None: everywhere) ->
    WatershedResult.  rule="max": the watershed -- a voxel goes to the marker it reaches over the lowest pass, nearest in steps, then lowest label; rule="sum": the marker
    of the smallest summed cost (the marker's own cost not counted), the lowest label among equals.  Neighbours: generate_binary_structure(3, connectivity).  Refused
    (ValueError): float costs, costs outside 0 .. 2^32 - 2, markers outside 0 .. 2^24 - 1 (on device inputs: found by the kernel's count, after the run).  A "sum" distance
    beyond 2^40 - 2 raises WatershedError unless allow_overflow=True (the voxels then stay unreached and res.overflowed counts those beside a reached one).  max_sweeps:
    per phase; WatershedError when they run out -- a state that is not the fixed point is never returned.  chunk: sweeps per call; the per-sweep counts come to the host
    between calls.  skip=False visits every brick in every sweep (the same result; for measuring)."""
    _check_args(connectivity, rule, max_sweeps, chunk)
    L._check_bool(return_device, "return_device"); L._check_bool(allow_overflow, "allow_overflow"); L._check_bool(skip, "skip")
    cost_dev, markers_dev, mask_dev, shp = _to_device(cost, markers, mask, shape)
    torch = V._torch()
    t0 = time.perf_counter()
    out = watershed_device(cost_dev, markers_dev, mask_dev, shp, connectivity, rule, max_sweeps, chunk, skip)
    torch.cuda.synchronize()
    sec = {"watershed": time.perf_counter() - t0}
    reached, unreached, overflowed, invalid = out["counts"]
    if invalid:
        raise ValueError(f"{invalid} markers lie outside 0 .. {LABEL_MAX}")
    if overflowed and not allow_overflow:
        raise WatershedError(f"{overflowed} voxels lie beside a reached voxel but beyond the largest distance 2^40 - 2 (allow_overflow=True leaves them unreached)")
    host = lambda t, dt: t if return_device else t.cpu().numpy().view(dt).reshape(shp, order="F")
    fields = dict(labels=host(out["labels"], np.int32), height=None, steps=None, distance=None)
    if rule == "max":
        fields.update(height=host(out["height"], np.uint32), steps=host(out["steps"], np.uint32))
    else:
        fields.update(distance=host(out["distance"], np.uint64))
    return WatershedResult(sweeps=tuple(len(c) for c in out["changed"]), changed=out["changed"], reached=reached, unreached=unreached, overflowed=overflowed, invalid=invalid,
                           rule=rule, connectivity=int(connectivity), shape=shp, seconds=sec, **fields)


# ---- splitting lesions --------------------------------------------------------------------------------------------------------------------------------------------------
def number_markers(core_size, core_owner, n_components, min_seed_voxels=1):
    """core_size / core_owner: int [n_cores] (voxels; the component, 1-based, a core lies in) -> (core_number int32 [n_cores + 1], component_number int32 [n_components + 1],
    parent int32 [n]): a core is kept when it has at least min_seed_voxels voxels or is its component's only core; the kept cores are numbered first, in label order; a
    component without a kept core is wholly its own marker, numbered after the cores in component order.  0: no marker."""
    core_size, core_owner = np.asarray(core_size, np.int64), np.asarray(core_owner, np.int64)
    per_comp = np.bincount(core_owner, minlength=n_components + 1)
    keep = (core_size >= int(min_seed_voxels)) | (per_comp[core_owner] == 1)
    core_number = np.zeros(len(core_size) + 1, np.int32)
    core_number[1:][keep] = np.arange(1, int(keep.sum()) + 1)
    has = np.zeros(n_components + 1, bool)
    has[core_owner[keep]] = True
    bare = np.flatnonzero(~has[1:]) + 1
    comp_number = np.zeros(n_components + 1, np.int32)
    comp_number[bare] = int(keep.sum()) + np.arange(1, len(bare) + 1)
    return core_number, comp_number, np.concatenate([core_owner[keep], bare]).astype(np.int32)


def _check_split_args(pixdim, seed_depth_mm, connectivity, min_seed_voxels, quantum_mm2):
    p = V._check_pixdim(pixdim)
    V._check_connectivity(connectivity)
    if not L._is_number(seed_depth_mm) or not (np.isfinite(float(seed_depth_mm)) and float(seed_depth_mm) > 0.0):
        raise ValueError(f"seed_depth_mm is a positive finite number, not {seed_depth_mm!r}")
    if not L._is_int(min_seed_voxels) or int(min_seed_voxels) < 1:
        raise ValueError(f"min_seed_voxels is an integer >= 1, not {min_seed_voxels!r}")
    if quantum_mm2 is not None and (not L._is_number(quantum_mm2) or not (np.isfinite(float(quantum_mm2)) and float(quantum_mm2) > 0.0)):
        raise ValueError(f"quantum_mm2 is None or a positive finite number, not {quantum_mm2!r}")
    return p, float((p * p).min()) / 4.0 if quantum_mm2 is None else float(quantum_mm2)


def split_inputs_device(mask_dev, shape, pixdim=(1, 1, 1), seed_depth_mm=SEED_DEPTH_MM, connectivity=1, min_seed_voxels=1, quantum_mm2=None):
    """what split_lesions hands the watershed, for a mask with at least one voxel -> (cost, markers: flat int32 device tensors, n_components, n_cores, parent)"""
    p, quantum = _check_split_args(pixdim, seed_depth_mm, connectivity, min_seed_voxels, quantum_mm2)
    torch = V._torch()
    inside = mask_dev != 0
    comp, n_comp = V.label_device(mask_dev, shape, connectivity)
    d2 = V.edt_sq_device(mask_dev, shape, p, features_nonzero=False)          # the squared depth: to the nearest voxel outside the mask (+inf when there is none)
    core_mask = (inside & (d2 >= float(seed_depth_mm) ** 2)).to(torch.uint8)
    cores, n_cores = V.label_device(core_mask, shape, connectivity)
    in_core = cores > 0
    size = torch.bincount(cores[in_core].long(), minlength=n_cores + 1)[1:].cpu().numpy()
    owner = torch.zeros(n_cores + 1, dtype=torch.int32, device="cuda")
    owner[cores[in_core].long()] = comp[in_core]                                # (every voxel of a core writes the same component)
    core_number, comp_number, parent = number_markers(size, owner[1:].cpu().numpy(), n_comp, min_seed_voxels)
    if len(parent) > LABEL_MAX:
        raise ValueError(f"{len(parent)} parts are more than the {LABEL_MAX} labels a marker can carry")
    from_core = torch.from_numpy(core_number).cuda()[cores.long()]
    markers = torch.where(from_core > 0, from_core, torch.from_numpy(comp_number).cuda()[comp.long()]).to(torch.int32).contiguous()
    finite = inside & torch.isfinite(d2)
    d2max = float(torch.where(finite, d2, torch.zeros_like(d2)).max().item())
    return depth_cost_device(d2, mask_dev, shape, d2max, quantum), markers, n_comp, int((core_number > 0).sum()), parent


def split_lesions_device(mask_dev, shape, pixdim=(1, 1, 1), seed_depth_mm=SEED_DEPTH_MM, connectivity=1, min_seed_voxels=1, quantum_mm2=None):
    """split_lesions on a flat uint8 device mask -> SplitLesions with labels on the device"""
    _check_split_args(pixdim, seed_depth_mm, connectivity, min_seed_voxels, quantum_mm2)
    torch = V._torch()
    shape = tuple(int(v) for v in shape)
    t0 = time.perf_counter()
    N = int(np.prod(shape))
    if N == 0 or not bool(mask_dev.any().item()):
        return SplitLesions(labels=torch.zeros(N, dtype=torch.int32, device="cuda"), n=0, n_components=0, n_cores=0, parent=np.zeros(0, np.int32), sweeps=(0, 0), table=None,
                            shape=shape, seconds={"split": time.perf_counter() - t0})
    cost, markers, n_comp, n_cores, parent = split_inputs_device(mask_dev, shape, pixdim, seed_depth_mm, connectivity, min_seed_voxels, quantum_mm2)
    out = watershed_device(cost, markers, mask_dev, shape, connectivity, "max")
    reached, unreached, _, invalid = out["counts"]
    assert unreached == 0 and invalid == 0, (unreached, invalid)              # every component holds a marker
    torch.cuda.synchronize()
    return SplitLesions(labels=out["labels"], n=len(parent), n_components=n_comp, n_cores=n_cores, parent=parent,
                        sweeps=tuple(len(c) for c in out["changed"]), table=None, shape=shape, seconds={"split": time.perf_counter() - t0})


def split_lesions(mask, pixdim=(1, 1, 1), seed_depth_mm=SEED_DEPTH_MM, connectivity=1, min_seed_voxels=1, quantum_mm2=None, return_device=False, shape=None):
    """The parts of mask != 0 -> SplitLesions: lesions that touch over a bridge come apart where the bridge is narrowest.  The mask's components are found; d2 is the exact
    squared depth (mm^2, the distance to the nearest voxel outside the mask); the cores are the components of d2 >= seed_depth_mm^2, those under min_seed_voxels voxels
    dropped unless a core is its component's only one; the markers are the kept cores, numbered first in label order, and every component without a core, wholly its own
    marker, numbered after them in component order; the cost is floor((max d2 - d2) / quantum) with quantum_mm2 = a quarter of the smallest squared spacing by default;
    the watershed (rule "max") grows the markers back inside the mask.  Every mask voxel gets a part, nothing outside does; the parts of one component partition it.  The
    labels go where label_volume's go: component_table, lesion_shapes, tracking.label_pairs.  seed_depth_mm: a deeper core splits less; the default is a conventional,
    configurable starting value, not clinically validated."""
    _check_split_args(pixdim, seed_depth_mm, connectivity, min_seed_voxels, quantum_mm2)
    L._check_bool(return_device, "return_device")
    V._check_mask_host(mask, shape)
    dev, shp = V._mask_to_device(mask, shape)
    res = split_lesions_device(dev, shp, pixdim, seed_depth_mm, connectivity, min_seed_voxels, quantum_mm2)
    res.labels = V._result(res.labels, shp, bool(return_device))
    return res

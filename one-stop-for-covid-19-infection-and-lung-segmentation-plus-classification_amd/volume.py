"""A CT scan in, a mask volume out: the first half of the reference's read_nii / read_nii_demo (T1:281-297, 310-337; the same text in T3:284-300),
the dataset loop around it (T1:390-393, 421-429) and the way back from a predicted 224 x 224 map of the two fused lung crops to the patient's volume.

    load_volume(path_or_array, kind)      kind = "demo" | "lungs" | "cts" | "infections": the four uses of read_nii / read_nii_demo
    build_dataset(rows)                   rows of (ct, lung_mask, infection_mask) -> cts, infections for the runners' data= argument
    segment_volume(ct, model, ...)        -> VolumeSegmentation: mask volume in the CT's geometry, infected volume in ml, optional .nii(.gz) file
    label_volume(mask, connectivity)      -> (labels, n): connected components on the device, numbered as skimage.measure.label numbers them
    component_table(labels, n, pixdim)    -> one row per component: voxels, ml, bounding box, centroid
    remove_small / keep_largest(mask)     -> the mask without its small components / with its k largest only
    surface(mask, connectivity)           -> the mask's surface voxels (mask ^ binary_erosion)
    distance_transform(mask, pixdim)      -> float64 distance of every foreground voxel to the background, in mm (scipy's distance_transform_edt with sampling=)
    score_volume(pred, truth, pixdim)     -> VolumeScore: Dice / IoU / volume error, Hausdorff / HD95 / surface distances in mm, lesion-wise detection
    binary_dilation / _erosion / _opening / _closing(mask, connectivity, iterations, border_value, per_slice)     scipy.ndimage's, on the device
    dilate_mm / erode_mm / open_mm / close_mm(mask, radius_mm, pixdim)     the same by a ball of radius_mm millimetres, from the exact distance transform
    fill_holes(mask, connectivity, per_slice)     scipy.ndimage.binary_fill_holes
    postprocess(mask, steps, pixdim)      a list of (name, kwargs) cleaning steps applied in order on the device; segment_volume(postprocess=steps) runs it
    segment_volume_ensemble(ct, models, tta, combine, weights)     several models x the square's symmetries (TTA) on one CT: mean / voted mask, agreement map and statistics
    vote_volume(masks, rule) / dihedral(x, code) / models_from_weights(paths, input_size)     the pieces: up to 32 masks voted on the device, one symmetry, fold files -> models
    intensity_stats(ct, mask | labels, n, region, edges)     -> IntensityStats: what the CT holds under a mask or per lesion -- voxels per HU band (HU_BANDS), min / max,
                                          mean / std, percentiles, per slice; segment_volume(density=True) fills res.density / res.lung_density with it
    split_lungs(lung_mask, orientation)   -> LungSides: the lung mask told into the patient's left (1) and right (2) lung from the file's orientation (nifti_min: sform /
                                          qform); lungs that touch are separated by eroding until two seeds remain, every voxel then goes to the nearer seed
    lung_burden(infection, sides)         -> LungBurden: lung / infected volume and fraction per lung, every lesion's side, per slice; segment_volume(per_lung=True)
                                          fills res.per_lung with it
    render_planes(ct, planes, layers)     -> RenderedSheet: axial / coronal / sagittal planes and maximum / minimum projections of the CT, windowed and colour-mapped
                                          (WINDOWS, BONE), with up to four label layers blended and outlined on top (Layer), drawn on the device into one RGB sheet and
                                          written as a PNG (png_min); segment_volume(render=True) fills res.sheet with the key slices (key_slices) and a coronal projection
    project_volume(ct, axis, slab, mode)  -> the maximum / minimum of the CT and the largest label of every layer along one axis
    resample_volume(ct, spacing | shape | like | grid)     -> ResampledVolume: the CT on another grid (trilinear or nearest, on the device); resample_mask / resample_labels
                                          for masks and label volumes; Grid, resample_target, resample_matrix: the grids and the matrices between them
    reorient_volume(vol, "RAS")           -> the volume stored under other axis codes (a signed axis permutation, the stored elements kept)
    change_between(mask_a, grid_a, mask_b, grid_b)     -> VolumeChange: persistent / new / resolved voxels and millilitres of two masks on two grids, and their Dice
    extract_surface(x, iso | select)      -> SurfaceMesh: the surface of a mask, a label volume or a scalar volume as an indexed triangle mesh (marching tetrahedra on the
                                          device), its area in mm^2, enclosed volume in ml, Euler characteristic; .measure() per group, .write() as STL / PLY / OBJ
                                          (mesh_min); lesion_shapes(labels, n): area, volume, sphericity per lesion; segment_volume(mesh=True) fills res.mesh
    register_volumes(fixed, moving)       -> Registration: the rigid transform (RigidTransform) that takes a baseline CT's world onto a follow-up's, found by maximising
                                          the mutual information of their joint histogram (joint_histogram, mutual_information) on the device; Registration.resample
                                          and change_between(transform=) then compare the two scans in one frame

The voxels are uploaded once as stored (nifti_min reads the file); decode, np.rot90, the slice trim, cv2.resize(float64, INTER_AREA) and the min-max run
in unet_vol_slices_f64, CLAHE / crop / fuse / resize in the uint8 kernels of preprocess.py on device pointers: between the upload and the returned batch
only the lung rectangles live on the host.  Like the rest of the product there is no CPU fallback.

Two ways to pair a CT slice with its lung rectangles (`box_indexing`):
  "reference"  T1:347-353 as written: the rectangle list was shortened by every skipped (uniform) lung slice but is indexed by raw slice number, so every
               slice after a skipped one takes its neighbour's boxes and the last slices find none and fall through uncropped
  "slice"      rectangles keyed by slice number; only the slices whose lung mask was uniform fall through
A slice that falls through is not cropped: here its whole frame goes through the same uint8 resize to new_dim (no CLAHE: T1:348 sits inside the `if`).
The reference instead carries the float [0, 1] frame to T1:520's np.uint8 cast, which leaves a near-black image; such slices are listed in the
returned info so that a caller can drop them.
"""
from __future__ import annotations

import os
import time
import warnings

import numpy as np

from . import _lib, mesh_min, nifti_min, png_min
from . import preprocess as PRE

KINDS = ("demo", "lungs", "cts", "infections")
BOX_INDEXING = ("reference", "slice")


def _torch():
    import torch
    return torch


def trim_range(n_slices, trim=(0.2, 0.8)):
    """array[:, :, round(slices*0.2):round(slices*0.8)] (T1:288-289): Python's round of the float product."""
    z0, z1 = round(n_slices * trim[0]), round(n_slices * trim[1])
    if not 0 <= z0 < z1 <= n_slices:
        raise ValueError(f"trim {trim} keeps no slice of {n_slices}")
    return z0, z1


def box_plan(n_slices, kept, box_indexing="reference"):
    """For kept-range slices 0..n_slices-1: the index into the rectangle list each one uses, or -1 where it falls through.  `kept`: the slice numbers
    the rectangle list was built from (the non-uniform lung slices, in order)."""
    if box_indexing not in BOX_INDEXING:
        raise ValueError(f"box_indexing must be one of {BOX_INDEXING}, not {box_indexing!r}")
    kept = [int(k) for k in kept]
    plan = np.full(n_slices, -1, np.int64)
    if box_indexing == "reference":                                 # T1:347 `img_no < len(all_points1)`, T1:352 `all_points1[img_no]`
        m = min(n_slices, len(kept))
        plan[:m] = np.arange(m)
    else:
        for k, s in enumerate(kept):
            if 0 <= s < n_slices:
                plan[s] = k
    return plan


def whole_frame_rects(n, size):
    """The boxes used when there is no lung mask: the left and the right half of the frame."""
    half = size // 2
    r1 = np.tile(np.array([0, 0, half, size], np.int32), (n, 1))
    r2 = np.tile(np.array([half, 0, size - half, size], np.int32), (n, 1))
    return r1, r2


def drop_constant(cts, infections):
    """T1:421-429: the slices whose infection mask holds a single value are deleted from both lists.  -> (cts, infections, dropped indices)"""
    keep, dropped = [], []
    for i in range(len(infections)):
        (dropped if np.unique(np.asarray(infections[i])).size == 1 else keep).append(i)
    return [cts[i] for i in keep], [infections[i] for i in keep], dropped


def _source(path_or_array):
    """-> nifti_min.NiftiVolume for a path, a NiftiVolume, or a bare [X, Y, Z] array (taken as get_fdata's result: not scaled, 1 mm voxels)."""
    if isinstance(path_or_array, nifti_min.NiftiVolume):
        return path_or_array
    if isinstance(path_or_array, (str, os.PathLike)):
        return nifti_min.read(path_or_array)
    a = np.asarray(path_or_array)
    if a.ndim != 3:
        raise ValueError(f"a volume is [X, Y, Z]; got {a.ndim} dimensions")
    if a.dtype.str[1:] not in ("u1", "i1", "i2", "u2", "i4", "u4", "f4", "f8"):
        a = a.astype(np.float64)
    a = np.asfortranarray(a.astype(a.dtype.newbyteorder("="), copy=False))
    return nifti_min.NiftiVolume(a, 0.0, 0.0, (1.0, 1.0, 1.0), nifti_min.default_header(a.shape), "<")


def _ctx():
    torch = _torch()
    if not torch.cuda.is_available():
        raise _lib.UNetHipError("volume: no GPU visible to torch; the kernels have no CPU fallback")
    return _lib.load(), _lib.Context.get(torch.cuda.current_device())


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def upload(vol):
    """The raw voxels of a NiftiVolume as one device byte buffer in Fortran order."""
    torch = _torch()
    raw = np.asfortranarray(vol.raw)
    flat = raw.reshape(-1, order="F").view(np.uint8)
    return torch.from_numpy(flat).cuda()


def slices_f64(vol, dev, z0, z1, size, want=("f32",)):
    """unet_vol_slices_f64 on an uploaded volume: dict of device tensors for the wanted outputs ("f32", "u8", "lung") + "uniform" [n] int32 and "minmax" [n, 2]."""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = vol.raw.shape
    n = z1 - z0
    code = {v: k for k, v in nifti_min.DTYPES.items()}[vol.raw.dtype.str[1:]]
    sc = vol.scaling
    out = {"uniform": torch.empty(n, dtype=torch.int32, device="cuda"), "minmax": torch.empty((n, 2), dtype=torch.float64, device="cuda")}
    if "f32" in want:
        out["f32"] = torch.empty((n, size, size), dtype=torch.float32, device="cuda")
    if "u8" in want:
        out["u8"] = torch.empty((n, size, size), dtype=torch.uint8, device="cuda")
    if "lung" in want:
        out["lung"] = torch.empty((n, size, size), dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(lib.unet_vol_slices_ws_bytes(n, size), 16), dtype=torch.uint8, device="cuda")
    ptr = lambda k: out[k].data_ptr() if k in out else None
    ctx.check(lib.unet_vol_slices_f64(ctx.handle, dev.data_ptr(), code, X, Y, Z, 1 if sc else 0, sc[0] if sc else 1.0, sc[1] if sc else 0.0, z0, z1, size,
                                      ptr("f32"), ptr("u8"), ptr("lung"), out["uniform"].data_ptr(), out["minmax"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "vol_slices_f64")
    out["_ws"] = ws                                                 # (the float64 stage, for the tests; freed with the dict)
    return out


def _flat_slices(mm):
    """slice indices whose resized image has max == min (numpy's 0/0: NaN image, 0 in uint8) -- reported, not repaired"""
    return [int(i) for i in np.nonzero(mm[:, 0] == mm[:, 1])[0]]


def _resize_dev(x, rects, out, x0, dw, interp):
    lib, ctx = _ctx()
    PRE._resize_into(lib, ctx, x, rects, out, x0, dw, interp)


def _chain_u8(u8, boxed_u8, rects1, rects2, plan, new_dim):
    """crop + INTER_AREA to 125 x 250 + fuse for the slices with boxes (from boxed_u8), the whole frame of u8 for those that fall through, INTER_LINEAR to
    new_dim, / 255: [n, new_dim, new_dim, 1] float32 on the device (+ per-slice "the uint8 image before the last resize holds one value")."""
    torch = _torch(); lib, ctx = _ctx()
    n = u8.shape[0]
    boxed = np.nonzero(plan >= 0)[0]; fell = np.nonzero(plan < 0)[0]
    if new_dim is None and len(fell) and len(boxed):
        raise ValueError("new_dim=None: slices that fall through stay at the frame size and cannot share an array with the 250 x 250 fused ones; pass new_dim")
    constant = torch.zeros(n, dtype=torch.bool, device="cuda")
    side = int(new_dim) if new_dim is not None else (250 if len(boxed) else u8.shape[1])
    out_u8 = torch.empty((n, side, side), dtype=torch.uint8, device="cuda")
    if len(boxed):
        idx = torch.from_numpy(boxed).cuda()
        x = boxed_u8 if len(boxed) == n else boxed_u8.index_select(0, idx).contiguous()
        r1 = np.asarray(rects1, np.int32).reshape(-1, 4)[plan[boxed]]; r2 = np.asarray(rects2, np.int32).reshape(-1, 4)[plan[boxed]]
        fused = torch.empty((len(boxed), 250, 250), dtype=torch.uint8, device="cuda")
        _resize_dev(x, r1, fused, 0, 125, PRE.INTER_AREA)
        _resize_dev(x, r2, fused, 125, 125, PRE.INTER_AREA)
        constant[idx] = fused.flatten(1).amax(1) == fused.flatten(1).amin(1)
        if new_dim is None:
            res = fused
        else:
            res = torch.empty((len(boxed), side, side), dtype=torch.uint8, device="cuda")
            _resize_dev(fused, None, res, 0, side, PRE.INTER_LINEAR)
        if len(boxed) == n:
            out_u8 = res
        else:
            out_u8[idx] = res
    if len(fell):
        idx = torch.from_numpy(fell).cuda()
        x = u8 if len(fell) == n else u8.index_select(0, idx).contiguous()
        constant[idx] = x.flatten(1).amax(1) == x.flatten(1).amin(1)
        if new_dim is None:
            res = x
        else:
            res = torch.empty((len(fell), side, side), dtype=torch.uint8, device="cuda")
            _resize_dev(x, None, res, 0, side, PRE.INTER_LINEAR)
        if len(fell) == n:
            out_u8 = res
        else:
            out_u8[idx] = res
    out = torch.empty(out_u8.shape, dtype=torch.float32, device="cuda")
    ctx.check(lib.unet_pre_u8_to_unit(ctx.handle, out_u8.data_ptr(), out.data_ptr(), out_u8.numel(), _stream()), "pre_u8_to_unit")
    return out[..., None], constant


def load_volume(path_or_array, kind, img_size=512, trim=(0.2, 0.8), rects=None, box_indexing="reference", new_dim=None, return_info=False):
    """read_nii_demo(filepath, data) / read_nii(filepath, data, string) for one file (T1:281-297, 310-376); everything stays on the device.

    kind "demo"        -> float32 [n, img_size, img_size] tensor: the min-max normalised slices
         "lungs"       -> (rects1, rects2, kept_slice_numbers): `all_points1`, `all_points2` (int32 [k, 4] (x, y, w, h)) of the non-uniform slices (T1:333, 339-345);
                          the contour search is the library's host code (unet_pre_contours_u8), so the uint8 lung images make the one trip to the host
         "cts"         -> float32 [n, d, d, 1] tensor: min-max -> CLAHE -> crop / fuse with `rects` -> INTER_LINEAR to new_dim -> / 255
         "infections"  -> the same chain without CLAHE
    rects: what a "lungs" call returned (None: no cropping at all, every slice's whole frame).  Slice numbers count from the first kept slice.
    return_info=True adds a dict: z0, z1, shape, pixdim, fell_through, flat (slices with max == min: NaN / 0, as numpy gives), constant (cts / infections:
    slices whose uint8 image before the last resize holds a single value -- the T1:423 test), seconds (decode / upload / device)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    torch = _torch()
    t0 = time.perf_counter()
    vol = _source(path_or_array)
    t1 = time.perf_counter()
    X, Y, Z = vol.raw.shape
    z0, z1 = trim_range(Z, trim)
    n = z1 - z0
    S = int(img_size)
    dev = upload(vol)
    info = {"z0": z0, "z1": z1, "shape": (X, Y, Z), "pixdim": vol.pixdim, "header": vol.header, "fell_through": [], "flat": [], "constant": []}
    info["seconds"] = {"decode": t1 - t0}
    want = {"demo": ("f32",), "lungs": ("lung",), "cts": ("u8",), "infections": ("u8",)}[kind]
    st = slices_f64(vol, dev, z0, z1, S, want)
    if kind == "demo":
        result = st["f32"]
        info["flat"] = _flat_slices(st["minmax"].cpu().numpy())
    elif kind == "lungs":
        uniform = st["uniform"].cpu().numpy()
        kept = [int(i) for i in np.nonzero(uniform == 0)[0]]
        if kept:
            lung = (st["lung"] if len(kept) == n else st["lung"][torch.from_numpy(np.asarray(kept)).cuda()]).cpu().numpy()
            r1, r2 = PRE.lung_rects(lung)
        else:
            r1, r2 = np.zeros((0, 4), np.int32), np.zeros((0, 4), np.int32)
        info["uniform"] = [int(i) for i in np.nonzero(uniform)[0]]
        result = (r1, r2, kept)
    else:
        if rects is None:
            plan = np.full(n, -1, np.int64); r1 = r2 = None
        else:
            r1, r2, kept = rects
            plan = box_plan(n, kept, box_indexing)
        u8 = st["u8"]
        boxed_u8 = PRE._clahe_device(u8, 3.0, (8, 8)) if (kind == "cts" and (plan >= 0).any()) else u8
        result, constant = _chain_u8(u8, boxed_u8, r1, r2, plan, new_dim)
        mm = st["minmax"].cpu().numpy()                             # (16 bytes per slice: the report, not image data)
        info["flat"] = _flat_slices(mm)
        info["fell_through"] = [int(i) for i in np.nonzero(plan < 0)[0]] if rects is not None else []
        info["constant"] = [int(i) for i in np.nonzero(constant.cpu().numpy())[0]]
    if info["flat"]:
        warnings.warn(f"load_volume({kind!r}): slices {info['flat']} (of the kept range) are constant after the resize: (img - min)/(max - min) is 0/0 there "
                      "(NaN in the float image, 0 in uint8, as numpy gives)", RuntimeWarning, stacklevel=2)
    return (result, info) if return_info else result


def build_dataset(rows, img_size=512, new_dim=224, trim=(0.2, 0.8), box_indexing="reference", return_info=False):
    """The T1:390-393 loop over (ct_scan, lung_mask, infection_mask) rows (paths or [X, Y, Z] arrays) -- lungs first, for the rectangles, then cts and
    infections with them -- and the empty-mask filter of T1:421-429.  -> (cts, infections) float32 [N, new_dim, new_dim, 1] numpy arrays, the `data=` argument
    of the runners (holdout_runner_unet_infection_segmentation(data=build_dataset(rows)))."""
    torch = _torch()
    cts, infs, report = [], [], []
    for ct, lung, inf in rows:
        rects = load_volume(lung, "lungs", img_size, trim)
        c, ci = load_volume(ct, "cts", img_size, trim, rects, box_indexing, new_dim, return_info=True)
        with warnings.catch_warnings():                              # an empty infection mask is expected here: T1:421-429 drops it below
            warnings.simplefilter("ignore", RuntimeWarning)
            m, mi = load_volume(inf, "infections", img_size, trim, rects, box_indexing, new_dim, return_info=True)
        if c.shape != m.shape:
            raise ValueError(f"the CT gives {tuple(c.shape)} slices but its infection mask {tuple(m.shape)}")
        keep = np.ones(c.shape[0], bool); keep[mi["constant"]] = False          # T1:423: np.unique(infections[i]).size == 1
        k = torch.from_numpy(np.nonzero(keep)[0]).cuda()
        cts.append(c.index_select(0, k)); infs.append(m.index_select(0, k))
        report.append({"kept": int(keep.sum()), "dropped": mi["constant"], "fell_through": ci["fell_through"], "flat": sorted(set(ci["flat"]) | set(mi["flat"]))})
    x, y = torch.cat(cts).cpu().numpy(), torch.cat(infs).cpu().numpy()
    return (x, y, report) if return_info else (x, y)


class VolumeSegmentation:
    """mask: uint8 [X, Y, Z] in the CT's own geometry (numpy, Fortran order); voxel_ml; counts / ml_per_slice [Z] (0 on the trimmed slices); total_ml;
    lung_ml and infected_share when a lung mask was given; fell_through / flat: kept-range slice numbers; z0, z1; seconds: where the time went;
    lesions / n_lesions / removed_ml: the component table of the mask, its length and the volume a min_lesion_ml filter removed (None when not asked for);
    score: the VolumeScore of the final mask against the `truth` given to segment_volume (None without one);
    postprocess_ml: the volume the `postprocess` steps added to the mask (negative: removed; None without steps);
    density / lung_density: the IntensityStats of the CT under the final mask (per lesion when the lesion table was computed) and under the lung mask (None unless
    segment_volume was given density=);
    per_lung / per_lung_error: the LungBurden of the final mask per lung (None unless segment_volume was given per_lung=) and, when the lungs could not be split, why;
    distribution / distribution_error: the zones.LungDistribution of the final mask -- where in the lungs it sits -- (None unless segment_volume was given distribution=)
    and, when the lungs could not be split, why;
    sheet: the RenderedSheet of the final mask over the CT (None unless segment_volume was given render=);
    mesh / lung_mesh: the SurfaceMesh of the final mask and of the lung mask (None unless segment_volume was given mesh=);
    lesion_parts: the watershed.SplitLesions of the final mask with its own table (the field exists only when segment_volume was given split_lesions=)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def paste_back(prob, rects1, rects2, size):
    """unet_vol_paste_back: prob [n, d, d(, 1)] float32 device tensor -> canvas [n, size, size]; rects*: int [n, 4] with w <= 0 for "none"."""
    torch = _torch(); lib, ctx = _ctx()
    p = prob.reshape(prob.shape[0], prob.shape[1], prob.shape[2]).contiguous()
    n, d = p.shape[0], p.shape[1]
    r = None
    if rects1 is not None:
        r = np.ascontiguousarray(np.concatenate([np.asarray(rects1, np.int32).reshape(n, 4), np.asarray(rects2, np.int32).reshape(n, 4)], 1))
    canvas = torch.empty((n, size, size), dtype=torch.float32, device="cuda")
    ctx.check(lib.unet_vol_paste_back(ctx.handle, p.data_ptr(), n, d, r.ctypes.data if r is not None else None, canvas.data_ptr(), size, _stream()), "vol_paste_back")
    return canvas


def unslice(canvas, threshold, shape, z0, z1):
    """unet_vol_unslice: canvas [z1 - z0, S, S] -> (mask uint8 device tensor of X*Y*Z bytes in Fortran order, counts int64 [z1 - z0])."""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = (int(v) for v in shape)
    canvas = canvas.contiguous()
    mask = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    counts = torch.empty(z1 - z0, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_unslice(ctx.handle, canvas.data_ptr(), canvas.shape[1], float(threshold), X, Y, Z, z0, z1, mask.data_ptr(), counts.data_ptr(), _stream()),
              "vol_unslice")
    return mask, counts


# ---- connected components of a mask volume (csrc/kernels_components.hip) ------------------------------------------------------------------------
# one record of unet_vol_component_stats (include/unet_hip.h): 64 bytes
_STAT_DTYPE = np.dtype([("voxels", "<i8"), ("sx", "<i8"), ("sy", "<i8"), ("sz", "<i8"), ("x0", "<i4"), ("x1", "<i4"), ("y0", "<i4"), ("y1", "<i4"),
                        ("z0", "<i4"), ("z1", "<i4"), ("pad", "<i4", (2,))])
LESION_DTYPE = np.dtype([("label", np.int32), ("voxels", np.int64), ("ml", np.float64), ("x0", np.int32), ("x1", np.int32), ("y0", np.int32), ("y1", np.int32),
                         ("z0", np.int32), ("z1", np.int32), ("cx", np.float64), ("cy", np.float64), ("cz", np.float64)])


def _check_connectivity(connectivity):
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1 (6 neighbours), 2 (18) or 3 (26), not {connectivity!r}")
    return int(connectivity)


def _mask_to_device(mask, shape=None):
    """-> (device uint8 tensor of X*Y*Z bytes in Fortran order, (X, Y, Z)).  A numpy [X, Y, Z] array of any integer / bool dtype and order (foreground = non-zero),
    or the device byte tensor `unslice` returns together with shape=."""
    torch = _torch()
    if isinstance(mask, torch.Tensor):
        if shape is None:
            raise ValueError("a device mask is a flat Fortran-order byte buffer: pass shape=(X, Y, Z)")
        shape = tuple(int(v) for v in shape)
        if mask.dtype != torch.uint8 or not mask.is_cuda or mask.numel() != int(np.prod(shape)):
            raise ValueError(f"a device mask is a uint8 cuda tensor of prod(shape) = {int(np.prod(shape))} elements")
        return mask.contiguous().reshape(-1), shape
    a = np.asarray(mask)
    if a.ndim != 3:
        raise ValueError(f"a volume is [X, Y, Z]; got {a.ndim} dimensions")
    if a.dtype.kind not in "biu":
        raise ValueError(f"a mask has a bool or integer dtype, not {a.dtype}")
    flat = np.asfortranarray((a != 0).astype(np.uint8)).reshape(-1, order="F")
    return torch.from_numpy(flat).cuda(), tuple(int(v) for v in a.shape)


def _check_structure(connectivity, per_slice):
    """the structuring element of the morphology / per-slice labelling: generate_binary_structure(3, connectivity), per_slice: without its z = -1, +1 planes"""
    if per_slice:
        if connectivity not in (1, 2):
            raise ValueError(f"per_slice: connectivity must be 1 (4 neighbours in the slice) or 2 (8), not {connectivity!r}")
        return int(connectivity)
    return _check_connectivity(connectivity)


def label_device(mask_dev, shape, connectivity=1, per_slice=False):
    """unet_vol_label (per_slice: unet_vol_label_planar) on a device mask -> (labels: int32 device tensor of X*Y*Z elements in Fortran order, n)."""
    connectivity = _check_structure(connectivity, per_slice)
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    if X * Y * Z >= 2 ** 31:
        raise ValueError(f"a volume of {X} x {Y} x {Z} has 2^31 voxels or more")
    labels = torch.empty(X * Y * Z, dtype=torch.int32, device="cuda")
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_label_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    entry = lib.unet_vol_label_planar if per_slice else lib.unet_vol_label
    ctx.check(entry(ctx.handle, mask_dev.data_ptr(), X, Y, Z, connectivity, labels.data_ptr(), n_dev.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "vol_label_planar" if per_slice else "vol_label")
    return labels, int(n_dev.item())


def label_volume(mask, connectivity=1, return_device=False, shape=None, per_slice=False):
    """Connected components of mask != 0 -> (labels, n): int32 [X, Y, Z] (numpy, Fortran order; return_device=True: the flat device tensor), 0 on the background,
    components 1..n in the order of their first voxel in C order -- skimage.measure.label(mask != 0, connectivity=connectivity) element for element.
    per_slice=True: components never cross from one axial slice to the next (connectivity 1, 2 = 4, 8 neighbours in the slice): scipy.ndimage.label(mask, s) with
    s = generate_binary_structure(3, connectivity) and s[:, :, 0] = s[:, :, 2] = False; the numbering rule is the same."""
    _check_structure(connectivity, per_slice)
    dev, shape = _mask_to_device(mask, shape)
    labels, n = label_device(dev, shape, connectivity, per_slice)
    return (labels if return_device else labels.cpu().numpy().reshape(shape, order="F")), n


def component_stats_device(labels_dev, shape, n):
    """unet_vol_component_stats -> numpy records [n] (voxels, sx, sy, sz, x0, x1, y0, y1, z0, z1): 64 bytes per component come back, the labels stay."""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    st = torch.empty(max(n, 1) * _STAT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_component_stats(ctx.handle, labels_dev.data_ptr(), X, Y, Z, n, st.data_ptr(), _stream()), "vol_component_stats")
    return st[:n * _STAT_DTYPE.itemsize].cpu().numpy().view(_STAT_DTYPE)


def table_from_stats(stats, pixdim=(1, 1, 1)):
    """records of component_stats_device (or any arrays voxels, sx.., x0..) -> the LESION_DTYPE table: ml = voxels * prod(pixdim) / 1000, centroid = sum / count"""
    n = len(stats["voxels"])
    voxel_mm3 = float(np.prod(np.asarray(pixdim, np.float64)))
    t = np.zeros(n, LESION_DTYPE)
    t["label"] = np.arange(1, n + 1)
    t["voxels"] = stats["voxels"]
    t["ml"] = np.asarray(stats["voxels"], np.int64) * voxel_mm3 / 1000.0
    for k in ("x0", "x1", "y0", "y1", "z0", "z1"):
        t[k] = stats[k]
    cnt = np.asarray(stats["voxels"], np.float64)
    for k in "xyz":
        t["c" + k] = np.asarray(stats["s" + k], np.float64) / cnt
    return t


def component_table(labels, n, pixdim=(1, 1, 1), shape=None):
    """One row per component, sorted by label: label, voxels, ml, x0, x1, y0, y1, z0, z1 (inclusive bounds), cx, cy, cz (float64 voxel coordinates).
    labels: what label_volume returned (numpy [X, Y, Z], or the device tensor together with shape=)."""
    torch = _torch()
    if isinstance(labels, torch.Tensor):
        if shape is None:
            raise ValueError("device labels are a flat Fortran-order buffer: pass shape=(X, Y, Z)")
        dev, shape = labels.contiguous().reshape(-1), tuple(int(v) for v in shape)
    else:
        a = np.asarray(labels)
        if a.ndim != 3:
            raise ValueError(f"a volume is [X, Y, Z]; got {a.ndim} dimensions")
        shape = tuple(int(v) for v in a.shape)
        dev = torch.from_numpy(np.asfortranarray(a.astype(np.int32, copy=False)).reshape(-1, order="F")).cuda()
    return table_from_stats(component_stats_device(dev, shape, int(n)), pixdim)


def filter_components(labels_dev, keep, n, shape, z0=0, z1=None):
    """unet_vol_filter_components: keep [n + 1] (bool; entry 0 is the background's and is forced to 0) -> (mask device bytes, counts int64 [z1 - z0] device)."""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    z1 = Z if z1 is None else z1
    k = np.ascontiguousarray(np.asarray(keep).astype(bool).astype(np.uint8))
    if k.shape != (n + 1,):
        raise ValueError(f"keep has one entry per label 0..{n}, not {k.shape}")
    k[0] = 0
    kd = torch.from_numpy(k).cuda()
    mask = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    counts = torch.empty(max(z1 - z0, 0), dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_filter_components(ctx.handle, labels_dev.data_ptr(), kd.data_ptr(), n, X, Y, Z, z0, z1, mask.data_ptr(), counts.data_ptr(), _stream()),
              "vol_filter_components")
    return mask, counts


def min_voxels_from_ml(min_ml, pixdim):
    """the smallest voxel count whose volume reaches min_ml millilitres: ceil(min_ml * 1000 / prod(pixdim))"""
    return int(np.ceil(float(min_ml) * 1000.0 / float(np.prod(np.asarray(pixdim, np.float64)))))


def largest_labels(voxels, k):
    """labels (1-based, ascending) of the k components with the most voxels, ties to the lower label"""
    voxels = np.asarray(voxels, np.int64)
    order = np.lexsort((np.arange(voxels.size), -voxels))
    return np.sort(order[:max(0, int(k))] + 1)


def _filtered(mask, connectivity, choose, return_device, shape):
    dev, shape = _mask_to_device(mask, shape)
    labels, n = label_device(dev, shape, connectivity)
    st = component_stats_device(labels, shape, n)
    keep = np.zeros(n + 1, bool)
    keep[1:] = choose(st["voxels"])
    out, _ = filter_components(labels, keep, n, shape, 0, 0)
    return out if return_device else out.cpu().numpy().reshape(shape, order="F")


def remove_small(mask, min_voxels=None, min_ml=None, pixdim=None, connectivity=1, return_device=False, shape=None):
    """The mask (uint8 0 / 1) without the components of fewer than min_voxels voxels: skimage.morphology.remove_small_objects(mask != 0, min_size=min_voxels,
    connectivity=connectivity).  min_ml (with pixdim in mm) instead: min_voxels = ceil(min_ml * 1000 / prod(pixdim))."""
    if (min_voxels is None) == (min_ml is None):
        raise ValueError("pass exactly one of min_voxels, min_ml")
    if min_ml is not None:
        if pixdim is None:
            raise ValueError("min_ml needs pixdim (the voxel's edge lengths in mm)")
        min_voxels = min_voxels_from_ml(min_ml, pixdim)
    mv = int(min_voxels)
    return _filtered(mask, connectivity, lambda v: v >= mv, return_device, shape)


def keep_largest(mask, k=2, connectivity=1, return_device=False, shape=None):
    """The mask (uint8 0 / 1) with only its k components of the most voxels, ties to the lower label (the 3-D form of the reference's "two largest regions")."""
    def choose(v):
        sel = np.zeros(v.size, bool)
        sel[largest_labels(v, k) - 1] = True
        return sel
    return _filtered(mask, connectivity, choose, return_device, shape)

# ---- a mask volume against its ground truth (csrc/kernels_volscore.hip) ------------------------------------------------------
EDT_MAX_DIM = 4096                                                  # UNET_VOL_EDT_MAX_DIM
_SURFDIST_WS_BYTES = 32768                                          # UNET_VOL_SURFDIST_WS_BYTES
SCORED_LESION_DTYPE = {"truth": np.dtype(LESION_DTYPE.descr + [("covered_voxels", "<i8"), ("covered_share", "<f8"), ("detected", "?")]),
                       "pred": np.dtype(LESION_DTYPE.descr + [("covered_voxels", "<i8"), ("covered_share", "<f8"), ("matched", "?")])}


def _check_pixdim(pixdim):
    try:
        p = np.asarray(pixdim, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"pixdim is three positive finite numbers, not {pixdim!r}") from None
    if p.shape != (3,) or not np.isfinite(p).all() or not (p > 0).all() or not np.isfinite(p * p).all() or not (p * p > 0).all():
        raise ValueError(f"pixdim is three positive finite numbers (with finite, non-zero squares), not {pixdim!r}")
    return p


def _check_volume_dims(shape):
    X, Y, Z = shape
    if X * Y * Z >= 2 ** 31:
        raise ValueError(f"a volume of {X} x {Y} x {Z} has 2^31 voxels or more")


def confusion_device(pred_dev, truth_dev, shape):
    """unet_vol_confusion -> int64 [Z, 3] numpy: tp, fp, fn of every slice"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    _check_volume_dims(shape)
    counts = torch.empty((max(Z, 1), 3), dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_confusion(ctx.handle, pred_dev.data_ptr(), truth_dev.data_ptr(), X, Y, Z, counts.data_ptr(), _stream()), "vol_confusion")
    return counts[:Z].cpu().numpy()


def surface_device(mask_dev, shape, connectivity=1):
    """unet_vol_surface -> (surface: uint8 device tensor of X*Y*Z bytes in Fortran order, the number of surface voxels)"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    _check_volume_dims(shape)
    surf = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_surface(ctx.handle, mask_dev.data_ptr(), X, Y, Z, _check_connectivity(connectivity), surf.data_ptr(), count.data_ptr(), _stream()), "vol_surface")
    return surf, int(count.item())


def edt_sq_device(vol_dev, shape, pixdim=(1, 1, 1), features_nonzero=True):
    """unet_vol_edt_sq -> float64 device tensor of X*Y*Z elements: the exact squared distance (mm^2) of every voxel to the nearest feature -- the non-zero voxels of
    vol_dev, or its zero voxels; +inf everywhere when there is none."""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    p = _check_pixdim(pixdim)
    _check_volume_dims(shape)
    if max(shape) > EDT_MAX_DIM:
        raise ValueError(f"the distance transform takes at most {EDT_MAX_DIM} voxels per axis, not {X} x {Y} x {Z}")
    w = np.ascontiguousarray(p * p)
    d2 = torch.empty(X * Y * Z, dtype=torch.float64, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_edt_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_edt_sq(ctx.handle, vol_dev.data_ptr(), X, Y, Z, 1 if features_nonzero else 0, w.ctypes.data, d2.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "vol_edt_sq")
    return d2


def sqrt_device(x):
    """unet_vol_sqrt_f64: in place on a contiguous float64 device tensor"""
    lib, ctx = _ctx()
    ctx.check(lib.unet_vol_sqrt_f64(ctx.handle, x.data_ptr(), x.numel(), _stream()), "vol_sqrt_f64")
    return x


def surface_distances_device(surf_dev, d2_dev, shape, capacity):
    """unet_vol_surface_distances -> (count, max d2, sum of sqrt(d2), the d2 values of the surface voxels as a device tensor of min(count, capacity) doubles)"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    res = torch.zeros(3, dtype=torch.int64, device="cuda")
    gathered = torch.empty(max(int(capacity), 1), dtype=torch.float64, device="cuda")
    ws = torch.empty(_SURFDIST_WS_BYTES, dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_surface_distances(ctx.handle, surf_dev.data_ptr(), d2_dev.data_ptr(), X, Y, Z, res.data_ptr(), gathered.data_ptr(), int(capacity), ws.data_ptr(),
                                             ws.numel(), _stream()), "vol_surface_distances")
    r = res.cpu().numpy()
    count = int(r[0])
    return count, float(r[1:2].view(np.float64)[0]), float(r[2:3].view(np.float64)[0]), gathered[:min(count, int(capacity))]


def lesion_overlap_device(labels_t, n_t, labels_p, n_p, shape):
    """unet_vol_lesion_overlap -> (cover_t int64 [n_t], cover_p int64 [n_p]) numpy"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    ct = torch.zeros(max(n_t, 1), dtype=torch.int64, device="cuda"); cp = torch.zeros(max(n_p, 1), dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_lesion_overlap(ctx.handle, labels_t.data_ptr(), n_t, labels_p.data_ptr(), n_p, X, Y, Z, ct.data_ptr(), cp.data_ptr(), _stream()), "vol_lesion_overlap")
    return ct[:n_t].cpu().numpy(), cp[:n_p].cpu().numpy()


def surface(mask, connectivity=1, return_device=False, shape=None):
    """The surface voxels of mask != 0 as uint8 0 / 1: the foreground voxels with a background neighbour among the 6 / 18 / 26 of `connectivity` 1 / 2 / 3, voxels
    outside the volume counting as background -- m ^ scipy.ndimage.binary_erosion(m, generate_binary_structure(3, connectivity))."""
    _check_connectivity(connectivity)
    dev, shape = _mask_to_device(mask, shape)
    surf, _ = surface_device(dev, shape, connectivity)
    return surf if return_device else surf.cpu().numpy().reshape(shape, order="F")


def distance_transform(mask, pixdim=(1, 1, 1), squared=False, return_device=False, shape=None):
    """float64 distance (pixdim's unit) of every foreground voxel to the nearest background voxel, 0 on the background:
    scipy.ndimage.distance_transform_edt(mask != 0, sampling=pixdim).  squared=True: the exact squared distance of unet_vol_edt_sq (include/unet_hip.h states it
    operation by operation); otherwise its square root, taken on the device.  A mask without background gives +inf everywhere."""
    _check_pixdim(pixdim)
    dev, shape = _mask_to_device(mask, shape)
    d = edt_sq_device(dev, shape, pixdim, features_nonzero=False)
    if not squared:
        sqrt_device(d)
    return d if return_device else d.cpu().numpy().reshape(shape, order="F")


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        if not (isinstance(a, np.ndarray) and isinstance(b, np.ndarray)) or a.dtype != b.dtype or a.shape != b.shape:
            return False
        if a.dtype.names:
            return all(_same(a[k], b[k]) for k in a.dtype.names)
        return bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    return type(a) is type(b) and a == b


class VolumeScore:
    """What score_volume returns.  Overlap: tp, fp, fn, dice, iou, precision, recall, pred_ml, truth_ml, volume_error_ml, and per slice tp_per_slice, fp_per_slice,
    fn_per_slice, per_slice_dice [Z].  Surface (in pixdim's unit): hd_pred_to_truth, hd_truth_to_pred, hd, asd_pred_to_truth, asd_truth_to_pred, assd, hd95 (at
    `percentile`), n_surface_pred, n_surface_truth.  Lesions (None when not asked for): truth_lesions (the component table + covered_voxels, covered_share, detected),
    pred_lesions (+ covered_voxels, covered_share, matched), n_truth_lesions, n_pred_lesions, lesion_recall, lesion_precision, missed_lesions, false_positive_lesions.
    Two scores compare equal when every field holds the same values (nan equal to nan)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __eq__(self, other):
        return isinstance(other, VolumeScore) and self.__dict__.keys() == other.__dict__.keys() and all(_same(v, other.__dict__[k]) for k, v in self.__dict__.items())

    __hash__ = None

    def __repr__(self):
        return f"VolumeScore(dice={self.dice:.4f}, hd95={self.hd95:.3f}, assd={self.assd:.3f}, lesion_recall={self.lesion_recall})"


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def _lerp(a, b, t):
    """numpy's _lerp between two order statistics (floats or arrays): a + (b - a) t, and b - (b - a)(1 - t) from t = 0.5 on"""
    with np.errstate(invalid="ignore"):
        d = np.subtract(b, a)
        return np.where(np.asarray(t) >= 0.5, b - d * (1.0 - t), a + d * t)[()]


def _percentile_of_sorted(sorted_dev, q):
    """np.percentile(values, q) (linear interpolation) of sqrt(values) from an ascending device tensor of squared values: the two order statistics come to the host,
    sqrt is monotone, so they are the order statistics of the square roots"""
    n = sorted_dev.numel()
    pos = (float(q) / 100.0) * (n - 1)
    lo = min(int(np.floor(pos)), n - 1); hi = min(lo + 1, n - 1)
    a, b = (float(v) for v in np.sqrt(sorted_dev[[lo, hi]].cpu().numpy()))
    return float(_lerp(a, b, pos - lo))


def score_volume(pred, truth, pixdim=(1, 1, 1), connectivity=1, lesion_connectivity=1, percentile=95.0, min_overlap_voxels=1, lesions=True, shape=None):
    """A predicted mask against the ground truth of the same geometry -> VolumeScore.  pred, truth: numpy [X, Y, Z] arrays (bool / integer, foreground = non-zero) or
    flat device byte tensors with shape=; pixdim: the voxel's edge lengths in mm.  `connectivity` (1, 2, 3) is the structuring element of the surfaces,
    `lesion_connectivity` that of the lesions; a truth lesion is detected (a predicted one matched) when at least min_overlap_voxels of its voxels are marked by the
    other mask.  Both masks empty: every distance 0.0, dice = iou = 1.0; exactly one empty: every distance inf.  Everything is computed on the device; the Hausdorff
    distance is the host's sqrt of the device's exact maximum, hd95 the host's interpolation between two order statistics of the device's sort."""
    torch = _torch()
    p = _check_pixdim(pixdim)
    _check_connectivity(connectivity); _check_connectivity(lesion_connectivity)
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"percentile must lie in [0, 100], not {percentile!r}")
    for m in (pred, truth):                                         # refused before anything is uploaded or launched
        if not isinstance(m, torch.Tensor):
            a = np.asarray(m)
            if a.ndim != 3:
                raise ValueError(f"a volume is [X, Y, Z]; got {a.ndim} dimensions")
            if a.dtype.kind not in "biu":
                raise ValueError(f"a mask has a bool or integer dtype, not {a.dtype}")
    said = [(None if shape is None else tuple(int(v) for v in shape)) if isinstance(m, torch.Tensor) else tuple(np.shape(m)) for m in (pred, truth)]
    if None not in said and said[0] != said[1]:
        raise ValueError(f"the prediction is {said[0]}, the truth {said[1]}")
    pd, ps = _mask_to_device(pred, shape)
    td, ts = _mask_to_device(truth, shape)
    if ps != ts:
        raise ValueError(f"the prediction is {ps}, the truth {ts}")
    shape = ps
    _check_volume_dims(shape)
    if max(shape) > EDT_MAX_DIM:
        raise ValueError(f"the distance transform takes at most {EDT_MAX_DIM} voxels per axis, not {shape}")
    X, Y, Z = shape
    f = {}
    counts = confusion_device(pd, td, shape)
    tp, fp, fn = (int(v) for v in counts.sum(axis=0)) if Z else (0, 0, 0)
    voxel_mm3 = float(np.prod(p))
    empty = tp + fp + fn == 0
    den = (2 * counts[:, 0] + counts[:, 1] + counts[:, 2]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_slice = np.where(den > 0, 2.0 * counts[:, 0] / den, np.nan)
    f.update(tp=tp, fp=fp, fn=fn, dice=1.0 if empty else 2.0 * tp / (2 * tp + fp + fn), iou=1.0 if empty else tp / (tp + fp + fn),
             precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn), pred_ml=float(tp + fp) * voxel_mm3 / 1000.0, truth_ml=float(tp + fn) * voxel_mm3 / 1000.0,
             tp_per_slice=counts[:, 0].copy(), fp_per_slice=counts[:, 1].copy(), fn_per_slice=counts[:, 2].copy(), per_slice_dice=per_slice, percentile=float(percentile))
    f["volume_error_ml"] = f["pred_ml"] - f["truth_ml"]
    # surfaces and their distances: A = surface(pred), B = surface(truth); d(a, B) from the transform whose features are B's voxels
    sa, na = surface_device(pd, shape, connectivity) if X * Y * Z else (pd, 0)
    sb, nb = surface_device(td, shape, connectivity) if X * Y * Z else (td, 0)
    f.update(n_surface_pred=na, n_surface_truth=nb)
    names = ("hd_pred_to_truth", "hd_truth_to_pred", "hd", "asd_pred_to_truth", "asd_truth_to_pred", "assd", "hd95")
    if na == 0 or nb == 0:
        f.update({k: 0.0 if na == nb else float("inf") for k in names})
    else:
        d2 = edt_sq_device(sb, shape, p, True)
        ca, max_a, sum_a, ga = surface_distances_device(sa, d2, shape, na)
        d2 = edt_sq_device(sa, shape, p, True)
        cb, max_b, sum_b, gb = surface_distances_device(sb, d2, shape, nb)
        del d2
        if (ca, cb) != (na, nb):
            raise _lib.UNetHipError(f"score_volume: the surfaces hold {na} and {nb} voxels but {ca} and {cb} distances were gathered")
        f["hd_pred_to_truth"], f["hd_truth_to_pred"] = float(np.sqrt(max_a)), float(np.sqrt(max_b))
        f["hd"] = max(f["hd_pred_to_truth"], f["hd_truth_to_pred"])
        f["asd_pred_to_truth"], f["asd_truth_to_pred"] = sum_a / na, sum_b / nb
        f["assd"] = (f["asd_pred_to_truth"] + f["asd_truth_to_pred"]) / 2.0
        pooled, _ = torch.sort(torch.cat([ga, gb]))                 # ~10^6 values: plumbing
        f["hd95"] = _percentile_of_sorted(pooled, percentile)
    del sa, sb
    f.update(truth_lesions=None, pred_lesions=None, n_truth_lesions=None, n_pred_lesions=None, lesion_recall=None, lesion_precision=None, missed_lesions=None,
             false_positive_lesions=None)
    if lesions:
        mov = int(min_overlap_voxels)
        lt, nt = label_device(td, shape, lesion_connectivity)
        lp, npred = label_device(pd, shape, lesion_connectivity)
        cover_t, cover_p = lesion_overlap_device(lt, nt, lp, npred, shape)
        tables = {}
        for who, lab, n, cover, flag in (("truth", lt, nt, cover_t, "detected"), ("pred", lp, npred, cover_p, "matched")):
            base = table_from_stats(component_stats_device(lab, shape, n), p)
            t = np.zeros(n, SCORED_LESION_DTYPE[who])
            for k in LESION_DTYPE.names:
                t[k] = base[k]
            t["covered_voxels"] = cover
            t["covered_share"] = cover.astype(np.float64) / base["voxels"].astype(np.float64)
            t[flag] = cover >= mov
            tables[who] = t
        det, mat = int(tables["truth"]["detected"].sum()), int(tables["pred"]["matched"].sum())
        f.update(truth_lesions=tables["truth"], pred_lesions=tables["pred"], n_truth_lesions=nt, n_pred_lesions=npred, lesion_recall=_ratio(det, nt),
                 lesion_precision=_ratio(mat, npred), missed_lesions=nt - det, false_positive_lesions=npred - mat)
    return VolumeScore(**f)

# ---- binary morphology of a mask volume (csrc/kernels_morph.hip) ----------------------------------------------------------------
MORPH_MAX_ITERATIONS = _lib.MORPH_MAX_ITERATIONS                     # UNET_VOL_MORPH_MAX_ITERATIONS


def _check_mask_host(mask, shape=None):
    """what _mask_to_device refuses, before anything is uploaded or launched"""
    torch = _torch()
    if isinstance(mask, torch.Tensor):
        if shape is None:
            raise ValueError("a device mask is a flat Fortran-order byte buffer: pass shape=(X, Y, Z)")
        return
    a = np.asarray(mask)
    if a.ndim != 3:
        raise ValueError(f"a volume is [X, Y, Z]; got {a.ndim} dimensions")
    if a.dtype.kind not in "biu":
        raise ValueError(f"a mask has a bool or integer dtype, not {a.dtype}")


def _check_morph(op, connectivity, iterations, border_value, per_slice):
    if op not in _lib.MORPH_OPS:
        raise ValueError(f"op must be one of {tuple(_lib.MORPH_OPS)}, not {op!r}")
    connectivity = _check_structure(connectivity, per_slice)
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 1 <= iterations <= MORPH_MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer in 1..{MORPH_MAX_ITERATIONS} (scipy's iterations < 1, \"until stable\", is not offered), not {iterations!r}")
    if border_value not in (0, 1):
        raise ValueError(f"border_value must be 0 or 1, not {border_value!r}")
    return connectivity, int(iterations), int(border_value)


def _check_radius(radius_mm):
    try:
        r = float(radius_mm)
    except (TypeError, ValueError):
        raise ValueError(f"radius_mm is a finite number >= 0, not {radius_mm!r}") from None
    if not (np.isfinite(r) and r >= 0.0 and np.isfinite(r * r)):
        raise ValueError(f"radius_mm is a finite number >= 0 (with a finite square), not {radius_mm!r}")
    return r


def morph_device(mask_dev, shape, op, connectivity=1, iterations=1, border_value=0, per_slice=False):
    """unet_vol_morph on a device mask -> (result: uint8 device tensor of X*Y*Z bytes in Fortran order, counts: int64 [Z] device tensor, the set voxels per slice)"""
    connectivity, iterations, border_value = _check_morph(op, connectivity, iterations, border_value, per_slice)
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    _check_volume_dims(shape)
    out = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(Z, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_morph_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_morph(ctx.handle, mask_dev.data_ptr(), X, Y, Z, _lib.MORPH_OPS[op], connectivity, 1 if per_slice else 0, iterations, border_value, out.data_ptr(),
                                 counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "vol_morph")
    return out, counts


def ball_device(mask_dev, shape, radius_mm, pixdim, dilate):
    """The mask dilated (dilate=True) or eroded by the closed ball of radius_mm: unet_vol_edt_sq to the foreground / to the background, then unet_vol_ball with
    r2 = fl(r r) -> (result device bytes, counts int64 [Z] device)"""
    r = _check_radius(radius_mm)
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    d2 = edt_sq_device(mask_dev, shape, pixdim, features_nonzero=bool(dilate))
    out = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(Z, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_ball(ctx.handle, d2.data_ptr(), X, Y, Z, r * r, 1 if dilate else 0, out.data_ptr(), counts.data_ptr(), _stream()), "vol_ball")
    return out, counts


def fill_holes_device(mask_dev, shape, connectivity=1, per_slice=False):
    """unet_vol_fill_holes on a device mask -> (result device bytes, counts int64 [Z] device)"""
    connectivity = _check_structure(connectivity, per_slice)
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    _check_volume_dims(shape)
    out = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(Z, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_fill_holes_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_fill_holes(ctx.handle, mask_dev.data_ptr(), X, Y, Z, connectivity, 1 if per_slice else 0, out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream()), "vol_fill_holes")
    return out, counts


def _result(dev, shape, return_device):
    return dev if return_device else dev.cpu().numpy().reshape(shape, order="F")


def _binary(op, mask, connectivity, iterations, border_value, per_slice, return_device, shape):
    _check_morph(op, connectivity, iterations, border_value, per_slice)
    _check_mask_host(mask, shape)
    dev, shape = _mask_to_device(mask, shape)
    return _result(morph_device(dev, shape, op, connectivity, iterations, border_value, per_slice)[0], shape, return_device)


def binary_dilation(mask, connectivity=1, iterations=1, border_value=0, per_slice=False, return_device=False, shape=None):
    """scipy.ndimage.binary_dilation(mask != 0, generate_binary_structure(3, connectivity), iterations=iterations, border_value=border_value) as uint8 0 / 1, element for
    element.  connectivity 1, 2, 3 = 6, 18, 26 neighbours; iterations 1..64; border_value 0 / 1: what the voxels outside the volume hold at every step.  per_slice=True:
    the structure without its z = -1 and z = +1 planes (connectivity 1 or 2): every axial slice on its own."""
    return _binary("dilate", mask, connectivity, iterations, border_value, per_slice, return_device, shape)


def binary_erosion(mask, connectivity=1, iterations=1, border_value=0, per_slice=False, return_device=False, shape=None):
    """scipy.ndimage.binary_erosion with the structure and parameters of binary_dilation.  border_value=0 erodes from the volume's faces, 1 does not."""
    return _binary("erode", mask, connectivity, iterations, border_value, per_slice, return_device, shape)


def binary_opening(mask, connectivity=1, iterations=1, border_value=0, per_slice=False, return_device=False, shape=None):
    """scipy.ndimage.binary_opening: `iterations` erosions, then as many dilations, all with the same border_value."""
    return _binary("open", mask, connectivity, iterations, border_value, per_slice, return_device, shape)


def binary_closing(mask, connectivity=1, iterations=1, border_value=0, per_slice=False, return_device=False, shape=None):
    """scipy.ndimage.binary_closing: `iterations` dilations, then as many erosions, all with the same border_value (with 0, the erosions eat into what touches a face)."""
    return _binary("close", mask, connectivity, iterations, border_value, per_slice, return_device, shape)


def _ball(ops, mask, radius_mm, pixdim, return_device, shape):
    _check_radius(radius_mm); _check_pixdim(pixdim)
    _check_mask_host(mask, shape)
    dev, shape = _mask_to_device(mask, shape)
    for dilate in ops:
        dev, _ = ball_device(dev, shape, radius_mm, pixdim, dilate)
    return _result(dev, shape, return_device)


def dilate_mm(mask, radius_mm, pixdim=(1, 1, 1), return_device=False, shape=None):
    """The mask dilated by the closed ball of radius_mm millimetres under the voxel spacing pixdim: every voxel whose exact squared distance to the foreground
    (unet_vol_edt_sq, include/unet_hip.h) is <= fl(radius_mm^2).  Nothing outside the volume is foreground."""
    return _ball((True,), mask, radius_mm, pixdim, return_device, shape)


def erode_mm(mask, radius_mm, pixdim=(1, 1, 1), return_device=False, shape=None):
    """The mask eroded by that ball: every voxel whose squared distance to the background is > fl(radius_mm^2).  The distance transform has no feature outside the
    volume, so the outside counts as FOREGROUND here: a lesion that touches a face is not eroded from that face, and a mask without background stays whole."""
    return _ball((False,), mask, radius_mm, pixdim, return_device, shape)


def open_mm(mask, radius_mm, pixdim=(1, 1, 1), return_device=False, shape=None):
    """erode_mm, then dilate_mm: removes what the ball does not fit into"""
    return _ball((False, True), mask, radius_mm, pixdim, return_device, shape)


def close_mm(mask, radius_mm, pixdim=(1, 1, 1), return_device=False, shape=None):
    """dilate_mm, then erode_mm: closes gaps narrower than the ball (the erosion's outside is foreground, so nothing is lost at the faces)"""
    return _ball((True, False), mask, radius_mm, pixdim, return_device, shape)


def fill_holes(mask, connectivity=1, per_slice=False, return_device=False, shape=None):
    """scipy.ndimage.binary_fill_holes(mask != 0, generate_binary_structure(3, connectivity)) as uint8 0 / 1: the mask plus every background component (under that
    connectivity) that does not reach a face of the volume.  per_slice=True: the structure without its z = -1, +1 planes -- every slice's holes are filled in 2-D, the
    border being the slice's four edges."""
    _check_structure(connectivity, per_slice)
    _check_mask_host(mask, shape)
    dev, shape = _mask_to_device(mask, shape)
    return _result(fill_holes_device(dev, shape, connectivity, per_slice)[0], shape, return_device)


_MORPH_STEPS = {"dilate": "dilate", "erode": "erode", "open": "open", "close": "close",
                "binary_dilation": "dilate", "binary_erosion": "erode", "binary_opening": "open", "binary_closing": "close"}
_BALL_STEPS = {"dilate_mm": (True,), "erode_mm": (False,), "open_mm": (False, True), "close_mm": (True, False)}
POSTPROCESS_STEPS = tuple(_MORPH_STEPS) + tuple(_BALL_STEPS) + ("fill_holes", "remove_small", "keep_largest")
_STEP_KEYS = {"morph": {"connectivity", "iterations", "border_value", "per_slice"}, "ball": {"radius_mm", "pixdim"}, "fill_holes": {"connectivity", "per_slice"},
              "remove_small": {"min_voxels", "min_ml", "pixdim", "connectivity"}, "keep_largest": {"k", "connectivity"}}


def _check_steps(steps, pixdim):
    """-> [(kind, name, kwargs)] with every argument checked on the host: a bad step is refused before the first one runs"""
    if pixdim is not None:
        _check_pixdim(pixdim)
    out = []
    try:
        steps = list(steps)
    except TypeError:
        raise ValueError(f"steps is a list of (name, kwargs) pairs, not {steps!r}") from None
    for st in steps:
        if isinstance(st, str):
            st = (st, {})
        if not isinstance(st, (tuple, list)) or len(st) != 2 or not isinstance(st[0], str) or not isinstance(st[1], (dict, type(None))):
            raise ValueError(f"a step is a (name, kwargs) pair, not {st!r}")
        name, kw = st[0], dict(st[1] or {})
        if name not in POSTPROCESS_STEPS:
            raise ValueError(f"unknown step {name!r}: one of {POSTPROCESS_STEPS}")
        kind = "morph" if name in _MORPH_STEPS else "ball" if name in _BALL_STEPS else name
        extra = set(kw) - _STEP_KEYS[kind]
        if extra:
            raise ValueError(f"step {name!r} takes {sorted(_STEP_KEYS[kind])}, not {sorted(extra)}")
        if kind == "morph":
            _check_morph(_MORPH_STEPS[name], kw.get("connectivity", 1), kw.get("iterations", 1), kw.get("border_value", 0), kw.get("per_slice", False))
        elif kind == "ball":
            if "radius_mm" not in kw:
                raise ValueError(f"step {name!r} needs radius_mm")
            kw.setdefault("pixdim", pixdim)
            if kw["pixdim"] is None:
                raise ValueError(f"step {name!r} needs pixdim (the voxel's edge lengths in mm)")
            _check_radius(kw["radius_mm"]); _check_pixdim(kw["pixdim"])
        elif kind == "fill_holes":
            _check_structure(kw.get("connectivity", 1), kw.get("per_slice", False))
        elif kind == "remove_small":
            _check_connectivity(kw.get("connectivity", 1))
            if (kw.get("min_voxels") is None) == (kw.get("min_ml") is None):
                raise ValueError("remove_small: pass exactly one of min_voxels, min_ml")
            if kw.get("min_ml") is not None:
                kw.setdefault("pixdim", pixdim)
                if kw["pixdim"] is None:
                    raise ValueError("remove_small: min_ml needs pixdim (the voxel's edge lengths in mm)")
                kw["min_voxels"] = min_voxels_from_ml(kw["min_ml"], _check_pixdim(kw["pixdim"]))
            kw["min_voxels"] = int(kw["min_voxels"])
        else:
            _check_connectivity(kw.get("connectivity", 1))
            kw["k"] = int(kw.get("k", 2))
        out.append((kind, name, kw))
    return out


def _components_step(dev, shape, connectivity, choose):
    labels, n = label_device(dev, shape, connectivity)
    st = component_stats_device(labels, shape, n)
    keep = np.zeros(n + 1, bool)
    keep[1:] = choose(st["voxels"])
    return filter_components(labels, keep, n, shape, 0, shape[2])


def postprocess_device(mask_dev, shape, steps, pixdim=None):
    """the checked steps on a device mask -> (result device bytes, counts int64 [Z] device or None when there was no step)"""
    counts = None
    for kind, name, kw in _check_steps(steps, pixdim):
        if kind == "morph":
            mask_dev, counts = morph_device(mask_dev, shape, _MORPH_STEPS[name], kw.get("connectivity", 1), kw.get("iterations", 1), kw.get("border_value", 0),
                                            kw.get("per_slice", False))
        elif kind == "ball":
            for dilate in _BALL_STEPS[name]:
                mask_dev, counts = ball_device(mask_dev, shape, kw["radius_mm"], kw["pixdim"], dilate)
        elif kind == "fill_holes":
            mask_dev, counts = fill_holes_device(mask_dev, shape, kw.get("connectivity", 1), kw.get("per_slice", False))
        elif kind == "remove_small":
            mv = kw["min_voxels"]
            mask_dev, counts = _components_step(mask_dev, shape, kw.get("connectivity", 1), lambda v: v >= mv)
        else:
            def choose(v, k=kw["k"]):
                sel = np.zeros(v.size, bool)
                sel[largest_labels(v, k) - 1] = True
                return sel
            mask_dev, counts = _components_step(mask_dev, shape, kw.get("connectivity", 1), choose)
    return mask_dev, counts


def postprocess(mask, steps, pixdim=None, return_device=False, shape=None):
    """The cleaning steps, in order, on the device; the mask goes up once and comes back once.  steps: a list of (name, kwargs) pairs (a bare name: no arguments):
        "dilate" / "erode" / "open" / "close"              connectivity, iterations, border_value, per_slice          (binary_dilation ... binary_closing)
        "dilate_mm" / "erode_mm" / "open_mm" / "close_mm"  radius_mm, pixdim (default: this call's pixdim)
        "fill_holes"                                       connectivity, per_slice
        "remove_small"                                     min_voxels or min_ml (+ pixdim, default this call's), connectivity
        "keep_largest"                                     k, connectivity
    The usual clinical cleaning: [("close", {"iterations": 2}), ("fill_holes", {}), ("remove_small", {"min_ml": 0.05})].  Every step's arguments are checked before the
    first one runs."""
    _check_steps(steps, pixdim)
    _check_mask_host(mask, shape)
    dev, shape = _mask_to_device(mask, shape)
    return _result(postprocess_device(dev, shape, steps, pixdim)[0], shape, return_device)


def _check_lungs(lungs, lung_mask):
    """segment_volume's lungs= -> None (off) or the checked keyword arguments of lungs.lung_mask"""
    if lungs is None or lungs is False:
        return None
    if lung_mask is not None:
        raise ValueError("lungs= computes the lung mask and lung_mask= gives one: pass one of them")
    if lungs is not True and not isinstance(lungs, dict):
        raise ValueError(f"lungs is True or a dict of lungs.lung_mask keyword arguments, not {lungs!r}")
    from . import lungs as L
    kw = {} if lungs is True else dict(lungs)
    if set(kw) - L._LUNG_MASK_KEYS:
        raise ValueError(f"lungs takes {sorted(L._LUNG_MASK_KEYS)}, not {sorted(set(kw) - L._LUNG_MASK_KEYS)}")
    L._check_lung_mask_args(**kw)
    return kw


def _check_vessels(vessels, lung_mask):
    """segment_volume's vessels= -> None (off) or the checked keyword arguments of vessels.vessel_mask"""
    if vessels is None or vessels is False:
        return None
    if vessels is not True and not isinstance(vessels, dict):
        raise ValueError(f"vessels is True or a dict of vessels.vessel_mask keyword arguments, not {vessels!r}")
    from . import vessels as VS
    kw = {} if vessels is True else dict(vessels)
    if set(kw) - VS._VESSEL_MASK_KEYS:
        raise ValueError(f"vessels takes {sorted(VS._VESSEL_MASK_KEYS)}, not {sorted(set(kw) - VS._VESSEL_MASK_KEYS)}")
    VS._check_vessel_mask_args(**kw)
    if lung_mask is None:
        raise ValueError("vessels needs lung_mask (or lungs=): the vessels are searched inside the lungs")
    return kw


def _check_airway_tree(airway_tree, lungs):
    """segment_volume's airway_tree= -> None (off) or the checked keyword arguments of skeleton.airway_tree; lungs: the checked lungs= (or None)"""
    if airway_tree is None or airway_tree is False:
        return None
    if airway_tree is not True and not isinstance(airway_tree, dict):
        raise ValueError(f"airway_tree is True or a dict of skeleton.airway_tree keyword arguments, not {airway_tree!r}")
    from . import skeleton as SK
    kw = {} if airway_tree is True else dict(airway_tree)
    SK._check_tree_args(kw, "airway_tree")
    if lungs is None or lungs.get("airways", "auto") is False:
        raise ValueError("airway_tree needs lungs= with its airway step: the airway it thins is the one lungs.lung_mask grows")
    return kw


def _segmentation_airway_tree(kw, lm, ct, lungs):
    """the airway tree of the airway lungs.lung_mask grew, from the device buffers it left -> the extra result fields; the superior end: airway_tree's own orientation /
    affine, else lungs=' orientation, else the axis codes of the CT (a NiftiVolume by now: a path is decoded once, in front).  An airway step that did not run leaves
    res.airway_tree None and the reason in res.airway_tree_error."""
    from . import skeleton as SK
    if lm.airways is None:
        return dict(airway_tree=None, airway_tree_error=lm.airway_error)
    kw = dict(kw)
    if kw.get("orientation") is None and kw.get("affine") is None:
        kw["orientation"] = lungs.get("orientation")
        if kw["orientation"] is None and isinstance(ct, nifti_min.NiftiVolume) and ct.affine is not None:
            try:
                kw["orientation"] = ct.axcodes
            except nifti_min.NiftiFormatError:
                kw["orientation"] = None
    return dict(airway_tree=SK.airway_tree(lm, **kw), airway_tree_error=None)


def _check_split_lesions(split_lesions):
    """segment_volume's split_lesions= -> None (off) or the checked keyword arguments of watershed.split_lesions_device"""
    if split_lesions is None or split_lesions is False:
        return None
    if split_lesions is not True and not isinstance(split_lesions, dict):
        raise ValueError(f"split_lesions is True or a dict of watershed.split_lesions keyword arguments, not {split_lesions!r}")
    from . import watershed as W
    kw = {} if split_lesions is True else dict(split_lesions)
    unknown = sorted(set(kw) - {"seed_depth_mm", "connectivity", "min_seed_voxels", "quantum_mm2"})
    if unknown:
        raise ValueError(f"split_lesions takes seed_depth_mm, connectivity, min_seed_voxels and quantum_mm2, not {unknown}")
    W._check_split_args((1.0, 1.0, 1.0), kw.get("seed_depth_mm", W.SEED_DEPTH_MM), kw.get("connectivity", 1), kw.get("min_seed_voxels", 1), kw.get("quantum_mm2"))
    return kw


def _segmentation_lesion_parts(kw, mask_dev, shape, pixdim):
    """the parts of the final mask and their table -> the extra result field"""
    from . import watershed as W
    parts = W.split_lesions_device(mask_dev, shape, pixdim, **kw)
    parts.table = table_from_stats(component_stats_device(parts.labels, shape, parts.n), pixdim)
    parts.labels = _host_of(parts.labels, np.int32, shape)
    return dict(lesion_parts=parts)


def _segmentation_vessels(vessels, vol, lv, mask_dev, shape, density):
    """the vessel mask inside the lung mask, the infection's volume on it and, with density=, the infection's density without it -> the extra result fields"""
    from . import lungs as L
    from . import vessels as VS
    torch = _torch()
    lungs_dev = _mask_to_device(lv.get_fdata() != 0, None)[0]
    vm = VS.vessel_mask(vol, lungs_dev, pixdim=vol.pixdim, return_device=True, **vessels)
    on = int(torch.count_nonzero((mask_dev != 0) & (vm.mask != 0)).item())
    out = dict(vessels=vm, infected_ml_on_vessels=float(on) * float(np.prod(np.asarray(vol.pixdim, np.float64))) / 1000.0)
    if density is not None:
        out["vessel_free_density"] = intensity_stats(vol, mask=mask_dev, region=L._and_not(lungs_dev, vm.mask, shape), shape=shape, **density)
    vm.mask = _host_of(vm.mask, np.uint8, shape)
    vm.vesselness.response, vm.vesselness.scale = _host_of(vm.vesselness.response, np.float32, shape), _host_of(vm.vesselness.scale, np.uint8, shape)
    return out


def _computed_lungs(ct, lungs, lung_mask, airway_tree=None):
    """-> (the lung mask segment_volume goes on with, (extra result fields, extra seconds)): lungs.lung_mask(ct) as a host array when lungs= asks for it.  airway_tree
    (the checked keyword arguments, or None): the lung mask then stays on the device until the airway it grew has been thinned, and comes to the host after that."""
    if lungs is None:
        return lung_mask, ({}, {})
    from . import lungs as L
    t0 = time.perf_counter()
    if airway_tree is None:
        lm = L.lung_mask(ct, **lungs)
        return lm.mask, (dict(lungs=lm), dict(lungs=time.perf_counter() - t0))
    lm = L.lung_mask(ct, return_device=True, **lungs)
    _torch().cuda.synchronize(); t1 = time.perf_counter()
    extra = _segmentation_airway_tree(airway_tree, lm, ct, lungs)
    _torch().cuda.synchronize(); t2 = time.perf_counter()
    lm.mask = _host_of(lm.mask, np.uint8, lm.shape)
    if lm.airways is not None:
        lm.airways.mask = _host_of(lm.airways.mask, np.uint8, lm.shape)
    return lm.mask, (dict(lungs=lm, **extra), dict(lungs=t1 - t0 + time.perf_counter() - t2, airway_tree=t2 - t1))


def _prepare_segmentation(ct, lung_mask, truth, img_size, trim, input_size):
    """The front of segment_volume / segment_volume_ensemble: decode the CT (and the truth and lung masks), the lung rectangles keyed by slice number, the prepared
    batch x [n, d, d, 1] on the device (d = input_size(), asked for once the truth mask has been checked) -> (vol, lv, truth_mask, z0, z1, S, x, info, R1, R2, has, seconds); R1, R2: int32 [n, 4] per kept slice, zeros where has is False."""
    torch = _torch()
    sec = {}
    t0 = time.perf_counter()
    vol = _source(ct)
    sec["decode"] = time.perf_counter() - t0
    X, Y, Z = vol.raw.shape
    truth_mask = None
    if truth is not None:
        tv = _source(truth)
        if tv.raw.shape != vol.raw.shape:
            raise ValueError(f"the truth mask is {tv.raw.shape}, the CT {vol.raw.shape}")
        truth_mask = tv.get_fdata() != 0
    z0, z1 = trim_range(Z, trim)
    n, S = z1 - z0, int(img_size)
    d = input_size()
    if lung_mask is not None:
        lv = _source(lung_mask)
        if lv.raw.shape != vol.raw.shape:
            raise ValueError(f"the lung mask is {lv.raw.shape}, the CT {vol.raw.shape}")
        r1, r2, kept = load_volume(lv, "lungs", S, trim)
    else:
        lv = None
        r1, r2 = whole_frame_rects(n, S); kept = list(range(n))
    plan = box_plan(n, kept, "slice")
    t0 = time.perf_counter()
    x, info = load_volume(vol, "cts", S, trim, (r1, r2, kept), "slice", d, return_info=True)
    torch.cuda.synchronize(); sec["load_volume"] = time.perf_counter() - t0
    R1, R2 = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
    has = plan >= 0
    R1[has], R2[has] = np.asarray(r1, np.int32).reshape(-1, 4)[plan[has]], np.asarray(r2, np.int32).reshape(-1, 4)[plan[has]]
    return vol, lv, truth_mask, z0, z1, S, x, info, R1, R2, has, sec


def segment_volume(ct, model, lung_mask=None, threshold=0.547, batch_size=32, out_path=None, img_size=512, trim=(0.2, 0.8), min_lesion_ml=None, connectivity=1,
                   lesions=False, truth=None, postprocess=None, density=None, per_lung=None, render=None, mesh=None, distribution=None, lungs=None, vessels=None, airway_tree=None,
                   split_lesions=None):
    """CT file (or array) -> VolumeSegmentation.  `model`: a UNetModel or a routed.ClusterRoutedModel (only `predict` is used); lung_mask=None: whole-frame
    boxes (the two halves of the frame); boxes are keyed by slice number (box_indexing="slice"); out_path: the mask as .nii / .nii.gz with the CT's geometry.
    min_lesion_ml: connected components (`connectivity` 1, 2, 3 = 6, 18, 26 neighbours) smaller than that are removed on the device before the mask comes to the
    host or reaches out_path; counts, ml_per_slice, total_ml, infected_share then describe the filtered mask and removed_ml what went.  lesions=True (or a
    filter): res.lesions = the component_table of the final mask, res.n_lesions its length.  The labels never leave the device.
    truth: the ground-truth mask in the CT's geometry (path or [X, Y, Z] array, foreground = non-zero): the final mask is scored against it before it leaves the
    device, res.score = score_volume(mask, truth, pixdim, lesion_connectivity=connectivity); None without a truth.
    postprocess: a list of steps as volume.postprocess takes them (pixdim: the CT's), run on the device right after the mask volume is formed and before min_lesion_ml,
    lesions and truth: counts, ml_per_slice, total_ml, infected_share, the lesion table and the score then describe the cleaned mask (counts over all Z slices: a
    dilation may reach a trimmed slice), res.postprocess_ml is the volume the steps added (negative: removed) and seconds["postprocess"] their time; None: nothing
    runs and res.postprocess_ml is None.
    density: True, or a dict of intensity_stats keyword arguments (edges, names, percentiles, moments, per_slice): after postprocess / min_lesion_ml, res.density =
    intensity_stats of the CT under the final mask -- one row per lesion of res.lesions when the lesion table is computed (the device labels are reused, not relabelled),
    one group otherwise --, res.lung_density the same under the lung mask (None without one), seconds["density"] their time.  The CT's raw voxels are uploaded a second
    time for it.  None: nothing runs, both fields are None.
    per_lung: True, or a dict of split_lungs keyword arguments (orientation, pixdim, connectivity, min_ratio, erode_mm); needs lung_mask (ValueError before any device
    work without one).  After postprocess / min_lesion_ml, on the final mask: the lung mask is split (split_lungs; orientation: the lung mask file's own, else the CT's;
    pixdim: the CT's) and res.per_lung = the LungBurden of the final mask -- its `lesions` rows align with res.lesions when the lesion table is computed (the device labels
    are reused), `sides` is the LungSides, and with density= as well `density` = intensity_stats(ct, labels=sides, n=2): two rows, left then right.  A LungSplitError does
    not lose the segmentation: res.per_lung is None and res.per_lung_error holds its message.  seconds["per_lung"]: its time.  None: nothing runs.
    render: True, or a dict of render_planes keyword arguments (window, cmap, mm_per_px, tile_size, roi, cols, gap, background, interp) plus n (the number of key slices,
    default 6) and out_path (a PNG).  After postprocess / min_lesion_ml / per_lung: res.sheet = the RenderedSheet of the key_slices(counts, n) axial planes -- the middle
    slice when no slice holds infection -- followed by one coronal maximum projection of the whole volume; its layers are the final mask, taken from the device (fill 128,
    outline 255, PALETTE_INFECTION), and, with a lung mask, the lungs as an outline only (PALETTE_LUNG).  The sheet does not mark left and right.  seconds["render"]: its
    time.  None: nothing runs and res.sheet is None.
    mesh: True, or a dict {what: "infection" (default) | "lung" | "both", out_path: an .stl / .ply / .obj file, lesions: bool}.  After render: res.mesh = the
    SurfaceMesh (extract_surface, closed) of the final mask, taken from the device, in the CT's world frame (its affine; "scaled voxel" by its pixdim without one);
    lesions=True labels the final mask (`connectivity`) and meshes the labels with groups, res.mesh.lesions = lesion_shapes' table, its rows aligned with res.lesions;
    res.lung_mesh = the mesh of the lung mask for what "lung" / "both" (needs lung_mask: ValueError before any device work).  out_path receives the infection mesh (the
    lung mesh for what="lung"; with "both" the lung mesh goes to <stem>_lung<suffix>).  seconds["mesh"]: its time.  None: nothing runs, both fields are None.
    distribution: True, or a dict of zones.lung_zones / lung_distribution keyword arguments (zones, ap_parts, extent, depth, fill, severity_edges, predominance); needs
    per_lung (ValueError before any work without it).  Right after per_lung, on the sides and the lesion labels it left on the device: res.distribution = the
    LungDistribution of the final mask -- where in the lungs the infection sits: per region, per depth shell, per lesion (rows aligned with res.lesions when the lesion
    table is computed), a severity score per region and the words of a report; its zone map is on the host.  When the lungs could not be split res.distribution is None
    and res.distribution_error holds the reason.  seconds["distribution"]: its time.  None: nothing runs and no other field changes.
    lungs: True, or a dict of lungs.lung_mask keyword arguments: the lung mask is computed from the CT first (lungs.lung_mask; a lung U-Net under its model= key) and used
    exactly as a lung_mask= array in the CT's orientation would be; res.lungs is the LungMask and seconds["lungs"] its time.  Giving both lungs= and lung_mask= is a
    ValueError.  None: nothing runs and nothing changes.
    vessels: True, or a dict of vessels.vessel_mask keyword arguments (threshold, dense_hu, max_radius_mm, min_ml, connectivity, erode_mm, sigmas_mm, alpha, beta, c,
    bright); needs a lung mask (lung_mask= or lungs=; ValueError before any work without one).  After density, on the final mask: res.vessels = the VesselMask inside the
    lung mask (host arrays; the CT's pixdim), res.infected_ml_on_vessels the volume of infection AND vessels -- the infection U-Net's false positives sit there -- and,
    with density= as well, res.vessel_free_density = intensity_stats(ct, mask=infection, region=lungs & ~vessels) beside the unchanged res.density.  The infection mask
    itself is never altered.  A float64 CT is refused as filters refuse it.  seconds["vessels"]: its time.  None: nothing runs and no field is added.
    airway_tree: True, or a dict of skeleton.airway_tree keyword arguments; needs lungs= with its airway step (ValueError before any work otherwise).  Right after the
    lung mask: res.airway_tree = the CenterlineTree of the airway lungs.lung_mask grew -- centerline, branch graph, generations from the superior end, the airway voxels
    of every branch; a cycle marks a leak.  The superior end comes from the keyword's own orientation / affine, else from lungs=' orientation, else from the CT file's
    axis codes; it is never guessed.  When the airway step did not run res.airway_tree is None and res.airway_tree_error says why.  seconds["airway_tree"]: its time.
    None: nothing runs and no field is added.
    split_lesions: True, or a dict of watershed.split_lesions keyword arguments (seed_depth_mm, connectivity, min_seed_voxels, quantum_mm2; the pixdim is the CT's).  On
    the final mask, after the component filter: res.lesion_parts = the SplitLesions of the mask -- lesions that touch over a narrow bridge come apart -- with its labels on
    the host and its own component_table in res.lesion_parts.table.  res.lesions and every other field stay what they are without it.  seconds["split_lesions"]: its
    time.  None: nothing runs and no field is added."""
    _check_connectivity(connectivity)
    lungs = _check_lungs(lungs, lung_mask)
    airway_tree = _check_airway_tree(airway_tree, lungs)
    split_lesions = _check_split_lesions(split_lesions)
    lung_mask = True if lungs is not None else lung_mask          # (the checks below ask only whether there is one)
    vessels = _check_vessels(vessels, lung_mask)
    density = _check_density(density)
    per_lung = _check_per_lung(per_lung, lung_mask)
    distribution = _check_distribution(distribution, per_lung)
    render = _check_render(render)
    mesh = _check_mesh(mesh, lung_mask)
    if postprocess is not None:
        _check_steps(postprocess, (1.0, 1.0, 1.0))                   # the steps' own arguments, before any work (the CT's pixdim takes this one's place below)
    torch = _torch()
    if airway_tree is not None and isinstance(ct, (str, os.PathLike)):
        ct = nifti_min.read(ct)                                      # once: the lung mask, the airway tree's axis codes and the slices below all take the decoded volume
    lung_mask, found = _computed_lungs(ct, lungs, lung_mask, airway_tree)
    vol, lv, truth_mask, z0, z1, S, x, info, R1, R2, has, sec = _prepare_segmentation(ct, lung_mask, truth, img_size, trim, lambda: int(getattr(model, "h", None) or model.base.h))
    sec.update(found[1])
    X, Y, Z = vol.raw.shape
    t0 = time.perf_counter()
    prob = torch.from_numpy(np.ascontiguousarray(model.predict(x, batch_size=batch_size), np.float32)).cuda()
    torch.cuda.synchronize(); sec["predict"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    canvas = paste_back(prob, R1, R2, S)
    mask_dev, counts_dev = unslice(canvas, threshold, (X, Y, Z), z0, z1)
    return _finish_segmentation(vol, lv, truth_mask, mask_dev, counts_dev, z0, z1, has, info, threshold, sec, t0, postprocess, min_lesion_ml, lesions, connectivity, out_path,
                                density=density, per_lung=per_lung, render=render, mesh=mesh, distribution=distribution, vessels=vessels, split_lesions=split_lesions,
                                **found[0])


def _finish_segmentation(vol, lv, truth_mask, mask_dev, counts_dev, z0, z1, has, info, threshold, sec, t0, postprocess, min_lesion_ml, lesions, connectivity, out_path,
                         density=None, per_lung=None, render=None, mesh=None, distribution=None, vessels=None, split_lesions=None, **extra):
    """What segment_volume and segment_volume_ensemble do with the mask volume once it is formed (mask_dev, counts_dev [z1 - z0], both on the device): postprocess,
    min_lesion_ml / lesions, density (the checked keyword arguments of intensity_stats, or None), per_lung (those of split_lungs, or None), render (those of the sheet, or None), mesh (the checked dict of _check_mesh, or None), distribution (the checked pair of _check_distribution, or None), truth, the download, the lung share and out_path -> VolumeSegmentation (+ `extra` fields).  t0: when the paste-back began."""
    torch = _torch()
    X, Y, Z = vol.raw.shape
    voxel_mm3 = float(np.prod(np.asarray(vol.pixdim, np.float64)))          # count * prod(pixdim) / 1000 = millilitres
    cz0, cz1 = z0, z1                                               # the slices counts_dev speaks about
    postprocess_ml = None
    if postprocess is not None:
        torch.cuda.synchronize(); tp = time.perf_counter()
        before = int(counts_dev.sum().item())
        mask_dev, cleaned = postprocess_device(mask_dev, (X, Y, Z), postprocess, vol.pixdim)
        if cleaned is not None:
            counts_dev, cz0, cz1 = cleaned, 0, Z
        postprocess_ml = float(int(counts_dev.sum().item()) - before) * voxel_mm3 / 1000.0
        torch.cuda.synchronize(); sec["postprocess"] = time.perf_counter() - tp
    table, removed_ml = None, None
    labels_dev, keep = None, None
    if min_lesion_ml is not None or lesions:
        torch.cuda.synchronize(); tc = time.perf_counter()
        labels_dev, n_comp = label_device(mask_dev, (X, Y, Z), connectivity)
        table = table_from_stats(component_stats_device(labels_dev, (X, Y, Z), n_comp), vol.pixdim)
        if min_lesion_ml is not None:
            before = int(counts_dev.sum().item())
            keep = np.zeros(n_comp + 1, bool)
            keep[1:] = table["voxels"] >= min_voxels_from_ml(min_lesion_ml, vol.pixdim)
            mask_dev, counts_dev = filter_components(labels_dev, keep, n_comp, (X, Y, Z), cz0, cz1)
            table = table[keep[1:]]                                  # the kept components keep their order: renumbered, this is the table of the filtered mask
            table["label"] = np.arange(1, len(table) + 1)
            removed_ml = float(before) * voxel_mm3 / 1000.0 - float(counts_dev.sum().item()) * voxel_mm3 / 1000.0
        if density is None and per_lung is None:                      # (distribution= needs per_lung=)
            labels_dev = None
        torch.cuda.synchronize(); sec["components"] = time.perf_counter() - tc
    if split_lesions is not None:                                   # (the fields exist only when it is asked for)
        torch.cuda.synchronize(); tw = time.perf_counter()
        extra.update(_segmentation_lesion_parts(split_lesions, mask_dev, (X, Y, Z), vol.pixdim))
        torch.cuda.synchronize(); sec["split_lesions"] = time.perf_counter() - tw
    dens, lung_dens = None, None
    if density is not None:
        torch.cuda.synchronize(); td = time.perf_counter()
        if labels_dev is not None:                                  # per lesion, on the labels the table came from; a filtered lesion's voxels left the mask (region=)
            dens = intensity_stats(vol, labels=labels_dev, n=n_comp, region=mask_dev if keep is not None else None, shape=(X, Y, Z), **density)
            if keep is not None:
                dens = dens.take_groups(keep[1:])
        else:
            dens = intensity_stats(vol, mask=mask_dev, shape=(X, Y, Z), **density)
        if lv is not None:
            lung_dens = intensity_stats(vol, mask=lv.get_fdata() != 0, **density)
        torch.cuda.synchronize(); sec["density"] = time.perf_counter() - td
    if vessels is not None:                                         # (the checked keyword arguments of vessels.vessel_mask; the fields exist only when it is asked for)
        torch.cuda.synchronize(); tv = time.perf_counter()
        extra.update(_segmentation_vessels(vessels, vol, lv, mask_dev, (X, Y, Z), density))
        torch.cuda.synchronize(); sec["vessels"] = time.perf_counter() - tv
    burden, burden_error = None, None
    distr, distr_error = None, None
    if per_lung is not None:
        torch.cuda.synchronize(); tl = time.perf_counter()
        kw = dict(per_lung)
        if kw.get("orientation") is None and lv.affine is None and vol.affine is not None:
            kw["orientation"] = vol.affine                          # the two files share one geometry
        kw.setdefault("pixdim", vol.pixdim)
        try:
            ls = split_lungs(lv, return_device=True, **kw)
        except LungSplitError as e:
            burden_error = str(e)
        else:
            if labels_dev is not None:                              # the labels the lesion table came from; a filtered lesion's rows go with it
                totals, les, ps = side_table_device(ls.sides, mask_dev, labels_dev, n_comp, (X, Y, Z))
                if keep is not None:
                    les = les[keep[1:]]
            else:
                own, n_own = label_device(mask_dev, (X, Y, Z), connectivity)
                totals, les, ps = side_table_device(ls.sides, mask_dev, own, n_own, (X, Y, Z))
                del own
            burden = burden_from_tables(totals, les, ps, vol.pixdim)
            if density is not None:
                burden.density = intensity_stats(vol, labels=ls.sides.to(torch.int32), n=2, shape=(X, Y, Z), **density)
            sides_dev = ls.sides
            ls.sides = ls.sides.cpu().numpy().reshape((X, Y, Z), order="F")
            burden.sides = ls
        torch.cuda.synchronize(); sec["per_lung"] = time.perf_counter() - tl
        if distribution is not None:
            td = time.perf_counter()
            if burden is None:
                distr_error = burden_error
            else:
                distr = _segmentation_distribution(distribution, ls, sides_dev, mask_dev, labels_dev, n_comp if labels_dev is not None else None, keep, (X, Y, Z), connectivity)
                del sides_dev
            torch.cuda.synchronize(); sec["distribution"] = time.perf_counter() - td
    labels_dev = None
    sheet = None
    if render is not None:
        torch.cuda.synchronize(); tr = time.perf_counter()
        kw = dict(render)
        per_slice = np.zeros(Z, np.int64); per_slice[cz0:cz1] = counts_dev.cpu().numpy()
        keys = key_slices(per_slice, kw.pop("n", 6)) or [Z // 2]
        over = [Layer(mask_dev, PALETTE_INFECTION, 128, 255)]
        if lv is not None:
            over.append(Layer((lv.get_fdata() != 0).astype(np.uint8), PALETTE_LUNG, 0, 255))
        sheet = render_planes(vol, [("axial", z) for z in keys] + [("mip", "coronal", 0, Y)], over, shape=(X, Y, Z), **kw)
        torch.cuda.synchronize(); sec["render"] = time.perf_counter() - tr
    surf, lung_surf = None, None
    if mesh is not None:
        torch.cuda.synchronize(); tm = time.perf_counter()
        surf, lung_surf = _segmentation_meshes(mesh, vol, lv, mask_dev, (X, Y, Z), connectivity)
        torch.cuda.synchronize(); sec["mesh"] = time.perf_counter() - tm
    score = None
    if truth_mask is not None:
        torch.cuda.synchronize(); ts = time.perf_counter()
        score = score_volume(mask_dev, truth_mask, vol.pixdim, lesion_connectivity=connectivity, shape=(X, Y, Z))
        torch.cuda.synchronize(); sec["score"] = time.perf_counter() - ts
    mask = mask_dev.cpu().numpy().reshape((X, Y, Z), order="F")
    counts = np.zeros(Z, np.int64); counts[cz0:cz1] = counts_dev.cpu().numpy()
    sec["paste_unslice"] = time.perf_counter() - t0
    res = VolumeSegmentation(mask=mask, counts=counts, voxel_ml=voxel_mm3 / 1000.0, ml_per_slice=counts * voxel_mm3 / 1000.0,
                             total_ml=float(counts.sum()) * voxel_mm3 / 1000.0, lung_ml=None,
                             infected_share=None, fell_through=[int(i) for i in np.nonzero(~has)[0]], flat=info["flat"], z0=z0, z1=z1, pixdim=vol.pixdim,
                             threshold=float(threshold), seconds=sec, lesions=table, n_lesions=None if table is None else len(table), removed_ml=removed_ml, score=score,
                             postprocess_ml=postprocess_ml, density=dens, lung_density=lung_dens, per_lung=burden, per_lung_error=burden_error, sheet=sheet, mesh=surf, lung_mesh=lung_surf,
                             distribution=distr, distribution_error=distr_error, **extra)
    if lv is not None:
        lung_vox = int(np.count_nonzero(lv.get_fdata()[:, :, z0:z1]))
        res.lung_ml = lung_vox * voxel_mm3 / 1000.0
        res.infected_share = (res.total_ml / res.lung_ml) if lung_vox else float("nan")
    if out_path is not None:
        nifti_min.write(out_path, mask, vol.header)
    return res


# ---- several models and test-time symmetries on one volume (csrc/kernels_ensemble.hip) ---------------------------------------
TTA = ("id", "rot90", "rot180", "rot270", "hflip", "vflip", "transpose", "antitranspose")          # unet_vol_dihedral's codes, by their numpy meaning on axes (1, 2)
DIHEDRAL_INVERSE = (0, 3, 2, 1, 4, 5, 6, 7)                         # rot90 <-> rot270; the others are their own inverses
MAX_MEMBERS = 32                                                    # one bit per member in a uint32 vote word


def _dihedral_code(code):
    if isinstance(code, str):
        if code not in TTA:
            raise ValueError(f"unknown symmetry {code!r}: one of {TTA}")
        return TTA.index(code)
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or not 0 <= code < len(TTA):
        raise ValueError(f"a symmetry is one of {TTA} or its index 0..7, not {code!r}")
    return int(code)


def dihedral_device(x, code):
    """unet_vol_dihedral on a float32 device tensor [n, d, d(, 1)] -> a new tensor of the same shape"""
    torch = _torch(); lib, ctx = _ctx()
    x = x.contiguous()
    out = torch.empty_like(x)
    ctx.check(lib.unet_vol_dihedral(ctx.handle, x.data_ptr(), x.shape[0], x.shape[1], int(code), out.data_ptr(), _stream()), "vol_dihedral")
    return out


def dihedral(x, code, inverse=False, return_device=False):
    """One of the eight symmetries of the square (TTA, by name or index) applied to every slice of x: [n, d, d] or [n, d, d, 1] float32, a numpy array or a device tensor.
    The result has x's shape and is a bit-exact copy: np.rot90(x, k, (1, 2)) for rot90 / rot180 / rot270, x[:, :, ::-1] for hflip, x[:, ::-1] for vflip, the swap of
    axes 1 and 2 for transpose and its rot180 for antitranspose.  inverse=True applies the symmetry that undoes `code`."""
    code = _dihedral_code(code)
    if inverse:
        code = DIHEDRAL_INVERSE[code]
    torch = _torch()
    shape = tuple(x.shape)
    if len(shape) not in (3, 4) or shape[1] != shape[2] or (len(shape) == 4 and shape[3] != 1):
        raise ValueError(f"dihedral takes [n, d, d] or [n, d, d, 1], not {shape}")
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32:
            raise ValueError(f"dihedral takes float32, not {x.dtype}")
        dev = x.cuda()
    else:
        a = np.asarray(x)
        if a.dtype != np.float32:
            raise ValueError(f"dihedral takes float32, not {a.dtype}")
        dev = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = dihedral_device(dev, code)
    return out if return_device else out.cpu().numpy()


def min_votes_of(rule, M):
    """The smallest number of votes that makes a voxel foreground: "majority" M // 2 + 1 (strict: a tie is background), "any" 1, "all" M, an int k with 1 <= k <= M."""
    if isinstance(rule, str):
        if rule not in ("majority", "any", "all"):
            raise ValueError(f"rule must be \"majority\", \"any\", \"all\" or an int in 1..{M}, not {rule!r}")
        return {"majority": M // 2 + 1, "any": 1, "all": M}[rule]
    if isinstance(rule, bool) or not isinstance(rule, (int, np.integer)) or not 1 <= rule <= M:
        raise ValueError(f"rule must be \"majority\", \"any\", \"all\" or an int in 1..{M}, not {rule!r}")
    return int(rule)


def vote_pack_device(mask_dev, member, words, first):
    """unet_vol_vote_pack: bit `member` of the uint32 vote words (an int32 device tensor of one element per voxel) = mask_dev != 0"""
    lib, ctx = _ctx()
    ctx.check(lib.unet_vol_vote_pack(ctx.handle, mask_dev.data_ptr(), int(member), 1 if first else 0, words.data_ptr(), mask_dev.numel(), _stream()), "vol_vote_pack")


def vote_reduce_device(words, M, shape, min_votes):
    """unet_vol_vote_reduce -> dict of device tensors: mask, votes (uint8, X*Y*Z in Fortran order), counts int64 [Z], member_voxels [M], pair [M, M], hist [M + 1]"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    N = X * Y * Z
    out = {"mask": torch.empty(N, dtype=torch.uint8, device="cuda"), "votes": torch.empty(N, dtype=torch.uint8, device="cuda"),
           "counts": torch.zeros(Z, dtype=torch.int64, device="cuda"), "member_voxels": torch.zeros(M, dtype=torch.int64, device="cuda"),
           "pair": torch.zeros((M, M), dtype=torch.int64, device="cuda"), "hist": torch.zeros(M + 1, dtype=torch.int64, device="cuda")}
    ctx.check(lib.unet_vol_vote_reduce(ctx.handle, words.data_ptr(), M, X, Y, Z, int(min_votes), out["mask"].data_ptr(), out["votes"].data_ptr(), out["counts"].data_ptr(),
                                       out["member_voxels"].data_ptr(), out["pair"].data_ptr(), out["hist"].data_ptr(), _stream()), "vol_vote_reduce")
    return out


def pairwise_dice(pair):
    """2 pair[a, b] / (v_a + v_b) with v = diag(pair): float64 [M, M], NaN where both members are empty"""
    pair = np.asarray(pair, np.int64)
    v = np.diag(pair).astype(np.float64)
    den = v[:, None] + v[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, 2.0 * pair.astype(np.float64) / den, np.nan)


class VoteResult:
    """What vote_volume returns.  mask: uint8 [X, Y, Z], votes >= min_votes; votes: uint8 [X, Y, Z], the members that marked each voxel (both numpy in Fortran order, or
    flat device tensors with return_device=True); counts int64 [Z]: the mask's voxels per slice; member_voxels int64 [M]; pair int64 [M, M]: the voxels two members
    share (its diagonal is member_voxels); pairwise_dice float64 [M, M]; hist int64 [M + 1]: the voxels with k votes; unanimous_voxels = hist[M];
    uncertain_voxels = sum(hist[1:M]): marked by some member but not by all; min_votes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _vote_stats(r, M, min_votes):
    pair, hist = r["pair"].cpu().numpy(), r["hist"].cpu().numpy()
    return dict(counts=r["counts"].cpu().numpy(), member_voxels=r["member_voxels"].cpu().numpy(), pair=pair, pairwise_dice=pairwise_dice(pair), hist=hist,
                unanimous_voxels=int(hist[M]), uncertain_voxels=int(hist[1:M].sum()), min_votes=int(min_votes))


def vote_volume(masks, rule="majority", return_device=False, shape=None):
    """Up to 32 mask volumes of one geometry (several models' or several raters' masks of one CT) -> VoteResult: the consensus mask under `rule` ("majority": more than
    half, a tie is background; "any"; "all"; an int k: at least k votes), the per-voxel vote count and how far the members agree.  masks: a list of numpy [X, Y, Z]
    arrays (bool / integer, foreground = non-zero) or flat device byte tensors with shape=, as the other functions of this module take them.  Each mask is packed into
    one bit of a 32-bit word per voxel (unet_vol_vote_pack); one pass over the words (unet_vol_vote_reduce) gives everything else in integer arithmetic."""
    torch = _torch()
    try:
        masks = list(masks)
    except TypeError:
        raise ValueError(f"masks is a list of mask volumes, not {masks!r}") from None
    M = len(masks)
    if M == 0:
        raise ValueError("vote_volume needs at least one mask")
    if M > MAX_MEMBERS:
        raise ValueError(f"vote_volume takes at most {MAX_MEMBERS} masks (one bit each in a 32-bit word), not {M}")
    min_votes = min_votes_of(rule, M)
    said = None
    for m in masks:                                                 # refused before anything is uploaded or launched
        _check_mask_host(m, shape)
        sh = tuple(int(v) for v in shape) if isinstance(m, torch.Tensor) else tuple(np.shape(m))
        if said is not None and sh != said:
            raise ValueError(f"the masks have different shapes: {said} and {sh}")
        said = sh
    _check_volume_dims(said)
    N = int(np.prod(said))
    words = torch.empty(N, dtype=torch.int32, device="cuda")
    for k, m in enumerate(masks):
        dev, _ = _mask_to_device(m, shape)
        vote_pack_device(dev, k, words, k == 0)
        del dev
    r = vote_reduce_device(words, M, said, min_votes)
    conv = (lambda t: t) if return_device else (lambda t: t.cpu().numpy().reshape(said, order="F"))
    return VoteResult(mask=conv(r["mask"]), votes=conv(r["votes"]), shape=said, **_vote_stats(r, M, min_votes))


def canvas_axpy_device(canvas, w, acc, first):
    """unet_vol_canvas_axpy: acc = first ? w canvas : acc + w canvas, the product and the sum rounded to float32 on their own"""
    lib, ctx = _ctx()
    ctx.check(lib.unet_vol_canvas_axpy(ctx.handle, canvas.data_ptr(), float(np.float32(w)), acc.data_ptr(), canvas.numel(), 1 if first else 0, _stream()), "vol_canvas_axpy")


def canvas_div_device(acc, denom):
    """unet_vol_canvas_div: acc /= denom in place, the correctly rounded float32 quotient"""
    lib, ctx = _ctx()
    ctx.check(lib.unet_vol_canvas_div(ctx.handle, acc.data_ptr(), float(np.float32(denom)), acc.numel(), _stream()), "vol_canvas_div")


def unslice_prob(canvas, shape, z0, z1):
    """unet_vol_unslice_prob: canvas [z1 - z0, S, S] -> float32 device tensor of X*Y*Z elements in Fortran order: the value unslice compares with its threshold"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = (int(v) for v in shape)
    canvas = canvas.contiguous()
    prob = torch.empty(X * Y * Z, dtype=torch.float32, device="cuda")
    ctx.check(lib.unet_vol_unslice_prob(ctx.handle, canvas.data_ptr(), canvas.shape[1], X, Y, Z, z0, z1, prob.data_ptr(), _stream()), "vol_unslice_prob")
    return prob


def models_from_weights(paths, input_size, **kw):
    """One UNetModel(input_size, **kw) per weight file (.hdf5 / .h5 / .npz, what model.save_weights and the k-fold runners write: unet_covid_fold1.hdf5 ...), each
    with its file loaded: the `models` argument of segment_volume_ensemble."""
    from .keras_like import UNetModel
    paths = [os.fspath(p) for p in paths]
    if not paths:
        raise ValueError("models_from_weights needs at least one weight file")
    for p in paths:
        if not p.lower().endswith((".hdf5", ".h5", ".npz")):
            raise ValueError(f"{p!r} is not a .hdf5, .h5 or .npz weight file")
        if not os.path.exists(p):
            raise ValueError(f"weight file {p!r} does not exist")
    models = []
    for p in paths:
        m = UNetModel(int(input_size), **kw)
        m.load_weights(p)
        m.verbose = 0
        models.append(m)
    return models


def _check_ensemble(models, tta, combine, weights):
    """-> (models, members [(model index, tta name)], member weights float32 [M], wsum float32, min_votes or None for combine="mean", the models' input size); every
    refusal is a ValueError raised before any device work"""
    try:
        models = list(models)
    except TypeError:
        raise ValueError(f"models is a list of models, not {models!r}") from None
    if not models:
        raise ValueError("segment_volume_ensemble needs at least one model")
    if isinstance(tta, str):
        tta = (tta,)
    tta = tuple(tta)
    if not tta:
        raise ValueError("tta needs at least one symmetry (\"id\")")
    for name in tta:
        if not isinstance(name, str) or name not in TTA:
            raise ValueError(f"unknown tta symmetry {name!r}: one of {TTA}")
    if len(set(tta)) != len(tta):
        raise ValueError(f"tta repeats a symmetry: {tta}")
    M = len(models) * len(tta)
    if M > MAX_MEMBERS:
        raise ValueError(f"{len(models)} models x {len(tta)} symmetries = {M} members; at most {MAX_MEMBERS} (one bit each in a 32-bit vote word)")
    if weights is None:
        w = np.ones(len(models), np.float32)
    else:
        try:
            w = np.asarray(list(weights), np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"weights is one number per model, not {weights!r}") from None
        if w.shape != (len(models),):
            raise ValueError(f"weights has one entry per model ({len(models)}), not {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError(f"weights are finite and not negative, not {weights!r}")
    sizes = []
    for m in models:
        h = getattr(m, "h", None) or getattr(getattr(m, "base", None), "h", None)
        if h is None:
            raise ValueError(f"{m!r} has no input size (h): not a model segment_volume accepts")
        sizes.append(int(h))
    if len(set(sizes)) != 1:
        raise ValueError(f"the models have different input sizes: {sizes}")
    members = [(i, name) for i in range(len(models)) for name in tta]
    mw = np.asarray([w[i] for i, _ in members], np.float32)
    wsum = np.float32(0.0)
    for v in mw:                                                    # the float32 sum in member order
        wsum = np.float32(wsum + v)
    if not wsum > 0:
        raise ValueError("the weights sum to 0")
    min_votes = None
    if not (isinstance(combine, str) and combine == "mean"):
        try:
            min_votes = min_votes_of(combine, M)
        except ValueError:
            raise ValueError(f"combine must be \"mean\", \"majority\", \"any\", \"all\" or an int in 1..{M}, not {combine!r}") from None
    return models, members, mw, wsum, min_votes, sizes[0]


def _predict_device(model, x, batch_size):
    """the model's probabilities for the device batch x as a float32 device tensor: predict_device where the model has one, else predict and an upload"""
    torch = _torch()
    if hasattr(model, "predict_device"):
        return model.predict_device(x, batch_size=batch_size).to(device="cuda", dtype=torch.float32)
    return torch.from_numpy(np.ascontiguousarray(model.predict(x, batch_size=batch_size), np.float32)).cuda()


def segment_volume_ensemble(ct, models, tta=("id",), combine="mean", weights=None, lung_mask=None, threshold=0.547, batch_size=32, out_path=None, img_size=512,
                            trim=(0.2, 0.8), min_lesion_ml=None, connectivity=1, lesions=False, truth=None, postprocess=None, return_prob=False, prob_path=None,
                            votes_path=None, density=None, per_lung=None, render=None, mesh=None, distribution=None, lungs=None):
    """segment_volume with several members: every (model, symmetry) pair of `models` (each anything segment_volume accepts, all of one input size) and `tta` (names of
    TTA, no repeats), in model-major order, at most 32.  A member sees the prepared batch under its symmetry (transformed once, on the device), its probabilities are
    transformed back, pasted onto the canvas and (a) thresholded into the member's mask, which becomes one bit of a vote word per voxel, (b) added into the weighted
    mean canvas: acc = w_0 c_0, acc = acc + w_m c_m in member order, then acc / wsum, every float32 operation rounded on its own (weights: one per model, None: all 1;
    wsum: the float32 sum of the member weights in order).  combine="mean": the final mask is the thresholded mean probability; "majority" / "any" / "all" / int k: the
    members' masks voted (vote_volume's rules).  Everything after the mask is formed -- postprocess, min_lesion_ml, lesions, density, per_lung, distribution, render, mesh, truth, out_path, the lung share -- is
    segment_volume's, and so are the result's fields.  Added: members [(model index, tta name)], votes (uint8 [X, Y, Z]: how many members marked the voxel),
    member_ml, pairwise_dice, vote_hist (voxels with k votes), unanimous_ml (all members), uncertain_ml (some but not all), combine, seconds["members"] (predict time per
    member), and prob (float32 [X, Y, Z], the mean probability in patient space) with return_prob=True or prob_path (None otherwise).  prob_path / votes_path: those two
    volumes as .nii / .nii.gz with the CT's header.  The vote statistics describe the members' masks at `threshold` in both modes (combine="mean" counts them under the
    majority rule).  One member ("id",) with combine="mean" and weight 1 is segment_volume bit for bit.  Under data parallelism every rank runs every member."""
    _check_connectivity(connectivity)
    lungs = _check_lungs(lungs, lung_mask)
    lung_mask = True if lungs is not None else lung_mask
    mesh = _check_mesh(mesh, lung_mask)
    models, members, mw, wsum, min_votes, d = _check_ensemble(models, tta, combine, weights)
    density = _check_density(density)
    per_lung = _check_per_lung(per_lung, lung_mask)
    distribution = _check_distribution(distribution, per_lung)
    render = _check_render(render)
    if postprocess is not None:
        _check_steps(postprocess, (1.0, 1.0, 1.0))
    torch = _torch()
    M = len(members)
    lung_mask, found = _computed_lungs(ct, lungs, lung_mask)
    vol, lv, truth_mask, z0, z1, S, x, info, R1, R2, has, sec = _prepare_segmentation(ct, lung_mask, truth, img_size, trim, lambda: d)
    sec.update(found[1])
    X, Y, Z = vol.raw.shape
    _check_volume_dims((X, Y, Z))
    sec["members"] = []
    t0 = time.perf_counter()
    words = torch.empty(X * Y * Z, dtype=torch.int32, device="cuda")
    acc = torch.empty((z1 - z0, S, S), dtype=torch.float32, device="cuda")
    batches = {"id": x}
    for k, (mi, name) in enumerate(members):
        if name not in batches:                                     # each symmetry of the batch is made once and serves every model
            batches[name] = dihedral_device(x, TTA.index(name))
        torch.cuda.synchronize(); tm = time.perf_counter()
        prob = _predict_device(models[mi], batches[name], batch_size)
        torch.cuda.synchronize(); sec["members"].append(time.perf_counter() - tm)
        if name != "id":
            prob = dihedral_device(prob, DIHEDRAL_INVERSE[TTA.index(name)])
        canvas = paste_back(prob, R1, R2, S)
        member_mask, _ = unslice(canvas, threshold, (X, Y, Z), z0, z1)
        vote_pack_device(member_mask, k, words, k == 0)
        canvas_axpy_device(canvas, mw[k], acc, k == 0)
        del prob, canvas, member_mask
    del batches
    torch.cuda.synchronize()
    sec["predict"] = float(sum(sec["members"])); sec["member_loop"] = time.perf_counter() - t0          # member_loop: predict + symmetries, paste-back, unslice, pack, axpy
    t0 = time.perf_counter()
    canvas_div_device(acc, wsum)
    mask_dev, counts_dev = unslice(acc, threshold, (X, Y, Z), z0, z1)
    prob_dev = unslice_prob(acc, (X, Y, Z), z0, z1) if (return_prob or prob_path is not None) else None
    del acc
    r = vote_reduce_device(words, M, (X, Y, Z), min_votes if min_votes is not None else min_votes_of("majority", M))
    del words
    if min_votes is not None:
        mask_dev, counts_dev = r["mask"], r["counts"][z0:z1].contiguous()          # no member marks a trimmed slice
    st = _vote_stats(r, M, min_votes if min_votes is not None else min_votes_of("majority", M))
    voxel_ml = float(np.prod(np.asarray(vol.pixdim, np.float64))) / 1000.0
    votes = r["votes"].cpu().numpy().reshape((X, Y, Z), order="F")
    prob = None if prob_dev is None else prob_dev.cpu().numpy().reshape((X, Y, Z), order="F")
    del r, prob_dev
    extra = dict(members=members, votes=votes, member_ml=st["member_voxels"].astype(np.float64) * voxel_ml, pairwise_dice=st["pairwise_dice"], vote_pair=st["pair"],
                 vote_hist=st["hist"], unanimous_ml=float(st["unanimous_voxels"]) * voxel_ml, uncertain_ml=float(st["uncertain_voxels"]) * voxel_ml, combine=combine,
                 weights=mw, prob=prob, **found[0])
    res = _finish_segmentation(vol, lv, truth_mask, mask_dev, counts_dev, z0, z1, has, info, threshold, sec, t0, postprocess, min_lesion_ml, lesions, connectivity, out_path,
                               density=density, per_lung=per_lung, render=render, mesh=mesh, distribution=distribution, **extra)
    if prob_path is not None:
        nifti_min.write(prob_path, prob, vol.header)
    if votes_path is not None:
        nifti_min.write(votes_path, votes, vol.header)
    return res


# ---- what the CT holds under a mask (csrc/kernels_intensity.hip) ---------------------------------------------------------------
# The default value bands: conventional thresholds of the CT densitometry literature in Hounsfield units -- below -950 (emphysema-like / air), -950 .. -750 (well aerated
# lung), -750 .. -300 (ground-glass opacity), -300 .. 50 (consolidation), above.  They are configurable (edges=, names=) and NOT clinically validated here; they mean
# Hounsfield units only when the file's slope / inter decode to them.  A band holds edge[b - 1] <= v < edge[b].
HU_BAND_NAMES = ("below", "aerated", "ggo", "consolidation", "above")
HU_BAND_EDGES = (-950.0, -750.0, -300.0, 50.0)
HU_BANDS = (HU_BAND_NAMES, HU_BAND_EDGES)
INTENSITY_MAX_EDGES = _lib.INTENSITY_MAX_EDGES                       # UNET_VOL_INTENSITY_MAX_EDGES
_DENSITY_KEYS = {"edges", "names", "percentiles", "moments", "per_slice"}


def intensity_group_dtype(n_bands, n_percentiles):
    """one row of IntensityStats.groups for B bands and Q percentiles"""
    B, Q = int(n_bands), int(n_percentiles)
    return np.dtype([("label", np.int32), ("voxels", np.int64), ("nan_voxels", np.int64), ("ml", np.float64), ("min", np.float64), ("max", np.float64),
                     ("mean", np.float64), ("std", np.float64), ("percentiles", np.float64, (Q,)), ("band_voxels", np.int64, (B,)), ("band_ml", np.float64, (B,)),
                     ("band_share", np.float64, (B,)), ("dominant_band", np.int32)])


class IntensityStats:
    """What intensity_stats returns.  names / edges: the B = len(edges) + 1 bands; qs: the percentiles asked for; n: the number of groups.  Of the union of the groups:
    voxels (taking-part voxels, NaN ones included), nan_voxels, ml, min, max, mean, std (population), percentiles {q: value} -- all over the non-NaN values, nan when
    there is none, mean / std / percentiles None with moments=False --, band_voxels / band_ml / band_share [B] (share of the non-NaN voxels), slice_band_voxels [Z, B]
    and slice_nan_voxels [Z] (None with per_slice=False).  groups: one row per label 1..n (intensity_group_dtype): the same quantities + dominant_band (the band with
    the most voxels, ties to the lower band, -1 for a group without values); with moments=False its mean / std / percentiles are nan."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def band(self, name):
        """the union's voxel count of the named band"""
        return int(self.band_voxels[self.names.index(name)])

    def take_groups(self, keep):
        """the same statistics with only the rows of `keep` (bool [n]), renumbered 1..; for rows that hold no voxel (the union does not change)"""
        keep = np.asarray(keep, bool)
        if keep.shape != (len(self.groups),) or self.groups["voxels"][~keep].any() or self.groups["nan_voxels"][~keep].any():
            raise ValueError("take_groups drops empty groups only")
        g = self.groups[keep].copy()
        g["label"] = np.arange(1, len(g) + 1)
        return IntensityStats(**{**self.__dict__, "groups": g, "n": len(g)})

    def __repr__(self):
        return f"IntensityStats(voxels={self.voxels}, mean={self.mean}, bands={dict(zip(self.names, self.band_voxels.tolist()))})"


def _check_intensity_args(edges=HU_BAND_EDGES, names=HU_BAND_NAMES, percentiles=(5, 25, 50, 75, 95), moments=True, per_slice=True):
    """-> (edges float64 [E], names tuple [E + 1], percentiles tuple of float), or ValueError: no device is needed"""
    try:
        e = np.asarray(edges, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"edges are finite ascending numbers, not {edges!r}") from None
    if not 1 <= e.size <= INTENSITY_MAX_EDGES:
        raise ValueError(f"1 to {INTENSITY_MAX_EDGES} edges are taken, not {e.size}")
    if not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise ValueError(f"edges must be finite and strictly ascending, not {edges!r}")
    if names is None:
        names = tuple(f"band{b}" for b in range(e.size + 1))
    names = tuple(str(v) for v in names)
    if len(names) != e.size + 1:
        raise ValueError(f"{e.size} edges make {e.size + 1} bands, but {len(names)} names were given")
    try:
        qs = tuple(float(q) for q in percentiles)
    except (TypeError, ValueError):
        raise ValueError(f"percentiles are numbers in [0, 100], not {percentiles!r}") from None
    if any(not 0.0 <= q <= 100.0 for q in qs):                      # (a NaN fails both comparisons)
        raise ValueError(f"a percentile must lie in [0, 100], not {percentiles!r}")
    return e, names, qs


def _check_density(density):
    """segment_volume's density= -> None (off) or the checked keyword arguments of intensity_stats"""
    if density is None or density is False:
        return None
    kw = {} if density is True else dict(density)
    if set(kw) - _DENSITY_KEYS:
        raise ValueError(f"density takes {sorted(_DENSITY_KEYS)}, not {sorted(set(kw) - _DENSITY_KEYS)}")
    _check_intensity_args(**kw)
    return kw


def _check_group_volume(a, what, vshape, shape, want_dtype):
    """a mask / label / region volume against the CT's shape, on the host: numpy [X, Y, Z] (bool / integer) or a flat device tensor with shape="""
    torch = _torch()
    if isinstance(a, torch.Tensor):
        if shape is None:
            raise ValueError(f"device {what} is a flat Fortran-order buffer: pass shape=(X, Y, Z)")
        if tuple(int(v) for v in shape) != vshape:
            raise ValueError(f"{what} is {tuple(shape)}, the CT {vshape}")
        if a.dtype != want_dtype or not a.is_cuda or a.numel() != int(np.prod(vshape)):
            raise ValueError(f"device {what} is a {want_dtype} cuda tensor of prod(shape) = {int(np.prod(vshape))} elements")
        return
    a = np.asarray(a)
    if a.ndim != 3:
        raise ValueError(f"a volume is [X, Y, Z]; {what} has {a.ndim} dimensions")
    if a.dtype.kind not in "biu":
        raise ValueError(f"{what} has a bool or integer dtype, not {a.dtype}")
    if tuple(a.shape) != vshape:
        raise ValueError(f"{what} is {tuple(a.shape)}, the CT {vshape}")


def _vox_args(vol):
    """the arguments that describe an uploaded volume to the intensity kernels: dtype code, X, Y, Z, scaled, slope, inter"""
    X, Y, Z = (int(v) for v in vol.raw.shape)
    sc = vol.scaling
    return (_CODE_OF_DTYPE[vol.raw.dtype.str[1:]], X, Y, Z, 1 if sc else 0, sc[0] if sc else 1.0, sc[1] if sc else 0.0)


_CODE_OF_DTYPE = {v: k for k, v in nifti_min.DTYPES.items()}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def intensity_bands_device(vol, dev, labels_dev, mask_dev, n, region_dev, edges, per_slice=True, minmax=True):
    """unet_vol_intensity_bands on an uploaded volume (dev = upload(vol)) -> (band_counts int64 [n, B + 1], slice_counts int64 [Z, B + 1] or None,
    minmax float64 [n, 2] or None), numpy; column B counts NaN voxels."""
    torch = _torch(); lib, ctx = _ctx()
    e = np.ascontiguousarray(edges, np.float64)
    W, Z = e.size + 2, int(vol.raw.shape[2])
    bc = torch.empty((max(n, 1), W), dtype=torch.int64, device="cuda")
    sc = torch.empty((max(Z, 1), W), dtype=torch.int64, device="cuda") if per_slice else None
    mm = torch.empty((max(n, 1), 2), dtype=torch.float64, device="cuda") if minmax else None
    ctx.check(lib.unet_vol_intensity_bands(ctx.handle, dev.data_ptr(), *_vox_args(vol), _ptr(labels_dev), _ptr(mask_dev), int(n), _ptr(region_dev), e.ctypes.data, e.size,
                                           bc.data_ptr(), _ptr(sc), _ptr(mm), _stream()), "vol_intensity_bands")
    return bc[:n].cpu().numpy(), (sc[:Z].cpu().numpy() if per_slice else None), (mm[:n].cpu().numpy() if minmax else None)


def intensity_gather_device(vol, dev, labels_dev, mask_dev, n, region_dev, capacity, want_groups=True, values=None, groups=None):
    """unet_vol_intensity_gather -> (count, values, groups): the number of taking-part non-NaN voxels and device tensors of min(count, capacity) doubles / int32 group
    numbers (None without want_groups), in no particular order.  values / groups: buffers of the caller's to write into (at least `capacity` elements)."""
    torch = _torch(); lib, ctx = _ctx()
    capacity = int(capacity)
    if values is None:
        values = torch.empty(max(capacity, 1), dtype=torch.float64, device="cuda")
    if groups is None and want_groups:
        groups = torch.empty(max(capacity, 1), dtype=torch.int32, device="cuda")
    if values.numel() < capacity or (groups is not None and groups.numel() < capacity):
        raise ValueError(f"the gather buffers hold fewer than capacity = {capacity} elements")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_intensity_gather(ctx.handle, dev.data_ptr(), *_vox_args(vol), _ptr(labels_dev), _ptr(mask_dev), int(n), _ptr(region_dev), values.data_ptr(),
                                            _ptr(groups), capacity, count.data_ptr(), _stream()), "vol_intensity_gather")
    c = int(count.item())
    k = min(c, capacity)
    return c, values[:k], (groups[:k] if groups is not None else None)


def group_moments_device(values_dev, offsets, n):
    """unet_vol_group_moments: values_dev ordered by (group, value), offsets int64 [n + 1] (numpy) -> float64 [n, 2] numpy: (sum, sum of squared deviations) per group"""
    torch = _torch(); lib, ctx = _ctx()
    n = int(n)
    off = np.ascontiguousarray(offsets, np.int64)
    if off.shape != (n + 1,) or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != values_dev.numel():
        raise ValueError(f"offsets are [n + 1] = {n + 1} non-decreasing positions from 0 to the number of values")
    if n == 0:
        return np.zeros((0, 2), np.float64)
    od = torch.from_numpy(off).cuda()
    out = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_group_moments_ws_bytes(int(off[-1]), n)), 16), dtype=torch.uint8, device="cuda")
    vals = values_dev.contiguous()
    ctx.check(lib.unet_vol_group_moments(ctx.handle, vals.data_ptr(), od.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "vol_group_moments")
    return out.cpu().numpy()


def sort_by_group_value(values, groups):
    """gathered (values, groups) -> (the values in ascending order, the values ordered by (group, value)): one sort of the values, then a stable sort by group"""
    torch = _torch()
    sv, order = torch.sort(values)
    if groups is None:
        return sv, sv
    _, perm = torch.sort(groups[order], stable=True)
    return sv, sv[perm]


def _order_statistics(run_dev, starts, sizes, qs):
    """np.percentile(run, qs) for every run [starts[g], + sizes[g]) of an ascending-per-run device tensor -> float64 [G, Q] (nan for an empty run): the two order
    statistics of every (run, q) come to the host in one indexing, the interpolation is numpy's linear rule (_lerp)"""
    torch = _torch()
    starts, sizes = np.asarray(starts, np.int64), np.asarray(sizes, np.int64)
    G, Q = starts.size, len(qs)
    out = np.full((G, Q), np.nan)
    if G == 0 or Q == 0 or not (sizes > 0).any():
        return out
    m1 = np.maximum(sizes - 1, 0).astype(np.float64)[:, None]
    pos = (np.asarray(qs, np.float64)[None, :] / 100.0) * m1
    lo = np.minimum(np.floor(pos).astype(np.int64), np.maximum(sizes - 1, 0)[:, None])
    hi = np.minimum(lo + 1, np.maximum(sizes - 1, 0)[:, None])
    idx = np.stack([starts[:, None] + lo, starts[:, None] + hi])
    idx = np.where((sizes > 0)[None, :, None], idx, 0)
    ab = run_dev[torch.from_numpy(np.ascontiguousarray(idx.reshape(-1))).cuda()].cpu().numpy().reshape(2, G, Q)
    r = _lerp(ab[0], ab[1], pos - lo)
    out[sizes > 0] = r[sizes > 0]
    return out


def _moment_fields(sums, sizes):
    """(sum, ssd) [G, 2] and the run lengths -> (mean, population std), nan for an empty run"""
    m = np.asarray(sizes, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(m > 0, sums[:, 0] / m, np.nan)
        std = np.where(m > 0, np.sqrt(sums[:, 1] / m), np.nan)
    return mean, std


def intensity_stats(ct, mask=None, labels=None, n=None, region=None, edges=HU_BAND_EDGES, names=HU_BAND_NAMES, percentiles=(5, 25, 50, 75, 95), moments=True,
                    per_slice=True, shape=None):
    """What the CT holds where a mask is set -> IntensityStats.  ct: a path, a NiftiVolume or an [X, Y, Z] array (as for segment_volume); its raw voxels are uploaded and
    decoded on the device as get_fdata() decodes them.  Exactly one of mask (non-zero = the one group) and labels (int, groups 1..n, n given; other labels take no part);
    region: only voxels where it is non-zero take part.  mask / labels / region: numpy [X, Y, Z] arrays (bool / integer), or flat device tensors in Fortran order (uint8 /
    int32 / uint8, what unslice and label_volume return) with shape=.  edges / names: the value bands (default HU_BANDS: conventional literature thresholds in Hounsfield
    units, configurable, not clinically validated here); band b of a value = np.searchsorted(edges, v, side="right").  A NaN voxel is counted in nan_voxels and nowhere else.
    Counts, min and max are exact.  mean, std and percentiles come from one sort of the gathered values on the device: a percentile is np.percentile's (linear) on the
    two order statistics; sum and sum of squared deviations are the fixed two-level tree of unet_vol_group_moments over the ascending values, so they are the same bits on
    every run.  moments=False skips gather and sort (mean, std, percentiles: None); per_slice=False skips the per-slice counts.  Every argument error is a ValueError
    raised before anything is uploaded or launched."""
    torch = _torch()
    e, names, qs = _check_intensity_args(edges, names, percentiles)
    if (mask is None) == (labels is None):
        raise ValueError("pass exactly one of mask, labels")
    if labels is not None and n is None:
        raise ValueError("labels need n, the number of groups (what label_volume returned)")
    n = 1 if labels is None else int(n)
    if n < 0:
        raise ValueError(f"n is the number of groups, not {n}")
    vol = _source(ct)
    vshape = tuple(int(v) for v in vol.raw.shape)
    _check_volume_dims(vshape)
    for a, what, dt in ((mask, "the mask", torch.uint8), (labels, "the label volume", torch.int32), (region, "the region", torch.uint8)):
        if a is not None:
            _check_group_volume(a, what, vshape, shape, dt)
    X, Y, Z = vshape
    def flat(a):                                                    # (a volume without voxels still hands the entry points a buffer: null means "not given" there)
        a = torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F")).cuda() if not isinstance(a, torch.Tensor) else a.contiguous().reshape(-1)
        return a if a.numel() else torch.zeros(16, dtype=a.dtype, device="cuda")
    as_bytes = lambda a: flat(a if isinstance(a, torch.Tensor) else (np.asarray(a) != 0).astype(np.uint8))
    mask_dev = as_bytes(mask) if mask is not None else None
    region_dev = as_bytes(region) if region is not None else None
    labels_dev = None
    if labels is not None:
        if isinstance(labels, torch.Tensor):
            labels_dev = flat(labels)
        else:
            a = np.asarray(labels)
            labels_dev = flat(np.where((a >= 1) & (a <= n), a, 0).astype(np.int32))          # a label outside 1..n takes no part: it must not wrap into the range
    dev = flat(upload(vol))
    B, Q = e.size + 1, len(qs)
    bc, sc, mm = intensity_bands_device(vol, dev, labels_dev, mask_dev, n, region_dev, e, per_slice=per_slice)
    sizes, nans = bc[:, :B].sum(axis=1), bc[:, B].copy()              # non-NaN / NaN voxels per group
    total = int(sizes.sum())
    voxel_ml = float(np.prod(np.asarray(vol.pixdim, np.float64))) / 1000.0
    t = np.zeros(n, intensity_group_dtype(B, Q))
    t["label"] = np.arange(1, n + 1)
    t["voxels"], t["nan_voxels"] = sizes + nans, nans
    t["ml"] = (sizes + nans) * voxel_ml
    t["min"], t["max"] = np.where(sizes > 0, mm[:, 0], np.nan), np.where(sizes > 0, mm[:, 1], np.nan)
    t["band_voxels"] = bc[:, :B]
    t["band_ml"] = bc[:, :B] * voxel_ml
    with np.errstate(invalid="ignore", divide="ignore"):
        t["band_share"] = np.where(sizes[:, None] > 0, bc[:, :B] / sizes[:, None].astype(np.float64), np.nan)
    t["dominant_band"] = np.where(sizes > 0, np.argmax(bc[:, :B], axis=1) if n else 0, -1)
    t["mean"] = t["std"] = np.nan
    t["percentiles"] = np.nan
    band = bc[:, :B].sum(axis=0)
    f = dict(names=names, edges=e, qs=qs, n=n, voxels=total + int(nans.sum()), nan_voxels=int(nans.sum()), ml=(total + int(nans.sum())) * voxel_ml,
             min=float(mm[:, 0].min()) if total else float("nan"), max=float(mm[:, 1].max()) if total else float("nan"), mean=None, std=None, percentiles=None,
             band_voxels=band, band_ml=band * voxel_ml, band_share=band / float(total) if total else np.full(B, np.nan),
             slice_band_voxels=sc[:, :B].copy() if per_slice else None, slice_nan_voxels=sc[:, B].copy() if per_slice else None, voxel_ml=voxel_ml)
    if moments:
        count, vals, grps = intensity_gather_device(vol, dev, labels_dev, mask_dev, n, region_dev, total, want_groups=n > 1)
        if count != total:
            raise _lib.UNetHipError(f"intensity_stats: the bands hold {total} values but {count} were gathered")
        sv, gv = sort_by_group_value(vals, grps)                    # plumbing, as in score_volume
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        gsum = group_moments_device(gv, off, n)
        t["mean"], t["std"] = _moment_fields(gsum, sizes)
        t["percentiles"] = _order_statistics(gv, off[:-1], sizes, qs)
        if n == 1:
            usum, upct = gsum, t["percentiles"]
        else:
            usum = group_moments_device(sv, np.array([0, total], np.int64), 1)
            upct = _order_statistics(sv, [0], [total], qs)
        um, us = _moment_fields(usum, [total])
        f.update(mean=float(um[0]), std=float(us[0]), percentiles={q: float(v) for q, v in zip(qs, upct[0])})
    return IntensityStats(groups=t, **f)


# ---- left and right lung (csrc/kernels_lungside.hip) ----------------------------------------------------------------------------
# The defaults of the split: a second component counts as the other lung once it holds min_ratio of the largest one's voxels, and the mask is eroded by these radii
# (mm, in order) until that happens.  Conventional values, configurable (min_ratio=, erode_mm=) and NOT clinically validated here.
LUNG_MIN_RATIO = 0.25
LUNG_ERODE_MM = (1, 2, 3, 4, 5, 6, 8, 10)
_PER_LUNG_KEYS = {"orientation", "pixdim", "connectivity", "min_ratio", "erode_mm"}
LUNG_LESION_DTYPE = np.dtype([("label", np.int32), ("voxels_outside", np.int64), ("voxels_left", np.int64), ("voxels_right", np.int64), ("side", "U5")])
SIDE_NAMES = ("none", "left", "right")                              # by side value 0, 1, 2


class LungSplitError(ValueError):
    """The lung mask cannot be told into a left and a right lung: no orientation, fewer than two large enough components at every radius, or two seeds at the same
    world x."""


class LungSides:
    """What split_lungs returns.  sides: uint8 [X, Y, Z], 0 off the mask, 1 = the patient's left lung, 2 = the right (numpy, Fortran order; return_device=True: the
    flat device tensor); shape; radius_mm: the erosion radius that separated the lungs (0: they were separate already); voxels / ml: (left, right); seed_voxels: (left,
    right) voxels of the two seeds; axcodes: the direction in which every voxel axis grows; pixdim."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"LungSides(radius_mm={self.radius_mm}, voxels={self.voxels}, axcodes={self.axcodes})"


class LungSideBurden:
    """One lung of a LungBurden: lung_voxels, infected_voxels, lung_ml, infected_ml, fraction = infected / lung (nan for an empty lung)."""

    def __init__(self, lung_voxels, infected_voxels, voxel_ml):
        self.lung_voxels, self.infected_voxels = int(lung_voxels), int(infected_voxels)
        self.lung_ml, self.infected_ml = self.lung_voxels * voxel_ml, self.infected_voxels * voxel_ml
        self.fraction = (self.infected_ml / self.lung_ml) if self.lung_voxels else float("nan")

    def __repr__(self):
        return f"LungSideBurden(lung_ml={self.lung_ml:.1f}, infected_ml={self.infected_ml:.1f}, fraction={self.fraction:.3f})"


class LungBurden:
    """What lung_burden returns.  left / right: LungSideBurden; outside_voxels / outside_ml: infected outside both lungs; lesions: LUNG_LESION_DTYPE rows (label,
    voxels_outside, voxels_left, voxels_right, side = "left" / "right" by where most of the lesion's in-lung voxels lie, a tie to left, "none" when no voxel of it lies in
    a lung); per_slice: int64 [Z, 6] = {lung left, lung right, infected outside, infected left, infected right, 0}; bilateral: both fractions > 0; voxel_ml.  From
    segment_volume(per_lung=): also sides (the LungSides, on the host) and density (IntensityStats with two rows, left then right; None without density=)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"LungBurden(left={self.left!r}, right={self.right!r}, outside_ml={self.outside_ml:.1f}, bilateral={self.bilateral})"


def _check_orientation(orientation):
    """split_lungs' orientation= -> (float64 3 x 3 linear part or None, axcodes or None): a 3-letter code string / tuple or an affine; ValueError otherwise"""
    if orientation is None:
        return None, None
    if isinstance(orientation, str) or (isinstance(orientation, (tuple, list)) and len(orientation) == 3 and all(isinstance(c, str) for c in orientation)):
        nifti_min.check_axcodes(orientation)
        return nifti_min.affine_from_axcodes(orientation)[:3, :3], tuple(str(c) for c in orientation)
    try:
        m = np.asarray(orientation, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"orientation is a 3-letter code such as 'LPS' or a 4 x 4 affine, not {orientation!r}") from None
    if m.shape != (4, 4):
        raise ValueError(f"orientation is a 3-letter code such as 'LPS' or a 4 x 4 affine, not an array of shape {m.shape}")
    try:
        codes = nifti_min.axcodes_from_affine(m)
    except nifti_min.NiftiFormatError as e:
        raise ValueError(f"orientation: {e}") from None
    return m[:3, :3].copy(), codes


def _check_split_args(orientation=None, pixdim=None, connectivity=1, min_ratio=LUNG_MIN_RATIO, erode_mm=LUNG_ERODE_MM):
    """-> (linear part or None, axcodes or None, pixdim float64 [3] or None, connectivity, min_ratio, radii), or ValueError: no device is needed"""
    lin, codes = _check_orientation(orientation)
    p = None if pixdim is None else _check_pixdim(pixdim)
    connectivity = _check_connectivity(connectivity)
    try:
        ratio = float(min_ratio)
    except (TypeError, ValueError):
        raise ValueError(f"min_ratio is a number in (0, 1], not {min_ratio!r}") from None
    if not 0.0 < ratio <= 1.0:
        raise ValueError(f"min_ratio is a number in (0, 1], not {min_ratio!r}")
    try:
        radii = tuple(_check_radius(r) for r in erode_mm)
    except TypeError:
        raise ValueError(f"erode_mm is a sequence of ascending radii in mm, not {erode_mm!r}") from None
    if any(r <= 0.0 for r in radii) or any(b <= a for a, b in zip(radii, radii[1:])):
        raise ValueError(f"erode_mm must be positive and strictly ascending, not {erode_mm!r}")
    return lin, codes, p, connectivity, ratio, radii


def _check_per_lung(per_lung, lung_mask):
    """segment_volume's per_lung= -> None (off) or the checked keyword arguments of split_lungs"""
    if per_lung is None or per_lung is False:
        return None
    kw = {} if per_lung is True else dict(per_lung)
    if set(kw) - _PER_LUNG_KEYS:
        raise ValueError(f"per_lung takes {sorted(_PER_LUNG_KEYS)}, not {sorted(set(kw) - _PER_LUNG_KEYS)}")
    _check_split_args(**kw)
    if lung_mask is None:
        raise ValueError("per_lung needs lung_mask: the lungs are split from it")
    return kw


def side_assign_device(mask_dev, d2_a, d2_b, shape, side_a=1, side_b=2):
    """unet_vol_side_assign -> (sides: uint8 device tensor of X*Y*Z bytes in Fortran order, counts int64 [3] numpy: the voxels holding 0, 1, 2)"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    _check_volume_dims(shape)
    sides = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_side_assign(ctx.handle, mask_dev.data_ptr(), d2_a.data_ptr(), d2_b.data_ptr(), X, Y, Z, int(side_a), int(side_b), sides.data_ptr(), counts.data_ptr(),
                                       _stream()), "vol_side_assign")
    return sides, counts.cpu().numpy()


def side_table_device(sides_dev, infection_dev, labels_dev, n, shape, per_slice=True):
    """unet_vol_side_table -> (totals int64 [2, 3], lesion_side int64 [n, 3], per_slice int64 [Z, 6] or None), numpy"""
    torch = _torch(); lib, ctx = _ctx()
    X, Y, Z = shape
    _check_volume_dims(shape)
    n = int(n)
    totals = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    les = torch.zeros((max(n, 1), 3), dtype=torch.int64, device="cuda")
    ps = torch.zeros((max(Z, 1), 6), dtype=torch.int64, device="cuda") if per_slice else None
    ctx.check(lib.unet_vol_side_table(ctx.handle, sides_dev.data_ptr(), _ptr(infection_dev), _ptr(labels_dev), n, X, Y, Z, totals.data_ptr(), les.data_ptr(), _ptr(ps), _stream()),
              "vol_side_table")
    return totals.cpu().numpy(), les[:n].cpu().numpy(), (ps[:Z].cpu().numpy() if per_slice else None)


def split_lungs(lung_mask, orientation=None, pixdim=None, connectivity=1, min_ratio=LUNG_MIN_RATIO, erode_mm=LUNG_ERODE_MM, return_device=False, shape=None, out_path=None):
    """A lung mask -> LungSides: which of its voxels belong to the patient's left lung (1) and which to the right (2).  lung_mask: a path, a NiftiVolume, a host array or
    a device uint8 volume with shape=; non-zero = lung.  orientation: None = the volume's own affine (its sform / qform), or a 3-letter code such as "LPS" (the direction
    in which every voxel axis grows), or a 4 x 4 affine; pixdim: the voxel's edge lengths in mm, default the volume's own.  Without an orientation from either, LungSplitError
    is raised before any device work: left and right are never guessed.
      1. Seeds.  For r = 0 and then every radius of erode_mm in order: c_r = the mask (r = 0) or erode_mm(mask, r, pixdim) -- one distance transform to the background,
         thresholded per radius --, labelled with `connectivity`; A and B = its two components of the most voxels (ties to the lower label).  The first r with at least two
         components and count(B) >= min_ratio * count(A) ends the search; no such r: LungSplitError naming the largest two counts seen.
      2. Which seed is left.  xw(c) = affine[0, :3] . centroid(c), centroid = sum / count in float64.  NIfTI's world is RAS+ (+x = the patient's right): the seed with the
         smaller xw is the patient's LEFT; equal values raise LungSplitError.
      3. Assignment.  Every non-zero voxel of the ORIGINAL mask gets side 1 when its exact squared distance (unet_vol_edt_sq, w = pixdim^2) to the left seed is <= the one
         to the right seed, else 2: a tie goes to the patient's left, whichever way the volume is stored.  The distance is Euclidean through the volume, not geodesic
         through the lung.
    min_ratio / erode_mm: conventional defaults (LUNG_MIN_RATIO, LUNG_ERODE_MM), configurable and not clinically validated here.  out_path: sides as .nii / .nii.gz with
    the source's header.  Every argument error is a ValueError raised before anything is uploaded or launched."""
    torch = _torch()
    lin, codes, p, connectivity, ratio, radii = _check_split_args(orientation, pixdim, connectivity, min_ratio, erode_mm)
    src = None
    if isinstance(lung_mask, torch.Tensor):
        _check_mask_host(lung_mask, shape)
    else:
        src = _source(lung_mask)
        if lin is None and src.affine is not None:
            try:
                lin, codes = src.affine[:3, :3].copy(), src.axcodes
            except nifti_min.NiftiFormatError as e:
                raise LungSplitError(f"split_lungs: {e}") from None
        if p is None:
            p = _check_pixdim(src.pixdim)
    if lin is None:
        raise LungSplitError("split_lungs: neither the lung mask nor orientation= says which voxel direction is the patient's left; pass orientation='LPS' (or the "
                             "volume's code) or an affine -- left and right are not guessed")
    if p is None:
        p = np.ones(3)
    if src is not None:
        dev, shape = _mask_to_device(src.get_fdata() != 0, None)
    else:
        dev, shape = _mask_to_device(lung_mask, shape)
    X, Y, Z = shape
    _check_volume_dims(shape)
    d2_bg = None
    best, found = (0, 0), None
    for r in (0.0,) + radii:
        if r == 0.0:
            cand = dev
        else:
            lib, ctx = _ctx()
            if d2_bg is None:
                d2_bg = edt_sq_device(dev, shape, p, features_nonzero=False)
            cand = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
            ctx.check(lib.unet_vol_ball(ctx.handle, d2_bg.data_ptr(), X, Y, Z, r * r, 0, cand.data_ptr(), None, _stream()), "vol_ball")
        labels, n = label_device(cand, shape, connectivity)
        st = component_stats_device(labels, shape, n)
        order = np.lexsort((np.arange(n), -st["voxels"].astype(np.int64)))[:2]          # the two largest, ties to the lower label
        counts = tuple(int(st["voxels"][k]) for k in order) + (0,) * (2 - len(order))
        if counts > best:
            best = counts
        if n >= 2 and float(counts[1]) >= ratio * float(counts[0]):
            found = (r, labels, n, st, order)
            break
    del d2_bg
    if found is None:
        raise LungSplitError(f"split_lungs: no erosion radius of {(0.0,) + radii} mm leaves two components with the second holding {ratio} of the first; the largest "
                             f"two counts seen were {best[0]} and {best[1]} voxels")
    r, labels, n, st, order = found
    xw = []
    for k in order:
        cnt = float(st["voxels"][k])
        c = (float(st["sx"][k]) / cnt, float(st["sy"][k]) / cnt, float(st["sz"][k]) / cnt)
        xw.append(float(lin[0, 0]) * c[0] + float(lin[0, 1]) * c[1] + float(lin[0, 2]) * c[2])
    if xw[0] == xw[1]:
        raise LungSplitError(f"split_lungs: the two seeds have the same world x ({xw[0]}): the orientation does not separate them")
    left, right = (order[0], order[1]) if xw[0] < xw[1] else (order[1], order[0])
    d2 = []
    for k in (left, right):
        keep = np.zeros(n + 1, bool)
        keep[k + 1] = True
        seed, _ = filter_components(labels, keep, n, shape, 0, 0)
        d2.append(edt_sq_device(seed, shape, p, features_nonzero=True))
        del seed
    del labels
    sides, cnt = side_assign_device(dev, d2[0], d2[1], shape, 1, 2)
    del d2
    voxel_ml = float(np.prod(p)) / 1000.0
    res = LungSides(sides=sides if return_device else sides.cpu().numpy().reshape(shape, order="F"), shape=shape, radius_mm=float(r), voxels=(int(cnt[1]), int(cnt[2])),
                    ml=(int(cnt[1]) * voxel_ml, int(cnt[2]) * voxel_ml), seed_voxels=(int(st["voxels"][left]), int(st["voxels"][right])), axcodes=codes,
                    pixdim=tuple(float(v) for v in p))
    if out_path is not None:
        host = res.sides.cpu().numpy().reshape(shape, order="F") if return_device else res.sides
        nifti_min.write(out_path, host, src.header if src is not None else None, res.pixdim)
    return res


def _lesion_sides(lesion_side):
    """int64 [n, 3] -> LUNG_LESION_DTYPE rows: the side holding most of the lesion's in-lung voxels, a tie to left, "none" when it has none"""
    t = np.zeros(len(lesion_side), LUNG_LESION_DTYPE)
    t["label"] = np.arange(1, len(t) + 1)
    t["voxels_outside"], t["voxels_left"], t["voxels_right"] = lesion_side[:, 0], lesion_side[:, 1], lesion_side[:, 2]
    code = np.where(lesion_side[:, 1] + lesion_side[:, 2] == 0, 0, np.where(lesion_side[:, 1] >= lesion_side[:, 2], 1, 2))
    t["side"] = np.asarray(SIDE_NAMES)[code] if len(t) else t["side"]
    return t


def burden_from_tables(totals, lesion_side, per_slice, pixdim=(1, 1, 1)):
    """the three tables of unet_vol_side_table -> LungBurden"""
    voxel_ml = float(np.prod(np.asarray(pixdim, np.float64))) / 1000.0
    left, right = LungSideBurden(totals[0, 1], totals[1, 1], voxel_ml), LungSideBurden(totals[0, 2], totals[1, 2], voxel_ml)
    return LungBurden(left=left, right=right, outside_voxels=int(totals[1, 0]), outside_ml=int(totals[1, 0]) * voxel_ml, lesions=_lesion_sides(np.asarray(lesion_side, np.int64)),
                      per_slice=per_slice, bilateral=bool(left.fraction > 0 and right.fraction > 0), voxel_ml=voxel_ml, sides=None, density=None)


def lung_burden(infection, sides, labels=None, n=None, pixdim=(1, 1, 1), connectivity=1, shape=None):
    """How much of each lung an infection mask takes -> LungBurden.  infection: a host [X, Y, Z] mask (non-zero = infected) or a flat device uint8 tensor with shape=;
    sides: a LungSides or a 0 / 1 / 2 volume of the same shape (host array, or device tensor with shape=); labels / n: the infection's lesions as label_volume returned
    them (host array or device int32 tensor) -- without them the infection mask is labelled here with `connectivity`; pixdim: the voxel's edge lengths in mm."""
    torch = _torch()
    p = _check_pixdim(pixdim)
    connectivity = _check_connectivity(connectivity)
    if labels is not None and n is None:
        raise ValueError("labels need n, the number of lesions (what label_volume returned)")
    if labels is not None and int(n) < 0:
        raise ValueError(f"n is the number of lesions, not {n}")
    if isinstance(sides, LungSides):
        sides_v, sides_shape = sides.sides, sides.shape
    else:
        sides_v, sides_shape = sides, shape
    _check_mask_host(infection, shape)
    _check_mask_host(sides_v, sides_shape)
    if not isinstance(sides_v, torch.Tensor) and not isinstance(infection, torch.Tensor) and np.asarray(sides_v).shape != np.asarray(infection).shape:
        raise ValueError(f"sides is {np.asarray(sides_v).shape}, the infection mask {np.asarray(infection).shape}")
    inf_dev, vshape = _mask_to_device(infection, shape)
    if isinstance(sides_v, torch.Tensor):
        if tuple(int(v) for v in sides_shape) != vshape or sides_v.dtype != torch.uint8 or sides_v.numel() != int(np.prod(vshape)):
            raise ValueError(f"device sides are a uint8 cuda tensor of the infection mask's shape {vshape}")
        sides_dev = sides_v.contiguous().reshape(-1)
    else:
        a = np.asarray(sides_v)
        if tuple(a.shape) != vshape:
            raise ValueError(f"sides is {tuple(a.shape)}, the infection mask {vshape}")
        sides_dev = torch.from_numpy(np.asfortranarray(np.where((a >= 0) & (a <= 2), a, 0).astype(np.uint8)).reshape(-1, order="F")).cuda()
    if labels is None:
        labels_dev, n = label_device(inf_dev, vshape, connectivity)
    elif isinstance(labels, torch.Tensor):
        if labels.dtype != torch.int32 or labels.numel() != int(np.prod(vshape)):
            raise ValueError(f"device labels are an int32 cuda tensor of the infection mask's shape {vshape}")
        labels_dev = labels.contiguous().reshape(-1)
    else:
        a = np.asarray(labels)
        if tuple(a.shape) != vshape or a.dtype.kind not in "iu":
            raise ValueError(f"labels are an integer volume of the infection mask's shape {vshape}")
        labels_dev = torch.from_numpy(np.asfortranarray(np.where((a >= 1) & (a <= int(n)), a, 0).astype(np.int32)).reshape(-1, order="F")).cuda()
    totals, les, ps = side_table_device(sides_dev, inf_dev, labels_dev, int(n), vshape)
    if ps is None or not int(np.prod(vshape)):
        ps = np.zeros((vshape[2], 6), np.int64)
    return burden_from_tables(totals, les, ps, p)


def _check_distribution(distribution, per_lung):
    """segment_volume's distribution= -> None (off) or the checked keyword arguments (zones._check_distribution)"""
    if distribution is None or distribution is False:
        return None
    from . import zones
    return zones._check_distribution(distribution, per_lung)


def _segmentation_distribution(distribution, ls, sides_dev, mask_dev, labels_dev, n_comp, keep, shape, connectivity):
    """segment_volume's distribution=: zones.lung_zones on the sides per_lung= left on the device, zones.lung_distribution on the final mask and the labels the lesion table
    came from (a filtered lesion's rows go with it) -> LungDistribution, its zone map on the host"""
    from . import zones
    kw, rep = distribution
    dev_sides = LungSides(**{**ls.__dict__, "sides": sides_dev})
    lz = zones.lung_zones(dev_sides, return_device=True, **kw)
    if labels_dev is None:
        labels_dev, n_comp = label_device(mask_dev, shape, connectivity)
    d = zones.lung_distribution(mask_dev, lz, labels=labels_dev, n=n_comp, shape=shape, **rep)
    if keep is not None:
        d.lesions = d.lesions[keep[1:]]
        d.lesions["label"] = np.arange(1, len(d.lesions) + 1)
    lz.zone_map = lz.zone_map.cpu().numpy().reshape(shape, order="F")
    lz.sides, lz.d2 = None, None                                    # device buffers of the size of the volume do not outlive the call
    return d


# ---- a picture of the result (csrc/kernels_render.hip) ---------------------------------------------------------------------------------
# The display windows (lo, hi) in Hounsfield units: conventional values of CT reading rooms, configurable (window=(lo, hi)); they serve DISPLAY ONLY and are not
# clinically validated here.
WINDOWS = {"lung": (-1350.0, 150.0), "mediastinum": (-160.0, 240.0)}
GRAY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
# matplotlib.colormaps["bone"](np.arange(256), bytes=True)[:, :3], as numbers: a closed-form interpolation of the map's segments differs from matplotlib in 23 of the 768
# entries, so the table is not derived (tests/test_render_host.py compares it with matplotlib where matplotlib is at hand)
BONE = np.array([
    (0, 0, 0), (0, 0, 1), (1, 1, 2), (2, 2, 3), (3, 3, 4), (4, 4, 6), (5, 5, 7), (6, 6, 8),
    (7, 6, 9), (7, 7, 10), (8, 8, 12), (9, 9, 13), (10, 10, 14), (11, 11, 15), (12, 12, 17), (13, 13, 18),
    (14, 13, 19), (14, 14, 20), (15, 15, 21), (16, 16, 23), (17, 17, 24), (18, 18, 25), (19, 19, 26), (20, 20, 28),
    (21, 20, 29), (21, 21, 30), (22, 22, 31), (23, 23, 32), (24, 24, 34), (25, 25, 35), (26, 26, 36), (27, 27, 37),
    (28, 27, 38), (28, 28, 40), (29, 29, 41), (30, 30, 42), (31, 31, 43), (32, 32, 45), (33, 33, 46), (34, 34, 47),
    (35, 34, 48), (35, 35, 49), (36, 36, 51), (37, 37, 52), (38, 38, 53), (39, 39, 54), (40, 40, 56), (41, 41, 57),
    (42, 41, 58), (42, 42, 59), (43, 43, 60), (44, 44, 62), (45, 45, 63), (46, 46, 64), (47, 47, 65), (48, 48, 66),
    (49, 48, 68), (49, 49, 69), (50, 50, 70), (51, 51, 71), (52, 52, 73), (53, 53, 74), (54, 54, 75), (55, 55, 76),
    (56, 55, 77), (56, 56, 79), (57, 57, 80), (58, 58, 81), (59, 59, 82), (60, 60, 84), (61, 61, 85), (62, 62, 86),
    (63, 62, 87), (63, 63, 88), (64, 64, 90), (65, 65, 91), (66, 66, 92), (67, 67, 93), (68, 68, 94), (69, 69, 96),
    (70, 69, 97), (70, 70, 98), (71, 71, 99), (72, 72, 101), (73, 73, 102), (74, 74, 103), (75, 75, 104), (76, 76, 105),
    (77, 76, 107), (77, 77, 108), (78, 78, 109), (79, 79, 110), (80, 80, 112), (81, 81, 113), (82, 82, 114), (83, 83, 114),
    (84, 84, 115), (84, 86, 116), (85, 87, 117), (86, 88, 118), (87, 89, 119), (88, 90, 120), (89, 92, 121), (90, 93, 121),
    (91, 94, 122), (91, 95, 123), (92, 96, 124), (93, 98, 125), (94, 99, 126), (95, 100, 127), (96, 101, 128), (97, 102, 128),
    (98, 104, 129), (98, 105, 130), (99, 106, 131), (100, 107, 132), (101, 109, 133), (102, 110, 134), (103, 111, 135), (104, 112, 135),
    (105, 113, 136), (105, 115, 137), (106, 116, 138), (107, 117, 139), (108, 118, 140), (109, 119, 141), (110, 121, 142), (111, 122, 142),
    (112, 123, 143), (112, 124, 144), (113, 125, 145), (114, 127, 146), (115, 128, 147), (116, 129, 148), (117, 130, 149), (118, 131, 149),
    (119, 133, 150), (119, 134, 151), (120, 135, 152), (121, 136, 153), (122, 137, 154), (123, 139, 155), (124, 140, 156), (125, 141, 156),
    (126, 142, 157), (126, 143, 158), (127, 145, 159), (128, 146, 160), (129, 147, 161), (130, 148, 162), (131, 149, 163), (132, 151, 163),
    (133, 152, 164), (133, 153, 165), (134, 154, 166), (135, 155, 167), (136, 157, 168), (137, 158, 169), (138, 159, 170), (139, 160, 170),
    (140, 161, 171), (140, 163, 172), (141, 164, 173), (142, 165, 174), (143, 166, 175), (144, 167, 176), (145, 169, 177), (146, 170, 177),
    (147, 171, 178), (147, 172, 179), (148, 173, 180), (149, 175, 181), (150, 176, 182), (151, 177, 183), (152, 178, 184), (153, 179, 184),
    (154, 181, 185), (154, 182, 186), (155, 183, 187), (156, 184, 188), (157, 186, 189), (158, 187, 190), (159, 188, 191), (160, 189, 191),
    (161, 190, 192), (161, 192, 193), (162, 193, 194), (163, 194, 195), (164, 195, 196), (165, 196, 197), (166, 198, 198), (167, 199, 198),
    (168, 199, 199), (170, 200, 200), (171, 201, 201), (172, 202, 202), (174, 203, 203), (175, 204, 204), (177, 205, 205), (178, 206, 205),
    (179, 206, 206), (181, 207, 207), (182, 208, 208), (183, 209, 209), (185, 210, 210), (186, 211, 211), (188, 212, 212), (189, 213, 212),
    (190, 213, 213), (192, 214, 214), (193, 215, 215), (194, 216, 216), (196, 217, 217), (197, 218, 218), (198, 219, 219), (200, 220, 219),
    (201, 220, 220), (203, 221, 221), (204, 222, 222), (205, 223, 223), (207, 224, 224), (208, 225, 225), (209, 226, 226), (211, 227, 226),
    (212, 227, 227), (213, 228, 228), (215, 229, 229), (216, 230, 230), (218, 231, 231), (219, 232, 232), (220, 233, 233), (222, 234, 233),
    (223, 234, 234), (224, 235, 235), (226, 236, 236), (227, 237, 237), (229, 238, 238), (230, 239, 239), (231, 240, 240), (233, 241, 240),
    (234, 241, 241), (235, 242, 242), (237, 243, 243), (238, 244, 244), (239, 245, 245), (241, 246, 246), (242, 247, 247), (244, 248, 247),
    (245, 248, 248), (246, 249, 249), (248, 250, 250), (249, 251, 251), (250, 252, 252), (252, 253, 253), (253, 254, 254), (255, 255, 255)], np.uint8)
COLORMAPS = {"bone": BONE, "gray": GRAY}
PALETTE_INFECTION = np.array([(0, 0, 0), (255, 0, 0)], np.uint8)               # entry 0 is never drawn: label L > 0 takes palette[1 + (L - 1) % (P - 1)]
PALETTE_LUNG = np.array([(0, 0, 0), (0, 255, 255)], np.uint8)
PALETTE_LESIONS = np.array([(0, 0, 0), (230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230)], np.uint8)
VIEWS = {"sagittal": 0, "coronal": 1, "axial": 2}                   # the axis a view looks along
PROJECTIONS = {"mip": 0, "minip": 1}                                # unet_vol_project's mode
INTERP = {"nearest": 0, "linear": 1}
RENDER_MAX_TILES, RENDER_MAX_LAYERS = _lib.RENDER_MAX_TILES, _lib.RENDER_MAX_LAYERS
ROI_MARGIN = 8                                                      # voxels around the first layer's bounding box for roi="layers"
_IN_PLANE = ((1, 2), (0, 2), (0, 1))                                # by axis: the axis along the image columns, the axis against the image rows
_RENDER_KEYS = {"n", "out_path", "window", "cmap", "mm_per_px", "tile_size", "roi", "cols", "gap", "background", "interp"}


def _check_alpha(a, what):
    if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 0 <= int(a) <= 255:
        raise ValueError(f"{what} is an integer in 0..255, not {a!r}")
    return int(a)


def _check_palette(palette):
    p = palette if isinstance(palette, np.ndarray) else np.asarray(palette)
    if p.dtype != np.uint8:
        raise ValueError(f"a palette is a uint8 array [P, 3], not {p.dtype}")
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 2:
        raise ValueError(f"a palette is uint8 [P, 3] with P >= 2 (entry 0 stands for the background and is never drawn), not {p.shape}")
    return np.ascontiguousarray(p)


class Layer:
    """One overlay of render_planes: labels (a label or mask volume of the CT's shape: a host array of bool / integer dtype, a path, a NiftiVolume, or a flat uint8 / int32
    device tensor in Fortran order together with render_planes' shape=), palette (uint8 [P, 3], P >= 2: label L > 0 is drawn in palette[1 + (L - 1) % (P - 1)], L <= 0 not
    at all), fill_alpha and outline_alpha in 0..255 (default 128: the reference's alpha=0.5 of plot_sample; the one-pixel outline solid)."""

    def __init__(self, labels, palette=PALETTE_INFECTION, fill_alpha=128, outline_alpha=255):
        self.labels, self.palette = labels, _check_palette(palette)
        self.fill_alpha, self.outline_alpha = _check_alpha(fill_alpha, "fill_alpha"), _check_alpha(outline_alpha, "outline_alpha")


class SheetTile:
    """plane: as it was asked for; axis; index (None for a projection) / slab (a, b) (None for a plain plane); x0, y0, w, h: its rectangle on the canvas;
    mm_per_px: (along the columns, along the rows); roi: the voxel ranges (lo, hi) of the two in-plane axes it shows."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"SheetTile({self.plane!r} at ({self.x0}, {self.y0}) {self.w} x {self.h})"


class RenderedSheet:
    """image: uint8 [H, W, 3] RGB (numpy; return_device=True: the device tensor); tiles: one SheetTile per plane, in the order asked for; window (lo, hi); roi
    ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)); mm_per_px; background; interp; launches: the unet_vol_render calls made.  The sheet does not mark left and right."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _check_layers(layers):
    layers = [l if isinstance(l, Layer) else Layer(l) for l in (layers or ())]
    if len(layers) > RENDER_MAX_LAYERS:
        raise ValueError(f"at most {RENDER_MAX_LAYERS} layers are drawn, not {len(layers)}")
    for l in layers:                                                # (a Layer's fields may have been changed since it was built)
        _check_palette(l.palette); _check_alpha(l.fill_alpha, "fill_alpha"); _check_alpha(l.outline_alpha, "outline_alpha")
    return layers


def _check_view(view):
    if not isinstance(view, str) or view not in VIEWS:
        raise ValueError(f"a view is one of {sorted(VIEWS)}, not {view!r}")
    return VIEWS[view]


def _check_planes(planes, vshape):
    """-> [(plane as given, axis, index or None, (a, b) or None, mode or None)]"""
    out = []
    for p in planes:
        p = tuple(p)
        if len(p) == 2:
            axis = _check_view(p[0])
            k = p[1]
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < vshape[axis]:
                raise ValueError(f"plane {p!r}: the index lies outside the volume's 0..{vshape[axis] - 1}")
            out.append((p, axis, int(k), None, None))
        elif len(p) == 4 and isinstance(p[0], str) and p[0] in PROJECTIONS:
            axis = _check_view(p[1])
            a, b = p[2], p[3]
            if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (a, b)) or not 0 <= int(a) < int(b) <= vshape[axis]:
                raise ValueError(f"plane {p!r}: the slab [a, b) is empty or leaves the volume's 0..{vshape[axis]}")
            out.append((p, axis, None, (int(a), int(b)), PROJECTIONS[p[0]]))
        else:
            raise ValueError(f"a plane is (view, index) or ('mip' | 'minip', view, a, b), not {p!r}")
    if not out:
        raise ValueError("no plane to draw")
    return out


def _minmax_window(vol):
    raw = vol.raw
    if raw.dtype.kind == "f":
        raw = raw[np.isfinite(raw)]
    if raw.size == 0:
        raise ValueError("window='minmax': the volume has no finite voxel")
    dec = nifti_min.apply_scaling(np.array([raw.min(), raw.max()]), vol.slope, vol.inter)          # decoding is monotone: a negative slope swaps the two
    lo, hi = float(dec.min()), float(dec.max())
    if not lo < hi:
        raise ValueError(f"window='minmax': the volume is constant ({lo})")
    return lo, hi


def _check_window(window, vol=None):
    if isinstance(window, str):
        if window == "minmax":
            return _minmax_window(vol) if vol is not None else None
        if window not in WINDOWS:
            raise ValueError(f"a window is one of {sorted(WINDOWS)}, 'minmax' or a (lo, hi) pair, not {window!r}")
        return WINDOWS[window]
    try:
        lo, hi = (float(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"a window is one of {sorted(WINDOWS)}, 'minmax' or a (lo, hi) pair, not {window!r}") from None
    if not lo < hi:                                                 # (a NaN fails the comparison)
        raise ValueError(f"a window needs lo < hi, not {window!r}")
    return lo, hi


def _check_cmap(cmap):
    if isinstance(cmap, str):
        if cmap not in COLORMAPS:
            raise ValueError(f"a colour map is one of {sorted(COLORMAPS)} or a uint8 [256, 3] table, not {cmap!r}")
        return COLORMAPS[cmap]
    t = np.asarray(cmap)
    if t.dtype != np.uint8 or t.shape != (256, 3):
        raise ValueError(f"a colour table is uint8 [256, 3], not {t.dtype} {t.shape}")
    return np.ascontiguousarray(t)


def _check_background(background):
    try:
        bg = tuple(background)
    except TypeError:
        bg = ()
    if len(bg) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255 for v in bg):
        raise ValueError(f"the background is three integers in 0..255, not {background!r}")
    return tuple(int(v) for v in bg)


def _check_sheet_args(window="lung", cmap="bone", mm_per_px=None, tile_size=None, roi=None, cols=None, gap=2, background=(0, 0, 0), interp="linear", vshape=None):
    """the arguments of render_planes that need no volume -> (table, interp code, background, tile_size, cols, gap, roi), or ValueError"""
    table, bg = _check_cmap(cmap), _check_background(background)
    _check_window(window)
    if not isinstance(interp, str) or interp not in INTERP:
        raise ValueError(f"interp is one of {sorted(INTERP)}, not {interp!r}")
    if mm_per_px is not None and not (isinstance(mm_per_px, (int, float, np.integer, np.floating)) and np.isfinite(mm_per_px) and mm_per_px > 0):
        raise ValueError(f"mm_per_px is a positive number, not {mm_per_px!r}")
    if tile_size is not None:
        try:
            tile_size = tuple(int(v) for v in tile_size)
        except (TypeError, ValueError):
            tile_size = ()
        if len(tile_size) != 2 or min(tile_size) < 1:
            raise ValueError("tile_size is (w, h) in pixels, both at least 1")
    for v, what, least in ((cols, "cols", 1), (gap, "gap", 0)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least):
            raise ValueError(f"{what} is an integer of at least {least}, not {v!r}")
    if roi is not None and not (isinstance(roi, str) and roi == "layers"):
        try:
            roi = tuple((int(a), int(b)) for a, b in roi)
        except (TypeError, ValueError):
            roi = ()
        if len(roi) != 3 or any(a >= b or a < 0 for a, b in roi) or (vshape is not None and any(b > n for (a, b), n in zip(roi, vshape))):
            raise ValueError("roi is None, 'layers' or three non-empty voxel ranges ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)) inside the volume")
    return table, INTERP[interp], bg, tile_size, cols, int(gap), roi


def _check_render(render):
    """segment_volume's render= -> None (off) or the checked keyword arguments of the sheet"""
    if render is None or render is False:
        return None
    kw = {} if render is True else dict(render)
    if set(kw) - _RENDER_KEYS:
        raise ValueError(f"render takes {sorted(_RENDER_KEYS)}, not {sorted(set(kw) - _RENDER_KEYS)}")
    n = kw.get("n", 6)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"render: n is the number of key slices, at least 1, not {n!r}")
    _check_sheet_args(**{k: v for k, v in kw.items() if k not in ("n", "out_path")})
    return kw


def _label_source(labels, what, vshape, shape):
    """a layer's volume, checked against the CT's shape on the host -> a device tensor as given, or a host array uint8 / int32 [X, Y, Z]"""
    torch = _torch()
    if isinstance(labels, torch.Tensor):
        if shape is None:
            raise ValueError(f"device {what} is a flat Fortran-order buffer: pass shape=(X, Y, Z)")
        if tuple(int(v) for v in shape) != vshape:
            raise ValueError(f"{what} is {tuple(shape)}, the CT {vshape}")
        if labels.dtype not in (torch.uint8, torch.int32) or not labels.is_cuda or labels.numel() != int(np.prod(vshape)):
            raise ValueError(f"device {what} is a uint8 or int32 cuda tensor of prod(shape) = {int(np.prod(vshape))} elements")
        return labels
    if isinstance(labels, (str, os.PathLike, nifti_min.NiftiVolume)):
        v = _source(labels)
        a = v.raw if v.scaling is None and v.raw.dtype.kind in "biu" else np.rint(v.get_fdata())
    else:
        a = np.asarray(labels)
        if a.dtype.kind not in "biu":
            raise ValueError(f"{what} has a bool or integer dtype, not {a.dtype}")
    if a.ndim != 3 or tuple(a.shape) != vshape:
        raise ValueError(f"{what} is {tuple(a.shape)}, the CT {vshape}")
    return a.astype(np.uint8) if a.dtype.kind == "b" or a.dtype == np.uint8 else a.astype(np.int32)


def _label_device(a):
    """-> (flat device tensor, NIfTI datatype code 2 | 8)"""
    torch = _torch()
    t = a.contiguous().reshape(-1) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F")).cuda()
    return t, (2 if t.dtype == torch.uint8 else 8)


def project_device(vargs, dev, axis, a, b, mode, labels=()):
    """unet_vol_project on an uploaded volume (vargs = _vox_args(vol), dev = upload(vol)); labels: (flat device tensor, datatype code) pairs or None ->
    (plane: float64 device tensor, [label planes or None]), each a flat Fortran-order volume with extent 1 along `axis`."""
    torch = _torch(); lib, ctx = _ctx()
    import ctypes as C
    dims = list(vargs[1:4]); dims[axis] = 1
    n = int(np.prod(dims))
    plane = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")
    k = len(labels)
    outs = [None if l is None else torch.empty(max(n, 1), dtype=l[0].dtype, device="cuda") for l in labels]
    lp = (C.c_void_p * max(k, 1))(*[None if l is None else l[0].data_ptr() for l in labels])
    lo = (C.c_void_p * max(k, 1))(*[None if o is None else o.data_ptr() for o in outs])
    ld = (C.c_int32 * max(k, 1))(*[0 if l is None else int(l[1]) for l in labels])
    ctx.check(lib.unet_vol_project(ctx.handle, dev.data_ptr(), *vargs, int(axis), int(a), int(b), int(mode), lp, ld, lo, k, plane.data_ptr(), _stream()), "vol_project")
    return plane, outs


def render_device(vargs, dev, roi, window, table_dev, interp, background, fill_background, layers, tiles, canvas):
    """unet_vol_render: layers = (labels device tensor, datatype code, palette device tensor [P, 3], fill_alpha, outline_alpha) tuples, tiles = (axis, index, x0, y0, w, h)
    tuples, roi = ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)), canvas = uint8 device tensor [H, W, 3], drawn in place."""
    lib, ctx = _ctx()
    import ctypes as C
    L = (_lib.RenderLayer * max(len(layers), 1))()
    for i, (t, code, pal, fa, oa) in enumerate(layers):
        L[i] = _lib.RenderLayer(t.data_ptr(), pal.data_ptr(), int(code), int(pal.shape[0]), int(fa), int(oa))
    T = (_lib.RenderTile * max(len(tiles), 1))()
    for i, t in enumerate(tiles):
        T[i] = _lib.RenderTile(*(int(v) for v in t))
    r = (C.c_int32 * 6)(*[int(v) for ab in roi for v in ab])
    bg = (background[0] << 16) | (background[1] << 8) | background[2]
    ctx.check(lib.unet_vol_render(ctx.handle, dev.data_ptr(), *vargs, r, float(window[0]), float(window[1]), table_dev.data_ptr(), int(interp), bg, 1 if fill_background else 0,
                                  L, len(layers), T, len(tiles), canvas.data_ptr(), int(canvas.shape[0]), int(canvas.shape[1]), _stream()), "vol_render")


def project_volume(ct, axis, slab=None, mode="max", layers=(), shape=None):
    """The maximum (mode="max") or minimum ("min") of the CT along `axis` (0, 1, 2 or a view name: the axis the view looks along) over the slab [a, b) (None: the whole
    axis), NaN voxels skipped -- np.fmax.reduce / np.fmin.reduce of get_fdata() --, and for every layer (a Layer or a label volume as Layer takes it; None is passed
    through) the largest label of each column -> (plane float64, [label planes]) as numpy volumes with extent 1 along `axis`.  Both are independent of the order of the
    walk; mean projections are not offered (a float sum is not).  Every argument error is a ValueError raised before any device work."""
    axis = _check_view(axis) if isinstance(axis, str) else axis
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not 0 <= axis <= 2:
        raise ValueError(f"axis is 0, 1, 2 or one of {sorted(VIEWS)}, not {axis!r}")
    if mode not in ("max", "min"):
        raise ValueError(f"mode is 'max' or 'min', not {mode!r}")
    layers = list(layers or ())
    if len(layers) > RENDER_MAX_LAYERS:
        raise ValueError(f"at most {RENDER_MAX_LAYERS} label volumes are projected, not {len(layers)}")
    vol = _source(ct)
    vshape = tuple(int(v) for v in vol.raw.shape)
    _check_volume_dims(vshape)
    a, b = (0, vshape[axis]) if slab is None else (int(slab[0]), int(slab[1]))
    if not 0 <= a < b <= vshape[axis]:
        raise ValueError(f"the slab [{a}, {b}) is empty or leaves the axis of {vshape[axis]} voxels")
    src = [None if l is None else _label_source(l.labels if isinstance(l, Layer) else l, f"layer {i}", vshape, shape) for i, l in enumerate(layers)]
    dev = upload(vol)
    plane, outs = project_device(_vox_args(vol), dev, int(axis), a, b, 0 if mode == "max" else 1, [None if s is None else _label_device(s) for s in src])
    pshape = tuple(1 if d == axis else n for d, n in enumerate(vshape))
    host = lambda t: t.cpu().numpy().reshape(pshape, order="F")
    return host(plane), [None if o is None else host(o) for o in outs]


def key_slices(per_slice_counts, n=6):
    """The n slices that hold the most infected voxels (ties to the lower z), in ascending z; fewer when fewer slices hold any.  Host arithmetic."""
    c = np.asarray(per_slice_counts).reshape(-1)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"n is a number of slices, not {n!r}")
    z = [int(k) for k in np.lexsort((np.arange(c.size), -c.astype(np.int64))) if c[k] > 0][:int(n)]
    return sorted(z)


def tile_pixels(extent_vox, spacing_mm, mm_per_px):
    """max(1, round(n * pixdim / mm_per_px)): Python's round of the float quotient"""
    return max(1, round(extent_vox * spacing_mm / mm_per_px))


def sheet_layout(sizes, cols=None, gap=2):
    """Tiles of sizes [(w, h)] on a grid of `cols` columns (None: ceil(sqrt(count))), row-major in the order given; a column is as wide as its widest tile, a row as high as
    its highest, `gap` pixels lie between cells and around the sheet, a tile sits in the top-left corner of its cell -> ([(x0, y0)], H, W)."""
    k = len(sizes)
    cols = int(cols) if cols is not None else int(np.ceil(np.sqrt(k)))
    cols = max(1, min(cols, k))
    rows = (k + cols - 1) // cols
    colw = [max(sizes[i][0] for i in range(c, k, cols)) for c in range(cols)]
    rowh = [max(sizes[i][1] for i in range(r * cols, min(k, (r + 1) * cols))) for r in range(rows)]
    pos = [(gap + sum(colw[:i % cols]) + gap * (i % cols), gap + sum(rowh[:i // cols]) + gap * (i // cols)) for i in range(k)]
    return pos, gap + sum(rowh) + gap * rows, gap + sum(colw) + gap * cols


def _bbox(a, vshape):
    """the bounding box of the non-zero voxels of a host [X, Y, Z] array or a flat device tensor -> [(lo, hi)] per axis, or None when there is none"""
    torch = _torch()
    if isinstance(a, torch.Tensor):
        X, Y, Z = vshape
        nz = (a.reshape(Z, Y, X) != 0)                              # plumbing: three any-reductions and 3 short downloads
        hit = [nz.any(0).any(0).cpu().numpy(), nz.any(0).any(1).cpu().numpy(), nz.any(1).any(1).cpu().numpy()]
    else:
        nz = a != 0
        hit = [nz.any((1, 2)), nz.any((0, 2)), nz.any((0, 1))]
    if not hit[0].any():
        return None
    return [(int(np.nonzero(h)[0][0]), int(np.nonzero(h)[0][-1]) + 1) for h in hit]


def render_planes(ct, planes, layers=(), window="lung", cmap="bone", mm_per_px=None, tile_size=None, roi=None, cols=None, gap=2, background=(0, 0, 0), interp="linear",
                  out_path=None, return_device=False, shape=None, _dev=None):
    """Planes of a CT with label layers on top, drawn on the device into one RGB sheet -> RenderedSheet.  The reference's plot_sample (imshow(ct, cmap='bone') under
    imshow(mask, alpha=0.5)) and its np.hstack grids, without a download of the volume.
    ct: a path, a NiftiVolume or an [X, Y, Z] array, as for segment_volume.  planes: ("axial" | "coronal" | "sagittal", index) -- the plane z / y / x = index -- and
    ("mip" | "minip", view, a, b) -- the maximum / minimum of the slab [a, b) along the view's axis (project_volume), with the largest label of every layer.  Every
    view shows np.rot90 of its slice, as the reference does: image columns run along the first in-plane axis, rows against the second.
    layers: up to 4 Layer objects (or bare label volumes: Layer's defaults), blended in order; window: a name of WINDOWS, a (lo, hi) pair or "minmax" (the finite minimum
    and maximum of the decoded volume; a constant volume is a ValueError) -- display only, not clinically validated; cmap: "bone", "gray" or a uint8 [256, 3] table.
    Tile size: w = max(1, round(n_u pixdim_u / mm_per_px)), h likewise, n_u, n_v the extents of the region in the plane; mm_per_px defaults to the smallest spacing among
    the in-plane axes of the planes asked for, so anisotropic scans come out undistorted; tile_size=(w, h) sets every tile's size instead.  roi: None (the whole volume),
    three voxel ranges, or "layers": the bounding box of the first layer's non-zero voxels plus ROI_MARGIN voxels, clipped to the volume and widened to hold every plain
    plane asked for.  The tiles are laid out by sheet_layout(sizes, cols, gap) on `background`; interp: "linear" or "nearest" for the CT (labels are always sampled
    nearest; outlines are one output pixel wide at any zoom).  out_path: the sheet as a PNG (png_min).  shape=: the (X, Y, Z) of layers given as flat device tensors.
    All plain planes go into one unet_vol_render call per 64 tiles, every projected plane costs one unet_vol_project and one more call.  The sheet does not mark the
    patient's left and right.  Every argument error is a ValueError raised before any device work."""
    torch = _torch()
    layers = _check_layers(layers)
    vol = _source(ct)
    vshape = tuple(int(v) for v in vol.raw.shape)
    _check_volume_dims(vshape)
    table, interp, bg, tile_size, cols, gap, roi = _check_sheet_args(window, cmap, mm_per_px, tile_size, roi, cols, gap, background, interp, vshape)
    plist = _check_planes(planes, vshape)
    pix = tuple(float(v) for v in vol.pixdim)
    _check_pixdim(pix)
    src = [_label_source(l.labels, f"layer {i}", vshape, shape) for i, l in enumerate(layers)]
    win = _check_window(window, vol)
    if roi is not None and roi != "layers":
        for p, axis, index, slab, mode in plist:
            if index is not None and not roi[axis][0] <= index < roi[axis][1]:
                raise ValueError(f"plane {p!r} lies outside the region {roi[axis]} of its axis")
    # ---- device work from here
    dev = _dev if _dev is not None else upload(vol)
    ldev = [_label_device(s) for s in src]
    if roi is None:
        roi = tuple((0, n) for n in vshape)
    elif roi == "layers":
        box = _bbox(ldev[0][0], vshape) if ldev else None
        box = [(0, n) for n in vshape] if box is None else [(max(0, a - ROI_MARGIN), min(n, b + ROI_MARGIN)) for (a, b), n in zip(box, vshape)]
        for p, axis, index, slab, mode in plist:
            if index is not None:
                box[axis] = (min(box[axis][0], index), max(box[axis][1], index + 1))
        roi = tuple(box)
    if mm_per_px is None:
        mm_per_px = min(pix[d] for p, axis, *_ in plist for d in _IN_PLANE[axis])
    sizes = []
    for p, axis, index, slab, mode in plist:
        au, av = _IN_PLANE[axis]
        nu, nv = roi[au][1] - roi[au][0], roi[av][1] - roi[av][0]
        sizes.append(tile_size if tile_size is not None else (tile_pixels(nu, pix[au], mm_per_px), tile_pixels(nv, pix[av], mm_per_px)))
    pos, H, W = sheet_layout(sizes, cols, gap)
    if H > 65535 or H * W * 3 >= 2 ** 31:
        raise ValueError(f"a sheet of {H} x {W} pixels is too large (at most 65535 rows and 2^31 bytes)")
    canvas = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    table_dev = torch.from_numpy(table).cuda()
    pals = [torch.from_numpy(l.palette).cuda() for l in layers]
    lspec = [(t, code, pal, l.fill_alpha, l.outline_alpha) for (t, code), pal, l in zip(ldev, pals, layers)]
    vargs = _vox_args(vol)
    tiles, plain, launches = [], [], 0
    for k, (p, axis, index, slab, mode) in enumerate(plist):
        au, av = _IN_PLANE[axis]
        (x0, y0), (w, h) = pos[k], sizes[k]
        tiles.append(SheetTile(plane=p, axis=axis, index=index, slab=slab, x0=x0, y0=y0, w=w, h=h, roi=(roi[au], roi[av]),
                               mm_per_px=((roi[au][1] - roi[au][0]) * pix[au] / w, (roi[av][1] - roi[av][0]) * pix[av] / h)))
        if index is not None:
            plain.append((axis, index, x0, y0, w, h))
    for i in range(0, len(plain), RENDER_MAX_TILES):                # the first call fills what no tile of its own covers; the later ones draw over that
        render_device(vargs, dev, roi, win, table_dev, interp, bg, launches == 0, lspec, plain[i:i + RENDER_MAX_TILES], canvas)
        launches += 1
    for t in tiles:
        if t.slab is None:
            continue
        plane, lplanes = project_device(vargs, dev, t.axis, t.slab[0], t.slab[1], PROJECTIONS[t.plane[0]], ldev)
        pargs = (64,) + tuple(1 if d == t.axis else n for d, n in enumerate(vshape)) + (0, 1.0, 0.0)
        proi = tuple((0, 1) if d == t.axis else r for d, r in enumerate(roi))
        pl = [(lp, code, pal, fa, oa) for lp, (_, code, pal, fa, oa) in zip(lplanes, lspec)]
        render_device(pargs, plane, proi, win, table_dev, interp, bg, launches == 0, pl, [(t.axis, 0, t.x0, t.y0, t.w, t.h)], canvas)
        launches += 1
    image = canvas if return_device else canvas.cpu().numpy()
    if out_path is not None:
        png_min.write(out_path, canvas.cpu().numpy())
    return RenderedSheet(image=image, tiles=tiles, window=win, roi=roi, mm_per_px=float(mm_per_px), background=bg, interp=("nearest", "linear")[interp], launches=launches)


# ---- a volume on another grid: spacing, shape, an affine, an orientation --------------------------------------------------------------------
RESAMPLE_ORDERS = ("nearest", "linear")
RESAMPLE_MODES = {"nearest": 0, "constant": 1}                      # unet_vol_resample_*'s mode: the edge voxel repeats / outside reads cval (scipy's grid-constant)
RESAMPLE_DTYPES = ("float32", "float64", "raw")
_RESAMPLE_DST = {"float64": 64, "float32": 16}                      # unet_vol_resample_linear's dst_dtype (2 = the uint8 mask of resample_mask)
_TORCH_OF_CODE = {2: "uint8", 256: "int8", 4: "int16", 8: "int32", 16: "float32", 64: "float64"}


class Grid:
    """Where a volume's voxels lie: shape (X, Y, Z) and affine (float64 4 x 4, voxel index -> RAS+ world in mm, as nifti_min reads it; a 3 x 4 is completed).  pixdim:
    the lengths of the affine's three columns; axcodes: nifti_min.axcodes_from_affine (None for an unoriented grid); voxel_ml: |det| / 1000.
    oriented=False marks a grid whose affine only carries a spacing (Grid.of of a volume without sform / qform: diag(pixdim)): it can be resampled to a spacing or a
    shape of its own, but every operation BETWEEN two grids (like=, grid=, resample_matrix, change_between, reorient_volume) refuses it -- left and right are never
    guessed (section 4u)."""

    def __init__(self, shape, affine, oriented=True):
        try:
            shp = tuple(int(v) for v in shape)
            exact = all(int(v) == v for v in shape)
        except (TypeError, ValueError):
            shp, exact = (), False
        if len(shp) != 3 or not exact or any(v < 1 for v in shp):
            raise ValueError(f"a grid's shape is three positive integers (X, Y, Z), not {shape!r}")
        try:
            m = np.array(affine, np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"a grid's affine is a finite 4 x 4 matrix, not {affine!r}") from None
        if m.shape == (3, 4):
            m = np.vstack([m, [0.0, 0.0, 0.0, 1.0]])
        if m.shape != (4, 4) or not np.isfinite(m).all() or not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("a grid's affine is a finite 4 x 4 matrix whose last row is (0, 0, 0, 1)")
        det = float(np.linalg.det(m[:3, :3]))
        if not np.isfinite(det) or det == 0.0:
            raise ValueError("a grid's affine must be invertible (its three columns span the space)")
        self.shape, self.affine, self.oriented = shp, m, bool(oriented)

    @property
    def pixdim(self):
        return tuple(float(v) for v in np.sqrt((self.affine[:3, :3] * self.affine[:3, :3]).sum(axis=0)))

    @property
    def axcodes(self):
        return nifti_min.axcodes_from_affine(self.affine) if self.oriented else None

    @property
    def voxel_ml(self):
        return abs(float(np.linalg.det(self.affine[:3, :3]))) / 1000.0

    @classmethod
    def of(cls, vol, pixdim=None, affine=None):
        """The grid of a path, a NiftiVolume or an [X, Y, Z] array: affine= when given, else the file's affine (sform, else qform), else diag(pixdim or the file's
        pixdim), marked oriented=False."""
        v = _source(vol)
        if affine is not None:
            return cls(v.raw.shape, affine, True)
        if pixdim is None and v.affine is not None:
            return cls(v.raw.shape, v.affine, True)
        p = _check_pixdim(v.pixdim if pixdim is None else pixdim)
        return cls(v.raw.shape, np.diag([p[0], p[1], p[2], 1.0]), False)

    def __repr__(self):
        return f"Grid(shape={self.shape}, pixdim={tuple(round(p, 4) for p in self.pixdim)}, axcodes={self.axcodes}, oriented={self.oriented})"


class ResampledVolume:
    """data: the volume on the new grid -- numpy [X', Y', Z'] in Fortran order, or with return_device=True the flat device tensor --; grid: its Grid; matrix: float64
    3 x 4, output voxel index -> source voxel coordinate, the 12 numbers the kernel received; slope, inter: the scaling of the stored elements (dtype="raw" and
    reorient_volume keep the source's, everything else is decoded: 0, 0)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"ResampledVolume({self.grid!r})"


class VolumeChange:
    """What change_between returns, on a's grid: persistent (in both), new (in b only), resolved (in a only) -- voxels, and *_ml at a's voxel volume --, dice between a
    and b-on-a's-grid (nan when both are empty), per_slice int64 [Z, 3] (persistent, new, resolved), b_on_a: b's mask on a's grid (uint8; the device tensor with
    return_device=True), grid: a's."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"VolumeChange(persistent_ml={self.persistent_ml:.2f}, new_ml={self.new_ml:.2f}, resolved_ml={self.resolved_ml:.2f}, dice={self.dice:.4f})"


def _need_oriented(g, what):
    if not isinstance(g, Grid):
        raise ValueError(f"{what} is a Grid, not {type(g).__name__}")
    if not g.oriented:
        raise ValueError(f"{what} has no orientation (its volume carries neither sform nor qform and no affine= was given): two grids are only related through their "
                         "affines -- left and right are not guessed")
    return g


def _check_matrix(M):
    """-> float64 [3, 4], C order: the 12 finite numbers the kernels take; ValueError otherwise"""
    try:
        m = np.array(M, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"a resampling matrix is 3 x 4 (or 4 x 4), not {M!r}") from None
    if m.shape == (4, 4):
        m = m[:3]
    if m.shape != (3, 4):
        raise ValueError(f"a resampling matrix is 3 x 4 (or 4 x 4), not {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError("the resampling matrix has a non-finite entry")
    return np.ascontiguousarray(m)


def resample_matrix(src_grid, dst_grid):
    """inv(A_src) @ A_dst in float64, its top three rows [3, 4]: the source voxel coordinate of every voxel index of dst_grid.  Both grids must be oriented."""
    a, b = _need_oriented(src_grid, "the source grid"), _need_oriented(dst_grid, "the target grid")
    with np.errstate(over="ignore", invalid="ignore"):              # (an overflow is reported by _check_matrix, as a ValueError)
        return _check_matrix((np.linalg.inv(a.affine) @ b.affine)[:3])


def _zoom_target(g, new_shape):
    """the grid of the same field of view with new_shape voxels: output voxel i has its centre at s = (i + 0.5)(n / n') - 0.5 (half-voxel centres, section 4v)"""
    z = np.array([n / m for n, m in zip(g.shape, new_shape)], np.float64)
    M = np.zeros((3, 4))
    M[:, :3] = np.diag(z)
    M[:, 3] = 0.5 * z - 0.5
    return Grid(new_shape, g.affine @ np.vstack([M, [0.0, 0.0, 0.0, 1.0]]), g.oriented), _check_matrix(M)


def resample_target(src_grid, spacing=None, shape=None, like=None, grid=None):
    """-> (the target Grid, M float64 [3, 4]) of resample_volume's spacing= / shape= / like= / grid=; exactly one of them.  Host arithmetic, no device.
    spacing=(p'x, p'y, p'z) and shape=(n'x, n'y, n'z) keep the field of view: n' = max(1, round(n p / p')) (Python's round) for spacing=, M = [diag(n / n') | 0.5 n / n'
    - 0.5] and the new affine is A [M; 0 0 0 1] -- these work on an unoriented grid too, and hand its mark on.  like= (a Grid, a path or a NiftiVolume) and grid= (a
    Grid) name another grid: M = resample_matrix(src_grid, target), and both must be oriented."""
    if not isinstance(src_grid, Grid):
        raise ValueError(f"the source grid is a Grid, not {type(src_grid).__name__}")
    given = [k for k, v in (("spacing", spacing), ("shape", shape), ("like", like), ("grid", grid)) if v is not None]
    if len(given) != 1:
        raise ValueError(f"exactly one of spacing=, shape=, like= and grid= names the target grid; got {given if given else 'none'}")
    if spacing is not None:
        p = _check_pixdim(spacing)
        new_shape = tuple(max(1, int(round(n * q / float(v)))) for n, q, v in zip(src_grid.shape, src_grid.pixdim, p))
        return _zoom_target(src_grid, new_shape)
    if shape is not None:
        return _zoom_target(src_grid, Grid(shape, np.eye(4)).shape)
    if grid is not None:
        target = grid
    else:
        target = like if isinstance(like, Grid) else Grid.of(like)
    return target, resample_matrix(src_grid, _need_oriented(target, "the target grid"))


def reorient_matrix(shape, src_codes, dst_codes):
    """The signed axis permutation that stores a volume of `shape` with axis codes src_codes under dst_codes -> (M float64 [3, 4], the new shape): output axis j runs
    along the source axis a with the same world axis, s_a = i_j when the two letters agree and (n_a - 1) - i_j when they are opposite.  Integers, exact in float64."""
    src, dst = nifti_min.check_axcodes(src_codes), nifti_min.check_axcodes(dst_codes)
    shp = Grid(shape, np.eye(4)).shape
    M, new_shape = np.zeros((3, 4)), [0, 0, 0]
    for j, (w, sign) in enumerate(dst):
        a = [k for k, (ws, _) in enumerate(src) if ws == w][0]
        new_shape[j] = shp[a]
        if src[a][1] == sign:
            M[a, j] = 1.0
        else:
            M[a, j], M[a, 3] = -1.0, float(shp[a] - 1)
    return _check_matrix(M), tuple(new_shape)


class _ResampleSource:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _resample_source(x, pixdim=None, affine=None, src_shape=None, kind="volume"):
    """What resample_* take -> _ResampleSource(vol: the NiftiVolume still to upload, or None; tensor: the flat device tensor given, or None; shape; vargs: dtype code, X,
    Y, Z, scaled, slope, inter; grid; header: the file's 348 bytes or None).  kind "mask": foreground = non-zero, as uint8 0 / 1; "labels": as int32; no device work."""
    torch = _torch()
    if pixdim is not None and affine is not None:
        raise ValueError("pixdim= and affine= both describe the source grid: give one")
    if isinstance(x, torch.Tensor):
        if src_shape is None:
            raise ValueError("a device volume is a flat Fortran-order buffer: pass src_shape=(X, Y, Z)")
        shp = Grid(src_shape, np.eye(4)).shape
        code = {getattr(torch, v): k for k, v in _TORCH_OF_CODE.items()}.get(x.dtype)
        want = {"mask": (2,), "labels": (8,)}.get(kind, tuple(_TORCH_OF_CODE))
        if code not in want or not x.is_cuda or x.numel() != int(np.prod(shp)):
            raise ValueError(f"a device {kind} is a cuda tensor of dtype {' / '.join(_TORCH_OF_CODE[c] for c in want)} with prod(src_shape) = {int(np.prod(shp))} elements")
        _check_volume_dims(shp)
        if affine is not None:
            g = Grid(shp, affine, True)
        else:
            p = _check_pixdim((1.0, 1.0, 1.0) if pixdim is None else pixdim)
            g = Grid(shp, np.diag([p[0], p[1], p[2], 1.0]), False)
        return _ResampleSource(vol=None, tensor=x.contiguous().reshape(-1), shape=shp, vargs=(code,) + shp + (0, 1.0, 0.0), grid=g, header=None)
    if src_shape is not None:
        raise ValueError("src_shape= describes a flat device tensor; a host volume carries its own shape")
    vol = _source(x)
    g = Grid.of(vol, pixdim, affine)
    header = vol.header if isinstance(x, (str, os.PathLike, nifti_min.NiftiVolume)) else None
    if kind in ("mask", "labels"):
        dec = vol.raw if vol.scaling is None else vol.get_fdata()
        if dec.dtype.kind not in "biu":
            if isinstance(x, (str, os.PathLike, nifti_min.NiftiVolume)):
                dec = np.rint(dec)                                  # (a mask file stored as float, or scaled: as _label_source reads it)
            else:
                raise ValueError(f"a {kind} volume has a bool or integer dtype, not {dec.dtype}")
        a = np.asfortranarray((dec != 0).astype(np.uint8) if kind == "mask" else dec.astype(np.int32))
        vol = nifti_min.NiftiVolume(a, 0.0, 0.0, vol.pixdim, vol.header, "<")
    shp = tuple(int(v) for v in vol.raw.shape)
    _check_volume_dims(shp)
    return _ResampleSource(vol=vol, tensor=None, shape=shp, vargs=_vox_args(vol), grid=g, header=header)


def _check_resample_args(order="linear", mode="nearest", cval=None, dtype="float32", orders=RESAMPLE_ORDERS):
    if not isinstance(order, str) or order not in orders:
        raise ValueError(f"order is one of {list(orders)}, not {order!r}")
    if not isinstance(mode, str) or mode not in RESAMPLE_MODES:
        raise ValueError(f"mode is one of {sorted(RESAMPLE_MODES)}, not {mode!r}")
    if not isinstance(dtype, str) or dtype not in RESAMPLE_DTYPES:
        raise ValueError(f"dtype is one of {list(RESAMPLE_DTYPES)}, not {dtype!r}")
    if dtype == "raw" and order != "nearest":
        raise ValueError("dtype='raw' keeps the stored elements, which only order='nearest' can move; order='linear' blends decoded values")
    if cval is not None and (isinstance(cval, (bool, str)) or not isinstance(cval, (int, float, np.integer, np.floating))):
        raise ValueError(f"cval is a number, not {cval!r}")


def _stored_extreme(src, lowest=True):
    """the stored element that decodes to the volume's minimum (lowest) -- NaNs aside --, as a numpy scalar of the stored dtype; no finite element: ValueError"""
    code, scaled, slope = src.vargs[0], src.vargs[4], src.vargs[5]
    take_min = lowest == (not scaled or slope > 0)
    if src.vol is not None:
        raw = src.vol.raw
        if raw.dtype.kind == "f":
            raw = raw[~np.isnan(raw)]
        if raw.size == 0:
            raise ValueError("cval: the volume has no voxel that is not NaN; pass cval=")
        return raw.min() if take_min else raw.max()
    t = src.tensor
    if t.dtype.is_floating_point:
        t = t[~t.isnan()]
    if t.numel() == 0:
        raise ValueError("cval: the volume has no voxel that is not NaN; pass cval=")
    return np.array((t.min() if take_min else t.max()).item(), nifti_min.DTYPES[code])[()]


def _decode_scalar(src, v):
    sc = (src.vargs[5], src.vargs[6]) if src.vargs[4] else None
    return float(v) if sc is None else float(np.float64(v) * sc[0] + sc[1])


def resample_nearest_device(dev, elem_bytes, src_shape, M, mode, cval_bits, out_shape):
    """unet_vol_resample_nearest -> a uint8 device tensor of prod(out_shape) * elem_bytes bytes (the moved elements, Fortran order)"""
    M = _check_matrix(M)
    torch = _torch(); lib, ctx = _ctx()
    out = torch.empty(int(np.prod(out_shape)) * int(elem_bytes), dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_resample_nearest(ctx.handle, dev.data_ptr(), int(elem_bytes), *(int(v) for v in src_shape), M.ctypes.data, int(mode), int(cval_bits), out.data_ptr(),
                                            *(int(v) for v in out_shape), _stream()), "vol_resample_nearest")
    return out


def resample_linear_device(dev, vargs, M, mode, cval, out_shape, dst_dtype):
    """unet_vol_resample_linear -> a float64 (dst_dtype 64), float32 (16) or uint8 (2) device tensor of prod(out_shape) elements in Fortran order"""
    M = _check_matrix(M)
    torch = _torch(); lib, ctx = _ctx()
    out = torch.empty(int(np.prod(out_shape)), dtype={64: torch.float64, 16: torch.float32, 2: torch.uint8}[dst_dtype], device="cuda")
    ctx.check(lib.unet_vol_resample_linear(ctx.handle, dev.data_ptr(), *vargs, M.ctypes.data, int(mode), float(cval), out.data_ptr(), int(dst_dtype),
                                           *(int(v) for v in out_shape), _stream()), "vol_resample_linear")
    return out


def _bits_of(v, np_dtype):
    """the stored bytes of one element as an unsigned integer (unet_vol_resample_nearest's cval_bits)"""
    return int.from_bytes(np.array(v).astype(np_dtype).tobytes(), "little")


def _resample_raw(src, M, mode, cval_stored, out_shape):
    """the nearest kernel on the source as stored -> a flat device tensor of the stored dtype"""
    torch = _torch()
    code = src.vargs[0]
    npdt = np.dtype(nifti_min.DTYPES[code])
    dev = src.tensor if src.tensor is not None else upload(src.vol)
    out = resample_nearest_device(dev, npdt.itemsize, src.shape, M, mode, _bits_of(cval_stored, npdt), out_shape)
    if code in _TORCH_OF_CODE:
        return out.view(getattr(torch, _TORCH_OF_CODE[code]))
    return out                                                      # (uint16 / uint32: torch has no arithmetic type for them; the bytes)


def _host_of(t, np_dtype, shape):
    a = t.cpu().numpy()
    if a.dtype != np.dtype(np_dtype):
        a = a.view(np_dtype)
    return a.reshape(shape, order="F")


def _write_resampled(out_path, host, g):
    nifti_min.write(out_path, host, nifti_min.header_with_affine(g.shape, g.affine))


def _check_out_path(out_path, stored_dtype):
    if out_path is not None and np.dtype(stored_dtype) not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise ValueError(f"out_path: nifti_min writes uint8 and float32 volumes, not {np.dtype(stored_dtype)}; ask for dtype='float32'")


def resample_volume(ct, spacing=None, shape=None, like=None, grid=None, order="linear", mode="nearest", cval=None, dtype="float32", return_device=False, out_path=None,
                    pixdim=None, affine=None, src_shape=None):
    """A CT on another grid, computed on the device -> ResampledVolume(data, grid, matrix).  ct: a path, a NiftiVolume, an [X, Y, Z] array (its grid then from pixdim=
    or affine=, default 1 mm unoriented) or a flat device tensor in Fortran order with src_shape=(X, Y, Z) (uint8, int8, int16, int32, float32 or float64, not scaled).
    The target, exactly one of (resample_target): spacing= or shape= (the same field of view with other voxels; they also work on a volume without an orientation), like=
    (a Grid, a path or a NiftiVolume) or grid= (a Grid) -- then both the volume and the target must carry an orientation.
    order "linear": trilinear blend of the decoded voxels ((float64(v) slope) + inter, as get_fdata), a + (b - a) w along x, then y, then z, in float64; a NaN voxel makes
    every output that touches it NaN, even at weight 0, as scipy.ndimage does.  "nearest": the voxel at floor(s + 0.5).  mode "nearest": outside the volume the edge
    voxel repeats; "constant": outside reads cval (scipy's grid-constant), which defaults to the volume's decoded minimum (NaNs aside; air, for a CT).
    dtype "float32" (the float64 result rounded once) or "float64"; "raw" needs order="nearest" and keeps the stored element type with its slope and inter -- cval= is then a
    STORED value, by default the stored element that decodes to the minimum; with every other dtype cval= is a decoded value, in both orders.  order="nearest" with a
    float dtype moves the stored elements on the device and decodes them on the host (an explicit cval= is written there, where the same kernel finds a volume of ones
    outside), so it cannot be combined with return_device=True.  out_path: the result as .nii / .nii.gz with the new grid as its sform (float32 or uint8 data).
    Neither order filters before it coarsens: coarsening by more than 2x aliases (filters.gaussian_filter is the low-pass to run first).  Every argument error is a ValueError raised before any device work."""
    _check_resample_args(order, mode, cval, dtype)
    if order == "nearest" and dtype != "raw" and return_device:
        raise ValueError("order='nearest' moves stored elements; with return_device=True ask for dtype='raw' (the decode to a float dtype happens on the host)")
    src = _resample_source(ct, pixdim, affine, src_shape)
    target, M = resample_target(src.grid, spacing, shape, like, grid)
    _check_volume_dims(target.shape)
    npdt = np.dtype(nifti_min.DTYPES[src.vargs[0]])
    _check_out_path(out_path, npdt if dtype == "raw" else dtype)
    m = RESAMPLE_MODES[mode]
    if order == "nearest":
        decoded_cval = m == 1 and cval is not None and dtype != "raw"          # the outside of a decoded result reads cval itself, which need not be a stored value
        stored = 0 if m == 0 or decoded_cval else (_stored_extreme(src) if cval is None else cval)
        if npdt.kind in "iu" and not (np.isfinite(float(stored)) and float(stored) == int(stored) and np.iinfo(npdt).min <= int(stored) <= np.iinfo(npdt).max):
            raise ValueError(f"cval {stored!r} is not a value of the stored dtype {npdt}")
        out = _resample_raw(src, M, m, stored, target.shape)
        if dtype == "raw":
            data = out if return_device else _host_of(out, npdt, target.shape)
            res = ResampledVolume(data=data, grid=target, matrix=M, slope=src.vargs[5] if src.vargs[4] else 0.0, inter=src.vargs[6] if src.vargs[4] else 0.0)
        else:
            host = nifti_min.apply_scaling(_host_of(out, npdt, target.shape), *((src.vargs[5], src.vargs[6]) if src.vargs[4] else (0.0, 0.0)))
            if decoded_cval:                                        # where the outputs lie inside: the same kernel on a volume of ones, background 0
                ones = _torch().ones(int(np.prod(src.shape)), dtype=_torch().uint8, device="cuda")
                inside = _host_of(resample_nearest_device(ones, 1, src.shape, M, 1, 0, target.shape), np.uint8, target.shape)
                host[inside == 0] = float(cval)
            res = ResampledVolume(data=np.asfortranarray(host.astype(dtype)), grid=target, matrix=M, slope=0.0, inter=0.0)
    else:
        c = 0.0 if m == 0 else (_decode_scalar(src, _stored_extreme(src)) if cval is None else float(cval))
        dev = src.tensor if src.tensor is not None else upload(src.vol)
        out = resample_linear_device(dev, src.vargs, M, m, c, target.shape, _RESAMPLE_DST[dtype])
        res = ResampledVolume(data=out if return_device else _host_of(out, dtype, target.shape), grid=target, matrix=M, slope=0.0, inter=0.0)
    if out_path is not None:
        _write_resampled(out_path, _host_of(res.data, npdt if dtype == "raw" else dtype, target.shape) if return_device else res.data, target)
    return res


def _label_mode(mode, spacing, shape):
    """masks and labels: by default the edge repeats where the field of view is kept (spacing= / shape=) and the outside is background (0) on another grid"""
    return ("nearest" if (spacing is not None or shape is not None) else "constant") if mode is None else mode


def resample_mask(mask, spacing=None, shape=None, like=None, grid=None, order="nearest", mode=None, return_device=False, out_path=None, pixdim=None, affine=None,
                  src_shape=None):
    """A mask on another grid -> ResampledVolume whose data is uint8 0 / 1.  mask: as resample_volume takes a volume; non-zero = foreground (a device mask is a uint8
    tensor of 0 / 1 with src_shape=).  order "nearest": the voxel at floor(s + 0.5); "linear": the 0 / 1 mask blended trilinearly and cut at 0.5 (result >= 0.5), which
    keeps smooth borders when the voxels shrink.  mode: "nearest" / "constant" (background outside); default: "nearest" for spacing= / shape=, "constant" for like= /
    grid=.  The targets, out_path and the errors are resample_volume's."""
    mode = _label_mode(mode, spacing, shape)
    _check_resample_args(order, mode, None, "raw" if order == "nearest" else "float32")
    src = _resample_source(mask, pixdim, affine, src_shape, "mask")
    target, M = resample_target(src.grid, spacing, shape, like, grid)
    _check_volume_dims(target.shape)
    m = RESAMPLE_MODES[mode]
    if order == "nearest":
        out = _resample_raw(src, M, m, 0, target.shape)
    else:
        dev = src.tensor if src.tensor is not None else upload(src.vol)
        out = resample_linear_device(dev, src.vargs, M, m, 0.0, target.shape, 2)
    res = ResampledVolume(data=out if return_device else _host_of(out, np.uint8, target.shape), grid=target, matrix=M, slope=0.0, inter=0.0)
    if out_path is not None:
        _write_resampled(out_path, _host_of(out, np.uint8, target.shape), target)
    return res


def resample_labels(labels, spacing=None, shape=None, like=None, grid=None, order="nearest", mode=None, return_device=False, pixdim=None, affine=None, src_shape=None):
    """A label volume on another grid -> ResampledVolume whose data is int32: every output takes the label at floor(s + 0.5).  Nearest only: labels are names, not
    amounts (no majority vote, no per-label blending); outside the volume: mode, as for resample_mask, with label 0 as the constant."""
    if order != "nearest":
        raise ValueError(f"labels are resampled with order='nearest' only (a blend of two labels is no label), not {order!r}")
    mode = _label_mode(mode, spacing, shape)
    _check_resample_args("nearest", mode, None, "raw")
    src = _resample_source(labels, pixdim, affine, src_shape, "labels")
    target, M = resample_target(src.grid, spacing, shape, like, grid)
    _check_volume_dims(target.shape)
    out = _resample_raw(src, M, RESAMPLE_MODES[mode], 0, target.shape)
    return ResampledVolume(data=out if return_device else _host_of(out, np.int32, target.shape), grid=target, matrix=M, slope=0.0, inter=0.0)


def reorient_volume(vol, codes="RAS", orientation=None, return_device=False, src_shape=None):
    """The volume stored under other axis codes (default "RAS", the canonical orientation: the axes grow to the patient's right, anterior, superior) -> ResampledVolume:
    a signed permutation of the axes through the nearest kernel -- its coordinates are integers, exact in float64 --, the stored element type, slope and inter kept.
    vol: a path, a NiftiVolume, an array or a flat device tensor with src_shape=; orientation: None = the volume's own affine, or its axis codes such as "LPS", or a 4 x 4
    affine.  The new grid carries the permuted affine (A [M; 0 0 0 1]) and pixdim; for an oblique affine the codes are those of axcodes_from_affine and the affine stays
    oblique.  A volume without an orientation from either is a ValueError: left and right are never guessed."""
    lin, src_codes = _check_orientation(orientation)
    nifti_min.check_axcodes(codes)
    src = _resample_source(vol, None, None, src_shape)
    if orientation is not None:
        named = isinstance(orientation, str) or all(isinstance(c, str) for c in orientation)
        g = Grid(src.shape, nifti_min.affine_from_axcodes(src_codes, src.grid.pixdim) if named else np.asarray(orientation, np.float64), True)
    else:
        g = _need_oriented(src.grid, "the volume's grid")
        try:
            src_codes = g.axcodes
        except nifti_min.NiftiFormatError as e:
            raise ValueError(f"reorient_volume: {e}") from None
    M, new_shape = reorient_matrix(src.shape, src_codes, codes)
    target = Grid(new_shape, g.affine @ np.vstack([M, [0.0, 0.0, 0.0, 1.0]]), True)
    npdt = np.dtype(nifti_min.DTYPES[src.vargs[0]])
    out = _resample_raw(src, M, 0, 0, new_shape)
    return ResampledVolume(data=out if return_device else _host_of(out, npdt, new_shape), grid=target, matrix=M, slope=src.vargs[5] if src.vargs[4] else 0.0,
                           inter=src.vargs[6] if src.vargs[4] else 0.0)


def change_between(mask_a, grid_a, mask_b, grid_b, return_device=False, transform=None):
    """Two masks of one patient on two grids (a baseline a and a follow-up b, a prediction and a truth drawn at another slice thickness) -> VolumeChange on a's grid.
    b is put on a's grid with the nearest kernel, background outside b's volume; unet_vol_confusion then counts persistent (a and b), new (b only) and resolved (a only)
    voxels per slice; millilitres at a's voxel volume; dice = 2 persistent / (2 persistent + new + resolved).  mask_a / mask_b: host arrays (non-zero = foreground) or
    uint8 device tensors of prod(grid.shape) elements; both grids must be oriented Grids.  transform=None: the two affines are taken as they are (two re-griddings of one
    acquisition).  transform= a RigidTransform, a Registration (register_volumes(ct_a, ct_b)) or a 4 x 4 matrix T, a's world -> b's world: b's affine is replaced by
    inv(T) @ A_b first, so a follow-up in which the patient lies differently is compared in the baseline's frame (section 4x).  transform= a DeformableRegistration
    (refine_registration, or register_volumes(..., deformable=True)) of a onto b: b's mask goes onto a's grid through its displacement field as well
    (unet_vol_warp_field, nearest, background outside; section 4y) -- grid_a and grid_b must then be the grids the field was found on."""
    ga, gb = _need_oriented(grid_a, "grid_a"), _need_oriented(grid_b, "grid_b")
    deform = transform if isinstance(transform, DeformableRegistration) else None
    if deform is not None:
        for g, want, what in ((ga, deform.field.fixed_grid, "grid_a"), (gb, deform.field.moving_grid, "grid_b")):
            if g.shape != want.shape or not np.array_equal(g.affine, want.affine):
                raise ValueError(f"{what} is not the grid the deformable registration was found on ({g!r} for {want!r})")
    elif transform is not None:
        gb = Grid(gb.shape, np.linalg.inv(_world_matrix(transform)) @ gb.affine, True)
    torch = _torch()
    srcs = []
    for mk, g, what in ((mask_a, ga, "mask_a"), (mask_b, gb, "mask_b")):
        s = _resample_source(mk, None, g.affine, g.shape if isinstance(mk, torch.Tensor) else None, "mask")
        if s.shape != g.shape:
            raise ValueError(f"{what} is {s.shape}, its grid {g.shape}")
        srcs.append(s)
    dev_a = srcs[0].tensor if srcs[0].tensor is not None else upload(srcs[0].vol)
    if deform is not None:
        M = deform.field.voxel_matrix
        b_on_a = deform.field._warp(srcs[1], 0, 1, 0.0, 0, 2)
    else:
        M = resample_matrix(gb, ga)
        b_on_a = _resample_raw(srcs[1], M, 1, 0, ga.shape)
    counts = confusion_device(b_on_a, dev_a, ga.shape)
    tp, fp, fn = (int(v) for v in counts.sum(axis=0))
    ml = ga.voxel_ml
    return VolumeChange(persistent=tp, new=fp, resolved=fn, persistent_ml=tp * ml, new_ml=fp * ml, resolved_ml=fn * ml, dice=_ratio(2 * tp, 2 * tp + fp + fn),
                        per_slice=counts, b_on_a=b_on_a if return_device else _host_of(b_on_a, np.uint8, ga.shape), grid=ga, matrix=M)


# ---- a follow-up onto its baseline: rigid registration by mutual information (csrc/kernels_register.hip) --------------------------------------
JOINT_HIST_MAX_K = _lib.JOINT_HIST_MAX_K                             # UNET_VOL_JOINT_HIST_MAX_K: candidates per launch
JOINT_HIST_MAX_BINS = _lib.JOINT_HIST_MAX_BINS                       # UNET_VOL_JOINT_HIST_MAX_BINS
REGISTER_METRICS = ("mi", "nmi")
REGISTER_LEVELS_MM = (8.0, 4.0, 2.0)
REGISTER_WINDOW = (-1000.0, 400.0)                                  # air to dense tissue: everything above clamps into the last bin
REGISTER_MAX_BATCHES = 400
REGISTER_STOP = 0.05                                                # a level ends when its translation step falls below this share of its spacing


def _rotation(rx, ry, rz):
    """R = Rz Ry Rx (radians): about x first, then y, then z"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    Ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    Rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return Rz @ (Ry @ Rx)


class RigidTransform:
    """A rigid motion of the world, fixed world -> moving world, in millimetres and radians: x_m = R (x - c) + c + t with R = Rz(rz) Ry(ry) Rx(rx), params = (tx, ty,
    tz, rx, ry, rz) and centre c (the point the rotation turns about; it only changes how the same motion splits into R and t).  matrix: the 4 x 4 of that map --
    the identity, exactly, for params of zero.  inverse() and compose() return RigidTransforms about the same centre; from_matrix reads the six numbers back from a
    4 x 4 (|ry| < 90 degrees)."""

    def __init__(self, params=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), centre=(0.0, 0.0, 0.0)):
        try:
            p, c = np.array(params, np.float64).reshape(-1), np.array(centre, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"a rigid transform is six numbers (tx, ty, tz in mm, rx, ry, rz in radians) and a centre of three, not {params!r}, {centre!r}") from None
        if p.shape != (6,) or c.shape != (3,) or not np.isfinite(p).all() or not np.isfinite(c).all():
            raise ValueError(f"a rigid transform is six finite numbers (tx, ty, tz in mm, rx, ry, rz in radians) and a finite centre of three, not {params!r}, {centre!r}")
        self.params, self.centre = p, c

    @property
    def rotation(self):
        return _rotation(*self.params[3:])

    @property
    def matrix(self):
        R, c, t = self.rotation, self.centre, self.params[:3]
        m = np.eye(4)
        m[:3, :3] = R
        m[:3, 3] = (c + t) - R @ c
        return m

    @classmethod
    def from_matrix(cls, matrix, centre=(0.0, 0.0, 0.0), tol=1e-9):
        """the RigidTransform about `centre` whose matrix is `matrix` (4 x 4 or 3 x 4): R must be a rotation (R^T R = 1 and det R = +1 within tol) -- a zoom, a shear or a
        mirror is a ValueError."""
        m = _world_matrix(matrix)
        c = cls((0.0,) * 6, centre).centre
        R = m[:3, :3]
        if not np.allclose(R.T @ R, np.eye(3), rtol=0.0, atol=tol) or abs(float(np.linalg.det(R)) - 1.0) > tol:
            raise ValueError("the matrix is not rigid: its 3 x 3 part is no rotation (a zoom, a shear or a mirror)")
        ry = float(np.arcsin(min(1.0, max(-1.0, -R[2, 0]))))
        rx, rz = float(np.arctan2(R[2, 1], R[2, 2])), float(np.arctan2(R[1, 0], R[0, 0]))
        t = (m[:3, 3] - c) + R @ c
        return cls((t[0], t[1], t[2], rx, ry, rz), c)

    def inverse(self):
        """moving world -> fixed world, about the same centre"""
        return RigidTransform.from_matrix(np.linalg.inv(self.matrix), self.centre)

    def compose(self, first):
        """self after `first`: x -> self(first(x)), about self's centre"""
        return RigidTransform.from_matrix(self.matrix @ _world_matrix(first), self.centre)

    def __repr__(self):
        t, r = self.params[:3], np.rad2deg(self.params[3:])
        return f"RigidTransform(t=({t[0]:.3f}, {t[1]:.3f}, {t[2]:.3f}) mm, r=({r[0]:.3f}, {r[1]:.3f}, {r[2]:.3f}) deg, centre=({self.centre[0]:.2f}, {self.centre[1]:.2f}, {self.centre[2]:.2f}))"


def _world_matrix(t):
    """a RigidTransform, a Registration or a 4 x 4 (3 x 4) world matrix -> float64 4 x 4, finite, invertible, last row (0, 0, 0, 1); ValueError otherwise"""
    if isinstance(t, Registration):
        t = t.transform
    if isinstance(t, RigidTransform):
        return t.matrix
    try:
        m = np.array(t, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"a world transform is a RigidTransform, a Registration or a 4 x 4 matrix, not {t!r}") from None
    if m.shape == (3, 4):
        m = np.vstack([m, [0.0, 0.0, 0.0, 1.0]])
    if m.shape != (4, 4) or not np.isfinite(m).all() or not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("a world transform is a finite 4 x 4 matrix whose last row is (0, 0, 0, 1)")
    det = float(np.linalg.det(m[:3, :3]))
    if not np.isfinite(det) or det == 0.0:
        raise ValueError("a world transform must be invertible")
    return m


def voxel_matrix(fixed_grid, moving_grid, transform=None):
    """inv(A_moving) @ T @ A_fixed in float64, its top three rows [3, 4]: the moving voxel coordinate of every fixed voxel index under the world transform T (None: the
    identity, which makes it resample_matrix(moving_grid, fixed_grid)).  Both grids must be oriented."""
    f, m = _need_oriented(fixed_grid, "the fixed grid"), _need_oriented(moving_grid, "the moving grid")
    T = np.eye(4) if transform is None else _world_matrix(transform)
    with np.errstate(over="ignore", invalid="ignore"):
        return _check_matrix((np.linalg.inv(m.affine) @ T @ f.affine)[:3])


def _check_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= JOINT_HIST_MAX_BINS:
        raise ValueError(f"bins is an integer from 2 to {JOINT_HIST_MAX_BINS}, not {bins!r}")
    return int(bins)


def _check_hist_window(window, what="window"):
    try:
        w = np.array(window, np.float64).reshape(-1)
    except (TypeError, ValueError):
        w = np.zeros(0)
    with np.errstate(over="ignore"):
        bad = w.shape != (2,) or not np.isfinite(w).all() or not w[1] > w[0] or not np.isfinite(w[1] - w[0])
    if bad:
        raise ValueError(f"{what} is two finite numbers (lo, hi) with hi > lo, not {window!r}")
    return float(w[0]), float(w[1])


def _check_fixed_mask(mask, shape):
    """a mask on the fixed grid, checked on the host (no device work): a host array [X, Y, Z] of a bool or integer dtype, or a uint8 device tensor of prod(shape) elements"""
    if mask is None:
        return None
    torch = _torch()
    if isinstance(mask, torch.Tensor):
        if mask.dtype != torch.uint8 or not mask.is_cuda or mask.numel() != int(np.prod(shape)):
            raise ValueError(f"a device mask is a uint8 cuda tensor of prod(shape) = {int(np.prod(shape))} elements")
        return mask
    a = np.asarray(mask)
    if a.dtype.kind not in "biu" or tuple(a.shape) != tuple(shape):
        raise ValueError(f"mask is a bool or integer array on the fixed grid {tuple(shape)}, not {a.dtype} {tuple(a.shape)}")
    return a


def joint_hist_device(fixed_dev, fixed_vargs, mask_dev, moving_dev, moving_vargs, matrices, bins, window, moving_window):
    """unet_vol_joint_hist on uploaded volumes -> uint32 numpy [K, B, B] (fixed bin major) for matrices [K, 3, 4]; K beyond JOINT_HIST_MAX_K takes several launches"""
    torch = _torch(); lib, ctx = _ctx()
    Ms = np.ascontiguousarray(np.asarray(matrices, np.float64).reshape(-1, 3, 4))
    K = len(Ms)
    counts = torch.empty((K, bins, bins), dtype=torch.int32, device="cuda")
    for k0 in range(0, K, JOINT_HIST_MAX_K):
        part = np.ascontiguousarray(Ms[k0:k0 + JOINT_HIST_MAX_K])
        ctx.check(lib.unet_vol_joint_hist(ctx.handle, fixed_dev.data_ptr(), *fixed_vargs, _ptr(mask_dev), moving_dev.data_ptr(), *moving_vargs, part.ctypes.data, len(part),
                                          int(bins), window[0], window[1], moving_window[0], moving_window[1], counts[k0:].data_ptr(), _stream()), "vol_joint_hist")
    return counts.cpu().numpy().view(np.uint32)


def _world_matrices(transforms):
    """None (the identity), one world transform or a sequence of them -> a list of 4 x 4"""
    if transforms is None:
        return [np.eye(4)]
    if isinstance(transforms, (RigidTransform, Registration)) or (isinstance(transforms, np.ndarray) and transforms.ndim == 2):
        return [_world_matrix(transforms)]
    try:
        ts = list(transforms)
    except TypeError:
        raise ValueError(f"transforms is None, a world transform or a sequence of them, not {transforms!r}") from None
    if len(ts) and not isinstance(ts[0], (RigidTransform, Registration)) and np.ndim(ts[0]) == 1:          # (one matrix given as nested lists)
        return [_world_matrix(transforms)]
    if not ts:
        raise ValueError("transforms is empty")
    return [_world_matrix(t) for t in ts]


def joint_histogram(fixed, moving, transforms=None, bins=32, window=REGISTER_WINDOW, moving_window=None, mask=None, fixed_affine=None, moving_affine=None, fixed_shape=None,
                    moving_shape=None):
    """The joint intensity histogram of two CTs under candidate world transforms, on the device -> uint32 [K, B, B], fixed bin major.  fixed, moving: as resample_volume
    takes a volume -- a path, a NiftiVolume, an [X, Y, Z] array with fixed_affine= / moving_affine=, or a flat device tensor with the affine and fixed_shape= /
    moving_shape= --; both must carry an orientation.  transforms: None (the identity), a RigidTransform, a 4 x 4 world matrix (fixed world -> moving world) or a
    sequence of them; candidate c counts every fixed voxel whose moving coordinate inv(A_moving) @ T_c @ A_fixed (i, j, k) lies inside the moving volume, whose value and
    trilinear moving sample are not NaN, and which mask (on the fixed grid; non-zero = take) admits, in cell (bin(fixed), bin(sample)): bin(v) = floor((v - lo) B / (hi -
    lo)) clamped to [0, B - 1], window for the fixed and moving_window (default: the same) for the moving volume.  Every argument error is a ValueError before any device
    work."""
    B, wf = _check_bins(bins), _check_hist_window(window)
    wm = wf if moving_window is None else _check_hist_window(moving_window, "moving_window")
    f, m = _resample_source(fixed, None, fixed_affine, fixed_shape), _resample_source(moving, None, moving_affine, moving_shape)
    Ms = [voxel_matrix(f.grid, m.grid, T) for T in _world_matrices(transforms)]
    mk = _check_fixed_mask(mask, f.shape)
    fd = f.tensor if f.tensor is not None else upload(f.vol)
    md = m.tensor if m.tensor is not None else upload(m.vol)
    mask_dev = None if mk is None else _mask_to_device(mk, f.shape)[0]
    return joint_hist_device(fd, f.vargs, mask_dev, md, m.vargs, Ms, B, wf, wm)


def mutual_information(hist, normalized=False):
    """Host float64, from the integer counts alone.  hist [B, B] -> a float; [K, B, B] -> float64 [K].  p = h / sum h, p_f and p_m its row and column sums:
    MI = sum p log(p / (p_f p_m)) over the non-zero cells (nats); normalized: (H_f + H_m) / H_fm, from 1 (independent) to 2 (one determines the other), and 1 when every
    counted voxel fell into one cell (all three entropies are 0).  An empty histogram scores -inf."""
    h = np.asarray(hist)
    if h.ndim == 3:
        return np.array([mutual_information(x, normalized) for x in h], np.float64)
    if h.ndim != 2 or h.shape[0] != h.shape[1] or h.dtype.kind not in "iu" or (h.dtype.kind == "i" and (h < 0).any()):
        raise ValueError(f"a joint histogram is a square array of non-negative integer counts [B, B] (or [K, B, B]), not {h.dtype} {h.shape}")
    h = h.astype(np.float64)
    n = float(h.sum())
    if n == 0.0:
        return float("-inf")
    p = h / n
    pf, pm = p.sum(axis=1), p.sum(axis=0)
    nz = p > 0.0
    if normalized:
        hf, hm = -float((pf[pf > 0.0] * np.log(pf[pf > 0.0])).sum()), -float((pm[pm > 0.0] * np.log(pm[pm > 0.0])).sum())
        hfm = -float((p[nz] * np.log(p[nz])).sum())
        return (hf + hm) / hfm if hfm > 0.0 else 1.0
    return float((p[nz] * np.log(p[nz] / np.outer(pf, pm)[nz])).sum())


class RegistrationLevel:
    """One level of the search: spacing (mm, sets the steps), grid (where the level's fixed volume lies), voxels (how many fixed voxels the level's mask admits: what
    min_overlap is a share of) and evaluate: matrices float64 [K, 3, 4] (level voxel index -> moving voxel coordinate) -> counts uint32 [K, B, B]."""

    def __init__(self, spacing, grid, voxels, evaluate):
        self.spacing, self.grid, self.voxels, self.evaluate = float(spacing), grid, int(voxels), evaluate


class Registration:
    """What register_volumes returns.  transform: the RigidTransform found, fixed world -> moving world, about the centre of the fixed field of view; voxel_matrix:
    inv(A_moving) @ T @ A_fixed [3, 4] on the two native grids; metric / metric_init: the metric at the result and at the start, both on the last level; overlap: the
    share of the last level's voxels counted at the result; batches: 12-neighbour launches; evaluations: histograms in all; converged: False when max_batches ended the
    search; history: one dict per level (spacing, shape, batches, evaluations, metric, params); seconds; fixed_grid, moving_grid."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def resample(self, moving, kind="volume", order=None, **kw):
        """The moving scan (kind "volume"), or a mask ("mask") or a label volume ("labels") drawn on it, on the fixed grid: resample_volume / resample_mask /
        resample_labels with the moving grid's affine replaced by inv(T) @ A_moving and grid= the fixed grid.  order and the other keywords are theirs (a device
        tensor needs src_shape=)."""
        fn = {"volume": resample_volume, "mask": resample_mask, "labels": resample_labels}.get(kind)
        if fn is None:
            raise ValueError(f"kind is 'volume', 'mask' or 'labels', not {kind!r}")
        for k in ("spacing", "shape", "like", "grid", "pixdim", "affine"):
            if k in kw:
                raise ValueError(f"Registration.resample sets {k}= itself: the target is the fixed grid, the source affine inv(T) @ A_moving")
        if order is not None:
            kw["order"] = order
        return fn(moving, grid=self.fixed_grid, affine=np.linalg.inv(self.transform.matrix) @ self.moving_grid.affine, **kw)

    def __repr__(self):
        return f"Registration({self.transform!r}, metric={self.metric:.4f} from {self.metric_init:.4f}, overlap={self.overlap:.3f}, batches={self.batches}, converged={self.converged})"


def _grid_centre(g):
    """the world position of the centre of a grid's field of view"""
    return (g.affine @ np.array([(g.shape[0] - 1) / 2.0, (g.shape[1] - 1) / 2.0, (g.shape[2] - 1) / 2.0, 1.0]))[:3]


def _check_register_args(levels_mm=REGISTER_LEVELS_MM, bins=32, window=REGISTER_WINDOW, moving_window=None, init="geometry", min_overlap=0.25,
                         max_batches=REGISTER_MAX_BATCHES, metric="mi"):
    try:
        lv = tuple(float(v) for v in levels_mm)
    except (TypeError, ValueError):
        lv = ()
    if not lv or not all(np.isfinite(v) and v > 0 for v in lv) or any(b >= a for a, b in zip(lv, lv[1:])):
        raise ValueError(f"levels_mm is a strictly descending sequence of positive spacings in mm, not {levels_mm!r}")
    B, wf = _check_bins(bins), _check_hist_window(window)
    wm = wf if moving_window is None else _check_hist_window(moving_window, "moving_window")
    if not (isinstance(init, RigidTransform) or (isinstance(init, str) and init in ("geometry", "identity"))):
        raise ValueError(f"init is 'geometry', 'identity' or a RigidTransform, not {init!r}")
    if isinstance(min_overlap, (bool, str)) or not isinstance(min_overlap, (int, float, np.integer, np.floating)) or not 0.0 < float(min_overlap) <= 1.0:
        raise ValueError(f"min_overlap is a share in (0, 1], not {min_overlap!r}")
    if isinstance(max_batches, bool) or not isinstance(max_batches, (int, np.integer)) or int(max_batches) < 1:
        raise ValueError(f"max_batches is a positive integer, not {max_batches!r}")
    if not isinstance(metric, str) or metric not in REGISTER_METRICS:
        raise ValueError(f"metric is one of {list(REGISTER_METRICS)}, not {metric!r}")
    return lv, B, wf, wm


def registration_level_grids(fixed_grid, levels_mm=REGISTER_LEVELS_MM):
    """Host arithmetic: per level (spacing, Grid, M): the isotropic grid of that spacing over the fixed field of view (resample_target(spacing=)) with the matrix that
    resamples the fixed volume onto it, or (spacing, fixed_grid, None) -- the fixed volume itself -- for a level whose spacing does not exceed the fixed volume's
    smallest: resampling would coarsen no axis."""
    g = _need_oriented(fixed_grid, "the fixed grid")
    out = []
    for L in levels_mm:
        if L <= min(g.pixdim):
            out.append((float(L), g, None))
        else:
            target, M = resample_target(g, spacing=(L, L, L))
            out.append((float(L), target, M))
    return out


def initial_transform(fixed_grid, moving_grid, init="geometry"):
    """-> the RigidTransform a search starts from, about the centre of the fixed field of view.  "geometry": the translation that puts the centre of the fixed field of
    view onto the centre of the moving one, no rotation; "identity": the two world frames as they are; a RigidTransform: that motion, re-expressed about the centre."""
    c = _grid_centre(_need_oriented(fixed_grid, "the fixed grid"))
    if isinstance(init, RigidTransform):
        return RigidTransform.from_matrix(init.matrix, c)
    if init == "identity":
        return RigidTransform((0.0,) * 6, c)
    t = _grid_centre(_need_oriented(moving_grid, "the moving grid")) - c
    return RigidTransform((t[0], t[1], t[2], 0.0, 0.0, 0.0), c)


def rigid_search(levels, fixed_grid, moving_grid, init="geometry", min_overlap=0.25, max_batches=REGISTER_MAX_BATCHES, metric="mi"):
    """The deterministic pattern search of register_volumes over caller-supplied evaluators (levels: RegistrationLevels, coarse to fine) -> Registration.  No device
    work of its own: register_volumes hands it unet_vol_joint_hist, the tests the numpy oracle -- the same loop, the same counts, the same transform.
    Per level the six parameters (about the centre of the fixed field of view) start from the previous level's result with steps of 2 x spacing mm for tx, ty, tz and
    the same number in degrees for rx, ry, rz.  A batch scores the 12 neighbours (+step, -step per parameter, in parameter order) with one call of evaluate; a
    candidate that counts fewer than min_overlap x level.voxels voxels scores -inf.  The best neighbour (ties: the lowest index) is taken if it is strictly better than
    the current point; otherwise all steps are halved.  The level ends when the translation step falls below 0.05 x spacing, the search when max_batches are spent."""
    _check_register_args(init=init, min_overlap=min_overlap, max_batches=max_batches, metric=metric)
    fg, mg = _need_oriented(fixed_grid, "the fixed grid"), _need_oriented(moving_grid, "the moving grid")
    if not levels:
        raise ValueError("no levels to search")
    t0 = time.perf_counter()
    start = initial_transform(fg, mg, init)
    centre, params = start.centre, start.params.copy()
    normalized = metric == "nmi"
    inv_m = np.linalg.inv(mg.affine)

    def score(level, plist):
        Ms = np.stack([_check_matrix((inv_m @ RigidTransform(p, centre).matrix @ level.grid.affine)[:3]) for p in plist])
        counts = np.asarray(level.evaluate(Ms))
        if counts.shape[0] != len(plist) or counts.ndim != 3:
            raise ValueError(f"evaluate returned {counts.shape} for {len(plist)} matrices")
        n = counts.reshape(len(plist), -1).sum(axis=1, dtype=np.int64)
        val = mutual_information(counts, normalized)
        val[n < min_overlap * level.voxels] = -np.inf
        return val, n

    batches = evaluations = 0
    converged, history = True, []
    cur = -np.inf
    for level in levels:
        step = np.array([2.0 * level.spacing] * 3 + [np.deg2rad(2.0 * level.spacing)] * 3)
        cur = float(score(level, [params])[0][0])
        lb, le = 0, 1
        while step[0] >= REGISTER_STOP * level.spacing:
            if batches >= max_batches:
                converged = False
                break
            cand = []
            for q in range(6):
                for sign in (1.0, -1.0):
                    c = params.copy()
                    c[q] += sign * step[q]
                    cand.append(c)
            val, _ = score(level, cand)
            batches += 1; lb += 1; le += len(cand)
            best = int(np.argmax(val))                               # (the first of equal maxima)
            if val[best] > cur:
                params, cur = cand[best], float(val[best])
            else:
                step = step * 0.5
        evaluations += le
        history.append(dict(spacing=level.spacing, shape=level.grid.shape, batches=lb, evaluations=le, metric=cur, params=params.copy()))
        if not converged:
            break
    last = levels[len(history) - 1]
    val0, _ = score(last, [start.params])
    _, n_end = score(last, [params])
    evaluations += 2
    T = RigidTransform(params, centre)
    return Registration(transform=T, voxel_matrix=voxel_matrix(fg, mg, T), metric=cur, metric_init=float(val0[0]), overlap=float(n_end[0]) / max(last.voxels, 1),
                        batches=batches, evaluations=evaluations, converged=converged, history=history, seconds=time.perf_counter() - t0, fixed_grid=fg, moving_grid=mg,
                        metric_name=metric)


def register_volumes(fixed, moving, levels_mm=REGISTER_LEVELS_MM, bins=32, window=REGISTER_WINDOW, mask=None, init="geometry", min_overlap=0.25,
                     max_batches=REGISTER_MAX_BATCHES, metric="mi", moving_window=None, fixed_affine=None, moving_affine=None, fixed_shape=None, moving_shape=None,
                     deformable=None):
    """Register a follow-up CT (moving) to its baseline (fixed) on the device -> Registration: the rigid transform, fixed world -> moving world, that maximises the mutual
    information ("mi") or its normalised form ("nmi") of the joint histogram (joint_histogram: bins, window, moving_window, mask on the fixed grid).  fixed, moving: as
    joint_histogram takes them; both must carry an orientation.
    The search is rigid_search's and deterministic: the same inputs give the same transform on every run.  Per level of levels_mm (coarse to fine) the fixed volume is put
    on an isotropic grid of that spacing over the same field of view with resample_volume (linear, float32) -- a level whose spacing does not exceed the fixed volume's
    smallest uses the fixed volume itself --, the mask with resample_mask (nearest); the moving volume stays on its own grid.  init: "geometry" (the centres of the two
    fields of view aligned), "identity" or a RigidTransform.  Registration.resample and change_between(transform=) apply the result.
    Hard bins, no gradients (section 4x).  deformable=None: rigid only, a Registration.  deformable=True, or a dict of refine_registration's keywords (levels_mm,
    iterations, field_sigma, image_sigma, max_step): the rigid result is refined with a demons displacement field (section 4y; the same mask) and the
    DeformableRegistration is returned, its .rigid the Registration.  Every argument error is a ValueError before any device work."""
    lv, B, wf, wm = _check_register_args(levels_mm, bins, window, moving_window, init, min_overlap, max_batches, metric)
    if deformable is not None and deformable is not True and not isinstance(deformable, dict):
        raise ValueError(f"deformable is None, True or a dict of refine_registration's keywords, not {deformable!r}")
    dkw = dict(deformable) if isinstance(deformable, dict) else {}
    if deformable is not None:
        bad = sorted(set(dkw) - {"levels_mm", "iterations", "field_sigma", "image_sigma", "max_step"})
        if bad:
            raise ValueError(f"deformable= takes levels_mm, iterations, field_sigma, image_sigma and max_step, not {bad}")
        _check_deform_args(**dkw)
    f, m = _resample_source(fixed, None, fixed_affine, fixed_shape), _resample_source(moving, None, moving_affine, moving_shape)
    fg, mg = _need_oriented(f.grid, "the fixed volume's grid"), _need_oriented(m.grid, "the moving volume's grid")
    mk = _check_fixed_mask(mask, f.shape)
    grids = registration_level_grids(fg, lv)
    for _, g, _ in grids:
        _check_volume_dims(g.shape)
    torch = _torch()
    t0 = time.perf_counter()
    fd = f.tensor if f.tensor is not None else upload(f.vol)
    md = m.tensor if m.tensor is not None else upload(m.vol)
    mask_dev = None if mk is None else _mask_to_device(mk, f.shape)[0]
    levels = []
    for L, g, M in grids:
        if M is None:
            ldev, lvargs, lmask = fd, f.vargs, mask_dev
        else:
            ldev = resample_linear_device(fd, f.vargs, M, 0, 0.0, g.shape, 16)
            lvargs = (16,) + g.shape + (0, 1.0, 0.0)
            lmask = None if mask_dev is None else resample_nearest_device(mask_dev, 1, f.shape, M, 0, 0, g.shape)
        voxels = int(np.prod(g.shape)) if lmask is None else int(torch.count_nonzero(lmask).item())

        def evaluate(Ms, ldev=ldev, lvargs=lvargs, lmask=lmask):
            return joint_hist_device(ldev, lvargs, lmask, md, m.vargs, Ms, B, wf, wm)

        levels.append(RegistrationLevel(L, g, voxels, evaluate))
    reg = rigid_search(levels, fg, mg, init, min_overlap, max_batches, metric)
    torch.cuda.synchronize()
    reg.seconds = time.perf_counter() - t0
    if deformable is not None:
        return refine_registration(fixed, moving, reg, mask=mask, fixed_affine=fixed_affine, moving_affine=moving_affine, fixed_shape=fixed_shape, moving_shape=moving_shape, **dkw)
    return reg


# ---- the deformable refinement of a registered follow-up: demons on the device (csrc/kernels_deform.hip) ------------------------------------------
SMOOTH_MAX_RADIUS = _lib.SMOOTH_MAX_RADIUS                           # UNET_VOL_SMOOTH_MAX_RADIUS: taps either side of a Gaussian pass
DEFORM_LEVELS_MM = (8.0, 4.0)                                       # conventional, configurable starting values; not clinically validated (section 4y)
DEFORM_ITERATIONS = (30, 15)


def gaussian_weights(sigma):
    """The 2 R + 1 weights of one pass of a normalised Gaussian of width sigma (in voxels), R = ceil(3 sigma): exp(-t^2 / (2 sigma^2)) / their sum, float64, computed
    once on the host -> float64 [2 R + 1]; sigma = 0 -> None (no pass)."""
    if isinstance(sigma, (bool, str)) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not np.isfinite(sigma) or sigma < 0:
        raise ValueError(f"a Gaussian width is a finite number of voxels >= 0, not {sigma!r}")
    if sigma == 0:
        return None
    R = int(np.ceil(3.0 * float(sigma)))
    if R > SMOOTH_MAX_RADIUS:
        raise ValueError(f"a Gaussian width of {sigma} voxels needs {R} taps either side; a pass takes {SMOOTH_MAX_RADIUS} (coarsen the level instead)")
    t = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(t * t) / (2.0 * float(sigma) * float(sigma)))
    return w / w.sum()


def _check_deform_args(levels_mm=DEFORM_LEVELS_MM, iterations=DEFORM_ITERATIONS, field_sigma=1.5, image_sigma=1.0, max_step=1.0):
    """-> (levels, iterations per level, the field's weights or None, the images' weights or None, max_step); ValueError otherwise"""
    try:
        lv = tuple(float(v) for v in levels_mm)
    except (TypeError, ValueError):
        lv = ()
    if not lv or not all(np.isfinite(v) and v > 0 for v in lv) or any(b >= a for a, b in zip(lv, lv[1:])):
        raise ValueError(f"levels_mm is a strictly descending sequence of positive spacings in mm, not {levels_mm!r}")
    try:
        its = tuple(iterations)
    except TypeError:
        its = ()
    if len(its) != len(lv) or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0 for v in its):
        raise ValueError(f"iterations is one non-negative integer per level ({len(lv)}), not {iterations!r}")
    if isinstance(max_step, (bool, str)) or not isinstance(max_step, (int, float, np.integer, np.floating)) or not np.isfinite(max_step) or not max_step > 0:
        raise ValueError(f"max_step is a finite positive number of level voxels, not {max_step!r}")
    return lv, tuple(int(v) for v in its), gaussian_weights(field_sigma), gaussian_weights(image_sigma), float(max_step)


def _check_mat3(m, what):
    """-> float64 [3, 3], C order, finite; ValueError otherwise"""
    a = np.ascontiguousarray(np.asarray(m, np.float64))
    if a.shape != (3, 3) or not np.isfinite(a).all():
        raise ValueError(f"{what} is a finite 3 x 3 matrix")
    return a


def smooth_axis_device(x, C, shape, axis, weights):
    """unet_vol_smooth_axis -> a new float32 device tensor: one pass of `weights` along `axis` of the C volumes of `shape` stored one after the other in x"""
    torch = _torch(); lib, ctx = _ctx()
    w = np.ascontiguousarray(weights, np.float64)
    out = torch.empty_like(x)
    ctx.check(lib.unet_vol_smooth_axis(ctx.handle, x.data_ptr(), int(C), *(int(v) for v in shape), int(axis), (w.size - 1) // 2, w.ctypes.data, out.data_ptr(), _stream()),
              "vol_smooth_axis")
    return out


def demons_step_device(fixed_dev, fixed_vargs, mask_dev, moving_dev, moving_vargs, W, L, Ginv, delta, field):
    """unet_vol_demons_step -> u + v, a new float32 device tensor [3 X Y Z]"""
    torch = _torch(); lib, ctx = _ctx()
    W, L, G = _check_matrix(W), _check_mat3(L, "L"), _check_mat3(Ginv, "Ginv")
    out = torch.empty_like(field)
    ctx.check(lib.unet_vol_demons_step(ctx.handle, fixed_dev.data_ptr(), *fixed_vargs, _ptr(mask_dev), moving_dev.data_ptr(), *moving_vargs, W.ctypes.data, L.ctypes.data,
                                       G.ctypes.data, float(delta), field.data_ptr(), out.data_ptr(), _stream()), "vol_demons_step")
    return out


def warp_field_device(dev, vargs, W, L, field, field_shape, F, order, mode, cval, cval_bits, out_shape, dst_dtype):
    """unet_vol_warp_field -> order 1: a float64 (dst_dtype 64), float32 (16) or uint8 (2) device tensor of prod(out_shape) elements; order 0: the moved elements as a
    uint8 tensor of prod(out_shape) x the element size bytes (dst_dtype = the source's code)"""
    torch = _torch(); lib, ctx = _ctx()
    W, L = _check_matrix(W), _check_mat3(L, "L")
    F = None if F is None else _check_matrix(F)
    n = int(np.prod(out_shape))
    if order == 1:
        out = torch.empty(n, dtype={64: torch.float64, 16: torch.float32, 2: torch.uint8}[dst_dtype], device="cuda")
    else:
        out = torch.empty(n * np.dtype(nifti_min.DTYPES[vargs[0]]).itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(lib.unet_vol_warp_field(ctx.handle, dev.data_ptr(), *vargs, W.ctypes.data, L.ctypes.data, field.data_ptr(), *(int(v) for v in field_shape),
                                      None if F is None else F.ctypes.data, int(order), int(mode), float(cval), int(cval_bits), out.data_ptr(), int(dst_dtype),
                                      *(int(v) for v in out_shape), _stream()), "vol_warp_field")
    return out


def jacobian_device(field, shape, Ainv):
    """unet_vol_jacobian -> (det: float32 device tensor of prod(shape) elements, the number of voxels with det <= 0)"""
    torch = _torch(); lib, ctx = _ctx()
    Ai = _check_mat3(Ainv, "Ainv")
    det = torch.empty(int(np.prod(shape)), dtype=torch.float32, device="cuda")
    folded = torch.empty(1, dtype=torch.int32, device="cuda")
    ctx.check(lib.unet_vol_jacobian(ctx.handle, field.data_ptr(), *(int(v) for v in shape), Ai.ctypes.data, det.data_ptr(), folded.data_ptr(), _stream()), "vol_jacobian")
    return det, int(folded.item()) & 0xFFFFFFFF


class DeformOps:
    """The operations refine_registration's loop is written over, on the device: volumes and fields are flat device tensors in Fortran order.  tests/deform_oracle.py
    has the same methods over numpy arrays, so the host test and the device test run the SAME loop (as rigid_search takes its evaluators)."""

    def upload(self, src):
        return src.tensor if src.tensor is not None else upload(src.vol)

    def upload_mask(self, mask, shape):
        return None if mask is None else _mask_to_device(mask, shape)[0]

    def linear(self, dev, vargs, M, out_shape):
        """the volume on a level grid: unet_vol_resample_linear, clamped, float32"""
        return resample_linear_device(dev, vargs, M, 0, 0.0, out_shape, 16)

    def nearest_mask(self, dev, shape, M, out_shape):
        return resample_nearest_device(dev, 1, shape, M, 0, 0, out_shape)

    def zeros(self, n):
        return _torch().zeros(int(n), dtype=_torch().float32, device="cuda")

    def stack(self, parts):
        return _torch().cat(list(parts))

    smooth_axis = staticmethod(smooth_axis_device)
    demons_step = staticmethod(demons_step_device)
    warp_field = staticmethod(warp_field_device)
    jacobian = staticmethod(jacobian_device)

    def rms(self, f, warped, mask):
        """-> (the RMS of f - warped over the voxels the mask admits where neither is NaN, in float64; how many those are)"""
        d = f.double() - warped
        ok = ~d.isnan() if mask is None else (~d.isnan() & (mask != 0))
        n = int(ok.sum().item())
        return (float((d[ok] * d[ok]).sum().sqrt().item() / np.sqrt(n)) if n else float("nan")), n

    def minmax(self, det):
        return float(det.min().item()), float(det.max().item())

    def sync(self):
        _torch().cuda.synchronize()


class DisplacementField:
    """A dense displacement field u (section 4y).  tensor: float32 [3 X Y Z] on the device, component major, each component in Fortran order on `grid` (a level grid over
    the fixed field of view), in millimetres of the fixed world frame; rigid: the world transform T it refines, fixed world -> moving world (what was given:
    a Registration, a RigidTransform or a 4 x 4), matrix its 4 x 4; fixed_grid, moving_grid: the two volumes' grids.  A fixed world point p corresponds to the moving
    world point T (p + u(p)); voxel_matrix = inv(A_moving) T A_fixed [3, 4]."""

    def __init__(self, tensor, grid, rigid, fixed_grid, moving_grid):
        self.tensor, self.grid, self.rigid, self.fixed_grid, self.moving_grid = tensor, grid, rigid, fixed_grid, moving_grid
        self.matrix = _world_matrix(rigid)
        self.voxel_matrix = voxel_matrix(fixed_grid, moving_grid, self.matrix)
        self.mm_to_voxels = _check_mat3((np.linalg.inv(moving_grid.affine) @ self.matrix)[:3, :3], "L")
        same = grid.shape == fixed_grid.shape and np.array_equal(grid.affine, fixed_grid.affine)
        self.field_matrix = None if same else resample_matrix(grid, fixed_grid)          # F: fixed voxel index -> field voxel coordinate

    def _warp(self, src, order, mode, cval, cval_bits, dst_dtype):
        dev = src.tensor if src.tensor is not None else upload(src.vol)
        return warp_field_device(dev, src.vargs, self.voxel_matrix, self.mm_to_voxels, self.tensor, self.grid.shape, self.field_matrix, order, mode, cval, cval_bits,
                                 self.fixed_grid.shape, dst_dtype)

    def resample(self, moving, kind="volume", order=None, mode=None, cval=None, dtype="float32", return_device=False, src_shape=None):
        """The moving scan (kind "volume"), or a mask ("mask") or a label volume ("labels") drawn on it, on the fixed grid through T and the field: unet_vol_warp_field
        -> ResampledVolume (matrix: the rigid voxel matrix).  It mirrors Registration.resample: order "linear" (default for a volume; a mask is then blended and cut at
        0.5) or "nearest" (default for masks and labels, the only one for labels; a volume then needs dtype="raw": the stored elements move); mode "nearest" (default for
        a volume) or "constant" (default for masks and labels: background outside); cval, dtype and return_device as resample_volume has them; a device tensor needs
        src_shape=.  moving must lie on the moving grid."""
        if kind not in ("volume", "mask", "labels"):
            raise ValueError(f"kind is 'volume', 'mask' or 'labels', not {kind!r}")
        order = ("linear" if kind == "volume" else "nearest") if order is None else order
        mode = ("nearest" if kind == "volume" else "constant") if mode is None else mode
        if kind == "labels" and order != "nearest":
            raise ValueError(f"labels are resampled with order='nearest' only (a blend of two labels is no label), not {order!r}")
        if kind != "volume":
            dtype = "raw" if order == "nearest" else "float32"
        _check_resample_args(order, mode, cval, dtype)
        if order == "nearest" and dtype != "raw":
            raise ValueError("order='nearest' moves stored elements: ask for dtype='raw'")
        src = _resample_source(moving, None, self.moving_grid.affine, src_shape, kind)
        if src.shape != self.moving_grid.shape:
            raise ValueError(f"the {kind} is {src.shape}, the moving grid {self.moving_grid.shape}")
        m = RESAMPLE_MODES[mode]
        code = src.vargs[0]
        npdt = np.dtype(nifti_min.DTYPES[code])
        shape = self.fixed_grid.shape
        if order == "nearest":
            stored = 0 if m == 0 or kind != "volume" else (_stored_extreme(src) if cval is None else cval)
            if npdt.kind in "iu" and not (np.isfinite(float(stored)) and float(stored) == int(stored) and np.iinfo(npdt).min <= int(stored) <= np.iinfo(npdt).max):
                raise ValueError(f"cval {stored!r} is not a value of the stored dtype {npdt}")
            out = self._warp(src, 0, m, 0.0, _bits_of(stored, npdt), code)
            if code in _TORCH_OF_CODE:
                out = out.view(getattr(_torch(), _TORCH_OF_CODE[code]))
            keep = kind == "volume" and src.vargs[4]
            return ResampledVolume(data=out if return_device else _host_of(out, npdt, shape), grid=self.fixed_grid, matrix=self.voxel_matrix,
                                   slope=src.vargs[5] if keep else 0.0, inter=src.vargs[6] if keep else 0.0)
        if kind == "mask":
            out, host_dt = self._warp(src, 1, m, 0.0, 0, 2), np.uint8
        else:
            c = 0.0 if m == 0 else (_decode_scalar(src, _stored_extreme(src)) if cval is None else float(cval))
            out, host_dt = self._warp(src, 1, m, c, 0, _RESAMPLE_DST[dtype]), dtype
        return ResampledVolume(data=out if return_device else _host_of(out, host_dt, shape), grid=self.fixed_grid, matrix=self.voxel_matrix, slope=0.0, inter=0.0)

    def jacobian(self, return_device=False):
        """-> (det(I + du/dp) per field voxel: float32 [X, Y, Z] on the field grid -- the flat device tensor with return_device=True --, folded: how many are <= 0)"""
        det, folded = jacobian_device(self.tensor, self.grid.shape, np.linalg.inv(self.grid.affine[:3, :3]))
        return (det if return_device else _host_of(det, np.float32, self.grid.shape)), folded

    def magnitude(self):
        """-> (the largest, the mean) |u| in mm over the field grid"""
        u = self.tensor.reshape(3, -1).double()
        norm = (u * u).sum(dim=0).sqrt()
        return float(norm.max().item()), float(norm.mean().item())

    def host(self):
        """-> float32 [3, X, Y, Z]"""
        a = self.tensor if isinstance(self.tensor, np.ndarray) else self.tensor.cpu().numpy()
        return np.stack([c.reshape(self.grid.shape, order="F") for c in a.reshape(3, -1)])

    def __repr__(self):
        return f"DisplacementField({self.grid!r})"


class DeformableRegistration:
    """What refine_registration returns.  field: the DisplacementField on the last level's grid; rigid: the transform it started from, as given; residual_init /
    residual: the RMS of f - m_w on the last level with the rigid transform alone and with the field (over the voxels the mask admits where the fixed level image and
    the warped moving level image -- unet_vol_warp_field, linear, NaN outside, float64 -- are both numbers); jacobian_min, jacobian_max, folded: of the final field;
    history: one dict per level (spacing, shape, iterations, residual_start, residual, voxels); seconds.  resample() is the field's."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def resample(self, moving, kind="volume", order=None, **kw):
        return self.field.resample(moving, kind, order, **kw)

    def __repr__(self):
        return (f"DeformableRegistration(residual={self.residual:.2f} from {self.residual_init:.2f}, jacobian=[{self.jacobian_min:.3f}, {self.jacobian_max:.3f}], "
                f"folded={self.folded})")


def refine_registration(fixed, moving, rigid, levels_mm=DEFORM_LEVELS_MM, iterations=DEFORM_ITERATIONS, field_sigma=1.5, image_sigma=1.0, max_step=1.0, mask=None,
                        fixed_affine=None, moving_affine=None, fixed_shape=None, moving_shape=None, ops=None):
    """Refine a rigid registration of a follow-up CT (moving) onto its baseline (fixed) with a dense displacement field, on the device -> DeformableRegistration.  A
    demons iteration (Thirion's additive force of the squared difference, diffusion-regularised): u <- G_sigma * (u + v), v = d g / (|g|^2 + d^2 / delta^2) with d = f -
    m(T (p + u)), g the world gradient of f and delta = max_step x the level spacing, which bounds a step to delta / 2.  fixed, moving: as register_volumes takes them;
    rigid: a Registration, a RigidTransform or a 4 x 4, fixed world -> moving world.  field_sigma, image_sigma and max_step are in level voxels; a sigma of 0 means no
    smoothing.  mask: on the fixed grid, the voxels that may pull.
    Per level of levels_mm, coarse to fine: both volumes are put on isotropic grids of the level spacing over their own fields of view (unet_vol_resample_linear,
    float32; point-sampled, no anti-aliasing filter: the Gaussian comes after), the mask with the nearest kernel; both level images are smoothed with image_sigma; the
    field starts from zeros, or from the previous level's field put on this level's grid component by component; then iterations[level] times: one
    unet_vol_demons_step and three unet_vol_smooth_axis passes over the field.  There is no convergence test: the loop is the specification.  The starting values of
    levels_mm, iterations and the three widths are conventional and not clinically validated.
    ops: the operations the loop runs over (default: DeformOps(), the device); the tests hand in the numpy restatement.  Every argument error is a ValueError before any
    device work."""
    lv, its, wf, wi, step = _check_deform_args(levels_mm, iterations, field_sigma, image_sigma, max_step)
    T = _world_matrix(rigid)
    f, m = _resample_source(fixed, None, fixed_affine, fixed_shape), _resample_source(moving, None, moving_affine, moving_shape)
    fg, mg = _need_oriented(f.grid, "the fixed volume's grid"), _need_oriented(m.grid, "the moving volume's grid")
    mk = _check_fixed_mask(mask, f.shape)
    fgrids, mgrids = registration_level_grids(fg, lv), registration_level_grids(mg, lv)
    for _, g, _ in fgrids + mgrids:
        _check_volume_dims(g.shape)
    ops = DeformOps() if ops is None else ops
    t0 = time.perf_counter()
    fd, md, mask_dev = ops.upload(f), ops.upload(m), ops.upload_mask(mk, f.shape)
    eye = np.eye(4)[:3]
    field = prev = None
    history = []

    def residual(fl, ml, mv, lmask, W, L, u, g):
        warped = ops.warp_field(ml, mv, W, L, u, g.shape, None, 1, 1, float("nan"), 0, g.shape, 64)
        return ops.rms(fl, warped, lmask)

    for (spacing, g, M), (_, gm, Mm), n_it in zip(fgrids, mgrids, its):
        fl = ops.linear(fd, f.vargs, eye if M is None else M, g.shape)
        ml = ops.linear(md, m.vargs, eye if Mm is None else Mm, gm.shape)
        lmask = mask_dev if (mask_dev is None or M is None) else ops.nearest_mask(mask_dev, f.shape, M, g.shape)
        if wi is not None:
            for axis in range(3):
                fl, ml = ops.smooth_axis(fl, 1, g.shape, axis, wi), ops.smooth_axis(ml, 1, gm.shape, axis, wi)
        fv, mv = (16,) + g.shape + (0, 1.0, 0.0), (16,) + gm.shape + (0, 1.0, 0.0)
        W = voxel_matrix(g, gm, T)
        L = _check_mat3((np.linalg.inv(gm.affine) @ T)[:3, :3], "L")
        Ginv = _check_mat3(np.linalg.inv(g.affine[:3, :3]).T, "Ginv")
        n = int(np.prod(g.shape))
        if prev is None:
            field = ops.zeros(3 * n)
        else:
            pn, Mf = int(np.prod(prev.shape)), resample_matrix(prev, g)
            field = ops.stack([ops.linear(field[c * pn:(c + 1) * pn], (16,) + prev.shape + (0, 1.0, 0.0), Mf, g.shape) for c in range(3)])
        r_start, _ = residual(fl, ml, mv, lmask, W, L, field, g)
        for _ in range(n_it):
            field = ops.demons_step(fl, fv, lmask, ml, mv, W, L, Ginv, step * spacing, field)
            if wf is not None:
                for axis in range(3):
                    field = ops.smooth_axis(field, 3, g.shape, axis, wf)
        r_end, counted = residual(fl, ml, mv, lmask, W, L, field, g)
        history.append(dict(spacing=spacing, shape=g.shape, iterations=n_it, residual_start=r_start, residual=r_end, voxels=counted))
        prev = g
    r_init, _ = residual(fl, ml, mv, lmask, W, L, ops.zeros(3 * n), prev)
    det, folded = ops.jacobian(field, prev.shape, np.linalg.inv(prev.affine[:3, :3]))
    jmin, jmax = ops.minmax(det)
    ops.sync()
    return DeformableRegistration(field=DisplacementField(field, prev, rigid, fg, mg), rigid=rigid, residual_init=r_init, residual=history[-1]["residual"], jacobian_min=jmin,
                                  jacobian_max=jmax, folded=folded, history=history, seconds=time.perf_counter() - t0)


# ---- the surface of a mask, a label volume or a scalar volume as a triangle mesh (csrc/kernels_mesh.hip) ---------------------------------------
# Marching tetrahedra on the Freudenthal split of every lattice cell: an indexed, consistently wound mesh whose vertices, triangle order and float32 coordinates are defined
# bit for bit by tests/mesh_oracle.py.  The surface has the topology of the lattice's 14-neighbourhood (6 axis neighbours, 6 face diagonals of one orientation, 2 body
# diagonals): two lesions that touch along such a diagonal share a surface.  The mesh of a BINARY mask is a staircase: its area is 26-27 % above a sphere's at every
# radius (it does not converge) and the sphericity of a binary ball is about 0.79, not 1; meshing a probability volume (segment_volume_ensemble's prob) at the threshold is
# the smooth alternative.  The shape figures are conventional, configurable (iso, pixdim / affine) and NOT clinically validated.
MESH_KINDS = ("mask", "labels", "scalar")
MESH_WHAT = ("infection", "lung", "both")
_MESH_KEYS = {"what", "out_path", "lesions"}
SHAPE_DTYPE = np.dtype([("label", np.int64), ("triangles", np.int64), ("area_mm2", np.float64), ("mesh_ml", np.float64), ("sphericity", np.float64),
                        ("surface_to_volume", np.float64)])


def shape_descriptors(area_mm2, volume_mm3):
    """-> (sphericity = pi^(1/3) (6 V)^(2/3) / A, surface_to_volume = A / V in 1 / mm), nan where the area or the volume is not positive"""
    a, v = np.asarray(area_mm2, np.float64), np.asarray(volume_mm3, np.float64)
    with np.errstate(all="ignore"):
        sph = np.where((a > 0) & (v > 0), np.pi ** (1.0 / 3.0) * np.power(6.0 * np.abs(v), 2.0 / 3.0) / a, np.nan)
        s2v = np.where(v > 0, a / v, np.nan)
    return sph, s2v


class SurfaceMesh:
    """vertices: float32 [nv, 3] (numpy, or the device tensor with return_device=True), in the frame named by `frame`: "world" (RAS+ millimetres of the grid's affine) or
    "scaled voxel" (voxel index times pixdim: the volume carried no orientation, and left and right are not guessed); triangles: int32 [nt, 3], wound so that normals point
    out of the inside; groups: int32 [nt] (the label at the inside end of the triangle's first edge) or None; closed: whether the volume was padded with a layer of outside
    samples; euler: nv - nt / 2 for a closed mesh (2 per sphere-like component, 0 for a torus), else None; area_mm2: the sum of the triangle areas; volume_ml: the sum of
    the signed volumes / 1000; group_ids / group_triangles / group_area_mm2 / group_volume_ml: the same per group (one group, 1, without groups=True; volume_mm3 / group_volume_mm3: the sums before the division); kind: "mask" |
    "labels" | "scalar"; iso; launches: the kernel calls made; seconds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def measure(self):
        """-> SHAPE_DTYPE rows, one per group: label, triangles, area_mm2, mesh_ml, sphericity, surface_to_volume"""
        t = np.zeros(len(self.group_ids), SHAPE_DTYPE)
        t["label"], t["triangles"], t["area_mm2"] = self.group_ids, self.group_triangles, self.group_area_mm2
        t["mesh_ml"] = self.group_volume_ml
        t["sphericity"], t["surface_to_volume"] = shape_descriptors(self.group_area_mm2, self.group_volume_mm3)
        return t

    def _host(self, a):
        return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()

    def write(self, path):
        """the mesh as .stl (binary), .ply (binary_little_endian, with the groups as a face property) or .obj, by the suffix"""
        mesh_min.write(path, self._host(self.vertices), self._host(self.triangles), self._host(self.groups))

    def __repr__(self):
        return (f"SurfaceMesh({len(self.vertices)} vertices, {len(self.triangles)} triangles, frame={self.frame!r}, closed={self.closed}, euler={self.euler}, "
                f"area_mm2={self.area_mm2:.6g}, volume_ml={self.volume_ml:.6g})")


def _mesh_kind(x, iso, select, groups):
    """mask | labels | scalar from what was given: iso= makes any volume a scalar one; a bool volume is always a mask; without iso a uint8 volume is a mask, any other
    integer one (and a file, when select= or groups= asks for labels) a label volume, and a float one is refused"""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        kind_of = "b" if x.dtype == torch.bool else ("f" if x.dtype.is_floating_point else "i")
        u8 = x.dtype == torch.uint8
    elif isinstance(x, (str, os.PathLike, nifti_min.NiftiVolume)):
        kind_of, u8 = "file", False
    else:
        a = np.asarray(x)
        kind_of, u8 = ("b" if a.dtype.kind == "b" else ("f" if a.dtype.kind not in "iu" else "i")), a.dtype == np.uint8
    wants_labels = groups or select != 0
    if kind_of == "b":
        if iso is not None:
            raise ValueError("a mask has no iso value: inside is non-zero")
        if wants_labels:
            raise ValueError("select= and groups= need a label volume, not a bool mask")
        return "mask"
    if iso is not None:
        if wants_labels:
            raise ValueError("select= and groups= need a label volume; iso= describes a scalar volume")
        return "scalar"
    if kind_of == "f":
        raise ValueError("a scalar volume needs iso=: inside is value > iso")
    if kind_of == "file":
        return "labels" if wants_labels else "mask"
    if u8 and not wants_labels:
        return "mask"
    return "labels"


def _check_mesh_args(kind, iso, select, closed, pad_value, groups):
    """-> (iso, select, pad_value) as the entry points take them"""
    if isinstance(select, bool) or not isinstance(select, (int, np.integer)) or select < 0 or select >= 2 ** 31:
        raise ValueError(f"select is a label (0: every non-zero label), not {select!r}")
    if not isinstance(closed, (bool, np.bool_)) or not isinstance(groups, (bool, np.bool_)):
        raise ValueError("closed and groups are True or False")
    if kind != "scalar":
        if pad_value is not None:
            raise ValueError("pad_value belongs to a scalar volume: the virtual layer around a mask is simply outside")
        return 0.5, int(select), 0.0
    try:
        iso = float(iso)
        pad = iso if pad_value is None else float(pad_value)
    except (TypeError, ValueError):
        raise ValueError(f"iso and pad_value are finite numbers, not {iso!r}, {pad_value!r}") from None
    if not np.isfinite(iso) or not np.isfinite(pad):
        raise ValueError(f"iso and pad_value are finite numbers, not {iso!r}, {pad_value!r}")
    if pad > iso:
        raise ValueError(f"pad_value = {pad} > iso = {iso}: the virtual layer around the volume must be outside")
    return iso, 0, pad


def _check_mesh_lattice(shape, closed):
    p = 2 if closed else 0
    if (shape[0] + p) * (shape[1] + p) * (shape[2] + p) >= 2 ** 31:
        raise ValueError(f"the lattice of a {shape[0]} x {shape[1]} x {shape[2]} volume has 2^31 points or more")


def mesh_count_device(dev, kind, vargs, iso, select, closed, pad_value):
    """unet_vol_mesh_count -> (vertices, triangles, workspace): the two totals on the host and the filled workspace unet_vol_mesh_emit reads"""
    torch = _torch(); lib, ctx = _ctx()
    code, X, Y, Z, scaled, slope, inter = vargs
    ws = torch.empty(max(int(lib.unet_vol_mesh_ws_bytes(X, Y, Z, int(closed))), 16), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_mesh_count(ctx.handle, dev.data_ptr(), MESH_KINDS.index(kind), code, X, Y, Z, scaled, float(slope), float(inter), float(iso), int(select),
                                      int(closed), float(pad_value), ws.data_ptr(), ws.numel(), totals.data_ptr(), _stream()), "vol_mesh_count")
    nv, nt = (int(v) for v in totals.cpu().numpy())
    return nv, nt, ws


def mesh_emit_device(dev, kind, vargs, iso, select, closed, pad_value, M, ws, nv, nt, want_groups=True):
    """unet_vol_mesh_emit after mesh_count_device -> device tensors (vertices float32 [nv, 3], triangles int32 [nt, 3], groups int32 [nt] or None)"""
    torch = _torch(); lib, ctx = _ctx()
    if nv >= 2 ** 31 or nt >= 2 ** 31:
        raise ValueError(f"a mesh of {nv} vertices and {nt} triangles has 2^31 of either or more")
    code, X, Y, Z, scaled, slope, inter = vargs
    m = np.ascontiguousarray(np.asarray(M, np.float64)[:3, :4]).reshape(12)
    v = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    t = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    g = torch.empty(nt, dtype=torch.int32, device="cuda") if want_groups else None
    ctx.check(lib.unet_vol_mesh_emit(ctx.handle, dev.data_ptr(), MESH_KINDS.index(kind), code, X, Y, Z, scaled, float(slope), float(inter), float(iso), int(select),
                                     int(closed), float(pad_value), m.ctypes.data, ws.data_ptr(), ws.numel(), v.data_ptr() if nv else None, nv,
                                     t.data_ptr() if nt else None, _ptr(g) if nt else None, nt, _stream()), "vol_mesh_emit")
    return v, t, g


def mesh_measure_device(vertices, triangles):
    """unet_vol_mesh_measure -> device float64 (area [nt], signed volume [nt]) of the triangles, in the units of the vertices (mm^2, mm^3)"""
    torch = _torch(); lib, ctx = _ctx()
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    area = torch.empty(nt, dtype=torch.float64, device="cuda")
    vol = torch.empty(nt, dtype=torch.float64, device="cuda")
    if nt:
        ctx.check(lib.unet_vol_mesh_measure(ctx.handle, vertices.data_ptr() if nv else None, nv, triangles.data_ptr(), nt, area.data_ptr(), vol.data_ptr(), _stream()),
                  "vol_mesh_measure")
    return area, vol


def mesh_group_sums(per_triangle, groups):
    """The two-level sums of unet_vol_group_moments (the same bits on every run) of device float64 [k, nt] quantities: over all triangles, and per group after a stable
    device sort of the triangle groups -> (totals float64 [k], ids int64 [G], triangles per group int64 [G], sums float64 [k, G]); groups None: one group, 1."""
    torch = _torch()
    k, nt = int(per_triangle.shape[0]), int(per_triangle.shape[1])
    if nt == 0:
        return np.zeros(k), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((k, 0))
    whole = np.array([0, nt], np.int64)
    totals = np.array([group_moments_device(per_triangle[i], whole, 1)[0, 0] for i in range(k)], np.float64)
    if groups is None:
        return totals, np.array([1], np.int64), np.array([nt], np.int64), totals.reshape(k, 1).copy()
    sg, perm = torch.sort(groups, stable=True)
    ids, counts = torch.unique_consecutive(sg, return_counts=True)
    ids, counts = ids.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    sums = np.stack([group_moments_device(per_triangle[i][perm], offsets, len(ids))[:, 0] for i in range(k)])
    return totals, ids, counts, sums


def extract_surface(x, iso=None, select=0, closed=True, pad_value=None, pixdim=None, affine=None, groups=False, return_device=False, shape=None):
    """The surface of a volume as a SurfaceMesh, extracted and measured on the device.  x: a mask (bool or uint8: inside = non-zero), a label volume (any other integer
    dtype: inside = label == select, or every non-zero label with select=0; groups=True keeps the label of every triangle), a scalar volume (iso= required, which makes a
    volume of ANY dtype a scalar one: inside = value > iso, a NaN is outside, a value equal to iso is outside), a path or a NiftiVolume (a mask, or with select= / groups=
    a label volume, or with iso= the decoded scalar volume), or a flat Fortran-order device tensor together with shape=(X, Y, Z).  closed=True surrounds the volume with one
    layer of outside samples (of value pad_value <= iso for a scalar volume, default iso: the cap then lies on the virtual layer), so that a surface that touches the border
    is closed; closed=False meshes the real cells only.  The frame is the grid's: affine=, else the file's own, else diag(pixdim or the file's pixdim) -- "scaled voxel",
    and the mesh says so: left and right are never guessed.  Vertex normals, decimation and smoothing are out of scope."""
    torch = _torch()
    t0 = time.perf_counter()
    kind = _mesh_kind(x, iso, select, groups)
    iso_v, select_v, pad_v = _check_mesh_args(kind, iso, select, closed, pad_value, groups)
    if kind == "mask" and not isinstance(x, (torch.Tensor, str, os.PathLike, nifti_min.NiftiVolume)):
        x = np.asarray(x)
        if x.dtype.kind == "b":
            x = x.astype(np.uint8)
    src = _resample_source(x, pixdim, affine, shape, {"mask": "mask", "labels": "labels", "scalar": "volume"}[kind])
    _check_mesh_lattice(src.shape, closed)
    dev = src.tensor if src.tensor is not None else upload(src.vol)
    M = src.grid.affine[:3]
    nv, nt, ws = mesh_count_device(dev, kind, src.vargs, iso_v, select_v, closed, pad_v)
    v, t, g = mesh_emit_device(dev, kind, src.vargs, iso_v, select_v, closed, pad_v, M, ws, nv, nt, want_groups=bool(groups))
    del ws
    area, vol = mesh_measure_device(v, t)
    totals, ids, counts, sums = mesh_group_sums(torch.stack([area, vol]), g)
    launches = ["vol_mesh_count", "vol_mesh_emit"] + (["vol_mesh_measure", "vol_group_moments"] if nt else [])
    if not return_device:
        torch.cuda.synchronize()
        v, t, g = v.cpu().numpy(), t.cpu().numpy(), (None if g is None else g.cpu().numpy())
    return SurfaceMesh(vertices=v, triangles=t, groups=g, frame="world" if src.grid.oriented else "scaled voxel", closed=bool(closed),
                       euler=(nv - nt // 2) if closed else None, area_mm2=float(totals[0]), volume_ml=float(totals[1]) / 1000.0, group_ids=ids, group_triangles=counts,
                       group_area_mm2=sums[0], group_volume_mm3=sums[1], group_volume_ml=sums[1] / 1000.0, volume_mm3=float(totals[1]), kind=kind, iso=(iso_v if kind == "scalar" else None), matrix=np.array(M, np.float64),
                       grid=src.grid, launches=launches, seconds=time.perf_counter() - t0)


def lesion_shapes(labels, n, pixdim=None, affine=None, shape=None, return_mesh=False):
    """One extract_surface(labels, groups=True) call over a label volume (what label_volume returned: numpy [X, Y, Z], or the device tensor with shape=) -> SHAPE_DTYPE
    rows keyed like component_table, label 1..n: triangles, area_mm2, mesh_ml (the volume the closed surface encloses), sphericity, surface_to_volume.  Two lesions that
    touch along a diagonal of the lattice's 14-neighbourhood share one surface: every triangle still belongs to the label on its inside, but each label's patch is then
    open -- its area stays right, its mesh_ml and sphericity are those of an open patch and depend on the frame's origin.  Labels of label_volume(connectivity=3) never
    touch that way: every lesion's surface is closed.  A label outside 1..n is an error; a label without voxels has zeros and nan.  return_mesh=True: (table, SurfaceMesh)."""
    torch = _torch()
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"n is the number of labels, not {n!r}")
    if not isinstance(labels, torch.Tensor):
        a = np.asarray(labels) if not isinstance(labels, (str, os.PathLike, nifti_min.NiftiVolume)) else None
        if a is not None and (a.ndim != 3 or a.dtype.kind not in "iu"):
            raise ValueError(f"labels are an integer [X, Y, Z] volume, not {a.dtype} with {a.ndim} dimensions")
        if a is not None and a.dtype == np.uint8:
            labels = a.astype(np.int32)
    elif labels.dtype != torch.int32:
        raise ValueError("device labels are an int32 tensor")
    mesh = extract_surface(labels, groups=True, pixdim=pixdim, affine=affine, shape=shape)
    if len(mesh.group_ids) and (mesh.group_ids.min() < 1 or mesh.group_ids.max() > n):
        raise ValueError(f"the volume holds labels outside 1..{int(n)}")
    table = np.zeros(int(n), SHAPE_DTYPE)
    table["label"] = np.arange(1, int(n) + 1)
    table["sphericity"] = table["surface_to_volume"] = np.nan
    if len(mesh.group_ids):
        table[mesh.group_ids - 1] = mesh.measure()
    return (table, mesh) if return_mesh else table


def _check_mesh(mesh, lung_mask):
    """segment_volume's mesh= -> None (off) or the checked dict {what, out_path, lesions}"""
    if mesh is None or mesh is False:
        return None
    kw = {} if mesh is True else (dict(mesh) if isinstance(mesh, dict) else None)
    if kw is None:
        raise ValueError(f"mesh is True or a dict with {sorted(_MESH_KEYS)}, not {mesh!r}")
    if set(kw) - _MESH_KEYS:
        raise ValueError(f"mesh takes {sorted(_MESH_KEYS)}, not {sorted(set(kw) - _MESH_KEYS)}")
    kw.setdefault("what", "infection"); kw.setdefault("out_path", None); kw.setdefault("lesions", False)
    if kw["what"] not in MESH_WHAT:
        raise ValueError(f"mesh: what is one of {list(MESH_WHAT)}, not {kw['what']!r}")
    if kw["what"] != "infection" and lung_mask is None:
        raise ValueError(f"mesh: what={kw['what']!r} needs lung_mask")
    if not isinstance(kw["lesions"], (bool, np.bool_)):
        raise ValueError("mesh: lesions is True or False")
    if kw["out_path"] is not None:
        mesh_min.format_of(kw["out_path"])
    return kw


def _lung_mesh_path(path):
    root, ext = os.path.splitext(os.fspath(path))
    return root + "_lung" + ext


def _segmentation_meshes(kw, vol, lv, mask_dev, shape, connectivity):
    """the mesh= step of _finish_segmentation -> (mesh of the final mask or None, lung mesh or None); the frame is the CT's affine, else its pixdim"""
    where = dict(affine=vol.affine) if vol.affine is not None else dict(pixdim=vol.pixdim)
    mesh, lung = None, None
    if kw["what"] in ("infection", "both"):
        if kw["lesions"]:
            own, n_own = label_device(mask_dev, shape, connectivity)
            table, mesh = lesion_shapes(own, n_own, shape=shape, return_mesh=True, **where)
            mesh.lesions = table
            del own
        else:
            mesh = extract_surface(mask_dev, shape=shape, **where)
        if kw["out_path"] is not None:
            mesh.write(kw["out_path"])
    if kw["what"] in ("lung", "both"):
        lung = extract_surface((lv.get_fdata() != 0).astype(np.uint8), **where)
        if kw["out_path"] is not None:
            lung.write(kw["out_path"] if kw["what"] == "lung" else _lung_mesh_path(kw["out_path"]))
    return mesh, lung

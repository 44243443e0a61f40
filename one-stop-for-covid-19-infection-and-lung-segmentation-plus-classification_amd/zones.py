"""Where the infection sits in the lungs (csrc/kernels_zones.hip).

    lung_zones(sides, zones=, ap_parts=, extent=, depth=, fill=)      -> LungZones: every lung voxel's side x anatomical zone x depth shell under the lung surface -- the
                                                                         spec of the binning, the distance volume (on the device) and the zone map
    lung_distribution(infection, sides_or_zones, labels=, n=)         -> LungDistribution: lung and infected voxels per region, per shell and per side, a row per lesion,
                                                                         a semi-quantitative severity score per region and the words of a report (bilateral, upper /
                                                                         lower, peripheral / central)
    side_extents_device / zone_table_device                           -> the two entries (unet_vol_side_extents, unet_vol_zone_table) on device tensors

What the words mean here, plainly.  A ZONE is an equal part of a lung's bounding range along one voxel axis (the axis whose code is S or I; with ap_parts the A / P axis
as well): thirds of the range, NOT lobes -- fissures are unknown to this package.  DEPTH is the exact Euclidean distance (unet_vol_edt_sq, mm) of a lung voxel to the
nearest voxel outside the lungs, whichever surface that is: the costal pleura, the diaphragm and the MEDIASTINAL surface alike, so "peripheral" is "near any lung
surface".  The severity thresholds and the predominance share are conventional, configurable and NOT clinically validated here.  The device counts in integers; the host
turns a few hundred counters into the report.  There is no CPU fallback for the device steps.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

from . import _lib
from . import volume as V

MAX_PARTS, MAX_SHELLS, MAX_BINS = _lib.ZONE_MAX_PARTS, _lib.ZONE_MAX_SHELLS, _lib.ZONE_MAX_BINS
SEVERITY_EDGES = (5, 25, 50, 75)                                    # per cent of a region's lung voxels; conventional (the published lobe score), configurable, not validated here
PREDOMINANCE = 0.5
DEPTH_DEFAULT = ("relative", (1 / 3, 2 / 3))
SIDE_NAMES = ("left", "right")                                      # by side value 1, 2
NONE_KEY = 2 ** 64 - 1
REGION_DTYPE = np.dtype([("side", "U5"), ("zone", np.int32), ("ap", np.int32), ("lung_voxels", np.int64), ("infected_voxels", np.int64), ("lung_ml", np.float64),
                         ("infected_ml", np.float64), ("fraction", np.float64), ("score", np.int32)])
SHELL_DTYPE = np.dtype([("side", "U5"), ("shell", np.int32), ("lung_voxels", np.int64), ("infected_voxels", np.int64), ("lung_ml", np.float64), ("infected_ml", np.float64),
                        ("fraction", np.float64)])
_DISTRIBUTION_KEYS = {"zones", "ap_parts", "extent", "depth", "fill", "severity_edges", "predominance"}


def lesion_dtype(S):
    return np.dtype([("label", np.int32), ("side", "U5"), ("zone", np.int32), ("ap", np.int32), ("voxels_in_lung", np.int64), ("voxels_shell", np.int64, (int(S),)),
                     ("depth_mm", np.float64), ("subpleural", np.bool_)])


def zone_names(zones):
    return {1: ("all",), 2: ("upper", "lower"), 3: ("upper", "middle", "lower")}.get(int(zones), tuple(f"zone{k}" for k in range(int(zones))))


def key_to_double(k):
    """the double behind an order-preserving key (include/unet_hip.h); key 0 -- no voxel -- gives 0.0"""
    k = int(k)
    if k == 0:
        return 0.0
    u = (k ^ (1 << 63)) if (k >> 63) else (~k & NONE_KEY)
    return float(np.array([u], np.uint64).view(np.float64)[0])


# ---- the arguments ------------------------------------------------------------------------------------------------------------------------------------------
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_zone_args(zones=3, ap_parts=1, extent="per_lung", depth=DEPTH_DEFAULT, fill=True):
    """-> (zones, ap_parts, extent, depth = None or (mode, values), fill), or ValueError: no device is needed"""
    if not _is_int(zones) or not 1 <= int(zones) <= MAX_PARTS:
        raise ValueError(f"zones is an integer in 1..{MAX_PARTS}, not {zones!r}")
    if not _is_int(ap_parts) or not 1 <= int(ap_parts) <= MAX_PARTS:
        raise ValueError(f"ap_parts is an integer in 1..{MAX_PARTS}, not {ap_parts!r}")
    if extent not in ("per_lung", "both"):
        raise ValueError(f'extent is "per_lung" or "both", not {extent!r}')
    if not isinstance(fill, (bool, np.bool_)):
        raise ValueError(f"fill is True or False, not {fill!r}")
    if depth is not None:
        try:
            mode, values = depth
            values = tuple(float(v) for v in values)
        except (TypeError, ValueError):
            raise ValueError(f'depth is None, ("mm", radii) or ("relative", fractions), not {depth!r}') from None
        if mode not in ("mm", "relative"):
            raise ValueError(f'depth is None, ("mm", radii) or ("relative", fractions), not {depth!r}')
        if not 1 <= len(values) <= MAX_SHELLS - 1:
            raise ValueError(f"depth takes 1..{MAX_SHELLS - 1} boundaries ({MAX_SHELLS} shells at the most), not {len(values)}")
        if not all(math.isfinite(v) and v > 0.0 for v in values) or any(b <= a for a, b in zip(values, values[1:])):
            raise ValueError(f"the boundaries of depth are positive, finite and strictly ascending, not {values!r}")
        if mode == "relative" and values[-1] >= 1.0:
            raise ValueError(f"relative boundaries are fractions of the largest depth, below 1, not {values!r}")
        if mode == "mm" and not all(math.isfinite(v * v) for v in values):
            raise ValueError(f"a radius of depth has no finite square: {values!r}")
        depth = (mode, values)
    if 2 * int(zones) * int(ap_parts) * (1 if depth is None else len(depth[1]) + 1) > MAX_BINS or 2 * int(zones) * int(ap_parts) > 255:
        raise ValueError(f"2 x {zones} zones x {ap_parts} AP parts x the shells are more than {MAX_BINS} bins (or more than 255 regions)")
    return int(zones), int(ap_parts), extent, depth, bool(fill)


def _check_report_args(severity_edges=SEVERITY_EDGES, predominance=PREDOMINANCE):
    """-> (edges as exact fractions, the predominance share as an exact fraction), or ValueError"""
    try:
        edges = tuple(Fraction(e) for e in severity_edges)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"severity_edges are ascending percentages in (0, 100], not {severity_edges!r}") from None
    if not edges or any(not 0 < e <= 100 for e in edges) or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"severity_edges are strictly ascending percentages in (0, 100], not {severity_edges!r}")
    try:
        share = Fraction(predominance)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"predominance is a share in (0, 1], not {predominance!r}") from None
    if isinstance(predominance, bool) or not 0 < share <= 1:
        raise ValueError(f"predominance is a share in (0, 1], not {predominance!r}")
    return edges, share


def _check_distribution(distribution, per_lung):
    """segment_volume's distribution= -> None (off) or (the checked keyword arguments of lung_zones, those of the report)"""
    if distribution is None or distribution is False:
        return None
    kw = {} if distribution is True else dict(distribution)
    if set(kw) - _DISTRIBUTION_KEYS:
        raise ValueError(f"distribution takes {sorted(_DISTRIBUTION_KEYS)}, not {sorted(set(kw) - _DISTRIBUTION_KEYS)}")
    rep = {k: kw.pop(k) for k in ("severity_edges", "predominance") if k in kw}
    _check_zone_args(**kw)
    _check_report_args(**rep)
    if per_lung is None:
        raise ValueError("distribution needs per_lung: the zones are cut from the two lungs it splits")
    return kw, rep


def zone_axes(axcodes):
    """-> (the voxel axis running cranio-caudally, the one running antero-posteriorly, flip [3]): zone 0 is the most superior part and AP part 0 the most anterior, so an
    axis that grows towards S (towards A) is numbered against its coordinate"""
    codes = tuple(str(c) for c in axcodes)
    si = [j for j, c in enumerate(codes) if c in "SI"][0]
    ap = [j for j, c in enumerate(codes) if c in "AP"][0]
    flip = [0, 0, 0]
    flip[si] = 1 if codes[si] == "S" else 0
    flip[ap] = 1 if codes[ap] == "A" else 0
    return si, ap, tuple(flip)


def make_spec(parts, flip, lo, extent, r2=((), ())):
    """-> _lib.ZoneSpec (unet_zone_spec); r2: per side, the S - 1 squared radii"""
    spec = _lib.ZoneSpec()
    S = len(r2[0]) + 1
    if len(r2[1]) + 1 != S or not 1 <= S <= MAX_SHELLS:
        raise ValueError(f"r2 holds the same number (0..{MAX_SHELLS - 1}) of squared radii per side")
    for a in range(3):
        spec.parts[a], spec.flip[a] = int(parts[a]), int(flip[a])
        for s in (0, 1):
            spec.lo[s][a], spec.extent[s][a] = int(lo[s][a]), int(extent[s][a])
    spec.shells = S
    for s in (0, 1):
        for k in range(S - 1):
            spec.r2[s][k] = float(r2[s][k])
    return spec


# ---- the two entries ----------------------------------------------------------------------------------------------------------------------------------------
def side_extents_device(sides_dev, d2_dev, shape):
    """unet_vol_side_extents -> (box int32 [2, 6] = {x0, x1, y0, y1, z0, z1} of side 1 and 2, inclusive; dmax_key uint64 [2]), numpy"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = shape
    V._check_volume_dims(shape)
    box = torch.empty((2, 6), dtype=torch.int32, device="cuda")
    dmax = torch.empty(2, dtype=torch.int64, device="cuda")
    if X * Y * Z == 0:                                               # the entry touches nothing
        return np.array([[2 ** 31 - 1, -1] * 3] * 2, np.int32), np.zeros(2, np.uint64)
    ctx.check(lib.unet_vol_side_extents(ctx.handle, sides_dev.data_ptr(), V._ptr(d2_dev), X, Y, Z, box.data_ptr(), dmax.data_ptr(), V._stream()), "vol_side_extents")
    return box.cpu().numpy(), dmax.cpu().numpy().view(np.uint64)


def zone_table_device(sides_dev, spec, shape, infection_dev=None, labels_dev=None, n=0, d2_dev=None, want_map=False):
    """unet_vol_zone_table -> dict: table int64 [B, 2], outside, lesion_zone int64 [n, 2P], lesion_shell int64 [n, S], lesion_dmin_key uint64 [n] (numpy) and zone_map (the
    uint8 device tensor, None unless want_map)"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = shape
    V._check_volume_dims(shape)
    n = int(n)
    P, S = int(spec.parts[0]) * int(spec.parts[1]) * int(spec.parts[2]), int(spec.shells)
    table = torch.zeros((2 * P * S, 2), dtype=torch.int64, device="cuda")
    outside = torch.zeros(1, dtype=torch.int64, device="cuda")
    lz = torch.zeros((max(n, 1), 2 * P), dtype=torch.int64, device="cuda")
    lsh = torch.zeros((max(n, 1), S), dtype=torch.int64, device="cuda")
    ld = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    zmap = torch.zeros(X * Y * Z, dtype=torch.uint8, device="cuda") if want_map else None
    ctx.check(lib.unet_vol_zone_table(ctx.handle, sides_dev.data_ptr(), V._ptr(infection_dev), V._ptr(labels_dev), n, V._ptr(d2_dev), X, Y, Z, C.byref(spec), table.data_ptr(),
                                      outside.data_ptr(), lz.data_ptr(), lsh.data_ptr(), ld.data_ptr(), V._ptr(zmap), V._stream()), "vol_zone_table")
    return {"table": table.cpu().numpy(), "outside": int(outside.item()), "lesion_zone": lz[:n].cpu().numpy(), "lesion_shell": lsh[:n].cpu().numpy(),
            "lesion_dmin_key": ld[:n].cpu().numpy().view(np.uint64), "zone_map": zmap}


# ---- the zones of two lungs ---------------------------------------------------------------------------------------------------------------------------------------
class LungZones:
    """What lung_zones returns.  spec: the unet_zone_spec of the binning (parts, flip, lo, extent, shells, r2); box: int32 [2, 6], the inclusive bounding box of the left and
    the right lung; dmax_mm: (left, right) the largest depth of each lung (nan without depth); r_mm: per side the radii between the shells; zones, ap_parts, shells;
    si_axis / ap_axis: the voxel axes the zones / the AP parts are cut along; d2: the squared depth of every voxel as a float64 device tensor (None with depth=None);
    zone_map: uint8 [X, Y, Z] (numpy, Fortran order; return_device=True: the flat device tensor), 0 off the lungs, else region_codes[side, zone, ap] of the voxel's region;
    region_codes: uint8 [2, zones, ap_parts]; lung_voxels: int64 [2, zones, ap_parts, shells]; sides: the flat 0 / 1 / 2 device tensor the zones were cut from; shape,
    axcodes, pixdim."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"LungZones(zones={self.zones}, ap_parts={self.ap_parts}, shells={self.shells}, axcodes={self.axcodes})"


def region_order(parts, si, ap):
    """the device's (side, zone) index 0 .. 2P - 1 of every anatomical region, in the report's order: side, then cranio-caudal zone, then AP part"""
    P = int(parts[0]) * int(parts[1]) * int(parts[2])
    mul = (1, int(parts[0]), int(parts[0]) * int(parts[1]))
    return np.array([t * P + cc * mul[si] + a * mul[ap] for t in (0, 1) for cc in range(int(parts[si])) for a in range(int(parts[ap]))], np.int64)


def _sides_to_device(sides, orientation, pixdim, shape):
    """lung_zones' first argument -> (flat uint8 device tensor, shape, axcodes or None, pixdim or None); nothing is uploaded before the orientation is known"""
    torch = V._torch()
    if isinstance(sides, V.LungSides):
        codes = sides.axcodes if orientation is None else V._check_orientation(orientation)[1]
        p = sides.pixdim if pixdim is None else pixdim
        vol, vshape = sides.sides, sides.shape
    else:
        codes = V._check_orientation(orientation)[1]
        p, vol, vshape = pixdim, sides, shape
    if codes is None:
        raise ValueError("lung_zones: nothing says which voxel direction is superior and which anterior; pass a LungSides with axcodes or orientation='LPS' (or the volume's "
                         "code) -- they are not guessed")
    if p is None:
        raise ValueError("lung_zones: a plain 0 / 1 / 2 volume needs pixdim=, the voxel's edge lengths in mm")
    p = V._check_pixdim(p)

    def upload():
        if isinstance(vol, torch.Tensor):
            if vshape is None:
                raise ValueError("device sides are a flat Fortran-order byte buffer: pass shape=(X, Y, Z)")
            shp = tuple(int(v) for v in vshape)
            if vol.dtype != torch.uint8 or not vol.is_cuda or vol.numel() != int(np.prod(shp)):
                raise ValueError(f"device sides are a uint8 cuda tensor of prod(shape) = {int(np.prod(shp))} elements")
            return vol.contiguous().reshape(-1), shp
        a = np.asarray(vol)
        if a.ndim != 3 or a.dtype.kind not in "biu":
            raise ValueError(f"sides is an integer [X, Y, Z] volume of 0 / 1 / 2, not {a.dtype} with {a.ndim} dimensions")
        return torch.from_numpy(np.asfortranarray(np.where((a >= 0) & (a <= 2), a, 0).astype(np.uint8)).reshape(-1, order="F")).cuda(), tuple(int(v) for v in a.shape)
    return upload, tuple(str(c) for c in codes), p


def lung_zones(sides, zones=3, ap_parts=1, extent="per_lung", depth=DEPTH_DEFAULT, fill=True, return_device=False, orientation=None, pixdim=None, shape=None):
    """The two lungs cut into anatomical zones and depth shells -> LungZones.  sides: a LungSides (its axcodes are required), or a plain 0 / 1 / 2 volume (host array, or a
    flat device uint8 tensor with shape=) together with orientation= (a 3-letter code such as "LPS" or a 4 x 4 affine) and pixdim=.  Without an orientation a ValueError is
    raised before any device work: superior and anterior are never guessed, as left and right are not.
      zones     equal parts of the bounding range along the voxel axis whose code is S or I; zone 0 is the most superior whatever the storage.  NOT lobes.
      ap_parts  the same along the A / P axis; part 0 is the most anterior.
      extent    "per_lung": each lung's own bounding range is divided; "both": the union of the two ranges.  A voxel at coordinate c lies in part
                floor((c - lo) parts / extent), clamped (unet_vol_zone_table); an empty lung takes lo = 0, extent = 1.
      depth     ("mm", radii): shell k holds the voxels deeper than k of the radii, so shell 0 touches the surface; ("relative", fractions): r = f * sqrt(dmax of that side),
                r2 = r * r in float64, dmax the largest squared depth of the side; None: no shells, no distance transform.
      fill      the depth is the distance to the nearest voxel outside fill_holes(sides != 0) (connectivity 1), so that a vessel or a dense lesion missing from the lung mask
                is not taken for pleura; False: outside sides != 0.  The distance is to ANY lung surface, the mediastinal one included.
    Every argument error is a ValueError raised before anything is uploaded or launched."""
    torch = V._torch()
    zones, ap_parts, extent, depth, fill = _check_zone_args(zones, ap_parts, extent, depth, fill)
    upload, codes, p = _sides_to_device(sides, orientation, pixdim, shape)
    si, ap, flip = zone_axes(codes)
    dev, vshape = upload()
    X, Y, Z = vshape
    V._check_volume_dims(vshape)
    d2 = None
    if depth is not None:
        lung = ((dev == 1) | (dev == 2)).to(torch.uint8)                # a value above 2 counts as 0, as in the kernels
        if fill:
            lung, _ = V.fill_holes_device(lung, vshape, 1)
        d2 = V.edt_sq_device(lung, vshape, p, features_nonzero=False)
        del lung
    box, dkey = side_extents_device(dev, d2, vshape)
    lo, ext = np.zeros((2, 3), np.int64), np.ones((2, 3), np.int64)
    for a in range(3):
        have = [t for t in (0, 1) if box[t, 2 * a + 1] >= 0]
        for t in (0, 1):
            if extent == "both" and have:
                first, last = min(int(box[u, 2 * a]) for u in have), max(int(box[u, 2 * a + 1]) for u in have)
                lo[t, a], ext[t, a] = first, last - first + 1
            elif extent == "per_lung" and t in have:
                lo[t, a], ext[t, a] = int(box[t, 2 * a]), int(box[t, 2 * a + 1]) - int(box[t, 2 * a]) + 1
    dmax = tuple(key_to_double(k) for k in dkey)
    if depth is None:
        radii = ((), ())
    elif depth[0] == "mm":
        radii = (depth[1], depth[1])
    else:
        radii = tuple(tuple(f * math.sqrt(dm) for f in depth[1]) for dm in dmax)
    if not all(math.isfinite(r * r) for row in radii for r in row):
        raise ValueError("lung_zones: the largest depth of a lung is not finite (no voxel lies outside the lungs): relative shells cannot be cut")
    parts = [1, 1, 1]
    parts[si], parts[ap] = zones, ap_parts
    spec = make_spec(parts, flip, lo, ext, tuple(tuple(r * r for r in row) for row in radii))
    S = int(spec.shells)
    zt = zone_table_device(dev, spec, vshape, d2_dev=d2, want_map=True)
    order = region_order(parts, si, ap)
    lung_voxels = zt["table"][:, 0].reshape(2 * zones * ap_parts, S)[order].reshape(2, zones, ap_parts, S)
    zmap = zt["zone_map"]
    return LungZones(spec=spec, box=box, dmax_mm=tuple(math.sqrt(dm) if depth is not None else float("nan") for dm in dmax), r_mm=radii, zones=zones, ap_parts=ap_parts,
                     shells=S, si_axis=si, ap_axis=ap, d2=d2, zone_map=zmap if return_device else zmap.cpu().numpy().reshape(vshape, order="F"),
                     region_codes=(1 + order).astype(np.uint8).reshape(2, zones, ap_parts), lung_voxels=lung_voxels, sides=dev, shape=vshape, axcodes=codes,
                     pixdim=tuple(float(v) for v in p), extent=extent, depth=depth, fill=fill)


# ---- the report -------------------------------------------------------------------------------------------------------------------------------------------------
class LungDistribution:
    """What lung_distribution returns.
      regions    REGION_DTYPE rows, one per side x zone x AP part (left first, zone 0 = the most superior, AP part 0 = the most anterior): lung_voxels, infected_voxels,
                 lung_ml, infected_ml, fraction = infected / lung (nan for an empty region) and the severity score
      shells     SHELL_DTYPE rows, one per side x shell (shell 0 touches the lung surface)
      left / right    volume.LungSideBurden of the whole lung
      outside_voxels / outside_ml    infected outside both lungs
      lesions    lesion_dtype(S) rows: label; side / zone / ap of the region holding most of its in-lung voxels (a tie goes to the lower region: left before right, upper
                 before lower, anterior before posterior; "none" / -1 when no voxel of it lies in a lung); voxels_in_lung; voxels_shell [S]; depth_mm = the smallest depth
                 of its voxels (nan without depth or in-lung voxels); subpleural = it has a voxel in shell 0 (False without depth)
      severity   {"scores": int [2, zones, ap_parts], "total", "max_total", "edges"}: per region 0 when no voxel is infected, else 1 + #{e : 100 infected >= e lung}
      bilateral; craniocaudal ("upper" / "middle" / "lower" / "diffuse", "none" without infection, None with one zone); axial ("peripheral" = shell 0, "central" = the
      innermost shell, "mixed"; None without shells); anteroposterior ("anterior" / "posterior" / "diffuse"; None unless ap_parts == 2): a category is named when it holds
      at least `predominance` of the infected in-lung voxels, den count >= num total in integers from the share's exact rational; the first such category wins.
      zones      the LungZones behind it; voxel_ml."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"LungDistribution(bilateral={self.bilateral}, craniocaudal={self.craniocaudal!r}, axial={self.axial!r}, "
                f"severity={self.severity['total']}/{self.severity['max_total']})")

    def layer(self, fill_alpha=96, outline_alpha=255):
        """a volume.Layer over the zone map for render_planes: every anatomical region in a colour of its own (PALETTE_LESIONS, cycled)"""
        z = self.zones
        codes = z.region_codes.reshape(-1)
        palette = np.zeros((int(codes.max()) + 1, 3), np.uint8)
        for r, c in enumerate(codes):
            palette[int(c)] = V.PALETTE_LESIONS[1 + r % (len(V.PALETTE_LESIONS) - 1)]
        return V.Layer(z.zone_map, palette, fill_alpha, outline_alpha)


def severity_score(infected, lung, edges=SEVERITY_EDGES):
    """0 when no voxel is infected, else 1 + #{e : 100 infected >= e lung} in integers (edges in per cent, taken as exact rationals): 0 .. 1 + len(edges)"""
    infected, lung = int(infected), int(lung)
    if infected == 0:
        return 0
    return 1 + sum(1 for e in (Fraction(e) for e in edges) if 100 * infected * e.denominator >= e.numerator * lung)


def predominant(counts, names, share=Fraction(1, 2), none="none", other="diffuse"):
    """the first category with den count >= num total; `none` when the total is 0, `other` when no category reaches the share"""
    share = Fraction(share)
    total = sum(int(c) for c in counts)
    if total == 0:
        return none
    for c, name in zip(counts, names):
        if share.denominator * int(c) >= share.numerator * total:
            return name
    return other


def distribution_from_tables(zt, lz, severity_edges=SEVERITY_EDGES, predominance=PREDOMINANCE):
    """the tables of unet_vol_zone_table (zone_table_device's dict) and the LungZones they were counted on -> LungDistribution"""
    edges, share = _check_report_args(severity_edges, predominance)
    zones, apn, S = lz.zones, lz.ap_parts, lz.shells
    P = zones * apn
    voxel_ml = float(np.prod(np.asarray(lz.pixdim, np.float64))) / 1000.0
    parts = [int(lz.spec.parts[a]) for a in range(3)]
    order = region_order(parts, lz.si_axis, lz.ap_axis)
    t = np.asarray(zt["table"], np.int64).reshape(2 * P, S, 2)[order]
    reg = t.sum(axis=1)                                               # [2 P, 2] in the report's order
    regions = np.zeros(2 * P, REGION_DTYPE)
    for r in range(2 * P):
        lung, infd = int(reg[r, 0]), int(reg[r, 1])
        regions[r] = (SIDE_NAMES[r // P], (r % P) // apn, r % apn, lung, infd, lung * voxel_ml, infd * voxel_ml, (infd * voxel_ml) / (lung * voxel_ml) if lung else float("nan"),
                      severity_score(infd, lung, edges))
    sh = t.reshape(2, P, S, 2).sum(axis=1)
    shells = np.zeros(2 * S, SHELL_DTYPE)
    for s in (0, 1):
        for k in range(S):
            lung, infd = int(sh[s, k, 0]), int(sh[s, k, 1])
            shells[s * S + k] = (SIDE_NAMES[s], k, lung, infd, lung * voxel_ml, infd * voxel_ml, (infd * voxel_ml) / (lung * voxel_ml) if lung else float("nan"))
    side = reg.reshape(2, P, 2).sum(axis=1)
    lesz = np.asarray(zt["lesion_zone"], np.int64).reshape(-1, 2 * P)[:, order]
    lsh = np.asarray(zt["lesion_shell"], np.int64).reshape(-1, S)
    lesions = np.zeros(len(lesz), lesion_dtype(S))
    for i in range(len(lesz)):
        inl = int(lesz[i].sum())
        r = int(np.argmax(lesz[i])) if inl else -1
        deep = math.sqrt(key_to_double(zt["lesion_dmin_key"][i])) if inl and lz.d2 is not None else float("nan")
        lesions[i] = (i + 1, SIDE_NAMES[r // P] if inl else "none", (r % P) // apn if inl else -1, r % apn if inl else -1, inl, lsh[i], deep,
                      bool(lz.d2 is not None and lsh[i, 0] > 0))
    scores = regions["score"].astype(np.int64).reshape(2, zones, apn)
    inf_r = regions["infected_voxels"].reshape(2, zones, apn)
    inf_shell = sh[:, :, 1].sum(axis=0)
    return LungDistribution(regions=regions, shells=shells, left=V.LungSideBurden(side[0, 0], side[0, 1], voxel_ml), right=V.LungSideBurden(side[1, 0], side[1, 1], voxel_ml),
                            outside_voxels=int(zt["outside"]), outside_ml=int(zt["outside"]) * voxel_ml, lesions=lesions,
                            severity={"scores": scores, "total": int(scores.sum()), "max_total": int(scores.size * (1 + len(edges))), "edges": tuple(severity_edges)},
                            bilateral=bool(side[0, 1] > 0 and side[1, 1] > 0),
                            craniocaudal=None if zones == 1 else predominant(inf_r.sum(axis=(0, 2)), zone_names(zones), share),
                            axial=None if S == 1 else predominant((inf_shell[0], inf_shell[-1]), ("peripheral", "central"), share, other="mixed"),
                            anteroposterior=predominant(inf_r.sum(axis=(0, 1)), ("anterior", "posterior"), share) if apn == 2 else None,
                            zones=lz, voxel_ml=voxel_ml, predominance=predominance)


def lung_distribution(infection, sides_or_zones, labels=None, n=None, pixdim=None, severity_edges=SEVERITY_EDGES, predominance=PREDOMINANCE, connectivity=1, shape=None):
    """Where in the lungs an infection mask sits -> LungDistribution.  infection: a host [X, Y, Z] mask (non-zero = infected) or a flat device uint8 tensor with shape=;
    sides_or_zones: a LungZones, or a LungSides (cut with lung_zones' defaults: thirds, three relative depth shells); labels / n: the infection's lesions as label_volume
    returned them (host array or device int32 tensor) -- without them the mask is labelled here with `connectivity`; pixdim: the voxel's edge lengths for the millilitres,
    default the zones' own.
    severity: the published semi-quantitative CT score -- 0 for no involvement, 1 for under 5 %, 2 for 5 - 25 %, 3 for 25 - 50 %, 4 for 50 - 75 %, 5 above -- which the
    literature applies to the five LOBES; here it is applied to ZONES, equal parts of a bounding range.  The thresholds (severity_edges, per cent) and the predominance share
    are conventional and configurable and are NOT clinically validated here.  One pass over the volume (unet_vol_zone_table) counts everything."""
    torch = V._torch()
    _check_report_args(severity_edges, predominance)
    connectivity = V._check_connectivity(connectivity)
    if labels is not None and n is None:
        raise ValueError("labels need n, the number of lesions (what label_volume returned)")
    if labels is not None and int(n) < 0:
        raise ValueError(f"n is the number of lesions, not {n}")
    if pixdim is not None:
        pixdim = V._check_pixdim(pixdim)
    if not isinstance(sides_or_zones, (LungZones, V.LungSides)):
        raise ValueError("sides_or_zones is a LungZones (lung_zones) or a LungSides (split_lungs)")
    if isinstance(sides_or_zones, V.LungSides) and sides_or_zones.axcodes is None:
        raise ValueError("lung_distribution: the LungSides carries no axcodes; cut the zones with lung_zones(..., orientation=)")
    zshape = tuple(int(v) for v in sides_or_zones.shape)
    V._check_mask_host(infection, shape)
    if not isinstance(infection, torch.Tensor) and tuple(np.asarray(infection).shape) != zshape:
        raise ValueError(f"the infection mask is {tuple(np.asarray(infection).shape)}, the lungs {zshape}")
    if isinstance(infection, torch.Tensor) and shape is not None and tuple(int(v) for v in shape) != zshape:
        raise ValueError(f"the infection mask is {tuple(shape)}, the lungs {zshape}")
    lz = sides_or_zones if isinstance(sides_or_zones, LungZones) else lung_zones(sides_or_zones, return_device=True)
    inf_dev, vshape = V._mask_to_device(infection, shape if isinstance(infection, torch.Tensor) else None)
    if labels is None:
        labels_dev, n = V.label_device(inf_dev, vshape, connectivity)
    elif isinstance(labels, torch.Tensor):
        if labels.dtype != torch.int32 or labels.numel() != int(np.prod(vshape)):
            raise ValueError(f"device labels are an int32 cuda tensor of the infection mask's shape {vshape}")
        labels_dev = labels.contiguous().reshape(-1)
    else:
        a = np.asarray(labels)
        if tuple(a.shape) != vshape or a.dtype.kind not in "iu":
            raise ValueError(f"labels are an integer volume of the infection mask's shape {vshape}")
        labels_dev = torch.from_numpy(np.asfortranarray(np.where((a >= 1) & (a <= int(n)), a, 0).astype(np.int32)).reshape(-1, order="F")).cuda()
    zt = zone_table_device(lz.sides, lz.spec, vshape, inf_dev, labels_dev, int(n), lz.d2)
    if pixdim is not None and tuple(float(v) for v in pixdim) != lz.pixdim:
        lz = LungZones(**{**lz.__dict__, "pixdim": tuple(float(v) for v in pixdim)})
    return distribution_from_tables(zt, lz, severity_edges, predominance)

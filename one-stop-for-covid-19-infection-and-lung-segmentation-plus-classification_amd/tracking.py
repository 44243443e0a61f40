"""Every lesion from a baseline scan to its follow-up (csrc/kernels_track.hip).

    label_pairs(labels_a, n_a, labels_b, n_b)     -> the sparse contingency table of two label volumes on one grid: records (a, b, voxels) sorted by (a, b), counted on the
                                                  device in one pass (unet_vol_label_pairs)
    match_lesions(pairs, n_a, n_b)                -> LesionMatch: the lesions of both sides grouped into tracks (connected groups of the overlap graph), an event per track
                                                  (persistent / merged / split / complex / new / resolved) and the lookup tables label -> track.  Pure numpy.
    track_lesions(mask_a, grid_a, mask_b, grid_b, transform=)     -> LesionTracking: the follow-up put onto the baseline's grid as change_between puts it there, both
                                                  labelled, matched, and tabulated per track: voxels, millilitres, change, Dice, centroids, shift, doubling time; the
                                                  class map (resolved / shrinkage / both / growth / new) per voxel and per slice, and a Layer of it for render_planes
    track_series(masks, grids, transforms=)       -> LesionSeries: three or more time points on the baseline's grid, consecutive ones tracked, lineages over all of them

The device counts; the host matches (a table of at most a few MB).  The doubling time is the conventional formula interval ln 2 / ln(v_b / v_a), configurable through the
matching thresholds, and -- like the other tables of this package -- NOT clinically validated.  There is no CPU fallback for the device steps.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from . import volume as V

PAIR_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("voxels", np.int64)])
EVENTS = ("persistent", "merged", "split", "complex", "new", "resolved")
TRACK_DTYPE = np.dtype([("track", np.int32), ("event", "U10"), ("n_a", np.int32), ("n_b", np.int32), ("voxels_a", np.int64), ("voxels_b", np.int64), ("ml_a", np.float64),
                        ("ml_b", np.float64), ("overlap", np.int64), ("change_ml", np.float64), ("change_pct", np.float64), ("dice", np.float64),
                        ("xa", np.float64), ("ya", np.float64), ("za", np.float64), ("xb", np.float64), ("yb", np.float64), ("zb", np.float64), ("shift_mm", np.float64),
                        ("doubling_time_days", np.float64)])
CLS_NONE, CLS_RESOLVED, CLS_SHRINKAGE, CLS_BOTH, CLS_GROWTH, CLS_NEW = (_lib.TRACK_CLS_NONE, _lib.TRACK_CLS_RESOLVED, _lib.TRACK_CLS_SHRINKAGE, _lib.TRACK_CLS_BOTH,
                                                                       _lib.TRACK_CLS_GROWTH, _lib.TRACK_CLS_NEW)
CLASS_NAMES = ("none", "resolved", "shrinkage", "both", "growth", "new")          # by class value 0..5 (UNET_TRACK_CLS_*)
# the class map as a label volume of render_planes: label L > 0 takes palette[1 + (L - 1) % 5] = palette[L]
PALETTE_CHANGE = np.array([(0, 0, 0), (0, 130, 200), (70, 240, 240), (255, 225, 25), (245, 130, 48), (230, 25, 75)], np.uint8)
PAIRS_FIRST_CAPACITY = 1024


# ---- the contingency table ------------------------------------------------------------------------------------------------------------------------------------
def _check_count(n, what):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) < 2 ** 31:
        raise ValueError(f"{what} is an integer in 0 .. 2^31 - 1, not {n!r}")
    return int(n)


def _check_labels(labels, shape, what):
    """-> (the flat int32 labels in Fortran order -- the device tensor given, or a host array still to upload --, (X, Y, Z)); no device work"""
    torch = V._torch()
    if isinstance(labels, torch.Tensor):
        if shape is None:
            raise ValueError(f"{what}: device labels are a flat Fortran-order buffer: pass shape=(X, Y, Z)")
        shape = V.Grid(shape, np.eye(4)).shape
        if labels.dtype != torch.int32 or not labels.is_cuda or labels.numel() != int(np.prod(shape)):
            raise ValueError(f"{what}: device labels are an int32 cuda tensor of prod(shape) = {int(np.prod(shape))} elements")
        return labels.contiguous().reshape(-1), shape
    a = np.asarray(labels)
    if a.ndim != 3:
        raise ValueError(f"{what}: a volume is [X, Y, Z]; got {a.ndim} dimensions")
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: a label volume has an integer dtype, not {a.dtype}")
    if shape is not None and tuple(int(v) for v in shape) != a.shape:
        raise ValueError(f"{what}: shape= {tuple(shape)} is not the array's {a.shape}")
    return np.asfortranarray(a.astype(np.int32, copy=False)).reshape(-1, order="F"), tuple(int(v) for v in a.shape)


def first_capacity(n_a, n_b):
    """the slots label_pairs starts with: 4 (n_a + n_b + 2) rounded up to a power of two, at least 1024 (and at most the entry point's 2^30)"""
    want = max(4 * (int(n_a) + int(n_b) + 2), PAIRS_FIRST_CAPACITY)
    return min(1 << (want - 1).bit_length(), _lib.PAIRS_MAX_CAPACITY)


def label_pairs_device(la, n_a, lb, n_b, shape, capacity):
    """unet_vol_label_pairs -> (keys uint64 [capacity], counts int64 [capacity], info int64 [3]) as numpy: the table as the device left it, slots in no stated order"""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = shape
    V._check_volume_dims(shape)
    keys = torch.empty(capacity, dtype=torch.int64, device="cuda")
    counts = torch.empty(capacity, dtype=torch.int64, device="cuda")
    info = torch.empty(3, dtype=torch.int64, device="cuda")
    ctx.check(lib.unet_vol_label_pairs(ctx.handle, la.data_ptr(), int(n_a), lb.data_ptr(), int(n_b), X, Y, Z, keys.data_ptr(), counts.data_ptr(), int(capacity), info.data_ptr(),
                                       V._stream()), "vol_label_pairs")
    return keys.cpu().numpy().view(np.uint64), counts.cpu().numpy(), info.cpu().numpy()


def pairs_from_table(keys, counts):
    """an open-addressing table (key 0 = empty slot) -> PAIR_DTYPE records sorted by (a, b), which is the order of the keys"""
    keys = np.asarray(keys, np.uint64)
    used = np.flatnonzero(keys)
    order = used[np.argsort(keys[used], kind="stable")]
    out = np.zeros(len(order), PAIR_DTYPE)
    out["a"] = (keys[order] >> np.uint64(32)).astype(np.int64)
    out["b"] = (keys[order] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out["voxels"] = np.asarray(counts, np.int64)[order]
    return out


def label_pairs(labels_a, n_a, labels_b, n_b, shape=None):
    """The contingency table of two label volumes on one grid -> records (a, b, voxels) sorted by (a, b): the voxels with labels_a == a and labels_b == b, for every pair
    that occurs but (0, 0).  The rows (a, 0) and (0, b) are there, so the row and column sums are the lesion sizes.  labels_*: host integer arrays [X, Y, Z], or the flat
    int32 device tensors of label_volume(return_device=True) together with shape=; a label outside 0..n counts as 0.  The table on the device starts with
    first_capacity(n_a, n_b) slots and grows fourfold while the entry point reports voxels that found no slot; past 2^30 slots it is an error."""
    n_a, n_b = _check_count(n_a, "n_a"), _check_count(n_b, "n_b")
    la, sa = _check_labels(labels_a, shape, "labels_a")
    lb, sb = _check_labels(labels_b, shape, "labels_b")
    if sa != sb:
        raise ValueError(f"the two label volumes lie on one grid; got {sa} and {sb}")
    torch = V._torch()
    la, lb = (torch.from_numpy(l).cuda() if isinstance(l, np.ndarray) else l for l in (la, lb))
    capacity = first_capacity(n_a, n_b)
    while True:
        keys, counts, info = label_pairs_device(la, n_a, lb, n_b, sa, capacity)
        if info[1] == 0:
            return pairs_from_table(keys, counts)
        if capacity * 4 > _lib.PAIRS_MAX_CAPACITY:
            raise _lib.UNetHipError(f"label_pairs: {int(info[1])} voxels found no slot in a table of {capacity}, and the next one would pass 2^30 slots")
        capacity *= 4


# ---- the match --------------------------------------------------------------------------------------------------------------------------------------------------
class LesionMatch:
    """What match_lesions returns.  n_tracks; lut_a int32 [n_a + 1], lut_b int32 [n_b + 1]: label -> track, entry 0 = 0; per track t (index t - 1): members_a[t - 1],
    members_b[t - 1] (ascending int32 arrays of labels), voxels_a, voxels_b (int64: the sizes of its members), overlap (int64: the voxels of ALL pairs of its baseline
    members with its follow-up members, linked or not), events (a tuple of EVENTS names); size_a int64 [n_a + 1], size_b int64 [n_b + 1]: the lesion sizes (entry 0: the
    other side's voxels on this side's background); links: the records of `pairs` that were kept."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"LesionMatch({self.n_tracks} tracks: " + ", ".join(f"{self.events.count(e)} {e}" for e in EVENTS if e in self.events) + ")"


def event_of(na, nb):
    """the event of a track with na baseline and nb follow-up lesions"""
    if na == 0 or nb == 0:
        if na + nb == 0 or (na and nb):
            raise ValueError("a track holds at least one lesion")
        return "new" if na == 0 else "resolved"
    return ("persistent" if nb == 1 else "split") if na == 1 else ("merged" if nb == 1 else "complex")


def _check_match_args(min_overlap_voxels=1, min_fraction=0.0):
    if isinstance(min_overlap_voxels, bool) or not isinstance(min_overlap_voxels, (int, np.integer)) or int(min_overlap_voxels) < 1:
        raise ValueError(f"min_overlap_voxels is an integer >= 1, not {min_overlap_voxels!r}")
    if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float, np.integer, np.floating)) or not 0.0 <= float(min_fraction) <= 1.0:
        raise ValueError(f"min_fraction lies in 0 .. 1, not {min_fraction!r}")
    return int(min_overlap_voxels), float(min_fraction)


def _check_pairs(pairs, n_a, n_b):
    p = np.asarray(pairs)
    if p.dtype != PAIR_DTYPE or p.ndim != 1:
        raise ValueError("pairs is what label_pairs returns: a 1-d array of (a, b, voxels) records")
    if len(p) and (p["a"].min() < 0 or p["a"].max() > n_a or p["b"].min() < 0 or p["b"].max() > n_b or p["voxels"].min() < 0):
        raise ValueError(f"pairs holds a label outside 0 .. {n_a} / 0 .. {n_b}, or a negative count")
    return p


def match_lesions(pairs, n_a, n_b, min_overlap_voxels=1, min_fraction=0.0):
    """pairs (label_pairs) -> LesionMatch.  The size of a lesion is its row / column sum, the zero label included.  A link (a, b), a, b > 0, is kept when
    voxels >= min_overlap_voxels and voxels >= min_fraction * min(size_a, size_b) (compared in float64).  A track is a connected group of the kept links' bipartite graph;
    a lesion without a link is a group of its own.  Tracks are numbered from 1: the groups with a baseline lesion first, by their smallest a, then the groups of follow-up
    lesions only, by their smallest b.  The event follows from the numbers of lesions (|A|, |B|): (1, 1) persistent, (>1, 1) merged, (1, >1) split, (>1, >1) complex,
    (0, 1) new, (1, 0) resolved."""
    n_a, n_b = _check_count(n_a, "n_a"), _check_count(n_b, "n_b")
    min_overlap_voxels, min_fraction = _check_match_args(min_overlap_voxels, min_fraction)
    p = _check_pairs(pairs, n_a, n_b)
    size_a, size_b = np.zeros(n_a + 1, np.int64), np.zeros(n_b + 1, np.int64)
    np.add.at(size_a, p["a"], p["voxels"])
    np.add.at(size_b, p["b"], p["voxels"])
    both = p[(p["a"] > 0) & (p["b"] > 0)]
    smaller = np.minimum(size_a[both["a"]], size_b[both["b"]]).astype(np.float64)
    links = both[(both["voxels"] >= min_overlap_voxels) & (both["voxels"].astype(np.float64) >= min_fraction * smaller)]
    parent = np.arange(n_a + n_b, dtype=np.int64)                   # node a - 1 for a baseline lesion, n_a + b - 1 for a follow-up lesion

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in zip(links["a"].tolist(), links["b"].tolist()):
        ra, rb = find(a - 1), find(n_a + b - 1)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)                       # the root of a group is its smallest node: its smallest a, or without one its smallest b
    roots = np.array([find(i) for i in range(n_a + n_b)], np.int64)
    order = np.unique(roots)                                        # ascending roots = the stated numbering
    track_of_root = np.zeros(n_a + n_b + 1, np.int32)
    track_of_root[order] = np.arange(1, len(order) + 1)
    node_track = track_of_root[roots] if len(roots) else np.zeros(0, np.int32)
    lut_a, lut_b = np.zeros(n_a + 1, np.int32), np.zeros(n_b + 1, np.int32)
    lut_a[1:], lut_b[1:] = node_track[:n_a], node_track[n_a:]
    T = len(order)
    voxels_a, voxels_b, overlap = np.zeros(T + 1, np.int64), np.zeros(T + 1, np.int64), np.zeros(T + 1, np.int64)
    np.add.at(voxels_a, lut_a[1:], size_a[1:])
    np.add.at(voxels_b, lut_b[1:], size_b[1:])
    same = both[lut_a[both["a"]] == lut_b[both["b"]]]
    np.add.at(overlap, lut_a[same["a"]], same["voxels"])
    members_a = [np.flatnonzero(lut_a == t).astype(np.int32) for t in range(1, T + 1)]
    members_b = [np.flatnonzero(lut_b == t).astype(np.int32) for t in range(1, T + 1)]
    events = tuple(event_of(len(ma), len(mb)) for ma, mb in zip(members_a, members_b))
    return LesionMatch(n_tracks=T, n_a=n_a, n_b=n_b, lut_a=lut_a, lut_b=lut_b, members_a=members_a, members_b=members_b, voxels_a=voxels_a[1:], voxels_b=voxels_b[1:],
                       overlap=overlap[1:], events=events, size_a=size_a, size_b=size_b, links=links)


def class_tables(match):
    """-> (cls_a uint8 [n_a + 1], cls_b uint8 [n_b + 1]): the class of a voxel that only one side marks, by its lesion -- shrinkage / growth where the lesion's track has
    lesions on both sides, resolved / new where it has not.  Entry 0 is 0."""
    has_a = np.array([len(m) > 0 for m in match.members_a], bool)
    has_b = np.array([len(m) > 0 for m in match.members_b], bool)
    cls_a, cls_b = np.zeros(match.n_a + 1, np.uint8), np.zeros(match.n_b + 1, np.uint8)
    if match.n_a:
        cls_a[1:] = np.where(has_b[match.lut_a[1:] - 1], CLS_SHRINKAGE, CLS_RESOLVED)
    if match.n_b:
        cls_b[1:] = np.where(has_a[match.lut_b[1:] - 1], CLS_GROWTH, CLS_NEW)
    return cls_a, cls_b


# ---- the per-voxel maps -----------------------------------------------------------------------------------------------------------------------------------------
def track_map_device(la, n_a, lb, n_b, shape, lut_a, lut_b, cls_a, cls_b, want_cls=True, want_tracks=True, per_slice=True):
    """unet_vol_track_map -> (cls uint8, track_a int32, track_b int32: flat device tensors in Fortran order, or None where not asked for; per_slice int64 [Z, 6] numpy or
    None).  The four tables are host arrays of n + 1 entries."""
    torch = V._torch(); lib, ctx = V._ctx()
    X, Y, Z = shape
    V._check_volume_dims(shape)
    N = X * Y * Z
    tabs = [torch.from_numpy(np.ascontiguousarray(t, dt)).cuda() for t, dt in ((lut_a, np.int32), (lut_b, np.int32), (cls_a, np.uint8), (cls_b, np.uint8))]
    if tabs[0].numel() != n_a + 1 or tabs[2].numel() != n_a + 1 or tabs[1].numel() != n_b + 1 or tabs[3].numel() != n_b + 1:
        raise ValueError("the lookup and class tables have n + 1 entries")
    cls = torch.empty(N, dtype=torch.uint8, device="cuda") if want_cls else None
    ta = torch.empty(N, dtype=torch.int32, device="cuda") if want_tracks else None
    tb = torch.empty(N, dtype=torch.int32, device="cuda") if want_tracks else None
    ps = torch.zeros((max(Z, 1), 6), dtype=torch.int64, device="cuda") if per_slice else None
    ctx.check(lib.unet_vol_track_map(ctx.handle, la.data_ptr(), int(n_a), lb.data_ptr(), int(n_b), X, Y, Z, *(t.data_ptr() for t in tabs), V._ptr(cls), V._ptr(ta), V._ptr(tb),
                                     V._ptr(ps), V._stream()), "vol_track_map")
    return cls, ta, tb, (ps[:Z].cpu().numpy() if per_slice else None)


# ---- one follow-up -------------------------------------------------------------------------------------------------------------------------------------------------
class LesionTracking:
    """What track_lesions returns, everything on the baseline's grid (`grid`).
    tracks: TRACK_DTYPE records, one per track -- track, event, n_a / n_b (lesions on each side), voxels_a / voxels_b, ml_a / ml_b (at the grid's voxel volume), overlap,
      change_ml = (voxels_b - voxels_a) voxel_ml, change_pct = 100 (vb - va) / va (NaN for a new lesion), dice = 2 overlap / (va + vb), (xa, ya, za) / (xb, yb, zb): the
      voxel-weighted centroid of each side in world millimetres (NaN on a side without voxels), shift_mm between them (NaN for new / resolved), doubling_time_days =
      interval_days ln 2 / ln(vb / va) for a track with voxels on both sides and vb != va, NaN otherwise and without interval_days; a negative value is a halving time.
      The conventional formula; not clinically validated.
    labels_a / labels_b: per track the labels of its lesions (label_volume's numbering on this grid); match: the LesionMatch; pairs: label_pairs' table; n_a, n_b.
    persistent / new / resolved (+ _ml): the voxels in both masks, in b only, in a only -- change_between's totals; events: {event: {"count", "ml_a", "ml_b"}}.
    per_slice: int64 [Z, 6], the voxels of every class 0..5 (CLASS_NAMES) per axial slice.  class_map (uint8), track_a, track_b (int32): [X, Y, Z] host arrays in
    Fortran order, or with return_device=True the flat device tensors.  b_on_a: the follow-up's mask on this grid, as change_between returned it.  interval_days."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def layer(self, fill_alpha=128, outline_alpha=255):
        """the class map as an overlay of render_planes (pass shape= there when the maps are device tensors): resolved, shrinkage, both, growth, new in PALETTE_CHANGE"""
        return V.Layer(self.class_map, PALETTE_CHANGE, fill_alpha, outline_alpha)

    def __repr__(self):
        return (f"LesionTracking({len(self.tracks)} tracks: " + ", ".join(f"{v['count']} {e}" for e, v in self.events.items() if v["count"]) +
                f"; persistent_ml={self.persistent_ml:.2f}, new_ml={self.new_ml:.2f}, resolved_ml={self.resolved_ml:.2f})")


def _check_interval(interval_days):
    if interval_days is None:
        return None
    if isinstance(interval_days, bool) or not isinstance(interval_days, (int, float, np.integer, np.floating)) or not math.isfinite(interval_days) or interval_days <= 0:
        raise ValueError(f"interval_days is a positive number of days, not {interval_days!r}")
    return float(interval_days)


def world_centroid(affine, sx, sy, sz, count):
    """integer coordinate sums / the voxel count, then the affine: ((m0 cx + m1 cy) + m2 cz) + m3 per row, in float64; NaN without voxels"""
    if count == 0:
        return (float("nan"),) * 3
    m = np.asarray(affine, np.float64)
    cx, cy, cz = np.float64(sx) / np.float64(count), np.float64(sy) / np.float64(count), np.float64(sz) / np.float64(count)
    return tuple(float(((m[r, 0] * cx + m[r, 1] * cy) + m[r, 2] * cz) + m[r, 3]) for r in range(3))


def track_table(match, stats_a, stats_b, grid, interval_days=None):
    """LesionMatch + the component statistics of both sides (records with voxels, sx, sy, sz per label, label 1 first) -> TRACK_DTYPE records.  Pure numpy."""
    interval_days = _check_interval(interval_days)
    ml = grid.voxel_ml
    t = np.zeros(match.n_tracks, TRACK_DTYPE)
    nan = float("nan")
    for i in range(match.n_tracks):
        ma, mb = match.members_a[i], match.members_b[i]
        va, vb, ov = int(match.voxels_a[i]), int(match.voxels_b[i]), int(match.overlap[i])
        ca = world_centroid(grid.affine, *(int(stats_a[k][ma - 1].sum()) for k in ("sx", "sy", "sz")), va)
        cb = world_centroid(grid.affine, *(int(stats_b[k][mb - 1].sum()) for k in ("sx", "sy", "sz")), vb)
        d = [cb[k] - ca[k] for k in range(3)]
        dbl = nan
        if interval_days is not None and va > 0 and vb > 0 and va != vb:
            dbl = float(interval_days * np.log(2.0) / np.log(np.float64(vb) / np.float64(va)))
        t[i] = (i + 1, match.events[i], len(ma), len(mb), va, vb, va * ml, vb * ml, ov, (vb - va) * ml, (100.0 * (vb - va) / va) if va else nan, (2.0 * ov / (va + vb)) if va + vb else nan,
                ca[0], ca[1], ca[2], cb[0], cb[1], cb[2], float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])), dbl)
    return t


def event_summary(tracks):
    return {e: {"count": int((tracks["event"] == e).sum()), "ml_a": float(tracks["ml_a"][tracks["event"] == e].sum()), "ml_b": float(tracks["ml_b"][tracks["event"] == e].sum())}
            for e in EVENTS}


def _track_on_grid(dev_a, dev_b, grid, connectivity, min_overlap_voxels, min_fraction, interval_days, want_maps=True):
    """two uint8 device masks on one grid -> (n_a, n_b, stats_a, stats_b, pairs, match, tracks, maps): steps 2 .. 6 of track_lesions"""
    shape = grid.shape
    la, n_a = V.label_device(dev_a, shape, connectivity)
    lb, n_b = V.label_device(dev_b, shape, connectivity)
    stats_a, stats_b = V.component_stats_device(la, shape, n_a), V.component_stats_device(lb, shape, n_b)
    pairs = label_pairs(la, n_a, lb, n_b, shape)
    match = match_lesions(pairs, n_a, n_b, min_overlap_voxels, min_fraction)
    tracks = track_table(match, stats_a, stats_b, grid, interval_days)
    cls_a, cls_b = class_tables(match)
    maps = track_map_device(la, n_a, lb, n_b, shape, match.lut_a, match.lut_b, cls_a, cls_b, want_cls=want_maps, want_tracks=want_maps)
    return n_a, n_b, stats_a, stats_b, pairs, match, tracks, maps


def _check_track_args(connectivity=1, min_overlap_voxels=1, min_fraction=0.0, interval_days=None):
    V._check_connectivity(connectivity)
    _check_match_args(min_overlap_voxels, min_fraction)
    _check_interval(interval_days)


def track_lesions(mask_a, grid_a, mask_b, grid_b, transform=None, connectivity=1, min_overlap_voxels=1, min_fraction=0.0, interval_days=None, return_device=False):
    """A baseline mask a and a follow-up mask b of one patient -> LesionTracking on a's grid: which lesion grew by how much, which merged, which is new.
    mask_*, grid_*, transform: as change_between takes them (host arrays or uint8 device tensors; oriented Grids; None, a 4 x 4 matrix, a RigidTransform, a Registration
    or a DeformableRegistration) -- b is put onto a's grid BY change_between, so there is one definition of "onto the baseline".  Both masks are then labelled there
    (connectivity: label_volume's), their contingency table is counted (label_pairs), the lesions are matched (match_lesions: min_overlap_voxels, min_fraction) and the
    class and track maps are drawn (unet_vol_track_map).  interval_days: the days between the scans, for doubling_time_days = interval ln 2 / ln(vb / va) -- the
    conventional formula, not clinically validated.  An unoriented grid is refused as change_between refuses it: left and right are never guessed."""
    ga, gb = V._need_oriented(grid_a, "grid_a"), V._need_oriented(grid_b, "grid_b")
    _check_track_args(connectivity, min_overlap_voxels, min_fraction, interval_days)
    torch = V._torch()
    src = V._resample_source(mask_a, None, ga.affine, ga.shape if isinstance(mask_a, torch.Tensor) else None, "mask")
    if src.shape != ga.shape:
        raise ValueError(f"mask_a is {src.shape}, its grid {ga.shape}")
    dev_a = src.tensor if src.tensor is not None else V.upload(src.vol)
    change = V.change_between(dev_a, ga, mask_b, gb, return_device=True, transform=transform)
    n_a, n_b, _, _, pairs, match, tracks, (cls, ta, tb, per_slice) = _track_on_grid(dev_a, change.b_on_a, ga, connectivity, min_overlap_voxels, min_fraction, interval_days)
    totals = per_slice.sum(axis=0)
    persistent, new, resolved = int(totals[CLS_BOTH]), int(totals[CLS_GROWTH] + totals[CLS_NEW]), int(totals[CLS_RESOLVED] + totals[CLS_SHRINKAGE])
    if (persistent, new, resolved) != (change.persistent, change.new, change.resolved):
        raise _lib.UNetHipError(f"track_lesions: the class map counts {(persistent, new, resolved)} persistent / new / resolved voxels, change_between {(change.persistent, change.new, change.resolved)}")
    ml = ga.voxel_ml
    host = (lambda t, dt: t) if return_device else (lambda t, dt: V._host_of(t, dt, ga.shape))
    return LesionTracking(tracks=tracks, labels_a=match.members_a, labels_b=match.members_b, match=match, pairs=pairs, n_a=n_a, n_b=n_b, persistent=persistent, new=new,
                          resolved=resolved, persistent_ml=persistent * ml, new_ml=new * ml, resolved_ml=resolved * ml, dice=change.dice, events=event_summary(tracks),
                          per_slice=per_slice, class_map=host(cls, np.uint8), track_a=host(ta, np.int32), track_b=host(tb, np.int32),
                          b_on_a=change.b_on_a if return_device else V._host_of(change.b_on_a, np.uint8, ga.shape), grid=ga, matrix=change.matrix, interval_days=interval_days)


# ---- three or more time points ---------------------------------------------------------------------------------------------------------------------------------------
class LesionSeries:
    """What track_series returns.  n_lineages L, n_times T; ml float64 [L, T] and voxels int64 [L, T]: every lineage at every time point, on the baseline's grid; first,
    last: int [L], the first and last time point a lineage has voxels at; events: [L][T - 1] names -- the event of the step t -> t + 1's track that holds the lineage's
    lesions ("" where it has none there, "mixed" where several tracks with different events do); lineage_of: per time point int32 [n_t + 1], label -> lineage (entry 0 =
    0); counts: lesions per time point; steps: the LesionMatch of every step; grid: the baseline's."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return f"LesionSeries({self.n_lineages} lineages over {self.n_times} time points)"


def chain_series(matches, sizes):
    """Host logic of track_series.  matches: the LesionMatch of every step t -> t + 1; sizes: per time point int64 [n_t + 1], the voxels of every label (entry 0 unused).
    Lineages are the connected groups over all (t, label) nodes, two nodes joined when a step puts them into one track; they are numbered from 1 by their earliest time
    point, then by their smallest label there.  -> (lineage_of: per time point int32 [n_t + 1]; voxels int64 [L, T]; first, last int [L]; events [L][T - 1])."""
    T = len(sizes)
    if T < 2 or len(matches) != T - 1:
        raise ValueError("a series has T >= 2 time points and T - 1 steps")
    counts = [len(s) - 1 for s in sizes]
    for s, m in enumerate(matches):
        if (m.n_a, m.n_b) != (counts[s], counts[s + 1]):
            raise ValueError(f"step {s} matches {m.n_a} and {m.n_b} lesions, the time points hold {counts[s]} and {counts[s + 1]}")
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)          # node of (t, label) = base[t] + label - 1: ascending in (t, label)
    parent = np.arange(base[-1], dtype=np.int64)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for s, m in enumerate(matches):
        for ma, mb in zip(m.members_a, m.members_b):
            nodes = [base[s] + a - 1 for a in ma.tolist()] + [base[s + 1] + b - 1 for b in mb.tolist()]
            for v in nodes[1:]:
                r0, r1 = find(nodes[0]), find(v)
                if r0 != r1:
                    parent[max(r0, r1)] = min(r0, r1)                 # the root is the smallest node: the earliest time point, the smallest label there
    roots = np.array([find(i) for i in range(base[-1])], np.int64)
    order = np.unique(roots)
    lin = np.zeros(int(base[-1]) + 1, np.int32)
    lin[order] = np.arange(1, len(order) + 1)
    L = len(order)
    lineage_of, voxels = [], np.zeros((L + 1, T), np.int64)
    for t in range(T):
        lut = np.zeros(counts[t] + 1, np.int32)
        lut[1:] = lin[roots[base[t]:base[t + 1]]]
        lineage_of.append(lut)
        np.add.at(voxels[:, t], lut[1:], np.asarray(sizes[t], np.int64)[1:])
    voxels = voxels[1:]
    seen = voxels > 0
    first = np.where(seen.any(axis=1), seen.argmax(axis=1), -1)
    last = np.where(seen.any(axis=1), T - 1 - seen[:, ::-1].argmax(axis=1), -1)
    events = [[""] * (T - 1) for _ in range(L)]
    for s, m in enumerate(matches):
        for i in range(m.n_tracks):
            l = int(lineage_of[s][m.members_a[i][0]] if len(m.members_a[i]) else lineage_of[s + 1][m.members_b[i][0]]) - 1
            events[l][s] = m.events[i] if events[l][s] in ("", m.events[i]) else "mixed"
    return lineage_of, voxels, first, last, events


def track_series(masks, grids, transforms=None, connectivity=1, min_overlap_voxels=1, min_fraction=0.0):
    """Three or more time points -> LesionSeries.  masks[t], grids[t]: as track_lesions takes them; transforms[t] relates the baseline (time point 0) to time point t as
    change_between(transform=) takes it (transforms[0] is not read; None: the affines as they are).  Every mask is put on the baseline's grid by change_between,
    consecutive time points are tracked there (label_volume, label_pairs, match_lesions), and the lineages are chain_series' groups."""
    masks, grids = list(masks), list(grids)
    T = len(masks)
    if T < 3 or len(grids) != T:
        raise ValueError(f"a series has three or more time points and one grid per mask; got {T} masks and {len(grids)} grids")
    transforms = [None] * T if transforms is None else list(transforms)
    if len(transforms) != T:
        raise ValueError(f"transforms has one entry per time point ({T}), not {len(transforms)}")
    for t, g in enumerate(grids):
        V._need_oriented(g, f"grids[{t}]")
    _check_track_args(connectivity, min_overlap_voxels, min_fraction)
    torch = V._torch()
    g0 = grids[0]
    src = V._resample_source(masks[0], None, g0.affine, g0.shape if isinstance(masks[0], torch.Tensor) else None, "mask")
    if src.shape != g0.shape:
        raise ValueError(f"masks[0] is {src.shape}, its grid {g0.shape}")
    dev = [src.tensor if src.tensor is not None else V.upload(src.vol)]
    for t in range(1, T):
        dev.append(V.change_between(dev[0], g0, masks[t], grids[t], return_device=True, transform=transforms[t]).b_on_a)
    matches, sizes = [], []
    for t in range(T - 1):
        n_a, n_b, stats_a, stats_b, _, match, _, _ = _track_on_grid(dev[t], dev[t + 1], g0, connectivity, min_overlap_voxels, min_fraction, None, want_maps=False)
        matches.append(match)
        sizes.append(np.concatenate([[0], stats_a["voxels"]]).astype(np.int64))
        if t == T - 2:
            sizes.append(np.concatenate([[0], stats_b["voxels"]]).astype(np.int64))
    lineage_of, voxels, first, last, events = chain_series(matches, sizes)
    return LesionSeries(n_lineages=len(voxels), n_times=T, voxels=voxels, ml=voxels * g0.voxel_ml, first=first, last=last, events=events, lineage_of=lineage_of,
                        counts=[len(s) - 1 for s in sizes], steps=matches, grid=g0)

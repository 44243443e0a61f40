"""numpy restatement of csrc/kernels_track.hip and tracking.py: the contingency table by np.unique over packed keys, the match by a
label-propagation union of its own, the class / track maps, the per-track table by its stated formulas, and the chaining of a series.  Nothing here imports the package."""
import numpy as np

PAIR_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("voxels", np.int64)])
CLS_RESOLVED, CLS_SHRINKAGE, CLS_BOTH, CLS_GROWTH, CLS_NEW = 1, 2, 3, 4, 5


def clamp(labels, n):
    """a label outside 0..n counts as 0"""
    l = np.asarray(labels).astype(np.int64)
    return np.where((l < 0) | (l > n), 0, l)


def packed_keys(la, n_a, lb, n_b):
    return (clamp(la, n_a).astype(np.uint64) << np.uint64(32)) | clamp(lb, n_b).astype(np.uint64)


def pair_table(la, n_a, lb, n_b):
    """-> (keys uint64 ascending, counts int64): every pair but (0, 0)"""
    keys, counts = np.unique(packed_keys(la, n_a, lb, n_b).reshape(-1), return_counts=True)
    keep = keys != 0
    return keys[keep], counts[keep].astype(np.int64)


def pairs(la, n_a, lb, n_b):
    keys, counts = pair_table(la, n_a, lb, n_b)
    out = np.zeros(len(keys), PAIR_DTYPE)
    out["a"], out["b"], out["voxels"] = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), counts
    return out


def dense_table(la, n_a, lb, n_b):
    """the full (n_a + 1) x (n_b + 1) contingency table by np.add.at (small n only)"""
    t = np.zeros((n_a + 1, n_b + 1), np.int64)
    np.add.at(t, (clamp(la, n_a).reshape(-1), clamp(lb, n_b).reshape(-1)), 1)
    return t


def event_of(na, nb):
    return {(1, 1): "persistent", (2, 1): "merged", (1, 2): "split", (2, 2): "complex", (0, 1): "new", (1, 0): "resolved"}[(min(na, 2), min(nb, 2))]


def match(p, n_a, n_b, min_overlap_voxels=1, min_fraction=0.0):
    """-> dict(lut_a, lut_b, members_a, members_b, voxels_a, voxels_b, overlap, events, size_a, size_b).  Groups by propagating the smallest node number along the kept
    links until nothing changes; node a - 1 for a baseline lesion, n_a + b - 1 for a follow-up lesion, so a group's number is its smallest a, or its smallest b."""
    size_a, size_b = np.zeros(n_a + 1, np.int64), np.zeros(n_b + 1, np.int64)
    for a, b, v in p.tolist():
        size_a[a] += v
        size_b[b] += v
    links = [(a, b) for a, b, v in p.tolist() if a > 0 and b > 0 and v >= min_overlap_voxels and np.float64(v) >= np.float64(min_fraction) * np.float64(min(size_a[a], size_b[b]))]
    group = list(range(n_a + n_b))
    changed = True
    while changed:
        changed = False
        for a, b in links:
            i, j = a - 1, n_a + b - 1
            g = min(group[i], group[j])
            if group[i] != g or group[j] != g:
                group[i] = group[j] = g
                changed = True
    numbers = {g: k + 1 for k, g in enumerate(sorted(set(group)))}
    lut_a = np.array([0] + [numbers[group[a - 1]] for a in range(1, n_a + 1)], np.int32)
    lut_b = np.array([0] + [numbers[group[n_a + b - 1]] for b in range(1, n_b + 1)], np.int32)
    T = len(numbers)
    members_a = [[a for a in range(1, n_a + 1) if lut_a[a] == t] for t in range(1, T + 1)]
    members_b = [[b for b in range(1, n_b + 1) if lut_b[b] == t] for t in range(1, T + 1)]
    table = {(a, b): v for a, b, v in p.tolist()}
    return dict(lut_a=lut_a, lut_b=lut_b, members_a=members_a, members_b=members_b, size_a=size_a, size_b=size_b,
                voxels_a=np.array([sum(size_a[a] for a in m) for m in members_a], np.int64), voxels_b=np.array([sum(size_b[b] for b in m) for m in members_b], np.int64),
                overlap=np.array([sum(table.get((a, b), 0) for a in ma for b in mb) for ma, mb in zip(members_a, members_b)], np.int64),
                events=tuple(event_of(len(ma), len(mb)) for ma, mb in zip(members_a, members_b)))


def class_tables(m):
    cls_a = np.array([0] + [CLS_SHRINKAGE if m["members_b"][t - 1] else CLS_RESOLVED for t in m["lut_a"][1:]], np.uint8)
    cls_b = np.array([0] + [CLS_GROWTH if m["members_a"][t - 1] else CLS_NEW for t in m["lut_b"][1:]], np.uint8)
    return cls_a, cls_b


def track_map(la, n_a, lb, n_b, lut_a, lut_b, cls_a, cls_b):
    """-> (cls uint8, track_a int32, track_b int32, per_slice int64 [Z, 6]); entry 0 of every table reads as 0"""
    a, b = clamp(la, n_a), clamp(lb, n_b)
    lut_a, lut_b, cls_a, cls_b = (np.concatenate([[0], np.asarray(t)[1:]]) for t in (lut_a, lut_b, cls_a, cls_b))
    cls = np.where((a > 0) & (b > 0), CLS_BOTH, np.where(a > 0, cls_a[a], np.where(b > 0, cls_b[b], 0))).astype(np.uint8)
    per_slice = np.stack([(cls == c).sum(axis=(0, 1)) for c in range(6)], axis=1).astype(np.int64)
    return cls, lut_a[a].astype(np.int32), lut_b[b].astype(np.int32), per_slice


def coordinate_sums(labels, members):
    """-> (sx, sy, sz, count) of the voxels whose label is in members, as Python integers"""
    x, y, z = np.nonzero(np.isin(labels, members)) if len(members) else ((), (), ())
    return int(np.sum(x, dtype=np.int64)), int(np.sum(y, dtype=np.int64)), int(np.sum(z, dtype=np.int64)), len(x)


def centroid(affine, sx, sy, sz, count):
    """integer sums / count, then ((m0 cx + m1 cy) + m2 cz) + m3 per row of the affine"""
    if count == 0:
        return (np.nan,) * 3
    m = np.asarray(affine, np.float64)
    c = [np.float64(s) / np.float64(count) for s in (sx, sy, sz)]
    return tuple(((m[r, 0] * c[0] + m[r, 1] * c[1]) + m[r, 2] * c[2]) + m[r, 3] for r in range(3))


def formulas(va, vb, overlap, voxel_ml, interval_days=None):
    """-> dict(ml_a, ml_b, change_ml, change_pct, dice, doubling_time_days) by the stated formulas"""
    va, vb = int(va), int(vb)
    dbl = np.nan
    if interval_days is not None and va > 0 and vb > 0 and va != vb:
        dbl = np.float64(interval_days) * np.log(2.0) / np.log(np.float64(vb) / np.float64(va))
    return dict(ml_a=va * voxel_ml, ml_b=vb * voxel_ml, change_ml=(vb - va) * voxel_ml, change_pct=100.0 * (vb - va) / va if va else np.nan, dice=2.0 * int(overlap) / (va + vb),
                doubling_time_days=dbl)


def track(la, n_a, lb, n_b, affine, min_overlap_voxels=1, min_fraction=0.0, interval_days=None):
    """two label volumes on one grid -> dict(pairs, match, rows: one dict per track, cls, track_a, track_b, per_slice, persistent, new, resolved)"""
    p = pairs(la, n_a, lb, n_b)
    m = match(p, n_a, n_b, min_overlap_voxels, min_fraction)
    voxel_ml = abs(float(np.linalg.det(np.asarray(affine, np.float64)[:3, :3]))) / 1000.0
    rows = []
    for t in range(len(m["events"])):
        va, vb = m["voxels_a"][t], m["voxels_b"][t]
        ca = centroid(affine, *coordinate_sums(la, m["members_a"][t]))
        cb = centroid(affine, *coordinate_sums(lb, m["members_b"][t]))
        d = [cb[k] - ca[k] for k in range(3)]
        row = dict(track=t + 1, event=m["events"][t], n_a=len(m["members_a"][t]), n_b=len(m["members_b"][t]), voxels_a=va, voxels_b=vb, overlap=m["overlap"][t],
                   xa=ca[0], ya=ca[1], za=ca[2], xb=cb[0], yb=cb[1], zb=cb[2], shift_mm=np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        row.update(formulas(va, vb, m["overlap"][t], voxel_ml, interval_days))
        rows.append(row)
    cls, ta, tb, per_slice = track_map(la, n_a, lb, n_b, m["lut_a"], m["lut_b"], *class_tables(m))
    tot = per_slice.sum(axis=0)
    return dict(pairs=p, match=m, rows=rows, cls=cls, track_a=ta, track_b=tb, per_slice=per_slice, persistent=int(tot[3]), new=int(tot[4] + tot[5]), resolved=int(tot[1] + tot[2]))


def chain(matches, sizes):
    """matches: match() of every step; sizes: per time point the voxels per label (entry 0 unused) -> (lineage_of per time point, voxels [L, T], first, last, events).
    Lineages by propagating the smallest (t, label) over the tracks of every step until nothing changes; numbered by earliest time point, then smallest label there."""
    T = len(sizes)
    nodes = [(t, l) for t in range(T) for l in range(1, len(sizes[t]))]
    group = {nd: nd for nd in nodes}
    changed = True
    while changed:
        changed = False
        for s, m in enumerate(matches):
            for ma, mb in zip(m["members_a"], m["members_b"]):
                mem = [(s, a) for a in ma] + [(s + 1, b) for b in mb]
                g = min(group[nd] for nd in mem)
                for nd in mem:
                    if group[nd] != g:
                        group[nd] = g
                        changed = True
    number = {g: k + 1 for k, g in enumerate(sorted(set(group.values())))}
    L = len(number)
    lineage_of = [np.array([0] + [number[group[(t, l)]] for l in range(1, len(sizes[t]))], np.int32) for t in range(T)]
    voxels = np.zeros((L, T), np.int64)
    for (t, l) in nodes:
        voxels[number[group[(t, l)]] - 1, t] += sizes[t][l]
    first = np.array([min(t for t in range(T) if voxels[k, t] > 0) if voxels[k].any() else -1 for k in range(L)])
    last = np.array([max(t for t in range(T) if voxels[k, t] > 0) if voxels[k].any() else -1 for k in range(L)])
    events = [[""] * (T - 1) for _ in range(L)]
    for s, m in enumerate(matches):
        for ma, mb, ev in zip(m["members_a"], m["members_b"], m["events"]):
            k = number[group[(s, ma[0]) if ma else (s + 1, mb[0])]] - 1
            events[k][s] = ev if events[k][s] in ("", ev) else "mixed"
    return lineage_of, voxels, first, last, events


# ---- the scripted scene ---------------------------------------------------------------------------------------------------------------------------------------------
def _ball(shape, centre, radius):
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius * radius


def scene(shape=(48, 40, 24)):
    """-> (mask_a, mask_b) uint8 in Fortran order: a stable ball, a grown ball, two balls that merge, one that splits, a chain that makes a complex group, one resolved and
    one new lesion.  Lesions are separated by at least two voxels, so connectivity 1 labels them as drawn."""
    a, b = np.zeros(shape, bool), np.zeros(shape, bool)
    for m in (a, b):
        m |= _ball(shape, (6, 6, 5), 3)                             # stable
    a |= _ball(shape, (18, 6, 5), 2); b |= _ball(shape, (18, 6, 5), 4)          # grown
    a |= _ball(shape, (30, 6, 5), 2); a |= _ball(shape, (37, 6, 5), 2)          # two balls ...
    b[28:40, 5:8, 4:7] = True                                       # ... that merge into one bar
    a[4:16, 16:19, 4:7] = True                                      # one bar ...
    b |= _ball(shape, (6, 17, 5), 2); b |= _ball(shape, (13, 17, 5), 2)         # ... that splits
    a[22:28, 16:19, 4:7] = True; a[31:37, 16:19, 4:7] = True        # a chain a1 - b1 - a2 - b2: complex
    b[26:33, 16:19, 4:7] = True; b[35:42, 16:19, 4:7] = True
    a |= _ball(shape, (8, 30, 16), 3)                               # resolved
    b |= _ball(shape, (30, 30, 16), 3)                              # new
    return np.asfortranarray(a.astype(np.uint8)), np.asfortranarray(b.astype(np.uint8))


def label(mask, connectivity=1):
    """scipy.ndimage.label with generate_binary_structure(3, connectivity): components numbered by their first voxel in C order, as label_volume numbers them"""
    from scipy import ndimage
    lab, n = ndimage.label(np.ascontiguousarray(mask) != 0, ndimage.generate_binary_structure(3, connectivity))
    return np.asfortranarray(lab.astype(np.int32)), int(n)

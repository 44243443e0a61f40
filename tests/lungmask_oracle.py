"""CPU restatement of the lung mask found from the CT itself (csrc/kernels_lungmask.hip, covidseg_amd.lungs) in numpy only, on the other oracles: components_oracle
(labelling, component tables), morph_oracle (structures, per-slice labelling, hole filling, the ball).  tests/test_lungmask_host.py pins it against scipy.ndimage where
that imports.

  threshold        lo <= v < hi on the decoded values (and a region), the set voxels per slice                                     unet_vol_threshold
  geodesic         a literal breadth-first loop: step s reaches the unreached constraint voxels with a neighbour reached at s - 1     unet_vol_geodesic_begin / _steps
  reconstruct      the components of a mask that hold a marker voxel
  leak_rule        the front-count criterion of the airway growth, on the host in the product as well
  body_mask / find_trachea / grow_airways / lung_mask: the procedure of lungs.lung_mask, step for step
  phantom          the chest the tests run it on
"""
import numpy as np

import components_oracle as CO
import morph_oracle as MO

UNREACHED = 0xFFFF
MAX_STEP = 65534


# ---- the two kernels ------------------------------------------------------------------------------------------------------------------------------------------------
def decode(raw, slope=None, inter=None):
    """get_fdata: float64(raw), then (v * slope) + inter as two rounded operations when scaled (slope given)"""
    v = np.asarray(raw).astype(np.float64)
    return v if slope is None else (v * np.float64(slope)) + np.float64(inter)


def threshold(values, lo=None, hi=None, region=None):
    """-> (mask uint8 [X, Y, Z], slice_counts int64 [Z]): lo <= v < hi, None = unbounded; a NaN gives 0"""
    lo = -np.inf if lo is None else float(lo)
    hi = np.inf if hi is None else float(hi)
    if np.isnan(lo) or np.isnan(hi) or not lo < hi:
        raise ValueError("lo < hi, neither NaN")
    v = np.asarray(values, np.float64)
    with np.errstate(invalid="ignore"):
        m = (lo <= v) & (v < hi)
    if region is not None:
        m &= np.asarray(region) != 0
    return m.astype(np.uint8), m.sum(axis=(0, 1)).astype(np.int64)


def geodesic(seeds, constraint, connectivity=1, planar=False, max_steps=None):
    """-> (arrival uint16 [X, Y, Z], counts int64 [steps reached + 1]).  arrival: 0 on seeds & constraint, s where step s arrived, 0xFFFF elsewhere; counts[s]: the
    voxels reached at step s.  The loop ends at the first step that reaches nothing, or after max_steps steps."""
    c = np.asarray(constraint) != 0
    reached = (np.asarray(seeds) != 0) & c
    arrival = np.full(c.shape, UNREACHED, np.uint16)
    arrival[reached] = 0
    counts = [int(reached.sum())]
    offs = MO.offsets(connectivity, planar)
    limit = MAX_STEP if max_steps is None else min(int(max_steps), MAX_STEP)
    front, s = reached.copy(), 0
    while counts[0] > 0 and s < limit:
        new = MO.step(front, offs, 0, True) & c & ~reached
        n = int(new.sum())
        if n == 0:
            break
        s += 1
        arrival[new] = s
        reached |= new
        front = new
        counts.append(n)
    return arrival, np.array(counts, np.int64)


def reconstruct(mask, marker, connectivity=1):
    """the components of mask != 0 that hold a voxel of marker != 0, as uint8 0 / 1"""
    lab, n = CO.label(mask, connectivity)
    keep = np.zeros(n + 1, bool)
    keep[np.unique(lab[np.asarray(marker) != 0])] = True
    keep[0] = False
    return keep[lab].astype(np.uint8)


# ---- the leak rule --------------------------------------------------------------------------------------------------------------------------------------------------
def leak_rule(counts, leak_ratio=3.0, min_front=8, ref_steps=4):
    """counts[s]: the front of step s -> (leak_step or None, stop_step).  m = min(counts[:ref_steps]); the first s >= ref_steps with counts[s] > leak_ratio max(m, min_front)
    is the leak; m takes counts[s] in after each test.  stop_step: the last step before the leak whose count equals the running minimum at that point; without a leak the
    last step."""
    c = [int(v) for v in counts]
    if not c:
        raise ValueError("no counts")
    head = c[:ref_steps]
    m = min(head)
    stop = max(i for i, v in enumerate(head) if v == m)
    for s in range(ref_steps, len(c)):
        if float(c[s]) > float(leak_ratio) * float(max(m, min_front)):
            return s, stop
        if c[s] <= m:
            m, stop = c[s], s
    return None, len(c) - 1


# ---- the procedure --------------------------------------------------------------------------------------------------------------------------------------------------
def largest_component(mask, connectivity=1):
    lab, n = CO.label(mask, connectivity)
    if n == 0:
        return np.zeros(lab.shape, np.uint8)
    vox = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
    return (lab == CO.largest(vox, 1)[0]).astype(np.uint8)


def body_mask(values, body_hu=-500.0):
    """the component of most voxels (connectivity 1, ties to the lower label) of v >= body_hu, its holes filled slice by slice (connectivity 1)"""
    return MO.fill_holes(largest_component(threshold(values, lo=body_hu)[0], 1), 1, planar=True)


def find_trachea(air_in_body, pixdim, superior, area_mm2=(50.0, 1200.0), max_extent_mm=35.0, seed_slices=3, seed_shift_mm=10.0):
    """-> None or dict(label, z, cx, cy, voxels, mask uint8).  The per-slice components (connectivity 1) whose area lies in area_mm2 and whose in-plane bounding-box
    extents are both <= max_extent_mm are candidates.  Walking from the superior end ("z+": z = Z - 1 downwards, "z-": z = 0 upwards), slice by slice and candidate by
    candidate in label order: a candidate is the seed when a chain continues it through the next seed_slices - 1 slices, each link the lowest-labelled candidate of the
    next slice whose centroid lies within seed_shift_mm (in the plane, millimetres) of the current link's centroid."""
    px, py = float(pixdim[0]), float(pixdim[1])
    lab, n = MO.label_planar(air_in_body, 1)
    if n == 0:
        return None
    st = CO.stats(lab, n)
    Z = lab.shape[2]
    area = st["voxels"].astype(np.float64) * (px * py)
    ok = (area >= float(area_mm2[0])) & (area <= float(area_mm2[1]))
    ok &= ((st["x1"] - st["x0"] + 1).astype(np.float64) * px <= float(max_extent_mm)) & ((st["y1"] - st["y0"] + 1).astype(np.float64) * py <= float(max_extent_mm))
    cx, cy = st["sx"].astype(np.float64) / st["voxels"], st["sy"].astype(np.float64) / st["voxels"]
    by_slice = {}
    for i in np.flatnonzero(ok):
        by_slice.setdefault(int(st["z0"][i]), []).append(int(i))
    step = -1 if superior == "z+" else 1
    r2 = float(seed_shift_mm) * float(seed_shift_mm)
    for z in (range(Z - 1, -1, -1) if superior == "z+" else range(Z)):
        for i in by_slice.get(z, []):
            cur, good = i, True
            for k in range(1, int(seed_slices)):
                nxt = [j for j in by_slice.get(z + step * k, []) if ((cx[j] - cx[cur]) * px) ** 2 + ((cy[j] - cy[cur]) * py) ** 2 <= r2]
                if not nxt:
                    good = False
                    break
                cur = nxt[0]
            if good:
                return dict(label=i + 1, z=z, cx=float(cx[i]), cy=float(cy[i]), voxels=int(st["voxels"][i]), mask=(lab == i + 1).astype(np.uint8))
    return None


def grow_airways(values, seed, within, airway_hu=-950.0, leak_ratio=3.0, min_front=8, ref_steps=4, max_steps=2000, connectivity=1):
    """-> dict(mask, counts, leak_step, stop_step, arrival): geodesic(seed, within & (v < airway_hu)), the leak rule on its counts, arrival <= stop_step"""
    constraint = threshold(values, hi=airway_hu, region=within)[0]
    arrival, counts = geodesic(seed, constraint, connectivity, False, max_steps)
    leak, stop = leak_rule(counts, leak_ratio, min_front, ref_steps)
    return dict(mask=(arrival <= stop).astype(np.uint8), counts=counts, leak_step=leak, stop_step=stop, arrival=arrival)


def lung_mask(values, pixdim, superior=None, candidates=None, air_hu=-320.0, body_hu=-500.0, airways="auto", airway_dilate_mm=None, min_lung_ml=50.0, min_ratio=0.25,
              fill=True, close_mm=None, trachea_kw=None, **grow_kw):
    """lungs.lung_mask on decoded values -> dict(mask, airways: grow_airways' dict or None, airway_error, kept: the kept labels of the labelling, voxels: their counts,
    error: None or the LungMaskError's reason).  superior: "z+", "z-" or None (no orientation, or axis 2 is no S / I axis); candidates: a lung U-Net's thresholded
    prediction in place of (v < air_hu) & body_mask."""
    cand = (threshold(values, hi=air_hu, region=body_mask(values, body_hu))[0] if candidates is None else (np.asarray(candidates) != 0).astype(np.uint8))
    grown, why = None, None
    if airways is not False:
        if superior is None:
            why = "no orientation"
        else:
            seed = find_trachea(cand, pixdim, superior, **(trachea_kw or {}))
            if seed is None:
                why = "no trachea"
            else:
                grown = grow_airways(values, seed["mask"], reconstruct(cand, seed["mask"], 1), **grow_kw)
                wide = MO.dilation(grown["mask"], 3) if airway_dilate_mm is None else MO.dilate_mm(grown["mask"], airway_dilate_mm, pixdim)
                cand = cand & (1 - wide)
    lab, n = CO.label(cand, 1)
    vox = np.bincount(lab.reshape(-1), minlength=n + 1)[1:].astype(np.int64)
    least = CO.min_voxels_from_ml(min_lung_ml, pixdim)
    order = sorted((l for l in range(1, n + 1) if vox[l - 1] >= least), key=lambda l: (-int(vox[l - 1]), l))[:2]
    if not order:
        return dict(mask=None, airways=grown, airway_error=why, kept=[], voxels=[], error="no component reaches min_lung_ml")
    kept = order[:1] + [l for l in order[1:] if float(vox[l - 1]) >= float(min_ratio) * float(vox[order[0] - 1])]
    mask = np.isin(lab, kept).astype(np.uint8)
    if fill:
        mask = MO.fill_holes(mask, 1, planar=True)
    if close_mm is not None:
        mask = MO.close_mm(mask, close_mm, pixdim)
    return dict(mask=mask, airways=grown, airway_error=why, kept=sorted(kept), voxels=[int(vox[l - 1]) for l in sorted(kept)], error=None)


def dice(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return 2.0 * float((a & b).sum()) / float(a.sum() + b.sum())


# ---- test volumes ---------------------------------------------------------------------------------------------------------------------------------------------------
PHANTOM_SHAPE, PHANTOM_PIXDIM = (112, 96, 56), (1.5, 1.5, 3.0)


def _tube(P, a, b, ra, rb):
    """the voxels within a radius that tapers from ra at point a to rb at point b of the segment a-b (millimetres)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = b - a
    t = np.clip(((P - a) @ d) / float(d @ d), 0.0, 1.0)
    r = ra + (rb - ra) * t
    return ((P - (a + t[..., None] * d)) ** 2).sum(-1) <= r * r


def phantom(leak=False, superior="z-", seed=7, shape=PHANTOM_SHAPE, pixdim=PHANTOM_PIXDIM, noise=35.0):
    """A chest of 112 x 96 x 56 voxels of 1.5 x 1.5 x 3.0 mm as int16 HU -> dict(hu, lungs: the two true ellipsoids, trachea: the tube above the carina outside the
    lungs, leak_region, pixdim, superior).  An elliptic body cylinder at 40 HU in -1000 HU air, a table plate, two ellipsoid lungs at -850 HU, a trachea tube of 8 mm
    radius at -990 HU from the superior end to a carina, two tapering bronchi into the lungs, a vessel, a pleural consolidation, a bowel-gas pocket, Gaussian noise of
    sigma = 35 HU from a fixed seed; leak=True: a -975 HU region at the end of one bronchus.  Built with the superior end at z = 0 ("z-"); "z+" stores it flipped.
    The anatomy is laid out in millimetres inside 168 x 144 x 168 mm: another shape / pixdim samples the same chest (tools/lungmask_bench.py)."""
    X, Y, Z = shape
    px, py, pz = pixdim
    g = np.meshgrid(np.arange(X) * px, np.arange(Y) * py, np.arange(Z) * pz, indexing="ij")
    P = np.stack(g, -1)
    x, y, z = g
    hu = np.full(tuple(shape), -1000.0)
    body = ((x - 84.0) / 75.0) ** 2 + ((y - 72.0) / 60.0) ** 2 <= 1.0
    hu[body] = 40.0
    hu[(np.abs(x - 84.0) <= 64.0) & (y >= 136.5) & (y <= 141.0)] = 200.0                                     # the table plate, clear of the body
    lung_l = ((x - 52.0) / 24.0) ** 2 + ((y - 72.0) / 36.0) ** 2 + ((z - 96.0) / 48.0) ** 2 <= 1.0
    lung_r = ((x - 116.0) / 24.0) ** 2 + ((y - 72.0) / 36.0) ** 2 + ((z - 96.0) / 48.0) ** 2 <= 1.0
    lungs = lung_l | lung_r
    hu[lungs] = -850.0
    hu[_tube(P, (44.0, 84.0, 70.0), (44.0, 84.0, 125.0), 2.0, 2.0) & lungs] = 40.0                            # a vessel
    hu[(((x - 140.0) ** 2 + (y - 72.0) ** 2 + (z - 96.0) ** 2) <= 64.0) & lungs] = 20.0                       # a consolidation at the pleura
    hu[((x - 84.0) / 12.0) ** 2 + ((y - 96.0) / 8.0) ** 2 + ((z - 158.0) / 6.0) ** 2 <= 1.0] = -1000.0          # bowel gas
    carina = (84.0, 60.0, 66.0)
    trachea = _tube(P, (84.0, 60.0, -10.0), carina, 8.0, 8.0)
    ends = ((56.0, 68.0, 96.0), (112.0, 68.0, 96.0))
    airway = trachea | _tube(P, carina, ends[0], 6.0, 3.5) | _tube(P, carina, ends[1], 6.0, 3.5)
    hu[airway] = -990.0
    leak_region = (((x - ends[0][0]) ** 2 + (y - ends[0][1]) ** 2 + (z - ends[0][2] - 12.0) ** 2) <= 15.0 ** 2) & lung_l & ~airway
    if leak:
        hu[leak_region] = -975.0
    hu = np.rint(hu + np.random.default_rng(seed).normal(0.0, float(noise), tuple(shape))).astype(np.int16)
    out = dict(hu=hu, lungs=lungs.astype(np.uint8), trachea=(airway & ~lungs).astype(np.uint8), leak_region=leak_region.astype(np.uint8), pixdim=tuple(pixdim),
               superior=superior)
    if superior == "z+":
        for k in ("hu", "lungs", "trachea", "leak_region"):
            out[k] = np.ascontiguousarray(out[k][:, :, ::-1])
    return out


def serpentine(X, Y):
    """a corridor one voxel wide that runs along x, turns at the ends and covers every second row of an [X, Y, 1] volume -> (constraint, seed at its start, length)"""
    c = np.zeros((X, Y, 1), np.uint8)
    for y in range(0, Y, 2):
        c[:, y, 0] = 1
        if y + 1 < Y and y + 2 < Y:
            c[X - 1 if (y // 2) % 2 == 0 else 0, y + 1, 0] = 1
    s = np.zeros_like(c)
    s[0, 0, 0] = 1
    return c, s, int(c.sum())


# ---- the later trips of the bounded grids (tests/later_trips.py's rule) ---------------------------------------------------------------------------------------------
TPB, GRID_CAP, TH_VEC = 256, 256 * 32, 8                              # kernels_lungmask.hip, restated; tests/test_lungmask_host.py reads them out of its text
TRIP = GRID_CAP * TPB
LATER_THRESHOLD_VEC = (257, 254, 515)                                 # uint8, aligned: items of 8 voxels, two whole trips, a ragged third and a short last item
LATER_THRESHOLD_ONE = (67, 251, 250)                                  # int16 one element into its buffer: the one-voxel form
LATER_GROWTH = (2, 2051, 2047)                                        # one word per row: Y Z words, just above two trips of the step kernel, under 10 M voxels

"""-m gpu: csrc/kernels_zones.hip and zones.lung_zones / lung_distribution / segment_volume(distribution=) against tests/zones_oracle.py.  Boxes, tables, keys and the
zone map are integers, the distances behind them are the exact transform the other oracles define: every comparison is array_equal / ==.  Every output lies between
sentinel bands that must survive."""
import gzip
import os
import re
import struct

import numpy as np
import pytest

import later_trips as LT
import lungside_oracle as LO
import zones_oracle as ZO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
SMALL = (37, 29, 23)
SENT8, SENT64, SENT32 = 0x5A, -77, -55
PIX = (1.5, 1.5, 2.5)                                               # squares exact in binary: the stored orientation cannot change a distance bit
_WANT = {}

# ---- the launch arithmetic, read from the source ------------------------------------------------------------------------------------------------------------------
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc",
                         "kernels_zones.hip")).read()
TPB = LT.constant_value(re.search(r"constexpr int TPB = ([^;]+);", _SRC).group(1))
ZT_GRID = LT.constant_value(re.search(r"constexpr int ZT_GRID = ([^;]+);", _SRC).group(1))
ZT_TABLE = LT.constant_value(re.search(r"constexpr int ZT_TABLE = ([^;]+);", _SRC).group(1))
TRIP_ITEMS = ZT_GRID * TPB                                          # items one trip of either launch covers; an item is 4 voxels on the aligned path, 1 otherwise


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.asfortranarray(np.asarray(a).astype(dtype)).reshape(-1, order="F")).cuda()


def _dev_off(a, off):
    """the flat uint8 volume `off` bytes into a larger buffer"""
    import torch
    flat = np.asfortranarray(np.asarray(a).astype(np.uint8)).reshape(-1, order="F")
    buf = torch.zeros(flat.size + 16, dtype=torch.uint8, device="cuda")
    buf[off:off + flat.size] = torch.from_numpy(flat).cuda()
    return buf, buf.data_ptr() + off


def _flat(a):
    return np.asarray(a).reshape(-1, order="F")


def _cspec(spec):
    from covidseg_amd import zones as Z
    return Z.make_spec(spec["parts"], spec["flip"], spec["lo"], spec["extent"], spec["r2"])


def _run_table(o, shape, spec, sides, inf=None, labels=None, n=0, d2=None, want_map=True, off=0):
    """-> the outputs as zones_oracle.zone_table names them; off = 1: sides, infection and the zone map one byte off their 4-byte alignment (the one-voxel path)"""
    import ctypes
    import torch
    N = int(np.prod(shape))
    P, S = int(np.prod(spec["parts"])), len(spec["r2"][0]) + 1
    B = 2 * P * S
    keep = [_dev_off(sides, off), _dev_off(inf, off) if inf is not None else (None, None)]
    lt = _dev(labels, np.int32) if labels is not None else None
    dt = _dev(d2, np.float64) if d2 is not None else None
    table = torch.full((B * 2 + 8,), SENT64, dtype=torch.int64, device="cuda")
    outside = torch.full((1 + 4,), SENT64, dtype=torch.int64, device="cuda")
    lz = torch.full((n * 2 * P + 8,), SENT64, dtype=torch.int64, device="cuda")
    lsh = torch.full((n * S + 8,), SENT64, dtype=torch.int64, device="cuda")
    ld = torch.full((n + 8,), SENT64, dtype=torch.int64, device="cuda")
    zm = torch.full((off + N + 64,), SENT8, dtype=torch.uint8, device="cuda")
    cs = _cspec(spec)
    o.ck(o.lib.unet_vol_zone_table(o.h, keep[0][1], keep[1][1], lt.data_ptr() if lt is not None else None, n, dt.data_ptr() if dt is not None else None, *shape,
                                   ctypes.byref(cs), table.data_ptr(), outside.data_ptr(), lz.data_ptr(), lsh.data_ptr(), ld.data_ptr(),
                                   zm.data_ptr() + off if want_map else None, o.s), "zone_table")
    t, ou, a, b, c, z = (x.cpu().numpy() for x in (table, outside, lz, lsh, ld, zm))
    assert (t[B * 2:] == SENT64).all() and (ou[1:] == SENT64).all() and (a[n * 2 * P:] == SENT64).all() and (b[n * S:] == SENT64).all() and (c[n:] == SENT64).all()
    if want_map:
        assert (z[:off] == SENT8).all() and (z[off + N:] == SENT8).all()
    else:
        assert (z == SENT8).all()
    return {"table": t[:B * 2].reshape(B, 2), "outside": int(ou[0]), "lesion_zone": a[:n * 2 * P].reshape(n, 2 * P), "lesion_shell": b[:n * S].reshape(n, S),
            "lesion_dmin_key": c[:n].view(np.uint64), "zone_map": z[off:off + N] if want_map else None}


def _same_table(got, want, what):
    for k in ("table", "lesion_zone", "lesion_shell", "lesion_dmin_key"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    assert got["outside"] == want["outside"], what
    if got["zone_map"] is not None:
        assert np.array_equal(got["zone_map"], _flat(want["zone_map"])), (what, "zone_map")


def _inputs(shape, rng, n, lung_share=0.6, heavy=0.3):
    """sides: two blobs split along x plus values above 2, with whole waves off the lungs; labels with negatives, values above n and INT32_MAX, lesion 1 all over the
    volume; distances on a few values (ties on the shell edges) and +inf"""
    X, Y, Z = shape
    N = X * Y * Z
    g = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    sides = np.where(g[0] < X // 2, 1, 2).astype(np.uint8)
    sides[rng.random(shape) > lung_share] = 0
    sides[rng.random(shape) < 0.03] = rng.integers(3, 256, 1, dtype=np.uint8)[0]
    f = _flat(sides).copy()
    if N > 4096:
        f[1024:3072] = 0                                            # waves of either path that see neither lung nor infection
    sides = f.reshape(shape, order="F")
    inf = (rng.random(shape) < 0.35).astype(np.uint8) * rng.integers(1, 255, shape, dtype=np.uint8)
    fi = _flat(inf).copy()
    if N > 4096:
        fi[1024:2048] = 0
    inf = fi.reshape(shape, order="F")
    labels = rng.integers(-3, n + 3, shape).astype(np.int32)
    labels[rng.random(shape) < heavy] = 1
    labels[rng.random(shape) < 0.01] = 2 ** 31 - 1
    d2 = (rng.integers(0, 16, shape) * 0.5625).astype(np.float64)
    d2[rng.random(shape) < 0.02] = np.inf
    return sides, inf, labels, d2


def _r2(S, rng):
    """squared radii on the values the distances take, so that voxels sit exactly on a shell's edge; the two sides differ"""
    return tuple(tuple(sorted((rng.choice(np.arange(1, 15), S - 1, replace=False) * 0.5625).tolist())) for _ in (0, 1))


# ---- unet_vol_zone_table, small ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [(3, 1, 1), (1, 2, 3), (8, 8, 1)])
def test_zone_table_equals_the_oracle(parts):
    o = Ops()
    rng = np.random.default_rng(sum(parts))
    n = 4
    sides, inf, labels, d2 = _inputs(SMALL, rng, n)
    lo = ((5, -3, 2), (20, 4, 30))                                   # coordinates below lo and past lo + extent clamp
    extent = ((2, 1, 9), (11, 40, 2))                                # 2 into 3 parts, 1 into any
    for S in (1, 3, 4):
        r2 = _r2(S, rng)
        for fl in range(8):
            spec = ZO.make_spec(parts, (fl & 1, (fl >> 1) & 1, (fl >> 2) & 1), lo, extent, r2)
            _same_table(_run_table(o, SMALL, spec, sides, inf, labels, n, d2), ZO.zone_table(sides, spec, inf, labels, n, d2), (S, fl))
        # each optional input null in turn, on the last flip; then everything through the one-voxel path
        _same_table(_run_table(o, SMALL, spec, sides, None, labels, n, d2), ZO.zone_table(sides, spec, None, labels, n, d2), (S, "no infection"))
        _same_table(_run_table(o, SMALL, spec, sides, inf, None, n, d2), ZO.zone_table(sides, spec, inf, None, n, d2), (S, "no labels"))
        _same_table(_run_table(o, SMALL, spec, sides, inf, labels, 0, d2), ZO.zone_table(sides, spec, inf, labels, 0, d2), (S, "n = 0"))
        _same_table(_run_table(o, SMALL, spec, sides, inf, labels, n, d2, want_map=False), ZO.zone_table(sides, spec, inf, labels, n, d2), (S, "no map"))
        _same_table(_run_table(o, SMALL, spec, sides, inf, labels, n, d2, off=1), ZO.zone_table(sides, spec, inf, labels, n, d2), (S, "one voxel per lane"))
        if S == 1:
            _same_table(_run_table(o, SMALL, spec, sides, inf, labels, n, None), ZO.zone_table(sides, spec, inf, labels, n, None), "no d2")
            _same_table(_run_table(o, SMALL, spec, sides, inf, labels, n, None, off=1), ZO.zone_table(sides, spec, inf, labels, n, None), "no d2, one voxel per lane")


@pytest.mark.parametrize("n", [4, 3000])
def test_both_arms_of_the_per_lesion_table(n):
    """n (2 P + S) within the LDS table and beyond it; lesion 1 lies all over the volume, so many workgroups add to its rows"""
    o = Ops()
    rng = np.random.default_rng(n)
    parts, S = (1, 3, 2), 3
    assert (n * (2 * 6 + S) <= ZT_TABLE) == (n == 4) and int(np.prod(SMALL)) > 8 * TPB * 4
    sides, inf, labels, d2 = _inputs(SMALL, rng, n)
    spec = ZO.make_spec(parts, (0, 1, 0), ((0, 2, 1), (18, 0, 3)), ((18, 25, 20), (19, 29, 18)), _r2(S, rng))
    want = ZO.zone_table(sides, spec, inf, labels, n, d2)
    assert want["lesion_zone"][0].sum() > 0.1 * np.prod(SMALL) and (want["lesion_zone"].sum(axis=1) == 0).any() == (n == 3000)
    for off in (0, 1):
        _same_table(_run_table(o, SMALL, spec, sides, inf, labels, n, d2, off=off), want, (n, off))
    big = np.where(labels == 1, n, labels)                           # the heavy lesion is the LAST row
    want = ZO.zone_table(sides, spec, inf, big, n, d2)
    _same_table(_run_table(o, SMALL, spec, sides, inf, big, n, d2), want, (n, "last row"))


# ---- the later trips of the bounded grid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, n", [((70, 70, 1030), 5), ((257, 129, 127), 3000)])
def test_zone_table_on_the_later_trips(shape, n):
    """Both launches take min(ceil(items / TPB), ZT_GRID) workgroups of TPB lanes and stride over the rest: TRIP_ITEMS items a trip, an item = 4 voxels on the aligned
    path and 1 on the other.  Both shapes give every workgroup at least four whole trips on the aligned path (sixteen on the other) and a further one that ends inside a
    workgroup; it ends inside a wave as well (later_trips.shape_rule) except on the aligned path of 257 x 129 x 127, whose last item is short instead (N % 4 = 3).  A trip
    crosses many slice boundaries.  More than half of the voxels past the first trip carry information (lung or infection)."""
    o = Ops()
    N = int(np.prod(shape))
    for vox in (4, 1):
        items = (N + vox - 1) // vox
        full, rest = LT.later_trips(items, TRIP_ITEMS)
        assert full >= (4 if vox == 4 else 16) and rest % TPB != 0
        assert LT.shape_rule(items, TRIP_ITEMS) or (vox == 4 and shape == (257, 129, 127) and N % 4 == 3)
    assert shape[0] * shape[1] < TRIP_ITEMS                          # a trip holds several slices
    rng = np.random.default_rng(N % 1000)
    sides, inf, labels, d2 = _inputs(shape, rng, n, lung_share=0.55)
    assert LT.tail_share((sides == 1) | (sides == 2) | (inf != 0), TRIP_ITEMS * 4) >= 0.5 and LT.tail_share((sides == 1) | (sides == 2), TRIP_ITEMS * 4) >= 0.5
    S = 3
    spec = ZO.make_spec((2, 2, 3), (1, 0, 1), ((3, 1, 10), (30, 0, 0)), ((shape[0] // 2, shape[1], shape[2] - 20), (shape[0] // 2, shape[1] - 7, shape[2])), _r2(S, rng))
    want = ZO.zone_table(sides, spec, inf, labels, n, d2)
    _same_table(_run_table(o, shape, spec, sides, inf, labels, n, d2), want, "aligned")
    _same_table(_run_table(o, shape, spec, sides, inf, labels, n, d2, off=1), want, "one voxel per lane")


# ---- unet_vol_side_extents ------------------------------------------------------------------------------------------------------------------------------------------
def _run_extents(o, shape, sides, d2=None, off=0):
    import torch
    keep = _dev_off(sides, off)
    dt = _dev(d2, np.float64) if d2 is not None else None
    box = torch.full((12 + 8,), SENT32, dtype=torch.int32, device="cuda")
    dmax = torch.full((2 + 4,), SENT64, dtype=torch.int64, device="cuda")
    o.ck(o.lib.unet_vol_side_extents(o.h, keep[1], dt.data_ptr() if dt is not None else None, *shape, box.data_ptr(), dmax.data_ptr(), o.s), "side_extents")
    b, d = box.cpu().numpy(), dmax.cpu().numpy()
    assert (b[12:] == SENT32).all() and (d[2:] == SENT64).all()
    return b[:12].reshape(2, 6), d[:2].view(np.uint64)


def _check_extents(o, shape, sides, d2, what):
    wb, wd = ZO.side_extents(sides, d2)
    for off in (0, 1):
        gb, gd = _run_extents(o, shape, sides, d2, off)
        assert np.array_equal(gb, wb) and np.array_equal(gd, wd), (what, off)
    return wb, wd


def test_side_extents_equal_the_oracle():
    o = Ops()
    rng = np.random.default_rng(3)
    sides, _, _, d2 = _inputs(SMALL, rng, 1)
    _check_extents(o, SMALL, sides, d2, "random")
    wb, wd = _check_extents(o, SMALL, sides, None, "no d2")
    assert wd.tolist() == [0, 0]
    wb, wd = _check_extents(o, SMALL, np.where(sides == 2, 7, sides), d2, "an empty side")          # 7 counts as 0
    assert wb[1].tolist() == [2 ** 31 - 1, -1] * 3 and wd[1] == 0 and wd[0] > 0
    one = np.zeros(SMALL, np.uint8); one[36, 0, 22] = 2; one[5, 7, 11] = 1
    wb, wd = _check_extents(o, SMALL, one, d2, "single voxels")
    assert wb[1].tolist() == [36, 36, 0, 0, 22, 22] and wb[0].tolist() == [5, 5, 7, 7, 11, 11]
    faces = np.zeros(SMALL, np.uint8); faces[0, 3, 3] = faces[36, 4, 4] = faces[7, 0, 5] = faces[8, 28, 6] = faces[9, 9, 0] = faces[10, 10, 22] = 1
    wb, _ = _check_extents(o, SMALL, faces, d2, "all six faces")
    assert wb[0].tolist() == [0, 36, 0, 28, 0, 22]
    _check_extents(o, SMALL, np.zeros(SMALL, np.uint8), d2, "no lung at all")


def test_side_extents_on_the_later_trips():
    """the largest distance and the far corner of the box sit on voxels that only the last trip reaches"""
    o = Ops()
    shape = (257, 129, 127)
    N = int(np.prod(shape))
    assert LT.later_trips((N + 3) // 4, TRIP_ITEMS)[0] >= 4 and N % 4 == 3 and LT.shape_rule(N, TRIP_ITEMS)
    rng = np.random.default_rng(9)
    sides, _, _, d2 = _inputs(shape, rng, 1, lung_share=0.55)
    sides[:, :, 100:] = np.where(sides[:, :, 100:] == 2, 0, sides[:, :, 100:])
    d2[np.isinf(d2)] = 1.0
    sides[250, 120, 126], d2[250, 120, 126] = 2, 1e6                 # flat index past 4 trips of the aligned path
    sides[3, 2, 125], d2[3, 2, 125] = 1, np.inf
    assert 250 + 257 * (120 + 129 * 126) >= 4 * TRIP_ITEMS * 4
    wb, wd = _check_extents(o, shape, sides, d2, "later trips")
    assert wb[1, 5] == 126 and ZO.unkey(wd[1]) == 1e6 and ZO.unkey(wd[0]) == np.inf


# ---- what the entries refuse --------------------------------------------------------------------------------------------------------------------------------------------
def test_the_entries_refuse_bad_arguments_and_touch_nothing():
    import ctypes
    import torch
    o = Ops()
    shape = (8, 6, 5)
    N = int(np.prod(shape))
    sides, d2 = _dev(np.ones(shape), np.uint8), torch.ones(N + 2, dtype=torch.float64, device="cuda")
    labels = torch.ones(N, dtype=torch.int32, device="cuda")
    out = torch.full((4096,), SENT64, dtype=torch.int64, device="cuda")
    zm = torch.full((N,), SENT8, dtype=torch.uint8, device="cuda")
    good = dict(parts=(2, 1, 3), flip=(0, 1, 0), lo=((0, 0, 0), (1, 1, 1)), extent=((4, 6, 5), (3, 3, 3)), r2=((1.0, 2.0), (0.0, 0.0)))

    def call(spec=None, n=2, d=d2.data_ptr(), shp=shape, zmap=zm.data_ptr(), raw=None):
        cs = raw if raw is not None else _cspec(ZO.make_spec(**{**good, **(spec or {})}))
        p = out.data_ptr()
        rc = o.lib.unet_vol_zone_table(o.h, sides.data_ptr(), None, labels.data_ptr(), n, d, *shp, ctypes.byref(cs), p, p + 8192, p + 8200, p + 16384, p + 24576, zmap, o.s)
        torch.cuda.synchronize()
        return rc

    bad = [dict(parts=(0, 1, 1)), dict(parts=(9, 1, 1)), dict(flip=(0, 2, 0)), dict(extent=((4, 0, 5), (3, 3, 3))), dict(extent=((4, 6, 5), (3, 3, -1))),
           dict(r2=((-1.0, 2.0), (0.0, 0.0))), dict(r2=((2.0, 1.0), (0.0, 0.0))), dict(r2=((1.0, 2.0), (0.0, float("nan")))), dict(r2=((1.0, float("inf")), (0.0, 0.0))),
           dict(parts=(8, 8, 8), r2=((1.0,), (1.0,)))]
    for spec in bad:
        assert call(spec) == E_ARG, spec
    raw = _cspec(ZO.make_spec(**good))
    for S in (0, 5):
        raw.shells = S
        assert call(raw=raw) == E_ARG
    assert call(d=None) == E_ARG                                     # shells without distances
    assert call(dict(parts=(8, 8, 8), r2=((), ()))) == E_ARG          # 1024 regions do not fit the zone map's byte ...
    assert call(dict(parts=(8, 8, 8), r2=((), ())), zmap=None, n=0) == 0          # ... but the table alone is 1024 bins
    out.fill_(SENT64)
    assert call(n=-1) == E_ARG and call(d=d2.data_ptr() + 4) == E_ARG and call(shp=(2048, 2048, 512)) == E_ARG and call(shp=(-1, 6, 5)) == E_ARG
    assert call(shp=(8, 0, 5)) == 0                                  # a zero dimension: UNET_OK, nothing touched
    box = torch.full((12,), SENT32, dtype=torch.int32, device="cuda")
    ext = lambda shp, d=None: o.lib.unet_vol_side_extents(o.h, sides.data_ptr(), d, *shp, box.data_ptr(), out.data_ptr(), o.s)
    assert ext((8, 0, 5)) == 0 and ext((2048, 2048, 512)) == E_ARG and ext((8, 6, -5)) == E_ARG and ext(shape, d2.data_ptr() + 4) == E_ARG
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT64).all() and (zm.cpu().numpy() == SENT8).all() and (box.cpu().numpy() == SENT32).all()


# ---- zones.lung_zones / lung_distribution ---------------------------------------------------------------------------------------------------------------------------------
SHAPE = (48, 40, 36)
CODES = [("R", "A", "S"), ("L", "P", "S"), ("L", "A", "I"), ("S", "R", "A"), ("A", "I", "L"), ("P", "S", "R")]          # the last three permute all three axes
CONFIGS = {"thirds": dict(), "mm": dict(zones=2, ap_parts=2, extent="both", depth=("mm", (4.5, 9.0, 13.5)), fill=False)}


def _phantom():
    """in the canonical frame (axes grow to the patient's Right, Anterior, Superior): the sides of two fused lungs with a hole, an infection of a few blobs"""
    if "phantom" not in _WANT:
        lung = LO.fused_lungs(SHAPE, PIX)
        sides = LO.split(lung, LO.affine_of("RAS", PIX), PIX)["sides"].copy()
        sides[12:15, 18:21, 16:19] = 0                                # a vessel missing from the lung mask
        inf = np.zeros(SHAPE, np.uint8)
        inf[6:14, 12:22, 24:31] = 1                                   # high in one lung, through the hole's neighbourhood
        inf[30:36, 24:30, 6:12] = 1                                   # low and anterior in the other
        inf[22:26, 18:22, 15:20] = 1                                  # at the junction: both sides
        inf[12:15, 18:21, 16:19] = 1                                  # in the hole: outside the lungs
        inf[0:3, 0:3, 0:2] = 1                                        # outside
        _WANT["phantom"] = (sides, inf)
    return _WANT["phantom"]


def _rows(lesions):
    return sorted((str(r["side"]), int(r["zone"]), int(r["ap"]), int(r["voxels_in_lung"]), tuple(int(v) for v in r["voxels_shell"]),
                   None if np.isnan(r["depth_mm"]) else float(r["depth_mm"]), bool(r["subpleural"])) for r in lesions)


def _check_report(d, want, ordered=True):
    """a LungDistribution against zones_oracle.distribution's dict; ordered: the lesions row by row (one labelling), else as a set of rows"""
    zones, apn = want["scores"].shape[1:]
    assert np.array_equal(d.regions["lung_voxels"].reshape(2, zones, apn), want["region_voxels"][..., 0])
    assert np.array_equal(d.regions["infected_voxels"].reshape(2, zones, apn), want["region_voxels"][..., 1])
    assert np.array_equal(d.regions["lung_ml"].reshape(2, zones, apn), want["region_ml"][..., 0]) and np.array_equal(d.regions["infected_ml"].reshape(2, zones, apn), want["region_ml"][..., 1])
    S = want["shell_voxels"].shape[1]
    assert np.array_equal(d.shells["lung_voxels"].reshape(2, S), want["shell_voxels"][..., 0]) and np.array_equal(d.shells["infected_voxels"].reshape(2, S), want["shell_voxels"][..., 1])
    assert [d.left.lung_voxels, d.right.lung_voxels] == want["side_voxels"][:, 0].tolist() and [d.left.infected_voxels, d.right.infected_voxels] == want["side_voxels"][:, 1].tolist()
    assert d.outside_voxels == want["outside_voxels"] and d.outside_ml == want["outside_ml"]
    assert np.array_equal(d.severity["scores"], want["scores"]) and np.array_equal(d.regions["score"].reshape(2, zones, apn), want["scores"])
    assert d.severity["total"] == want["total"] and d.severity["max_total"] == want["max_total"]
    assert (d.bilateral, d.craniocaudal, d.axial, d.anteroposterior) == (want["bilateral"], want["craniocaudal"], want["axial"], want["anteroposterior"])
    if ordered:
        assert d.lesions["label"].tolist() == [r["label"] for r in want["lesions"]]
        for g, w in zip(d.lesions, want["lesions"]):
            assert (str(g["side"]), int(g["zone"]), int(g["ap"]), int(g["voxels_in_lung"]), bool(g["subpleural"])) == (w["side"], w["zone"], w["ap"], w["voxels_in_lung"], w["subpleural"])
            assert np.array_equal(g["voxels_shell"], w["voxels_shell"]) and (g["depth_mm"] == w["depth_mm"] or (np.isnan(g["depth_mm"]) and np.isnan(w["depth_mm"])))
    else:
        assert _rows(d.lesions) == _rows([{**w, "voxels_shell": np.asarray(w["voxels_shell"])} for w in want["lesions"]])


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("codes", CODES, ids=["".join(c) for c in CODES])
def test_lung_zones_and_distribution_equal_the_oracle_in_every_orientation(codes, name):
    from covidseg_amd import volume as V, zones as Z
    kw = CONFIGS[name]
    sides, inf = _phantom()
    if name not in _WANT:                                            # the canonical report, computed once
        _WANT[name] = ZO.distribution(inf, ZO.lung_zones(sides, ("R", "A", "S"), PIX, **kw))
    canon = _WANT[name]
    s, i, pix = LO.reorient(sides, codes), LO.reorient(inf, codes), LO.reorient_pixdim(PIX, codes)
    wz = ZO.lung_zones(s, codes, pix, **kw)
    want = ZO.distribution(i, wz)
    ls = V.LungSides(sides=s, shape=s.shape, axcodes=codes, pixdim=pix, radius_mm=0.0, voxels=None)
    lz = Z.lung_zones(ls, **kw)
    assert np.array_equal(lz.box, wz["box"]) and np.array_equal(lz.zone_map, wz["zone_map"]) and lz.zone_map.dtype == np.uint8
    assert [float(lz.spec.r2[t][k]) for t in (0, 1) for k in range(lz.shells - 1)] == [v for t in (0, 1) for v in wz["spec"]["r2"][t]]
    assert np.array_equal(np.asarray(lz.spec.lo).reshape(2, 3), wz["spec"]["lo"]) and np.array_equal(np.asarray(lz.spec.extent).reshape(2, 3), wz["spec"]["extent"])
    assert np.array_equal(lz.d2.cpu().numpy(), _flat(wz["d2"])) and lz.axcodes == codes
    assert np.array_equal(lz.lung_voxels.sum(axis=3), canon["region_voxels"][..., 0])
    d = Z.lung_distribution(i, lz)
    _check_report(d, want)
    _check_report(d, canon, ordered=False)                           # the same report whichever way the volume is stored
    b = V.lung_burden(i, s, pixdim=pix)                              # the regions add up to the per-lung numbers
    assert (d.left.lung_voxels, d.left.infected_voxels, d.right.lung_voxels, d.right.infected_voxels) == \
        (b.left.lung_voxels, b.left.infected_voxels, b.right.lung_voxels, b.right.infected_voxels) and d.outside_voxels == b.outside_voxels
    P = d.zones.zones * d.zones.ap_parts
    assert d.regions["lung_voxels"][:P].sum() == b.left.lung_voxels and d.regions["infected_voxels"][P:].sum() == b.right.infected_voxels
    if codes == CODES[3]:                                            # the other ways in: the caller's labels on the device, a plain array with orientation=, the default zones
        lab, n = V.label_volume(i, return_device=True)
        _check_report(Z.lung_distribution(_dev(i, np.uint8), lz, labels=lab, n=n, shape=s.shape), want)
        lz2 = Z.lung_zones(s, orientation="".join(codes), pixdim=pix, return_device=True, **kw)
        assert np.array_equal(lz2.zone_map.cpu().numpy(), _flat(wz["zone_map"]))
        if name == "thirds":
            _check_report(Z.lung_distribution(i, ls), want)
            assert canon["bilateral"] and canon["outside_voxels"] >= 27 + 18 and canon["total"] > 0
        layer = d.layer()
        assert layer.labels is d.zones.zone_map and layer.palette.shape == (2 * P + 1, 3) and len({tuple(c) for c in layer.palette[1:]}) == min(2 * P, 8)


def test_no_depth_and_an_empty_lung():
    from covidseg_amd import volume as V, zones as Z
    sides, inf = _phantom()
    one = np.where(sides == 2, 0, sides)                            # the right lung is missing
    codes = ("L", "P", "S")
    s, i, pix = LO.reorient(one, codes), LO.reorient(inf, codes), LO.reorient_pixdim(PIX, codes)
    ls = V.LungSides(sides=s, shape=s.shape, axcodes=codes, pixdim=pix)
    for kw in (dict(depth=None), dict(), dict(extent="both")):
        lz = Z.lung_zones(ls, **kw)
        wz = ZO.lung_zones(s, codes, pix, **kw)
        assert np.array_equal(lz.zone_map, wz["zone_map"]) and (lz.d2 is None) == ("depth" in kw)
        d = Z.lung_distribution(i, lz)
        _check_report(d, ZO.distribution(i, wz))
        assert not d.bilateral and np.isnan(d.right.fraction) and (d.axial is None) == ("depth" in kw)
        assert np.isnan(d.lesions["depth_mm"]).all() == ("depth" in kw)
    none = Z.lung_distribution(np.zeros(s.shape, np.uint8), lz)
    assert none.craniocaudal == "none" and none.axial == "none" and none.severity["total"] == 0 and len(none.lesions) == 0 and not none.bilateral


# ---- segment_volume(distribution=) ----------------------------------------------------------------------------------------------------------------------------------------
SIZE, NZ, NEW_DIM = 128, 20, 64
F = np.float32
PCODES = ("P", "L", "S")                                            # the lungs of the patient lie side by side along voxel axis 1, which grows to the patient's left


def _patient(tmp_path, oriented=True):
    """a CT (int16, slope 0.5, inter -1000) and its lung mask -- two ellipses per slice that grow with z --, both files with the same sform (or neither with one)"""
    from covidseg_amd import nifti_min
    from covidseg_amd.data import synthetic_ct
    x, _ = synthetic_ct(NZ, SIZE, seed=23)
    ct = np.empty((SIZE, SIZE, NZ), np.int16, order="F")
    lung = np.zeros((SIZE, SIZE, NZ), np.uint8, order="F")
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    for z in range(NZ):
        ct[:, :, z] = np.round(x[z, :, :, 0] * 2800).astype(np.int16)
        if z not in (0, NZ - 1):
            r = 1.0 + 0.015 * (z - NZ / 2)
            lung[:, :, z] = (((xx - 36) / (20 * r)) ** 2 + ((yy - 64) / (40 * r)) ** 2 < 1) | (((xx - 92) / (22 * r)) ** 2 + ((yy - 66) / (38 * r)) ** 2 < 1)
    pix = (0.75, 0.75, 5.0)
    hdr = bytearray(nifti_min.default_header(ct.shape, pix))
    if oriented:
        struct.pack_into("<h", hdr, 254, 1)
        struct.pack_into("<12f", hdr, 280, *LO.affine_of(PCODES, pix)[:3].reshape(-1))
    paths = [tmp_path / "ct.nii.gz", tmp_path / "lung.nii.gz"]
    nifti_min.write(paths[1], lung, bytes(hdr))
    h = bytearray(hdr)
    struct.pack_into("<2h", h, 70, 4, 16); struct.pack_into("<3f", h, 108, 352.0, 0.5, -1000.0)
    paths[0].write_bytes(gzip.compress(bytes(h) + b"\0\0\0\0" + ct.tobytes(order="F"), 1))
    return paths, lung, pix


class _Stub:
    """clip(a x + b ramp, 0, 1): a model that marks part of every slice without training"""

    def __init__(self, a, b, d=NEW_DIM):
        self.h, self.a, self.b = d, F(a), F(b)
        i, j = np.mgrid[0:d, 0:d].astype(F)
        self.ramp = ((F(1.3) * i + F(0.9) * j + i * j / F(d)) / F(3.2 * d)).astype(F)[None, :, :, None]

    def __call__(self, x):
        return np.clip((self.a * np.asarray(x, F) + (self.b * self.ramp).astype(F)).astype(F), F(0), F(1)).astype(F)

    def predict(self, x, batch_size=32):
        return self(x.cpu().numpy() if hasattr(x, "cpu") else x)


def _threshold(paths, stub):
    from covidseg_amd import volume as V
    r1, r2, kept = V.load_volume(paths[1], "lungs", img_size=SIZE)
    x = V.load_volume(paths[0], "cts", img_size=SIZE, rects=(r1, r2, kept), box_indexing="slice", new_dim=NEW_DIM).cpu().numpy()
    return float(np.quantile(stub(x), 0.9))


def _check_distribution(res, pix, connectivity=1, **kw):
    """res.distribution against the oracle applied to the sides and the mask the pipeline returned"""
    from covidseg_amd import volume as V
    pix = tuple(float(np.float32(v)) for v in pix)
    assert res.distribution_error is None and res.seconds["distribution"] > 0.0 and res.per_lung is not None
    sides = res.per_lung.sides.sides
    rep = {k: kw.pop(k) for k in ("severity_edges", "predominance") if k in kw}
    wz = ZO.lung_zones(sides, PCODES, pix, **kw)
    lab, n = V.label_volume(res.mask, connectivity)
    d = res.distribution
    _check_report(d, ZO.distribution(res.mask, wz, lab, n, **rep))
    assert isinstance(d.zones.zone_map, np.ndarray) and np.array_equal(d.zones.zone_map, wz["zone_map"]) and d.zones.d2 is None
    assert d.left.infected_voxels == res.per_lung.left.infected_voxels and d.right.lung_voxels == res.per_lung.right.lung_voxels and d.outside_voxels == res.per_lung.outside_voxels
    if res.lesions is not None:
        assert np.array_equal(d.lesions["label"], res.lesions["label"])
        assert np.array_equal(d.lesions["voxels_in_lung"], res.per_lung.lesions["voxels_left"] + res.per_lung.lesions["voxels_right"])
    return d


def test_segment_volume_reports_the_distribution(tmp_path):
    from covidseg_amd import volume as V
    paths, lung, pix = _patient(tmp_path)
    stub = _Stub(0.9, 0.35)
    kw = dict(lung_mask=paths[1], threshold=_threshold(paths, stub), batch_size=8, img_size=SIZE)
    with pytest.raises(ValueError, match="per_lung"):
        V.segment_volume(paths[0], stub, distribution=True, **kw)
    plain = V.segment_volume(paths[0], stub, min_lesion_ml=0.05, per_lung=True, **kw)
    assert plain.distribution is None and plain.distribution_error is None and "distribution" not in plain.seconds and plain.per_lung is not None
    res = V.segment_volume(paths[0], stub, min_lesion_ml=0.05, per_lung=True, distribution=True, **kw)          # on the labels of the filter
    assert res.mask.any() and res.n_lesions > 0
    for k, v in plain.__dict__.items():                              # distribution= changes nothing else
        if k in ("seconds", "distribution"):
            continue
        if k == "per_lung":
            for kk, vv in v.__dict__.items():
                if kk in ("left", "right"):
                    assert vv.__dict__ == res.per_lung.__dict__[kk].__dict__, kk
                elif kk == "sides":
                    assert np.array_equal(vv.sides, res.per_lung.sides.sides) and vv.voxels == res.per_lung.sides.voxels
                else:
                    assert V._same(vv, res.per_lung.__dict__[kk]) or vv == res.per_lung.__dict__[kk], kk
        else:
            assert V._same(v, res.__dict__[k]) or v == res.__dict__[k], k
    d = _check_distribution(res, pix)
    print(f"{res.n_lesions} lesions; {d!r}; scores {d.severity['scores'].reshape(-1).tolist()}")
    res = V.segment_volume(paths[0], stub, per_lung=True, connectivity=2, **kw,
                           distribution={"zones": 2, "ap_parts": 2, "depth": ("mm", (3.0,)), "extent": "both", "severity_edges": (10, 30), "predominance": 0.6})
    assert res.lesions is None                                       # no lesion table: the mask is labelled for the report alone
    _check_distribution(res, pix, connectivity=2, zones=2, ap_parts=2, depth=("mm", (3.0,)), extent="both", severity_edges=(10, 30), predominance=0.6)


def test_a_ct_without_orientation_keeps_the_segmentation(tmp_path):
    from covidseg_amd import volume as V
    paths, lung, pix = _patient(tmp_path, oriented=False)
    stub = _Stub(0.9, 0.35)
    kw = dict(lung_mask=paths[1], threshold=_threshold(paths, stub), batch_size=8, img_size=SIZE)
    plain = V.segment_volume(paths[0], stub, lesions=True, **kw)
    res = V.segment_volume(paths[0], stub, lesions=True, per_lung=True, distribution=True, **kw)
    assert res.distribution is None and "orientation" in res.distribution_error and res.distribution_error == res.per_lung_error
    assert np.array_equal(res.mask, plain.mask) and np.array_equal(res.lesions, plain.lesions) and res.seconds["distribution"] >= 0.0
    res = V.segment_volume(paths[0], stub, lesions=True, per_lung={"orientation": "PLS"}, distribution={"zones": 3}, **kw)          # the orientation as an argument
    _check_distribution(res, pix, zones=3)


def test_segment_volume_ensemble_reports_the_distribution(tmp_path):
    from covidseg_amd import volume as V
    paths, lung, pix = _patient(tmp_path)
    stubs = [_Stub(0.9, 0.35), _Stub(0.6, 0.8)]
    kw = dict(tta=("id", "hflip"), combine="majority", lung_mask=paths[1], threshold=_threshold(paths, stubs[0]), batch_size=8, img_size=SIZE)
    with pytest.raises(ValueError, match="per_lung"):
        V.segment_volume_ensemble(paths[0], stubs, distribution=True, **kw)
    res = V.segment_volume_ensemble(paths[0], stubs, lesions=True, per_lung=True, distribution=True, **kw)
    assert res.mask.any()
    _check_distribution(res, pix)

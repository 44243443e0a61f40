"""CPU: tests/zones_oracle.py against a per-voxel loop and scipy.ndimage, the severity and predominance rules at their edges, the anatomical numbering under all 48 axis
codes, the new entries' declarations and bindings, and every argument error of zones.lung_zones / lung_distribution / segment_volume(distribution=), which must be
raised before a device is needed."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import lungside_oracle as LO
import zones_oracle as ZO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unet_vol_side_extents": 9, "unet_vol_zone_table": 17}
PIX = (1.5, 1.5, 2.5)                                                # squares exact in binary: a stored orientation cannot change a distance bit


# ---- the oracle against a per-voxel loop ----------------------------------------------------------------------------------------------------------------------
def _key_py(d):
    u = int(np.array([d], np.float64).view(np.uint64)[0])
    return (~u & (2 ** 64 - 1)) if (u >> 63) else (u | (1 << 63))


def _brute(sides, spec, infection, labels, n, d2):
    parts, flip = spec["parts"], spec["flip"]
    P, S = parts[0] * parts[1] * parts[2], len(spec["r2"][0]) + 1
    table = np.zeros((2 * P * S, 2), np.int64)
    lz, lsh, ld = np.zeros((n, 2 * P), np.int64), np.zeros((n, S), np.int64), [2 ** 64 - 1] * n
    zmap = np.zeros(sides.shape, np.uint8)
    outside = 0
    for x in range(sides.shape[0]):
        for y in range(sides.shape[1]):
            for z in range(sides.shape[2]):
                s = int(sides[x, y, z])
                s = s if s in (1, 2) else 0
                inf = infection is not None and infection[x, y, z] != 0
                if s == 0:
                    outside += inf
                    continue
                q = []
                for a, c in enumerate((x, y, z)):
                    lo, ext = int(spec["lo"][s - 1][a]), int(spec["extent"][s - 1][a])
                    d = (lo + ext - 1 - c) if flip[a] else (c - lo)
                    q.append(min(max((d * parts[a]) // ext, 0), parts[a] - 1))
                zone = q[0] + parts[0] * (q[1] + parts[1] * q[2])
                d = 0.0 if d2 is None else float(d2[x, y, z])
                shell = sum(1 for k in range(S - 1) if _key_py(d) > _key_py(spec["r2"][s - 1][k]))
                b = ((s - 1) * P + zone) * S + shell
                table[b, 0] += 1
                table[b, 1] += inf
                zmap[x, y, z] = 1 + (s - 1) * P + zone
                l = 0 if labels is None else int(labels[x, y, z])
                if 1 <= l <= n:
                    lz[l - 1, (s - 1) * P + zone] += 1
                    lsh[l - 1, shell] += 1
                    ld[l - 1] = min(ld[l - 1], _key_py(d))
    return table, outside, lz, lsh, np.array(ld, np.uint64), zmap


def _small(rng, shape=(9, 8, 7)):
    sides = rng.integers(0, 5, shape).astype(np.uint8)                # 3 and 4 count as 0
    inf = (rng.random(shape) < 0.4).astype(np.uint8) * 7
    labels = rng.integers(-2, 7, shape).astype(np.int32)
    labels[0, 0, 0] = 2 ** 31 - 1
    d2 = (rng.integers(0, 12, shape) * 0.75).astype(np.float64)
    d2[1::5, ::2, ::3] = np.inf
    return sides, inf, labels, d2


@pytest.mark.parametrize("parts, flip, S", [((3, 1, 1), (0, 0, 0), 1), ((1, 2, 3), (1, 0, 1), 3), ((2, 2, 2), (1, 1, 1), 4), ((8, 8, 1), (0, 1, 0), 2)])
def test_the_oracle_equals_a_loop_over_the_voxels(parts, flip, S):
    rng = np.random.default_rng(sum(parts) + S)
    sides, inf, labels, d2 = _small(rng)
    r2 = tuple(tuple(sorted(rng.choice(np.arange(1, 11) * 0.75, S - 1, replace=False).tolist())) for _ in (0, 1))          # on the values of d2: ties on the shell edges
    spec = ZO.make_spec(parts, flip, lo=((1, 0, 2), (-3, 2, 0)), extent=((5, 8, 2), (9, 1, 7)), r2=r2)
    n = 4
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0 if S == 1 else 1)):
        i, l, d = (inf if use[0] else None), (labels if use[1] else None), (d2 if use[2] else None)
        got = ZO.zone_table(sides, spec, i, l, n, d)
        table, outside, lz, lsh, ld, zmap = _brute(sides, spec, i, l, n, d)
        assert np.array_equal(got["table"], table) and got["outside"] == outside and np.array_equal(got["zone_map"], zmap), use
        assert np.array_equal(got["lesion_zone"], lz) and np.array_equal(got["lesion_shell"], lsh) and np.array_equal(got["lesion_dmin_key"], ld), use
    assert got["table"][:, 0].sum() == np.isin(sides, (1, 2)).sum()


def test_extents_and_keys():
    rng = np.random.default_rng(5)
    sides, _, _, d2 = _small(rng)
    box, dmax = ZO.side_extents(sides, d2)
    for t in (0, 1):
        idx = np.argwhere(sides == t + 1)
        assert box[t].tolist() == [idx[:, 0].min(), idx[:, 0].max(), idx[:, 1].min(), idx[:, 1].max(), idx[:, 2].min(), idx[:, 2].max()]
        assert ZO.unkey(dmax[t]) == d2[sides == t + 1].max()
    box, dmax = ZO.side_extents(np.where(sides == 2, 0, sides))
    assert box[1].tolist() == [2 ** 31 - 1, -1] * 3 and dmax.tolist() == [0, 0] and ZO.unkey(0) == 0.0
    vals = np.array([0.0, 5e-324, 0.75, 1.0, 1e300, np.inf])
    k = ZO.key(vals)
    assert (np.diff(k.astype(object)) > 0).all() and [ZO.unkey(v) for v in k] == vals.tolist()          # key order is value order, and unkey inverts it


def test_the_depth_is_scipys_distance_to_the_filled_lungs_complement():
    ndi = pytest.importorskip("scipy.ndimage")
    lung = LO.fused_lungs((24, 20, 18), PIX).astype(np.uint8)
    lung[7:9, 9:11, 8:10] = 0                                        # a hole in the lung mask: a vessel
    for fill in (True, False):
        got = ZO.lung_distance(lung, PIX, fill)
        ref = ndi.binary_fill_holes(lung) if fill else lung != 0
        want = ndi.distance_transform_edt(ref, sampling=PIX)
        assert np.allclose(np.sqrt(got), want, rtol=1e-12, atol=0.0)          # both are one rounding away from the exact root
        assert (got[8, 10, 9] > 0) == fill


# ---- the report's rules at their edges ------------------------------------------------------------------------------------------------------------------------
def test_the_severity_rule_at_its_edges():
    from covidseg_amd import zones as Z
    lung = 400
    assert Z.severity_score(0, lung) == ZO.score_of(0, lung) == 0 and Z.severity_score(0, 0) == 0
    for pct, score in ((5, 2), (25, 3), (50, 4), (75, 5)):
        at = lung * pct // 100                                       # exactly pct per cent
        for inf, want in ((at - 1, score - 1), (at, score), (at + 1, score)):
            assert Z.severity_score(inf, lung) == ZO.score_of(inf, lung) == want, (pct, inf)
    assert Z.severity_score(1, lung) == 1 and Z.severity_score(lung, lung) == 5
    assert Z.severity_score(1, 40, (2.5,)) == 2 and Z.severity_score(1, 41, (2.5,)) == 1          # 2.5 % as the exact rational 5 / 2
    assert Z.severity_score(30, 100, (10, 30)) == 3 == ZO.score_of(30, 100, (10, 30))


def test_the_predominance_rule_at_exactly_the_threshold():
    from covidseg_amd import zones as Z
    names = ("upper", "middle", "lower")
    for f in (Z.predominant, ZO.predominant):
        assert f((5, 3, 2), names, 0.5) == "upper"                   # exactly half
        assert f((499, 301, 200), names, 0.5) == "diffuse"           # one voxel short of half
        assert f((5, 5, 0), names, 0.5) == "upper"                   # two categories at the share: the first
        assert f((0, 0, 0), names, 0.5) == "none"
        assert f((1, 2), ("peripheral", "central"), Fraction(2, 3), other="mixed") == "central"
        assert f((1, 1), ("peripheral", "central"), Fraction(2, 3), other="mixed") == "mixed"
    assert Z.predominant((3, 7), ("upper", "lower"), Fraction(3, 10)) == "upper"
    assert Z.predominant((3, 7), ("upper", "lower"), 0.1 + 0.2) == "lower"    # a float share is taken as its exact rational: 0.30000000000000004 is above 3 / 10


# ---- anatomical numbering -----------------------------------------------------------------------------------------------------------------------------------------
def _phantom(shape=(20, 16, 14)):
    lung = LO.fused_lungs(shape, PIX)
    lung[5:7, 7:9, 6:8] = 0
    sides = LO.split(lung, LO.affine_of("RAS", PIX), PIX)["sides"]
    inf = np.zeros(shape, np.uint8)
    inf[3:8, 5:9, 9:13] = 1                                          # upper (high z in RAS), one lung
    inf[12:15, 10:14, 2:5] = 1                                       # lower, the other lung, anterior (high y)
    inf[9:11, 7:9, 6:9] = 1                                          # at the junction
    inf[0:2, 0:2, 0:2] = 1                                           # outside the lungs
    return sides, inf


def _report_equal(a, b):
    for k in ("region_voxels", "shell_voxels", "side_voxels", "scores"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("outside_voxels", "total", "max_total", "bilateral", "craniocaudal", "axial", "anteroposterior"):
        assert a[k] == b[k], k
    key = lambda r: (r["side"], r["zone"], r["ap"], r["voxels_in_lung"], tuple(r["voxels_shell"].tolist()), None if np.isnan(r["depth_mm"]) else r["depth_mm"], r["subpleural"])
    assert sorted(key(r) for r in a["lesions"]) == sorted(key(r) for r in b["lesions"])          # the labelling numbers the lesions by storage order


@pytest.mark.parametrize("kw", [dict(), dict(zones=2, ap_parts=2, extent="both", depth=("mm", (3.0, 6.0, 9.0)))])
def test_the_report_does_not_depend_on_the_stored_orientation(kw):
    sides, inf = _phantom()
    canon = ZO.distribution(inf, ZO.lung_zones(sides, ("R", "A", "S"), PIX, **kw))
    assert canon["region_voxels"][..., 0].sum() == (sides != 0).sum() and canon["outside_voxels"] == int(((inf != 0) & (sides == 0)).sum()) >= 8 and canon["bilateral"]
    assert canon["region_voxels"][:, 0, :, 1].sum() > 0 and canon["region_voxels"][:, -1, :, 1].sum() > 0
    for codes in LO.all_axcodes():
        s, i = LO.reorient(sides, codes), LO.reorient(inf, codes)
        got = ZO.distribution(i, ZO.lung_zones(s, codes, LO.reorient_pixdim(PIX, codes), **kw))
        _report_equal(got, canon)


def test_zone_0_is_the_most_superior_and_ap_part_0_the_most_anterior():
    sides, _ = _phantom()
    lz = ZO.lung_zones(sides, ("R", "A", "S"), PIX, zones=3, ap_parts=2, depth=None)
    order = ZO.region_order(lz["spec"], lz["si"], lz["ap"])
    zm = lz["zone_map"]
    code = (1 + order).reshape(2, 3, 2)
    zs = [np.argwhere(zm == code[0, z, 0])[:, 2].mean() for z in range(3)]
    assert zs[0] > zs[1] > zs[2]                                     # RAS: z grows to the head
    ys = [np.argwhere(np.isin(zm, code[:, :, a]))[:, 1].mean() for a in range(2)]
    assert ys[0] > ys[1]                                             # y grows to the front


# ---- declarations, bindings, exports ------------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_bound_and_built():
    import covidseg_amd
    from covidseg_amd import _lib, zones as Z
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr)
        assert m and m.group(1).count(",") + 1 == nargs, name
        assert name in _lib._PROTOS and len(_lib._PROTOS[name][1]) == nargs and _lib._PROTOS[name][0] is _lib.i32 and name in _lib.EXPORTED_SYMBOLS
    assert "typedef struct unet_zone_spec" in text and "DESIGN.md section 4ac" in text
    import ctypes
    assert ctypes.sizeof(_lib.ZoneSpec) == 128 and _lib.ZoneSpec.r2.offset == 80 and _lib.ZoneSpec.shells.offset == 72
    for d, v in (("UNET_VOL_ZONE_MAX_PARTS", _lib.ZONE_MAX_PARTS), ("UNET_VOL_ZONE_MAX_SHELLS", _lib.ZONE_MAX_SHELLS), ("UNET_VOL_ZONE_MAX_BINS", _lib.ZONE_MAX_BINS)):
        assert re.search(rf"#define {d} {v}\b", text)
    mk = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernels_zones\.hip\b", mk, flags=re.M)
    assert os.path.exists(os.path.join(os.path.dirname(_lib.__file__), "csrc", "kernels_zones.hip"))
    for name in ("lung_zones", "lung_distribution", "LungZones", "LungDistribution"):
        assert getattr(covidseg_amd, name) is getattr(Z, name) and name in covidseg_amd.__all__
    assert "zones" in covidseg_amd.__all__
    doc = Z.lung_distribution.__doc__
    assert "LOBES" in doc and "ZONES" in doc and "NOT clinically validated" in doc


# ---- every argument error comes before a device is needed ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from covidseg_amd import volume as V

    def boom(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(V, "_ctx", boom)
    monkeypatch.setattr(V, "_mask_to_device", boom)
    monkeypatch.setattr(V, "label_device", boom)
    monkeypatch.setattr(V, "edt_sq_device", boom)
    return V


def test_lung_zones_refuses_its_arguments_before_any_device_work(no_device):
    from covidseg_amd import zones as Z
    V = no_device
    sides = np.zeros((4, 4, 4), np.uint8)
    ok = dict(orientation="LPS", pixdim=(1, 1, 1))
    with pytest.raises(ValueError, match="superior"):
        Z.lung_zones(sides, pixdim=(1, 1, 1))                        # never guessed
    with pytest.raises(ValueError, match="superior"):
        Z.lung_zones(V.LungSides(sides=sides, shape=(4, 4, 4), axcodes=None, pixdim=(1, 1, 1)))
    with pytest.raises(ValueError, match="pixdim"):
        Z.lung_zones(sides, orientation="LPS")
    for bad in (dict(zones=0), dict(zones=9), dict(zones=2.0), dict(zones=True), dict(ap_parts=0), dict(ap_parts=9), dict(extent="lobes"), dict(fill=1),
                dict(depth="mm"), dict(depth=("voxels", (1,))), dict(depth=("mm", ())), dict(depth=("mm", (1, 2, 3, 4))), dict(depth=("mm", (2.0, 1.0))),
                dict(depth=("mm", (0.0,))), dict(depth=("mm", (float("inf"),))), dict(depth=("mm", (1e200,))), dict(depth=("relative", (0.5, 1.0))),
                dict(depth=("relative", (0.5, 0.5))), dict(orientation="LPX"), dict(pixdim=(1, 0, 1))):
        with pytest.raises(ValueError):
            Z.lung_zones(sides, **{**ok, **bad})
    with pytest.raises(ValueError, match="0 / 1 / 2"):
        Z.lung_zones(np.zeros((4, 4), np.uint8), **ok)
    with pytest.raises(ValueError, match="0 / 1 / 2"):
        Z.lung_zones(np.zeros((4, 4, 4), np.float32), **ok)


def test_lung_distribution_refuses_its_arguments_before_any_device_work(no_device):
    from covidseg_amd import zones as Z
    V = no_device
    inf = np.zeros((4, 4, 4), np.uint8)
    ls = V.LungSides(sides=inf, shape=(4, 4, 4), axcodes=("L", "P", "S"), pixdim=(1.0, 1.0, 1.0))
    for bad in (dict(severity_edges=()), dict(severity_edges=(25, 5)), dict(severity_edges=(0, 5)), dict(severity_edges=(5, 101)), dict(severity_edges=("a",)),
                dict(predominance=0), dict(predominance=1.5), dict(predominance=True), dict(predominance="half"), dict(labels=inf.astype(np.int32)),
                dict(labels=inf.astype(np.int32), n=-1), dict(pixdim=(1, 1)), dict(connectivity=4)):
        with pytest.raises(ValueError):
            Z.lung_distribution(inf, ls, **bad)
    with pytest.raises(ValueError, match="LungZones"):
        Z.lung_distribution(inf, inf)
    with pytest.raises(ValueError, match="axcodes"):
        Z.lung_distribution(inf, V.LungSides(sides=inf, shape=(4, 4, 4), axcodes=None, pixdim=(1.0, 1.0, 1.0)))
    with pytest.raises(ValueError, match="the lungs"):
        Z.lung_distribution(np.zeros((4, 4, 5), np.uint8), ls)
    with pytest.raises(ValueError, match="dimensions"):
        Z.lung_distribution(np.zeros((4, 4), np.uint8), ls)


def test_segment_volume_refuses_distribution_before_any_work(no_device):
    V = no_device
    ct = np.zeros((8, 8, 4), np.int16)
    with pytest.raises(ValueError, match="per_lung"):
        V.segment_volume(ct, None, lung_mask=ct, distribution=True)
    with pytest.raises(ValueError, match="per_lung"):
        V.segment_volume_ensemble(ct, [type("Model", (), {"h": 8})()], lung_mask=ct, distribution={"zones": 2})
    for bad in ({"lobes": 5}, {"zones": 0}, {"depth": ("mm", ())}, {"severity_edges": (50, 5)}, {"predominance": 2}):
        with pytest.raises(ValueError):
            V.segment_volume(ct, None, lung_mask=ct, per_lung=True, distribution=bad)
    assert V._check_distribution(None, None) is None and V._check_distribution(False, None) is None
    kw, rep = V._check_distribution({"zones": 2, "predominance": 0.6}, {})
    assert kw == {"zones": 2} and rep == {"predominance": 0.6}

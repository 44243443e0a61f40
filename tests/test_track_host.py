"""CPU: tests/track_oracle.py against a dense contingency table, tracking.match_lesions / track_table / chain_series against the oracle on a scripted scene, the formulas and
their NaN cases, the argument checks that run before the device is touched, and the declarations of the two entry points.  Every comparison is an equality."""
import os
import re

import numpy as np
import pytest

import track_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unet_vol_label_pairs": 13, "unet_vol_track_map": 17}
AFFINE = np.array([[-0.8, 0.0, 0.0, 90.0], [0.0, 0.75, 0.0, -60.0], [0.0, 0.0, 2.5, -30.0], [0.0, 0.0, 0.0, 1.0]])


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def scripted():
    """the scene, labelled: (la, n_a, lb, n_b)"""
    ma, mb = TO.scene()
    return TO.label(ma) + TO.label(mb)


def _stats(labels, n):
    """what component_stats_device returns, as far as track_table reads it"""
    st = np.zeros(n, [("voxels", "<i8"), ("sx", "<i8"), ("sy", "<i8"), ("sz", "<i8")])
    for l in range(1, n + 1):
        sx, sy, sz, count = TO.coordinate_sums(labels, [l])
        st[l - 1] = (count, sx, sy, sz)
    return st


def _check_match(got, want):
    assert np.array_equal(got.lut_a, want["lut_a"]) and np.array_equal(got.lut_b, want["lut_b"]) and got.lut_a.dtype == np.int32
    assert got.events == want["events"] and got.n_tracks == len(want["events"])
    assert [m.tolist() for m in got.members_a] == want["members_a"] and [m.tolist() for m in got.members_b] == want["members_b"]
    for k in ("voxels_a", "voxels_b", "overlap", "size_a", "size_b"):
        assert np.array_equal(getattr(got, k), want[k]), k


@pytest.mark.parametrize("shape, n_a, n_b", [((1, 1, 1), 1, 1), ((5, 3, 2), 2, 3), ((17, 6, 5), 7, 4), ((9, 8, 7), 0, 5), ((9, 8, 7), 6, 0)])
def test_the_oracles_pairs_are_the_dense_contingency_table(shape, n_a, n_b):
    rng = np.random.default_rng(sum(shape) + n_a)
    la = rng.integers(-2, n_a + 3, shape) * (rng.random(shape) < 0.5)          # values outside 0..n on purpose
    lb = rng.integers(-2, n_b + 3, shape) * (rng.random(shape) < 0.5)
    dense = TO.dense_table(la, n_a, lb, n_b)
    p = TO.pairs(la, n_a, lb, n_b)
    want = [(a, b, int(dense[a, b])) for a in range(n_a + 1) for b in range(n_b + 1) if (a, b) != (0, 0) and dense[a, b]]
    assert p.tolist() == want                                       # sorted by (a, b), (0, 0) left out, nothing else
    assert int(p["voxels"].sum()) == int(np.count_nonzero((TO.clamp(la, n_a) != 0) | (TO.clamp(lb, n_b) != 0)))


def test_the_package_reads_a_table_as_the_oracle_sorts_it():
    from covidseg_amd import tracking as T
    rng = np.random.default_rng(3)
    la, lb = rng.integers(0, 6, (9, 7, 5)), rng.integers(0, 4, (9, 7, 5))
    keys, counts = TO.pair_table(la, 5, lb, 3)
    slots = rng.permutation(64)[:len(keys)]                         # the pairs in arbitrary slots of a table with empty ones between them
    tk, tc = np.zeros(64, np.uint64), np.full(64, -5, np.int64)
    tk[slots], tc[slots] = keys, counts
    got = T.pairs_from_table(tk, tc)
    assert got.dtype == T.PAIR_DTYPE == TO.PAIR_DTYPE and got.tolist() == TO.pairs(la, 5, lb, 3).tolist()
    assert T.first_capacity(0, 0) == 1024 and T.first_capacity(100, 154) == 1024 and T.first_capacity(100, 155) == 2048 and T.first_capacity(2 ** 31 - 1, 2 ** 31 - 1) == 2 ** 30


def test_the_scripted_scene_is_matched_as_drawn(scripted):
    from covidseg_amd import tracking as T
    la, n_a, lb, n_b = scripted
    assert (n_a, n_b) == (8, 8)
    p = TO.pairs(la, n_a, lb, n_b)
    got = T.match_lesions(p, n_a, n_b)
    _check_match(got, TO.match(p, n_a, n_b))
    assert sorted(got.events) == sorted(["persistent", "persistent", "merged", "split", "complex", "resolved", "new"])
    # the numbering: groups with a baseline lesion by their smallest a, then the follow-up-only groups
    firsts = [int(m[0]) for m in got.members_a if len(m)]
    assert firsts == sorted(firsts) and all(len(m) for m in got.members_a[:len(firsts)]) and got.events[-1] == "new" and len(got.members_a[-1]) == 0
    assert got.lut_a[0] == 0 and got.lut_b[0] == 0 and set(got.lut_a[1:]) | set(got.lut_b[1:]) == set(range(1, got.n_tracks + 1))
    by_event = {e: i for i, e in enumerate(got.events)}
    assert (len(got.members_a[by_event["merged"]]), len(got.members_b[by_event["merged"]])) == (2, 1)
    assert (len(got.members_a[by_event["split"]]), len(got.members_b[by_event["split"]])) == (1, 2)
    assert (len(got.members_a[by_event["complex"]]), len(got.members_b[by_event["complex"]])) == (2, 2)
    # the voxel counts and the sums over the tracks
    assert int(got.voxels_a.sum()) == int((la > 0).sum()) and int(got.voxels_b.sum()) == int((lb > 0).sum())
    assert int(got.overlap.sum()) == int(((la > 0) & (lb > 0)).sum())          # with every link kept no overlap crosses two tracks
    grown = [i for i, e in enumerate(got.events) if e == "persistent" and got.voxels_b[i] > got.voxels_a[i]]
    assert len(grown) == 1 and got.overlap[grown[0]] == got.voxels_a[grown[0]]
    cls_a, cls_b = T.class_tables(got)
    wa, wb = TO.class_tables(TO.match(p, n_a, n_b))
    assert np.array_equal(cls_a, wa) and np.array_equal(cls_b, wb) and cls_a.dtype == np.uint8
    assert sorted(set(cls_a[1:])) == [1, 2] and sorted(set(cls_b[1:])) == [4, 5]


def test_the_track_table_follows_the_stated_formulas(scripted):
    from covidseg_amd import tracking as T, volume as V
    la, n_a, lb, n_b = scripted
    grid = V.Grid(la.shape, AFFINE)
    want = TO.track(la, n_a, lb, n_b, AFFINE, interval_days=90)
    m = T.match_lesions(TO.pairs(la, n_a, lb, n_b), n_a, n_b)
    rows = T.track_table(m, _stats(la, n_a), _stats(lb, n_b), grid, interval_days=90)
    assert rows.dtype == T.TRACK_DTYPE and len(rows) == len(want["rows"])
    for got, w in zip(rows, want["rows"]):
        for k in T.TRACK_DTYPE.names:
            assert (got[k] == w[k]) if k == "event" else _same(got[k], w[k]), (k, got[k], w[k])
    ev = T.event_summary(rows)
    assert {e: v["count"] for e, v in ev.items()} == {"persistent": 2, "merged": 1, "split": 1, "complex": 1, "new": 1, "resolved": 1}
    assert sum(v["ml_a"] for v in ev.values()) == pytest.approx(float((la > 0).sum()) * grid.voxel_ml, rel=1e-12)
    new, res = rows[rows["event"] == "new"][0], rows[rows["event"] == "resolved"][0]
    assert np.isnan(new["change_pct"]) and np.isnan(new["shift_mm"]) and np.isnan(new["doubling_time_days"]) and np.isnan(new["xa"]) and new["dice"] == 0.0
    assert res["change_pct"] == -100.0 and np.isnan(res["shift_mm"]) and np.isnan(res["doubling_time_days"]) and np.isnan(res["xb"])
    stable = [r for r in rows if r["event"] == "persistent" and r["voxels_a"] == r["voxels_b"]][0]
    assert stable["dice"] == 1.0 and stable["change_pct"] == 0.0 and stable["shift_mm"] == 0.0 and np.isnan(stable["doubling_time_days"])
    assert np.isnan(T.track_table(m, _stats(la, n_a), _stats(lb, n_b), grid)["doubling_time_days"]).all()          # no interval, no doubling time


def test_the_formulas_on_hand_numbers():
    f = TO.formulas(1000, 1400, 900, 0.002, interval_days=60)
    assert f["change_pct"] == 100.0 * 400 / 1000 and f["dice"] == 1800.0 / 2400 and f["change_ml"] == 400 * 0.002
    assert f["doubling_time_days"] == 60.0 * np.log(2.0) / np.log(1.4) and 123.0 < f["doubling_time_days"] < 124.0
    assert TO.formulas(1000, 500, 500, 0.002, interval_days=30)["doubling_time_days"] == -30.0          # a halving time
    assert np.isnan(TO.formulas(0, 5, 0, 1.0, 30)["change_pct"]) and np.isnan(TO.formulas(5, 5, 5, 1.0, 30)["doubling_time_days"])
    assert np.isnan(TO.formulas(5, 0, 0, 1.0, 30)["doubling_time_days"]) and np.isnan(TO.formulas(5, 9, 3, 1.0)["doubling_time_days"])
    assert TO.centroid(AFFINE, 10, 20, 30, 10) == (90.0 - 0.8, -60.0 + 1.5, -30.0 + 7.5) and np.isnan(TO.centroid(AFFINE, 0, 0, 0, 0)).all()


def test_each_threshold_cuts_a_link():
    from covidseg_amd import tracking as T
    # lesion 1 of a (100 voxels) meets lesion 1 of b (80 voxels) in 3 voxels; lesion 2 of a meets lesion 2 of b in 50
    p = np.array([(0, 1, 77), (0, 2, 10), (1, 0, 97), (1, 1, 3), (2, 0, 5), (2, 2, 50)], T.PAIR_DTYPE)
    assert T.match_lesions(p, 2, 2).events == ("persistent", "persistent")
    for kw in (dict(min_overlap_voxels=4), dict(min_fraction=0.05)):          # 3 < 4; 3 < 0.05 * min(100, 80) = 4
        got = T.match_lesions(p, 2, 2, **kw)
        _check_match(got, TO.match(p, 2, 2, **kw))
        assert got.events == ("resolved", "persistent", "new") and got.lut_a.tolist() == [0, 1, 2] and got.lut_b.tolist() == [0, 3, 2]
        assert got.overlap.tolist() == [0, 50, 0] and len(got.links) == 1          # the three shared voxels belong to no track's overlap
    for kw in (dict(min_overlap_voxels=3), dict(min_fraction=3 / 80)):         # exactly on the threshold: kept
        assert T.match_lesions(p, 2, 2, **kw).events == ("persistent", "persistent")
    assert T.match_lesions(np.zeros(0, T.PAIR_DTYPE), 0, 0).n_tracks == 0
    lone = T.match_lesions(np.array([(1, 0, 4)], T.PAIR_DTYPE), 1, 0)
    assert lone.events == ("resolved",) and lone.lut_b.tolist() == [0]


def _series_scene():
    """three time points: lesion A persists throughout; B and C are apart at t0, t1 and merge at t2; D is there at t1 only; E appears at t2"""
    shape = (40, 12, 8)
    t = [np.zeros(shape, np.uint8) for _ in range(3)]
    for m in t:
        m[2:6, 2:6, 2:6] = 1                                        # A
    t[0][10:14, 2:6, 2:6] = 1; t[0][17:21, 2:6, 2:6] = 1           # B, C
    t[1][10:15, 2:6, 2:6] = 1; t[1][16:21, 2:6, 2:6] = 1
    t[2][10:21, 2:6, 2:6] = 1                                       # merged
    t[1][26:29, 2:5, 2:5] = 1                                       # D
    t[2][33:36, 2:5, 2:5] = 1                                       # E
    return t


def test_a_series_of_three_time_points_is_chained_as_the_oracle_chains_it():
    from covidseg_amd import tracking as T
    labelled = [TO.label(m) for m in _series_scene()]
    sizes = [np.bincount(l.reshape(-1), minlength=n + 1).astype(np.int64) for l, n in labelled]
    pairs = [TO.pairs(labelled[s][0], labelled[s][1], labelled[s + 1][0], labelled[s + 1][1]) for s in range(2)]
    got = T.chain_series([T.match_lesions(pairs[s], labelled[s][1], labelled[s + 1][1]) for s in range(2)], sizes)
    want = TO.chain([TO.match(pairs[s], labelled[s][1], labelled[s + 1][1]) for s in range(2)], sizes)
    assert all(np.array_equal(g, w) for g, w in zip(got[0], want[0])) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]
    lineage_of, voxels, first, last, events = got
    assert len(voxels) == 4 and voxels[:, 0].tolist() == [64, 128, 0, 0]          # A; B + C (one lineage: they merge at t2); D; E
    assert first.tolist() == [0, 0, 1, 2] and last.tolist() == [2, 2, 1, 2]
    assert events == [["persistent", "persistent"], ["persistent", "merged"], ["new", "resolved"], ["", "new"]]
    assert lineage_of[0].tolist() == [0, 1, 2, 2] and lineage_of[2].tolist() == [0, 1, 2, 4]
    with pytest.raises(ValueError):
        T.chain_series([], sizes)


def test_argument_errors_come_before_the_device_is_touched():
    from covidseg_amd import tracking as T, volume as V
    g = V.Grid((4, 4, 4), AFFINE)
    bare = V.Grid((4, 4, 4), np.diag([1.0, 1.0, 1.0, 1.0]), oriented=False)
    m = np.zeros((4, 4, 4), np.uint8)
    for call in (lambda: T.track_lesions(m, bare, m, g), lambda: T.track_lesions(m, g, m, bare), lambda: T.track_lesions(m, g, m, (4, 4, 4)),
                 lambda: T.track_lesions(m, g, m, g, connectivity=4), lambda: T.track_lesions(m, g, m, g, min_overlap_voxels=0),
                 lambda: T.track_lesions(m, g, m, g, min_overlap_voxels=1.5), lambda: T.track_lesions(m, g, m, g, min_fraction=1.5),
                 lambda: T.track_lesions(m, g, m, g, min_fraction=-0.1), lambda: T.track_lesions(m, g, m, g, interval_days=0),
                 lambda: T.track_lesions(m, g, m, g, interval_days=float("nan")), lambda: T.track_lesions(np.zeros((4, 4, 5), np.uint8), g, m, g),
                 lambda: T.track_lesions(m.astype(np.float32), g, m, g),
                 lambda: T.track_series([m, m], [g, g]), lambda: T.track_series([m, m, m], [g, g]), lambda: T.track_series([m, m, m], [g, g, bare]),
                 lambda: T.track_series([m, m, m], [g, g, g], transforms=[None, None]), lambda: T.track_series([m, m, m], [g, g, g], min_fraction=2),
                 lambda: T.label_pairs(m, -1, m, 0), lambda: T.label_pairs(m, 2 ** 31, m, 0), lambda: T.label_pairs(m, 1, m[:3], 1), lambda: T.label_pairs(m[0], 1, m[0], 1),
                 lambda: T.label_pairs(m.astype(np.float64), 1, m, 1), lambda: T.label_pairs(m, 1, m, 1, shape=(4, 4, 5)),
                 lambda: T.match_lesions(np.zeros(3), 1, 1), lambda: T.match_lesions(np.array([(2, 0, 1)], T.PAIR_DTYPE), 1, 1),
                 lambda: T.match_lesions(np.zeros(0, T.PAIR_DTYPE), 1, 1, min_overlap_voxels=0)):
        with pytest.raises(ValueError):
            call()


def test_the_new_entries_are_declared_and_bound():
    import covidseg_amd
    from covidseg_amd import _lib, tracking as T, volume as V
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/unet_hip.h"
        assert m.group(1).count(",") + 1 == nargs
        assert name in _lib._PROTOS and len(_lib._PROTOS[name][1]) == nargs and _lib._PROTOS[name][0] is _lib.i32 and name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 16 and "#define UNET_ABI_VERSION 16" in text
    defines = {k: int(v) for k, v in re.findall(r"#define (UNET_VOL_PAIRS_\w+|UNET_TRACK_CLS_\w+) (\d+)", text)}
    assert defines["UNET_VOL_PAIRS_CHUNK"] == _lib.PAIRS_CHUNK and defines["UNET_VOL_PAIRS_LDS_SLOTS"] == _lib.PAIRS_LDS_SLOTS and _lib.PAIRS_LDS_SLOTS < _lib.PAIRS_CHUNK
    assert [defines["UNET_TRACK_CLS_" + n] for n in ("NONE", "RESOLVED", "SHRINKAGE", "BOTH", "GROWTH", "NEW")] == [0, 1, 2, 3, 4, 5]
    assert (T.CLS_RESOLVED, T.CLS_SHRINKAGE, T.CLS_BOTH, T.CLS_GROWTH, T.CLS_NEW) == (TO.CLS_RESOLVED, TO.CLS_SHRINKAGE, TO.CLS_BOTH, TO.CLS_GROWTH, TO.CLS_NEW) == (1, 2, 3, 4, 5)
    mk = open(os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernels_track\.hip\b", mk, flags=re.M)
    assert not re.search(r"kernels_track\.o[^\n]*EXTRA", mk)          # no floating point in the file: no -ffp-contract entry
    for name in ("track_lesions", "track_series", "label_pairs", "match_lesions", "LesionTracking", "LesionSeries", "LesionMatch", "PALETTE_CHANGE"):
        assert getattr(covidseg_amd, name) is getattr(T, name) and name in covidseg_amd.__all__
    assert "tracking" in covidseg_amd.__all__
    assert T.PALETTE_CHANGE.dtype == np.uint8 and T.PALETTE_CHANGE.shape == (6, 3) and len({tuple(c) for c in T.PALETTE_CHANGE}) == 6
    assert V.Layer(np.zeros((2, 2, 2), np.uint8), T.PALETTE_CHANGE).palette is not None
    assert len(T.CLASS_NAMES) == 6 and T.EVENTS == ("persistent", "merged", "split", "complex", "new", "resolved")

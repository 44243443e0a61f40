"""CPU: tests/lungside_oracle.py on phantoms with a known answer and against scipy.ndimage, the new entries' declarations and bindings, and every argument error of
volume.split_lungs / lung_burden / segment_volume(per_lung=), which must be raised before a device is needed."""
import os
import re

import numpy as np
import pytest

import lungside_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unet_vol_side_assign": 12, "unet_vol_side_table": 12}
LPS = LO.affine_of("LPS")                                            # voxel x grows to the patient's left: low x is the patient's right
RAS = LO.affine_of("RAS")
A, B = ((2, 9), (2, 10), (2, 8)), ((13, 20), (2, 10), (2, 8))        # two boxes in a 22 x 12 x 10 volume, 4 voxels apart along x


def _bridge(thick):
    """the boxes joined along x by a bar of thick x thick voxels (away from every face of the volume)"""
    return LO.boxes((22, 12, 10), A, B, ((9, 13), (5, 5 + thick), (4, 4 + thick)))


@pytest.mark.parametrize("thick, radius", [(1, 1.0), (2, 1.0), (3, 2.0)])
def test_a_bridge_goes_at_the_radius_its_thickness_implies(thick, radius):
    """Erosion by r removes the voxels whose distance to the background is <= r.  At pixdim 1 a voxel of a bar 1 or 2 voxels thick has a background neighbour (distance
    1): the bar goes at r = 1.  The centre line of a bar 3 thick is 2 voxels from the background: it survives r = 1 and goes at r = 2.  The boxes (7 x 8 x 6) keep a
    core at both radii."""
    m = _bridge(thick)
    got = LO.split(m, LPS)
    assert got["radius_mm"] == radius
    sides = got["sides"]
    assert np.array_equal(sides != 0, m != 0)
    assert (sides[A[0][0]:A[0][1], A[1][0]:A[1][1], A[2][0]:A[2][1]] == 2).all()          # LPS: the low-x box is the patient's right
    assert (sides[B[0][0]:B[0][1], B[1][0]:B[1][1], B[2][0]:B[2][1]] == 1).all()
    core = lambda box, r: int(np.prod([hi - lo - 2 * r for lo, hi in box]))
    left, right = got["seed_voxels"]                                 # the eroded box, and the few face voxels the bar's foot shields from the background
    assert left == right and core(B, int(radius)) < left <= core(B, int(radius)) + int(radius) * thick * thick
    flipped = LO.split(m, RAS)                                       # the same storage read the other way round: left and right swap
    assert np.array_equal(flipped["sides"], np.where(sides == 0, 0, 3 - sides))


def test_two_separate_blobs_need_no_erosion_and_one_blob_cannot_be_split():
    m = LO.boxes((22, 12, 10), A, B)
    got = LO.split(m, LPS)
    assert got["radius_mm"] == 0.0 and got["seed_voxels"] == (7 * 8 * 6, 7 * 8 * 6) == got["voxels"]
    one = LO.boxes((22, 12, 10), A, A)
    with pytest.raises(LO.SplitError, match="336 and 0"):
        LO.split(one, LPS)
    small = one.copy(); small[15:17, 3:5, 3:5] = 1                   # a second component below min_ratio of the first
    with pytest.raises(LO.SplitError, match="336 and 8"):
        LO.split(small, LPS)
    assert LO.split(small, LPS, min_ratio=8 / 336)["radius_mm"] == 0.0
    with pytest.raises(LO.SplitError, match="same world x"):
        LO.split(m, LO.affine_of("ARS"))                             # the boxes differ along voxel x only, which this orientation calls anterior


def test_a_tie_goes_to_the_patients_left_in_either_storage_order():
    ras_like = np.zeros((23, 12, 10), np.uint8)                      # an odd extent: the plane x = 11 is equidistant from two mirrored boxes joined by a bar
    ras_like[2:9] = 1; ras_like[14:21] = 1; ras_like[9:14, 5, 4] = 1; ras_like[11, 2:10, 2:8] = 1
    ras_like[:, :2] = 0; ras_like[:, 10:] = 0; ras_like[:, :, :2] = 0; ras_like[:, :, 8:] = 0
    for affine, left_is_low_x in ((RAS, True), (LPS, False)):
        got = LO.split(ras_like, affine)
        d2l, d2r = got["d2_left"], got["d2_right"]
        tie = (ras_like != 0) & (d2l == d2r)
        assert tie[11].sum() >= 48 and not tie[:11].any() and not tie[12:].any()
        assert (got["sides"][tie] == 1).all()                        # <=: the tie is the left lung's
        assert (got["sides"][:11][ras_like[:11] != 0] == (1 if left_is_low_x else 2)).all()
    s, c = LO.side_assign(np.ones(4), np.array([1.0, 2.0, 2.0, np.inf]), np.array([2.0, 2.0, 1.0, np.inf]), 1, 2)
    assert s.tolist() == [1, 1, 2, 1] and c.tolist() == [0, 3, 1]
    s, c = LO.side_assign(np.ones(4), np.array([1.0, 2.0, 2.0, np.inf]), np.array([2.0, 2.0, 1.0, np.inf]), 2, 1)          # seed b is the left one now
    assert s.tolist() == [2, 1, 1, 1] and c.tolist() == [0, 3, 1]


def test_the_oracles_pieces_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    pixdim = (0.75, 0.75, 2.5)
    m = LO.fused_lungs((48, 40, 12), pixdim)
    for r in (0, 1, 2, 3):
        cand = m if r == 0 else LO.MO.erode_mm(m, r, pixdim)
        assert np.array_equal(cand != 0, ndi.distance_transform_edt(m != 0, sampling=pixdim) > r) or r == 0
        for c in (1, 2, 3):
            lab, n = LO.CO.label(cand, c)
            want, wn = ndi.label(cand, ndi.generate_binary_structure(3, c))
            assert n == wn and np.array_equal(lab, want)
    got = LO.split(m, LPS, pixdim)
    assert got["radius_mm"] > 0
    r, lab, ab, st = LO.seeds(m, pixdim)
    for k, d2 in zip(sorted(ab, key=lambda k: LO.world_x(LPS, st, k)), (got["d2_left"], got["d2_right"])):
        want = ndi.distance_transform_edt(lab != k + 1, sampling=pixdim) ** 2
        assert np.allclose(d2, want, rtol=4 * 2.0 ** -52, atol=0.0)          # sqrt and its square: two roundings of a value this oracle holds exactly
    cx = ndi.center_of_mass(lab == ab[0] + 1)
    assert np.isclose(LO.world_x(LPS, st, ab[0]), -cx[0])
    # the split itself, restated with scipy alone
    sides = np.where(m != 0, np.where(ndi.distance_transform_edt(got["d2_left"] != 0, sampling=pixdim) <= ndi.distance_transform_edt(got["d2_right"] != 0, sampling=pixdim), 1, 2), 0)
    assert (sides != got["sides"]).sum() <= (got["d2_left"] == got["d2_right"]).sum() + 4          # (scipy's rounded distances may break an exact tie either way)


def test_side_table_and_burden_on_a_known_case():
    sides = np.zeros((6, 4, 3), np.uint8); sides[:3, :, :2] = 1; sides[3:, :, :2] = 2
    inf = np.zeros_like(sides); inf[1:5, 1, 0] = 1; inf[0, 3, 2] = 1; inf[5, 0, 1] = 7
    lab, n = LO.CO.label(inf)
    totals, les, ps = LO.side_table(sides, inf, lab, n)
    assert totals.tolist() == [[24, 24, 24], [1, 2, 3]]
    assert n == 3 and sorted(les.tolist()) == sorted([[0, 2, 2], [1, 0, 0], [0, 0, 1]])
    assert ps.tolist() == [[12, 12, 0, 2, 2, 0], [12, 12, 0, 0, 1, 0], [0, 0, 1, 0, 0, 0]]
    b = LO.burden(inf, sides, pixdim=(1.0, 2.0, 5.0))
    assert b["left"] == {"lung_ml": 0.24, "infected_ml": 0.02, "fraction": 0.02 / 0.24} and b["right"]["infected_ml"] == 0.03 and b["outside_ml"] == 0.01
    assert sorted(b["side"].tolist()) == ["left", "none", "right"] and b["bilateral"]
    t, l, p = LO.side_table(np.full((2, 2, 1), 9, np.uint8), None, np.array([[[5], [1]], [[-1], [2]]]), 2)          # side values above 2 count as 0; labels outside 1..n are ignored
    assert t.tolist() == [[4, 0, 0], [0, 0, 0]] and l.tolist() == [[1, 0, 0], [1, 0, 0]] and p.tolist() == [[0] * 6]
    e = LO.burden(np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8))
    assert np.isnan(e["left"]["fraction"]) and np.isnan(e["right"]["fraction"]) and not e["bilateral"] and len(e["side"]) == 0


def test_reorientation_round_trips():
    rng = np.random.default_rng(0)
    v = rng.integers(0, 100, (5, 4, 3))
    for codes in LO.all_axcodes():
        w = LO.reorient(v, codes)
        assert np.array_equal(LO.to_canonical(w, codes), v)
        assert w.shape == tuple(v.shape[k] for k in [[i for i, p in enumerate(LO.LETTERS) if c in p][0] for c in codes])
    assert np.array_equal(LO.reorient(v, "RAS"), v) and np.array_equal(LO.reorient(v, "LAS"), v[::-1])


def test_the_new_entries_are_declared_and_bound():
    import covidseg_amd
    from covidseg_amd import _lib, nifti_min, volume as V
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/unet_hip.h"
        assert m.group(1).count(",") + 1 == nargs
        assert name in _lib._PROTOS, f"{name} is not bound in _lib._PROTOS"
        assert len(_lib._PROTOS[name][1]) == nargs and _lib._PROTOS[name][0] is _lib.i32
        assert name in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 16 and "#define UNET_ABI_VERSION 16" in text
    mk = open(os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernels_lungside\.hip\b", mk, flags=re.M)
    assert "ASAN_OBJS = $(addprefix $(ASAN_DIR)/,$(OBJS))" in mk and "UBSAN_OBJS = $(addprefix $(UBSAN_DIR)/,$(OBJS))" in mk          # the sanitizer rules take every source
    for name in ("split_lungs", "lung_burden", "LungSides", "LungBurden", "LungSplitError"):
        assert getattr(covidseg_amd, name) is getattr(V, name) and name in covidseg_amd.__all__
    for name in ("side_assign_device", "side_table_device", "burden_from_tables"):
        assert callable(getattr(V, name))
    assert issubclass(V.LungSplitError, ValueError)
    assert V.LUNG_MIN_RATIO == LO.MIN_RATIO and V.LUNG_ERODE_MM == LO.ERODE_MM
    assert [nifti_min.AXIS_LETTERS[k] for k in range(3)] == list(LO.LETTERS)
    for codes in LO.all_axcodes():
        assert np.array_equal(nifti_min.affine_from_axcodes(codes, (0.5, 0.75, 2.5)), LO.affine_of(codes, (0.5, 0.75, 2.5)))


class _NoModel:
    h = 64

    def predict(self, *a, **k):
        raise AssertionError("the model must not be reached")


def test_argument_errors_need_no_device(tmp_path):
    from covidseg_amd import nifti_min, volume as V
    m = LO.boxes((22, 12, 10), A, B)
    with pytest.raises(V.LungSplitError, match="orientation"):       # a bare array carries no orientation: left and right are not guessed
        V.split_lungs(m)
    p = tmp_path / "lung.nii"
    nifti_min.write(p, m)
    with pytest.raises(V.LungSplitError, match="orientation"):       # nor does a file without qform / sform
        V.split_lungs(p)
    bad = [dict(orientation="RAR"), dict(orientation="XYZ"), dict(orientation="RA"), dict(orientation=("R", "A", "A")), dict(orientation=np.eye(3)),
           dict(orientation=np.zeros((4, 4))), dict(orientation=5),
           dict(erode_mm=(3, 2, 1)), dict(erode_mm=(1, 1)), dict(erode_mm=(0, 1)), dict(erode_mm=(-1,)), dict(erode_mm=(1, np.inf)), dict(erode_mm=3),
           dict(min_ratio=0), dict(min_ratio=1.5), dict(min_ratio="x"), dict(min_ratio=float("nan")),
           dict(connectivity=4), dict(pixdim=(1, 1)), dict(pixdim=(1, 0, 1))]
    for kw in bad:
        kw.setdefault("orientation", "LPS")
        with pytest.raises(ValueError) as e:
            V.split_lungs(m, **kw)
        assert not isinstance(e.value, V.LungSplitError), kw
    with pytest.raises(ValueError):
        V.split_lungs(m.astype(np.float32)[0], orientation="LPS")    # not a volume
    ct = np.zeros((22, 12, 10), np.int16)
    for call in (V.segment_volume, lambda c, mdl, **kw: V.segment_volume_ensemble(c, [mdl], **kw)):
        with pytest.raises(ValueError, match="lung_mask"):
            call(ct, _NoModel(), per_lung=True)
        with pytest.raises(ValueError, match="lung_mask"):
            call(ct, _NoModel(), per_lung={"orientation": "LPS"})
        for per_lung in ({"erode_mm": (2, 1)}, {"orientation": "RAR"}, {"shape": (1, 2, 3)}, {"return_device": True}, {"min_ratio": 2}):
            with pytest.raises(ValueError):
                call(ct, _NoModel(), lung_mask=m, per_lung=per_lung)
    assert V._check_per_lung(None, None) is None and V._check_per_lung(False, None) is None and V._check_per_lung(True, m) == {}
    assert V._check_per_lung({"orientation": "LPS"}, m) == {"orientation": "LPS"}
    inf = np.zeros((22, 12, 10), np.uint8)
    for kw in (dict(sides=np.zeros((22, 12, 9), np.uint8)), dict(sides=np.zeros((22, 12, 10), np.float32)), dict(sides=m, labels=inf.astype(np.int32)),
               dict(sides=m, labels=inf.astype(np.int32), n=-1), dict(sides=m, pixdim=(1, 1)), dict(sides=m, connectivity=0)):
        with pytest.raises(ValueError):
            V.lung_burden(inf, **kw)
    with pytest.raises(ValueError):
        V.lung_burden(inf.astype(np.float64), m)
    b = V.burden_from_tables(np.array([[24, 24, 24], [1, 2, 3]]), np.array([[0, 2, 2], [1, 0, 0], [0, 0, 1], [0, 1, 2]]), np.zeros((3, 6), np.int64), (1.0, 2.0, 5.0))
    assert b.lesions.dtype == V.LUNG_LESION_DTYPE and b.lesions["side"].tolist() == ["left", "none", "right", "right"] and b.lesions["label"].tolist() == [1, 2, 3, 4]
    assert b.left.lung_ml == 0.24 and b.left.fraction == 0.02 / 0.24 and b.right.infected_ml == 0.03 and b.outside_ml == 0.01 and b.bilateral
    e = V.burden_from_tables(np.zeros((2, 3), np.int64), np.zeros((0, 3), np.int64), np.zeros((1, 6), np.int64))
    assert np.isnan(e.left.fraction) and not e.bilateral and len(e.lesions) == 0

"""CPU: the volume score's host side -- tests/volscore_oracle.py against itself (brute force == line scan, bit for bit), against scipy.ndimage where it imports,
on hand-made cases with known answers, and the new entries' bindings."""
import math
import os
import re

import numpy as np
import pytest

import components_oracle as CO
import volscore_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACINGS = [(1.0, 1.0, 1.0), (0.7, 0.7, 1.25), (0.68359375, 0.68359375, 5.0), (0.3, 0.7, 1.1)]
ENTRIES = {"unet_vol_confusion": 8, "unet_vol_surface": 9, "unet_vol_edt_ws_bytes": 3, "unet_vol_edt_sq": 11, "unet_vol_sqrt_f64": 4, "unet_vol_surface_distances": 12,
           "unet_vol_lesion_overlap": 11}
ULP = 2.0 ** -53


@pytest.mark.parametrize("pixdim", SPACINGS)
def test_brute_force_equals_the_line_scan(pixdim):
    for seed, (shape, density) in enumerate([((9, 7, 5), 0.05), ((13, 1, 11), 0.3), ((1, 1, 1), 1.0), ((6, 10, 8), 0.6), ((12, 12, 3), 0.01)]):
        m = CO.random_mask(shape, density, seed)
        for nonzero in (True, False):
            a, b = SO.edt_sq_brute(m, nonzero, pixdim), SO.edt_sq_lines(m, nonzero, pixdim)
            assert a.dtype == np.float64 and np.array_equal(a, b), (shape, nonzero)
    none = np.zeros((4, 3, 2), np.uint8)
    assert np.isinf(SO.edt_sq_lines(none, True, pixdim)).all() and np.isinf(SO.edt_sq_brute(none, True, pixdim)).all()
    assert not SO.edt_sq_lines(none, False, pixdim).any()


def test_the_distance_transform_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for seed, shape in enumerate([(24, 17, 9), (11, 30, 6)]):
        m = CO.ellipsoids(shape, 3, 0.02, seed) | CO.random_mask(shape, 0.2, seed)
        m[0, 0, 0] = 0                                               # scipy needs a background voxel
        for pixdim in SPACINGS:
            got = np.sqrt(SO.edt_sq_lines(m, False, pixdim))
            want = ndi.distance_transform_edt(m != 0, sampling=pixdim)
            if pixdim in SPACINGS[:1] + SPACINGS[2:3]:               # unit and dyadic spacing: every product is exact, so the order of the sum does not matter
                assert np.array_equal(got, want), pixdim
            else:                                                    # scipy adds the three products in another order: 2 ulp expected, 4 the margin
                rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
                print(f"edt against scipy, spacing {pixdim}: worst relative difference {rel.max():.3g}")
                assert rel.max() <= 4 * ULP, pixdim


def test_the_surface_against_scipy_erosion():
    ndi = pytest.importorskip("scipy.ndimage")
    masks = [CO.random_mask((14, 9, 11), 0.7, 1), CO.ellipsoids((30, 22, 12), 4, 0.01, 2), np.ones((5, 6, 7), np.uint8), np.zeros((3, 3, 3), np.uint8)]
    touching = np.zeros((12, 10, 8), np.uint8); touching[:, 2:8, 1:7] = 1; touching[3:9, :, 2:6] = 1; touching[4:8, 3:7, :] = 1          # reaches all six faces
    masks.append(touching)
    for m in masks:
        for c in (1, 2, 3):
            want = (m != 0) ^ ndi.binary_erosion(m != 0, ndi.generate_binary_structure(3, c))
            got = SO.surface(m, c)
            assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8)), (m.shape, c)
    assert np.array_equal(SO.surface(np.ones((5, 6, 7), np.uint8), 1)[1:-1, 1:-1, 1:-1], np.zeros((3, 4, 5), np.uint8))


def test_two_voxels_k_apart():
    for pixdim in SPACINGS:
        for axis in range(3):
            for k in (1, 4, 9):
                a = np.zeros((13, 13, 13), np.uint8); b = a.copy()
                p = [2, 3, 1]; a[tuple(p)] = 1
                p[axis] += k; b[tuple(p)] = 1
                s = SO.score(a, b, pixdim)
                want = float(np.sqrt(np.float64(pixdim[axis]) ** 2 * (k * k)))
                assert s["hd"] == s["hd_pred_to_truth"] == s["hd_truth_to_pred"] == s["hd95"] == s["assd"] == want
                assert math.isclose(want, k * pixdim[axis], rel_tol=2 * ULP)
                assert (s["tp"], s["fp"], s["fn"]) == (0, 1, 1) and s["dice"] == 0.0 and s["n_surface_pred"] == 1
                assert s["lesion_recall"] == 0.0 and s["lesion_precision"] == 0.0 and s["missed_lesions"] == 1 and s["false_positive_lesions"] == 1


def test_cube_against_itself_and_against_its_shift():
    a = np.zeros((20, 18, 16), np.uint8); a[4:12, 5:13, 3:11] = 1
    s = SO.score(a, a, (0.7, 0.7, 1.25))
    assert s["dice"] == 1.0 and s["iou"] == 1.0 and s["fp"] == s["fn"] == 0 and s["tp"] == 512 and s["volume_error_ml"] == 0.0
    assert s["hd"] == s["hd95"] == s["assd"] == 0.0 and s["n_surface_pred"] == s["n_surface_truth"] == 8 ** 3 - 6 ** 3
    assert s["lesion_recall"] == 1.0 and s["lesion_precision"] == 1.0 and s["cover_t"].tolist() == [512]
    b = np.roll(a, 1, axis=0)
    s = SO.score(a, b, (2.0, 1.0, 1.0))
    assert (s["tp"], s["fp"], s["fn"]) == (7 * 64, 64, 64) and s["dice"] == 2 * 448 / 1024 and s["iou"] == 448 / 576
    assert s["precision"] == s["recall"] == 448 / 512
    assert s["hd"] == 2.0 and s["hd_pred_to_truth"] == 2.0 and s["hd_truth_to_pred"] == 2.0          # a face moved by one voxel of 2 mm along x
    assert 0.0 < s["assd"] < 2.0 and s["hd95"] == 2.0
    assert np.isnan(s["per_slice_dice"][0]) and s["per_slice_dice"][5] == 2 * 56 / 128 and s["pred_ml"] == 512 * 2.0 / 1000.0


def test_empty_mask_conventions():
    z = np.zeros((6, 5, 4), np.uint8); m = z.copy(); m[2:4, 1:3, 1:3] = 1
    s = SO.score(z, z)
    assert s["dice"] == 1.0 and s["iou"] == 1.0 and math.isnan(s["precision"]) and math.isnan(s["recall"])
    assert all(s[k] == 0.0 for k in ("hd", "hd95", "assd", "asd_pred_to_truth", "hd_truth_to_pred")) and np.isnan(s["per_slice_dice"]).all()
    assert math.isnan(s["lesion_recall"]) and math.isnan(s["lesion_precision"])
    for pred, truth in ((z, m), (m, z)):
        s = SO.score(pred, truth)
        assert s["dice"] == 0.0 and all(s[k] == float("inf") for k in ("hd", "hd95", "assd", "asd_pred_to_truth", "hd_truth_to_pred"))
    s = SO.score(z, m)
    assert s["recall"] == 0.0 and math.isnan(s["precision"]) and s["lesion_recall"] == 0.0 and math.isnan(s["lesion_precision"]) and s["missed_lesions"] == 1


def test_lesion_cover_and_min_overlap():
    t = np.zeros((16, 8, 4), np.uint8); p = t.copy()
    t[1:4, 1:4, 1:3] = 1; t[8:12, 2:6, 0:2] = 1; t[14, 7, 3] = 1
    p[3:6, 1:4, 1:3] = 1; p[8:12, 2:6, 0:2] = 1; p[0, 7, 0] = 1
    c = SO.lesion_cover(p, t, 1, 1)
    assert c["n_t"] == 3 and c["n_p"] == 3 and c["cover_t"].tolist() == [6, 32, 0] and c["cover_p"].tolist() == [0, 6, 32]
    assert c["lesion_recall"] == 2 / 3 and c["lesion_precision"] == 2 / 3 and c["missed_lesions"] == 1 and c["false_positive_lesions"] == 1
    c = SO.lesion_cover(p, t, 1, 7)
    assert c["detected"].tolist() == [False, True, False] and c["lesion_recall"] == 1 / 3


def test_sum_chain_follows_the_documented_shape():
    assert SO.sum_chain(1) == 16 + 1 + 18 and SO.sum_chain(256 * 16 * 4096) == 16 + 16 + 18 and SO.sum_chain(512 * 512 * 301) == 16 * 5 + 16 + 18
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    assert "#define UNET_VOL_SURFDIST_WS_BYTES 32768" in hdr and "16 ceil(items / (256 G)) + ceil(G / 256) + 18" in hdr


def test_the_new_entries_are_bound_and_public():
    from covidseg_amd import _lib, volume as V
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/unet_hip.h"
        assert m.group(1).count(",") + 1 == nargs
        assert name in _lib._PROTOS, f"{name} is not bound in _lib._PROTOS"
        assert len(_lib._PROTOS[name][1]) == nargs
    assert _lib.ABI_VERSION == 16 and "#define UNET_ABI_VERSION 16" in text
    m = re.search(r"#define UNET_VOL_EDT_MAX_DIM (\d+)", text)
    assert m and int(m.group(1)) >= 2048 and int(m.group(1)) == V.EDT_MAX_DIM
    for name in ("score_volume", "surface", "distance_transform", "VolumeScore"):
        assert callable(getattr(V, name))
    pkg = os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc")
    mk = open(os.path.join(pkg, "Makefile")).read()
    assert "kernels_volscore.hip" in mk and re.search(r"kernels_volscore\.o[^\n]*: EXTRA = -ffp-contract=off", mk)
    assert "asm" not in re.sub(r"//[^\n]*", "", open(os.path.join(pkg, "kernels_volscore.hip")).read())


def test_score_equality_and_refusals_that_need_no_device():
    from covidseg_amd import volume as V
    a = V.VolumeScore(dice=0.5, hd=float("nan"), t=np.array([1.0, np.nan]), tab=np.zeros(2, V.SCORED_LESION_DTYPE["truth"]), none=None)
    b = V.VolumeScore(dice=0.5, hd=float("nan"), t=np.array([1.0, np.nan]), tab=np.zeros(2, V.SCORED_LESION_DTYPE["truth"]), none=None)
    assert a == b
    b.tab["covered_voxels"][1] = 3
    assert a != b
    assert a != V.VolumeScore(dice=0.5)
    ones = np.ones((4, 4, 4), np.uint8)
    for kw in ({"pixdim": (1, 1)}, {"pixdim": (1, 0, 1)}, {"pixdim": (1, float("inf"), 1)}, {"pixdim": (1, -2, 1)}, {"pixdim": (1, float("nan"), 1)}, {"connectivity": 0},
               {"connectivity": 4}, {"lesion_connectivity": 7}, {"percentile": -1}, {"percentile": 100.5}):
        with pytest.raises(ValueError):
            V.score_volume(ones, ones, **kw)
    with pytest.raises(ValueError):
        V.score_volume(ones, np.ones((4, 4, 5), np.uint8))
    with pytest.raises(ValueError):
        V.score_volume(ones.astype(np.float32), ones)
    with pytest.raises(ValueError):
        V.score_volume(ones, ones[0])
    with pytest.raises(ValueError):
        V.distance_transform(ones, pixdim=(0, 1, 1))
    with pytest.raises(ValueError):
        V.surface(ones, connectivity=5)
    with pytest.raises(ValueError):
        V.segment_volume(np.zeros((4, 4, 10), np.int16), None, truth=np.zeros((4, 4, 9), np.uint8))

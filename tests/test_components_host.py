"""CPU: the component step's host side -- tests/components_oracle.py against the scikit-image goldens (this pins the oracle) and against scipy.ndimage where it
imports, the table / min_ml / tie rules of covidseg_amd.volume on hand-made statistics, and the new entries' bindings."""
import os
import re

import numpy as np
import pytest

import components_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "component_goldens.npz")
ENTRIES = {"unet_vol_label_ws_bytes": 3, "unet_vol_label": 11, "unet_vol_component_stats": 8, "unet_vol_filter_components": 12}


def _cases():
    g = np.load(GOLD)
    for name in sorted({k.split("/")[0] for k in g.files}):
        shape = tuple(int(v) for v in g[name + "/shape"])
        size = int(np.prod(shape))
        mask = np.unpackbits(g[name + "/bits"])[:size].reshape(shape).astype(np.uint8)
        if name + "/values" in g.files:
            mask[mask != 0] = g[name + "/values"]
        yield name, mask, g


def test_the_oracle_reproduces_every_golden():
    names = []
    for name, mask, g in _cases():
        c = int(g[name + "/c"])
        labels, n = CO.label(mask, c)
        assert n == int(g[name + "/n"]) and labels.dtype == np.int32 and np.array_equal(labels, g[name + "/labels"]), name
        removed = np.unpackbits(g[name + "/removed_bits"])[:mask.size].reshape(mask.shape)
        assert np.array_equal(CO.remove_small(mask, int(g[name + "/min_size"]), c), removed), name
        names.append(name)
    assert len(names) >= 12 and any("multivalued" in n for n in names) and any("serpentine" in n for n in names)
    assert os.path.getsize(GOLD) < 1 << 20


def test_golden_cases_are_what_they_claim():
    by = {name: (mask, g) for name, mask, g in _cases()}
    assert int(by["serpentine_c1"][1]["serpentine_c1/n"]) == 1
    cb = by["checkerboard_c1"][0]
    assert int(by["checkerboard_c1"][1]["checkerboard_c1/n"]) == int(cb.sum()) and int(by["checkerboard_c2"][1]["checkerboard_c2/n"]) == 1
    assert int(by["ones_c1"][1]["ones_c1/n"]) == 1 and int(by["zeros_c3"][1]["zeros_c3/n"]) == 0
    assert set(np.unique(by["multivalued_c1"][0])) == {0, 1, 2, 255}


def test_the_oracle_equals_scipy_on_fresh_masks():
    ndi = pytest.importorskip("scipy.ndimage")
    for seed, (shape, density) in enumerate([((40, 48, 24), 0.35), ((33, 17, 29), 0.31), ((64, 9, 40), 0.1), ((1, 50, 3), 0.5), ((70, 66, 10), 0.62)]):
        m = CO.random_mask(shape, density, seed)
        for c in (1, 2, 3):
            want, wn = ndi.label(m, ndi.generate_binary_structure(3, c))
            labels, n = CO.label(m, c)
            assert n == wn and np.array_equal(labels, want), (shape, c)
    for m in (CO.serpentine((40, 31, 13)), CO.spiral((40, 31, 13))):
        want, wn = ndi.label(m)
        labels, n = CO.label(m, 1)
        assert n == wn == 1 and np.array_equal(labels, want)


def test_oracle_statistics_on_a_hand_made_volume():
    lab = np.zeros((4, 5, 6), np.int32)
    lab[0, 0, 0] = 1
    lab[1:3, 2:5, 1] = 2
    st = CO.stats(lab, 2)
    assert st["voxels"].tolist() == [1, 6] and st["sx"].tolist() == [0, 9] and st["sy"].tolist() == [0, 18] and st["sz"].tolist() == [0, 6]
    assert (st["x0"].tolist(), st["x1"].tolist(), st["y0"].tolist(), st["y1"].tolist(), st["z0"].tolist(), st["z1"].tolist()) == ([0, 1], [0, 2], [0, 2], [0, 4], [0, 1], [0, 1])


def test_table_min_ml_and_ties():
    from covidseg_amd import volume as V
    st = {"voxels": np.array([4, 10, 10, 1]), "sx": np.array([6, 45, 5, 7]), "sy": np.array([2, 0, 30, 0]), "sz": np.array([0, 90, 10, 3]),
          "x0": np.array([1, 0, 0, 7]), "x1": np.array([2, 9, 1, 7]), "y0": np.array([0, 0, 1, 0]), "y1": np.array([1, 0, 5, 0]),
          "z0": np.array([0, 9, 1, 3]), "z1": np.array([0, 9, 1, 3])}
    t = V.table_from_stats(st, (0.5, 0.5, 2.0))
    assert t.dtype.names == ("label", "voxels", "ml", "x0", "x1", "y0", "y1", "z0", "z1", "cx", "cy", "cz")
    assert t["label"].tolist() == [1, 2, 3, 4] and t["voxels"].tolist() == [4, 10, 10, 1]
    assert t["ml"].tolist() == [4 * 0.5 / 1000.0, 10 * 0.5 / 1000.0, 10 * 0.5 / 1000.0, 0.5 / 1000.0]
    assert t["cx"].tolist() == [1.5, 4.5, 0.5, 7.0] and t["cy"].tolist() == [0.5, 0.0, 3.0, 0.0] and t["cz"].tolist() == [0.0, 9.0, 1.0, 3.0]
    assert t["x1"].tolist() == [2, 9, 1, 7] and t["cx"].dtype == np.float64 and V._STAT_DTYPE.itemsize == 64          # what comes back per component
    assert len(V.table_from_stats({k: v[:0] for k, v in st.items()})) == 0
    # ceil(min_ml * 1000 / prod(pixdim)): 0.8 x 0.8 x 5 mm voxels are 3.2 mm^3 -> 0.05 ml = 15.6.. -> 16 voxels; an exact multiple is not rounded up
    assert V.min_voxels_from_ml(0.05, (0.8, 0.8, 5.0)) == 16 == CO.min_voxels_from_ml(0.05, (0.8, 0.8, 5.0))
    assert V.min_voxels_from_ml(0.008, (1.0, 1.0, 1.0)) == 8 and V.min_voxels_from_ml(0.5, (0.5, 0.5, 2.0)) == 1000
    # the k largest, ties to the lower label
    assert V.largest_labels(st["voxels"], 1).tolist() == [2] and V.largest_labels(st["voxels"], 2).tolist() == [2, 3]
    assert V.largest_labels(st["voxels"], 3).tolist() == [1, 2, 3] and V.largest_labels(st["voxels"], 9).tolist() == [1, 2, 3, 4] and V.largest_labels(st["voxels"], 0).tolist() == []
    assert CO.largest(st["voxels"], 2).tolist() == [2, 3]
    with pytest.raises(ValueError):
        V.remove_small(np.ones((2, 2, 2), np.uint8))
    with pytest.raises(ValueError):
        V.remove_small(np.ones((2, 2, 2), np.uint8), min_ml=1.0)
    with pytest.raises(ValueError):
        V.segment_volume(np.zeros((4, 4, 10), np.int16), None, connectivity=0)


def test_the_new_entries_are_bound_with_the_declared_argument_counts():
    from covidseg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/unet_hip.h"
        assert m.group(1).count(",") + 1 == nargs
        assert name in _lib._PROTOS, f"{name} is not bound in _lib._PROTOS"
        assert len(_lib._PROTOS[name][1]) == nargs
    assert _lib.ABI_VERSION == 16 and "#define UNET_ABI_VERSION 16" in open(os.path.join(ROOT, "include", "unet_hip.h")).read()


def test_the_kernel_file_is_built_and_keeps_phases_apart():
    src = open(os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc", "kernels_components.hip")).read()
    mk = open(os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc", "Makefile")).read()
    assert "kernels_components.hip" in mk
    assert "asm" not in re.sub(r"//[^\n]*", "", src)                  # no inline assembly

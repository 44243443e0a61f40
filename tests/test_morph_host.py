"""CPU: tests/morph_oracle.py (the numpy restatement the GPU tests compare with) against scipy.ndimage, the new prototypes, and the host-side refusals of the new
covidseg_amd.volume functions.  Everything is compared with np.array_equal / ==."""
import os
import re

import numpy as np
import pytest

import components_oracle as CO
import morph_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
try:
    import scipy.ndimage as ndi
except ImportError:                                                  # the scipy comparisons skip; the binding and refusal tests do not need it
    ndi = None
needs_scipy = pytest.mark.skipif(ndi is None, reason="scipy does not import here")

SHAPES = [(1, 1, 1), (17, 1, 33), (5, 9, 2), (63, 40, 6), (65, 23, 11)]
NEW_ENTRIES = ("unet_vol_morph_ws_bytes", "unet_vol_morph", "unet_vol_ball", "unet_vol_label_planar", "unet_vol_fill_holes_ws_bytes", "unet_vol_fill_holes")


def _structure(c, planar=False):
    s = ndi.generate_binary_structure(3, c)
    if planar:
        s = s.copy(); s[:, :, 0] = False; s[:, :, 2] = False
    return s


@needs_scipy
def test_structure_is_scipys():
    for c in (1, 2, 3):
        assert np.array_equal(MO.structure(c), _structure(c))
    for c in (1, 2):
        assert np.array_equal(MO.structure(c, True), _structure(c, True))
    with pytest.raises(ValueError):
        MO.structure(3, True)


@needs_scipy
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", [1, 2, 3])
def test_operators_against_scipy(shape, c):
    fns = {"dilate": ndi.binary_dilation, "erode": ndi.binary_erosion, "open": ndi.binary_opening, "close": ndi.binary_closing}
    for i, density in enumerate((0.03, 0.4, 0.9)):
        m = CO.random_mask(shape, density, 11 + i)
        for it in (1, 2, 3, 5):
            for b in (0, 1):
                for op, fn in fns.items():
                    want = fn(m != 0, structure=_structure(c), iterations=it, border_value=b)
                    got = MO.OPS[op](m, c, it, b)
                    assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, c, density, it, b, op)
                    if c < 3:
                        want = fn(m != 0, structure=_structure(c, True), iterations=it, border_value=b)
                        assert np.array_equal(MO.OPS[op](m, c, it, b, planar=True), want), (shape, c, density, it, b, op, "planar")


@needs_scipy
def test_planar_operators_are_the_slices_on_their_own():
    m = CO.random_mask((33, 20, 7), 0.2, 4)
    got = MO.closing(m, 2, 2, 0, planar=True)
    for z in range(m.shape[2]):
        assert np.array_equal(got[:, :, z], ndi.binary_closing(m[:, :, z] != 0, structure=ndi.generate_binary_structure(2, 2), iterations=2))


@pytest.mark.parametrize("b", [0, 1])
def test_duality(b):
    for c in (1, 2, 3):
        for planar in ((False, True) if c < 3 else (False,)):
            m = CO.random_mask((31, 17, 9), 0.5, c)
            for it in (1, 3):
                assert np.array_equal(MO.erosion(m, c, it, b, planar), 1 - MO.dilation(1 - m, c, it, 1 - b, planar))


@needs_scipy
@pytest.mark.parametrize("shape", SHAPES)
def test_planar_labels_against_scipy(shape):
    for c in (1, 2):
        for i, density in enumerate((0.05, 0.45, 0.8)):
            m = CO.random_mask(shape, density, 21 + i)
            want, wn = ndi.label(m, structure=_structure(c, True))
            got, n = MO.label_planar(m, c)
            assert n == wn and got.dtype == np.int32 and np.array_equal(got, want), (shape, c, density)


@needs_scipy
@pytest.mark.parametrize("shape", SHAPES + [(40, 33, 17)])
def test_fill_holes_against_scipy(shape):
    for i, density in enumerate((0.3, 0.6, 0.8)):
        m = CO.random_mask(shape, density, 31 + i)
        for c in (1, 2, 3):
            assert np.array_equal(MO.fill_holes(m, c), ndi.binary_fill_holes(m, structure=_structure(c))), (shape, density, c)
        for c in (1, 2):
            assert np.array_equal(MO.fill_holes(m, c, planar=True), ndi.binary_fill_holes(m, structure=_structure(c, True))), (shape, density, c, "planar")


@needs_scipy
def test_shell_and_tube():
    """Per-slice filling never fills less than 3-D filling with the same in-plane structure: a background path inside a slice to the slice's edge is also a path to a
    face of the volume.  So: a closed shell is filled both ways; a shell with an opening in one slice is filled nowhere in 3-D and, per slice, everywhere but in the slice
    that is cut open; a tube that is open at one z end is filled per slice and not in 3-D."""
    shape = (24, 20, 12)
    shell = MO.hollow_shell(shape, (3, 4, 2), (15, 14, 8))
    full = shell.copy(); full[3:16, 4:15, 2:9] = 1
    assert np.array_equal(MO.fill_holes(shell), full) and np.array_equal(MO.fill_holes(shell, planar=True), full)
    cut = shell.copy(); cut[15, 9, 5] = 0                             # an opening in the wall, in slice 5 only
    assert np.array_equal(MO.fill_holes(cut), cut)
    per = MO.fill_holes(cut, planar=True)
    want = full.copy(); want[:, :, 5] = cut[:, :, 5]
    assert np.array_equal(per, want) and per.sum() > cut.sum()
    tube = MO.open_tube(shape, (3, 4, 0), (15, 14, 8))
    assert np.array_equal(MO.fill_holes(tube), tube)
    filled = tube.copy(); filled[3:16, 4:15, 0:9] = 1
    assert np.array_equal(MO.fill_holes(tube, planar=True), filled)
    for m in (shell, cut, tube):
        assert np.array_equal(MO.fill_holes(m), ndi.binary_fill_holes(m)) and np.array_equal(MO.fill_holes(m, planar=True), ndi.binary_fill_holes(m, structure=_structure(1, True)))


@needs_scipy
def test_ball_operators():
    """unit spacing and an integer r^2: the squared distances are exact integers, so the ball operators are scipy's with the ball as footprint (erosion: border_value=1,
    the outside is foreground)"""
    m = CO.ellipsoids((130, 70, 37), 12, 0.001, 3)
    fp = MO.ball_footprint(2.0)
    assert fp.shape == (5, 5, 5) and fp.sum() == 33
    assert np.array_equal(MO.dilate_mm(m, 2.0), ndi.binary_dilation(m, structure=fp))
    assert np.array_equal(MO.erode_mm(m, 2.0), ndi.binary_erosion(m, structure=fp, border_value=1))
    small = CO.ellipsoids((40, 33, 17), 5, 0.002, 1)
    pixdim = (0.7, 0.7, 1.25)
    fp = MO.ball_footprint(1.5, pixdim)
    assert np.array_equal(MO.dilate_mm(small, 1.5, pixdim), ndi.binary_dilation(small, structure=fp))
    assert np.array_equal(MO.erode_mm(small, 1.5, pixdim), ndi.binary_erosion(small, structure=fp, border_value=1))
    assert np.array_equal(MO.close_mm(small, 1.5, pixdim), MO.erode_mm(MO.dilate_mm(small, 1.5, pixdim), 1.5, pixdim))
    assert np.array_equal(MO.dilate_mm(small, 0.0), small) and np.array_equal(MO.erode_mm(small, 0.0), small)
    assert MO.erode_mm(np.ones((4, 4, 4), np.uint8), 3.0).all() and not MO.dilate_mm(np.zeros((4, 4, 4), np.uint8), 3.0).any()


def test_new_prototypes_are_bound_and_declared():
    from covidseg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name in NEW_ENTRIES:
        assert name in _lib._PROTOS, name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert len(_lib._PROTOS["unet_vol_morph"][1]) == 15 and len(_lib._PROTOS["unet_vol_fill_holes"][1]) == 12
    assert _lib._PROTOS["unet_vol_label_planar"] == _lib._PROTOS["unet_vol_label"]
    assert _lib.MORPH_OPS == {"dilate": 0, "erode": 1, "open": 2, "close": 3}
    for k, v in (("UNET_MORPH_DILATE", 0), ("UNET_MORPH_ERODE", 1), ("UNET_MORPH_OPEN", 2), ("UNET_MORPH_CLOSE", 3)):
        assert re.search(k + r"\s*=\s*%d\b" % v, hdr), k
    assert re.search(r"UNET_VOL_MORPH_MAX_ITERATIONS\s+%d\b" % _lib.MORPH_MAX_ITERATIONS, hdr)


def test_host_side_refusals_need_no_gpu():
    """every bad argument is refused on the host, before a device is looked for"""
    from covidseg_amd import volume as V
    m = np.ones((4, 4, 4), np.uint8)
    four = (V.binary_dilation, V.binary_erosion, V.binary_opening, V.binary_closing)
    bad = []
    for fn in four:
        bad += [lambda fn=fn: fn(m, connectivity=0), lambda fn=fn: fn(m, connectivity=4), lambda fn=fn: fn(m, connectivity=3, per_slice=True),
                lambda fn=fn: fn(m, iterations=0), lambda fn=fn: fn(m, iterations=-1), lambda fn=fn: fn(m, iterations=65), lambda fn=fn: fn(m, iterations=1.5),
                lambda fn=fn: fn(m, border_value=2), lambda fn=fn: fn(m, border_value=-1), lambda fn=fn: fn(m.astype(np.float32)), lambda fn=fn: fn(m[0])]
    for fn in (V.dilate_mm, V.erode_mm, V.open_mm, V.close_mm):
        bad += [lambda fn=fn: fn(m, -1.0, (1, 1, 1)), lambda fn=fn: fn(m, float("nan"), (1, 1, 1)), lambda fn=fn: fn(m, float("inf"), (1, 1, 1)),
                lambda fn=fn: fn(m, 1.0, (1, 0, 1)), lambda fn=fn: fn(m, 1.0, (1, 1)), lambda fn=fn: fn(m[0], 1.0, (1, 1, 1)), lambda fn=fn: fn(m * 0.5, 1.0, (1, 1, 1))]
    bad += [lambda: V.fill_holes(m, connectivity=0), lambda: V.fill_holes(m, connectivity=4), lambda: V.fill_holes(m, connectivity=3, per_slice=True),
            lambda: V.fill_holes(m.astype(np.float64)), lambda: V.fill_holes(m[0]),
            lambda: V.label_volume(m, connectivity=3, per_slice=True), lambda: V.label_volume(m, connectivity=0, per_slice=True),
            lambda: V.postprocess(m, [("shrink", {})]), lambda: V.postprocess(m, [("close", {"radius_mm": 1.0})]), lambda: V.postprocess(m, [("close", {"iterations": 0})]),
            lambda: V.postprocess(m, [("close_mm", {"radius_mm": 1.0})]), lambda: V.postprocess(m, [("close_mm", {})], pixdim=(1, 1, 1)),
            lambda: V.postprocess(m, [("fill_holes", {"connectivity": 3, "per_slice": True})]), lambda: V.postprocess(m, [("remove_small", {})]),
            lambda: V.postprocess(m, [("remove_small", {"min_ml": 0.1})]), lambda: V.postprocess(m, [("close", {}), ("fill_holes", {"connectivity": 7})]),
            lambda: V.postprocess(m, [("close",)]), lambda: V.postprocess(m, 5), lambda: V.postprocess(m.astype(np.float32), [("close", {})]),
            lambda: V.segment_volume(np.zeros((8, 8, 8), np.int16), None, postprocess=[("close", {"iterations": 99})])]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
    assert V.MORPH_MAX_ITERATIONS == 64 and "close" in V.POSTPROCESS_STEPS and "fill_holes" in V.POSTPROCESS_STEPS

"""CPU: tests/resample_oracle.py against scipy.ndimage.affine_transform, and the host side of covidseg_amd.volume's resampling: the grids, the
matrices of spacing= / shape= / like= and of the 48 orientations, the NIfTI header with an sform, and every refusal -- none of which needs a device."""
import os

import numpy as np
import pytest

import lungside_oracle as LO
import resample_oracle as RS
from covidseg_amd import _lib, nifti_min
from covidseg_amd import volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC_SHAPE, OUT_SHAPE = (7, 5, 6), (11, 6, 15)
MATRICES = {"anisotropic": RS.anisotropic_matrix(), "oblique": RS.oblique_matrix()}


def _values():
    return np.random.default_rng(7).uniform(-1024.0, 3000.0, SRC_SHAPE)


@pytest.mark.parametrize("mode", ["nearest", "constant"])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_linear_oracle_equals_scipy(name, mode):
    """bound: 1e-12 max|v|, the figure tests/test_augment_host.py uses for the same kind of pin (the two differ by a few 1e-16 max|v|: scipy weighs the eight
    neighbours instead of nesting three blends)"""
    ndi = pytest.importorskip("scipy.ndimage")
    v, M = _values(), MATRICES[name]
    cval = -1000.0
    want = ndi.affine_transform(v, M[:, :3], M[:, 3], OUT_SHAPE, order=1, mode="nearest" if mode == "nearest" else "grid-constant", cval=cval)
    got = RS.linear(v, M, OUT_SHAPE, RS.MODES[mode], cval)
    err = float(np.abs(got - want).max()) / float(np.abs(v).max())
    print(f"linear {name} {mode}: max|oracle - scipy| / max|v| = {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("mode", ["nearest", "constant"])
@pytest.mark.parametrize("name", sorted(MATRICES))
def test_nearest_oracle_equals_scipy_order_0(name, mode):
    ndi = pytest.importorskip("scipy.ndimage")
    v, M = _values(), MATRICES[name]
    cval = -1000.0
    want = ndi.affine_transform(v, M[:, :3], M[:, 3], OUT_SHAPE, order=0, mode="nearest" if mode == "nearest" else "grid-constant", cval=cval)
    got = RS.nearest(v, M, OUT_SHAPE, RS.MODES[mode], cval)
    tie = np.zeros(OUT_SHAPE, bool)
    for s in RS.coords(M, OUT_SHAPE):
        tie |= np.abs((s + 0.5) - np.rint(s + 0.5)) < 1e-9
    print(f"nearest {name} {mode}: {int(tie.sum())} of {tie.size} outputs lie on a tie")
    assert tie.mean() <= 0.01
    assert np.array_equal(got[~tie], want[~tie])


def test_identity_returns_the_decoded_source():
    raw = np.random.default_rng(3).integers(-1200, 600, SRC_SHAPE).astype(np.int16)
    fd = RS.decode(raw, (0.5, -100.0))
    assert np.array_equal(fd, nifti_min.apply_scaling(raw, 0.5, -100.0))
    g = V.Grid(SRC_SHAPE, np.diag([0.7, 0.7, 2.5, 1.0]), False)
    target, M = V.resample_target(g, shape=SRC_SHAPE)
    assert np.array_equal(M, np.eye(4)[:3]) and target.shape == SRC_SHAPE and np.array_equal(target.affine, g.affine)
    for mode in (0, 1):
        assert np.array_equal(RS.linear(fd, M, SRC_SHAPE, mode, -7.0), fd)
        assert np.array_equal(RS.nearest(raw, M, SRC_SHAPE, mode, -7), raw)


def test_a_coordinate_that_overflows_reads_the_edge_or_cval():
    """an M whose coordinates overflow to inf, -inf and NaN (inf - inf): clamped in mode 0 (a NaN to 0), outside in mode 1, where both forms give cval and no NaN"""
    fd = _values()
    M = np.array([[1.7e308, -1.7e308, 0.0, 0.0], [0.0, 1.7e308, 0.0, 0.0], [0.0, 0.0, -1.7e308, 0.0]])
    out = (4, 4, 3)
    for mode in (0, 1):
        lin, near = RS.linear(fd, M, out, mode, -5.5), RS.nearest(fd, M, out, mode, -5.5)
        assert not np.isnan(lin).any() and not np.isnan(near).any()
        assert lin[0, 0, 0] == near[0, 0, 0] == fd[0, 0, 0]
        if mode == 1:
            assert (lin[2:, 2:, :] == -5.5).all() and (near[2:, 2:, :] == -5.5).all() and (lin[:, :, 2] == -5.5).all()
        else:
            assert lin[2, 2, 0] == near[2, 2, 0] == fd[0, 4, 0] and lin[0, 0, 2] == near[0, 0, 2] == fd[0, 0, 0] and lin[3, 0, 0] == fd[6, 0, 0]


def test_integer_up_zoom_in_nearest_is_np_repeat():
    raw = np.random.default_rng(4).integers(0, 200, SRC_SHAPE).astype(np.uint8)
    g = V.Grid(SRC_SHAPE, np.diag([1.0, 1.0, 3.0, 1.0]), False)
    target, M = V.resample_target(g, shape=(14, 15, 24))
    want = np.repeat(np.repeat(np.repeat(raw, 2, axis=0), 3, axis=1), 4, axis=2)
    assert np.array_equal(RS.nearest(raw, M, target.shape, 0), want)
    assert np.allclose(target.pixdim, (0.5, 1.0 / 3.0, 0.75))


def test_all_48_orientations_agree_with_the_lung_side_oracle():
    ras = np.random.default_rng(5).integers(-1000, 1000, (12, 10, 6)).astype(np.int16)
    codes_all = LO.all_axcodes()
    assert len(codes_all) == 48
    for codes in codes_all:
        stored = LO.reorient(ras, codes)
        M, shp = V.reorient_matrix(stored.shape, codes, "RAS")
        assert shp == ras.shape and np.array_equal(M, np.rint(M))
        back = RS.nearest(stored, M, shp, 0)
        assert np.array_equal(back, ras) and np.array_equal(back, LO.to_canonical(stored, codes))
        M2, shp2 = V.reorient_matrix(ras.shape, "RAS", codes)
        assert shp2 == stored.shape and np.array_equal(RS.nearest(ras, M2, shp2, 0), stored)
        # the permuted affine names the new codes
        A = LO.affine_of(codes, LO.reorient_pixdim(np.array([0.7, 0.8, 2.5]), codes))
        new = A @ np.vstack([M, [0, 0, 0, 1]])
        assert nifti_min.axcodes_from_affine(new) == ("R", "A", "S") and np.allclose(np.abs(new[:3, :3]).sum(axis=0), (0.7, 0.8, 2.5))


def test_header_with_affine_round_trips(tmp_path):
    A = RS.oblique_affine((0.7, 0.7, 2.5))
    h = nifti_min.header_with_affine((5, 4, 3), A)
    assert len(h) == 348
    bo, f = nifti_min.parse_header(h)
    assert f["sform_code"] == 1 and f["qform_code"] == 0 and tuple(f["dim"][:4]) == (3, 5, 4, 3)
    assert np.allclose(f["pixdim"][1:4], (0.7, 0.7, 2.5), rtol=1e-6)
    vol = np.arange(60, dtype=np.float32).reshape((5, 4, 3), order="F")
    for name in ("a.nii", "a.nii.gz"):
        path = tmp_path / name
        nifti_min.write(path, vol, header=h)
        back = nifti_min.read(path)
        assert back.affine_source == "sform" and np.array_equal(back.raw, vol)
        assert np.array_equal(back.affine[:3], A[:3].astype(np.float32).astype(np.float64)) and np.array_equal(back.affine[3], [0, 0, 0, 1])
    with pytest.raises(nifti_min.NiftiFormatError):
        nifti_min.header_with_affine((5, 4, 3), np.zeros((4, 4)))
    bad = A.copy(); bad[0, 0] = np.nan
    with pytest.raises(nifti_min.NiftiFormatError):
        nifti_min.header_with_affine((5, 4, 3), bad)


def test_spacing_and_shape_give_the_stated_grid():
    shape, pix = (67, 9, 7), (0.7, 0.7, 2.5)
    A = RS.oblique_affine(pix)
    g = V.Grid(shape, A)
    assert np.allclose(g.pixdim, pix, rtol=1e-15) and g.oriented and g.axcodes == ("R", "A", "S")
    target, M = V.resample_target(g, spacing=(1.0, 1.0, 1.0))
    n2 = tuple(max(1, round(n * p / 1.0)) for n, p in zip(shape, g.pixdim))
    assert target.shape == n2 == (47, 6, 18)
    for tgt, m, shp in ((target, M, n2),) + tuple((*V.resample_target(g, shape=s), s) for s in ((33, 9, 14), (1, 1, 1), (200, 3, 7))):
        z = np.array([n / k for n, k in zip(shape, shp)])
        want = np.zeros((3, 4)); want[:, :3] = np.diag(z); want[:, 3] = 0.5 * z - 0.5
        assert np.array_equal(m, want) and tgt.shape == tuple(shp) and tgt.oriented
        assert np.array_equal(tgt.affine, A @ np.vstack([want, [0, 0, 0, 1]]))
        # the field of view is kept: the outer faces of the first and the last voxel stay where they were
        for corner, new_corner in ((np.array([-0.5, -0.5, -0.5, 1.0]), np.array([-0.5, -0.5, -0.5, 1.0])),
                                   (np.array([n - 0.5 for n in shape] + [1.0]), np.array([k - 0.5 for k in shp] + [1.0]))):
            assert np.allclose(A @ corner, tgt.affine @ new_corner, atol=1e-9)
    # like= / grid=: inv(A_src) @ A_dst
    other = V.Grid((20, 21, 22), RS.oblique_affine((1.0, 1.0, 1.0), deg=-4.0))
    for kw in ({"like": other}, {"grid": other}):
        tgt, m = V.resample_target(g, **kw)
        assert tgt is other and np.array_equal(m, (np.linalg.inv(A) @ other.affine)[:3]) and np.array_equal(m, V.resample_matrix(g, other))


def test_grid_of_a_volume():
    a = np.zeros((4, 5, 6), np.int16)
    g = V.Grid.of(a)
    assert not g.oriented and g.axcodes is None and g.pixdim == (1.0, 1.0, 1.0) and g.shape == (4, 5, 6)
    g = V.Grid.of(a, pixdim=(0.5, 0.6, 2.0))
    assert not g.oriented and np.allclose(g.pixdim, (0.5, 0.6, 2.0)) and abs(g.voxel_ml - 0.0006) < 1e-15
    A = LO.affine_of(("L", "P", "S"), (0.5, 0.6, 2.0))
    g = V.Grid.of(a, affine=A)
    assert g.oriented and g.axcodes == ("L", "P", "S")
    vol = nifti_min.NiftiVolume(np.asfortranarray(a), 0.0, 0.0, (0.5, 0.6, 2.0), nifti_min.header_with_affine(a.shape, A), "<")
    g = V.Grid.of(vol)
    assert g.oriented and g.axcodes == ("L", "P", "S") and np.allclose(g.pixdim, (0.5, 0.6, 2.0), rtol=1e-6)
    for bad_shape in ((4, 5), (4, 5, 0), (4.5, 5, 6), "abc"):
        with pytest.raises(ValueError):
            V.Grid(bad_shape, np.eye(4))
    for bad_affine in (np.zeros((4, 4)), np.eye(3), np.full((4, 4), np.nan), np.diag([1.0, 1.0, 0.0, 1.0])):
        with pytest.raises(ValueError):
            V.Grid((4, 5, 6), bad_affine)


def test_every_refusal_fires_without_a_device():
    a = np.zeros((4, 5, 6), np.int16)
    mask = np.zeros((4, 5, 6), np.uint8)
    oriented = V.Grid((4, 5, 6), LO.affine_of(("L", "P", "S")))
    bare = V.Grid.of(a)
    with pytest.raises(ValueError, match="exactly one"):
        V.resample_volume(a, spacing=(1, 1, 1), shape=(4, 5, 6))
    with pytest.raises(ValueError, match="exactly one"):
        V.resample_volume(a)
    with pytest.raises(ValueError, match="exactly one"):
        V.resample_mask(mask, like=oriented, grid=oriented)
    with pytest.raises(ValueError, match="orientation"):
        V.resample_volume(a, like=oriented)                         # the source is unoriented
    with pytest.raises(ValueError, match="orientation"):
        V.resample_volume(a, affine=oriented.affine, like=bare)     # the target is
    with pytest.raises(ValueError, match="orientation"):
        V.resample_matrix(bare, oriented)
    with pytest.raises(ValueError, match="orientation"):
        V.change_between(mask, oriented, mask, bare)
    with pytest.raises(ValueError, match="orientation"):
        V.change_between(mask, bare, mask, oriented)
    with pytest.raises(ValueError, match="orientation"):
        V.reorient_volume(a, "RAS")
    with pytest.raises(ValueError, match="raw"):
        V.resample_volume(a, spacing=(1, 1, 1), order="linear", dtype="raw")
    with pytest.raises(ValueError, match="nearest"):
        V.resample_labels(a.astype(np.int32), spacing=(1, 1, 1), order="linear")
    with pytest.raises(ValueError, match="non-finite"):
        V.resample_linear_device(None, (4, 4, 5, 6, 0, 1.0, 0.0), np.full((3, 4), np.inf), 0, 0.0, (4, 5, 6), 64)
    with pytest.raises(ValueError, match="non-finite"):
        V.resample_nearest_device(None, 2, (4, 5, 6), np.full((3, 4), np.nan), 0, 0, (4, 5, 6))
    with pytest.raises(ValueError, match="non-finite"):            # two finite affines whose product overflows
        far = np.eye(4); far[:3, 3] = 1e250
        V.resample_matrix(V.Grid((4, 5, 6), np.diag([1e-100, 1e-100, 1e-100, 1.0])), V.Grid((4, 5, 6), far))
    for kw in ({"order": "cubic"}, {"mode": "reflect"}, {"dtype": "int16"}, {"cval": "air"}, {"spacing": (1, 0, 1)}, {"spacing": (1, 1)}, {"shape": (4, 0, 6)},
               {"order": "nearest", "return_device": True}, {"dtype": "float64", "out_path": "x.nii"}):
        full = {"spacing": (1, 1, 1), **kw} if "shape" not in kw else kw
        with pytest.raises(ValueError):
            V.resample_volume(a, **full)
    with pytest.raises(ValueError):
        V.resample_mask(np.zeros((4, 5, 6), np.float32), spacing=(1, 1, 1))
    with pytest.raises(ValueError):
        V.change_between(np.zeros((4, 5, 5), np.uint8), oriented, mask, oriented)
    with pytest.raises(ValueError):
        V.reorient_volume(a, "RAX", orientation="LPS")


def test_the_declarations_and_bindings_exist():
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    for name, nargs in (("unet_vol_resample_nearest", 14), ("unet_vol_resample_linear", 18)):
        assert f"int32_t {name}(" in hdr
        assert name in _lib._PROTOS and len(_lib._PROTOS[name][1]) == nargs and name in _lib.EXPORTED_SYMBOLS
    mk = open(os.path.join(os.path.dirname(V.__file__), "csrc", "Makefile")).read()
    assert "kernels_resample.hip" in mk.split("SRCS =")[1].split("\n")[0]
    assert all("kernels_resample.o" in line for line in mk.splitlines() if line.endswith("EXTRA = -ffp-contract=off"))
    assert _lib.ABI_VERSION == 16 and "#define UNET_ABI_VERSION 16" in hdr

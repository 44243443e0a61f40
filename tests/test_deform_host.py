"""CPU: tests/deform_oracle.py (the numpy restatement of csrc/kernels_deform.hip) against scipy and against closed forms, the argument checks of
volume.refine_registration / DisplacementField, the four entries in the header and the bindings, and the whole loop of refine_registration over the oracle on a phantom
with a known field."""
import os
import re

import numpy as np
import pytest

import deform_oracle as DO
import resample_oracle as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4)[:3]
I3 = np.eye(3)
ENTRIES = {"unet_vol_smooth_axis": 11, "unet_vol_demons_step": 25, "unet_vol_warp_field": 26, "unet_vol_jacobian": 9}


# ---- the Gaussian pass ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sigma", [0.4, 1.5, 4.0])
def test_smoothing_is_correlate1d_with_the_edge_repeated(axis, sigma):
    from scipy import ndimage
    from covidseg_amd import volume as V
    w = V.gaussian_weights(sigma)
    assert w.size == 2 * int(np.ceil(3 * sigma)) + 1 and abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1])
    x = (np.random.default_rng(3).normal(size=(2, 9, 7, 5)) * 300).astype(np.float32)          # extents shorter than the radius at sigma = 4
    got = DO.smooth_axis(x, axis, w)
    want = ndimage.correlate1d(x.astype(np.float64), w, axis=axis + 1, mode="nearest")
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max() + np.abs(want).max() * 2.0 ** -24          # (the float32 store on top of scipy's 1e-12)
    # before the store: the float64 sum itself within 1e-12 max|x|
    acc = sum(w[t] * np.take(x.astype(np.float64), np.clip(np.arange(x.shape[axis + 1]) + t - w.size // 2, 0, x.shape[axis + 1] - 1), axis=axis + 1) for t in range(w.size))
    assert np.abs(acc - want).max() <= 1e-12 * np.abs(x).max()


def test_radius_zero_is_a_copy_and_sigma_zero_is_no_pass():
    from covidseg_amd import volume as V
    x = (np.random.default_rng(4).normal(size=(5, 4, 3)) * 50).astype(np.float32)
    x[1, 1, 1] = -0.0
    for axis in range(3):
        assert DO.same_bits(DO.smooth_axis(x, axis, [1.0]), x + np.float32(0.0))          # (0 + -0 = +0: the sum starts from 0)
    assert V.gaussian_weights(0) is None and V.gaussian_weights(0.0) is None
    for bad in (-1.0, np.nan, np.inf, "1", None, True, 11.0):
        with pytest.raises(ValueError):
            V.gaussian_weights(bad)
    assert V.gaussian_weights(32 / 3.0).size == 65


# ---- the warp ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_zero_field_is_the_plain_resampling():
    rng = np.random.default_rng(5)
    src = rng.integers(-1000, 500, (9, 7, 6)).astype(np.int16)
    out = (8, 6, 5)
    zero = np.zeros((3,) + out, np.float32)
    coarse = np.zeros((3, 4, 3, 2), np.float32)
    L = rng.normal(size=(3, 3))
    for M in (EYE, RS.anisotropic_matrix(), RS.oblique_matrix()):
        for field, F in ((zero, None), (coarse, RS.oblique_matrix(5.0))):
            for mode in (0, 1):
                for dst in (64, 16, 2):
                    assert np.array_equal(DO.warp(src, (0.5, -100.0), M, L, field, F, out, 1, mode, -7.5, dst), RS.linear(RS.decode(src, (0.5, -100.0)), M, out, mode, -7.5, dst))
                assert np.array_equal(DO.warp(src, None, M, L, field, F, out, 0, mode, -3), RS.nearest(src, M, out, mode, -3))


def test_a_field_of_whole_voxels_is_an_index_shift():
    rng = np.random.default_rng(6)
    src = rng.normal(size=(9, 8, 7))
    shift = (2, -1, 3)
    spacing = np.array([2.0, 0.5, 4.0])                              # L takes millimetres to voxels
    field = np.zeros((3, 9, 8, 7), np.float32)
    for c in range(3):
        field[c] = shift[c] * spacing[c]
    L = np.diag(1.0 / spacing)
    got = DO.warp(src, None, EYE, L, field, None, src.shape, 1, 1, np.nan, 64)
    want = np.full(src.shape, np.nan)
    want[:7, 1:, :4] = src[2:, :7, 3:]
    # (an output whose upper neighbour falls outside blends NaN at weight 0: NaN, as section 4w has it)
    inside = ~np.isnan(got)
    assert inside.sum() == 6 * 7 * 3 and np.array_equal(got[inside], want[inside]) and not inside[6:].any() and not inside[:, 0].any()
    near = DO.warp(src, None, EYE, L, field, None, src.shape, 0, 1, -1.0)
    assert np.array_equal(near[:7, 1:, :4], src[2:, :7, 3:]) and (near[7:] == -1.0).all() and (near[:, 0] == -1.0).all() and (near[:, :, 4:] == -1.0).all()
    # the same field on a coarser field grid, looked up through F: a constant field blends to the same constant
    coarse = np.zeros((3, 3, 2, 2), np.float32)
    for c in range(3):
        coarse[c] = shift[c] * spacing[c]
    F = np.array([[0.25, 0, 0, 0], [0, 0.125, 0, 0], [0, 0, 0.15, 0.05]])
    assert np.array_equal(DO.warp(src, None, EYE, L, coarse, F, src.shape, 0, 1, -1.0), near)


# ---- the demons step ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_sign_a_ramp_shifted_by_a_moves_by_plus_a():
    """m(x) = f(x - a): the fixed point x is found at x + a of the moving image, so the first unsmoothed update is +a along x"""
    a = 0.75
    f = np.arange(16, dtype=np.float64).reshape(16, 1, 1) * 10.0
    m = f - 10.0 * a                                                # m(x) = f(x - a)
    zero = np.zeros((3, 16, 1, 1), np.float32)
    u = DO.demons_step(f, m, EYE, I3, I3, 1e6, zero)                # (a bound far above a: v = d g / |g|^2 = a)
    assert np.allclose(u[0], a, rtol=1e-6, atol=0) and not u[1].any() and not u[2].any()
    u = DO.demons_step(f, m, EYE, I3, I3, 1.0, zero)                # bounded: d g / (g^2 + d^2) -- the same sign, below delta / 2
    assert np.allclose(u[0], (10 * a * 10) / (100 + (10 * a) ** 2), rtol=1e-6) and (u[0] > 0).all() and (u[0] <= 0.5).all()
    # with that update applied the residual is gone: the moving sample at x + a is f(x), where it is still inside
    v, ok, mw = DO.demons_force(f, m, EYE, I3, I3, 1e6, np.stack([np.full((16, 1, 1), a, np.float32)] + [np.zeros((16, 1, 1), np.float32)] * 2))
    assert ok[:15].all() and not ok[15] and np.array_equal(mw[:15], f[:15]) and not np.any(v[0])          # (x = 15 looks at 15.75: outside)
    # an anisotropic, flipped grid: Ginv turns the index gradient into the world gradient, L the update back into voxels
    A = np.diag([-2.0, 1.0, 1.0])
    u = DO.demons_step(f, m, EYE, np.linalg.inv(A), np.linalg.inv(A).T, 1e6, zero)
    assert np.allclose(u[0], a * -2.0, rtol=1e-6)                   # a voxels along +x are a * (-2) mm of the world


def test_the_voxels_that_do_not_pull():
    rng = np.random.default_rng(8)
    f = rng.normal(size=(8, 6, 5)) * 100
    m = rng.normal(size=(8, 6, 5)) * 100
    zero = np.zeros((3, 8, 6, 5), np.float32)
    base, ok, _ = DO.demons_force(f, m, EYE, I3, I3, 2.0, zero)
    assert ok.all() and all(np.all(v != 0) for v in base)
    # the mask
    mask = (rng.random(f.shape) < 0.5).astype(np.uint8) * 3
    v, ok, _ = DO.demons_force(f, m, EYE, I3, I3, 2.0, zero, mask)
    assert np.array_equal(ok, mask != 0) and all(np.array_equal(v[c], np.where(mask != 0, base[c], 0.0)) for c in range(3))
    # NaN in f (and its neighbours: a NaN gradient is a NaN denominator) and in m
    fn = f.copy(); fn[3, 3, 2] = np.nan
    v, ok, _ = DO.demons_force(fn, m, EYE, I3, I3, 2.0, zero)
    out = np.zeros(f.shape, bool); out[3, 3, 2] = out[2, 3, 2] = out[4, 3, 2] = out[3, 2, 2] = out[3, 4, 2] = out[3, 3, 1] = out[3, 3, 3] = True
    assert np.array_equal(~ok, out) and all(not np.isnan(v[c]).any() and not v[c][out].any() for c in range(3))
    mn = m.copy(); mn[5, 1, 1] = np.nan
    v, ok, _ = DO.demons_force(f, mn, EYE, I3, I3, 2.0, zero)
    out = np.zeros(f.shape, bool); out[4:6, 0:2, 0:2] = True          # (a NaN neighbour makes the sample NaN even at weight 0, section 4w: the eight voxels that touch it)
    assert np.array_equal(~ok, out) and not np.isnan(np.stack(v)).any() and not np.stack(v)[:, out].any()
    # out of the moving volume: a shift of half a voxel puts the last x outside; exactly n - 1 is inside, one ulp beyond is not
    W = EYE.copy(); W[0, 3] = 0.5
    _, ok, _ = DO.demons_force(f, m, W, I3, I3, 2.0, zero)
    assert not ok[7].any() and ok[:7].all()
    top = np.array([[0.0, 0, 0, 7.0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    assert DO.demons_force(f, m, top, I3, I3, 2.0, zero)[1].all()
    top[0, 3] = np.nextafter(7.0, np.inf)
    assert not DO.demons_force(f, m, top, I3, I3, 2.0, zero)[1].any()
    # ... and the field can push a voxel out as well
    push = zero.copy(); push[1, :, 5, :] = 0.25
    _, ok, _ = DO.demons_force(f, m, EYE, I3, I3, 2.0, push)
    assert not ok[:, 5].any() and ok[:, :5].all()
    # a vanishing denominator: no gradient and no difference
    flat = np.full(f.shape, 40.0)
    v, ok, _ = DO.demons_force(flat, flat, EYE, I3, I3, 2.0, zero)
    assert not ok.any() and not np.stack(v).any()
    u = DO.demons_step(flat, flat, EYE, I3, I3, 2.0, push)
    assert np.array_equal(u, push)


# ---- the Jacobian --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_jacobian_of_a_linear_field_is_exact():
    B = np.array([[0.25, -0.5, 0.0], [0.125, 0.5, 0.25], [0.0, -0.25, -0.375]])          # dyadic: every product and sum below is exact
    A = np.diag([2.0, 4.0, 0.5])
    shape = (6, 5, 7)
    p = DO.world_points(shape, np.vstack([np.hstack([A, [[-8.0], [4.0], [16.0]]]), [0, 0, 0, 1]]))
    field = np.moveaxis(p @ B.T, -1, 0).astype(np.float32)           # u = B p
    assert np.array_equal(field.astype(np.float64), np.moveaxis(p @ B.T, -1, 0))
    det, folded = DO.jacobian(field, np.linalg.inv(A))
    want = np.float32(np.linalg.det(np.eye(3) + B))
    assert want == np.float32(1.2890625) and (det == want).all() and folded == 0          # (a linear field: the one-sided differences at the borders are exact too)
    # a fold: u_x = -1.5 x turns x over, det = 1 - 1.5 < 0 everywhere
    Bf = np.diag([-1.5, 0.0, 0.0])
    det, folded = DO.jacobian(np.moveaxis(p @ Bf.T, -1, 0).astype(np.float32), np.linalg.inv(A))
    assert (det == np.float32(-0.5)).all() and folded == det.size
    # folded in one place only, and a singular voxel (det = 0) counts
    field = np.zeros((3,) + shape, np.float32)
    field[0, 3, 2, 3] = -4.0                                        # x = 2 -> 3 loses 4 mm over 2 voxels of 2 mm: 1 - 1 = 0 at x = 2 and, from the other side, 1 + 1 at x = 4
    det, folded = DO.jacobian(field, np.linalg.inv(A))
    assert det[2, 2, 3] == 0.0 and det[4, 2, 3] == 2.0 and folded == 1
    # an axis of extent 1 has no derivative
    det, folded = DO.jacobian(np.random.default_rng(1).normal(size=(3, 1, 1, 1)).astype(np.float32), np.linalg.inv(A))
    assert det.shape == (1, 1, 1) and det[0, 0, 0] == 1.0 and folded == 0


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _centred(shape, pix, centre=(0.0, 0.0, 0.0)):
    A = np.diag([pix[0], pix[1], pix[2], 1.0])
    A[:3, 3] = np.asarray(centre) - A[:3, :3] @ ((np.asarray(shape) - 1) / 2.0)
    return A


def test_every_argument_error_is_a_value_error_before_any_device_work():
    from covidseg_amd import volume as V
    shape = (6, 5, 4)
    A = _centred(shape, (2.0, 2.0, 2.0))
    vol = np.zeros(shape, np.int16)
    ops = DO.OracleOps()
    ok = dict(levels_mm=(4, 2), iterations=(1, 1), fixed_affine=A, moving_affine=A, ops=ops)
    V.refine_registration(vol, vol, np.eye(4), **ok)                # (the call itself is sound)
    bad = [dict(levels_mm=()), dict(levels_mm=(2, 4)), dict(levels_mm=(4, 4)), dict(levels_mm=(4, -2)), dict(levels_mm=(np.nan, 2)), dict(levels_mm=4),
           dict(iterations=(1,)), dict(iterations=(1, 2, 3)), dict(iterations=(1, -1)), dict(iterations=(1, 1.5)), dict(iterations=(True, 1)), dict(iterations=3),
           dict(field_sigma=-1), dict(field_sigma=np.nan), dict(field_sigma="2"), dict(field_sigma=11), dict(image_sigma=-0.5), dict(image_sigma=np.inf),
           dict(image_sigma=20), dict(max_step=0), dict(max_step=-1), dict(max_step=np.nan), dict(max_step="1"), dict(max_step=True),
           dict(mask=np.zeros((6, 5, 3), np.uint8)), dict(mask=np.zeros(shape, np.float32)), dict(fixed_affine=None), dict(moving_affine=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            V.refine_registration(vol, vol, np.eye(4), **{**ok, **kw})
    for rigid in (None, np.eye(3), np.zeros((4, 4)), np.full((4, 4), np.nan), "identity"):
        with pytest.raises(ValueError):
            V.refine_registration(vol, vol, rigid, **ok)
    with pytest.raises(ValueError):
        V.refine_registration(np.zeros((6, 5), np.int16), vol, np.eye(4), **ok)
    # register_volumes(deformable=) is checked before the rigid search starts
    for d in (False, 1, "yes", dict(levels=(4, 2)), dict(iterations=(1,)), dict(field_sigma=-1), dict(mask=None)):
        with pytest.raises(ValueError):
            V.register_volumes(vol, vol, fixed_affine=A, moving_affine=A, deformable=d)
    # the field's own surface
    g = V.Grid(shape, A)
    fld = V.DisplacementField(np.zeros(3 * 120, np.float32), g, np.eye(4), g, V.Grid((7, 5, 4), _centred((7, 5, 4), (2.0, 2.0, 2.0))))
    assert fld.field_matrix is None and fld.host().shape == (3,) + shape
    for kw in (dict(kind="image"), dict(kind="labels", order="linear"), dict(order="cubic"), dict(mode="wrap"), dict(dtype="int16"), dict(order="nearest"), dict(cval="air")):
        with pytest.raises(ValueError):
            fld.resample(np.zeros((7, 5, 4), np.int16), **kw)
    with pytest.raises(ValueError):
        fld.resample(vol)                                           # not on the moving grid
    with pytest.raises(ValueError):
        fld.resample(np.zeros((7, 5, 4), np.float32), kind="mask")
    with pytest.raises(ValueError):
        V.DisplacementField(np.zeros(360, np.float32), g, np.eye(4), g, V.Grid(shape, A, oriented=False))
    # change_between takes the deformable result only on the grids it was found on
    reg = V.DeformableRegistration(field=fld)
    other = V.Grid(shape, _centred(shape, (2.0, 2.0, 2.5)))
    with pytest.raises(ValueError):
        V.change_between(np.zeros(shape, np.uint8), other, np.zeros((7, 5, 4), np.uint8), fld.moving_grid, transform=reg)
    with pytest.raises(ValueError):
        V.change_between(np.zeros(shape, np.uint8), g, np.zeros(shape, np.uint8), g, transform=reg)


# ---- the header and the bindings ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_four_entries_are_declared_bound_and_exported_under_abi_16():
    import ctypes
    from covidseg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    assert re.search(r"#define UNET_ABI_VERSION 16\b", hdr) and _lib.ABI_VERSION == 16
    assert int(re.search(r"#define UNET_VOL_SMOOTH_MAX_RADIUS (\d+)", hdr).group(1)) == _lib.SMOOTH_MAX_RADIUS == 32
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name, argc in ENTRIES.items():
        m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code)
        assert m and m.group(1).count(",") + 1 == argc, name
        restype, args = _lib._PROTOS[name]
        assert restype is ctypes.c_int32 and len(args) == argc and args[0] is ctypes.c_void_p and args[-1] is ctypes.c_void_p
    lib = _lib.load()
    assert lib.unet_abi_version() == 16
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    assert src.count("kernels_deform") >= 5                          # SRCS, the -ffp-contract=off list, the two sanitizer lists, the header dependency


# ---- the whole loop over the oracle ---------------------------------------------------------------------------------------------------------------------------------------
RATIO_CAP = 0.60                                                    # the oracle's measured ratio, rounded up to the next 0.05


def test_the_loop_recovers_a_known_field_on_the_phantom():
    from covidseg_amd import volume as V
    case = DO.phantom_case()
    reg = V.refine_registration(case.fixed, case.moving, case.rigid, levels_mm=(4, 2), fixed_affine=case.fixed_affine, moving_affine=case.moving_affine, ops=DO.OracleOps())
    assert [h["shape"] for h in reg.history] == [(20, 18, 18), (40, 36, 36)] and [h["iterations"] for h in reg.history] == [30, 15]
    assert reg.field.grid.shape == case.fixed.shape
    u = np.moveaxis(reg.field.host().astype(np.float64), 0, -1)
    big = np.linalg.norm(case.u_true, axis=-1) > 1.0
    rigid_only = float(np.linalg.norm(case.u_true, axis=-1)[big].mean())
    refined = float(np.linalg.norm(u - case.u_true, axis=-1)[big].mean())
    print(f"residual {reg.residual_init:.3f} -> {reg.residual:.3f} HU; endpoint error over {int(big.sum())} voxels {rigid_only:.4f} -> {refined:.4f} mm: ratio {refined / rigid_only:.4f}; "
          f"jacobian [{reg.jacobian_min:.4f}, {reg.jacobian_max:.4f}], folded {reg.folded}, {reg.seconds:.2f} s")
    assert big.sum() > 1000
    assert reg.residual < reg.residual_init
    assert refined < rigid_only
    assert refined / rigid_only <= RATIO_CAP
    assert reg.folded == 0 and reg.jacobian_min > 0

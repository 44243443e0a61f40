"""CPU: the host side of covidseg_amd.volume's registration -- mutual_information against scikit-learn, RigidTransform against matrix algebra,
the properties of tests/register_oracle.py, the pattern search of rigid_search over the oracle evaluator on an analytic phantom, and every refusal; no device."""
import os

import numpy as np
import pytest

import lungside_oracle as LO
import register_oracle as RO
import resample_oracle as RS
from covidseg_amd import _lib
from covidseg_amd import volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- mutual_information --------------------------------------------------------------------------------------------------------------------------------
def test_mutual_information_equals_sklearn():
    from sklearn.metrics import mutual_info_score
    rng = np.random.default_rng(3)
    hists = [rng.integers(0, 50, (8, 8)).astype(np.uint32), (rng.integers(0, 1000, (32, 32)) * (rng.random((32, 32)) < 0.2)).astype(np.uint32),
             np.diag(np.arange(1, 17)).astype(np.uint32), np.full((4, 4), 7, np.uint32)]
    h = np.zeros((64, 64), np.uint32); h[3, 5] = 2 ** 31 - 1; h[60, 1] = 12345; h[3, 1] = 1
    hists.append(h)
    for h in hists:
        assert abs(V.mutual_information(h) - mutual_info_score(None, None, contingency=h.astype(np.int64))) < 1e-12
    # from the counts alone: the same value for any integer dtype, and for a stack
    stack = np.stack([hists[1], hists[1].T])
    got = V.mutual_information(stack)
    assert got.shape == (2,) and got[0] == V.mutual_information(hists[1].astype(np.int64)) and abs(got[0] - got[1]) < 1e-12


def test_mutual_information_of_special_histograms():
    assert V.mutual_information(np.zeros((32, 32), np.uint32)) == float("-inf")
    assert V.mutual_information(np.zeros((32, 32), np.uint32), normalized=True) == float("-inf")
    one = np.zeros((4, 4), np.uint32); one[2, 1] = 9                 # every voxel in one cell: no information either way
    assert V.mutual_information(one) == 0.0 and V.mutual_information(one, normalized=True) == 1.0
    d = np.diag([5, 5, 5, 5]).astype(np.uint32)                      # one determines the other: MI = H = log 4, NMI = 2
    assert abs(V.mutual_information(d) - np.log(4.0)) < 1e-15 and abs(V.mutual_information(d, normalized=True) - 2.0) < 1e-15
    ind = np.outer([1, 2, 3], [4, 5, 6]).astype(np.uint32)           # independent: MI = 0, NMI = 1
    assert abs(V.mutual_information(ind)) < 1e-15 and abs(V.mutual_information(ind, normalized=True) - 1.0) < 1e-15
    for bad in (np.zeros((3, 4), np.uint32), np.zeros(4, np.uint32), np.zeros((4, 4), np.float64), -np.ones((4, 4), np.int32)):
        with pytest.raises(ValueError):
            V.mutual_information(bad)


# ---- RigidTransform ------------------------------------------------------------------------------------------------------------------------------------
def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {0: np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), 1: np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), 2: np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float64)


def test_rigid_transform_is_its_definition():
    p, c = (5.3, -3.7, 4.1, 0.075, -0.045, 0.117), np.array([10.0, -20.0, 30.0])
    T = V.RigidTransform(p, c)
    R = _rot(2, p[5]) @ _rot(1, p[4]) @ _rot(0, p[3])
    assert np.array_equal(T.rotation, R)
    for x in (np.zeros(3), c, np.array([1.0, 2.0, 3.0]), np.array([-40.0, 55.0, 7.5])):
        want = R @ (x - c) + c + np.asarray(p[:3])
        assert np.allclose((T.matrix @ np.append(x, 1.0))[:3], want, rtol=0, atol=1e-12)
    assert np.array_equal(T.matrix[3], [0, 0, 0, 1]) and abs(np.linalg.det(T.matrix[:3, :3]) - 1.0) < 1e-15
    # identity parameters -> the identity matrix exactly, about any centre
    for centre in ((0, 0, 0), (10.5, -20.25, 1e3), (0.1, 0.2, 0.3)):
        assert np.array_equal(V.RigidTransform((0,) * 6, centre).matrix, np.eye(4))
    assert np.array_equal(V.RigidTransform().matrix, np.eye(4))


def test_rigid_transform_round_trips_inverts_and_composes():
    rng = np.random.default_rng(8)
    for _ in range(20):
        p = np.concatenate([rng.uniform(-50, 50, 3), rng.uniform(-1.2, 1.2, 3)])
        c, c2 = rng.uniform(-100, 100, 3), rng.uniform(-100, 100, 3)
        T = V.RigidTransform(p, c)
        back = V.RigidTransform.from_matrix(T.matrix, c)
        assert np.allclose(back.params, p, rtol=0, atol=1e-12) and np.array_equal(back.centre, c)
        other = V.RigidTransform.from_matrix(T.matrix, c2)           # the same motion about another centre: other parameters, the same matrix
        assert np.allclose(other.matrix, T.matrix, rtol=0, atol=1e-10) and np.allclose(other.params[3:], p[3:], rtol=0, atol=1e-12)
        inv = T.inverse()
        assert np.allclose(inv.matrix, np.linalg.inv(T.matrix), rtol=0, atol=1e-10) and np.allclose(inv.matrix @ T.matrix, np.eye(4), rtol=0, atol=1e-10)
        assert np.array_equal(inv.centre, c)
        U = V.RigidTransform(np.concatenate([rng.uniform(-50, 50, 3), rng.uniform(-0.3, 0.3, 3)]), c2)
        assert np.allclose(T.compose(U).matrix, T.matrix @ U.matrix, rtol=0, atol=1e-10)          # T after U
        assert np.allclose(T.compose(T.inverse()).matrix, np.eye(4), rtol=0, atol=1e-10)
    for bad in (np.diag([2.0, 1.0, 1.0, 1.0]), np.diag([-1.0, 1.0, 1.0, 1.0]), np.eye(4) + np.eye(4, k=1) * 0.1):          # a zoom, a mirror, a shear
        with pytest.raises(ValueError, match="rigid"):
            V.RigidTransform.from_matrix(bad)
    for bad in ((1, 2, 3), (1, 2, 3, 4, 5, np.nan), "abc"):
        with pytest.raises(ValueError):
            V.RigidTransform(bad)
    with pytest.raises(ValueError):
        V.RigidTransform((0,) * 6, (1, 2))


def test_voxel_matrix_is_the_stated_product():
    A, B = LO.affine_of(("L", "P", "S"), (0.7, 0.7, 2.5)), RS.oblique_affine((1.1, 0.9, 1.3))
    gf, gm = V.Grid((9, 8, 7), A), V.Grid((6, 5, 4), B)
    T = V.RigidTransform((1, 2, 3, 0.1, 0.2, 0.3), (4, 5, 6))
    assert np.array_equal(V.voxel_matrix(gf, gm, T), (np.linalg.inv(B) @ T.matrix @ A)[:3])
    assert np.array_equal(V.voxel_matrix(gf, gm), (np.linalg.inv(B) @ np.eye(4) @ A)[:3])
    assert np.array_equal(V.voxel_matrix(gf, gm, T.matrix), V.voxel_matrix(gf, gm, T))


# ---- the oracle's properties ---------------------------------------------------------------------------------------------------------------------------
def test_identity_on_equal_volumes_is_a_diagonal_that_counts_every_voxel():
    v = np.random.default_rng(5).uniform(-1100.0, 500.0, (7, 6, 5))
    h = RO.joint_hist(v, v, np.eye(4)[:3][None], 32, (-1000, 400))
    assert h.shape == (1, 32, 32) and h.dtype == np.uint32 and h.sum() == v.size
    assert np.array_equal(h[0], np.diag(np.diag(h[0]))) and h[0, 0, 0] > 0 and h[0, 31, 31] > 0          # both clamps occur
    assert np.array_equal(np.diag(h[0]), np.bincount(RO.bin_of(v, 32, (-1000, 400)).ravel(), minlength=32))


def test_a_shift_that_puts_everything_outside_counts_nothing():
    v = np.random.default_rng(6).uniform(-1000.0, 400.0, (7, 6, 5))
    far = np.eye(4)[:3].copy(); far[:, 3] = 4000.0
    edge = np.eye(4)[:3].copy(); edge[0, 3] = np.nextafter(0.0, -1.0)          # x = 0 falls one ulp below 0: that column is out, the rest is in
    h = RO.joint_hist(v, v, np.stack([far, np.eye(4)[:3], edge]), 16, (-1000, 400))
    assert h[0].sum() == 0 and h[1].sum() == v.size and h[2].sum() == v.size - 30


def test_the_mask_and_nan_exclusions():
    rng = np.random.default_rng(7)
    f, m = rng.uniform(-1000.0, 400.0, (7, 6, 5)), rng.uniform(-1000.0, 400.0, (7, 6, 5))
    eye = np.eye(4)[:3][None]
    mask = (rng.random(f.shape) < 0.5).astype(np.uint8) * 3
    full = RO.joint_hist(f, m, eye, 8, (-1000, 400))
    assert RO.joint_hist(f, m, eye, 8, (-1000, 400), mask=mask).sum() == np.count_nonzero(mask)
    assert np.array_equal(RO.joint_hist(f, m, eye, 8, (-1000, 400), mask=np.ones_like(mask)), full)
    fn = f.copy(); fn[2, 3, 1] = np.nan                              # a NaN fixed voxel: that voxel alone
    assert RO.joint_hist(fn, m, eye, 8, (-1000, 400)).sum() == f.size - 1
    mn = m.copy(); mn[2, 3, 1] = np.nan                              # a NaN moving voxel at the identity: the voxel itself and the seven whose upper neighbours (weight 0) include it
    assert RO.joint_hist(f, mn, eye, 8, (-1000, 400)).sum() == f.size - 8
    mi = m.copy(); mi[3, 2, 2] = np.inf; mi[5, 4, 3] = -np.inf        # +-inf samples clamp into the end bins -- where the inf is the upper neighbour on every axis; as a lower
    half = np.eye(4)[:3].copy(); half[:, 3] = 0.5                     # neighbour, or at weight 0, a + (b - a) w makes inf - inf or inf * 0 = NaN, which is not counted
    for M in (np.eye(4)[:3], half):
        ok, sample = RO.counted(f, mi, M)
        h = RO.joint_hist(f, mi, M[None], 8, (-1000, 400))
        assert h.sum() == np.count_nonzero(ok) and np.isnan(sample).any()
    assert np.isposinf(sample[ok]).sum() >= 1 and np.isneginf(sample[ok]).sum() >= 1 and h[0, :, 7].sum() >= 1 and h[0, :, 0].sum() >= 1
    # two windows: the moving one bins the columns
    h2 = RO.joint_hist(f, m, eye, 8, (-1000, 400), (-500, 0))
    assert np.array_equal(h2[0].sum(axis=1), full[0].sum(axis=1)) and not np.array_equal(h2[0].sum(axis=0), full[0].sum(axis=0))


# ---- the search over the oracle evaluator -----------------------------------------------------------------------------------------------------------------
FIXED_SHAPE, FIXED_PIX = (40, 36, 28), (2.0, 2.0, 2.5)
MOVING_SHAPE, MOVING_PIX = (44, 40, 24), (1.8, 1.8, 3.0)
TRUE_MOTION = (5.3, -3.7, 4.1) + tuple(np.deg2rad([4.3, -2.6, 6.7]))          # off the search lattice on purpose


def _centred(shape, pix, centre=(0.0, 0.0, 0.0)):
    A = np.diag([pix[0], pix[1], pix[2], 1.0])
    A[:3, 3] = np.asarray(centre) - A[:3, :3] @ ((np.asarray(shape) - 1) / 2.0)
    return A


def _search_once():
    Af, Am = _centred(FIXED_SHAPE, FIXED_PIX), _centred(MOVING_SHAPE, MOVING_PIX, (3.0, -2.0, 2.5))
    truth = V.RigidTransform(TRUE_MOTION, (0.0, 0.0, 0.0))
    fixed = RO.phantom(FIXED_SHAPE, Af, 1)
    moving = RO.phantom(MOVING_SHAPE, np.linalg.inv(truth.matrix) @ Am, 2)          # the patient moved by `truth`, other noise
    fg, mg = V.Grid(FIXED_SHAPE, Af), V.Grid(MOVING_SHAPE, Am)
    levels = []
    for L, g, M in V.registration_level_grids(fg, (8, 4, 2)):
        fd = fixed if M is None else RS.linear(fixed, M, g.shape, 0, 0.0, 16).astype(np.float64)
        levels.append(V.RegistrationLevel(L, g, int(np.prod(g.shape)), lambda Ms, fd=fd: RO.joint_hist(fd, moving, Ms, 32, (-1000, 400))))
    return V.rigid_search(levels, fg, mg), truth, fg, mg


def test_the_search_recovers_an_off_lattice_motion_to_sub_voxel():
    """Measured on this phantom: largest corner error 10.65 mm at the start ("geometry"), 0.565 mm at the result, in 54 batches / 653 histograms; MI 0.5950 -> 1.1818
    (at the truth: 1.1875)."""
    reg, truth, fg, mg = _search_once()
    before = RO.corner_error(V.initial_transform(fg, mg).matrix, truth.matrix, FIXED_SHAPE, fg.affine)
    after = RO.corner_error(reg.transform.matrix, truth.matrix, FIXED_SHAPE, fg.affine)
    print(f"corner error {before:.3f} mm -> {after:.3f} mm, metric {reg.metric_init:.4f} -> {reg.metric:.4f}, batches {reg.batches}, evaluations {reg.evaluations}")
    assert before > 5.0                                              # the test cannot pass at the start
    assert after < 0.5 * min(FIXED_PIX)                              # sub-voxel: below half the smallest fixed voxel spacing
    assert reg.metric > reg.metric_init and reg.converged and 0.25 <= reg.overlap <= 1.0
    assert [h["shape"] for h in reg.history] == [(10, 9, 9), (20, 18, 18), FIXED_SHAPE] and [h["spacing"] for h in reg.history] == [8.0, 4.0, 2.0]
    assert sum(h["batches"] for h in reg.history) == reg.batches and reg.evaluations == 12 * reg.batches + 3 + 2
    assert np.array_equal(reg.voxel_matrix, (np.linalg.inv(mg.affine) @ reg.transform.matrix @ fg.affine)[:3])
    assert np.array_equal(reg.transform.centre, [0.0, 0.0, 0.0])
    again = _search_once()[0]                                        # deterministic: the same inputs give the same transform
    assert np.array_equal(again.transform.params, reg.transform.params) and again.metric == reg.metric and again.batches == reg.batches


def test_the_search_rules():
    """ties go to the lowest index, a move needs a strict improvement, a poor overlap scores -inf, max_batches ends the search"""
    g = V.Grid((8, 8, 8), np.eye(4))
    flat = np.zeros((12, 4, 4), np.uint32); flat[:, 0, 0] = 100; flat[:, 1, 1] = 100
    calls = []

    def constant(Ms):                                                # every candidate scores the same: nothing is strictly better, the steps halve to the end
        calls.append(len(Ms))
        return flat[:len(Ms)]

    reg = V.rigid_search([V.RegistrationLevel(2.0, g, 200, constant)], g, g, init="identity")
    assert np.array_equal(reg.transform.params, np.zeros(6)) and reg.converged and reg.metric == reg.metric_init
    assert reg.batches == 6 and calls == [1] + [12] * 6 + [1, 1]      # steps 4, 2, 1, 0.5, 0.25, 0.125 mm; 0.0625 < 0.05 * 2 ends the level

    def prefers_plus_y_and_minus_rz(Ms):                              # candidates 2 (+ty) and 11 (-rz) tie for the best on the first batch: index 2 is taken
        h = flat[:len(Ms)].copy()
        if len(Ms) == 12 and not prefers_plus_y_and_minus_rz.moved:
            h[2] = h[11] = np.diag([50, 50, 50, 50]).astype(np.uint32)
            prefers_plus_y_and_minus_rz.moved = True
        return h
    prefers_plus_y_and_minus_rz.moved = False
    reg = V.rigid_search([V.RegistrationLevel(2.0, g, 200, prefers_plus_y_and_minus_rz)], g, g, init="identity")
    assert np.array_equal(reg.transform.params, [0.0, 4.0, 0.0, 0.0, 0.0, 0.0])

    def better_but_thin(Ms):                                          # a better histogram from too few voxels never wins
        h = flat[:len(Ms)].copy()
        if len(Ms) == 12:
            h[0] = np.diag([10, 10, 10, 10]).astype(np.uint32)       # 40 < 0.25 * 200
        return h
    reg = V.rigid_search([V.RegistrationLevel(2.0, g, 200, better_but_thin)], g, g, init="identity")
    assert np.array_equal(reg.transform.params, np.zeros(6))
    reg = V.rigid_search([V.RegistrationLevel(2.0, g, 200, constant)], g, g, init="identity", max_batches=3)
    assert reg.batches == 3 and not reg.converged


def test_initial_transform_and_level_grids():
    Af, Am = _centred(FIXED_SHAPE, FIXED_PIX, (1.0, 2.0, 3.0)), _centred(MOVING_SHAPE, MOVING_PIX, (4.0, -2.0, 2.5))
    fg, mg = V.Grid(FIXED_SHAPE, Af), V.Grid(MOVING_SHAPE, Am)
    t = V.initial_transform(fg, mg)
    assert np.allclose(t.centre, [1.0, 2.0, 3.0], rtol=0, atol=1e-12) and np.allclose(t.params, [3.0, -4.0, -0.5, 0, 0, 0], rtol=0, atol=1e-12)
    assert np.array_equal(V.initial_transform(fg, mg, "identity").matrix, np.eye(4))
    given = V.RigidTransform((1, 2, 3, 0.1, 0.0, -0.1), (50, 50, 50))
    assert np.allclose(V.initial_transform(fg, mg, given).matrix, given.matrix, rtol=0, atol=1e-10)
    grids = V.registration_level_grids(fg, (8, 4, 2, 1))
    assert [g.shape for _, g, _ in grids] == [(10, 9, 9), (20, 18, 18), FIXED_SHAPE, FIXED_SHAPE]
    assert grids[2][1] is fg and grids[2][2] is None and grids[3][2] is None          # 2 mm does not exceed the smallest spacing: the volume itself
    assert np.allclose(grids[0][1].pixdim, (8.0, 8.0, 70.0 / 9), rtol=0, atol=1e-12)
    for _, g, _ in grids:                                            # every level covers the same field of view
        assert np.allclose(V._grid_centre(g), [1.0, 2.0, 3.0], rtol=0, atol=1e-9)


# ---- refusals and declarations ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_fires_without_a_device():
    a = np.zeros((4, 5, 6), np.int16)
    A = LO.affine_of(("L", "P", "S"))
    ok = dict(fixed_affine=A, moving_affine=A)
    for fn in (V.joint_histogram, V.register_volumes):
        with pytest.raises(ValueError, match="orientation"):
            fn(a, a, moving_affine=A)                               # the fixed volume is unoriented
        with pytest.raises(ValueError, match="orientation"):
            fn(a, a, fixed_affine=A)                                # the moving one is
        for kw in ({"bins": 1}, {"bins": 65}, {"bins": 32.0}, {"bins": True}, {"window": (400, -1000)}, {"window": (0, 0)}, {"window": (0, np.inf)}, {"window": (np.nan, 1)},
                   {"window": (1, 2, 3)}, {"window": "lung"}, {"moving_window": (5, 5)}, {"window": (-1e308, 1e308)}, {"mask": np.zeros((4, 5, 5), np.uint8)},
                   {"mask": np.zeros((4, 5, 6), np.float32)}):
            with pytest.raises(ValueError):
                fn(a, a, **ok, **kw)
        with pytest.raises(ValueError):
            fn(np.zeros((4, 5), np.int16), a, **ok)
    for kw in ({"transforms": np.eye(3)}, {"transforms": []}, {"transforms": [np.full((4, 4), np.nan)]}, {"transforms": np.zeros((4, 4))}, {"transforms": "identity"}):
        with pytest.raises(ValueError):
            V.joint_histogram(a, a, **ok, **kw)
    for kw in ({"levels_mm": ()}, {"levels_mm": (2, 4)}, {"levels_mm": (4, 4)}, {"levels_mm": (4, 0)}, {"levels_mm": 4}, {"init": "centre"}, {"init": np.eye(4)},
               {"min_overlap": 0}, {"min_overlap": 1.5}, {"min_overlap": "half"}, {"max_batches": 0}, {"max_batches": 2.5}, {"metric": "ncc"}):
        with pytest.raises(ValueError):
            V.register_volumes(a, a, **ok, **kw)
    with pytest.raises(ValueError, match="non-finite"):              # two finite affines whose product overflows
        far = np.eye(4); far[:3, 3] = 1e250
        V.joint_histogram(a, a, fixed_affine=far, moving_affine=np.diag([1e-100, 1e-100, 1e-100, 1.0]))
    g = V.Grid((4, 5, 6), A)
    with pytest.raises(ValueError):
        V.rigid_search([], g, g)
    with pytest.raises(ValueError, match="orientation"):
        V.rigid_search([V.RegistrationLevel(2.0, g, 120, lambda Ms: None)], g, V.Grid.of(a))
    mask = np.zeros((4, 5, 6), np.uint8)
    for bad in (np.zeros((4, 4)), np.eye(3), "rigid", np.full((4, 4), np.inf)):
        with pytest.raises(ValueError):
            V.change_between(mask, g, mask, g, transform=bad)
    reg = V.Registration(transform=V.RigidTransform(), fixed_grid=g, moving_grid=g)
    for kw in ({"kind": "image"}, {"grid": g}, {"spacing": (1, 1, 1)}, {"affine": A}):
        with pytest.raises(ValueError):
            reg.resample(a, **kw)
    with pytest.raises(ValueError):
        reg.resample(a, order="cubic")


def test_the_declarations_and_bindings_exist():
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    assert "int32_t unet_vol_joint_hist(" in hdr
    assert len(_lib._PROTOS["unet_vol_joint_hist"][1]) == 27 and "unet_vol_joint_hist" in _lib.EXPORTED_SYMBOLS
    assert f"#define UNET_VOL_JOINT_HIST_MAX_K {_lib.JOINT_HIST_MAX_K}\n" in hdr and f"#define UNET_VOL_JOINT_HIST_MAX_BINS {_lib.JOINT_HIST_MAX_BINS}\n" in hdr
    assert (V.JOINT_HIST_MAX_K, V.JOINT_HIST_MAX_BINS) == (16, 64)
    mk = open(os.path.join(os.path.dirname(V.__file__), "csrc", "Makefile")).read()
    assert "kernels_register.hip" in mk.split("SRCS =")[1].split("\n")[0]
    assert all("kernels_register.o" in line for line in mk.splitlines() if line.endswith("EXTRA = -ffp-contract=off"))
    assert _lib.ABI_VERSION == 16 and "#define UNET_ABI_VERSION 16" in hdr

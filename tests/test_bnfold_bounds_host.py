"""CPU: the per-element checks of test_gpu_bnfold_elem.py (tests/bnfold_checks.py) can fail.  "got" is the float64 reference rounded to fp32 -- it must pass every
check with a ratio below 0.1 -- and then carries ONE defect of the kind the kernels of the BatchNorm -> conv3x3 fold could have; each must be rejected by the check
of its launch.  Also pins the references themselves: the two formulations of the forward agree, the dispatch transcription reaches every arm, and the
dx = f(x) (K0 dz + K1 x + K2) formula is torch.autograd's gradient through a training-mode BatchNorm."""
import numpy as np
import pytest
import torch

import bnfold_checks as B


def f32(t):
    return t.to(torch.float32).to(torch.float64)


@pytest.fixture(scope="module")
def fwd():
    case = B.make_case(2, 5, 9, 64, 32, "bn", 11)
    return case, B.fwd_problem(case)


@pytest.fixture(scope="module")
def wg():
    case = B.make_case(5, 5, 5, 64, 16, "bn", 12)
    return case, B.wgrad_problem(case)


@pytest.fixture(scope="module")
def dg():
    case = B.make_case(2, 5, 9, 64, 32, "bn", 13)
    x, mean, istd = (B.t64(case[v]) for v in ("x", "mean", "istd"))
    sums = B.exact_sums(B.dgrad64(B.t64(case["dy"]), B.t64(case["k"])), x, mean, istd)
    return case, sums


def rejected(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def test_forward_reference_has_two_formulations_and_the_rounded_one_passes(fwd):
    case, P = fwd
    x, k, b, sc, sh = (B.t64(case[v]) for v in ("x", "k", "b", "scale", "shift"))
    tab = B.bias_table64(k, b, sh)
    folded = B.conv64(x, k * sc[None, None, :, None]) + tab[torch.as_tensor(P["cls"])]
    assert float((folded - P["pre"]).abs().max()) < 1e-12 * float(P["a1"].max())
    from gpu_util import conv_abs_sums
    a1 = conv_abs_sums(case["x"], (k * sc[None, None, :, None]).numpy(), np.zeros_like(case["dy"]), with_floor=False)["y_a1"]
    assert np.abs(a1 - P["a1"].numpy()).max() < 1e-12 * a1.max()
    for act in (0, 1):
        assert B.check_fwd(f32(P["pre"].clamp_min(0.0) if act else P["pre"]), P, act, "host fwd") < 0.1


def test_a_corner_that_takes_the_edge_row_of_the_table_is_rejected(fwd):
    case, P = fwd
    tab = B.bias_table64(*(B.t64(case[v]) for v in ("k", "b", "shift")))
    got = f32(P["pre"]).clone()
    got[:, 0, 0] += tab[4] - tab[5]                          # pixel (0, 0) is class 4 * 1 + 1; class 4 is the first row away from the corners
    rejected(B.check_fwd, got, P, 0, "host fwd corner")
    got = f32(P["pre"]).clone()
    got[:, -1, -1] += tab[2] - tab[10]                       # (H-1, W-1): class 4 * 2 + 2 takes the last column's row
    rejected(B.check_fwd, got.clamp_min(0.0), P, 1, "host fwd corner")


def test_scale_on_the_wrong_channel_block_is_rejected(fwd, wg):
    case, P = fwd
    x, k, b, sc, sh = (B.t64(case[v]) for v in ("x", "k", "b", "scale", "shift"))
    tab = B.bias_table64(k, b, sh)
    got = B.conv64(x, k * torch.roll(sc, 32)[None, None, :, None]) + tab[torch.as_tensor(P["cls"])]
    rejected(B.check_fwd, f32(got), P, 0, "host fwd block")
    case, W = wg
    sc, sh = B.t64(case["scale"]), B.t64(case["shift"])
    dw = torch.roll(sc, 32)[None, None, :, None] * W["dw_raw"] + sh[None, None, :, None] * W["S"][:, :, None, :]
    rejected(B.check_wgrad, f32(dw), f32(W["db"]), W, "host wgrad block")


def test_weight_gradient_rounded_passes_and_tap_sum_defects_are_rejected(wg):
    case, W = wg
    assert max(B.check_wgrad(f32(W["dw"]), f32(W["db"]), W, "host wgrad")) < 0.1
    pre = torch.linspace(-3.0, 5.0, W["sums"].numel(), dtype=torch.float64)
    assert max(B.check_bn_sums(W["sums"] + pre, pre, W, "host sums")) < 0.1
    rejected(B.check_bn_sums, W["sums"], pre, W, "host sums overwritten")          # (sums that were not ADDED to)
    sc, sh, dy = (B.t64(case[v]) for v in ("scale", "shift", "dy"))

    def dw_with(S):
        return f32(sc[None, None, :, None] * W["dw_raw"] + sh[None, None, :, None] * S[:, :, None, :])

    assert case["shape"][0] * 4 > 16
    for kw in (dict(corner=False), dict(swap_rows=True), dict(images=slice(0, 4))):          # no corner term; first <-> last row; the entries from 16 on (images 4 ...) left out
        S = B.tap_terms64(dy, **kw)[4]
        rejected(B.check_wgrad, dw_with(S), f32(W["db"]), W, f"host wgrad {kw}")


def test_taps_outside_a_one_row_image_are_held_to_the_residue_of_S():
    case = B.make_case(5, 1, 7, 16, 16, "bn", 14)
    W = B.wgrad_problem(case)
    assert W["outside"][0].all() and W["outside"][2].all() and not W["outside"][1].any()
    assert max(B.check_wgrad(f32(W["dw"]), f32(W["db"]), W, "host one-row")) < 0.1
    got = f32(W["dw"]).clone()
    got[0, 1] += 1e-3 * B.t64(case["shift"])[:, None].abs()                        # far beyond shift * (rounding residue of S)
    rejected(B.check_wgrad, got, f32(W["db"]), W, "host one-row residue")


@pytest.mark.parametrize("mode,producer", [(0, "none"), (1, "relu"), (2, "elu"), (3, "elu_drop")])
def test_data_gradient_formula_is_autograd_and_its_defects_are_rejected(mode, producer):
    case = B.make_case(2, 5, 9, 64, 32, "bn", 20 + mode, producer=producer, rate=0.25, drop_seed=77)
    g, sc64, mean64, istd64 = B.bn_train_dx_autograd(case)
    c64 = dict(case, scale=sc64.numpy(), mean=mean64.numpy(), istd=istd64.numpy())
    x = B.t64(case["x"])
    dz = B.dgrad64(B.t64(case["dy"]), B.t64(case["k"]))
    P0 = B.dgrad_problem(c64, B.exact_sums(dz, x, mean64, istd64))
    assert float((P0["ref"] - g).abs().max()) < 1e-10 * float(g.abs().max())       # the formula (signs included) IS the gradient through the training-mode BatchNorm
    sums = B.exact_sums(dz, x, B.t64(case["mean"]), B.t64(case["istd"]))
    P = B.dgrad_problem(case, sums, mode, 0.25, 77)
    if mode:
        f = B.mask_factor64(x, mode, 0.25, 77)
        assert float((P["ref"] - f * B.dgrad_problem(case, sums)["ref"]).abs().max()) == 0.0 and 0.05 < float((f == 0).double().mean() if mode != 2 else (f < 1).double().mean()) < 0.95
    assert B.check_dgrad(f32(P["ref"]), P, f"host dgrad mode {mode}") < 0.1
    rejected(B.check_dgrad, f32(B.dgrad_problem(case, sums, mode, 0.25, 77, drop_k2=True)["ref"]), P, "host dgrad without K2")


def test_k1_x_above_x_channels_is_rejected(dg):
    case, sums = dg
    P = B.dgrad_problem(case, sums, x_channels=32)
    assert B.check_dgrad(f32(P["ref"]), P, "host dgrad limit") < 0.1
    rejected(B.check_dgrad, f32(B.dgrad_problem(case, sums, x_channels=32, ignore_limit=True)["ref"]), P, "host dgrad K1 x above the limit")
    nan = dict(case, x=case["x"].copy()); nan["x"][..., 32:] = np.nan            # the reference never reads x above the limit
    assert float((B.dgrad_problem(nan, sums, x_channels=32)["ref"] - P["ref"]).abs().max()) == 0.0


def test_dispatch_transcription_reaches_every_arm():
    for cu in (256, 304, 64):
        seen = {B.h2_arm(cu, 1, 5, 9, 64)}
        for arm in B.ARMS[1:]:
            n, h, w, M = B.arm_shape(cu, arm)
            assert B.h2_arm(cu, n, h, w, M) == arm and (n == 1 or B.h2_arm(cu, n - 1, h, w, M) != arm)
            seen.add(arm)
        assert seen == set(B.ARMS)
    assert [B.arm_shape(256, a)[0] for a in B.ARMS[1:]] == [16, 4, 16, 16]

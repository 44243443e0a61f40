"""-m gpu: the three launches of the BatchNorm-folded conv3x3 through the C ABI, each against a float64 reference PER ELEMENT:
  (a) unet_conv3x3_bnfold_fwd          conv_h2_kernel with the MASK_BIAS_TAB epilogue, on every instance k_conv3x3_h2_fwd dispatches to;
  (b) unet_conv3x3_bnfold_bwd_weights  dw, db and the BatchNorm's backward sums, with and without the sums pointer, NS = 4 n beyond one trip of the tap-sum loop;
  (c) unet_conv3x3_bnfold_bwd_data     the MASK_BN_BWD / _RELU / _ELU / _ELU_DROP epilogues and mask_climit (x_channels), on every instance;
  (d) (b) -> (c) chained on the device's own sums, against torch.autograd through a training-mode BatchNorm.
References, bounds (with their derivations) and check functions: tests/bnfold_checks.py; tests/test_bnfold_bounds_host.py shows that each check rejects a defect of
its launch.  Two parameter regimes (bnfold_checks.make_case): scale / shift independent of x, and the BatchNorm of x itself where every fourth channel has
mean = 30 std -- the regime include/unet_hip.h warns about: the products and the table cancel to a thirtieth of their size.

The context runs with CONV_PP = 0, so 32-channel launches stay on conv_h2_kernel.  The shapes of the four larger instances follow from the device's CU count
(bnfold_checks.arm_shape) and each test asserts, from the transcribed dispatch arithmetic, that its launch takes the intended instance; <0,2,4,2> has RW * NB = 8, so
its mask / table is read by the path without the prefetch.  A limit below cin needs a multiple of 32 below cin, which M = 32 does not have: the `1,2,4 inb=1` instance
runs the data gradient without a limit only.

Every check prints its worst error / bound ratio ("bound-ratio ...", run with -s).  Measured on an MI355X (256 CUs), worst per family:
  (a) forward: tiny shapes 0.10 (independent parameters) / 0.11 (BatchNorm of x), the four larger instances 0.14, worst single border class 0.14;
  (b) dw 0.19, the taps wholly outside a one-row / one-column image 0.033, db 0.078, sum dz 0.0052, sum dz xhat 0.0075 (dw / db bit-identical with and without the
      sums pointer in all 12 cases);
  (c) dx: modes NONE 0.16, RELU 0.13, ELU 0.16, ELU_DROP 0.20; the channels above x_channels 0.16; the larger instances 0.25 (also above the limit: <0,2,4,2>);
  (d) the chain 0.045 against the formula and against autograd (the parameter rounding moves the reference by 0.005 of the allowance).
No ratio above 1: the tests found no defect in the kernels.
"""
import numpy as np
import pytest
import torch

import bnfold_checks as B
from gpu_util import cu_count
from test_gpu_conv_pp import PPOps

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
# (n, h, w, cin, cout): every channel case of the fold at a tiny size; one-row and one-column images; 48 / 80: the ragged last slice of bn_fold_taps_kernel
TINY = [(2, 33, 9, 16, 16), (3, 1, 40, 48, 32), (2, 40, 1, 80, 64), (1, 5, 33, 64, 256), (2, 2, 9, 512, 256), (1, 9, 5, 48, 32)]
REGIMES = ["indep", "bn"]


@pytest.fixture(scope="module")
def ops():
    o = PPOps(0)
    assert o.lib.unet_ctx_get_option(o.h, 13) == 0
    return o


def ptr(t):
    return t.data_ptr() if t is not None else None


def run_fwd(ops, case, act):
    n, h, w, ci, co = case["shape"]
    y = torch.full((n, h, w, co), SENT, dtype=torch.float32, device=DEV)
    ws = ops.z(int(ops.lib.unet_conv3x3_bnfold_ws_floats(n, ci, co)))
    ops.ck(ops.lib.unet_conv3x3_bnfold_fwd(ops.h, ops.d(case["x"]).data_ptr(), ops.d(B.bnp_of(case)).data_ptr(), ops.d(case["k"]).data_ptr(), ops.d(case["b"]).data_ptr(), y.data_ptr(),
                                           n, h, w, ci, co, act, 0, ws.data_ptr(), ops.s), "fold fwd")
    return y


def run_wgrad(ops, case, sums):
    """sums: None (the NULL path, fold_fix_kernel) or a device double[2 cin] that is added to"""
    n, h, w, ci, co = case["shape"]
    gb = int(ops.lib.unet_conv3x3_bwd_weights_ws_bytes(n, h, w, ci, co)); gws = ops.z(max(gb // 4, 4))
    ws = ops.z(int(ops.lib.unet_conv3x3_bnfold_ws_floats(n, ci, co)))
    dw = torch.full((3, 3, ci, co), SENT, dtype=torch.float32, device=DEV); db = torch.full((co,), SENT, dtype=torch.float32, device=DEV)
    ops.ck(ops.lib.unet_conv3x3_bnfold_bwd_weights(ops.h, ops.d(case["x"]).data_ptr(), ops.d(B.bnp_of(case)).data_ptr(), ops.d(case["dy"]).data_ptr(), ops.d(case["k"]).data_ptr(),
                                                   dw.data_ptr(), db.data_ptr(), ptr(sums), gws.data_ptr(), gb, ws.data_ptr(), n, h, w, ci, co, 0, ops.s), "fold wgrad")
    return dw, db


def call_dgrad(ops, case, x_dev, sums, mode, rate, seed, x_channels, dx, algo=0, count=None, shape=None):
    n, h, w, ci, co = shape or case["shape"]
    coef = ops.z(3 * ci)
    return ops.lib.unet_conv3x3_bnfold_bwd_data(ops.h, ops.d(case["dy"]).data_ptr(), ops.d(case["k"]).data_ptr(), ops.d(B.bnp_of(case)).data_ptr(), sums.data_ptr(),
                                                float(n * h * w) if count is None else count, ptr(x_dev), x_channels, mode, rate, seed, dx.data_ptr(), ops.wws(ci, co), coef.data_ptr(),
                                                n, h, w, ci, co, algo, ops.s)


def run_dgrad(ops, case, sums, mode=0, rate=0.0, seed=0, x_channels=None):
    n, h, w, ci, co = case["shape"]
    lim = ci if x_channels is None else x_channels
    x = case["x"].copy()
    if lim < ci:
        x[..., lim:] = np.nan                                # the launch must not read x from the limit on
    dx = torch.full((n, h, w, ci), SENT, dtype=torch.float32, device=DEV)
    ops.ck(call_dgrad(ops, case, ops.d(x), sums.contiguous(), mode, rate, seed, lim, dx), "fold dgrad")
    return dx


def dev_sums(case):
    """the exact float64 sums (sum dz, sum dz xhat) of the reference data gradient under the case's fp32 mean / invstd, on the device"""
    x, k, dy, mean, istd = (B.t64(case[v], DEV) for v in ("x", "k", "dy", "mean", "istd"))
    return B.exact_sums(B.dgrad64(dy, k), x, mean, istd)


# ---- (a) forward -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", TINY)
def test_forward_tiny_every_channel_case(ops, shape, regime):
    n, h, w, ci, co = shape
    assert n * h * w <= 2000 and B.h2_arm(cu_count(), n, h, w, co) == B.ARMS[0]
    case = B.make_case(*shape, regime, 100 + ci + h)
    P = B.fwd_problem(case, DEV)
    for act in (0, 1):
        B.check_fwd(run_fwd(ops, case, act), P, act, f"fwd {shape} {regime}")


@pytest.mark.parametrize("arm", B.ARMS[1:])
def test_forward_on_every_larger_instance(ops, arm):
    """K = 16 input channels keep the reference cheap; the batch is the smallest at which this device's CU count sends the launch to `arm`"""
    n, h, w, M = B.arm_shape(cu_count(), arm)
    assert B.h2_arm(cu_count(), n, h, w, M) == arm
    case = B.make_case(n, h, w, 16, M, "bn", 200 + M + h)
    P = B.fwd_problem(case, DEV)
    for act in (0, 1):
        B.check_fwd(run_fwd(ops, case, act), P, act, f"fwd <{arm}> {case['shape']}")


# ---- (b) weight gradient, db, the BatchNorm sums -------------------------------------------------------------------------------------------------------------------------
# n in {1, 5, 9}: NS = 4, 20, 36 entries -- one, two, three trips of fold_tap_sums_kernel's loop; cout 16 / 64 / 256: nsl = 16 / 4 / 1 in border_sums_kernel
WGRAD = [(1, 1, 7, 16, 16, "indep"), (5, 1, 7, 16, 64, "bn"), (9, 7, 1, 48, 16, "bn"), (5, 7, 1, 512, 256, "indep"), (9, 2, 3, 16, 256, "bn"), (5, 2, 3, 48, 64, "indep"),
         (1, 5, 5, 512, 16, "bn"), (9, 5, 5, 48, 256, "indep"), (5, 6, 33, 16, 16, "bn"), (9, 6, 33, 512, 64, "bn"), (1, 6, 33, 48, 256, "indep"), (5, 5, 5, 16, 64, "indep")]


@pytest.mark.parametrize("cfg", WGRAD)
def test_weight_gradient_bias_gradient_and_bn_sums(ops, cfg):
    n, h, w, ci, co, regime = cfg
    assert n == 1 or 4 * n > 16
    case = B.make_case(n, h, w, ci, co, regime, 300 + 7 * n + ci + co)
    P = B.wgrad_problem(case, DEV)
    dw0, db0 = run_wgrad(ops, case, None)
    pre = torch.linspace(-3.0, 5.0, 2 * ci, dtype=torch.float64, device=DEV)
    sums = pre.clone()
    dw1, db1 = run_wgrad(ops, case, sums)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)          # both paths evaluate fmaf(scale, dw_raw, shift * S) on the same dw_raw
    B.check_wgrad(dw1, db1, P, f"wgrad {cfg}")
    B.check_bn_sums(sums, pre, P, f"wgrad {cfg}")


# ---- (c) data gradient ----------------------------------------------------------------------------------------------------------------------------------------------------
MODES = [(0, "none"), (1, "relu"), (2, "elu"), (3, "elu_drop")]


@pytest.mark.parametrize("mode,producer", MODES)
@pytest.mark.parametrize("shape", TINY[:5])
def test_data_gradient_every_mode(ops, shape, mode, producer):
    rate, seed = (0.25, 1234567 + shape[3]) if mode == 3 else (0.0, 0)
    for regime in (REGIMES if mode == 0 else ["bn"]):
        case = B.make_case(*shape, regime, 400 + mode + shape[3], producer=producer, rate=rate, drop_seed=seed)
        sums = dev_sums(case)
        P = B.dgrad_problem(case, sums, mode, rate, seed, dev=DEV)
        B.check_dgrad(run_dgrad(ops, case, sums, mode, rate, seed), P, f"dgrad {shape} mode {mode} {regime}")


@pytest.mark.parametrize("shape", [TINY[3], TINY[4]])
def test_data_gradient_above_x_channels_leaves_without_reading_x(ops, shape):
    ci = shape[3]
    case = B.make_case(*shape, "bn", 500 + ci)
    sums = dev_sums(case)
    P = B.dgrad_problem(case, sums, x_channels=ci // 2, dev=DEV)
    K0, _, K2 = P["K"]
    assert float((P["ref"][..., ci // 2:] - (K0 * P["dz"] + K2)[..., ci // 2:]).abs().max()) == 0.0
    B.check_dgrad(run_dgrad(ops, case, sums, x_channels=ci // 2), P, f"dgrad {shape} x_channels {ci // 2}")


@pytest.mark.parametrize("arm,limit", [(a, l) for a in B.ARMS[1:] for l in (False, True) if not (l and B.ARM_CASES[a][0] == 32)])          # (M = 32: see the module docstring)
def test_data_gradient_on_every_larger_instance(ops, arm, limit):
    n, h, w, M = B.arm_shape(cu_count(), arm)
    assert B.h2_arm(cu_count(), n, h, w, M) == arm
    case = B.make_case(n, h, w, M, 16, "bn", 600 + M + h)
    sums = dev_sums(case)
    lim = M // 2 if limit else None
    P = B.dgrad_problem(case, sums, x_channels=lim, dev=DEV)
    B.check_dgrad(run_dgrad(ops, case, sums, x_channels=lim), P, f"dgrad <{arm}> {case['shape']} x_channels {lim}")


def test_data_gradient_refusals_write_nothing(ops):
    shape = (1, 5, 9, 64, 32)
    case = B.make_case(*shape, "indep", 700)
    sums = dev_sums(case).contiguous()
    x = ops.d(case["x"])
    dx = torch.full(shape[:4], SENT, dtype=torch.float32, device=DEV)
    E_ARG, E_SHAPE = -1, -3
    assert call_dgrad(ops, case, x, sums, 0, 0.0, 0, 48, dx) == E_ARG                              # not a multiple of 32
    assert call_dgrad(ops, case, x, sums, 0, 0.0, 0, 96, dx) == E_ARG and call_dgrad(ops, case, x, sums, 0, 0.0, 0, 0, dx) == E_ARG
    assert call_dgrad(ops, case, x, sums, 1, 0.0, 0, 32, dx) == E_ARG                              # a limit leaves no x for the derivative of its producer
    assert call_dgrad(ops, case, x, sums, 0, 0.0, 0, 64, dx, count=0.5) == E_ARG
    assert call_dgrad(ops, case, None, sums, 0, 0.0, 0, 64, dx) == E_ARG
    assert call_dgrad(ops, case, x, sums, 4, 0.0, 0, 64, dx) == E_ARG and call_dgrad(ops, case, x, sums, 3, 1.0, 0, 64, dx) == E_ARG
    assert call_dgrad(ops, case, x, sums, 0, 0.0, 0, 24, dx, shape=(1, 5, 9, 24, 32)) == E_SHAPE      # cin not a multiple of 16
    assert call_dgrad(ops, case, x, sums, 0, 0.0, 0, 64, dx, shape=(1, 5, 9, 64, 48)) == E_SHAPE      # cout not a divisor of 256
    assert call_dgrad(ops, case, x, sums, 0, 0.0, 0, 64, dx, algo=1) == E_SHAPE                      # the direct kernels have no such epilogue
    torch.cuda.synchronize()
    assert bool((dx == SENT).all())
    ops.ck(call_dgrad(ops, case, x, sums, 0, 0.0, 0, 64, dx), "fold dgrad after the refusals")
    B.check_dgrad(dx, B.dgrad_problem(case, sums, dev=DEV), "dgrad after the refusals")


# ---- (d) the chain as a training step runs it -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 9, 5, 64, 32), (2, 5, 2, 512, 256)])
def test_chain_weight_gradient_sums_into_data_gradient_against_autograd(ops, shape):
    """bnfold_bwd_weights leaves the sums, bnfold_bwd_data consumes them.  Allowance: (c)'s bound plus what the sums' error does to dx = sc (dz - k1 - xhat k2):
    |scale_c| (e_k1 + |xhat| e_k2), e_k = (b)'s sums bounds / count.  Against the formula under the fp32 (scale, mean, invstd) the device was given, and against
    torch.autograd's gradient, whose float64 mean / invstd differ from those by one fp32 rounding: the exact effect of that rounding, |F(fp32 parameters) - F(float64
    parameters)| of the float64 formula, is added there (F(float64 parameters) = autograd to 1e-10)."""
    n, h, w, ci, co = shape
    case = B.make_case(*shape, "bn", 800 + ci)
    W = B.wgrad_problem(case, DEV)
    sums = torch.zeros(2 * ci, dtype=torch.float64, device=DEV)
    run_wgrad(ops, case, sums)
    dx = run_dgrad(ops, case, sums)
    P = B.dgrad_problem(case, dev_sums(case), dev=DEV)
    x, sc, mean, istd = (B.t64(case[v], DEV) for v in ("x", "scale", "mean", "istd"))
    e_k = W["sums_bound"] / W["count"]
    extra = sc.abs() * (e_k[:ci] + ((x - mean) * istd).abs() * e_k[ci:])
    B.check_elem(dx, P["ref"], P["bound"] + extra, f"chain {shape} against the formula")
    g, sc64, mean64, istd64 = B.bn_train_dx_autograd(case)
    c64 = dict(case, scale=sc64.numpy(), mean=mean64.numpy(), istd=istd64.numpy())
    F64 = B.dgrad_problem(c64, B.exact_sums(B.dgrad64(B.t64(case["dy"]), B.t64(case["k"])), B.t64(case["x"]), mean64, istd64))["ref"]
    assert float((F64 - g).abs().max()) < 1e-10 * float(g.abs().max())
    par = (P["ref"] - F64.to(DEV)).abs()
    print(f"chain {shape}: parameter rounding moves the reference by at most {float((par / (P['bound'] + extra)).max()):.3g} of the allowance")
    B.check_elem(dx, g.to(DEV), P["bound"] + extra + par, f"chain {shape} against autograd")

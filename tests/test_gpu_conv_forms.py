"""-m gpu: every launch form of the fp32 h2 conv kernels at ragged shapes (tests/conv_forms.py; the arithmetic that sends a shape to a form is checked on the CPU by
tests/test_conv_forms_host.py).  The op-level tests' ragged shapes all land in the instance for grids smaller than the chip (`1,1,4`); here the four larger instances
of conv_h2_kernel meet a short last row tile (also a 16-row tile whose second half lies outside the image), a short last column tile, a half-empty channel block, the
statistics / sign-bit / dropout / border-class epilogues on such tiles; the weight gradient walks two (sample, strip) units per workgroup with a short last unit block;
the pooled-sums data gradient runs its 16-row instance.  (The ConvT forward's four-block form with a short last column tile is a shape of test_gpu_ops.test_convT.)

Rules of every test: the context runs with CONV_PP = 0; the instance is asserted from the transcribed dispatch before the launch; inputs are seeded fp32, the reference
is float64 on the device (bnfold_checks.conv64 / dgrad64 / wgrad64: shifted matrix products); every output lies inside a larger allocation filled with a sentinel,
with a band of at least one image row before and behind it that must stay untouched, and is itself prefilled with the sentinel.  The per-element bound is the op
tests': |err| <= EPS_SPLIT * A1 (gpu_util; A1 = sum |a| |b| of the element, + |bias| forward), evaluated on the device by bnfold_checks.check_elem -- the same
quotient as gpu_util.elem_ratio.

The folded-BatchNorm forward takes cout only where 256 % cout == 0 (unet_conv3x3_bnfold_supported), so it runs on the two cases of the table with such an M and on
M = 256 at the 16-row and the two-block 8-row instance (conv_forms.FOLD_FWD_CASES); its data gradient (cin = M) runs on every case of the two-block arms and on M = 96.

Every check prints its worst error / bound ratio ("bound-ratio ...", run with -s).  Measured on an MI355X (256 CUs), worst per mode and arm
(`1,2,4 inb=1` | `1,2,4 inb=2` | `2,4,2` | `2,2,2`):
  (a) forward, bias / ReLU / channel slice            0.23 | 0.21 | 0.25 | 0.30
  (b) data gradient, plain / UNET_MASK_RELU           0.21 | 0.26 | 0.28 | 0.26
  (c) statistics, sum y and sum y^2, default context  0.00097 | 0.0027 | 0.00067 | 0.0012   (the (T + 2) u sum |y| bound is a worst case);
      deterministic context (the cases up to M = 256) 0.00097 | 0.00072 | 0.00044 | 0.00095  (the same figures as the default context case by case; two runs bit-equal)
  (d) sign bits: wrong words 0 everywhere; forward    0.24 | 0.20 | 0.28 | 0.27;  the bit-masked data gradient (bit-equal to the fp32-masked one) 0.19 | 0.19 | 0.25 | 0.23
  (e) ELU + dropout forward                           0.22 | - | 0.23 | 0.30;  negative side (|err| - split bound) / (u |want|) at most -68 (allowed 2); mask differences 0;
      UNET_MASK_ELU 0.19 | - | 0.27 | 0.24;  UNET_MASK_ELU_DROP 0.19 | - | 0.22 | 0.23
  (f) folded forward (worst border class the same)    0.14 | - | 0.13 | 0.14;  folded data gradient 0.18 | - | 0.23 | 0.22, the channels from x_channels on 0.18 | - | 0.22 | 0.20
  weight gradient with upb = 2: dw 0.055 (17 units) / 0.049 (16 units), db 2.2e-7 relative, algo 2 against algo 0 2.7e-7;  pooled sums, 16-row instance: sums 0.062 of
  their tolerance, dx 0.26.
"""
import functools

import numpy as np
import pytest
import torch

import bnfold_checks as B
import conv_forms as F
from gpu_util import EPS_SPLIT, U, cu_count, relerr
from test_gpu_conv_pp import PPOps

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -777.0
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    o = PPOps(0)
    assert o.lib.unet_ctx_get_option(o.h, 13) == 0
    return o


@pytest.fixture(scope="module", autouse=True)
def release_problems():
    """the cached problems hold float64 device tensors of up to 16 M elements: released when the module is done"""
    yield
    _fwd_problem.cache_clear(); _dgrad_problem.cache_clear(); _fold_case.cache_clear()
    torch.cuda.empty_cache()


# ---- outputs inside a guarded allocation --------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """a tensor of `shape` in the middle of one allocation, `band` sentinel elements before and behind it; the tensor itself prefilled with the sentinel"""

    def __init__(self, shape, band, dtype=F32, sent=SENT):
        size = int(np.prod(shape))
        self.band, self.sent = int(band), sent
        self.buf = torch.full((size + 2 * self.band,), sent, dtype=dtype, device=DEV)
        self.t = self.buf[self.band:self.band + size].view(*shape)
        assert self.t.data_ptr() == self.buf.data_ptr() + self.band * self.buf.element_size()

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        assert bool((self.buf[:self.band] == self.sent).all()), f"{what}: the band in front of the output was written"
        assert bool((self.buf[-self.band:] == self.sent).all()), f"{what}: the band behind the output was written"


def image(n, h, w, ld):
    """NHWC output with ld floats per pixel; band = two image rows"""
    return Guarded((n, h, w, ld), 2 * w * ld)


def shape_of(case):
    """(n, h, w, M) of the case on this device; asserts the launch form from the transcribed dispatch"""
    arm, (M, h, w), _ = case
    n = F.case_batch(cu_count(), case)
    assert B.h2_arm(cu_count(), n, h, w, M) == arm
    return n, h, w, M


def seed_of(case, salt):
    arm, (M, h, w), _ = case
    return 100000 * salt + 1000 * B.ARMS.index(arm) + M + 7 * h + 3 * w


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# ---- the problems (computed once per case, never modified) ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_problem(key):
    case = KEYS[key]
    n, h, w, M = shape_of(case)
    rng = np.random.default_rng(seed_of(case, 1))
    x = dv(rng.standard_normal((n, h, w, F.K_SIDE))); k = dv(rng.standard_normal((3, 3, F.K_SIDE, M)) * np.sqrt(2.0 / (9 * F.K_SIDE))); b = dv(rng.standard_normal(M) * 0.3)
    pre = B.conv64(x.double(), k.double()) + b.double()
    a1b = B.conv64(x.double().abs(), k.double().abs()) + b.double().abs()
    return dict(x=x, k=k, b=b, pre=pre, a1b=a1b, shape=(n, h, w, M))


@functools.lru_cache(maxsize=None)
def _dgrad_problem(key):
    case = KEYS[key]
    n, h, w, M = shape_of(case)
    rng = np.random.default_rng(seed_of(case, 2))
    dy = dv(rng.standard_normal((n, h, w, F.K_SIDE))); k = dv(rng.standard_normal((3, 3, M, F.K_SIDE)) * np.sqrt(2.0 / (9 * M)))
    g = torch.Generator(device=DEV); g.manual_seed(seed_of(case, 3))
    xm = torch.randn((n, h, w, M), generator=g, device=DEV, dtype=F32)          # what a mask mode reads: a tensor of the output's shape
    dz = B.dgrad64(dy.double(), k.double())
    a1 = B.dgrad64(dy.double().abs(), k.double().abs())
    return dict(dy=dy, k=k, xm=xm, dz=dz, a1=a1, shape=(n, h, w, M))


KEYS = {F.case_id(c): c for c in F.CASES + F.BITS_CASES + F.FOLD_FWD_EXTRA}


def fwd_problem(case):
    return _fwd_problem(F.case_id(case))


def dgrad_problem(case):
    return _dgrad_problem(F.case_id(case))


def conv_fwd(ops, P, y_ptr, act, rate=0.0, seed=0, algo=0, handle=None, ctx=None):
    n, h, w, M = P["shape"]
    rc = ops.lib.unet_conv3x3_fwd(handle or ops.h, P["x"].data_ptr(), P["k"].data_ptr(), P["b"].data_ptr(), y_ptr, n, h, w, F.K_SIDE, M, act, rate, seed, algo,
                                  ops.wws(F.K_SIDE, M) if algo == 0 else None, ops.s)
    (ctx or ops.ctx).check(rc, "conv fwd")
    torch.cuda.synchronize()


def conv_dgrad(ops, P, mask_ptr, mode, dx_ptr, rate=0.0, seed=0):
    n, h, w, M = P["shape"]
    ops.ck(ops.lib.unet_conv3x3_bwd_data(ops.h, P["dy"].data_ptr(), P["k"].data_ptr(), mask_ptr, mode, rate, seed, dx_ptr, ops.wws(M, F.K_SIDE), n, h, w, M, F.K_SIDE, 0, ops.s), "conv dgrad")


# ---- (a) forward ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_forward_bias_plain_relu_and_into_a_channel_slice(ops, case):
    """y = conv + bias and relu(conv + bias) per element within EPS_SPLIT (A1 + |b|); the ReLU launch once more through unet_conv3x3_fwd_ld into a buffer of M + 4 floats per
    pixel, whose four extra channels keep their sentinel"""
    P = fwd_problem(case)
    n, h, w, M = P["shape"]
    bound = EPS_SPLIT * P["a1b"]
    for relu in (0, 1):
        y = image(n, h, w, M)
        conv_fwd(ops, P, y.ptr(), relu)
        y.check(f"fwd {F.case_id(case)} relu={relu}")
        B.check_elem(y.t, P["pre"].clamp_min(0.0) if relu else P["pre"], bound, f"fwd <{case[0]}> {P['shape']} relu={relu}")
    ld = M + 4
    y = image(n, h, w, ld)
    ops.ck(ops.lib.unet_conv3x3_fwd_ld(ops.h, P["x"].data_ptr(), P["k"].data_ptr(), P["b"].data_ptr(), y.ptr(), ld, n, h, w, F.K_SIDE, M, 1, 0, ops.wws(F.K_SIDE, M), ops.s), "conv fwd ld")
    y.check(f"fwd ld {F.case_id(case)}")
    assert bool((y.t[..., M:] == SENT).all()), "the channels beside the slice were written"
    B.check_elem(y.t[..., :M], P["pre"].clamp_min(0.0), bound, f"fwd <{case[0]}> {P['shape']} relu=1 ld={ld}")


# ---- (b) data gradient ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_data_gradient_plain_and_relu_masked(ops, case):
    """cin = M, cout = 16: dx per element within EPS_SPLIT A1 (A1 = sum |dy| |w|), without a mask and with UNET_MASK_RELU of a tensor of dx's shape"""
    P = dgrad_problem(case)
    n, h, w, M = P["shape"]
    bound = EPS_SPLIT * P["a1"]
    for masked in (0, 1):
        dx = image(n, h, w, M)
        conv_dgrad(ops, P, P["xm"].data_ptr() if masked else None, masked, dx.ptr())
        dx.check(f"dgrad {F.case_id(case)} masked={masked}")
        want = P["dz"] * (P["xm"] > 0) if masked else P["dz"]
        B.check_elem(dx.t, want, bound, f"dgrad <{case[0]}> {P['shape']} masked={masked}")


# ---- (c) statistics epilogue -------------------------------------------------------------------------------------------------------------------------------------------
def stats_terms(arm):
    """terms of one fp32 partial of the statistics epilogue: a workgroup adds what it stored of ONE tile -- 4 waves x RW rows x 32 pixels per channel -- in fp32 (a lane
    its RW x 4 values, three shuffle steps across the 8 lanes of a channel quad, then the four waves) and posts that partial as a double"""
    return F.TILE_ROWS[arm] * 32


STATS_PARAMS = [(c, 0) for c in F.STATS_CASES] + [(c, 1) for c in F.STATS_DET_CASES]


@pytest.mark.parametrize("case,det", STATS_PARAMS, ids=[F.case_id(c) + ("-deterministic" if d else "-default") for c, d in STATS_PARAMS])
def test_statistics_epilogue_sums_what_the_launch_stored(ops, case, det):
    """unet_request_bn_stats -> conv (ReLU) -> unet_bn_stats folds the slots: per channel (sum y, sum y^2) of the tensor the launch STORED.
    That the sums come from the launch's epilogue and not from a pass over the tensor: the tensor is overwritten on the device between the launch and unet_bn_stats -- a
    fold still returns the sums of what was stored, the ordinary pass (a launch that declined the request, BN_FUSE_STATS off) would return those of the overwriting value.
    launch_h2 declines where the slot copies cannot hold 2 M values -- of four words each in deterministic mode, so that context runs the cases up to M = 256
    (conv_forms.STATS_DET_CASES, which still reach every instance and both kinds of last 16-row tile); the default context runs them all.
    Bound, as test_gpu_storage_ops.py derives bn_stats': a partial is an fp32 sum of T terms in some order -- at most T - 1 roundings on a term's way, each u times a
    partial sum that is at most sum |term| -- plus the rounding of the term's own arrival: (T + 2) u sum |y| for the sum and (T + 3) u sum y^2 for the squares (the
    fma's product is exact, the allowance of bn_stats is kept); T = stats_terms(arm) <= 16 x 32 = 512, so the factor is at most 515.  The partials then add as doubles
    (2^-50 sum |term| allowed for any number of them).  A partial tile only has fewer terms.
    Deterministic mode: exact window sums of the same fp32 partials -- two runs agree in every bit, and with the float64 sums to 1e-6 (relative L2, the rule of
    test_conv_epilogue_statistics_in_deterministic_mode_are_exact_window_sums).  Either way the unarmed pass over the (restored) tensor afterwards gives the same sums:
    nothing stale stays in the slots."""
    from covidseg_amd import _lib
    from gpu_util import check_sum
    P = fwd_problem(case)
    n, h, w, M = P["shape"]
    T = stats_terms(case[0])
    assert T + 3 <= 512 + 3 and F.stats_epilogue_accepts(M, det)
    ctx = _lib.Context.get(0, {"deterministic": 1, "conv_pp": 0}, private=True) if det else ops.ctx
    try:
        assert ops.lib.unet_ctx_get_option(ctx.handle, 13) == 0 and ops.lib.unet_ctx_get_option(ctx.handle, 6) == det and ops.lib.unet_ctx_get_option(ctx.handle, 5) == 1
        outs, stored = [], []
        for rep in range(2 if det else 1):
            y = image(n, h, w, M); sums = torch.zeros(2 * M, dtype=torch.float64, device=DEV)
            ctx.check(ops.lib.unet_request_bn_stats(ctx.handle, M), "arm")
            conv_fwd(ops, P, y.ptr(), 1, handle=ctx.handle, ctx=ctx)
            stored.append(y.t.clone())
            y.t.fill_(3.0)                                           # what an ordinary statistics pass would now see: sum 3 pixels, sum of squares 9 pixels
            torch.cuda.synchronize()
            ctx.check(ops.lib.unet_bn_stats(ctx.handle, y.ptr(), M, sums.data_ptr(), n * h * w, M, ops.s), "fold")
            torch.cuda.synchronize()
            y.check(f"stats {F.case_id(case)}")
            assert bool((y.t == 3.0).all())                          # (the fold wrote nothing)
            outs.append(sums.cpu().numpy().copy())
        y64 = stored[0].double().reshape(-1, M)
        assert bool((y64 >= 0).all()) and 0.2 < float((y64 > 0).double().mean()) < 0.8          # (the sentinel is negative: every element was written)
        s1, s2 = y64.sum(0).cpu().numpy(), (y64 * y64).sum(0).cpu().numpy()
        got = outs[0]
        assert float(np.abs(got[:M] - 3.0 * n * h * w).min()) > 0.25 * n * h * w, "unet_bn_stats read the tensor: the launch did not take the armed request"
        check_sum(got[:M], s1, ((T + 2) * U + 2.0 ** -50) * s1, f"stats <{case[0]}> {P['shape']} det={det} sum y")
        check_sum(got[M:], s2, ((T + 3) * U + 2.0 ** -50) * s2, f"stats <{case[0]}> {P['shape']} det={det} sum y^2")
        if det:
            assert torch.equal(stored[0], stored[1]) and np.array_equal(outs[0], outs[1])
            assert relerr(got, np.concatenate([s1, s2])) < 1e-6
        y.t.copy_(stored[-1])
        plain = torch.zeros(2 * M, dtype=torch.float64, device=DEV)
        ctx.check(ops.lib.unet_bn_stats(ctx.handle, y.ptr(), M, plain.data_ptr(), n * h * w, M, ops.s), "plain pass: nothing armed, slots clean")
        torch.cuda.synchronize()
        assert relerr(plain.cpu().numpy(), np.concatenate([s1, s2])) < 1e-6 and relerr(plain.cpu().numpy(), got) < 1e-6
    finally:
        if det:
            ctx.close()


# ---- (d) sign bits ------------------------------------------------------------------------------------------------------------------------------------------------------
def bit_words(pos):
    """the documented layout of unet_request_relu_bits from the boolean tensor pos [n, h, w, c]: 64-bit words [n][y][x / 8][c / 32][4], word k of a cell holds bit
    (x % 8) * 8 + (c % 32) / 4 for the channels with c % 4 == k (as test_relu_masks_as_one_bit_per_element computes them, on the device)"""
    n, h, w, c = pos.shape
    p7 = pos.view(n, h, w // 8, 8, c // 32, 8, 4)
    want = torch.zeros((n, h, w // 8, c // 32, 4), dtype=torch.int64, device=pos.device)
    for p in range(8):
        for q in range(8):
            want |= p7[:, :, :, p, :, q, :].to(torch.int64) << (p * 8 + q)
    return want


@pytest.mark.parametrize("case", F.BITS_CASES, ids=F.case_id)
def test_sign_bits_and_the_bit_masked_data_gradient(ops, case):
    """the words an armed ReLU forward writes are (y > 0) of what it stored, in the documented layout, on tiles that overhang the image; the data gradient masked with
    those words equals the one masked with the fp32 tensor in every bit"""
    P = fwd_problem(case)
    n, h, w, M = P["shape"]
    assert w % 8 == 0 and M % 32 == 0 and w % 32 != 0
    assert ops.lib.unet_relu_bits_supported(0, h, w, F.K_SIDE, M) == 1          # (the forward K_SIDE -> M, and the data gradient of a conv M -> K_SIDE: the same launch shape)
    words = n * h * w * M // 64
    assert int(ops.lib.unet_relu_bits_bytes(n, h, w, M)) == 8 * words
    bits = Guarded((words,), 2 * w * M // 64, dtype=torch.int64, sent=-1)
    y = image(n, h, w, M)
    ops.ck(ops.lib.unet_request_relu_bits(ops.h, bits.ptr()), "arm")
    conv_fwd(ops, P, y.ptr(), 1)
    y.check("fwd + bits: y"); bits.check("fwd + bits: words")
    B.check_elem(y.t, P["pre"].clamp_min(0.0), EPS_SPLIT * P["a1b"], f"bits fwd <{case[0]}> {P['shape']}")
    pos = y.t > 0
    assert 0.2 < float(pos.double().mean()) < 0.8
    want = bit_words(pos)
    bad = int((bits.t.view(want.shape) != want).sum())
    print(f"bound-ratio bits <{case[0]}> {P['shape']} wrong words {bad} of {words}")
    assert bad == 0
    # the data gradient of a following conv M -> 16 (its dx has M channels): bit mask == fp32 mask, bit for bit
    D = dgrad_problem(case)
    dx_f, dx_b = image(n, h, w, M), image(n, h, w, M)
    conv_dgrad(ops, D, y.ptr(), 1, dx_f.ptr())
    conv_dgrad(ops, D, bits.ptr(), 9, dx_b.ptr())
    dx_f.check("dgrad fp32 mask"); dx_b.check("dgrad bit mask")
    assert torch.equal(dx_f.t, dx_b.t) and float(dx_f.t.abs().sum()) > 0
    B.check_elem(dx_b.t, D["dz"] * pos, EPS_SPLIT * D["a1"], f"bits dgrad <{case[0]}> {D['shape']}")


# ---- (e) ELU + dropout (the GEN instances) ----------------------------------------------------------------------------------------------------------------------------------
RATE, DROP_SEED = 0.4, 4242
KS = float(np.float32(1.0) / (np.float32(1.0) - np.float32(RATE)))          # keep_scale's factor as the device forms it
# what the device's exponential may add on the negative side, in units of u |want|: measured on the MI355X against float64 as max (|err| - split bound) / (u |want|) over the
# kept elements with a negative pre-activation of the arm-`1,1,4` shapes of test_conv3x3_elu_dropout_and_mask_modes -- the figure
# test_elu_allowance_is_twice_what_the_small_grid_shapes_need measures again on every run; twice that, at least 2
ELU_MEASURED = -232.4
ELU_ALLOW = max(2.0, 2.0 * ELU_MEASURED)


def elu_forward_check(got, pre, a1b, keep, what):
    """got = keep ? KS elu(pre) : 0 per element.  pre >= 0: the split bound times KS.  pre < 0: the same bound (ELU is 1-Lipschitz) + ELU_ALLOW u |want|.
    Returns (worst ratio, the measured excess of the negative side in units of u |want|)."""
    want = torch.where(pre > 0, pre, torch.expm1(pre.clamp_max(0.0))) * KS
    split = EPS_SPLIT * a1b * KS
    bound = split + torch.where(pre < 0, ELU_ALLOW * U * want.abs(), torch.zeros_like(want))
    got = got.double()
    assert bool((got[~keep] == 0).all()), f"{what}: a removed element is not zero"
    neg = keep & (pre < 0)
    excess = float((((got - want).abs() - split) / (U * want.abs()).clamp_min(1e-300))[neg].max()) if bool(neg.any()) else 0.0
    print(f"bound-ratio {what} negative side: (|err| - split bound) / (u |want|) at most {excess:.3g} (allowed {ELU_ALLOW:g})")
    r = B.check_elem(got[keep], want[keep], bound[keep], what)
    return r, excess


def valu_keep_mask(ops, n, h, w, M, seed=DROP_SEED):
    """the keep mask of (RATE, seed) on a tensor [n, h, w, M] as the VALU kernel (algo 1) draws it: a conv of zeros with bias 1 and the dropout fused stores ks or 0
    (the probe of test_conv3x3_elu_dropout_and_mask_modes).  Not read off an ELU output: about one pre-activation in 1e8 is exactly 0 in fp32, and its kept value is 0 too."""
    km = image(n, h, w, M)
    x0 = torch.zeros((n, h, w, 8), dtype=F32, device=DEV); k0 = torch.zeros((3, 3, 8, M), dtype=F32, device=DEV); one = torch.ones(M, dtype=F32, device=DEV)
    ops.ck(ops.lib.unet_conv3x3_fwd(ops.h, x0.data_ptr(), k0.data_ptr(), one.data_ptr(), km.ptr(), n, h, w, 8, M, 0, RATE, seed, 1, None, ops.s), "mask probe")
    km.check("mask probe")
    assert bool(((km.t == 0) | (km.t == np.float32(KS))).all())
    return km.t != 0


ELU_MEASURE_SHAPES = [(2, 10, 14, 32, 64), (1, 8, 8, 96, 32), (1, 6, 6, 192, 64)]          # the h2-eligible shapes of test_conv3x3_elu_dropout_and_mask_modes


def test_elu_allowance_is_twice_what_the_small_grid_shapes_need(ops):
    """where ELU_MEASURED comes from: on the arm-`1,1,4` shapes of test_conv3x3_elu_dropout_and_mask_modes (its inputs, three seeds) the largest
    (|err| - split bound) / (u |want|) over the kept elements with a negative pre-activation, against float64.  Printed; ELU_ALLOW must be at least twice it (and at least
    2).  On the MI355X: -232 -- no element came within 232 u |want| of the split bound (|err| / (u |want|) itself reaches 1e5, all of it the split's share: |want| is
    small where pre is near 0), so the floor of 2 is what the larger instances are allowed."""
    worst = -float("inf")
    for shape in ELU_MEASURE_SHAPES:
        n, h, w, ci, co = shape
        assert B.h2_arm(cu_count(), n, h, w, co) == B.ARMS[0]
        rng = np.random.default_rng(31 + ci)
        x = dv(rng.standard_normal((n, h, w, ci))); k = dv(rng.standard_normal((3, 3, ci, co)) * 0.2); b = dv(rng.standard_normal(co))
        pre = B.conv64(x.double(), k.double()) + b.double(); a1b = B.conv64(x.double().abs(), k.double().abs()) + b.double().abs()
        for seed in (DROP_SEED, 99, 12345):
            y = image(n, h, w, co)
            ops.ck(ops.lib.unet_conv3x3_fwd(ops.h, x.data_ptr(), k.data_ptr(), b.data_ptr(), y.ptr(), n, h, w, ci, co, 2, RATE, seed, 0, ops.wws(ci, co), ops.s), "elu + dropout")
            y.check("elu + dropout")
            _, excess = elu_forward_check(y.t, pre, a1b, valu_keep_mask(ops, n, h, w, co, seed), f"elu measure {shape} seed {seed}")
            worst = max(worst, excess)
    print(f"bound-ratio elu measure: worst excess {worst:.4g} (ELU_MEASURED {ELU_MEASURED:g}, ELU_ALLOW {ELU_ALLOW:g})")
    assert ELU_ALLOW >= max(2.0, 2.0 * worst)


@pytest.mark.parametrize("case", F.GEN_CASES, ids=F.case_id)
def test_elu_dropout_forward_and_the_elu_mask_modes(ops, case):
    """act = ELU with dropout (rate 0.4) fused: the keep mask is element for element the one of the VALU kernel (algo 1) for the same (rate, seed) -- the Philox index of an
    element of a tile that overhangs the image: what the VALU kernel removes is stored as 0, what it keeps is KS elu(pre) within the bound of elu_forward_check (a wrongly
    removed element fails there: its bound is far below its value; a kept value that is itself 0 in fp32 passes there).  ELU_ALLOW: the test above.
    Data gradient (cin = M, cout = 16) behind an ELU output m (UNET_MASK_ELU: f = m > 0 ? 1 : m + 1) and behind a dropped ELU output m = ks elu (UNET_MASK_ELU_DROP:
    f = ks (a > 0 ? 1 : a + 1), a = m (1 - rate)), against f64(m) dz with f64 evaluated in float64 from the stored fp32 m:
    |dx - ref| <= |f| EPS_SPLIT A1 + |dz| e_f + 3 u |ref|.  e_f is what the roundings inside f cost: UNET_MASK_ELU_DROP ks u (|a| + |a + 1|) -- the product a and the
    sum a + 1 round once each (1 - rate and ks enter the reference as the fp32 values the device forms) --, UNET_MASK_ELU none (m + 1 is the first rounding of the
    3 u |ref|); the products with ks and with dz round once each: two (ELU: with m + 1, two) of the 3 u |ref|, one to spare."""
    P = fwd_problem(case)
    n, h, w, M = P["shape"]
    yd = image(n, h, w, M)
    conv_fwd(ops, P, yd.ptr(), 2, RATE, DROP_SEED)
    yd.check("elu + dropout")
    keep = valu_keep_mask(ops, n, h, w, M)
    assert abs(float(keep.double().mean()) - (1.0 - RATE)) < 0.01
    diff = int(((yd.t != 0) & ~keep).sum())
    zeros = int(((yd.t == 0) & keep).sum())
    print(f"bound-ratio gen keep mask <{case[0]}> {P['shape']} removed by the VALU kernel but stored {diff}, kept but stored as 0 (checked as values below) {zeros}")
    assert diff == 0
    elu_forward_check(yd.t, P["pre"], P["a1b"], keep, f"gen fwd <{case[0]}> {P['shape']}")
    # the data gradients: the mask source has dx's shape [n, h, w, M] -- and so the keep mask of (RATE, DROP_SEED) on it is `keep`
    D = dgrad_problem(case)
    m_elu = torch.where(D["xm"] > 0, D["xm"], torch.expm1(D["xm"].clamp_max(0.0)))          # an ELU output, fp32
    m_drop = (m_elu * keep * np.float32(KS)).to(F32)                                       # what the dropout behind it stored
    one_minus = float(np.float32(1.0) - np.float32(RATE))
    for mode, m in ((2, m_elu), (3, m_drop)):
        dx = image(n, h, w, M)
        conv_dgrad(ops, D, m.data_ptr(), mode, dx.ptr(), RATE if mode == 3 else 0.0, DROP_SEED if mode == 3 else 0)
        dx.check(f"dgrad mode {mode}")
        m64 = m.double()
        if mode == 2:
            f = torch.where(m64 > 0, torch.ones_like(m64), m64 + 1.0); e_f = torch.zeros_like(f)
        else:
            a = m64 * one_minus
            f = KS * keep * torch.where(a > 0, torch.ones_like(a), a + 1.0)
            e_f = KS * U * (a.abs() + (a + 1.0).abs()) * keep
        ref = f * D["dz"]
        bound = f.abs() * EPS_SPLIT * D["a1"] + D["dz"].abs() * e_f + 3.0 * U * ref.abs()
        B.check_elem(dx.t, ref, bound, f"gen dgrad <{case[0]}> {D['shape']} mode={mode}")


# ---- (f) folded BatchNorm ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _fold_case(key, fwd):
    case = KEYS[key]
    n, h, w, M = shape_of(case)
    return B.make_case(n, h, w, F.K_SIDE, M, "bn", seed_of(case, 4)) if fwd else B.make_case(n, h, w, M, F.K_SIDE, "bn", seed_of(case, 5))


@pytest.mark.parametrize("case", F.FOLD_FWD_CASES, ids=F.case_id)
def test_folded_batchnorm_forward_border_classes_inside_tiles(ops, case):
    """unet_conv3x3_bnfold_fwd (MASK_BIAS_TAB) where the last image row and column fall inside a tile: bnfold_checks.fwd_problem / check_fwd unchanged, per border class"""
    c = _fold_case(F.case_id(case), True)
    n, h, w, ci, co = c["shape"]
    assert ops.lib.unet_conv3x3_bnfold_supported(0, h, w, ci, co) == 1
    P = B.fwd_problem(c, DEV)
    ws = ops.z(int(ops.lib.unet_conv3x3_bnfold_ws_floats(n, ci, co)))
    for act in (0, 1):
        y = image(n, h, w, co)
        ops.ck(ops.lib.unet_conv3x3_bnfold_fwd(ops.h, ops.d(c["x"]).data_ptr(), ops.d(B.bnp_of(c)).data_ptr(), ops.d(c["k"]).data_ptr(), ops.d(c["b"]).data_ptr(), y.ptr(),
                                               n, h, w, ci, co, act, 0, ws.data_ptr(), ops.s), "fold fwd")
        y.check(f"fold fwd act={act}")
        B.check_fwd(y.t, P, act, f"fold fwd <{case[0]}> {c['shape']}")


@pytest.mark.parametrize("limit", [False, True], ids=["all_channels", "x_channels_below_cin"])
@pytest.mark.parametrize("case", F.FOLD_CASES, ids=F.case_id)
def test_folded_batchnorm_data_gradient(ops, case, limit):
    """unet_conv3x3_bnfold_bwd_data (MASK_BN_BWD; x_channels = cin, and a multiple of 32 below it: x is NaN from there on and must not be read):
    bnfold_checks.dgrad_problem / check_dgrad unchanged"""
    c = _fold_case(F.case_id(case), False)
    n, h, w, ci, co = c["shape"]
    assert ops.lib.unet_conv3x3_bnfold_supported(0, h, w, ci, co) == 1
    lim = (ci // 2) // 32 * 32 if limit else ci
    assert 32 <= lim <= ci and lim % 32 == 0
    x, k, dy, mean, istd = (B.t64(c[v], DEV) for v in ("x", "k", "dy", "mean", "istd"))
    sums = B.exact_sums(B.dgrad64(dy, k), x, mean, istd).contiguous()
    P = B.dgrad_problem(c, sums, x_channels=lim if limit else None, dev=DEV)
    xs = dv(c["x"])
    if lim < ci:
        xs[..., lim:] = float("nan")
    dx = image(n, h, w, ci); coef = ops.z(3 * ci)
    ops.ck(ops.lib.unet_conv3x3_bnfold_bwd_data(ops.h, ops.d(c["dy"]).data_ptr(), ops.d(c["k"]).data_ptr(), ops.d(B.bnp_of(c)).data_ptr(), sums.data_ptr(), float(n * h * w), xs.data_ptr(), lim,
                                                0, 0.0, 0, dx.ptr(), ops.wws(ci, co), coef.data_ptr(), n, h, w, ci, co, 0, ops.s), "fold dgrad")
    dx.check(f"fold dgrad x_channels={lim}")
    B.check_dgrad(dx.t, P, f"fold dgrad <{case[0]}> {c['shape']} x_channels {lim}")


# ---- the weight gradient with two units per workgroup -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.WGRAD_CASES)
def test_weight_gradient_walks_two_units_per_workgroup(ops, shape):
    """plan_wgrad_h2 gives a workgroup upb = 2 (sample, strip) units here (units = 17: nine unit blocks, the last one short, odd height; units = 16: the even twin).
    dw per element within EPS_SPLIT A1 (A1 = sum_p |x| |dy|) of nine float64 products, db to 2e-5 (relative L2); the strict fp32 MFMA kernel (algo 2) agrees to 3e-5."""
    n, h, w, ci, co = shape
    p = F.plan_wgrad_h2(*shape)
    assert p["upb"] >= 2 and p["ublocks"] == B.cdiv(p["units"], p["upb"]) and (p["units"] % p["upb"] != 0) == (shape == F.WGRAD_CASES[0])
    rng = np.random.default_rng(n + h + w)
    x = dv(rng.standard_normal((n, h, w, ci))); dy = dv(rng.standard_normal((n, h, w, co)))
    want = B.wgrad64(x.double(), dy.double()); a1 = B.wgrad64(x.double().abs(), dy.double().abs())
    want_db = dy.double().sum((0, 1, 2)).cpu().numpy()
    nb = int(ops.lib.unet_conv3x3_bwd_weights_ws_bytes(n, h, w, ci, co))
    outs = []
    for algo in (0, 2):
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        dw = Guarded((3, 3, ci, co), ci * co); db = Guarded((co,), co)          # (prefilled: both are overwritten, not added to)
        ops.ck(ops.lib.unet_conv3x3_bwd_weights(ops.h, x.data_ptr(), dy.data_ptr(), dw.ptr(), db.ptr(), ws.data_ptr(), nb, n, h, w, ci, co, algo, ops.s), f"wgrad algo {algo}")
        dw.check(f"wgrad algo {algo}: dw"); db.check(f"wgrad algo {algo}: db")
        outs.append((dw.t.clone(), db.t.clone()))
    dw0, db0 = outs[0]
    B.check_elem(dw0, want, EPS_SPLIT * a1, f"wgrad upb={p['upb']} {shape} dw")
    rdb = relerr(db0.cpu().numpy(), want_db)
    print(f"bound-ratio wgrad upb={p['upb']} {shape} db relative error {rdb:.3g} (allowed 2e-05)")
    assert rdb < 2e-5
    r2 = float((outs[1][0] - dw0).norm() / (dw0.norm() + 1e-20)); r2b = float((outs[1][1] - db0).norm() / (db0.norm() + 1e-20))
    print(f"bound-ratio wgrad {shape} algo 2 against algo 0: dw {r2:.3g} db {r2b:.3g} (allowed 3e-05)")
    assert r2 < 3e-5 and r2b < 3e-5


# ---- the pooled-sums data gradient, 16-row instance ----------------------------------------------------------------------------------------------------------------------
def test_pooled_sums_data_gradient_on_the_16_row_instance(ops):
    """unet_conv3x3_bwd_data_pool_sums at (1, 126, 250, 512 -> 16), rate 0.25: conv_h2_kernel<0, 2, 4, 2, 2>, last row tile 14 rows, last column tile 26 columns.  The
    references and tolerances of test_conv3x3_dgrad_with_pooled_sums_in_the_epilogue (restated; inputs drawn on the device): dx equals the plain data gradient bit for
    bit, the sums equal unet_maxpool2x2_dropout_bwd_sums on (pooled, dx) to 2e-6 of the largest, the gamma = 0 channel has no xhat term -- and dx per element within
    EPS_SPLIT A1 of the float64 data gradient."""
    (n, h, w, cin, cout), rate = F.POOL_CASE
    assert F.pool_sums_form(n, h, w, cin) == F.POOL_FORMS[1]
    assert ops.lib.unet_conv3x3_bwd_data_pool_sums_supported(ops.h, 0, w, cin, cout) == 1
    g = torch.Generator(device=DEV); g.manual_seed(cin + h)
    rng = np.random.default_rng(cin + h)
    xe = (torch.randn((n, 2 * h, 2 * w, cin), generator=g, device=DEV, dtype=F32) + 0.2).clamp_min(0.0)
    ge = rng.uniform(0.5, 1.5, cin).astype(np.float32); be = (rng.standard_normal(cin) * 0.3).astype(np.float32)
    ge[3] = 0.0; be[3] = 0.0; ge[5] = -0.7
    es = ops.z(2 * cin, dtype=torch.float64); bnp = ops.z(4 * cin); pooled = ops.z(n, h, w, cin); ybn = ops.z(n, 2 * h, 2 * w, cin)
    pix = n * 4 * h * w
    ops.ck(ops.lib.unet_bn_stats(ops.h, xe.data_ptr(), cin, es.data_ptr(), pix, cin, ops.s), "stats")
    ops.ck(ops.lib.unet_bn_finalize_train(ops.h, es.data_ptr(), float(pix), ops.d(ge).data_ptr(), ops.d(be).data_ptr(), ops.z(cin).data_ptr(), ops.z(cin).data_ptr(), bnp.data_ptr(), cin, ops.s), "fin")
    ops.ck(ops.lib.unet_bn_apply_maxpool_dropout_fwd(ops.h, xe.data_ptr(), cin, bnp.data_ptr(), ybn.data_ptr(), cin, pooled.data_ptr(), n, 2 * h, 2 * w, cin, rate, 77, ops.s), "pool fwd")
    removed = torch.signbit(pooled) & (pooled == 0)
    assert abs(float(removed.double().mean()) - rate) < 0.02 and bool((pooled[..., 3] == 0).all()) and 0.1 < float(torch.signbit(pooled[..., 3]).double().mean()) < 0.9
    k = dv(rng.standard_normal((3, 3, cin, cout)) * (2.0 / (9 * cin)) ** 0.5); dy = dv(rng.standard_normal((n, h, w, cout)))
    dx0, dx1 = image(n, h, w, cin), image(n, h, w, cin)
    s0 = ops.z(2 * cin, dtype=torch.float64); s1 = ops.z(2 * cin, dtype=torch.float64)
    ops.ck(ops.lib.unet_conv3x3_bwd_data(ops.h, dy.data_ptr(), k.data_ptr(), None, 0, 0.0, 0, dx0.ptr(), ops.wws(cin, cout), n, h, w, cin, cout, 0, ops.s), "dgrad")
    ops.ck(ops.lib.unet_maxpool2x2_dropout_bwd_sums(ops.h, pooled.data_ptr(), dx0.ptr(), ops.d(ge).data_ptr(), ops.d(be).data_ptr(), s0.data_ptr(), n, 2 * h, 2 * w, cin, rate, 77, ops.s), "sums pass")
    s1 += 1.0                                                        # the sums are ADDED to what is there
    ops.ck(ops.lib.unet_conv3x3_bwd_data_pool_sums(ops.h, dy.data_ptr(), k.data_ptr(), pooled.data_ptr(), ops.d(ge).data_ptr(), ops.d(be).data_ptr(), rate, dx1.ptr(),
                                                   s1.data_ptr(), ops.wws(cin, cout), n, h, w, cin, cout, ops.s), "dgrad + sums")
    dx0.check("plain dgrad"); dx1.check("dgrad + pooled sums")
    assert torch.equal(dx1.t, dx0.t)
    a, b = s0.cpu().numpy(), s1.cpu().numpy() - 1.0
    scale = np.abs(a).max()
    print(f"bound-ratio pooled sums <{F.POOL_FORMS[1]}> {F.POOL_CASE[0]} {np.abs(a - b).max() / (2e-6 * scale + 1e-9):.3g}")
    assert np.abs(a - b).max() < 2e-6 * scale + 1e-9, (np.abs(a - b).max(), scale)
    assert b[cin + 3] == 0.0                                         # gamma = 0: no xhat term (as the separate pass)
    B.check_elem(dx1.t, B.dgrad64(dy.double(), k.double()), EPS_SPLIT * B.dgrad64(dy.double().abs(), k.double().abs()), f"pooled sums <{F.POOL_FORMS[1]}> {F.POOL_CASE[0]} dx")

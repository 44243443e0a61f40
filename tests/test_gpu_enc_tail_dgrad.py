"""-m gpu: the skip half of a folded decoder BatchNorm's data gradient finished inside the encoder tail's backward (UNET_OPT_ENC_TAIL_DGRAD).

Op level -- unet_conv3x3_bnfold_bwd_data_enc_tail through the C ABI, the EPI 5 instances of conv_h2_kernel (one-block workgroups on the two-block image at C = 32, a
range of the two-block groups from C = 64 on):

  (A) every element against a float64 reference on the CPU.  x, the encoder scale and the encoder shift are small dyadic numbers, so y = fmaf(x, sc, sh) is exact in fp32
      and the 2x2 arg-max -- post-ReLU x is full of exact ties -- is the same decision in float64 (numpy.argmax: the first maximum, argmax4's rule).  The bound:

        dx = x > 0 ? sc (t - k1 - (x - mean) istd k2) : 0,   t = kk y + (K0 dz + K2) + sel g,   g = dy_pooled keep
        |dx - ref| <= |sc| (|K0| EPS_SPLIT A1 + 10 u S),     A1 = sum |dy| |w| over the skip channel's taps (the h2 product bound, gpu_util.EPS_SPLIT),
        S = |K0 dz| + |K2| + |kk y| + |sel g| + |k1| + |(x - mean) istd k2|

      Ten fp32 unit round-offs u of the pointwise terms' magnitudes: the longest chain is nine -- K2 is rounded when k_bn_bwd_coef stores it, its sums and products
      before that twice more (the allowance tests/bnfold_checks.py gives K0 dz + K2: four), then fmaf(kk, y, .), the addition of the pooled gradient, the subtraction
      of k1, the subtraction of the xhat term and the product with sc, one each; the xhat term itself carries four (x - mean, istd, k2 and k2's own rounding) plus the
      last two; g one (the keep factor) plus the last four -- and one to spare.  Where x <= 0 the bound is 0: the result must be exactly 0.  No element is excluded.

  (B) against today's two launches on the device with skip_k1 = NULL: unet_conv3x3_bnfold_bwd_data (x_channels = C) then unet_bn_maxpool_bwd_apply on its skip half.
      The pointwise operations are the same ones in the same order, so what may differ is the conv part (the two paths tile the image differently at these sizes: other
      block exponents): |new - old| <= 2 |sc K0| EPS_SPLIT A1.  The arg-max elements -- those whose output moves when dy_pooled is replaced by zeros -- are the same set
      on both paths, and that set is the reference's.  The share of bit-equal elements is printed, not asserted.

Model level -- HipUNet at 64 x 64 batch 2 and 32 x 64 batch 3 with the option at 0, 1 and 2 (2 = every level whatever its size: at these sizes the shape rule of value 1
keeps every level on the old pair, so only 2 runs the new launches): same loss, same op names, every gradient within the bounds test_live_oracle_all_grads_and_taps holds
the default engine to (activation gradients 2e-4, parameter gradients 3e-4, relative L2 against the float64 oracle on the engine's own ReLU / max-pool decisions).

Measured on an MI355X (256 CUs; run with -s): (A) worst error / bound 0.11 / 0.13 / 0.13 / 0.12 over the four cases (with skip_k1; 0.11 ... 0.13 without); (B) every element of
all four cases bit-equal to the two launches (share 1.0000, ratio 0), the arg-max sets equal; model: worst parameter gradient 2.2e-5 (c1b/bias, 64 x 64) and 3.1e-6 (c1a/bias,
32 x 64) relative, the same figure with the option at 0, 1 and 2; the activation gradients below relerr's absolute floor in every setting."""
import numpy as np
import pytest
import torch

import bnfold_checks as B
import philox_ref as PX
from gpu_util import EPS_SPLIT, U, Ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
# (n, h, w, C), rate, negative encoder scales: the one-block form | 32-column tile overhang, three row tiles, two-block groups | tile larger than the image, block range 2 of 4 |
# negative scales on a third of the channels over x with about half exact zeros
CASES = [((2, 16, 32, 32), 0.0, False), ((1, 24, 40, 64), 0.25, False), ((2, 8, 8, 128), 0.0, False), ((1, 16, 48, 32), 0.25, True)]
SEED = 0x5EED1234


@pytest.fixture(scope="module")
def ops():
    return Ops()


def make_case(shape, rate, neg, seed):
    n, h, w, c = shape
    rng = np.random.default_rng(seed)
    f32 = np.float32
    xs = np.maximum(rng.integers(-12, 13, (n, h, w, c)) / 4.0, 0.0).astype(f32)                    # max(grid, 0): about half exact zeros, many ties inside a window
    sc = (rng.integers(2, 13, c) / 8.0).astype(f32)
    if neg:
        sc[rng.permutation(c)[: c // 3]] *= -1.0
    sh = (rng.integers(-8, 9, c) / 4.0).astype(f32)
    assert ((xs * sc + sh).astype(f32) == xs.astype(np.float64) * sc + sh).all()                   # y is exact in fp32
    xcat = np.concatenate([rng.standard_normal((n, h, w, c)).astype(f32), xs], -1)
    enc_bnp = np.concatenate([sc, sh, rng.uniform(0.2, 1.5, c).astype(f32), rng.uniform(0.5, 2.0, c).astype(f32)])
    cnt = float(n * h * w)
    enc_sums = np.concatenate([rng.standard_normal(c) * 0.2, rng.standard_normal(c) * 0.3]) * cnt
    k = (rng.standard_normal((3, 3, 2 * c, c)) * np.sqrt(2.0 / (9 * c))).astype(f32)
    dy = rng.standard_normal((n, h, w, c)).astype(f32)
    dec = dict(scale=rng.uniform(0.4, 1.6, 2 * c).astype(f32), shift=(rng.standard_normal(2 * c) * 0.7).astype(f32), mean=rng.uniform(-1.0, 1.0, 2 * c).astype(f32),
               istd=rng.uniform(0.5, 2.0, 2 * c).astype(f32))
    dec_sums = np.concatenate([rng.standard_normal(2 * c) * 0.2, rng.standard_normal(2 * c) * 0.3]) * cnt
    return dict(shape=shape, rate=rate, xcat=xcat, enc_bnp=enc_bnp, enc_sums=enc_sums, k=k, dy=dy, dec=dec, dec_bnp=np.concatenate([dec["scale"], dec["shift"], dec["mean"], dec["istd"]]),
                dec_sums=dec_sums, kk=(rng.standard_normal(c) * 0.3).astype(f32), dyp=rng.standard_normal((n, h // 2, w // 2, c)).astype(f32), count=cnt)


_REF = {}


def reference(i):
    """float64 reference, bound and arg-max set of case i, computed once (with and without skip_k1)"""
    if i in _REF:
        return _REF[i]
    shape, rate, neg = CASES[i]
    cs = make_case(shape, rate, neg, 40 + i)
    n, h, w, c = shape
    t = B.t64
    x = t(cs["xcat"][..., c:]); sc, sh, mean, istd = (t(cs["enc_bnp"][j * c:(j + 1) * c]) for j in range(4))
    K0, _, K2 = B.bn_coef64(t(cs["dec"]["scale"]), t(cs["dec"]["mean"]), t(cs["dec"]["istd"]), t(cs["dec_sums"]), cs["count"])
    K0, K2 = K0[c:], K2[c:]
    dz = B.dgrad64(t(cs["dy"]), t(cs["k"]))[..., c:]; a1 = B.dgrad64(t(cs["dy"]).abs(), t(cs["k"]).abs())[..., c:]
    y = (x * sc + sh).numpy()
    win = np.stack([y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2]])          # argmax4's order; numpy.argmax: the first maximum
    kmax = win.argmax(0)
    sel = np.zeros((n, h, w, c))
    for j, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        sel[:, a::2, b::2] = kmax == j
    keep = PX.keep_scale_dense(cs["dyp"].shape, rate, SEED).astype(np.float64) if rate > 0 else np.ones(cs["dyp"].shape)
    g = t(np.repeat(np.repeat(cs["dyp"].astype(np.float64) * keep, 2, 1), 2, 2) * sel)
    k1, k2 = t(cs["enc_sums"][:c]) / cs["count"], t(cs["enc_sums"][c:]) / cs["count"]
    xhat_term = (x - mean) * istd * k2
    out = {}
    for tag, kk in (("k1", t(cs["kk"])), ("null", torch.zeros(c, dtype=B.F64))):
        tt = kk * t(y) + (K0 * dz + K2) + g
        ref = torch.where(x > 0, sc * (tt - k1 - xhat_term), torch.zeros_like(x))
        S = (K0 * dz).abs() + K2.abs() + (kk * t(y)).abs() + g.abs() + k1.abs() + xhat_term.abs()
        conv = sc.abs() * K0.abs() * EPS_SPLIT * a1
        bound = torch.where(x > 0, conv + sc.abs() * 10 * U * S, torch.zeros_like(x))
        out[tag] = dict(ref=ref, bound=bound, conv=conv)
    routed = ((x > 0) & (g != 0)).numpy()          # (sc is never 0) the elements the pooled gradient reaches and the ReLU mask lets through
    _REF[i] = (cs, out, routed)
    return _REF[i]


def run_new(ops, cs, skip_k1, dyp):
    n, h, w, c = cs["shape"]
    dx = torch.full((n, h, w, c), SENT, dtype=torch.float32, device=DEV)
    xcat = ops.d(cs["xcat"]); coef = ops.z(6 * c); es = torch.from_numpy(cs["enc_sums"]).cuda(); ds = torch.from_numpy(cs["dec_sums"]).cuda()
    ops.ck(ops.lib.unet_conv3x3_bnfold_bwd_data_enc_tail(ops.h, ops.d(cs["dy"]).data_ptr(), ops.d(cs["k"]).data_ptr(), ops.d(cs["dec_bnp"]).data_ptr(), ds.data_ptr(), cs["count"],
                                                         xcat.data_ptr() + 4 * c, 2 * c, ops.d(cs["enc_bnp"]).data_ptr(), es.data_ptr(), cs["count"],
                                                         ops.d(skip_k1).data_ptr() if skip_k1 is not None else None, ops.d(dyp).data_ptr(), cs["rate"], SEED, dx.data_ptr(),
                                                         ops.wws(2 * c, c), coef.data_ptr(), n, h, w, c, 0, ops.s), "enc tail dgrad")
    return dx.cpu().numpy()


def run_old(ops, cs, dyp):
    """today's pair: the data gradient with x_channels = C (the skip half leaves as K0 dz + K2), then the one-pass encoder tail on that half"""
    n, h, w, c = cs["shape"]
    dxcat = torch.full((n, h, w, 2 * c), SENT, dtype=torch.float32, device=DEV); dx = torch.full((n, h, w, c), SENT, dtype=torch.float32, device=DEV)
    xcat = ops.d(cs["xcat"]); coef = ops.z(6 * c); es = torch.from_numpy(cs["enc_sums"]).cuda(); ds = torch.from_numpy(cs["dec_sums"]).cuda()
    ops.ck(ops.lib.unet_conv3x3_bnfold_bwd_data(ops.h, ops.d(cs["dy"]).data_ptr(), ops.d(cs["k"]).data_ptr(), ops.d(cs["dec_bnp"]).data_ptr(), ds.data_ptr(), cs["count"], xcat.data_ptr(), c, 0,
                                                0.0, 0, dxcat.data_ptr(), ops.wws(2 * c, c), coef.data_ptr(), n, h, w, 2 * c, c, 0, ops.s), "fold dgrad")
    ops.ck(ops.lib.unet_bn_maxpool_bwd_apply(ops.h, xcat.data_ptr() + 4 * c, 2 * c, ops.d(cs["enc_bnp"]).data_ptr(), es.data_ptr(), cs["count"], dxcat.data_ptr() + 4 * c, 2 * c,
                                             ops.d(dyp).data_ptr(), dx.data_ptr(), c, n, h, w, c, cs["rate"], SEED, ops.s), "fused apply")
    return dx.cpu().numpy()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_enc_tail_entry_against_float64_per_element(ops, i):
    cs, P, _ = reference(i)
    for tag, kk in (("k1", cs["kk"]), ("null", None)):
        got = run_new(ops, cs, kk, cs["dyp"])
        assert np.isfinite(got).all()
        B.check_elem(got, P[tag]["ref"], P[tag]["bound"], f"enc tail {cs['shape']} rate {cs['rate']} skip_k1 {tag}")
    assert 0 <= ops.lib.unet_ctx_max_kernel_scratch_bytes(ops.h) <= 128


@pytest.mark.parametrize("i", range(len(CASES)))
def test_enc_tail_entry_against_the_two_launches(ops, i):
    cs, P, routed = reference(i)
    new, old = run_new(ops, cs, None, cs["dyp"]), run_old(ops, cs, cs["dyp"])
    print(f"bit-equal share {cs['shape']} rate {cs['rate']}: {float((new.view(np.uint32) == old.view(np.uint32)).mean()):.4f}")
    B.check_elem(new, torch.from_numpy(old.astype(np.float64)), 2.0 * P["null"]["conv"], f"enc tail vs two launches {cs['shape']}")
    zero = np.zeros_like(cs["dyp"])
    am_new = run_new(ops, cs, None, zero) != new; am_old = run_old(ops, cs, zero) != old
    # (a routed element whose pooled gradient is absorbed by the rounding of t would not move: none at these magnitudes -- the set equals the reference's)
    assert (am_new == am_old).all() and (am_new == routed).all(), (int(am_new.sum()), int(am_old.sum()), int(routed.sum()))


# ---- model level -------------------------------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def model_case(hw, n):
    """inputs, weights and the float64 oracle of one size, computed once and shared by the three option values"""
    from oracle import unet_oracle as O
    if (hw, n) not in _ORACLE:
        h, w_ = hw
        rng = np.random.default_rng(h + w_)
        wts = O.init_weights(seed=h)
        for k in wts:
            if k.endswith("/bias") or k.endswith("/beta"):
                wts[k] = (rng.standard_normal(wts[k].shape) * 0.1).astype(np.float32)
            if k.endswith("/gamma"):
                wts[k] = rng.uniform(0.5, 1.5, wts[k].shape).astype(np.float32)
        x = rng.random((n, h, w_, 1)).astype(np.float32)
        y = (np.round(rng.random((n, h, w_, 1)) ** 4 * 255) / 255).astype(np.float32)
        _ORACLE[(hw, n)] = dict(wts=wts, x=x, y=y, r=O.loss_and_grads(wts, x, y, dtype=torch.float64, want_acts=True), seen={})
    return _ORACLE[(hw, n)]


@pytest.mark.parametrize("value", [0, 1, 2])
@pytest.mark.parametrize("hw,n", [((64, 64), 2), ((32, 64), 3)])
def test_model_gradients_with_the_option(hw, n, value):
    from oracle import unet_oracle as O
    from test_gpu_model import make, relerr
    mc = model_case(hw, n)
    wts, x, y, r = mc["wts"], mc["x"], mc["y"], mc["r"]
    eng = make(hw[0], hw[1], dropout_rate=0.0, options={"enc_tail_dgrad": value})
    eng.set_weights(wts)
    ld = eng.forward_backward(x, y).cpu().numpy()
    assert abs(ld[0] - r["loss"]) < 1e-5 and abs(ld[1] - r["dice"]) < 1e-5
    fwd = [o[0] for o in eng.op_profile(n, 0)]; bwd = [o[0] for o in eng.op_profile(n, 1)]
    for k in range(1, 5):
        assert f"bn_pool_bwd_apply:bn{k}" in bwd and f"conv3x3_dgrad_bn_bwd:c{10 - k}a" in bwd
    # the new launches run where the option says so: a gradient tap of bn<k> exists only where the skip half of the concat's gradient is still written
    on = 0
    for k in range(1, 5):
        try:
            eng.tap(n, f"bn{k}", grad=True)
        except Exception:
            on += 1
    assert on == (4 if value == 2 else 0), (value, on)          # (value 1: these sizes leave resident slots empty at every level -- the shape rule keeps the old pair)
    seen = mc["seen"].setdefault("first", dict(fwd=fwd, bwd=bwd))
    assert fwd == seen["fwd"] and bwd == seen["bwd"]          # the same op names in every setting (the loss: test_model_loss_is_identical below)
    convs = [f"c{k}{ab}" for k in range(1, 10) for ab in "ab"]
    emasks = {name: (eng.tap(n, name) > 0) for name in convs}
    flips = sum(int((emasks[name] != (r["acts"][name] > 0)).sum()) for name in convs)
    assert flips <= 1e-5 * sum(m.size for m in emasks.values()) + 8, flips
    if flips:
        r = O.loss_and_grads(wts, x, y, dtype=torch.float64, want_acts=True, relu_masks={k: m.astype(np.float64) for k, m in emasks.items()},
                             pool_sel={f"p{k}": O.pool_selection(eng.tap(n, f"bn{k}")) for k in (1, 2, 3, 4)})
    tol_a, tol_g = 2e-4, 3e-4                                   # test_live_oracle_all_grads_and_taps
    for name, masked in (("c9a", True), ("u9", False), ("c5b", True), ("p4", False), ("c4b", True), ("c3b", True), ("c2b", True), ("c1b", True), ("c1a", True)):
        want = r["act_grads"][name] * ((eng.tap(n, name) > 0) if masked else 1.0)
        e = relerr(eng.tap(n, name, grad=True), want)
        print(f"relerr option {value} {hw} d{name} {e:.3g}")
        assert e < tol_a, (name, flips)
    g = eng.get_grads()
    worst = max((relerr(g[k], r["grads"][k]), k) for k in g)
    print(f"relerr option {value} {hw} worst parameter gradient {worst[0]:.3g} ({worst[1]})")
    for k in g:
        assert relerr(g[k], r["grads"][k]) < tol_g, (k, flips)


@pytest.mark.parametrize("hw,n", [((64, 64), 2), ((32, 64), 3)])
def test_model_loss_is_identical(hw, n):
    """the option changes nothing in front of the loss: bit-identical loss and Dice.  Deterministic mode, because the default mode's BatchNorm statistics go through fp64
    atomics whose order is free (two runs of ONE setting may differ in the last bit there); the new launches have no reduction, so they run in that mode as well"""
    from test_gpu_model import make
    mc = model_case(hw, n)
    out = []
    for value in (0, 1, 2):
        eng = make(hw[0], hw[1], dropout_rate=0.0, options={"enc_tail_dgrad": value, "deterministic": 1})
        eng.set_weights(mc["wts"])
        out.append(eng.forward_backward(mc["x"], mc["y"]).cpu().numpy().copy())
    assert (out[0] == out[1]).all() and (out[0] == out[2]).all(), out

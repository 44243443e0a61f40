"""The short kernels at the end of a step and the classifier's fp32 tail, PER ELEMENT against float64 through the C ABI: unet_dense_fwd / _bwd (fp32),
unet_cls_head_fwd / _bwd / unet_cls_loss_finalize, unet_adam_keras, unet_seg_metrics_sweep (default and deterministic mode), unet_gather_samples, unet_zero,
unet_cast_f32_to_bf16 / _bf16_to_f32.  References and allowances: tests/tail_checks.py (derived from each kernel's summation order; checked on the CPU against an
fp32 emulation and planted defects by tests/test_tail_bounds_host.py).  Every test asserts error / allowance <= 1 for every element and prints `bound-ratio` lines;
gather, zero and the casts are bit-exact.  Outputs lie inside one allocation between sentinel elements that must survive; the split-K scratch is poisoned between
two runs that must agree in every bit.

Measured on the MI355X (worst error / allowance per check over all cases of this file):
  dense fwd 0.017 (act 0), 0.015 (ReLU), 0.015 (ELU), 0.020 (one non-zero row, dropout); dense dx 0.67, dw 0.75 (B = 1: one product, one
  rounding), 0.64 at B = 3, at most 0.33 from B = 8 on (with one non-zero x row dw is ONE product under an allowance of B roundings: 0.004 at B = 257; a row taken
  from the wrong place is of order 1)
  head p 0.45, loss / f1 sums 0.075 (counts exact), finalize 0.74 (one fp32 rounding), dh 0.46, dw 0.051, db 0.083, db1 0.042
  Adam p 0.998 (where the step is far below p the allowance IS the one rounding of the subtract), m 0.62, v 0.60
  sweep 0.15 in both modes, counts exact; deterministic against default mode 0: both add the same fp32 workgroup partials in fp64, where a sum of at most 1024 of
  them is exact in any order -- the bound stays the derived one, it is the fp32 part of the chain that it allows for (0.15 against the reference)
  gather, zero, casts: bit-exact (a NaN stays a NaN; the quiet NaN 0x7FC00000 becomes 0x7FC0)
The dense forward sits at 0.015-0.02 because its allowance adds the depth of the longest chain (up to 166 roundings at K = 50176) linearly while rounding errors
of random signs grow with its square root; a dropped row or chunk is of order 1 against it (tests/test_tail_bounds_host.py plants them).
Transcendental constants (test_transcendental_constants; in units of u |value|, resp. u (|logit| + 1) for the loss row; in use = twice the measurement, rounded up):
  expm1f 1.26 -> C_EXPM1 = 3;  expf + add + divide of the sigmoid 1.76 -> C_SIGMOID = 4;  one loss row (logf, expf, log1pf, six plain operations) 2.9 -> C_BCE = 6
Wall time of the file on the MI355X: 5.5 s for its 71 tests; the longest are Adam at 4.2 M elements (0.8 s each, three steps with a float64 reference), the
deterministic sweep (0.5 s) and the sweep at the grid cap (0.24 s); the gather from a 2 GiB source takes under 0.1 s."""
import numpy as np
import pytest
import torch

import tail_checks as T

pytestmark = pytest.mark.gpu

SENT = 7.0
GUARD = 64                                    # sentinel floats in front of and behind every output (256 bytes: the 16-byte alignment of the tensor is kept)
E_ARG = -1
STRIDE4 = T.MAX_BLOCKS * T.TPB * 4            # elements one pass of a float4 grid-stride kernel covers
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def ops():
    from gpu_util import Ops
    return Ops()


def guarded(numel, dtype=torch.float32, fill=SENT):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + numel]


def guards_kept(buf, what, fill=SENT):
    b = buf.cpu()
    bad = int((b[:GUARD] != fill).sum() + (b[-GUARD:] != fill).sum())
    assert bad == 0, f"{what}: {bad} sentinel elements in front of / behind the output were overwritten"


def ck(ops, rc, what, handle=None):
    if rc != 0:
        msg = ops.lib.unet_last_error(handle if handle is not None else ops.h)
        raise AssertionError(f"{what}: status {rc}: {msg.decode() if msg else '?'}")
    torch.cuda.synchronize()


def rejected(ops, rc, what):
    torch.cuda.synchronize()
    msg = ops.lib.unet_last_error(ops.h)
    assert rc == E_ARG and msg, f"{what}: expected UNET_E_ARG with a message, got {rc} {msg!r}"


def host(t):
    return t.cpu().numpy()


# ---- dense, fp32 ----------------------------------------------------------------------------------------------------------------------------
# (1,4,4) smallest accepted; (9,260,32) kn = 4 in chunk 2, B one past a row group of 8; (8,256,32) one chunk; (3,768,8) odd chunk count; (65,512,4) a row group
# of 64 plus 1; (129,516,16) / (257,300,32) second and third dy tile with nb < DB, K no multiple of the 256 threads; (32,50176,32) the classifier's own, 196 chunks
DENSE_SHAPES = [(1, 4, 4), (9, 260, 32), (8, 256, 32), (3, 768, 8), (65, 512, 4), (129, 516, 16), (257, 300, 32), (32, 50176, 32)]


def dense_fwd(ops, xd, wd, bd, b, k, n, act, rate, seed, ws, nb, what):
    ybuf, y = guarded(b * n)
    ck(ops, ops.lib.unet_dense_fwd(ops.h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bd is not None else None, y.data_ptr(), b, k, n, act, rate, seed,
                                   ws.data_ptr(), nb, ops.s), what)
    guards_kept(ybuf, what)
    return host(y).reshape(b, n)


@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_fp32_per_element(ops, shape):
    b, k, n = shape
    nb = ops.lib.unet_dense_ws_bytes(b, k, n)
    assert nb == T.cdiv(k, T.DK) * b * n * 4
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    for sparse in (False, True):
        x, w, bias, dy = T.dense_case(shape, sparse=sparse)
        xd, wd, bd, dyd = ops.d(x), ops.d(w), ops.d(bias), ops.d(dy)
        variants = ((0, None, 0.0, 0), (1, bias, 0.4, 99)) if sparse else ((0, bias, 0.0, 0), (1, bias, 0.0, 0), (2, bias, 0.0, 0), (0, None, 0.0, 0), (1, bias, 0.4, 99))
        for act, bb, rate, seed in variants:
            what = f"dense fwd {shape}{' sparse' if sparse else ''} act={act} bias={bb is not None} rate={rate}"
            ws.fill_(0xFF)                                                # the split-K scratch holds NaN patterns: every word that is read was written by this launch
            got = dense_fwd(ops, xd, wd, bd if bb is not None else None, b, k, n, act, rate, seed, ws, nb, what)
            T.check_dense_fwd(got, x, w, bb, act, rate, seed, what)
            ws.fill_(0x7F)
            T.bits_equal(dense_fwd(ops, xd, wd, bd if bb is not None else None, b, k, n, act, rate, seed, ws, nb, what), got, what + ": rerun")
        what = f"dense bwd {shape}{' sparse' if sparse else ''}"
        outs = []
        for with_dx in (True, False, True):
            dxbuf, dx = guarded(b * k); dwbuf, dw = guarded(k * n)
            ck(ops, ops.lib.unet_dense_bwd(ops.h, xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), dx.data_ptr() if with_dx else None, dw.data_ptr(), b, k, n, ops.s), what)
            guards_kept(dxbuf, what + " dx"); guards_kept(dwbuf, what + " dw")
            outs.append((host(dx).reshape(b, k), host(dw).reshape(k, n)))
        T.check_dense_bwd(outs[0][0], outs[0][1], x, w, dy, what)
        assert (outs[1][0] == SENT).all(), "dx = NULL: nothing may be written"
        T.bits_equal(outs[1][1], outs[0][1], what + ": dw with dx = NULL")
        T.bits_equal(outs[2][0], outs[0][0], what + ": dx rerun"); T.bits_equal(outs[2][1], outs[0][1], what + ": dw rerun")


def test_dense_rejections_launch_nothing(ops):
    b, k, n = 9, 260, 32
    x, w, bias, dy = T.dense_case((b, k, n))
    xd, wd, bd = ops.d(x), ops.d(w), ops.d(bias)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    ybuf, y = guarded(b * 64)

    def fwd(kk, nn, nbytes):
        return ops.lib.unet_dense_fwd(ops.h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), b, kk, nn, 1, 0.0, 0, ws.data_ptr(), nbytes, ops.s)

    rejected(ops, fwd(258, 32, ws.numel()), "k % 4 != 0")
    rejected(ops, fwd(256, 12, ws.numel()), "n = 12")
    rejected(ops, fwd(64, 64, ws.numel()), "n = 64")
    rejected(ops, fwd(k, n, ops.lib.unet_dense_ws_bytes(b, k, n) - 1), "workspace one byte short")
    dwbuf, dw = guarded(k * 64)
    rejected(ops, ops.lib.unet_dense_bwd(ops.h, xd.data_ptr(), wd.data_ptr(), ops.d(dy).data_ptr(), None, dw.data_ptr(), b, 256, 12, ops.s), "bwd n = 12")
    rejected(ops, ops.lib.unet_dense_bwd(ops.h, xd.data_ptr(), wd.data_ptr(), ops.d(dy).data_ptr(), None, dw.data_ptr(), b, 64, 64, ops.s), "bwd n = 64")
    assert (ybuf == SENT).all() and (dwbuf == SENT).all() and not ws.any(), "a rejected call wrote something"


# ---- classifier head ------------------------------------------------------------------------------------------------------------------------
CW = (0.7, 1.9)


def head_fwd(ops, hd, wd, bd, td, b, n, sums, what):
    pbuf, p = guarded(b)
    ck(ops, ops.lib.unet_cls_head_fwd(ops.h, hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), p.data_ptr(), td.data_ptr() if td is not None else None, CW[0], CW[1],
                                      sums.data_ptr() if sums is not None else None, b, n, ops.s), what)
    guards_kept(pbuf, what)
    return host(p)


@pytest.mark.parametrize("n", [4, 8, 16, 32])
@pytest.mark.parametrize("b", [1, 7, 256, 257, 300])
def test_cls_head_per_element(ops, b, n):
    for bias_v in (0.0, 0.1):
        h, w, bias, t = T.head_case(b, n, seed=int(bias_v * 10))
        bias[0] = bias_v
        hd, wd, bd, td = ops.d(h), ops.d(w), ops.d(bias), ops.d(t)
        what = f"cls head B={b} N={n} bias={bias_v}"
        sums = ops.z(4, dtype=torch.float64)
        p = head_fwd(ops, hd, wd, bd, td, b, n, sums, what)
        s1 = host(sums).copy()
        T.check_head_fwd(p, s1, h, w, bias, t, *CW, what + " fwd")
        if bias_v == 0.0:
            assert p[0] == 1.0 and (b < 2 or p[1] == 0.5), "the special rows: saturated / exactly one half"
        p2 = head_fwd(ops, hd, wd, bd, td, b, n, sums, what)                     # a second call ADDS onto the same sums
        T.bits_equal(p2, p, what + ": p rerun")
        T.check_head_fwd(p2, host(sums), h, w, bias, t, *CW, what + " fwd, second call on top", pre=s1)
        T.bits_equal(head_fwd(ops, hd, wd, bd, None, b, n, None, what), p, what + ": p without labels")
        out = ops.z(2)
        ck(ops, ops.lib.unet_cls_loss_finalize(ops.h, sums.data_ptr(), float(2 * b), out.data_ptr(), ops.s), what + " finalize")
        T.ratio(host(out), *T.finalize_ref(host(sums), 2.0 * b), what + " finalize")
        pd = ops.d(p)
        bufs = {k_: guarded(sz) for k_, sz in (("dh", b * n), ("dw", n), ("db", 1), ("db1", n))}
        ck(ops, ops.lib.unet_cls_head_bwd(ops.h, hd.data_ptr(), wd.data_ptr(), pd.data_ptr(), td.data_ptr(), CW[0], CW[1], float(b), 0.4, bufs["dh"][1].data_ptr(),
                                          bufs["dw"][1].data_ptr(), bufs["db"][1].data_ptr(), bufs["db1"][1].data_ptr(), b, n, ops.s), what + " bwd")
        for k_, (buf, _) in bufs.items():
            guards_kept(buf, f"{what} bwd {k_}")
        got = {k_: host(v) for k_, (_, v) in bufs.items()}
        got["dh"] = got["dh"].reshape(b, n)
        T.check_head_bwd(got, h, w, p, t, *CW, float(b), 0.4, what + " bwd")
        outside = (p < T.LO32) | (p > T.HI32)
        assert not got["dh"][outside].any() and not got["dh"][h <= 0].any()          # exactly 0: outside the clip range, and wherever h <= 0
        if bias_v == 0.0:
            assert outside[:min(b, 8)].sum() >= min(b, 8) - 1, "the clip arm did not run"


def test_cls_head_forward_takes_any_multiple_of_4_the_backward_a_power_of_two(ops):
    """what include/unet_hip.h says of the two entry points' n"""
    b, n = 7, 12
    h, w, bias, t = T.head_case(b, n)
    hd, wd, bd, td = ops.d(h), ops.d(w), ops.d(bias), ops.d(t)
    sums = ops.z(4, dtype=torch.float64)
    p = head_fwd(ops, hd, wd, bd, td, b, n, sums, "cls head N=12")
    T.check_head_fwd(p, host(sums), h, w, bias, t, *CW, "cls head fwd N=12")
    dhbuf, dh = guarded(b * 64); small = ops.z(3, 64); small.fill_(SENT)
    for nn in (12, 64, 2):
        rejected(ops, ops.lib.unet_cls_head_bwd(ops.h, hd.data_ptr(), wd.data_ptr(), ops.d(p).data_ptr(), td.data_ptr(), CW[0], CW[1], float(b), 0.4, dh.data_ptr(),
                                                small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr(), b, nn, ops.s), f"cls head bwd n = {nn}")
    rejected(ops, ops.lib.unet_cls_head_fwd(ops.h, hd.data_ptr(), wd.data_ptr(), bd.data_ptr(), dh.data_ptr(), td.data_ptr(), CW[0], CW[1], sums.data_ptr(), b, 6, ops.s),
             "cls head fwd n = 6")
    assert (dhbuf == SENT).all() and (small == SENT).all(), "a rejected call wrote something"


def test_cls_loss_finalize_without_positives_is_zero_not_nan(ops):
    sums = torch.tensor([12.5, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda"); out = ops.z(2); out.fill_(SENT)
    ck(ops, ops.lib.unet_cls_loss_finalize(ops.h, sums.data_ptr(), 50.0, out.data_ptr(), ops.s), "finalize")
    got = host(out)
    assert got[0] == 0.25 and got[1] == 0.0, got
    sums = torch.tensor([1.0, 3.0, 4.0, 6.0], dtype=torch.float64, device="cuda")
    ck(ops, ops.lib.unet_cls_loss_finalize(ops.h, sums.data_ptr(), 8.0, out.data_ptr(), ops.s), "finalize")
    T.ratio(host(out), *T.finalize_ref([1.0, 3.0, 4.0, 6.0], 8.0), "finalize f1 = 0.6")


def test_transcendental_constants(ops):
    """measures the three constants of tail_checks.py where the pre-activation is exact, prints them, and holds them to the constants in use (twice the measurement)"""
    rng = np.random.default_rng(7)
    nrow = 4096
    # expm1f: dense K = 4, N = 4, x = (z, 0, 0, 0), W row 0 = 1, no bias: the pre-activation is z itself
    z = -(10.0 ** rng.uniform(-6, np.log10(20.0), nrow)).astype(f32)
    x = np.zeros((nrow, 4), f32); x[:, 0] = z
    w = np.zeros((4, 4), f32); w[0] = 1.0
    nb = ops.lib.unet_dense_ws_bytes(nrow, 4, 4); ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    y = dense_fwd(ops, ops.d(x), ops.d(w), None, nrow, 4, 4, 2, 0.0, 0, ws, nb, "elu of an exact z")
    ref = np.expm1(z.astype(f64))
    c_expm1 = float((np.abs(y[:, 0] - ref) / (T.U * np.abs(ref))).max())
    # expf + add + divide: head N = 4, h = |z| on column 0 (w = 1) or 1 (w = -1), bias = 0
    z = rng.uniform(-80.0, 17.0, nrow).astype(f32)
    h = np.zeros((nrow, 4), f32); h[np.arange(nrow), (z < 0).astype(int)] = np.abs(z)
    wv = np.array([1.0, -1.0, 0.0, 0.0], f32); zero = np.zeros(1, f32)
    p = head_fwd(ops, ops.d(h), ops.d(wv), ops.d(zero), None, nrow, 4, None, "sigmoid of an exact z")
    ref = 1.0 / (1.0 + np.exp(-z.astype(f64)))
    c_sig = float((np.abs(p - ref) / (T.U * ref)).max())
    # one loss row per launch (batch 1): sums[0] is cw bce of that row, from the kernel's own p
    rows = 512
    z = rng.uniform(-30.0, 30.0, rows).astype(f32); z[:8] = [0.0, 1e-3, -1e-3, 16.0, -16.0, 25.0, -25.0, 15.9]
    t = rng.choice(np.array([0.0, 1.0, 0.5, 0.3], f32), rows).astype(f32)
    h = np.zeros((rows, 4), f32); h[np.arange(rows), (z < 0).astype(int)] = np.abs(z)
    hd, td, wd, bd = ops.d(h), ops.d(t), ops.d(wv), ops.d(zero)
    pd = ops.z(rows); sums = ops.z(rows, 4, dtype=torch.float64)
    for i in range(rows):
        rc = ops.lib.unet_cls_head_fwd(ops.h, hd.data_ptr() + 16 * i, wd.data_ptr(), bd.data_ptr(), pd.data_ptr() + 4 * i, td.data_ptr() + 4 * i, CW[0], CW[1],
                                       sums.data_ptr() + 32 * i, 1, 4, ops.s)
        assert rc == 0
    torch.cuda.synchronize()
    bce, logit, _, _ = T._bce64(host(pd), t)
    cw = np.where(t >= 0.5, f64(f32(CW[1])), f64(f32(CW[0])))
    c_bce = float((np.abs(host(sums)[:, 0] - cw * bce) / (cw * T.U * (np.abs(logit) + 1))).max())
    print(f"measured-constant expm1 {c_expm1:.3g} (in use {T.C_EXPM1}) sigmoid {c_sig:.3g} (in use {T.C_SIGMOID}) bce-row {c_bce:.3g} (in use {T.C_BCE})")
    assert c_expm1 <= T.C_EXPM1 and c_sig <= T.C_SIGMOID and c_bce <= T.C_BCE, (c_expm1, c_sig, c_bce)


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
ADAM = dict(b1=0.9, b2=0.999, eps=1e-7)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, 2 * STRIDE4 + 7])
@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_adam_per_element_three_steps(ops, n, gs):
    """p, g, m, v are carved from ONE tensor (each slot padded to a multiple of 4 floats so that it starts on 16 bytes); the pads, 64 floats in front and the
    trailing 64 hold a sentinel that must survive.  Each step is checked against the float64 step from the state the kernel itself left."""
    npad = (n + 3) // 4 * 4
    p, g, m, v = T.adam_case(n)
    buf = torch.full((GUARD + 4 * npad + 64,), SENT, dtype=torch.float32, device="cuda")
    slot = [buf[GUARD + i * npad:GUARD + i * npad + n] for i in range(4)]
    for s_, a in zip(slot, (p, g, m, v)):
        s_.copy_(torch.from_numpy(a))
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    for i in range(4):
        inside[GUARD + i * npad:GUARD + i * npad + n] = True
    for step in (1, 2, 3):
        lr_t = T.adam_lr_t(step)
        ck(ops, ops.lib.unet_adam_keras(ops.h, slot[0].data_ptr(), slot[1].data_ptr(), slot[2].data_ptr(), slot[3].data_ptr(), n, lr_t, ADAM["b1"], ADAM["b2"],
                                        ADAM["eps"], gs, ops.s), "adam")
        whole = buf.cpu()
        assert bool((whole[~inside] == SENT).all()), f"adam n={n}: a sentinel around the buffers was overwritten"
        got = [whole[GUARD + i * npad:GUARD + i * npad + n].numpy().copy() for i in range(4)]
        T.bits_equal(got[1], g, "adam: g is read only")
        T.check_adam((got[0], got[2], got[3]), p, g, m, v, lr_t, gs=gs, what=f"adam n={n} gs={gs} step {step}", **ADAM)
        p, m, v = got[0], got[2], got[3]


# ---- metric sweep ---------------------------------------------------------------------------------------------------------------------------
SWEEP_COUNTS = [1, 255, 4551, 1024 * 2048 + 3 * 256 + 5]          # the last: the 1024-workgroup cap is reached, L = 9


def sweep(ops, handle, pd, gd, thr, out, n):
    rc = ops.lib.unet_seg_metrics_sweep(handle, pd.data_ptr(), gd.data_ptr(), ops.d(thr).data_ptr(), len(thr), out.data_ptr(), n, ops.s)
    ck(ops, rc, "sweep", handle)


@pytest.mark.parametrize("n", SWEEP_COUNTS)
def test_metrics_sweep_per_element(ops, n):
    assert T.sweep_grid(n) == {1: (1, 1), 255: (1, 1), 4551: (3, 6)}.get(n, (1024, 9))
    for nthr in (1, 8, 9, 17):
        p, gt, thr = T.sweep_case(n, nthr)
        assert (p[:4096, None] == thr[None, :]).any(), "no p == threshold tie in this case"
        pre = np.arange(3.0 * nthr).reshape(nthr, 3) + np.array([0.25, 0.0, 0.5])          # `out` is added to
        obuf, out = guarded(3 * nthr, torch.float64)
        out.copy_(torch.from_numpy(pre.reshape(-1)))
        sweep(ops, ops.h, ops.d(p), ops.d(gt), thr, out, n)
        guards_kept(obuf, "sweep")
        T.check_sweep(host(out), p, gt, thr, f"sweep n={n} T={nthr}", pre=pre)


def test_metrics_sweep_deterministic_mode(ops):
    """a private context with UNET_OPT_DETERMINISTIC: one slot copy per workgroup column, folded in index order, thresholds in rounds of 680"""
    from covidseg_amd import _lib
    ctx = _lib.Context.get(torch.cuda.current_device(), {"deterministic": 1}, private=True)
    fresh = None
    try:
        cases = [(n, nthr) for n in SWEEP_COUNTS for nthr in (1, 8, 9, 17)] + [(4551, T.SLOT_THRESHOLDS), (4551, T.SLOT_THRESHOLDS + 1), (4551, 2 * T.SLOT_THRESHOLDS + 1)]
        for n, nthr in cases:
            p, gt, thr = T.sweep_case(n, nthr)
            pd, gd = ops.d(p), ops.d(gt)
            outs = []
            for rep in range(2):
                obuf, out = guarded(3 * nthr, torch.float64, fill=0.0); obuf.fill_(SENT); out.zero_()
                sweep(ops, ctx.handle, pd, gd, thr, out, n)
                guards_kept(obuf, "deterministic sweep")
                outs.append(host(out).reshape(nthr, 3))
            T.bits_equal(outs[1], outs[0], f"deterministic sweep n={n} T={nthr}: rerun")
            T.check_sweep(outs[0], p, gt, thr, f"deterministic sweep n={n} T={nthr}")
            plain = ops.z(3 * nthr, dtype=torch.float64)
            sweep(ops, ops.h, pd, gd, thr, plain, n)
            plain = host(plain).reshape(nthr, 3)
            assert np.array_equal(plain[:, 1], outs[0][:, 1])
            T.ratio(outs[0], plain, T.sweep_ref(p, gt, thr)[1], f"deterministic against default sweep n={n} T={nthr}")
        # the slot copies were left all zero: the next launch gives the bits of a context that has never run anything
        n, nthr = 4551, 17
        p, gt, thr = T.sweep_case(n, nthr, seed=1)
        used = ops.z(3 * nthr, dtype=torch.float64); new = ops.z(3 * nthr, dtype=torch.float64)
        sweep(ops, ctx.handle, ops.d(p), ops.d(gt), thr, used, n)
        fresh = _lib.Context.get(torch.cuda.current_device(), {"deterministic": 1}, private=True)
        sweep(ops, fresh.handle, ops.d(p), ops.d(gt), thr, new, n)
        T.bits_equal(host(used), host(new), "deterministic sweep: a used context against a fresh one")
    finally:
        torch.cuda.synchronize()
        ctx.close()
        if fresh is not None:
            fresh.close()


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------
def gather(ops, src_i, idx, what):
    """src_i: int32 [samples, sample_floats] of random bits on the device; returns after checking dst against torch indexing bit for bit"""
    sf = src_i.shape[1]; n = len(idx)
    idx_d = torch.tensor(idx, dtype=torch.int64, device="cuda")
    dbuf, dst = guarded(n * sf, torch.int32, fill=7)
    ck(ops, ops.lib.unet_gather_samples(ops.h, src_i.data_ptr(), idx_d.data_ptr(), dst.data_ptr(), n, sf, ops.s), what)
    guards_kept(dbuf, what, fill=7)
    assert torch.equal(dst.view(n, sf), src_i[idx_d]), f"{what}: differs from src[idx]"


@pytest.mark.parametrize("sf", [4, 12, 4096])
def test_gather_samples_bit_exact(ops, sf):
    g = torch.Generator(device="cuda"); g.manual_seed(sf)
    ns = 37
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (ns, sf), dtype=torch.int32, device="cuda", generator=g)          # every bit pattern, NaNs included: a copy keeps them
    rng = np.random.default_rng(sf)
    gather(ops, src, list(range(ns))[::-1], f"gather sf={sf} reversed")
    gather(ops, src, rng.integers(0, ns, 50).tolist() + [3, 3, 3, 36, 0, 36], f"gather sf={sf} repeats")
    gather(ops, src, [36], f"gather sf={sf} one index")
    gather(ops, src[:1], [0], f"gather sf={sf} one sample in the source")
    if sf == 4096:                                                          # n sf / 4 = 532480 float4s > 2048 * 256: the stride loop runs
        idx = rng.integers(0, ns, 520).tolist()
        assert len(idx) * sf // 4 > T.MAX_BLOCKS * T.TPB
        gather(ops, src, idx, "gather stride loop")


def test_gather_samples_from_a_source_over_2_gib(ops):
    sf, ns = 4096, 131080                                                   # 131080 * 16 KiB = 2^31 + 128 KiB
    assert ns * sf * 4 > 2 ** 31
    src = torch.empty((ns, sf), dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    for r in (0, 1, ns - 2, ns - 1):
        src[r] = torch.randint(-2 ** 31, 2 ** 31 - 1, (sf,), dtype=torch.int32, device="cuda", generator=g)
    gather(ops, src, [ns - 1, 0, ns - 2, 1, ns - 1], "gather over 2 GiB")
    del src
    torch.cuda.empty_cache()


def test_gather_samples_rejects_sample_sizes_that_are_no_multiple_of_4(ops):
    src = torch.zeros(64, dtype=torch.int32, device="cuda"); idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    dbuf, dst = guarded(64, torch.int32, fill=7)
    for sf in (2, 6):
        rejected(ops, ops.lib.unet_gather_samples(ops.h, src.data_ptr(), idx.data_ptr(), dst.data_ptr(), 2, sf, ops.s), f"gather sample_floats = {sf}")
    assert (dbuf == 7).all()


# ---- zero -----------------------------------------------------------------------------------------------------------------------------------
ZERO_CASES = [(256, nb) for nb in (4, 8, 12, 16, 20, 28, 4096 + 12, T.MAX_BLOCKS * T.TPB * 16 * 2 + 8)] + [(260, 16), (260, 4096 + 12), (256, 6), (257, 7), (256, 0)]


@pytest.mark.parametrize("start,nbytes", ZERO_CASES)
def test_zero_exactly_the_requested_bytes(ops, start, nbytes):
    """(256, ...): a 16-byte aligned pointer, the vector path and its 1..3-word tail, two passes of the stride loop; (260, ...): the pointer 4 bytes off (fallback);
    6 / 7 bytes: no multiple of 4 (fallback); 0 bytes: nothing"""
    total = start + nbytes + 256
    buf = torch.from_numpy(T.zero_pattern(total)).cuda()
    assert buf.data_ptr() % 16 == 0
    ck(ops, ops.lib.unet_zero(ops.h, buf.data_ptr() + start, nbytes, ops.s), f"zero {start}+{nbytes}")
    T.check_zero(host(buf), start, nbytes, f"zero {start}+{nbytes}")


# ---- casts ----------------------------------------------------------------------------------------------------------------------------------
def cast_to_bf16(ops, f, what):
    n = f.size
    dbuf, dst = guarded(n, torch.int16, fill=7)
    ck(ops, ops.lib.unet_cast_f32_to_bf16(ops.h, ops.d(f).data_ptr(), dst.data_ptr(), n, ops.s), what)
    guards_kept(dbuf, what, fill=7)
    return host(dst).view(np.uint16)


def cast_to_f32(ops, b16, what):
    n = b16.size
    src = torch.from_numpy(b16.view(np.int16)).cuda()
    dbuf, dst = guarded(n, torch.int32, fill=7)
    ck(ops, ops.lib.unet_cast_bf16_to_f32(ops.h, src.data_ptr(), dst.data_ptr(), n, ops.s), what)
    guards_kept(dbuf, what, fill=7)
    return host(dst).view(np.uint32)


def test_casts_table_of_bit_patterns(ops):
    f = T.CAST_TABLE.view(f32)
    assert f.size % 4 == 0
    got = cast_to_bf16(ops, f, "cast table")
    T.check_cast_to_bf16(got, f, "cast f32 -> bf16 table")
    T.bits_equal(got, T.emu_cast(f), "cast f32 -> bf16 table: the quiet NaN stays 0x7FC0, round to nearest even on the bits")
    back = cast_to_f32(ops, got, "cast back")
    T.bits_equal(back, got.astype(np.uint32) << 16, "cast bf16 -> f32 table")
    T.bits_equal(back, T.f32_bits_torch(got).view(np.uint32), "cast bf16 -> f32 table against torch")


def test_casts_past_the_stride_on_random_bits(ops):
    n = 2 * STRIDE4 + 4
    rng = np.random.default_rng(11)
    f = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(f32)
    T.check_cast_to_bf16(cast_to_bf16(ops, f, "cast random"), f, "cast f32 -> bf16 random bits")
    b16 = rng.integers(0, 2 ** 16, n, dtype=np.uint32).astype(np.uint16)
    back = cast_to_f32(ops, b16, "cast back random")
    T.bits_equal(back, b16.astype(np.uint32) << 16, "cast bf16 -> f32 random bits")
    num = ~np.isnan(back.view(f32))
    T.bits_equal(back[num], T.f32_bits_torch(b16).view(np.uint32)[num], "cast bf16 -> f32 random bits against torch")

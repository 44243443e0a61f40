"""The matrix-core ops of the bf16-storage path (csrc/kernels_bf16.hip: conv3x3 / ConvT forward, data and weight gradients, their BatchNorm-statistics
epilogue; the first-layer conv; the bf16 dense tail of csrc/kernels_dense.hip) against float64 references PER ELEMENT, at the shapes where the kernels branch.
tests/test_gpu_bf16_ops.py holds the same ops to norm-wise figures only; a store that truncates, one wrong border column or a weight image that truncates
passes those.

Inputs: activations / gradients bf16-exact; weights are NOT bf16-exact (the kernels round them in wimg_kernel): the reference uses RNE_bf16(w), and a reference
built from truncated weights must fail the same check on a clear share of the elements (asserted per case).

Bounds (gpu_util: EPS_SPLIT = 4 * 2^-22, u = 2^-24).  A bf16 kernel multiplies bf16 values (exact in fp32) and accumulates in fp32 on the MFMA: the arithmetic
class of the strict fp32 MFMA family, which test_gpu_ops.py holds to EPS_SPLIT * A1 per element, A1 = sum |a| |b| of that output.  So the value v before the
store carries |v - ref64| <= EPS_SPLIT * (A1 + |bias|); each epilogue operation behind it adds k u of its result: ELU k = 4 (expm1f: 1 ulp = 2 u, and its
derivative is <= 1, so the accumulation allowance passes through unamplified), the keep scale k = 2 (the allowance scaled with it), the mask factors k = 3
(ELU: m + 1) and k = 4 (ELU + dropout: m (1 - rate) + 1, times the keep scale) of |v| (|factor| + the magnitude the factor's own evaluation rounds against).
  * bf16-stored outputs: gpu_util.check_store with that allowance as tol: RNE_bf16(ref - tol) <= got <= RNE_bf16(ref + tol), and a truncated copy of the
    reference must fail on > 20 % of the elements that need rounding (a condition on the data: test_data_conditions_hold_without_a_gpu evaluates it, and
    the weight-image condition, for every case on the CPU);
  * fp32 outputs (dw, db, dense y / dw): gpu_util.elem_ratio(got, ref, A1) <= 1;
  * statistics epilogue: the sums of the STORED bf16 values: reference = float64 sums of the kernel's own output, bound (n + T + k) u sum |terms| with
    n = RW rows x 2 pixels x the tiles a slot copy receives, T = 16 lanes + 4 waves folded in fp32, k = 2 (sum) / 3 (sum of squares).
Every check prints its largest error / bound ratio ("bound-ratio ...", run with -s); for a bf16 output it is the largest |ref64 - midpoint| / tol among the
elements that needed the midpoint allowance.  Measured on an MI355X: bf16 outputs <= 0.017 (conv3x3 forward 0.017, data gradient 0.017, ConvT forward 0.017,
ConvT data gradient 0.008, first layer 0: no element used the allowance), the allowance used by ~1e-4 of the elements (54 of 721 k forward outputs); dense dx
0.059.  fp32 outputs: conv3x3 dw 0.007-0.047, db <= 0.014; ConvT dw 0.039-0.085, db <= 0.005; first-layer dw 0.02-0.09; dense y 0.006-0.059, dense dw 0.04-0.33
(one fmaf per batch row: the fewest terms).  Statistics: epilogue sums 8e-4 - 0.025, sums of squares 0.03-0.05, epilogue against the plain pass 0.004-0.035
(conv3x3 and ConvT alike; the (n + T) u sum |terms| bound is a worst case).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import philox_ref as PX
from gpu_util import EPS_SPLIT, U, check_store, check_sum, convT_abs_sums, elem_ratio, rne_bf16, trunc_bf16

gpu = pytest.mark.gpu
SENT = 7.0                                    # sentinel around an output (bf16-exact): must survive every launch
BAD_IN = 30720.0                              # poison beside an input slice: a kernel that reads it leaves every bound far behind
GUARD = 2048                                  # sentinel elements in front of and behind an output tensor
E_SHAPE = -3


@pytest.fixture(scope="module")
def ops():
    from gpu_util import Ops
    return Ops()


# ---- values, buffers ------------------------------------------------------------------------------------------------------------------------
def bfx(a):
    """rounded to bf16 (nearest even) once, as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def T64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def nchw(a):
    return T64(a).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


_KEEP = []                                    # device inputs made inline for a call: alive until the launch has finished (the C ABI sees raw pointers only)


def dev16(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().cuda()
    _KEEP.append(t)
    return t


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def guarded(shape):
    """a bf16 device tensor of `shape` inside a flat buffer with GUARD sentinel elements on both sides; the tensor itself is filled with the sentinel too"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENT, dtype=torch.bfloat16, device="cuda")
    return buf, buf[GUARD:GUARD + numel].view(*shape)


def guards_kept(buf, what):
    b = host(buf)
    bad = np.count_nonzero(b[:GUARD] != SENT) + np.count_nonzero(b[-GUARD:] != SENT)
    assert bad == 0, f"{what}: {bad} sentinel elements in front of / behind the output were overwritten"


def ck(ops, rc, what, handle=None):
    if rc != 0:
        msg = ops.lib.unet_last_error(handle if handle is not None else ops.h)
        raise AssertionError(f"{what}: status {rc}: {msg.decode() if msg else '?'}")
    torch.cuda.synchronize()
    _KEEP.clear()


def rejected(ops, rc, what):
    torch.cuda.synchronize()
    msg = ops.lib.unet_last_error(ops.h)
    assert rc == E_SHAPE and msg, f"{what}: expected UNET_E_SHAPE with a message, got {rc} {msg!r}"


def pattern(a, kind):
    """dense: as is; border: only the border pixels of every image non-zero; pixel: one interior pixel of the last image non-zero"""
    n, h, w, _ = a.shape
    if kind == "border":
        m = np.zeros((h, w), bool); m[0] = m[-1] = True; m[:, 0] = m[:, -1] = True
        return a * m[None, :, :, None]
    if kind == "pixel":
        out = np.zeros_like(a); out[n - 1, h // 2, w // 3] = a[n - 1, h // 2, w // 3]
        return out
    return a


def weights_truncation_caught(ref, tol, ref_trunc, what):
    """the weight-image condition: the reference a TRUNCATING weight image would produce must fail the check on a clear share of the elements"""
    lo, hi = rne_bf16(ref - tol), rne_bf16(ref + tol)
    g = rne_bf16(ref_trunc)
    live = ref != 0
    share = float(((g < lo) | (g > hi))[live].mean())
    assert share > 0.2, f"{what}: the check is too weak here: truncated weights would fail on only {share:.1%} of the elements"


# ---- conv3x3 forward ------------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout), act, dropout rate, input pattern.  Tile forms of bf16_conv_tile: cout <= 32 (NB 1, RW 2: 8-row tiles), cout % 64 == 0 (NB 2, RW 4: 16 rows),
# the rest (48, 80, 96: NB 1, RW 4); cout = 16 / cout % 32 == 16: zero-padded rows of the weight image.  Widths around 32, heights around the tile height, h / w
# of 1-3, n >= 2 (the XCD block map crosses images), tile counts that are not a multiple of 8 (the wi >= total_blocks exit).
FWD_CASES = [
    ((2, 7, 31, 16, 32), 0, 0.0, "dense"), ((2, 8, 32, 32, 32), 1, 0.0, "dense"), ((2, 9, 33, 32, 16), 0, 0.0, "dense"),
    ((2, 15, 33, 32, 64), 0, 0.0, "dense"), ((1, 16, 32, 16, 64), 1, 0.0, "dense"), ((3, 17, 31, 64, 128), 0, 0.0, "dense"),
    ((2, 17, 33, 32, 48), 0, 0.0, "dense"), ((1, 16, 65, 16, 80), 1, 0.0, "dense"), ((2, 5, 40, 48, 96), 0, 0.0, "dense"),
    ((2, 1, 3, 32, 32), 0, 0.0, "dense"), ((2, 3, 1, 64, 64), 1, 0.0, "dense"), ((3, 2, 2, 16, 16), 0, 0.0, "dense"),
    ((1, 9, 20, 512, 32), 0, 0.0, "dense"),
    ((2, 12, 37, 32, 64), 0, 0.0, "border"), ((2, 12, 37, 32, 32), 0, 0.0, "pixel"),
    ((2, 10, 33, 32, 64), 2, 0.0, "dense"), ((2, 10, 33, 32, 32), 2, 0.4, "dense"), ((1, 9, 31, 64, 48), 2, 0.25, "dense"), ((2, 6, 34, 16, 96), 2, 0.0, "dense"),
]


def conv_fwd_ref(x, kq, b, act, rate, seed):
    """float64 reference and allowance of the forward epilogue (module docstring); kq: the weights as the kernel sees them"""
    v = nhwc(F.conv2d(nchw(x), T64(kq).permute(3, 2, 0, 1), T64(b), padding=1))
    a1 = nhwc(F.conv2d(nchw(np.abs(x)), T64(np.abs(kq)).permute(3, 2, 0, 1), padding=1)) + np.abs(b).astype(np.float64)
    tol = EPS_SPLIT * a1
    ref = v
    if act == 1:
        ref = np.maximum(v, 0.0)
    elif act == 2:
        ref = np.where(v > 0, v, np.expm1(np.minimum(v, 0.0))); tol = tol + 4 * U * np.abs(ref)
    if rate > 0:
        ks = PX.keep_scale_dense(ref.shape, rate, seed).astype(np.float64)
        ref = ref * ks; tol = tol * ks + 2 * U * np.abs(ref)
    return ref, tol


def conv_fwd_case(case):
    shape, act, rate, pat = case
    n, h, w, ci, co = shape
    rng = np.random.default_rng(ci * 1000 + co + h + w)
    x = pattern(bfx(rng.standard_normal((n, h, w, ci))), pat)
    k = (rng.standard_normal((3, 3, ci, co)) * 0.2).astype(np.float32)          # not bf16-exact
    b = (rng.standard_normal(co) * (0.0 if pat != "dense" else 1.0)).astype(np.float32)
    seed = 1234 + co
    ref, tol = conv_fwd_ref(x, bfx(k), b, act, rate, seed)
    ref_t, _ = conv_fwd_ref(x, trunc_bf16(k), b, act, rate, seed)
    return x, k, b, seed, ref, tol, ref_t


@gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(map(str, c[0])) + f"-act{c[1]}-{c[3]}" + ("-drop" if c[2] else ""))
def test_conv3x3_fwd_bf16_per_element(ops, case):
    shape, act, rate, pat = case
    n, h, w, ci, co = shape
    x, k, b, seed, ref, tol, ref_t = conv_fwd_case(case)
    buf, y = guarded((n, h, w, co))
    ck(ops, ops.lib.unet_conv3x3_fwd_bf16(ops.h, dev16(x).data_ptr(), ops.d(k).data_ptr(), ops.d(b).data_ptr(), y.data_ptr(), n, h, w, ci, co, act, rate, seed if rate else 0,
                                          ops.wws(ci, co), ops.s), "conv fwd bf16")
    guards_kept(buf, "conv fwd bf16")
    got = host(y)
    check_store(got, ref, None, None, "bf16", f"conv3x3 fwd {shape} act={act} rate={rate} {pat}", tol=tol)
    weights_truncation_caught(ref, tol, ref_t, "conv3x3 fwd")
    if rate:
        ks = PX.keep_scale_dense(ref.shape, rate, seed)
        assert np.array_equal(got[ref != 0] == 0, (ks == 0)[ref != 0]), "keep pattern differs from philox_ref"


# ---- conv3x3 data gradient ------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout) of the LAYER (the kernel contracts over cout and writes cin channels), mask mode, pattern of dy
DGRAD_CASES = [
    ((2, 9, 33, 32, 32), 0, "dense"), ((2, 15, 31, 64, 32), 1, "dense"), ((1, 17, 32, 16, 64), 1, "dense"), ((2, 7, 37, 48, 32), 0, "dense"),
    ((3, 16, 33, 128, 64), 0, "dense"), ((2, 1, 3, 32, 64), 1, "dense"), ((2, 12, 37, 32, 64), 0, "pixel"), ((2, 12, 37, 64, 32), 0, "border"),
    ((2, 10, 33, 32, 64), 2, "dense"), ((2, 10, 33, 64, 32), 3, "dense"), ((1, 9, 31, 48, 64), 3, "dense"), ((1, 6, 20, 80, 16), 2, "dense"),
]
DENORM = float(np.float32(2.0 ** -130))       # a bf16 denormal


def mask_source(rng, shape, mode, rate, seed):
    if mode == 0:
        return None
    if mode == 1:
        m = bfx(rng.standard_normal(shape))
        flat = m.reshape(-1)                                  # "bf16 > 0 <=> sign clear and magnitude non-zero": -0.0, +0.0 and a negative denormal close, a positive one opens
        flat[0], flat[1], flat[2], flat[3] = -0.0, DENORM, -DENORM, 0.0
        return m
    e = rng.standard_normal(shape)
    e = np.where(e > 0, e, np.expm1(e))
    if mode == 3:
        e = e * PX.keep_scale_dense(shape, rate, seed)
    return bfx(e)


def conv_dgrad_ref(dy, kq, m, mode, rate, seed):
    wt = T64(kq).permute(3, 2, 0, 1)                          # [co, ci, 3, 3]: conv_transpose2d's (in, out, kh, kw)
    v = nhwc(F.conv_transpose2d(nchw(dy), wt, padding=1))
    tol = EPS_SPLIT * nhwc(F.conv_transpose2d(nchw(np.abs(dy)), wt.abs(), padding=1))
    if mode == 0:
        return v, tol
    m64 = m.astype(np.float64)
    if mode == 1:
        mf = (m64 > 0).astype(np.float64)
        return v * mf, tol * mf
    if mode == 2:
        mf = np.where(m64 > 0, 1.0, m64 + 1.0); mA = np.where(m64 > 0, 0.0, np.abs(m64) + 1.0); kk = 3
    else:
        ks = PX.keep_scale_dense(m.shape, rate, seed).astype(np.float64)
        a = m64 * float(np.float32(1.0) - np.float32(rate))
        mf = ks * np.where(a > 0, 1.0, a + 1.0); mA = ks * (2 * np.abs(a) + 1.0); kk = 4
    return v * mf, tol * np.abs(mf) + kk * U * np.abs(v) * (np.abs(mf) + mA)


def conv_dgrad_case(case):
    shape, mode, pat = case
    n, h, w, ci, co = shape
    rng = np.random.default_rng(7 + ci * 1000 + co + h + w + mode)
    dy = pattern(bfx(rng.standard_normal((n, h, w, co))), pat)
    k = (rng.standard_normal((3, 3, ci, co)) * 0.2).astype(np.float32)
    rate, seed = (0.3, 4242 + ci) if mode == 3 else (0.0, 0)
    m = mask_source(rng, (n, h, w, ci), mode, rate, seed)
    ref, tol = conv_dgrad_ref(dy, bfx(k), m, mode, rate, seed)
    ref_t, _ = conv_dgrad_ref(dy, trunc_bf16(k), m, mode, rate, seed)
    return dy, k, m, rate, seed, ref, tol, ref_t


@gpu
@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "-".join(map(str, c[0])) + f"-mask{c[1]}-{c[2]}")
def test_conv3x3_bwd_data_bf16_per_element(ops, case):
    shape, mode, pat = case
    n, h, w, ci, co = shape
    dy, k, m, rate, seed, ref, tol, ref_t = conv_dgrad_case(case)
    md = dev16(m) if m is not None else None
    if mode == 1:
        assert host(md).reshape(-1)[1] == DENORM and np.signbit(host(md).reshape(-1)[0])          # the device tensor holds the denormal and the -0.0
    buf, dx = guarded((n, h, w, ci))
    ck(ops, ops.lib.unet_conv3x3_bwd_data_bf16(ops.h, dev16(dy).data_ptr(), ops.d(k).data_ptr(), md.data_ptr() if md is not None else None, mode, rate, seed, dx.data_ptr(),
                                               ops.wws(ci, co), n, h, w, ci, co, ops.s), "conv bwd data bf16")
    guards_kept(buf, "conv bwd data bf16")
    check_store(host(dx), ref, None, None, "bf16", f"conv3x3 dgrad {shape} mask={mode} {pat}", tol=tol)
    weights_truncation_caught(ref, tol, ref_t, "conv3x3 dgrad")


# ---- first-layer conv (cin = 1, fp32 image in) ----------------------------------------------------------------------------------------------
C1_SHAPES = [(2, 9, 37, 32), (1, 5, 7, 64), (2, 6, 12, 16), (3, 1, 3, 32)]          # (w % 4 == 0: four pixels per thread)


def c1_case(shape):
    n, h, w, co = shape
    rng = np.random.default_rng(3 + co + w)
    x = rng.standard_normal((n, h, w, 1)).astype(np.float32); k = (rng.standard_normal((3, 3, 1, co)) * 0.3).astype(np.float32)          # fp32 in: nothing is rounded
    b = rng.standard_normal(co).astype(np.float32); dy = bfx(rng.standard_normal((n, h, w, co)))
    ref, tol = conv_fwd_ref(x, k, b, 1, 0.0, 0)
    return x, k, b, dy, ref, tol


def conv_wgrad64(x, dy):
    """dw[a, b, c, o] = sum_p x[p + (a, b) - 1] dy[p], db, and their A1 = the same sums of magnitudes (float64)"""
    x64, d64 = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n, h, w, ci = x64.shape
    xp = np.pad(x64, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dw = np.zeros((3, 3, ci, d64.shape[-1])); a1 = np.zeros_like(dw)
    df, da = d64.reshape(-1, d64.shape[-1]), np.abs(d64).reshape(-1, d64.shape[-1])
    for a in range(3):
        for b in range(3):
            win = xp[:, a:a + h, b:b + w].reshape(-1, ci)
            dw[a, b] = win.T @ df; a1[a, b] = np.abs(win).T @ da
    return dw, a1, df.sum(0), da.sum(0)


@gpu
@pytest.mark.parametrize("shape", C1_SHAPES)
def test_conv3x3_first_layer_bf16_per_element(ops, shape):
    n, h, w, co = shape
    x, k, b, dy, ref, tol = c1_case(shape)
    buf, y = guarded((n, h, w, co))
    ck(ops, ops.lib.unet_conv3x3_first_fwd_bf16(ops.h, ops.d(x).data_ptr(), ops.d(k).data_ptr(), ops.d(b).data_ptr(), y.data_ptr(), n, h, w, co, 1, 0.0, 0, ops.s), "c1 fwd bf16")
    guards_kept(buf, "c1 fwd bf16")
    check_store(host(y), ref, None, None, "bf16", f"first-layer fwd {shape}", tol=tol)
    nb = ops.lib.unet_conv3x3_bwd_weights_ws_bytes_bf16(n, h, w, 1, co)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    dw = ops.z(3, 3, 1, co); db = ops.z(co); dw.fill_(123.0); db.fill_(-7.0)
    ck(ops, ops.lib.unet_conv3x3_first_bwd_weights_bf16(ops.h, ops.d(x).data_ptr(), dev16(dy).data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, n, h, w, co, ops.s), "c1 wgrad")
    rdw, adw, rdb, adb = conv_wgrad64(x, dy)
    r1, r2 = elem_ratio(dw.cpu().numpy(), rdw, adw), elem_ratio(db.cpu().numpy(), rdb, adb)
    print(f"bound-ratio first-layer wgrad {shape} dw {r1:.3g} db {r2:.3g}")
    assert r1 <= 1.0 and r2 <= 1.0, (shape, r1, r2)


@gpu
def test_first_layer_rejects_a_channel_count_its_kernel_cannot_take(ops):
    n, h, w, co = 1, 5, 7, 48                                  # 256 % (48 / 4) != 0
    y = ops.z(n, h, w, co, dtype=torch.bfloat16)
    rejected(ops, ops.lib.unet_conv3x3_first_fwd_bf16(ops.h, ops.z(n, h, w, 1).data_ptr(), ops.z(3, 3, 1, co).data_ptr(), None, y.data_ptr(), n, h, w, co, 1, 0.0, 0, ops.s), "c1 fwd cout=48")


# ---- ConvT ----------------------------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, cout), channel offset of the written / read slice in a concat buffer of 2 * cout channels.  cin % 64 == 0 and == 32: the NB choice of the data gradient
CONVT_CASES = [((2, 5, 33, 64, 32), 32), ((1, 1, 31, 96, 32), 0), ((2, 7, 9, 32, 64), 64), ((1, 4, 32, 128, 64), 0)]


def convT_case(case):
    shape, off = case
    n, h, w, ci, co = shape
    rng = np.random.default_rng(11 + ci + co + w)
    x = bfx(rng.standard_normal((n, h, w, ci))); k = (rng.standard_normal((2, 2, co, ci)) * 0.2).astype(np.float32)
    b = rng.standard_normal(co).astype(np.float32); dy = bfx(rng.standard_normal((n, 2 * h, 2 * w, co)))
    return x, k, b, dy


def convT_refs(x, kq, b, dy):
    x64, k64, d64 = x.astype(np.float64), np.asarray(kq, np.float64), dy.astype(np.float64)
    n, h, w, ci = x.shape
    co = k64.shape[2]
    y = np.zeros((n, 2 * h, 2 * w, co)); dx = np.zeros((4, n, h, w, ci)); dw = np.zeros((2, 2, co, ci))
    for a in range(2):
        for c in range(2):
            y[:, a::2, c::2] = x64 @ k64[a, c].T + b.astype(np.float64)
            dx[2 * a + c] = d64[:, a::2, c::2] @ k64[a, c]
            dw[a, c] = d64[:, a::2, c::2].reshape(-1, co).T @ x64.reshape(-1, ci)
    return y, dx, dw, d64.reshape(-1, co).sum(0)


@gpu
@pytest.mark.parametrize("case", CONVT_CASES, ids=lambda c: "-".join(map(str, c[0])) + f"-off{c[1]}")
def test_convT_bf16_per_element(ops, case):
    shape, off = case
    n, h, w, ci, co = shape
    ld = 2 * co
    x, k, b, dy = convT_case(case)
    kq = bfx(k)
    y64, dx4, dw64, db64 = convT_refs(x, kq, b, dy)
    yt, dxt, _, _ = convT_refs(x, trunc_bf16(k), b, dy)
    A = convT_abs_sums(x, kq, dy)
    xd, kd = dev16(x), ops.d(k)
    # forward into a channel slice of the concat buffer, sentinels in the other half and around the buffer
    buf, cat = guarded((n, 2 * h, 2 * w, ld))
    ck(ops, ops.lib.unet_convT2x2_fwd_bf16(ops.h, xd.data_ptr(), kd.data_ptr(), ops.d(b).data_ptr(), cat.data_ptr() + 2 * off, ld, n, h, w, ci, co, ops.wws(ci, co), ops.s), "convT fwd bf16")
    guards_kept(buf, "convT fwd bf16")
    got = host(cat)
    other = np.concatenate([got[..., :off].ravel(), got[..., off + co:].ravel()])
    assert (other == SENT).all(), "convT fwd: the other half of the concat buffer was written"
    tol = EPS_SPLIT * (A["y_a1"] + np.abs(b).astype(np.float64))
    for a in range(2):
        for c in range(2):
            check_store(got[:, a::2, c::2, off:off + co], y64[:, a::2, c::2], None, None, "bf16", f"convT fwd {shape} parity ({a},{c})", tol=tol[:, a::2, c::2])
    weights_truncation_caught(y64, tol, yt, "convT fwd")
    # data gradient: dU in its slice, poison in the other half; every parity plane on its own (a swapped parity is named), all four, and ReLU-masked
    dcat = np.full((n, 2 * h, 2 * w, ld), BAD_IN, np.float32); dcat[..., off:off + co] = dy
    da = np.abs(dy.astype(np.float64)); ka = np.abs(kq.astype(np.float64))
    for a in range(2):
        for c in range(2):
            one = np.full_like(dcat, BAD_IN); one[..., off:off + co] = 0.0; one[:, a::2, c::2, off:off + co] = dy[:, a::2, c::2]
            buf, dx = guarded((n, h, w, ci))
            ck(ops, ops.lib.unet_convT2x2_bwd_data_bf16(ops.h, dev16(one).data_ptr() + 2 * off, ld, kd.data_ptr(), None, dx.data_ptr(), n, h, w, ci, co, ops.wws(ci, co), ops.s), "convT dgrad")
            guards_kept(buf, "convT dgrad")
            check_store(host(dx), dx4[2 * a + c], None, None, "bf16", f"convT dgrad {shape} parity ({a},{c})", tol=EPS_SPLIT * (da[:, a::2, c::2] @ ka[a, c]))
    dcd = dev16(dcat)
    ref = dx4.sum(0); tol = EPS_SPLIT * A["dx_a1"]
    for masked in (False, True):
        buf, dx = guarded((n, h, w, ci))
        ck(ops, ops.lib.unet_convT2x2_bwd_data_bf16(ops.h, dcd.data_ptr() + 2 * off, ld, kd.data_ptr(), xd.data_ptr() if masked else None, dx.data_ptr(), n, h, w, ci, co, ops.wws(ci, co), ops.s),
           "convT dgrad")
        guards_kept(buf, "convT dgrad")
        mf = (x > 0).astype(np.float64) if masked else 1.0
        check_store(host(dx), ref * mf, None, None, "bf16", f"convT dgrad {shape} masked={masked}", tol=tol * mf)
    weights_truncation_caught(ref, tol, dxt.sum(0), "convT dgrad")
    # weight gradient with lddy > cout, outputs pre-filled with garbage, twice: bit-identical
    nb = ops.lib.unet_convT2x2_bwd_weights_ws_bytes_bf16(n, h, w, ci, co)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        dw = ops.z(2, 2, co, ci); db = ops.z(co); dw.fill_(3.0); db.fill_(-2.0)
        ck(ops, ops.lib.unet_convT2x2_bwd_weights_bf16(ops.h, xd.data_ptr(), dcd.data_ptr() + 2 * off, ld, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, n, h, w, ci, co, ops.s), "convT wgrad")
        runs.append((dw.cpu().numpy(), db.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "convT wgrad: two runs differ"
    r1, r2 = elem_ratio(runs[0][0], dw64, A["dw_a1"]), elem_ratio(runs[0][1], db64, A["db_a1"])
    print(f"bound-ratio convT wgrad {shape} dw {r1:.3g} db {r2:.3g}")
    assert r1 <= 1.0 and r2 <= 1.0, (shape, r1, r2)


@gpu
def test_convT_bf16_rejects_channel_counts_that_are_not_multiples_of_32(ops):
    n, h, w, ci, co = 1, 4, 4, 48, 32
    cat = ops.z(n, 2 * h, 2 * w, co, dtype=torch.bfloat16)
    rejected(ops, ops.lib.unet_convT2x2_fwd_bf16(ops.h, ops.z(n, h, w, ci, dtype=torch.bfloat16).data_ptr(), ops.z(2, 2, co, ci).data_ptr(), None, cat.data_ptr(), co, n, h, w, ci, co,
                                                 ops.wws(64, 32), ops.s), "convT fwd cin=48")


# ---- weight gradients -----------------------------------------------------------------------------------------------------------------------
# wave layouts of run_wgrad_bf16 (plan_wgrad_bf16: WA = 2 where cin % 64 == 0, WB = 2 where cout % 64 == 0): (2,2,1) 64->64, (2,1,2) 64->32, (1,2,2) 32->64, (1,1,4) 32->32;
# 16->16 with an even width (the pixel-pair path) and an odd one (plain); multiples of 8 that are not multiples of 16; heights that do not divide into
# rows_per_chunk (70 rows: 12-row chunks), several 32-column strips, n >= 3
WGRAD_SHAPES = [(3, 13, 37, 64, 64), (1, 9, 70, 64, 32), (2, 11, 33, 32, 64), (3, 7, 31, 32, 32), (3, 70, 40, 32, 32), (2, 28, 28, 16, 16), (2, 9, 27, 16, 16),
                (1, 10, 34, 24, 40), (2, 6, 20, 40, 24), (1, 37, 5, 48, 96)]


@gpu
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_conv3x3_bwd_weights_bf16_per_element(ops, shape):
    n, h, w, ci, co = shape
    rng = np.random.default_rng(ci * 100 + co + h)
    x = bfx(rng.standard_normal((n, h, w, ci))); dy = bfx(rng.standard_normal((n, h, w, co)))
    rdw, adw, rdb, adb = conv_wgrad64(x, dy)
    nb = ops.lib.unet_conv3x3_bwd_weights_ws_bytes_bf16(n, h, w, ci, co)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    xd, dyd = dev16(x), dev16(dy)
    runs = []
    for fill in (123.0, -9.0):                                  # overwritten, not accumulated; two runs bit-identical (fixed-order reduction)
        dw = ops.z(3, 3, ci, co); db = ops.z(co); dw.fill_(fill); db.fill_(-fill)
        ck(ops, ops.lib.unet_conv3x3_bwd_weights_bf16(ops.h, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, n, h, w, ci, co, ops.s), "conv wgrad bf16")
        runs.append((dw.cpu().numpy(), db.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "conv wgrad: two runs differ"
    r1, r2 = elem_ratio(runs[0][0], rdw, adw), elem_ratio(runs[0][1], rdb, adb)
    print(f"bound-ratio conv3x3 wgrad {shape} dw {r1:.3g} db {r2:.3g}")
    assert r1 <= 1.0 and r2 <= 1.0, (shape, r1, r2)


# ---- statistics epilogue --------------------------------------------------------------------------------------------------------------------
BN_SLOTS, TPB, BN_STATS_BLOCKS = 64, 256, 512          # common.h UNET_BN_SLOTS; kernels_pointwise.hip launch geometry


def cdiv(a, b):
    return -(-int(a) // int(b))


def pass_terms(pixels, c):
    """terms per thread + partials per workgroup of the statistics pass (bn_stats_kernel)"""
    ppb = TPB // (c // 4)
    return cdiv(pixels, max(1, min(cdiv(pixels, ppb * 16), BN_STATS_BLOCKS)) * ppb) + ppb


def stored_sums(y, c):
    y64 = y.reshape(-1, c)
    return y64.sum(0), (y64 * y64).sum(0), np.abs(y64).sum(0)


def epilogue_terms(n, h, w, m, nb, rw):
    """RW rows x 2 pixels x the tiles a slot copy receives, + the 16 lanes and 4 waves folded in fp32"""
    total = cdiv(w, 32) * cdiv(h, 4 * rw) * n * cdiv(m, 32 * nb)
    return 2 * rw * cdiv(8 * cdiv(total, 8), BN_SLOTS) + 20


def conv_tile(co):
    return (1, 2) if co <= 32 else ((2, 4) if co % 64 == 0 else (1, 4))


def stats_after(ops, handle, launch, y, ld, c, pixels, nt, what, folded):
    """arm, launch, then unet_bn_stats_bf16 on the written tensor.  folded: the epilogue took the sums -- the call must not read the tensor (it is overwritten in
    between) and must agree with the float64 sums of what was stored and with a plain pass; not folded: the call does its own pass over what it finds"""
    sums = ops.z(2 * c, dtype=torch.float64); plain = ops.z(2 * c, dtype=torch.float64)
    ck(ops, ops.lib.unet_request_bn_stats(handle, c), "arm", handle)
    launch()
    torch.cuda.synchronize()
    stored = host(y)[..., :c]
    keep = y.clone()
    y.fill_(2.0)                                                # the sentinel between the two calls
    ck(ops, ops.lib.unet_bn_stats_bf16(handle, y.data_ptr(), ld, sums.data_ptr(), pixels, c, ops.s), "stats after the armed launch", handle)
    got = sums.cpu().numpy()
    s1, s2, sa = stored_sums(stored, c)
    if folded:
        check_sum(got[:c], s1, (nt + 2) * U * sa, what + " epilogue sum", "bf16")
        check_sum(got[c:], s2, (nt + 3) * U * s2, what + " epilogue sum^2", "bf16")
    else:
        assert np.array_equal(got, np.concatenate([np.full(c, 2.0 * pixels), np.full(c, 4.0 * pixels)])), what + ": the launcher had to decline, the statistics call must read the tensor"
    y.copy_(keep)
    ck(ops, ops.lib.unet_bn_stats_bf16(handle, y.data_ptr(), ld, plain.data_ptr(), pixels, c, ops.s), "plain pass", handle)
    p = plain.cpu().numpy()
    np_ = pass_terms(pixels, c)
    check_sum(p[:c], s1, (np_ + 2) * U * sa, what + " pass sum", "bf16")
    check_sum(p[c:], s2, (np_ + 3) * U * s2, what + " pass sum^2", "bf16")
    if folded:
        check_sum(got[:c], p[:c], (nt + np_ + 4) * U * sa, what + " epilogue vs pass sum", "bf16")
        check_sum(got[c:], p[c:], (nt + np_ + 6) * U * s2, what + " epilogue vs pass sum^2", "bf16")


@gpu
@pytest.mark.parametrize("shape,folded", [((2, 20, 36, 32, 32), True), ((2, 17, 33, 64, 64), True), ((1, 9, 40, 32, 96), True), ((3, 16, 64, 16, 128), True),
                                          ((2, 12, 20, 32, 48), False), ((2, 12, 20, 32, 16), False)])          # (M % 32 == 16: declined)
def test_conv3x3_bf16_statistics_epilogue(ops, shape, folded):
    n, h, w, ci, co = shape
    rng = np.random.default_rng(ci + co + h)
    xd = dev16(rng.standard_normal((n, h, w, ci))); kd = ops.d((rng.standard_normal((3, 3, ci, co)) * (2.0 / (9 * ci)) ** 0.5).astype(np.float32))
    bd = ops.d((rng.standard_normal(co) * 0.3).astype(np.float32))
    y = ops.z(n, h, w, co, dtype=torch.bfloat16)
    nb, rw = conv_tile(co)
    stats_after(ops, ops.h, lambda: ck(ops, ops.lib.unet_conv3x3_fwd_bf16(ops.h, xd.data_ptr(), kd.data_ptr(), bd.data_ptr(), y.data_ptr(), n, h, w, ci, co, 1, 0.0, 0, ops.wws(ci, co), ops.s), "conv"),
                y, co, co, n * h * w, epilogue_terms(n, h, w, co, nb, rw), f"conv3x3 stats {shape}", folded)


@gpu
def test_conv3x3_bf16_statistics_declined_in_deterministic_mode_and_by_a_masked_launch(ops):
    from covidseg_amd import _lib
    n, h, w, ci, co = 2, 20, 36, 32, 32
    rng = np.random.default_rng(5)
    xd = dev16(rng.standard_normal((n, h, w, ci))); kd = ops.d((rng.standard_normal((3, 3, ci, co)) * 0.1).astype(np.float32))
    y = ops.z(n, h, w, co, dtype=torch.bfloat16)
    ctx = _lib.Context.get(0, {"deterministic": 1}, private=True)
    try:
        hd = ctx.handle
        stats_after(ops, hd, lambda: ck(ops, ops.lib.unet_conv3x3_fwd_bf16(hd, xd.data_ptr(), kd.data_ptr(), None, y.data_ptr(), n, h, w, ci, co, 1, 0.0, 0, ops.wws(ci, co), ops.s), "conv", hd),
                    y, co, co, n * h * w, 0, "conv3x3 stats deterministic", False)
    finally:
        ctx.close()
    dyd = dev16(rng.standard_normal((n, h, w, co))); dx = ops.z(n, h, w, ci, dtype=torch.bfloat16)
    stats_after(ops, ops.h, lambda: ck(ops, ops.lib.unet_conv3x3_bwd_data_bf16(ops.h, dyd.data_ptr(), kd.data_ptr(), xd.data_ptr(), 1, 0.0, 0, dx.data_ptr(), ops.wws(ci, co), n, h, w, ci, co, ops.s),
                                       "masked dgrad"), dx, ci, ci, n * h * w, 0, "conv3x3 stats masked launch", False)


@gpu
@pytest.mark.parametrize("shape", [(2, 6, 20, 64, 32), (1, 5, 33, 32, 64)])
def test_convT_bf16_statistics_epilogue_folds_the_four_planes(ops, shape):
    n, h, w, ci, co = shape
    rng = np.random.default_rng(ci + co)
    xd = dev16(rng.standard_normal((n, h, w, ci))); kd = ops.d((rng.standard_normal((2, 2, co, ci)) * (1.0 / ci) ** 0.5).astype(np.float32))
    bd = ops.d((rng.standard_normal(co) * 0.3).astype(np.float32))
    ld = 2 * co
    cat = ops.z(n, 2 * h, 2 * w, ld, dtype=torch.bfloat16)
    stats_after(ops, ops.h, lambda: ck(ops, ops.lib.unet_convT2x2_fwd_bf16(ops.h, xd.data_ptr(), kd.data_ptr(), bd.data_ptr(), cat.data_ptr(), ld, n, h, w, ci, co, ops.wws(ci, co), ops.s), "convT"),
                cat, ld, co, n * 4 * h * w, epilogue_terms(n, h, w, 4 * co, 2, 4), f"convT stats {shape}", True)


# ---- dense tail -----------------------------------------------------------------------------------------------------------------------------
DENSE_SHAPES = [(6, 3136, 32), (5, 64, 32), (32, 50176, 32), (3, 1000, 8), (130, 516, 16), (1, 4, 4)]          # test_gpu_classifier.py::test_dense_fwd_bwd's, all accepted


def dense_case(shape):
    b, k, n = shape
    rng = np.random.default_rng(b + k)
    x = bfx(rng.standard_normal((b, k))); w = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)          # fp32 weights: used as they are
    bias = rng.standard_normal(n).astype(np.float32); dy = rng.standard_normal((b, n)).astype(np.float32)
    ref = dy.astype(np.float64) @ w.astype(np.float64).T
    return x, w, bias, dy, ref, EPS_SPLIT * (np.abs(dy).astype(np.float64) @ np.abs(w).astype(np.float64).T)


@gpu
@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_bf16_per_element(ops, shape):
    b, k, n = shape
    x, w, bias, dy, rdx, tdx = dense_case(shape)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    nb = ops.lib.unet_dense_ws_bytes(b, k, n); ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    xd, wd, bd = dev16(x), ops.d(w), ops.d(bias)
    z = x64 @ w64 + bias
    a1 = np.abs(x64) @ np.abs(w64) + np.abs(bias)
    for act, rate, seed in ((1, 0.0, 0), (0, 0.0, 0), (1, 0.4, 99)):
        y = ops.z(b, n)
        ck(ops, ops.lib.unet_dense_fwd_bf16(ops.h, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), b, k, n, act, rate, seed, ws.data_ptr(), nb, ops.s), "dense fwd bf16")
        ks = PX.keep_scale_dense((b, n), rate, seed).astype(np.float64) if rate else np.ones((b, n))
        ref = (np.maximum(z, 0.0) if act else z) * ks
        got = y.cpu().numpy()
        r = elem_ratio(got, ref, a1 * ks)
        print(f"bound-ratio dense fwd {shape} act={act} rate={rate} {r:.3g}")
        assert r <= 1.0, (shape, act, rate, r)
        if rate:
            assert np.array_equal(got[ref != 0] == 0, (ks == 0)[ref != 0]), "dense fwd: keep pattern differs from philox_ref"
    dx = torch.full((b, k), SENT, dtype=torch.bfloat16, device="cuda"); dw = ops.z(k, n); dw.fill_(5.0)
    ck(ops, ops.lib.unet_dense_bwd_bf16(ops.h, xd.data_ptr(), wd.data_ptr(), ops.d(dy).data_ptr(), dx.data_ptr(), dw.data_ptr(), b, k, n, ops.s), "dense bwd bf16")
    check_store(host(dx), rdx, None, None, "bf16", f"dense dx {shape}", tol=tdx)
    r = elem_ratio(dw.cpu().numpy(), x64.T @ dy.astype(np.float64), np.abs(x64).T @ np.abs(dy).astype(np.float64))
    print(f"bound-ratio dense dw {shape} {r:.3g}")
    assert r <= 1.0, (shape, r)


# ---- the data conditions, without a GPU -----------------------------------------------------------------------------------------------------
def _store_checks():
    for case in FWD_CASES:
        _, _, _, _, ref, tol, ref_t = conv_fwd_case(case)
        yield f"conv3x3 fwd {case}", ref, tol, ref_t
    for case in DGRAD_CASES:
        ref, tol, ref_t = conv_dgrad_case(case)[-3:]
        yield f"conv3x3 dgrad {case}", ref, tol, ref_t
    for shape in C1_SHAPES:
        ref, tol = c1_case(shape)[-2:]
        yield f"first-layer fwd {shape}", ref, tol, None
    for case in CONVT_CASES:
        x, k, b, dy = convT_case(case)
        kq = bfx(k)
        y64, dx4, _, _ = convT_refs(x, kq, b, dy)
        yt, dxt, _, _ = convT_refs(x, trunc_bf16(k), b, dy)
        A = convT_abs_sums(x, kq, dy)
        yield f"convT fwd {case}", y64, EPS_SPLIT * (A["y_a1"] + np.abs(b)), yt
        yield f"convT dgrad {case}", dx4.sum(0), EPS_SPLIT * A["dx_a1"], dxt.sum(0)
    for shape in DENSE_SHAPES:
        ref, tol = dense_case(shape)[-2:]
        yield f"dense dx {shape}", ref, tol, None


def test_data_conditions_hold_without_a_gpu(capsys):
    """For every bf16-stored output of the cases above: RNE_bf16(reference) passes check_store (which also asserts that a truncated copy fails on > 20 % of the
    rounded elements), a truncated copy of the reference is refused, and a reference built from truncated weights fails on a clear share of the elements."""
    for what, ref, tol, ref_t in _store_checks():
        check_store(rne_bf16(ref), ref, None, None, "bf16", what, tol=tol)
        if (rne_bf16(ref) != ref).any():
            with pytest.raises(AssertionError):
                check_store(trunc_bf16(ref), ref, None, None, "bf16", what, tol=tol)
        if ref_t is not None:
            weights_truncation_caught(ref, tol, ref_t, what)
    m = torch.from_numpy(np.array([-0.0, DENORM, -DENORM], np.float32)).bfloat16().float().numpy()          # the mask source's special values survive the host's rounding
    assert np.signbit(m[0]) and m[1] == DENORM and m[2] == -DENORM

"""float64 references and PER-ELEMENT allowances for the short kernels at the end of a step and the classifier's fp32 tail: unet_dense_fwd / _bwd (fp32),
unet_cls_head_fwd / _bwd / unet_cls_loss_finalize (csrc/kernels_dense.hip), unet_adam_keras, unet_seg_metrics_sweep, unet_gather_samples, unet_zero and the two
casts (csrc/kernels_pointwise.hip).  No GPU here: tests/test_tail_bounds_host.py runs every check against an fp32 emulation of the kernel's own summation order
(the emu_* functions below, which also plant the defects), tests/test_gpu_tail_elem.py against the kernels.

Every allowance counts ONE rounding u = 2^-24 per fp32 arithmetic operation along the longest chain that reaches the element, times the sum of the magnitudes
that chain adds up; -ffp-contract=fast may fuse a multiply into an add, which only removes a rounding.  All bounds are first order in u.  An element whose
allowance is 0 must be exact.  The numbers DK, TPB, DB, MAX_BLOCKS, THR_CHUNK are the kernels' (kernels_dense.hip / kernels_pointwise.hip).

The error of expf / logf / log1pf / expm1f cannot be derived from this project; the three constants below are measured on the MI355X through the C ABI with
inputs whose pre-activation is exact (tests/test_gpu_tail_elem.py::test_transcendental_constants, which prints the measurement and asserts it stays below the
constant), then doubled and rounded up to a whole number:
  C_EXPM1    |elu(z) - expm1(z)| / (u |expm1 z|), z < 0 exact: one expm1f call.
  C_SIGMOID  |p - sigmoid(z)| / (u p), z exact: expf, the add, the divide.
  C_BCE      |bce - bce64(p)| / (u (|logit(pc)| + 1)) of ONE row, p the kernel's own fp32 probability: logf, expf, log1pf and the six plain operations of
             bce_clip (1 - pc, the divide, z t, the subtract, the add, the class weight)."""
import numpy as np
import torch

import philox_ref as PX

U = 2.0 ** -24
DK, TPB, DB, MAX_BLOCKS, THR_CHUNK = 256, 256, 128, 2048, 8
SWEEP_MAX_GX = 1024
SLOT_THRESHOLDS = 2048 // 3 // THR_CHUNK * THR_CHUNK          # 680: thresholds per round of the deterministic sweep (UNET_BN_SLOT_DOUBLES = 2048)
FLT_MIN = 2.0 ** -126
LO32, HI32 = np.float32(1e-7), np.float32(1.0) - np.float32(1e-7)          # the clip of bce_clip, as fp32 evaluates it

C_EXPM1 = 3          # measured 1.26 over 4096 z in [-20, -1e-6]
C_SIGMOID = 4        # measured 1.76 over 4096 z in [-80, 17]
C_BCE = 6            # measured 2.9 over 512 single-row launches, z in [-30, 30], t in {0, 0.3, 0.5, 1}: three calls and six plain operations, none above 8 on its own

f32, f64 = np.float32, np.float64


def cdiv(a, b):
    return -(-a // b)


def ratio(got, ref, tol, what):
    """max |got - ref| / tol over the elements (0 where the error is 0); prints it, asserts <= 1 everywhere.  Non-finite `got` where the reference is finite fails."""
    got = np.asarray(got, f64); ref = np.asarray(ref, f64); tol = np.broadcast_to(np.asarray(tol, f64), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(got) | ~np.isfinite(ref), err, np.inf)
    r = np.where(err == 0, 0.0, err / (tol + 1e-300))
    worst = float(r.max()) if r.size else 0.0
    print(f"bound-ratio {what} {worst:.3g}")
    bad = err > tol
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} / {bad.size} elements beyond their allowance; worst ratio {worst:.3g} at {np.unravel_index(int(np.argmax(r)), r.shape)}"
    return worst


def bits_equal(got, want, what):
    """bit-for-bit equality of two arrays of the same item size (NaN payloads and the sign of zero included)"""
    g = np.ascontiguousarray(got); w = np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (what, g.shape, w.shape)
    it = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    bad = g.view(it) != w.view(it)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} / {bad.size} elements differ in their bits; first at {np.argwhere(bad)[0]}"


# ---- dense ----------------------------------------------------------------------------------------------------------------------------------
def dense_case(shape, seed=0, sparse=False):
    """ordinary normals; sparse: only the LAST row of x and the LAST row of W are non-zero (a misplaced row cannot hide)"""
    b, k, n = shape
    rng = np.random.default_rng(1000 * seed + b + k + n)
    x = rng.standard_normal((b, k)).astype(f32); w = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(f32)
    bias = rng.standard_normal(n).astype(f32); dy = rng.standard_normal((b, n)).astype(f32)
    if sparse:
        x[:-1] = 0; w[:-1] = 0; w[-1] = rng.standard_normal(n).astype(f32)
    return x, w, bias, dy


def dense_depth(k):
    """four chains of DK / 4 fmas and their 2 adds per chunk; the chunks in two alternating chains of ceil(chunks / 2); s0 + s1 + bias"""
    chunks = cdiv(k, DK)
    return DK // 4 + 2 + cdiv(chunks, 2) + 2


def dense_fwd_ref(x, w, bias, act, rate=0.0, seed=0):
    """(ref, tol, keep) of unet_dense_fwd.  Pre-activation z: D u (sum_k |x||w| + |bias|), D = dense_depth(K).  ReLU and ELU are 1-Lipschitz: the allowance
    passes through; ELU adds C_EXPM1 u |elu(z)| where z < 0.  Dropout multiplies by the fp32 1 / (1 - rate) of philox_ref.keep_scale_dense: one more rounding;
    keep (bool) is the pattern the kernel must reproduce exactly."""
    x64, w64 = np.asarray(x, f64), np.asarray(w, f64)
    b64 = np.zeros(w64.shape[1]) if bias is None else np.asarray(bias, f64)
    z = x64 @ w64 + b64
    tol = dense_depth(x64.shape[1]) * U * (np.abs(x64) @ np.abs(w64) + np.abs(b64))
    if act == 1:
        ref = np.maximum(z, 0.0)
    elif act == 2:
        ref = np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
        tol = tol + C_EXPM1 * U * np.abs(np.minimum(ref, 0.0))
    else:
        ref = z
    keep = np.ones(z.shape, bool)
    if rate:
        ks = PX.keep_scale_dense(z.shape, rate, seed).astype(f64)
        keep = ks != 0
        tol = (tol + U * np.abs(ref)) * ks; ref = ref * ks
    return ref, tol, keep


def check_dense_fwd(got, x, w, bias, act, rate, seed, what):
    ref, tol, keep = dense_fwd_ref(x, w, bias, act, rate, seed)
    r = ratio(got, ref, tol, what)
    if rate:
        sure = np.abs(ref) > tol                                    # (an element within its allowance of 0 may be an exact 0 of its own)
        assert np.array_equal((np.asarray(got) != 0)[sure | ~keep], keep[sure | ~keep]), f"{what}: the keep pattern differs from philox_ref"
    return r


def dense_bwd_ref(x, w, dy):
    """(dx, tol_dx, dw, tol_dw) of unet_dense_bwd: dw[k][o] is ONE fma chain over the batch, B u sum_b |x||dy|; dx[b][k] a chain of N, N u sum_o |dy||w|"""
    x64, w64, d64 = np.asarray(x, f64), np.asarray(w, f64), np.asarray(dy, f64)
    b, n = d64.shape
    return d64 @ w64.T, n * U * (np.abs(d64) @ np.abs(w64).T), x64.T @ d64, b * U * (np.abs(x64).T @ np.abs(d64))


def check_dense_bwd(dx, dw, x, w, dy, what):
    rdx, tdx, rdw, tdw = dense_bwd_ref(x, w, dy)
    r = ratio(dw, rdw, tdw, what + " dw")
    return (ratio(dx, rdx, tdx, what + " dx") if dx is not None else 0.0), r


def _fma(a, b, c):
    """fl32(a b + c): the product of two floats is exact in float64; the double rounding of the sum is far below every bound here"""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def emu_dense_fwd(x, w, bias, act, rate=0.0, seed=0, defect=None):
    """the kernels' order in fp32: dense_fwd_partial_kernel + dense_fwd_reduce_kernel.  defect: 'partial_chunk' (the last, partial K chunk dropped), 'rows'
    (batch rows past the last full row group dropped), 'odd_chunk' (the odd chunk missed in the reduce), 'bias' (omitted)"""
    b, k = x.shape; n = w.shape[1]
    chunks = cdiv(k, DK); kp = chunks * DK
    xs = np.zeros((b, kp), f32); xs[:, :k] = x; ws = np.zeros((kp, n), f32); ws[:k] = w
    if defect == "partial_chunk" and k % DK:
        xs[:, k // DK * DK:] = 0
    xs = xs.reshape(b, chunks, DK // 4, 4); ws = ws.reshape(chunks, DK // 4, 4, n)
    acc = np.zeros((b, chunks, 4, n), f32)
    for i in range(DK // 4):
        acc = _fma(xs[:, :, i, :, None], ws[None, :, i], acc)
    part = (acc[:, :, 0] + acc[:, :, 1]) + (acc[:, :, 2] + acc[:, :, 3])          # [b][chunk][n]
    s0 = np.zeros((b, n), f32); s1 = np.zeros((b, n), f32)
    c = 0
    while c + 1 < chunks:
        s0 = s0 + part[:, c]; s1 = s1 + part[:, c + 1]; c += 2
    if c < chunks and defect != "odd_chunk":
        s0 = s0 + part[:, c]
    bb = np.zeros(n, f32) if (bias is None or defect == "bias") else np.asarray(bias, f32)
    z = (s0 + s1) + bb
    with np.errstate(over="ignore"):
        y = np.maximum(z, f32(0)) if act == 1 else np.where(z > 0, z, np.expm1(np.minimum(z, f32(0)))).astype(f32) if act == 2 else z
    if rate:
        y = y * PX.keep_scale_dense(y.shape, rate, seed)
    if defect == "rows":
        rows = TPB // n
        y = y.copy(); y[b // rows * rows:] = 0
    return y.astype(f32)


def emu_dense_bwd(x, w, dy, defect=None):
    """dense_bwd_kernel in fp32.  defect: 'tile2' (the dy tiles from b = DB on never reach dw), 'w_row' (dx reads the next row of W)"""
    b, k = x.shape; n = w.shape[1]
    dw = np.zeros((k, n), f32)
    for i in range(b if defect != "tile2" else min(b, DB)):
        dw = _fma(x[i][:, None], dy[i][None, :], dw)
    wr = np.roll(w, -1, 0) if defect == "w_row" else w
    dx = np.zeros((b, k), f32)
    for o in range(n):
        dx = _fma(dy[:, o][:, None], wr[:, o][None, :], dx)
    return dx, dw


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
def adam_case(n, seed=0):
    """magnitudes over several decades (a small p shows a wrong step, a small g a misplaced eps); every 5th element has v = 0, every 7th g = m = v = 0"""
    rng = np.random.default_rng(seed + n % 1000)
    p = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(f32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(f32)
    m = (rng.standard_normal(n) * 0.1).astype(f32); v = (rng.random(n) * 0.01).astype(f32)
    i = np.arange(n)
    v[i % 5 == 0] = 0
    still = i % 7 == 0
    g[still] = 0; m[still] = 0; v[still] = 0
    return p, g, m, v


def adam_lr_t(step, lr=5e-4, b1=0.9, b2=0.999):
    return lr * np.sqrt(1 - b2 ** step) / (1 - b1 ** step)


def adam_ref(p, g, m, v, lr_t, b1, b2, eps, gs):
    """(p, m, v) after unet_adam_keras and their allowances.  The hyper-parameters are the fp32 values the entry point receives; 1 - b1 and 1 - b2 are evaluated in
    fp32 (exactly, as the kernel does: 1.3e-5 relative on 1 - b2).  G = g gs costs a rounding only where gs is not a power of two (r = 0 or 1).
      m' = b1 m + (1-b1) G: two products and the add, (3 + r) u (|b1 m| + |(1-b1) G|)
      v' = b2 v + (1-b2) G G: three products and the add, (4 + 2r) u v' (every term is non-negative, v >= 0)
      p' = p - lr_t m' / (sqrt(v') + eps): tol_m lr_t / den through m'; sqrt(v') moves by (2 + r) u sqrt(v') <= (2 + r) u den through v'; sqrtf, the add,
           lr_t m', the divide: 4 u |step|; the subtract: u |p'|.  The bound rests on hipcc's default of correctly rounded fp32 divide and sqrt."""
    lr_t, b1, b2, eps, gs = (f64(f32(t)) for t in (lr_t, b1, b2, eps, gs))
    c1, c2 = f64(f32(1) - f32(b1)), f64(f32(1) - f32(b2))
    r = 0 if np.frexp(gs)[0] == 0.5 else 1
    p64, m64, v64 = np.asarray(p, f64), np.asarray(m, f64), np.asarray(v, f64)
    G = np.asarray(g, f64) * gs
    m1 = b1 * m64 + c1 * G; tm = (3 + r) * U * (np.abs(b1 * m64) + np.abs(c1 * G))
    v1 = b2 * v64 + c2 * G * G; tv = (4 + 2 * r) * U * v1
    den = np.sqrt(v1) + eps
    step = lr_t * m1 / den
    p1 = p64 - step
    tp = lr_t * tm / den + (6 + r) * U * np.abs(step) + U * np.abs(p1)
    return (p1, m1, v1), (tp, tm, tv)


def check_adam(got, p, g, m, v, lr_t, b1, b2, eps, gs, what):
    ref, tol = adam_ref(p, g, m, v, lr_t, b1, b2, eps, gs)
    rs = [ratio(got[i], ref[i], tol[i], f"{what} {'pmv'[i]}") for i in range(3)]
    still = (np.asarray(g) == 0) & (np.asarray(m) == 0) & (np.asarray(v) == 0)
    bits_equal(np.asarray(got[0], f32)[still], np.asarray(p, f32)[still], what + ": p where g = m = v = 0")
    return rs


def emu_adam(p, g, m, v, lr_t, b1, b2, eps, gs, defect=None):
    """adam_kernel in fp32.  defect: 'tail' (the n & 3 elements behind the last quad untouched), 'gs_sq' (grad_scale on g but not on g^2), 'eps_in' (eps inside
    the square root)"""
    lr_t, b1, b2, eps, gs = (f32(t) for t in (lr_t, b1, b2, eps, gs))
    G = g * gs
    M = b1 * m + (f32(1) - b1) * G
    V = b2 * v + ((f32(1) - b2) * g * g if defect == "gs_sq" else (f32(1) - b2) * G * G)
    P = p - lr_t * M / (np.sqrt(V + eps) if defect == "eps_in" else np.sqrt(V) + eps)
    P, M, V = P.astype(f32), M.astype(f32), V.astype(f32)
    if defect == "tail" and len(p) & 3:
        t = len(p) & ~3
        P[t:], M[t:], V[t:] = p[t:], m[t:], v[t:]
    return P, M, V


# ---- metric sweep ---------------------------------------------------------------------------------------------------------------------------
def sweep_case(n, nthr, seed=0):
    """p, thresholds and gt on the k / 255 grid in fp32 (ties are plentiful); thresholds unsorted, with 0, 1 and a duplicate"""
    rng = np.random.default_rng(seed + n % 9973 + nthr)
    p = (rng.integers(0, 256, n) / 255.0).astype(f32); gt = (np.round(rng.random(n) ** 3 * 255) / 255).astype(f32)
    thr = (rng.integers(1, 255, nthr) / 255.0).astype(f32)
    for i, t in enumerate((p[0], 0.0, 1.0, thr[0])[:nthr]):          # (p[0]: a tie even when n = 1)
        thr[(5 * i) % nthr if nthr > 3 else i] = t
    return p, gt, thr


def sweep_grid(n):
    gx = max(1, min(cdiv(n, TPB * 8), SWEEP_MAX_GX))
    return gx, cdiv(n, gx * TPB)


def sweep_ref(p, gt, thr):
    """(ref [T,3], tol [T,3]) of unet_seg_metrics_sweep: (sum gt [p > t], sum [p > t], sum gt), the comparison in fp32 and strict.  Column 1 is exact (integers
    below 2^24 in fp32, then fp64).  Columns 0 and 2: a per-thread chain of L = ceil(n / (gx 256)), 6 wave steps, 4 block adds in fp32, then fp64 atomics:
    (L + 10) u times the sum of the (non-negative) terms."""
    p, gt, thr = np.asarray(p, f32), np.asarray(gt, f32), np.asarray(thr, f32)
    _, L = sweep_grid(p.size)
    g64 = gt.astype(f64)
    ref = np.empty((thr.size, 3))
    for i, t in enumerate(thr):
        on = p > t
        ref[i] = (g64[on].sum(), np.count_nonzero(on), g64.sum())
    tol = (L + 10) * U * np.abs(ref); tol[:, 1] = 0
    return ref, tol


def check_sweep(got, p, gt, thr, what, pre=None):
    """`pre`: what `out` held before the launch (the sums are ADDED): integer-valued in column 1; the fp64 adds of gx workgroups cost gx 2^-53 of the total"""
    ref, tol = sweep_ref(p, gt, thr)
    if pre is not None:
        ref = ref + pre; tol = tol + sweep_grid(np.asarray(p).size)[0] * 2.0 ** -53 * np.abs(ref); tol[:, 1] = 0
    got = np.asarray(got, f64).reshape(ref.shape)
    assert np.array_equal(got[:, 1], ref[:, 1]), f"{what}: the counts differ at thresholds {np.flatnonzero(got[:, 1] != ref[:, 1])[:8]}"
    return ratio(got, ref, tol, what)


def _block_sum(v):
    """v [..., TPB] fp32 per-thread values -> the workgroup's fp32 sum: wave_sum's xor butterfly (6 steps), then 0 + the four wave sums in order"""
    v = v.reshape(v.shape[:-1] + (TPB // 64, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    s = np.zeros(v.shape[:-2], f32)
    for k in range(TPB // 64):
        s = s + v[..., k, 0]
    return s


def emu_sweep(p, gt, thr, defect=None):
    """metrics_sweep_kernel in fp32 + the fp64 atomics.  defect: 'ge' (>= instead of >), 'block' (the last workgroup's partial missing)"""
    p, gt, thr = np.asarray(p, f32), np.asarray(gt, f32), np.asarray(thr, f32)
    n = p.size; gx, L = sweep_grid(n)
    pp = np.full(L * gx * TPB, -1.0, f32); pp[:n] = p; gg = np.zeros(L * gx * TPB, f32); gg[:n] = gt
    pp = pp.reshape(L, gx, TPB); gg = gg.reshape(L, gx, TPB)
    out = np.zeros((thr.size, 3))
    sg = np.zeros((gx, TPB), f32)
    for j in range(L):
        sg = sg + gg[j]
    last = gx - 1 if defect == "block" else gx
    sgt = _block_sum(sg).astype(f64)[:last].sum()
    for i, t in enumerate(thr):
        tp = np.zeros((gx, TPB), f32); pr = np.zeros((gx, TPB), f32)
        for j in range(L):
            on = (pp[j] >= t) if defect == "ge" else (pp[j] > t)
            tp = tp + np.where(on, gg[j], f32(0)); pr = pr + on.astype(f32)
        out[i] = (_block_sum(tp).astype(f64)[:last].sum(), _block_sum(pr).astype(f64)[:last].sum(), sgt)
    return out


# ---- classifier head ------------------------------------------------------------------------------------------------------------------------
SPECIAL_ROWS = [(25.0, 0.5), (0.0, 0.5), (-25.0, 1.0), (25.0, 0.0), (-25.0, 0.0), (25.0, 1.0), (100.0, 0.0), (-100.0, 1.0), (0.0, 1.0), (20.0, 0.5), (-20.0, 0.5)]


def head_case(b, n, seed=0):
    """h = dropout(relu(normal)), labels from {0, 1, 0.5}, bias = 0, w[0] = 1, w[1] = -1.  The first rows are SPECIAL_ROWS (z, t): h = |z| on column 0 or 1 alone,
    so z is exact: saturated logits of both signs under both labels (the clip arm), h = 0 (p = 0.5 exactly), t p = 0.5 ties."""
    rng = np.random.default_rng(seed + 31 * b + n)
    h = (np.maximum(rng.standard_normal((b, n)), 0) * (rng.random((b, n)) >= 0.4) / 0.6).astype(f32)
    w = (rng.standard_normal(n) * 0.7).astype(f32); w[0] = 1.0; w[1] = -1.0
    t = rng.choice(np.array([0.0, 1.0, 0.5], f32), b).astype(f32)
    for i, (z, ti) in enumerate(SPECIAL_ROWS[:b]):
        h[i] = 0; h[i, 0 if z >= 0 else 1] = abs(z); t[i] = ti
    return h, w, np.zeros(1, f32), t


def _bce64(p32, t):
    """Keras' clipped binary cross-entropy of the fp32 probability p32 in float64, its logit, and whether p32 lies inside the clip range (fp32 comparison)"""
    p32 = np.asarray(p32, f32); t = np.asarray(t, f64)
    inr = (p32 >= LO32) & (p32 <= HI32)
    pc = np.clip(p32, LO32, HI32).astype(f64)
    bce = -(t * np.log(pc) + (1 - t) * np.log1p(-pc))
    return bce, np.log(pc) - np.log1p(-pc), inr, pc


def _rint_clip(a):
    return np.rint(np.clip(a, f32(0), f32(1))).astype(f64)          # np.rint: ties to even, as rintf


def head_fwd_ref(h, w, bias, n=None):
    """(p, tol) of unet_cls_head_fwd: z is a chain of N fmas onto the bias, (N + 1) u (sum |h||w| + |bias|), through sigmoid' = p (1 - p); expf, the add and the
    divide cost C_SIGMOID u p.  Below FLT_MIN the intermediate expf(-z) overflows (z < -88.7) and p is returned as 0: FLT_MIN absolute."""
    h64, w64, b64 = np.asarray(h, f64), np.asarray(w, f64), f64(np.asarray(bias).reshape(-1)[0])
    z = h64 @ w64 + b64
    p = 1.0 / (1.0 + np.exp(-z))
    return p, p * (1 - p) * (h64.shape[1] + 1) * U * (np.abs(h64) @ np.abs(w64) + abs(b64)) + C_SIGMOID * U * p + FLT_MIN


def head_sums_ref(p_got, t, cw0, cw1):
    """(sums [4], tol [4]) from the kernel's OWN fp32 p (the loss is a function of the stored probability; near the clip its slope in p is 1 / (1 - p) ~ 1e7, so a
    reference p cannot stand in): sum cw bce, sum rint(t p), sum rint(t), sum rint(p).  The counts are exact (t p is the fp32 product, ties to even).  The loss:
    C_BCE u (|logit| + 1) per row, then a per-thread chain of ceil(B / 256), 6 wave steps, 4 block adds over cw bce >= 0."""
    p32 = np.asarray(p_got, f32); t32 = np.asarray(t, f32)
    bce, z, _, _ = _bce64(p32, t32)
    cw = np.where(t32 >= f32(0.5), f64(f32(cw1)), f64(f32(cw0)))
    loss = float((cw * bce).sum())
    tol = float((np.abs(cw) * C_BCE * U * (np.abs(z) + 1)).sum()) + (cdiv(p32.size, TPB) + 10) * U * float((np.abs(cw) * bce).sum())
    return np.array([loss, _rint_clip(t32 * p32).sum(), _rint_clip(t32).sum(), _rint_clip(p32).sum()]), np.array([tol, 0.0, 0.0, 0.0])


def check_head_fwd(p_got, sums_got, h, w, bias, t, cw0, cw1, what, pre=None):
    p, tp = head_fwd_ref(h, w, bias)
    r = ratio(p_got, p, tp, what + " p")
    ref, tol = head_sums_ref(p_got, t, cw0, cw1)
    if pre is not None:
        ref = ref + pre; tol = tol + 2.0 ** -52 * np.abs(ref) * (tol > 0)
    return r, ratio(sums_got, ref, tol, what + " sums")


def finalize_ref(sums, count):
    """(loss, f1) of unet_cls_loss_finalize in float64 with K.epsilon() = 1e-7, each rounded to fp32 once: u |value| (+ 2^-50 for the order of the fp64 operations)"""
    s = np.asarray(sums, f64); eps = 1e-7
    prec, rec = s[1] / (s[3] + eps), s[1] / (s[2] + eps)
    ref = np.array([s[0] / count, 2.0 * (prec * rec) / (prec + rec + eps)])
    return ref, (U + 2.0 ** -50) * np.abs(ref)


def head_bwd_ref(h, w, p, t, cw0, cw1, count, rate):
    """references and allowances of unet_cls_head_bwd, p an INPUT (fp32, exact).  Inside the clip range dz = cw(t) (p_clipped - t) / count: the subtract, two
    products and the fp32 1 / count, 4 u |dz|; outside it dz is exactly 0.  dh = dz w scale where h > 0 (exactly 0 elsewhere): two more products and the fp32
    scale = 1 / (1 - rate) (a subtract and a divide): 8 u |dh|.  dw[o] = sum_b dz h, db = sum_b dz, db1[o] = sum_b dh: a chain of ceil(B / rows) per thread, then
    rows - 1 adds, rows = 256 / N, on top of the terms' own roundings."""
    h64, w64, t32, p32 = np.asarray(h, f64), np.asarray(w, f64), np.asarray(t, f32), np.asarray(p, f32)
    b, n = h64.shape; rows = TPB // n; chain = cdiv(b, rows) + rows - 1
    _, _, inr, pc = _bce64(p32, t32)
    cw = np.where(t32 >= f32(0.5), f64(f32(cw1)), f64(f32(cw0)))
    dz = np.where(inr, cw * (pc - t32.astype(f64)) / count, 0.0)
    dh = np.where(h64 > 0, dz[:, None] * w64[None, :] / (1.0 - f64(f32(rate))), 0.0)
    ref = {"dh": dh, "dw": dz @ h64, "db": np.array([dz.sum()]), "db1": dh.sum(0)}
    tol = {"dh": 8 * U * np.abs(dh), "dw": (4 + chain) * U * (np.abs(dz) @ np.abs(h64)), "db": np.array([(4 + chain) * U * np.abs(dz).sum()]),
           "db1": (8 + chain) * U * np.abs(dh).sum(0)}
    return ref, tol


def check_head_bwd(got, h, w, p, t, cw0, cw1, count, rate, what):
    ref, tol = head_bwd_ref(h, w, p, t, cw0, cw1, count, rate)
    return {k: ratio(np.asarray(got[k]).reshape(ref[k].shape), ref[k], tol[k], f"{what} {k}") for k in ("dh", "dw", "db", "db1")}


def emu_head_fwd(h, w, bias, t, cw0, cw1, defect=None):
    """cls_head_fwd_kernel in fp32 -> (p, sums).  defect: 'cw_swap' (class weights swapped), 'half_away' (round half away from zero)"""
    b, n = h.shape
    z = np.full(b, np.asarray(bias, f32).reshape(-1)[0], f32)
    for o in range(n):
        z = _fma(h[:, o], np.broadcast_to(w[o], (b,)), z)
    with np.errstate(over="ignore"):
        p = (f32(1) / (f32(1) + np.exp(-z))).astype(f32)
    pc = np.clip(p, LO32, HI32)
    zz = np.log(pc / (f32(1) - pc))
    bce = np.maximum(zz, f32(0)) - zz * t + np.log1p(np.exp(-np.abs(zz)))
    a, c = (cw0, cw1) if defect == "cw_swap" else (cw1, cw0)
    rnd = (lambda v: np.floor(np.clip(v, f32(0), f32(1)) + f32(0.5))) if defect == "half_away" else (lambda v: np.rint(np.clip(v, f32(0), f32(1))))
    terms = [np.where(t >= f32(0.5), f32(a), f32(c)) * bce, rnd(t * p), rnd(t), rnd(p)]
    sums = []
    for v in terms:
        vp = np.zeros(cdiv(b, TPB) * TPB, f32); vp[:b] = v
        acc = np.zeros(TPB, f32)
        for row in vp.reshape(-1, TPB):
            acc = acc + row
        sums.append(float(_block_sum(acc)))
    return p, np.array(sums)


def emu_head_bwd(h, w, p, t, cw0, cw1, count, rate, defect=None):
    """cls_head_bwd_kernel in fp32.  defect: 'no_clip' (dz not zeroed outside the clip range), 'cw_swap'"""
    b, n = h.shape; rows = TPB // n
    inv, scale = f32(1.0 / count), f32(1) / (f32(1) - f32(rate))
    inr = (p >= LO32) & (p <= HI32)
    pc = np.clip(p, LO32, HI32)
    a, c = (cw0, cw1) if defect == "cw_swap" else (cw1, cw0)
    dz = np.where(t >= f32(0.5), f32(a), f32(c)) * (pc - t) * inv
    if defect != "no_clip":
        dz = np.where(inr, dz, f32(0))
    dz = dz.astype(f32)
    dh = np.where(h > 0, dz[:, None] * w[None, :] * scale, f32(0)).astype(f32)
    bp = cdiv(b, rows) * rows
    pad = lambda a_: np.concatenate([a_, np.zeros((bp - b,) + a_.shape[1:], f32)]).reshape((bp // rows, rows) + a_.shape[1:])          # noqa: E731
    aw = np.zeros((rows, n), f32); ab = np.zeros(rows, f32); a1 = np.zeros((rows, n), f32)
    for zr, hr, gr in zip(pad(dz), pad(h), pad(dh)):
        aw = _fma(np.broadcast_to(zr[:, None], hr.shape), hr, aw); ab = ab + zr; a1 = a1 + gr
    dw, db, db1 = aw[0], ab[0], a1[0]
    for k in range(1, rows):
        dw = dw + aw[k]; db = db + ab[k]; db1 = db1 + a1[k]
    return {"dh": dh, "dw": dw, "db": np.array([db]), "db1": db1}


# ---- gather, zero, cast: bit-exact ------------------------------------------------------------------------------------------------------------
CAST_TABLE = np.array([
    0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0xBF808000, 0xBF818000,          # ties: to the even neighbour below, above; just past / short of a tie; negative
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000,                      # +-0, +-Inf, the quiet NaN
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F7F0000,                      # the largest finite floats: up to Inf (also from the tie), stay finite
    0x00800000, 0x80800000, 0x00808000, 0x007FFFFF, 0x00400000, 0x00008000, 0x00018000, 0x00000001, 0x80000001, 0x00007FFF, 0x00010000,          # smallest normals, subnormals
    0x3F800000, 0x40490FDB, 0xC2F6E979, 0x3EAAAAAB, 0x0000FFFF], dtype=np.uint32)


def bf16_bits_torch(f):
    """torch's fp32 -> bf16 (round to nearest even) as raw uint16"""
    return torch.from_numpy(np.ascontiguousarray(f, f32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


def f32_bits_torch(b16):
    return torch.from_numpy(np.ascontiguousarray(b16, np.uint16).view(np.int16)).view(torch.bfloat16).float().numpy()


def emu_cast(f, defect=None):
    """round to nearest even on the bit pattern (NaN -> the quiet NaN).  defect: 'trunc'"""
    u = np.ascontiguousarray(f, f32).view(np.uint32).astype(np.uint64)
    r = u >> 16 if defect == "trunc" else (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(np.isnan(f), 0x7FC0, r).astype(np.uint16)


def check_cast_to_bf16(got_bits, f, what):
    """bit-equal to torch's .bfloat16() wherever the input is a number; a NaN must come out as a NaN (torch's own CPU conversions write 0x7FC0 from the scalar
    path and 0xFFFF from the vector path, so there are no NaN bits to be equal to)"""
    got = np.asarray(got_bits, np.uint16); want = bf16_bits_torch(f)
    nan = np.isnan(np.asarray(f, f32))
    assert ((got[nan] & 0x7FFF) > 0x7F80).all(), f"{what}: a NaN did not stay a NaN"
    bits_equal(np.where(nan, 0, got).astype(np.uint16), np.where(nan, 0, want).astype(np.uint16), what)


ZERO_PATTERN_MOD = 251


def zero_pattern(nbytes):
    return (np.arange(nbytes, dtype=np.int64) % ZERO_PATTERN_MOD + 1).astype(np.uint8)          # never 0


def check_zero(got, start, nbytes, what):
    """`got`: the whole pattern buffer after unet_zero(start, nbytes): exactly those bytes are 0, every byte before and behind keeps its pattern"""
    want = zero_pattern(len(got)); want[start:start + nbytes] = 0
    bits_equal(np.asarray(got, np.uint8), want, what)


def emu_zero(total, start, nbytes, defect=None):
    """defect: 'tail' (the last of the 1..3 words behind the last 16-byte piece left)"""
    a = zero_pattern(total); pat = a.copy()
    a[start:start + nbytes] = 0
    if defect == "tail" and nbytes & 15:
        a[start + nbytes - 4:start + nbytes] = pat[start + nbytes - 4:start + nbytes]
    return a

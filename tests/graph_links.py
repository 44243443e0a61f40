"""Link checks of the U-Net++ and classifier graphs (pure CPU numpy / torch; test_gpu_graph_links.py runs them on the engine's taps, test_graph_links_host.py on a
stand-in made from the oracle).

A LINK is one materialised tensor (eng.tap(n, name), eng.tap(n, name, grad=True)) or one parameter gradient, together with the float64 function that produces it
from the nearest tensors the engine materialised.  Its inputs are the engine's own stored values -- exact in float64 -- so rounding cannot drift from link to link,
and a wiring error (a wrong buffer, slice, stride, seed, count or mask mode handed to a kernel by build_programs_pp / build_programs_cls in csrc/model.hip) is an
O(1) error of exactly the link it sits in.  The comparison is gpu_util.check_store per element, no element left out: a bf16 tensor must lie in
[RNE_bf16(ref - tol), RNE_bf16(ref + tol)], an fp32 output (parameter gradients, probabilities, the loss pair, h1) within tol of ref.

Allowances (u = 2^-24, EPS_SPLIT = 16 u): the ones the per-op test of the same kernel derives, unchanged; a link over two ops adds theirs.
  conv3x3 forward ......... test_gpu_bf16_conv_elem.py (conv_fwd_ref): EPS_SPLIT (A1 + |bias|), ELU + 4 u |ref|, keep scale: tol ks + 2 u |ref|
  conv3x3 data gradient ... test_gpu_bf16_conv_elem.py (conv_dgrad_ref): EPS_SPLIT A1, mask factors k = 3 (ELU) / 4 (ELU + dropout)
  conv3x3 / ConvT dw, db .. test_gpu_bf16_conv_elem.py: EPS_SPLIT A1 (gpu_util.elem_ratio)
  ConvT forward / dgrad ... test_gpu_bf16_conv_elem.py: EPS_SPLIT (A1 + |bias|) / EPS_SPLIT A1
  dense (bf16 storage) .... test_gpu_bf16_conv_elem.py: y, dw, dx EPS_SPLIT A1;  dense (fp32): tests/tail_checks.py dense_fwd_ref / dense_bwd_ref
  folded conv, 3 launches . tests/bnfold_checks.py fwd_problem / wgrad_problem / dgrad_problem (test_gpu_bnfold_elem.py)
  bn_stats ................ test_gpu_storage_ops.py: (n1 + T + 2) u sum |x|, (n1 + T + 3) u sum x^2 (stats_terms: the launch geometry)
  bn_apply (+ pool) ....... test_gpu_storage_ops.py: 2 u (|x scale| + |shift|), fused with the pool 3 u, the pooled value the window's maximum of both
  bn_bwd_stats / _apply ... test_gpu_storage_ops.py: (n1 + T + 2) u sum |dy|, (n1 + T + 5) u sum |dy xhat|;  8 u A
  pool_bwd_sums, bn_maxpool_bwd_apply ... test_gpu_storage_ops.py: (n1 + T + 3 / 6) u sum |terms|;  8 u A
  pool backward, accum_slices, copy_slice  test_gpu_storage_ops.py: exact routing / copy; one rounding of the fp32 sum, k = 2 per launch
  head (segmentation) ..... test_gpu_storage_ops.py head_check: p, loss sums (n1 + 12) u, dx k = 10, dw / db
  classifier head, loss ... tests/tail_checks.py head_fwd_ref / head_sums_ref / finalize_ref / head_bwd_ref
Terms a link adds because it spans ops (each written out where it is formed):
  * BatchNorm: in both graphs bn_stats reads the STORED tensor (model.hip: every bn_stats:<name> op of build_programs_pp and build_programs_cls calls
    unet_bn_stats[_bf16] on m->Av(in); neither builder arms a statistics epilogue), so the batch statistics are float64 statistics of the tap.  bn_finalize forms
    scale / shift in double from double sums and rounds to fp32: the reference scale / shift carry the bn_stats allowance pushed through mean, variance and
    1 / sqrt (bn_params: d_scale, d_shift), and a BatchNorm output |x| d_scale + d_shift on top of bn_apply's own.
  * BatchNorm backward: k1, k2 carry the bn_bwd_stats allowance divided by the count; dx adds |scale m| (e_k1 + |xhat| e_k2).
  * the classifier's fused tail takes its sums from the POOLED tensors (pool_bwd_sums: xhat of an arg-max element = (p (1 - rate) - beta) / gamma with p the stored
    pooled activation): the reference takes the same sums from the p tap -- the operation the kernel defines -- under that kernel's own allowance.
  * folded conv: the engine rounds scale[c] * w to bf16 again; a weight whose product lies within d_scale |w| of a rounding midpoint may round either way:
    sum |x| (hi - lo) over those weights is added (fp32 storage: sum |x| |w| d_scale), and the border table's sum |w| d_shift.
  * a gradient buffer written by several launches (pool backward, a ConvT's data gradient through its bf16 staging tensor, the accum_slice of the noted concat
    slices) is never seen between them: the reference follows the launches in program order as an interval [lo, hi] that is stored (rounded) after each
    (grad_sum; the interval's centre and half-width go to check_store, so its `bound-ratio` line reads 1 wherever an element sits on an end of a non-empty interval).
Dropout keep factors come from tests/philox_ref.py with the key the program uses, drop_seed + seed_of(conv) (fc1: drop_seed + a constant); every dropout link also
asserts that the zeros of the stored tensor are the dropped elements.  The max-pool routes to the first maximum of the stored values in the order (0,0) (0,1) (1,0)
(1,1) (bn_maxpool_bwd_apply: of the recomputed fp32 y = fma(x, scale, shift)), as test_gpu_storage_ops.py states it."""
import numpy as np
import torch
import torch.nn.functional as F

import bnfold_checks as B
import loss_family_oracle as LF
import philox_ref as PX
import tail_checks as T
from gpu_util import EPS_SPLIT, U, check_store, convT_abs_sums, rne_bf16
from oracle import unet_oracle as O

f64 = np.float64
M64 = (1 << 64) - 1
FC_SEED = 0xC2B2AE3D27D4EB4F
TPB = 256
BN_STATS_BLOCKS, BN_BWD_STATS_BLOCKS = 512, 1024          # kernels_pointwise.hip, as test_gpu_storage_ops.py mirrors them
HEAD_LPP_BLOCKS, HEAD_BWD_BLOCKS, MAX_BLOCKS = 2048, 1024, 2048
LO32, HI32 = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))
ELU, RELU = 2, 1
MASK_NONE, MASK_RELU, MASK_ELU, MASK_ELU_DROP = 0, 1, 2, 3


def cdiv(a, b):
    return -(-int(a) // int(b))


def nchw(a):
    return torch.as_tensor(np.array(a, f64)).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def conv64(x, k, b=None):
    return nhwc(F.conv2d(nchw(x), torch.as_tensor(np.asarray(k, f64)).permute(3, 2, 0, 1), None if b is None else torch.as_tensor(np.asarray(b, f64)), padding=1))


def dgrad64(dy, k):
    return nhwc(F.conv_transpose2d(nchw(dy), torch.as_tensor(np.asarray(k, f64)).permute(3, 2, 0, 1), padding=1))


def wgrad64(x, dy):
    return B.wgrad64(B.t64(x), B.t64(dy)).numpy()


def windows(a):
    return np.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]])


def unwindows(v):
    n, ho, wo, c = v.shape[1:]
    out = np.zeros((n, 2 * ho, 2 * wo, c), v.dtype)
    out[:, 0::2, 0::2], out[:, 0::2, 1::2], out[:, 1::2, 0::2], out[:, 1::2, 1::2] = v[0], v[1], v[2], v[3]
    return out


def route(dyp, x):
    """pool backward: dyp to the first maximum of every 2 x 2 window of x (np.argmax: the first of equal values), zero elsewhere"""
    arg = np.argmax(windows(x), 0)
    return unwindows(np.stack([np.where(arg == k, dyp, 0.0) for k in range(4)]))


def stats_terms(pixels, c, cap):
    ppb = TPB // (c // 4)
    grid = max(1, min(cdiv(pixels, ppb * 16), cap))
    return cdiv(pixels, grid * ppb) + ppb


def seed_of(table, conv):
    return ((([t[0] for t in table].index(conv)) + 1) * 0x9E3779B97F4A7C15) & M64


def mask_factor(mode, x, rate, ks):
    """(factor, the magnitude its fp32 evaluation rounds against) of the producer of x: test_gpu_storage_ops.mask_ref"""
    if mode == MASK_NONE:
        return np.ones_like(x), np.zeros_like(x)
    if mode == MASK_RELU:
        return (x > 0).astype(f64), np.zeros_like(x)
    if mode == MASK_ELU:
        return np.where(x > 0, 1.0, x + 1.0), np.where(x > 0, 0.0, np.abs(x) + 1.0)
    a = x * float(np.float32(1.0) - np.float32(rate))
    return ks * np.where(a > 0, 1.0, a + 1.0), ks * (2 * np.abs(a) + 1.0)


def case_weights(arch, seed, hw):
    """random parameters of a link case: biases / beta / gamma away from their initial 0 / 1; the conv and ConvT kernels the engine rounds to bf16 for the MFMA are bf16
    already (as test_gpu_bf16_model._case), so both sides hold one value; c1a, the 1 x 1 head and the dense layers run on fp32 weights"""
    rng = np.random.default_rng(seed)
    wts = O.pp_init_weights(seed=seed) if arch == "unetpp" else O.cls_init_weights(seed, 1, hw)
    for k in wts:
        if k.endswith("/bias") or k.endswith("/beta"):
            wts[k] = (rng.standard_normal(wts[k].shape) * 0.1).astype(np.float32)
        if k.endswith("/gamma"):
            wts[k] = rng.uniform(0.5, 1.5, wts[k].shape).astype(np.float32)
        if k.endswith("/kernel") and wts[k].ndim == 4 and k not in ("c1a/kernel", "out/kernel"):
            wts[k] = torch.from_numpy(wts[k]).bfloat16().float().numpy()
    return wts


class Src:
    """What the links read: act(name) / grad(name) -> float64 array (grad: None where the tap is not a tensor), the parameter gradients, the batch, the fp32
    parameters, the probabilities and the loss pair.  drop_seed: the key of this forward's dropout streams (None: dropout off); folded: the second convs whose
    BatchNorm in front is folded; fused_tail: the classifier's encoder tail runs pool_bwd_sums + bn_pool_bwd_apply; ops: the op names of the two programs (or None)."""

    def __init__(self, arch, dt, x, y, weights, act, grad, pgrads, p, loss, drop_seed=None, folded=(), fused_tail=True, class_weights=(1.0, 1.0), ops=None):
        self.arch, self.dt, self.x, self.y = arch, dt, np.asarray(x, f64), np.asarray(y, f64)
        self.w = {k: np.asarray(v, np.float32).astype(f64) for k, v in weights.items()}
        self._act, self._grad, self._ca, self._cg = act, grad, {}, {}
        self.pgrads = {k: np.asarray(v, f64) for k, v in pgrads.items()}
        self.p, self.loss = np.asarray(p, f64), np.asarray(loss, f64)
        self.drop_seed, self.folded, self.fused_tail, self.cw, self.ops = drop_seed, set(folded), fused_tail, class_weights, ops
        self.n = self.x.shape[0]
        self.table = O.pp_layer_table(self.x.shape[-1]) if arch == "unetpp" else O.cls_layer_table(self.x.shape[-1], self.x.shape[1:3])

    def act(self, name):
        if name not in self._ca:
            self._ca[name] = np.asarray(self._act(name), f64)
        return self._ca[name]

    def grad(self, name):
        if name not in self._cg:
            g = self._grad(name)
            self._cg[name] = None if g is None else np.asarray(g, f64)
        return self._cg[name]


def engine_src(eng, x, y, weights, class_weights=(1.0, 1.0)):
    """run forward + backward on `eng` (weights set by the caller) and wrap its taps"""
    from covidseg_amd import _lib
    n = len(x)
    key = (eng.seed * 1000003 + eng._drop_calls) & M64            # engine.forward_backward: the Philox key of this training forward (rank 0)
    loss = eng.forward_backward(x, y).cpu().numpy()

    def grad(name):
        try:
            return eng.tap(n, name, grad=True)
        except _lib.UNetHipError:
            return None

    ops = [o[0] for o in eng.op_profile(n, 0)] + [o[0] for o in eng.op_profile(n, 1)]
    folded = {o.split(":")[1] for o in ops if o.startswith("bn_fold_prepare:")}
    return Src(eng.arch, eng.dtype, x, y, weights, lambda nm: eng.tap(n, nm), grad, eng.get_grads(), eng._p_train.cpu().numpy(), loss,
               drop_seed=key if eng.dropout_rate > 0 else None, folded=folded, fused_tail=any(o.startswith("bn_pool_bwd_apply:") for o in ops),
               class_weights=class_weights, ops=ops)


class Links:
    """runs links on a Src.  collect=True: a failing link is recorded in .failed (name -> message) instead of raising"""

    def __init__(self, src, collect=False):
        self.s, self.collect = src, collect
        self.ran, self.failed, self.params = {}, {}, set()

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
    def _fail(self, link, msg):
        if not self.collect:
            raise AssertionError(f"link {link}: {msg}")
        self.failed.setdefault(link, msg)

    def chk(self, link, got, ref, tol, stored=True, ops=(), param=None):
        self.ran.setdefault(link, set()).update(ops)
        if param:
            self.params.add(param)
        got, ref = np.asarray(got, f64), np.asarray(ref, f64)
        if got.shape != ref.shape:
            return self._fail(link, f"shape {got.shape} against {ref.shape}")
        try:
            check_store(got, ref, None, None, self.s.dt if stored else "fp32", f"link {link}", tol=np.broadcast_to(np.asarray(tol, f64), ref.shape))
        except AssertionError as e:
            self._fail(link, str(e))

    def same(self, link, got, want, ops=()):
        self.ran.setdefault(link, set()).update(ops)
        if got.shape != want.shape or not np.array_equal(got, want):
            self._fail(link, "not an exact copy" if got.shape == want.shape else f"shape {got.shape} against {want.shape}")

    def st_lo(self, v):
        return rne_bf16(v) if self.s.dt == "bf16" else v - U * np.abs(v)

    def st_hi(self, v):
        return rne_bf16(v) if self.s.dt == "bf16" else v + U * np.abs(v)

    def kq(self, name):
        """the kernel of conv / ConvT `name` as the matrix cores see it: bf16 storage rounds it (the first conv and the 1 x 1 head run on fp32 weights)"""
        k = self.s.w[name + "/kernel"]
        return rne_bf16(k) if (self.s.dt == "bf16" and name not in ("c1a", "out")) else k

    def keep(self, shape, conv, rate):
        """fp32 keep factors of the dropout behind `conv` (None: dropout off), with the key the program uses"""
        if self.s.drop_seed is None or not rate:
            return None
        sd = FC_SEED if conv == "fc1" else seed_of(self.s.table, conv)
        return PX.keep_scale_dense(shape, rate, (self.s.drop_seed + sd) & M64).astype(f64)

    def zeros_agree(self, link, got, ks, ref, tol):
        if ks is None:
            return
        sure = np.abs(ref) > tol                                        # (an element within its allowance of 0 may be an exact 0 of its own)
        if (got[ks == 0] != 0).any() or (got[(ks != 0) & sure] == 0).any():
            self._fail(link, "the zeros of the stored tensor are not the elements philox_ref drops with drop_seed + seed_of(conv)")

    # ---- BatchNorm parameters from the stored input -----------------------------------------------------------------------------------------
    def bn_params(self, bn, x):
        """scale / shift / mean / istd as bn_finalize_train_kernel forms them (double statistics, fp32 results) from float64 statistics of the stored x, and how far
        the engine's may lie from them: bn_stats' allowance (e_m on the mean, e_q on the mean square) through var = q - m^2, istd = (var + eps)^-1/2 (slope
        istd^3 / 2), scale = gamma istd, shift = beta - mean scale, one fp32 rounding (u) per operation."""
        c = x.shape[-1]
        x2 = x.reshape(-1, c)
        pixels = x2.shape[0]
        gamma, beta = self.s.w[bn + "/gamma"], self.s.w[bn + "/beta"]
        mean = x2.mean(0); q = (x2 * x2).mean(0)
        var = np.maximum(q - mean * mean, 0.0)
        f32 = lambda a: np.asarray(a, np.float32).astype(f64)
        istd = f32(1.0 / np.sqrt(var + float(np.float32(O.BN_EPS))))
        sc = f32(gamma * istd); m32 = f32(mean); sh = f32(beta - m32 * sc)
        nt = stats_terms(pixels, c, BN_STATS_BLOCKS)
        e_m = (nt + 2) * U * np.abs(x2).mean(0); e_q = (nt + 3) * U * q
        e_var = e_q + 2 * np.abs(mean) * e_m
        d_istd = 0.5 * istd ** 3 * e_var + U * istd
        d_sc = np.abs(gamma) * d_istd + U * np.abs(sc)
        d_sh = np.abs(mean) * d_sc + np.abs(sc) * (e_m + U * np.abs(mean)) + 2 * U * (np.abs(beta) + np.abs(mean * sc))
        return dict(sc=sc, sh=sh, mean=m32, istd=istd, d_sc=d_sc, d_sh=d_sh, d_mean=e_m + U * np.abs(mean), d_istd=d_istd, pixels=pixels, gamma=gamma, beta=beta)

    # ---- forward links ----------------------------------------------------------------------------------------------------------------------
    def conv_fwd(self, name, src_name, act, rate):
        x = self.s.x if not src_name else self.s.act(src_name)
        kq, b = self.kq(name), self.s.w[name + "/bias"]
        v = conv64(x, kq, b)
        tol = EPS_SPLIT * (conv64(np.abs(x), np.abs(kq)) + np.abs(b))
        self._act_epilogue(f"fwd {name}", name, v, tol, act, rate, [f"conv3x3_fwd:{name}"])

    def _act_epilogue(self, link, name, v, tol, act, rate, ops):
        if act == RELU:
            ref = np.maximum(v, 0.0)
        else:
            ref = np.where(v > 0, v, np.expm1(np.minimum(v, 0.0))); tol = tol + 4 * U * np.abs(ref)
        ks = self.keep(ref.shape, name, rate)
        if ks is not None:
            ref = ref * ks; tol = tol * ks + 2 * U * np.abs(ref)
        got = self.s.act(name)
        self.chk(link, got, ref, tol, ops=ops)
        self.zeros_agree(link, got, ks, ref, tol)

    def conv_fwd_folded(self, name, x_name, bn, act, rate):
        """BatchNorm `bn` of the stored x folded into conv `name`: conv3x3(x, RNE_bf16(fp32(scale w))) + the border-class table of shift (bnfold_checks.fwd_problem:
        EPS_SPLIT A1 (1 + 1/16) + k_tab u (|b| + T1)), plus the two terms of the module docstring for the engine's own scale / shift."""
        x = self.s.act(x_name)
        P = self.bn_params(bn, x)
        k, b = self.s.w[name + "/kernel"], self.s.w[name + "/bias"]
        sc4 = P["sc"][None, None, :, None]
        ws = (k * sc4).astype(np.float32).astype(f64)
        dw = np.abs(k) * P["d_sc"][None, None, :, None] + U * np.abs(ws)
        if self.s.dt == "bf16":
            wq, wamb = rne_bf16(ws), rne_bf16(ws + dw) - rne_bf16(ws - dw)
        else:
            wq, wamb = ws, 2 * dw
        n, h, w, ci = x.shape
        shimg = np.broadcast_to(P["sh"], (1, h, w, ci))
        v = conv64(x, wq) + conv64(shimg, k, b)
        t1 = conv64(np.abs(shimg), np.abs(k))
        tol = EPS_SPLIT * conv64(np.abs(x), np.abs(wq)) * (1.0 + 1.0 / 16.0) + B.k_tab(ci) * U * (np.abs(b) + t1)
        tol = tol + conv64(np.abs(x), wamb) + conv64(np.broadcast_to(P["d_sh"], (1, h, w, ci)), np.abs(k))
        self._act_epilogue(f"fwd folded {bn}>{name}", name, v, tol, act, rate, [f"bn_stats:{bn}", f"bn_finalize:{bn}", f"bn_fold_prepare:{name}", f"conv3x3_fwd:{name}"])

    def bn_fwd(self, bn, x_name, out, pool=None):
        x = self.s.act(x_name)
        P = self.bn_params(bn, x)
        y = x * P["sc"] + P["sh"]
        tol = (3 if pool else 2) * U * (np.abs(x * P["sc"]) + np.abs(P["sh"])) + np.abs(x) * P["d_sc"] + P["d_sh"]
        ops = [f"bn_stats:{bn}", f"bn_finalize:{bn}", f"bn_apply_pool:{pool}" if pool else f"bn_apply:{bn}"]
        self.chk(f"fwd {bn}>{out}", self.s.act(out), y, tol, ops=ops)
        if pool:
            n, h, w, c = y.shape
            e = (slice(None), slice(0, h // 2 * 2), slice(0, w // 2 * 2))
            self.chk(f"fwd {bn}>{pool}", self.s.act(pool), windows(y[e]).max(0), windows(tol[e]).max(0), ops=ops)

    def convT_fwd(self, node, src_name, cat, c):
        x = self.s.act(src_name)
        u = "u" + node[1:]
        kq, b = self.kq(u), self.s.w[u + "/bias"]
        ref = O.convT2x2s2_bias(torch.as_tensor(x), torch.as_tensor(kq), torch.as_tensor(b)).numpy()
        a1 = convT_abs_sums(x, kq, np.zeros(ref.shape))["y_a1"]
        tol = EPS_SPLIT * (a1 + np.abs(b))
        self.chk(f"fwd {u} (tap)", self.s.act(u), ref, tol, ops=[f"convT_fwd:{u}"])
        self.chk(f"fwd {u} = {cat}[:{c}]", self.s.act(cat)[..., :c], ref, tol, ops=[f"convT_fwd:{u}"])

    # ---- backward links ---------------------------------------------------------------------------------------------------------------------
    def bn_bwd(self, bn, dy_name, x_name, mode, rate, drop_conv):
        """grad[x_name] = scale (dy - k1 - xhat k2) m(x) from grad[dy_name] and the stored x; gamma / beta gradients = the two sums"""
        dy, x = self.s.grad(dy_name), self.s.act(x_name)
        P = self.bn_params(bn, x)
        c = x.shape[-1]; pixels = P["pixels"]
        ks = self.keep(x.shape, drop_conv, rate) if mode == MASK_ELU_DROP else None
        if mode == MASK_ELU_DROP and ks is None:
            mode = MASK_ELU
        xh = (x - P["mean"]) * P["istd"]
        d_xh = P["istd"] * P["d_mean"] + np.abs(x - P["mean"]) * P["d_istd"]
        s1, s2 = dy.reshape(-1, c).sum(0), (dy * xh).reshape(-1, c).sum(0)
        ppb = TPB // (c // 4)
        nt = cdiv(pixels, max(1, min(cdiv(pixels, ppb * 16), BN_BWD_STATS_BLOCKS)) * ppb) + ppb
        e1 = (nt + 2) * U * np.abs(dy).reshape(-1, c).sum(0)
        e2 = (nt + 5) * U * np.abs(dy * xh).reshape(-1, c).sum(0) + (np.abs(dy) * d_xh).reshape(-1, c).sum(0)
        ops = [f"bn_bwd_stats:{bn}", f"bn_bwd_apply:{bn}"]
        self.chk(f"param {bn}/beta", self.s.pgrads[bn + "/beta"], s1, e1 + U * np.abs(s1), stored=False, ops=ops, param=bn + "/beta")
        self.chk(f"param {bn}/gamma", self.s.pgrads[bn + "/gamma"], s2, e2 + U * np.abs(s2), stored=False, ops=ops, param=bn + "/gamma")
        k1, k2 = s1 / pixels, s2 / pixels
        mf, mA = mask_factor(mode, x, rate, ks)
        D = dy - k1 - xh * k2
        ref = P["sc"] * D * mf
        A = np.abs(P["sc"]) * (np.abs(dy) + np.abs(k1) + np.abs(xh * k2)) * (np.abs(mf) + mA)
        tol = 8 * U * A + np.abs(mf) * (np.abs(P["sc"]) * (e1 / pixels + np.abs(xh) * e2 / pixels + np.abs(k2) * d_xh) + np.abs(D) * P["d_sc"])
        self.chk(f"bwd {bn}: {dy_name}>{x_name}", self.s.grad(x_name), ref, tol, ops=ops)
        if ks is not None and (self.s.grad(x_name)[ks == 0] != 0).any():
            self._fail(f"bwd {bn}: {dy_name}>{x_name}", "the backward's keep mask is not the forward's (philox_ref, drop_seed + seed_of(conv))")

    def conv_dgrad(self, name, in_name, mode, rate, drop_conv):
        dy, kq = self.s.grad(name), self.kq(name)
        v = dgrad64(dy, kq)
        tol = EPS_SPLIT * dgrad64(np.abs(dy), np.abs(kq))
        link = f"bwd dgrad {name}>{in_name}"
        if mode != MASK_NONE:
            m = self.s.act(in_name)
            ks = self.keep(m.shape, drop_conv, rate) if mode == MASK_ELU_DROP else None
            if mode == MASK_ELU_DROP and ks is None:
                mode = MASK_ELU
            mf, mA = mask_factor(mode, m, rate, ks)
            kk = {MASK_RELU: 0, MASK_ELU: 3, MASK_ELU_DROP: 4}[mode]
            v, tol = v * mf, tol * np.abs(mf) + kk * U * np.abs(v) * (np.abs(mf) + mA)
            if ks is not None and (self.s.grad(in_name)[ks == 0] != 0).any():
                self._fail(link, "the backward's keep mask is not the forward's (philox_ref, drop_seed + seed_of(conv))")
        self.chk(link, self.s.grad(in_name), v, tol, ops=[f"conv3x3_dgrad:{name}"])

    def conv_wgrad(self, name, in_name):
        x = self.s.x if not in_name else self.s.act(in_name)
        dy = self.s.grad(name)
        ops = [f"conv3x3_wgrad:{name}"]
        self.chk(f"param {name}/kernel", self.s.pgrads[name + "/kernel"], wgrad64(x, dy), EPS_SPLIT * wgrad64(np.abs(x), np.abs(dy)), stored=False, ops=ops, param=name + "/kernel")
        self.chk(f"param {name}/bias", self.s.pgrads[name + "/bias"], dy.sum((0, 1, 2)), EPS_SPLIT * np.abs(dy).sum((0, 1, 2)), stored=False, ops=ops, param=name + "/bias")

    def _fold_case(self, name, x_name, bn):
        x, dy = self.s.act(x_name), self.s.grad(name)
        P = self.bn_params(bn, x)
        n, h, w, ci = x.shape
        case = dict(x=x, k=self.s.w[name + "/kernel"], dy=dy, scale=P["sc"], shift=P["sh"], mean=P["mean"], istd=P["istd"], shape=(n, h, w, ci, dy.shape[-1]))
        return case, P, B.wgrad_problem(case)

    def folded_wgrad(self, name, x_name, bn):
        """the folded conv's corrected weight gradient scale dW_raw + shift S, its bias gradient, and the folded BatchNorm's gamma / beta from W . dW_raw and W . S
        (bnfold_checks.wgrad_problem); the engine's own scale / shift add |dW_raw| d_scale + |S| d_shift, its own mean / istd |s1| d_mean istd + (..) d_istd"""
        case, P, Q = self._fold_case(name, x_name, bn)
        ops = [f"conv3x3_wgrad:{name}", f"wgrad_bn_fold_fix:{name}"]
        tol = Q["dw_bound"].numpy() + np.abs(Q["dw_raw"].numpy()) * P["d_sc"][None, None, :, None] + np.abs(Q["S"].numpy())[:, :, None, :] * P["d_sh"][None, None, :, None]
        self.chk(f"param {name}/kernel (folded)", self.s.pgrads[name + "/kernel"], Q["dw"].numpy(), tol, stored=False, ops=ops, param=name + "/kernel")
        self.chk(f"param {name}/bias (folded)", self.s.pgrads[name + "/bias"], Q["db"].numpy(), Q["db_bound"].numpy(), stored=False, ops=ops, param=name + "/bias")
        ci = case["shape"][3]
        sums, sb = Q["sums"].numpy(), Q["sums_bound"].numpy()
        dzx = np.abs((Q["dz"].numpy() * case["x"]).reshape(-1, ci)).sum(0); dza = np.abs(Q["dz"].numpy()).reshape(-1, ci).sum(0)
        e2 = sb[ci:] + P["d_istd"] * (dzx + np.abs(P["mean"]) * dza) + P["istd"] * P["d_mean"] * dza
        self.chk(f"param {bn}/beta (folded)", self.s.pgrads[bn + "/beta"], sums[:ci], sb[:ci] + U * np.abs(sums[:ci]), stored=False, ops=ops, param=bn + "/beta")
        self.chk(f"param {bn}/gamma (folded)", self.s.pgrads[bn + "/gamma"], sums[ci:], e2 + U * np.abs(sums[ci:]), stored=False, ops=ops, param=bn + "/gamma")

    def folded_dgrad(self, name, x_name, bn, mode, rate, drop_conv):
        """from the folded conv's output gradient to the gradient of `x_name`'s output through the data-gradient epilogue (the folded BatchNorm's own gradient is
        not a tensor: its tap answers UNET_E_STATE): bnfold_checks.dgrad_problem on the float64 sums, plus the sums' own allowance (wgrad_problem) over the count"""
        if self.s.grad(bn) is not None:
            self._fail(f"bwd folded {name}>{x_name}", f"the gradient tap of the folded {bn} is a tensor")
        case, P, Q = self._fold_case(name, x_name, bn)
        seed = 0
        if mode == MASK_ELU_DROP and self.s.drop_seed is not None:
            seed = (self.s.drop_seed + seed_of(self.s.table, drop_conv)) & M64
        elif mode == MASK_ELU_DROP:
            mode = MASK_ELU
        D = B.dgrad_problem(case, Q["sums"], mode=mode, rate=rate if mode == MASK_ELU_DROP else 0.0, seed=seed)
        ci = case["shape"][3]; cnt = Q["count"]
        x = case["x"]
        f = B.mask_factor64(torch.as_tensor(x), mode, rate if mode == MASK_ELU_DROP else 0.0, seed).numpy()
        xh = (x - P["mean"]) * P["istd"]
        sb = Q["sums_bound"].numpy()
        K0dz = np.abs(P["sc"] * Q["dz"].numpy())
        tol = D["bound"].numpy() + np.abs(f) * (np.abs(P["sc"]) * (sb[:ci] / cnt + np.abs(xh) * sb[ci:] / cnt) + (K0dz + np.abs(D["ref"].numpy())) * P["d_sc"] / np.abs(P["sc"]))
        link = f"bwd folded {name}>{x_name}"
        self.chk(link, self.s.grad(x_name), D["ref"].numpy(), tol, ops=[f"conv3x3_dgrad_bn_bwd:{name}"])
        if mode == MASK_ELU_DROP and (self.s.grad(x_name)[f == 0] != 0).any():
            self._fail(link, "the backward's keep mask is not the forward's (philox_ref, drop_seed + seed_of(conv))")

    # ---- U-Net++ ------------------------------------------------------------------------------------------------------------------------------
    def run_unetpp(self):
        s = self.s
        nodes = {n[0]: n for n in O.PP_NODES}
        drop = s.drop_seed is not None
        enc_r, blk_r = (O.PP_ENC_DROP, O.PP_BLOCK_DROP) if drop else (0.0, 0.0)
        cat_off = {}
        for it in ["e1", "e2", "x1_2", "e3", "x2_2", "x1_3", "e4", "x3_2", "x2_3", "x1_4"]:
            if it[0] == "e":
                k = int(it[1])
                self.conv_fwd(f"c{k}a", "" if k == 1 else f"p{k - 1}", ELU, enc_r)
                self.conv_fwd(f"c{k}b", f"c{k}a", ELU, 0.0)
                self.bn_fwd(f"bn{k}", f"c{k}b", f"c{k}", pool=f"p{k}" if k <= 3 else None)
                continue
            _, c, src_name, skips = nodes[it]
            cat = "cat_" + it
            self.convT_fwd(it, src_name, cat, c)
            off = c
            for sk in skips:
                cw = O.PP_WIDTH[sk]
                cat_off[(it, sk)] = off
                self.same(f"fwd {sk} = {cat}[{off}:{off + cw}]", s.act(cat)[..., off:off + cw], s.act(sk), ops=[f"copy_slice:{sk}>{it}"])
                off += cw
            self.conv_fwd(it + "a", cat, ELU, blk_r)
            if it + "b" in s.folded:
                self.conv_fwd_folded(it + "b", it + "a", it + "abn", ELU, blk_r)
            else:
                self.bn_fwd(it + "abn", it + "a", it + "abn")
                self.conv_fwd(it + "b", it + "abn", ELU, blk_r)
            self.bn_fwd(it + "bbn", it + "b", it)
        self.seg_head()
        # backward, reverse creation order
        stages = O.pp_grad_stages()
        for it in reversed(["e1", "e2", "x1_2", "e3", "x2_2", "x1_3", "e4", "x3_2", "x2_3", "x1_4"]):
            if it[0] == "e":
                k = int(it[1])
                self.grad_sum(f"c{k}", stages.get(f"c{k}"), cat_off)
                self.bn_bwd(f"bn{k}", f"c{k}", f"c{k}b", MASK_ELU, 0.0, None)
                self.conv_wgrad(f"c{k}b", f"c{k}a")
                self.conv_dgrad(f"c{k}b", f"c{k}a", MASK_ELU_DROP, O.PP_ENC_DROP, f"c{k}a")
                self.conv_wgrad(f"c{k}a", "" if k == 1 else f"p{k - 1}")
                if k > 1:
                    self.conv_dgrad(f"c{k}a", f"p{k - 1}", MASK_NONE, 0.0, None)
                continue
            _, c, src_name, skips = nodes[it]
            cat, u = "cat_" + it, "u" + it[1:]
            if it != "x1_4":
                self.grad_sum(it, stages.get(it), cat_off)
            self.bn_bwd(it + "bbn", it, it + "b", MASK_ELU_DROP, O.PP_BLOCK_DROP, it + "b")
            if it + "b" in s.folded:
                self.folded_wgrad(it + "b", it + "a", it + "abn")
                self.folded_dgrad(it + "b", it + "a", it + "abn", MASK_ELU_DROP, O.PP_BLOCK_DROP, it + "a")
            else:
                self.conv_wgrad(it + "b", it + "abn")
                self.conv_dgrad(it + "b", it + "abn", MASK_NONE, 0.0, None)
                self.bn_bwd(it + "abn", it + "abn", it + "a", MASK_ELU_DROP, O.PP_BLOCK_DROP, it + "a")
            self.conv_wgrad(it + "a", cat)
            self.conv_dgrad(it + "a", cat, MASK_NONE, 0.0, None)
            self.same(f"bwd {u} = {cat}[:{c}] (gradient)", s.grad(u), s.grad(cat)[..., :c])
            x, du = s.act(src_name), s.grad(u)
            A = convT_abs_sums(x, self.kq(u), du)
            d = du.reshape(-1, c)
            dw = np.stack([np.stack([du[:, a::2, b::2].reshape(-1, c).T @ x.reshape(-1, x.shape[-1]) for b in range(2)]) for a in range(2)])
            self.chk(f"param {u}/kernel", s.pgrads[u + "/kernel"], dw, EPS_SPLIT * A["dw_a1"], stored=False, ops=[f"convT_wgrad:{u}"], param=u + "/kernel")
            self.chk(f"param {u}/bias", s.pgrads[u + "/bias"], d.sum(0), EPS_SPLIT * A["db_a1"], stored=False, ops=[f"convT_wgrad:{u}"], param=u + "/bias")
        self.ran.setdefault("bookkeeping", set()).update(["zero_sums", "zero_bwd_sums"])          # (memsets of the sums the links above read back through their results)

    def grad_sum(self, t, stages, cat_off):
        """the gradient buffer of a tensor several launches write, followed in program order as an interval that is stored after every launch (module docstring)"""
        s = self.s
        lo = hi = None
        ops = []
        for i, stage in enumerate(stages):
            clo = chi = A = 0.0
            for tag in stage:
                if tag[0] == "pool":
                    pk = "p" + t[1]
                    v = route(s.grad(pk), s.act(t)); clo, chi, A = clo + v, chi + v, A + np.abs(v)
                    ops.append(f"pool_bwd:{pk}")
                elif tag[0] == "skip":
                    off = cat_off[(tag[1], t)]
                    v = s.grad("cat_" + tag[1])[..., off:off + O.PP_WIDTH[t]]; clo, chi, A = clo + v, chi + v, A + np.abs(v)
                else:
                    u = "u" + tag[1][1:]
                    du, kq = s.grad(u), self.kq(u)
                    d = sum(du[:, a::2, b::2] @ kq[a, b] for a in range(2) for b in range(2))          # dx[i,j,c] = sum_{a,b,o} dU[2i+a,2j+b,o] K[a,b,o,c]
                    e = EPS_SPLIT * convT_abs_sums(s.act(t), kq, du)["dx_a1"]
                    if lo is None and len(stage) == 1 and len(stages) == 1:
                        clo, chi, A = clo + d - e, chi + d + e, A + np.abs(d) + e           # the only launch: the staging tensor is copied, its rounding is the buffer's
                    else:
                        clo, chi, A = clo + self.st_lo(d - e), chi + self.st_hi(d + e), A + np.abs(d) + e           # (through the bf16 staging tensor)
                    ops.append(f"convT_dgrad:{u}")
            if stage[0][0] == "skip":
                ops.append("accum_slice:" + "+".join(tg[1] for tg in stage) + ">" + t)
            if lo is not None:
                A = A + np.maximum(np.abs(lo), np.abs(hi))
            slack = (len(stage) + 1) * U * A
            lo_pre = (0.0 if lo is None else lo) + clo - slack
            hi_pre = (0.0 if hi is None else hi) + chi + slack
            if i + 1 < len(stages):
                lo, hi = self.st_lo(lo_pre), self.st_hi(hi_pre)
        self.chk(f"bwd sum >{t}: " + " | ".join("+".join(":".join(tg) for tg in st) for st in stages), s.grad(t), 0.5 * (lo_pre + hi_pre), 0.5 * (hi_pre - lo_pre), ops=ops)

    def seg_head(self):
        """head_fwd: p, the loss pair on the engine's own p; head_bwd: grad[x1_4], out/kernel, out/bias (test_gpu_storage_ops.head_check; the engine's loss sums carry
        (n1 + 12) u each, which moves the Dice coefficients A, B of dz by 3 (n1 + 12) u: added to k = 10 on their term)"""
        x = self.s.act("x1_4")
        n, h, w, cin = x.shape
        pixels = n * h * w
        k, b = self.s.w["out/kernel"].reshape(cin), float(self.s.w["out/bias"][0])
        x2 = x.reshape(-1, cin)
        z = x2 @ k + b
        pr = 1.0 / (1.0 + np.exp(-z))
        az = np.abs(x2) @ np.abs(k) + abs(b)
        bp = U * (pr * (1 - pr) * (6 + np.log2(cin // 4)) * az + 8 * pr)
        pg = self.s.p.reshape(-1)
        self.chk("fwd head p", pg, pr, bp, stored=False, ops=["head_fwd"])
        t = self.s.y.reshape(-1)
        pc = np.clip(pg, LO32, HI32)
        zl = np.log(pc / (1.0 - pc))
        l = np.maximum(zl, 0.0) - zl * t + np.log1p(np.exp(-np.abs(zl)))
        it = cdiv(pixels, max(1, min(cdiv(pixels, TPB * 2), HEAD_LPP_BLOCKS)) * TPB)
        I, St, Sp = (t * pg).sum(), t.sum(), pg.sum()
        dice = (2 * I + 1) / (St + Sp + 1)
        e_sum = (it + 12) * U
        loss = 0.5 * l.mean() + 0.5 * (1 - dice)
        e_l = 0.5 * (e_sum * l.mean() + 8 * U * (np.abs(zl) + 1).mean()) + 0.5 * 3 * e_sum * dice + 2 * U * abs(loss)
        self.chk("fwd loss, dice_coeff", self.s.loss[:2], np.array([loss, dice]), np.array([e_l, 3 * e_sum * dice + 2 * U * dice]), stored=False, ops=["head_fwd", "loss_finalize"])
        cb, A_, B_ = LF.coefs("bce_dice_loss", t, pg, 0.5, 0.5)
        inr = (pg >= LO32) & (pg <= HI32)
        q = pg * (1 - pg)
        dz = np.where(inr, cb * (pc - t), 0.0) + q * (A_ * t + B_)
        DA = np.where(inr, np.abs(cb * (pg - t)), 0.0) + q * (np.abs(A_ * t) + abs(B_))
        DS = q * (np.abs(A_ * t) + abs(B_)) * 3 * e_sum                                  # the engine's own loss sums in A, B
        ref = dz[:, None] * k[None, :]
        tol = (10 * U * DA + DS)[:, None] * np.abs(k)[None, :]
        self.chk("bwd head >x1_4", self.s.grad("x1_4").reshape(-1, cin), ref, tol, ops=["head_bwd"])
        lpp = cin // 4
        gridb = min(max(1, min(cdiv(pixels * lpp // 4, TPB), MAX_BLOCKS)), HEAD_BWD_BLOCKS)
        red = cdiv(pixels, gridb * TPB // lpp) + 6 + 4 + gridb + 1
        self.chk("param out/kernel", self.s.pgrads["out/kernel"].reshape(cin), dz @ x2, U * (10 * (DA @ np.abs(x2)) + red * (np.abs(dz) @ np.abs(x2))) + DS @ np.abs(x2),
                 stored=False, ops=["head_bwd"], param="out/kernel")
        self.chk("param out/bias", self.s.pgrads["out/bias"].reshape(1), np.array([dz.sum()]), np.array([U * (10 * DA.sum() + red * np.abs(dz).sum()) + DS.sum()]),
                 stored=False, ops=["head_bwd"], param="out/bias")

    # ---- classifier ---------------------------------------------------------------------------------------------------------------------------
    def run_classifier(self):
        s = self.s
        for k in (1, 2, 3):
            ca, cb, ba, bb, pk = f"c{k}a", f"c{k}b", f"bn{k}a", f"bn{k}b", f"p{k}"
            self.conv_fwd(ca, "" if k == 1 else f"p{k - 1}", RELU, 0.0)
            if cb in s.folded:
                self.conv_fwd_folded(cb, ca, ba, RELU, 0.0)
            else:
                self.bn_fwd(ba, ca, ba)
                self.conv_fwd(cb, ba, RELU, 0.0)
            self.bn_fwd(bb, cb, bb, pool=pk)
        self.cls_tail_fwd()
        self.cls_tail_bwd()
        for k in (3, 2, 1):
            ca, cb, ba, bb, pk = f"c{k}a", f"c{k}b", f"bn{k}a", f"bn{k}b", f"p{k}"
            if s.fused_tail:
                self.cls_fused_tail(k)
            else:
                self.chk(f"bwd pool {pk}>{bb}", s.grad(bb), route(s.grad(pk), s.act(bb)), 0.0, ops=[f"pool_bwd:{pk}"])
                self.bn_bwd(bb, bb, cb, MASK_RELU, 0.0, None)
            if cb in s.folded:
                self.folded_wgrad(cb, ca, ba)
                self.folded_dgrad(cb, ca, ba, MASK_RELU, 0.0, None)
            else:
                self.conv_wgrad(cb, ba)
                self.conv_dgrad(cb, ba, MASK_NONE, 0.0, None)
                self.bn_bwd(ba, ba, ca, MASK_RELU, 0.0, None)
            self.conv_wgrad(ca, "" if k == 1 else f"p{k - 1}")
            if k > 1:
                self.conv_dgrad(ca, f"p{k - 1}", MASK_NONE, 0.0, None)
        self.ran.setdefault("bookkeeping", set()).update(["zero_sums", "zero_bwd_sums"])

    def cls_tail_fwd(self):
        s = self.s
        p3 = s.act("p3")
        n = p3.shape[0]
        flat = p3.reshape(n, -1)                                              # channels_last Flatten: (i W + j) C + c
        w1, b1 = s.w["fc1/kernel"], s.w["fc1/bias"]
        rate = O.CLS_DROP if s.drop_seed is not None else 0.0
        seed = (s.drop_seed + FC_SEED) & M64 if rate else 0
        if s.dt == "bf16":
            z = flat @ w1 + b1
            ks = PX.keep_scale_dense(z.shape, rate, seed).astype(f64) if rate else np.ones(z.shape)
            ref, tol = np.maximum(z, 0.0) * ks, EPS_SPLIT * (np.abs(flat) @ np.abs(w1) + np.abs(b1)) * ks
        else:
            ref, tol, _ = T.dense_fwd_ref(flat, w1, b1, 1, rate, seed)
            ks = PX.keep_scale_dense(ref.shape, rate, seed).astype(f64) if rate else np.ones(ref.shape)
        h1 = s.act("h1").reshape(n, -1)
        self.chk("fwd fc1 >h1", h1, ref, tol, stored=False, ops=["dense_fwd:fc1"])
        self.zeros_agree("fwd fc1 >h1", h1, ks if rate else None, ref, tol)
        w2, b2 = s.w["fc2/kernel"].reshape(-1), s.w["fc2/bias"]
        p, tp = T.head_fwd_ref(h1, w2, b2)
        pg = s.p.reshape(-1)
        self.chk("fwd fc2 >p", pg, p, tp, stored=False, ops=["cls_head_fwd"])
        sums, tsum = T.head_sums_ref(pg, s.y.reshape(-1), s.cw[0], s.cw[1])
        ref, tl = T.finalize_ref(sums, float(n))
        tl = tl + np.array([tsum[0] / n, 0.0])
        self.chk("fwd loss, f1", s.loss[:2], ref, tl, stored=False, ops=["cls_head_fwd", "loss_finalize"])

    def cls_tail_bwd(self):
        s = self.s
        p3 = s.act("p3")
        n = p3.shape[0]
        flat = p3.reshape(n, -1)
        h1 = s.act("h1").reshape(n, -1)
        rate = O.CLS_DROP if s.drop_seed is not None else 0.0
        ref, tol = T.head_bwd_ref(h1, s.w["fc2/kernel"].reshape(-1), s.p.reshape(-1), s.y.reshape(-1), s.cw[0], s.cw[1], float(n), rate)
        dh = s.grad("h1").reshape(n, -1)
        self.chk("bwd head >h1", dh, ref["dh"], tol["dh"], stored=False, ops=["cls_head_bwd"])
        for key, pn in (("dw", "fc2/kernel"), ("db", "fc2/bias"), ("db1", "fc1/bias")):
            self.chk(f"param {pn}", s.pgrads[pn].reshape(ref[key].shape), ref[key], tol[key], stored=False, ops=["cls_head_bwd"], param=pn)
        w1 = s.w["fc1/kernel"]
        if s.dt == "bf16":
            tdx, tdw = EPS_SPLIT * (np.abs(dh) @ np.abs(w1).T), EPS_SPLIT * (np.abs(flat).T @ np.abs(dh))
            rdx, rdw = dh @ w1.T, flat.T @ dh
        else:
            rdx, tdx, rdw, tdw = T.dense_bwd_ref(flat, w1, dh)
        self.chk("bwd fc1 >p3", s.grad("p3").reshape(n, -1), rdx, tdx, ops=["dense_bwd:fc1"])
        self.chk("param fc1/kernel", s.pgrads["fc1/kernel"], rdw, tdw, stored=False, ops=["dense_bwd:fc1"], param="fc1/kernel")

    def cls_fused_tail(self, k):
        """pool_bwd_sums + bn_maxpool_bwd_apply (test_gpu_storage_ops.test_pool_bwd_bnstats_sums_and_apply): sums (sum g, sum g (p - beta) / gamma) over the POOLED
        tensors, then dx = [x > 0] scale (t - k1 - xhat k2), t = the pooled gradient routed to the first maximum of y = fma(x, scale, shift)"""
        s = self.s
        cb, bb, pk = f"c{k}b", f"bn{k}b", f"p{k}"
        x, g, pv = s.act(cb), s.grad(pk), s.act(pk)
        P = self.bn_params(bb, x)
        n, h, w, c = x.shape
        pixels = n * h * w
        ig = (np.float32(1.0) / P["gamma"].astype(np.float32)).astype(f64)
        u2 = g * (pv - P["beta"]) * ig
        total = n * (h // 2) * (w // 2) * (c // 4)
        grid2 = max(1, min(cdiv(total, TPB * 4), BN_STATS_BLOCKS))
        nt2 = cdiv(total, grid2 * TPB) + TPB // (c // 4)
        s1, s2 = g.reshape(-1, c).sum(0), u2.reshape(-1, c).sum(0)
        e1 = (nt2 + 3) * U * np.abs(g).reshape(-1, c).sum(0)
        e2 = (nt2 + 6) * U * (np.abs(g) * (np.abs(pv) + np.abs(P["beta"])) * np.abs(ig)).reshape(-1, c).sum(0)
        ops = [f"pool_bwd_sums:{pk}", f"bn_pool_bwd_apply:{bb}"]
        self.chk(f"param {bb}/beta (pooled sums)", s.pgrads[bb + "/beta"], s1, e1 + U * np.abs(s1), stored=False, ops=ops, param=bb + "/beta")
        self.chk(f"param {bb}/gamma (pooled sums)", s.pgrads[bb + "/gamma"], s2, e2 + U * np.abs(s2), stored=False, ops=ops, param=bb + "/gamma")
        y = x * P["sc"] + P["sh"]
        t = route(g, y)
        xh = (x - P["mean"]) * P["istd"]
        d_xh = P["istd"] * P["d_mean"] + np.abs(x - P["mean"]) * P["d_istd"]
        k1, k2 = s1 / pixels, s2 / pixels
        D = t - k1 - xh * k2
        ref = np.where(x > 0, P["sc"] * D, 0.0)
        A = np.abs(P["sc"]) * (np.abs(t) + np.abs(k1) + np.abs(xh * k2))
        tol = 8 * U * A + (x > 0) * (np.abs(P["sc"]) * (e1 / pixels + np.abs(xh) * e2 / pixels + np.abs(k2) * d_xh) + np.abs(D) * P["d_sc"])
        self.chk(f"bwd fused tail {pk}>{cb}", s.grad(cb), ref, tol, ops=ops)

    # ---- entry --------------------------------------------------------------------------------------------------------------------------------
    def run(self):
        (self.run_unetpp if self.s.arch == "unetpp" else self.run_classifier)()
        return self

    def assert_complete(self):
        """every op of the two programs belongs to a link that ran; every parameter gradient was checked"""
        covered = set().union(*self.ran.values())
        missing = [o for o in (self.s.ops or []) if o not in covered]
        assert not missing, f"ops of the programs that no link covers: {missing}"
        left = sorted(set(self.s.pgrads) - self.params)
        assert not left, f"parameter gradients that no link checked: {left}"

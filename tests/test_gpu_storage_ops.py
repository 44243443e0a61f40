"""-m gpu: the storage-templated BatchNorm, pooling / dropout, head and slice entries (kernels_pointwise.hip), each in its fp32 and its bf16 instance, against
float64 references per ELEMENT, at the channel counts, strides, pixel counts and modes where the kernels branch.

Inputs are bf16-exact in both dtypes (rounded once, to nearest even, by torch's CPU .bfloat16()), so the two instances see the same values; parameters (BatchNorm
scale / shift / mean / istd, the head's weights, labels, weight map) are fp32 and the references use exactly those fp32 values.  References: float64, from
oracle/unet_oracle.py (batchnorm, maxpool2x2, conv1x1_sigmoid, bce_dice_loss) and tests/loss_family_oracle.py, gradients by torch autograd; the keep masks from
tests/philox_ref.py.

Bounds (u = 2^-24, the fp32 unit round-off).  A kernel evaluates an expression in fp32; every fp32 operation rounds once with an error <= u times the magnitude of
its result, and every intermediate magnitude is <= A, the sum of the magnitudes of the expression's terms, derived per op in its test.  So the fp32 value v carries
|v - ref64| <= k u A, k = the number of roundings on the longest chain (plus a margin of 1-2).  Then
  * an fp32-stored output must satisfy |got - ref64| <= k u A per element;
  * a bf16-stored output must equal RNE_bf16(ref64) per element, except that where ref64 lies within k u A of a bf16 rounding midpoint either neighbour is
    accepted: the check is RNE_bf16(ref64 - k u A) <= got <= RNE_bf16(ref64 + k u A).  Each bf16 check also asserts that a copy of the reference truncated
    to bf16 (low bits dropped) FAILS it on a clear share (> 20 %) of the elements the store has to round: a store that truncates cannot pass;
  * an fp32 reduction of n terms in sequence carries <= (n - 1) u sum|terms|: the statistics kernels sum at most n1 terms per thread (grid-stride loop; n1 from
    the launch geometry, mirrored below), then a tree of at most T partials in the workgroup, then fp64 atomics / an fp64 fold (< 2^-40 relative, inside the
    margin).  Bound (n1 + T + k) u sum|terms|, with k the per-term roundings;
  * exact ops are bit-exact in both dtypes: max-pool forward without dropout (ties: the first of the four, row-major), pool backward routing, copy_slice, and
    the accumulating ops at rate 0, whose fp32 sums of bf16 values in a narrow exponent range are exact, so the bf16 result is ONE rounding of the float64 sum
    (the data is chosen so that rounding after every add differs on a share of elements, which the test asserts).
The largest ratio of the error to its bound is printed per check ("bound-ratio ..."; run with -s to see it); for a bf16 output it is the largest
|ref64 - midpoint| / (k u A) among the elements that needed the midpoint allowance.  Measured on an MI355X (both dtypes): per-element fp32 outputs 0.25-0.50
(bn_apply 0.50, bn_bwd_apply 0.40, pool outputs 0.48-0.50, head p 0.25, head dx 0.38); bf16 outputs <= 0.32, the allowance used by ~2e-5 of the
elements; reductions 5e-4 - 0.07 (the (n1 + T) u sum|terms| bound is a worst case; head dw 0.07, bn_stats sum x^2 0.04).
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_family_oracle as LF
import philox_ref as PX
from covidseg_amd import _lib
from gpu_util import U, check_store, check_sum, rne_bf16, trunc_bf16          # (the bf16 matrix-core op tests use the same checks)
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
DTYPES = ["fp32", "bf16"]
SENT = 7.0                                   # sentinel around an output slice (bf16-exact): must survive every launch unchanged
BAD_IN = 30720.0                              # sentinel around an input slice: a kernel that reads it leaves every bound far behind
BN_CS = [4, 16, 32, 48, 96, 256, 1024]       # 48, 96: 256 % (c/4) != 0 -> the generic (div/mod) paths of bn_apply / bn_bwd_apply; 1024: the widest bn_c_ok takes
SMALL = (2, 37, 53)                          # 3922 pixels: ragged, several workgroups at every channel count
POOL = (3, 10, 14)                           # pooled 5 x 7: odd Wo, odd Ho

# launch geometry of kernels_pointwise.hip (the per-thread term counts of the reduction bounds follow from it)
TPB, MAX_BLOCKS = 256, 2048
BN_STATS_BLOCKS, BN_BWD_STATS_BLOCKS, POOL_BWD_STATS_BLOCKS = 512, 1024, 768
HEAD_BLOCKS, HEAD_LPP_BLOCKS, HEAD_BWD_BLOCKS, SLOTS_DET = 8192, 2048, 1024, 1024


def cdiv(a, b):
    return -(-int(a) // int(b))


def grid_for(work):
    return max(1, min(cdiv(work, TPB), MAX_BLOCKS))


@pytest.fixture(scope="module")
def ops():
    from gpu_util import Ops
    return Ops()


class Ent:
    """the 17 storage-templated entries (+ the fp32 twins), called with this context / stream in dtype dt"""

    def __init__(self, ops, dt, handle=None):
        self.lib, self.h, self.s, self.bf = ops.lib, handle if handle is not None else ops.h, ops.s, dt == "bf16"

    def bn_stats(self, *a):
        return self.lib.unet_bn_stats_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_bn_stats(self.h, *a, self.s)

    def bn_stats_concat(self, *a):
        return self.lib.unet_bn_stats_concat_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_bn_stats_concat(self.h, *a, self.s)

    def bn_apply(self, *a):
        return self.lib.unet_bn_apply_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_bn_apply(self.h, *a, self.s)

    def bn_bwd_stats(self, *a):
        return self.lib.unet_bn_bwd_stats_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_bn_bwd_stats(self.h, *a, self.s)

    def bn_bwd_apply(self, *a):
        return self.lib.unet_bn_bwd_apply_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_bn_bwd_apply(self.h, *a, self.s)

    def pool_fwd(self, *a):
        return self.lib.unet_maxpool2x2_dropout_fwd_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_maxpool2x2_dropout_fwd(self.h, *a, self.s)

    def pool_bwd(self, *a):
        return self.lib.unet_maxpool2x2_dropout_bwd_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_maxpool2x2_dropout_bwd(self.h, *a, self.s)

    def bn_pool_fwd(self, *a):
        return self.lib.unet_bn_apply_maxpool_dropout_fwd_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_bn_apply_maxpool_dropout_fwd(self.h, *a, self.s)

    def pool_bwd_sums(self, *a):
        return self.lib.unet_maxpool2x2_dropout_bwd_sums_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_maxpool2x2_dropout_bwd_sums(self.h, *a, self.s)

    def pool_bwd_bnstats(self, *a):
        return self.lib.unet_maxpool2x2_dropout_bwd_bnstats_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_maxpool2x2_dropout_bwd_bnstats(self.h, *a, self.s)

    def bn_pool_bwd_apply(self, *a):
        return self.lib.unet_bn_maxpool_bwd_apply_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_bn_maxpool_bwd_apply(self.h, *a, self.s)

    def head_fwd(self, *a):
        return self.lib.unet_head_fwd_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_head_fwd(self.h, *a, self.s)

    def head_fwd_ex(self, *a):
        return self.lib.unet_head_fwd_bf16_ex(self.h, *a, self.s) if self.bf else self.lib.unet_head_fwd_ex(self.h, *a, self.s)

    def head_bwd(self, *a):
        return self.lib.unet_head_bwd_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_head_bwd(self.h, *a, self.s)

    def head_bwd_ex(self, *a):
        return self.lib.unet_head_bwd_bf16_ex(self.h, *a, self.s) if self.bf else self.lib.unet_head_bwd_ex(self.h, *a, self.s)

    def copy_slice(self, *a):
        return self.lib.unet_copy_slice_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_copy_slice(self.h, *a, self.s)

    def accum_slices(self, *a):
        return self.lib.unet_accum_slices_bf16(self.h, *a, self.s) if self.bf else self.lib.unet_accum_slices(self.h, *a, self.s)


_KEEP = []                                   # device inputs made inline for a call: alive until the launch has finished (the C ABI sees raw pointers only)


def ck(ops, rc, what, handle=None):
    if rc != 0:
        msg = ops.lib.unet_last_error(handle if handle is not None else ops.h)
        raise AssertionError(f"{what}: status {rc}: {msg.decode() if msg else '?'}")
    torch.cuda.synchronize()
    _KEEP.clear()


# ---- values, buffers ------------------------------------------------------------------------------------------------------------------------
def bfx(a):
    """round to bf16 (nearest even) once: the values both instances see, as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def dev(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    t = (t.bfloat16() if dt == "bf16" else t).cuda()
    _KEEP.append(t)
    return t


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def wide(a, ld, off, dt, fill):
    """a [..., c] inside a [..., ld] buffer at channel offset off, every other channel = fill"""
    b = np.full(a.shape[:-1] + (ld,), fill, np.float32)
    b[..., off:off + a.shape[-1]] = a
    return dev(b, dt)


def sentinels_kept(buf, off, c, what):
    b = host(buf)
    outside = np.concatenate([b[..., :off].ravel(), b[..., off + c:].ravel()])
    assert (outside == SENT).all(), f"{what}: {np.count_nonzero(outside != SENT)} sentinel elements around the output slice were overwritten"


def d64(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    _KEEP.append(t)
    return t


def windows(a):
    """(n, h, w, c) -> (4, n, h/2, w/2, c) in argmax4's order: (0,0) (0,1) (1,0) (1,1)"""
    return np.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]])


def unwindows(v):
    n, ho, wo, c = v.shape[1:]
    out = np.zeros((n, 2 * ho, 2 * wo, c), v.dtype)
    out[:, 0::2, 0::2], out[:, 0::2, 1::2], out[:, 1::2, 0::2], out[:, 1::2, 1::2] = v[0], v[1], v[2], v[3]
    return out


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------------------
def bn_inputs(rng, shape, c):
    x = bfx(rng.standard_normal(shape + (c,)) * rng.uniform(0.3, 3.0, c) + rng.uniform(-1.0, 1.0, c))
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32); beta = (rng.standard_normal(c) * 0.5).astype(np.float32)
    return x, gamma, beta


def bn_params(x, gamma, beta):
    """bnp = [scale C][shift C][mean C][istd C] (fp32) of the batch statistics of x, from the oracle's training-mode batchnorm"""
    _, mu, va = O.batchnorm(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), None, None, True)
    mu, va = mu.numpy(), va.numpy()
    istd = 1.0 / np.sqrt(va + O.BN_EPS); sc = gamma * istd; sh = beta - mu * sc
    return np.concatenate([sc, sh, mu, istd]).astype(np.float32)


def stats_terms(pixels, c, cap):
    """n1 + T of bn_stats_kernel: terms per thread of the grid-stride loop + the workgroup's partials"""
    ppb = TPB // (c // 4)
    grid = max(1, min(cdiv(pixels, ppb * 16), cap))
    return cdiv(pixels, grid * ppb) + ppb


def bn_stats_checks(E, ops, dt, x, c, pixels, what, handle=None, ldx_extra=8):
    """bn_stats of x (placed in the upper slice of a wider buffer, BAD_IN below it) against float64 sums; returns the sums"""
    ldx = c + ldx_extra
    xd = wide(x, ldx, ldx_extra, dt, BAD_IN)
    sums = ops.z(2 * c, dtype=torch.float64)
    ck(ops, E.bn_stats(ptr(xd, ldx_extra), ldx, sums.data_ptr(), pixels, c), what, handle)
    x64 = x.reshape(-1, c).astype(np.float64)
    n = stats_terms(pixels, c, BN_STATS_BLOCKS)
    got = sums.cpu().numpy()
    check_sum(got[:c], x64.sum(0), (n + 2) * U * np.abs(x64).sum(0), what + " sum x", dt)
    check_sum(got[c:], (x64 * x64).sum(0), (n + 3) * U * (x64 * x64).sum(0), what + " sum x^2", dt)
    return got


@pytest.mark.parametrize("c", BN_CS)
@pytest.mark.parametrize("dt", DTYPES)
def test_bn_stats_concat_and_apply(ops, dt, c):
    """bn_stats: per-channel (sum x, sum x^2), bound (n1 + T + 2) u sum|x| and (n1 + T + 3) u sum x^2 (the square is one more rounding).
    bn_stats_concat: the measured up half as bn_stats; the analytic skip half  pixels beta,  pixels (gamma^2 var / (var + eps) + beta^2)  is fp64 arithmetic of
    ~8 operations: 16 * 2^-53 relative.
    bn_apply: y = fma(x, scale, shift), one fp32 rounding: A = |x scale| + |shift|, k = 2; the output in the middle of a wider buffer, sentinels around it."""
    rng = np.random.default_rng(c)
    n, h, w = SMALL
    pixels = n * h * w
    x, gamma, beta = bn_inputs(rng, SMALL, c)
    E = Ent(ops, dt)
    bn_stats_checks(E, ops, dt, x, c, pixels, "bn_stats")
    # concat: up half measured, skip half from the source layer's statistics
    cs = 12
    src_mean = rng.standard_normal(cs); src_var = rng.uniform(0.2, 3.0, cs); src_count = 5000.0
    src = np.concatenate([src_mean * src_count, (src_var + src_mean ** 2) * src_count])
    sg = rng.uniform(0.5, 1.5, cs).astype(np.float32); sb = rng.standard_normal(cs).astype(np.float32)
    ldx = c + 8
    xd = wide(x, ldx, 8, dt, BAD_IN)
    sums = ops.z(2 * (c + cs), dtype=torch.float64)
    ck(ops, E.bn_stats_concat(ptr(xd, 8), ldx, d64(src).data_ptr(), src_count, ops.d(sg).data_ptr(), ops.d(sb).data_ptr(), sums.data_ptr(), pixels, c, cs), "bn_stats_concat")
    got = sums.cpu().numpy()
    x64 = x.reshape(-1, c).astype(np.float64)
    nt = stats_terms(pixels, c, BN_STATS_BLOCKS)
    check_sum(got[:c], x64.sum(0), (nt + 2) * U * np.abs(x64).sum(0), "bn_stats_concat up sum", dt)
    check_sum(got[c + cs:2 * c + cs], (x64 * x64).sum(0), (nt + 3) * U * (x64 * x64).sum(0), "bn_stats_concat up sum^2", dt)
    mean = src[:cs] / src_count; var = np.maximum(src[cs:] / src_count - mean ** 2, 0.0)
    g64, b64 = sg.astype(np.float64), sb.astype(np.float64)
    want1, want2 = pixels * b64, pixels * (g64 * g64 * var / (var + np.float32(O.BN_EPS).astype(np.float64)) + b64 * b64)
    check_sum(got[c:c + cs], want1, 16 * 2.0 ** -53 * np.abs(want1), "bn_stats_concat skip sum", dt)
    check_sum(got[2 * c + cs:], want2, 16 * 2.0 ** -53 * (np.abs(want2) + pixels * src[cs:] / src_count * g64 * g64 / var.min()), "bn_stats_concat skip sum^2", dt)
    # apply, inside a wider output buffer
    bnp = bn_params(x, gamma, beta)
    sc, sh = bnp[:c].astype(np.float64), bnp[c:2 * c].astype(np.float64)
    ldy, off = c + 12, 4
    y = wide(np.zeros(SMALL + (c,), np.float32), ldy, off, dt, SENT)
    ck(ops, E.bn_apply(ptr(xd, 8), ldx, ops.d(bnp).data_ptr(), ptr(y, off), ldy, pixels, c), "bn_apply")
    sentinels_kept(y, off, c, "bn_apply")
    xb = host(xd)
    assert (xb[..., :8] == BAD_IN).all() and np.array_equal(xb[..., 8:], x.astype(np.float64)), "an input buffer changed"
    ref = x.astype(np.float64) * sc + sh
    check_store(host(y)[..., off:off + c], ref, np.abs(x * sc) + np.abs(sh), 2, dt, "bn_apply")
    # the same affine map as the oracle's batchnorm (float64 scale / shift): only the fp32 rounding of the parameters apart
    yo = O.batchnorm(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), None, None, True)[0].numpy()
    assert np.abs(ref - yo).max() <= 4 * U * (np.abs(x * sc) + np.abs(sh)).max()


def mask_ref(mode, x, rate, ks):
    """mask_factor of the producer of x (common.h) in float64, and the magnitude its fp32 evaluation rounds against"""
    if mode == 0:
        return np.ones_like(x), np.zeros_like(x)
    if mode == 1:
        return (x > 0).astype(np.float64), np.zeros_like(x)
    if mode == 2:
        return np.where(x > 0, 1.0, x + 1.0), np.where(x > 0, 0.0, np.abs(x) + 1.0)
    a = x * float(np.float32(1.0) - np.float32(rate))
    return ks * np.where(a > 0, 1.0, a + 1.0), ks * (2 * np.abs(a) + 1.0)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("c", BN_CS)
@pytest.mark.parametrize("dt", DTYPES)
def test_bn_bwd_stats_and_apply(ops, dt, c, mode):
    """bn_bwd_stats: (sum dy, sum dy (x - mean) istd) with the fp32 mean / istd of bnp: per term 3 roundings -> (n1 + T + 5) u sum|dy xhat|.
    bn_bwd_apply: dx = scale (dy - k1 - (x - mean) istd k2) m(x), k1 / k2 = sums / count rounded to fp32, m the producer's derivative (mask modes 0-3; MASK_ELU_DROP
    with its keep factor from the Philox stream, quad index p * c/4 + q over the dense x).  A = |scale| ((|dy| + |k1| + |xhat k2|) (|m| + M) ) with M the
    magnitude m's own evaluation rounds against (ELU: |x| + 1; ELU + dropout: ks (2 |a| + 1), a = x (1 - rate)); chain of <= 7 roundings, k = 8.
    The closed form is checked against torch autograd of the oracle's batchnorm (float64 parameters) first."""
    rng = np.random.default_rng(100 * c + mode)
    n, h, w = SMALL
    pixels = n * h * w
    x, gamma, beta = bn_inputs(rng, SMALL, c)
    dy = bfx(rng.standard_normal(SMALL + (c,)))
    bnp = bn_params(x, gamma, beta)
    sc, mean, istd = (bnp[i * c:(i + 1) * c].astype(np.float64) for i in (0, 2, 3))
    E = Ent(ops, dt)
    ldx = c if mode == 3 else c + 8                                       # (MASK_ELU_DROP reads a dense x)
    xoff = ldx - c
    xd = wide(x, ldx, xoff, dt, BAD_IN); dyd = wide(dy, c + 4, 4, dt, BAD_IN)
    sums = ops.z(2 * c, dtype=torch.float64)
    ck(ops, E.bn_bwd_stats(ptr(dyd, 4), c + 4, ptr(xd, xoff), ldx, ops.d(bnp).data_ptr(), sums.data_ptr(), pixels, c), "bn_bwd_stats")
    g64, x64 = dy.astype(np.float64), x.astype(np.float64)
    xh = (x64 - mean) * istd
    s1, s2 = g64.reshape(-1, c).sum(0), (g64 * xh).reshape(-1, c).sum(0)
    nt = cdiv(pixels, max(1, min(cdiv(pixels, (TPB // (c // 4)) * 16), BN_BWD_STATS_BLOCKS)) * (TPB // (c // 4))) + TPB // (c // 4)
    got = sums.cpu().numpy()
    check_sum(got[:c], s1, (nt + 2) * U * np.abs(g64).reshape(-1, c).sum(0), "bn_bwd_stats sum dy", dt)
    check_sum(got[c:], s2, (nt + 5) * U * np.abs(g64 * xh).reshape(-1, c).sum(0), "bn_bwd_stats sum dy xhat", dt)
    rate, seed = (0.25, 4242 + c) if mode == 3 else (0.0, 0)
    ks = PX.keep_scale_dense(x.shape, rate, seed).astype(np.float64) if mode == 3 else np.ones_like(x64)
    k1, k2 = s1 / pixels, s2 / pixels
    mf, mA = mask_ref(mode, x64, rate, ks)
    D = g64 - k1 - xh * k2
    ref = sc * D * mf
    A = np.abs(sc) * (np.abs(g64) + np.abs(k1) + np.abs(xh * k2)) * (np.abs(mf) + mA)
    lddx, off = c + 8, 4
    dx = wide(np.zeros_like(x), lddx, off, dt, SENT)
    ck(ops, E.bn_bwd_apply(ptr(dyd, 4), c + 4, ptr(xd, xoff), ldx, ops.d(bnp).data_ptr(), d64(np.concatenate([s1, s2])).data_ptr(), float(pixels), mode, rate, seed,
                           ptr(dx, off), lddx, pixels, c), "bn_bwd_apply")
    sentinels_kept(dx, off, c, "bn_bwd_apply")
    got = host(dx)[..., off:off + c]
    check_store(got, ref, A, 8, dt, f"bn_bwd_apply mode {mode}")
    if mode == 3:                                   # the keep pattern: exactly the elements the restated stream drops are zero
        assert np.array_equal(got == 0, ks == 0), "bn_bwd_apply MASK_ELU_DROP: keep pattern differs from philox_ref"
        assert 0.7 < (ks != 0).mean() < 0.8
    if mode == 0 and c <= 96:                       # the closed form is the oracle's batchnorm backward
        xt = torch.from_numpy(x64).requires_grad_(True)
        yt = O.batchnorm(xt, torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)), None, None, True)[0]
        yt.backward(torch.from_numpy(g64))
        _, mu, va = O.batchnorm(torch.from_numpy(x64), torch.ones(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64), None, None, True)
        is64 = 1.0 / np.sqrt(va.numpy() + O.BN_EPS); xh64 = (x64 - mu.numpy()) * is64
        cf = gamma * is64 * (g64 - g64.reshape(-1, c).mean(0) - xh64 * (g64 * xh64).reshape(-1, c).mean(0))
        assert np.abs(cf - xt.grad.numpy()).max() <= 1e-9 * np.abs(xt.grad.numpy()).max()


# ---- pooling / dropout -----------------------------------------------------------------------------------------------------------------------
def pool_x(rng, shape, c):
    """bf16 values from a small set (many ties inside a window), no zeros (a dropped element is then the only zero)"""
    base = bfx(rng.uniform(0.5, 2.0, (3, c)))                              # three magnitudes per channel
    mag = np.take_along_axis(base, rng.integers(0, 3, (int(np.prod(shape)), c)), 0).reshape(shape + (c,))
    return bfx(mag * rng.choice([-1.0, 1.0], shape + (c,), p=[0.2, 0.8]))


def narrow(rng, shape):
    """bf16 values with exponents in [-3, 3]: sums of up to 5 of them are exact in fp32, and rarely bf16-exact"""
    return bfx(rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(-3, 4, shape)) * rng.choice([-1.0, 1.0], shape))


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("c", [4, 48, 64])
@pytest.mark.parametrize("dt", DTYPES)
def test_maxpool_dropout_fwd_bwd(ops, dt, c, rate):
    """max-pool forward: the oracle's maxpool2x2, times the restated keep factor; at rate 0 bit-exact (ties: the first element wins, which the backward shows),
    at 0.25 one fp32 product: A = |max ks|, k = 2, and exactly the restated elements are zero.  Backward, accumulate 0: the routed dy ks, exact at rate 0;
    accumulate 1: old + routed, one rounding of the float64 sum at rate 0 (the fp32 sum is exact), A = |dy ks| + |old + dy ks|, k = 2 at 0.25.
    Input in the upper slice of ldx = c + 8, output gradient inside lddx = c + 12 with sentinels."""
    rng = np.random.default_rng(c + int(rate * 100))
    n, h, w = POOL
    ho, wo = h // 2, w // 2
    x = pool_x(rng, POOL, c)
    seed = 777 + c
    E = Ent(ops, dt)
    ldx = c + 8
    xd = wide(x, ldx, 8, dt, BAD_IN)
    y = ops.z(n, ho, wo, c, dtype=torch.bfloat16 if dt == "bf16" else torch.float32)
    ck(ops, E.pool_fwd(ptr(xd, 8), ldx, y.data_ptr(), n, h, w, c, rate, seed), "maxpool fwd")
    mx = O.maxpool2x2(torch.from_numpy(x.astype(np.float64))).numpy()
    ks = PX.keep_scale_dense((n, ho, wo, c), rate, seed).astype(np.float64) if rate else np.ones_like(mx)
    got = host(y)
    if rate == 0:
        assert np.array_equal(got, mx), "maxpool fwd: not the exact maximum"
    else:
        check_store(got, mx * ks, np.abs(mx * ks), 2, dt, "maxpool fwd dropout")
        assert np.array_equal(got == 0, ks == 0), "maxpool fwd: keep pattern differs from philox_ref"
    # backward
    dyp = narrow(rng, (n, ho, wo, c))
    win = windows(x.astype(np.float64))
    arg = np.argmax(win, 0)                                               # first maximum
    assert (np.sum(win == win.max(0), 0) > 1).mean() > 0.2, "the data must have ties"
    g = dyp.astype(np.float64) * ks
    routed = unwindows(np.stack([np.where(arg == k, g, 0.0) for k in range(4)]))
    lddx, off = c + 12, 4
    for acc in (0, 1):
        old = narrow(rng, POOL + (c,)) if acc else np.full(POOL + (c,), 5.0, np.float32)
        dx = wide(old, lddx, off, dt, SENT)
        ck(ops, E.pool_bwd(ptr(xd, 8), ldx, dev(dyp, dt).data_ptr(), ptr(dx, off), lddx, n, h, w, c, rate, seed, acc), f"maxpool bwd acc={acc}")
        sentinels_kept(dx, off, c, "maxpool bwd")
        got = host(dx)[..., off:off + c]
        want = routed + (old.astype(np.float64) if acc else 0.0)
        if rate == 0 and acc == 0:
            assert np.array_equal(got, want), "maxpool bwd: routing not exact"
        elif rate == 0:
            assert np.array_equal(got, want if dt == "fp32" else rne_bf16(want)), "maxpool bwd accumulate: not one rounding of the float64 sum"
            if dt == "bf16":
                assert (rne_bf16(want) != want).mean() > 0.1            # (3 of 4 elements are the old value: nothing to round there)
        else:
            check_store(got, want, np.abs(routed) + np.abs(want), 2, dt, f"maxpool bwd dropout acc={acc}")
            kept = unwindows(np.stack([np.where(arg == k, ks, 1.0) for k in range(4)]))
            assert ((got - (old if acc else 0.0)) [kept == 0] == 0).all()


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("c", [4, 48, 64])
@pytest.mark.parametrize("dt", DTYPES)
def test_bn_apply_maxpool_dropout_fwd(ops, dt, c, rate):
    """y = fma(x, scale, shift) into the skip slice (ldy = 2c + 4, sentinels) and pooled = max(y) ks: A = |x scale| + |shift| (y), max over the window of
    that times ks (pooled), k = 3.  A dropped element is stored as -0.0, a kept one never is (MASK_POOL_SUMS reads the keep mask off the sign)."""
    rng = np.random.default_rng(3 * c + int(rate * 100))
    n, h, w = POOL
    ho, wo = h // 2, w // 2
    x, gamma, beta = bn_inputs(rng, POOL, c)
    bnp = bn_params(x, gamma, beta)
    sc, sh = bnp[:c].astype(np.float64), bnp[c:2 * c].astype(np.float64)
    seed = 31 + c
    E = Ent(ops, dt)
    ldx, ldy, off = c + 4, 2 * c + 4, c
    xd = wide(x, ldx, 4, dt, BAD_IN)
    y = wide(np.zeros_like(x), ldy, off, dt, SENT)
    pooled = ops.z(n, ho, wo, c, dtype=torch.bfloat16 if dt == "bf16" else torch.float32)
    ck(ops, E.bn_pool_fwd(ptr(xd, 4), ldx, ops.d(bnp).data_ptr(), ptr(y, off), ldy, pooled.data_ptr(), n, h, w, c, rate, seed), "bn_apply_maxpool fwd")
    sentinels_kept(y, off, c, "bn_apply_maxpool fwd")
    yr = x.astype(np.float64) * sc + sh
    ay = np.abs(x * sc) + np.abs(sh)
    check_store(host(y)[..., off:off + c], yr, ay, 3, dt, "bn_apply_maxpool y")
    ks = PX.keep_scale_dense((n, ho, wo, c), rate, seed).astype(np.float64) if rate else np.ones((n, ho, wo, c))
    pr = O.maxpool2x2(torch.from_numpy(yr)).numpy() * ks
    got = host(pooled)
    check_store(got, pr, windows(ay).max(0) * ks, 3, dt, "bn_apply_maxpool pooled")
    neg0 = (got == 0) & np.signbit(got)
    assert np.array_equal(neg0, ks == 0), "bn_apply_maxpool: the -0.0 marks are not the restated dropped elements"


def pooled_bwd_case(rng, c, rate, seed):
    n, h, w = POOL
    x, gamma, beta = bn_inputs(rng, POOL, c)
    x = np.maximum(x, 0.0)                                                 # post-ReLU: the encoder tail
    bnp = bn_params(x, gamma, beta)
    dyp = bfx(rng.standard_normal((n, h // 2, w // 2, c)))
    ks = PX.keep_scale_dense(dyp.shape, rate, seed).astype(np.float64) if rate else np.ones(dyp.shape)
    return x, gamma, beta, bnp, dyp, ks


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("c", [4, 32, 64, 48])
@pytest.mark.parametrize("dt", DTYPES)
def test_pool_bwd_bnstats_sums_and_apply(ops, dt, c, rate):
    """The encoder tail's backward entries (they need 256 % (c/4) == 0: c = 48 is refused with UNET_E_ARG, not launched).
    maxpool2x2_dropout_bwd_bnstats: dx = old + routed(dy ks) (old = the skip gradient, in a slice of lddx = 2c, sentinels), sums (sum v, sum v (y - beta) / gamma)
    of the fp32 v: per term <= 5 roundings, 4 terms per loop iteration: (4 n1 + T + 6) u sum|v| (|y| + |beta|) / |gamma|.
    maxpool2x2_dropout_bwd_sums: (sum dy ks, sum dy ks (p (1 - rate) - beta) / gamma) over the pooled tensors: (n1 + T + 6) u sum of the term magnitudes.
    bn_maxpool_bwd_apply: y = fma(x, scale, shift) recomputed (arg-max over the fp32 y), t = g_skip + routed(dy ks), dx = x > 0 ? scale (t - k1 - xhat k2) : 0:
    A = |scale| (|g_skip| + |dy ks| + |k1| + |xhat k2|), k = 8."""
    rng = np.random.default_rng(7 * c + int(rate * 100))
    n, h, w = POOL
    ho, wo = h // 2, w // 2
    pixels = n * h * w
    seed = 5151 + c
    x, gamma, beta, bnp, dyp, ks = pooled_bwd_case(rng, c, rate, seed)
    sc, sh, mean, istd = (bnp[i * c:(i + 1) * c].astype(np.float64) for i in range(4))
    E = Ent(ops, dt)
    gd, bd = ops.d(gamma), ops.d(beta)
    # y = BN(x) as the forward stores it, in the skip slice of a concat
    yv = bfx(x.astype(np.float64) * sc + sh) if dt == "bf16" else (x.astype(np.float64) * sc + sh).astype(np.float32)
    skip = narrow(rng, POOL + (c,))
    ld = 2 * c
    sums = ops.z(2 * c, dtype=torch.float64)
    if c == 48:
        yd = wide(yv, ld, c, dt, BAD_IN); dx = wide(skip, ld, c, dt, SENT); xd = dev(x, dt)
        assert E.pool_bwd_bnstats(ptr(yd, c), ld, dev(dyp, dt).data_ptr(), ptr(dx, c), ld, gd.data_ptr(), bd.data_ptr(), sums.data_ptr(), n, h, w, c, rate, seed) == -1
        assert E.pool_bwd_sums(dev(dyp, dt).data_ptr(), dev(dyp, dt).data_ptr(), gd.data_ptr(), bd.data_ptr(), sums.data_ptr(), n, h, w, c, rate, seed) == -1
        assert E.bn_pool_bwd_apply(xd.data_ptr(), c, ops.d(bnp).data_ptr(), sums.data_ptr(), float(pixels), None, 0, dev(dyp, dt).data_ptr(), xd.data_ptr(), c,
                                   n, h, w, c, rate, seed) == -1
        torch.cuda.synchronize()
        assert (host(dx)[..., :c] == SENT).all() and np.array_equal(host(dx)[..., c:], skip)
        return
    y64 = yv.astype(np.float64)
    win = windows(y64)
    arg = np.argmax(win, 0)
    g = dyp.astype(np.float64) * ks
    routed = unwindows(np.stack([np.where(arg == k, g, 0.0) for k in range(4)]))
    # pool_bwd_bnstats
    yd = wide(yv, ld, c, dt, BAD_IN)
    dx = wide(skip, ld, c, dt, SENT)
    ck(ops, E.pool_bwd_bnstats(ptr(yd, c), ld, dev(dyp, dt).data_ptr(), ptr(dx, c), ld, gd.data_ptr(), bd.data_ptr(), sums.data_ptr(), n, h, w, c, rate, seed), "pool_bwd_bnstats")
    sentinels_kept(dx, c, c, "pool_bwd_bnstats")
    v = skip.astype(np.float64) + routed
    check_store(host(dx)[..., c:], v, np.abs(routed) + np.abs(v), 2, dt, "pool_bwd_bnstats dx")
    ig = (np.float32(1.0) / gamma).astype(np.float64)
    total = n * ho * wo * (c // 4)
    grid = max(1, min(cdiv(total, TPB), POOL_BWD_STATS_BLOCKS))
    nt = 4 * cdiv(total, grid * TPB) + TPB // (c // 4)
    got = sums.cpu().numpy()
    av = np.abs(v) + np.abs(routed)                                        # (v = old + fl(dy ks): two roundings)
    check_sum(got[:c], v.reshape(-1, c).sum(0), (nt + 3) * U * av.reshape(-1, c).sum(0), "pool_bwd_bnstats sum v", dt)
    t2 = v * (y64 - beta) * ig
    check_sum(got[c:], t2.reshape(-1, c).sum(0), (nt + 6) * U * (av * (np.abs(y64) + np.abs(beta)) * np.abs(ig)).reshape(-1, c).sum(0),
              "pool_bwd_bnstats sum v xhat", dt)
    # pool_bwd_sums over the pooled tensors (p as bn_apply_maxpool_dropout_fwd stores it)
    p = win.max(0) * ks
    pv = bfx(p) if dt == "bf16" else p.astype(np.float32)
    sums2 = ops.z(2 * c, dtype=torch.float64)
    ck(ops, E.pool_bwd_sums(dev(pv, dt).data_ptr(), dev(dyp, dt).data_ptr(), gd.data_ptr(), bd.data_ptr(), sums2.data_ptr(), n, h, w, c, rate, seed), "pool_bwd_sums")
    unkeep = float(np.float32(1.0) - np.float32(rate))
    pv64 = pv.astype(np.float64)
    u2 = g * (pv64 * unkeep - beta) * ig
    grid2 = max(1, min(cdiv(total, TPB * 4), BN_STATS_BLOCKS))
    nt2 = cdiv(total, grid2 * TPB) + TPB // (c // 4)
    got2 = sums2.cpu().numpy()
    check_sum(got2[:c], g.reshape(-1, c).sum(0), (nt2 + 3) * U * np.abs(g).reshape(-1, c).sum(0), "pool_bwd_sums sum g", dt)
    check_sum(got2[c:], u2.reshape(-1, c).sum(0), (nt2 + 6) * U * (np.abs(g) * (np.abs(pv64 * unkeep) + np.abs(beta)) * np.abs(ig)).reshape(-1, c).sum(0),
              "pool_bwd_sums sum g xhat", dt)
    # bn_maxpool_bwd_apply: t = g_skip + routed, the BatchNorm backward of the ReLU-masked encoder output
    x64 = x.astype(np.float64)
    yf = (x64 * sc + sh).astype(np.float32).astype(np.float64)            # the fp32 y the kernel compares (fma of a bf16 and an fp32 value: exact in float64)
    arg2 = np.argmax(windows(yf), 0)
    routed2 = unwindows(np.stack([np.where(arg2 == k, g, 0.0) for k in range(4)]))
    t = skip.astype(np.float64) + routed2
    xh = (x64 - mean) * istd
    s1, s2 = t.reshape(-1, c).sum(0), (t * xh).reshape(-1, c).sum(0)
    k1, k2 = s1 / pixels, s2 / pixels
    ref = np.where(x64 > 0, sc * (t - k1 - xh * k2), 0.0)
    A = np.abs(sc) * (np.abs(skip) + np.abs(routed2) + np.abs(k1) + np.abs(xh * k2))
    gs = wide(skip, ld + 4, 4, dt, BAD_IN)
    out = wide(np.zeros_like(x), c + 8, 4, dt, SENT)
    ck(ops, E.bn_pool_bwd_apply(dev(x, dt).data_ptr(), c, ops.d(bnp).data_ptr(), d64(np.concatenate([s1, s2])).data_ptr(), float(pixels), ptr(gs, 4), ld + 4,
                                dev(dyp, dt).data_ptr(), ptr(out, 4), c + 8, n, h, w, c, rate, seed), "bn_maxpool_bwd_apply")
    sentinels_kept(out, 4, c, "bn_maxpool_bwd_apply")
    check_store(host(out)[..., 4:4 + c], ref, A, 8, dt, "bn_maxpool_bwd_apply")
    if rate:                                     # keep pattern: with no skip gradient, exactly the routed elements of dropped quads carry only the BatchNorm terms
        out0 = wide(np.zeros_like(x), c + 8, 4, dt, SENT)
        ck(ops, E.bn_pool_bwd_apply(dev(x, dt).data_ptr(), c, ops.d(bnp).data_ptr(), d64(np.zeros(2 * c)).data_ptr(), float(pixels), None, 0,
                                    dev(dyp, dt).data_ptr(), ptr(out0, 4), c + 8, n, h, w, c, rate, seed), "bn_maxpool_bwd_apply no skip")
        got0 = host(out0)[..., 4:4 + c]
        sel = unwindows(np.stack([(arg2 == k).astype(np.float64) for k in range(4)])) > 0
        kept = unwindows(np.stack([ks] * 4))
        live = sel & (x64 > 0)
        assert np.array_equal(got0[live] != 0, kept[live] != 0), "bn_maxpool_bwd_apply: keep pattern differs from philox_ref"
        assert (got0[~live] == 0).all()


# ---- 1x1 sigmoid head + losses ---------------------------------------------------------------------------------------------------------------
SEL = [("bce_dice_loss", 0.5, 0.5), ("binary_crossentropy", 0.5, 0.5), ("dice_loss", 0.5, 0.5), ("tversky_loss", 0.5, 0.5), ("tversky_loss", 0.7, 0.3),
       ("weighted_bce_dice_loss", 0.5, 0.5)]
SEL_IDS = ["bce_dice", "bce", "dice", "tversky", "tversky_0.7_0.3", "weighted"]
LO32, HI32 = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))          # the kernels' clip bounds (fp32)


def head_case(rng, shape, cin, scale=1.0):
    n, h, w = shape
    x = bfx(np.maximum(rng.standard_normal((n, h, w, cin)) * scale, 0.0))
    k = (rng.standard_normal(cin) * 1.5 / np.sqrt(cin)).astype(np.float32); b = np.array([0.1], np.float32)
    k[0] = abs(k[0]) + 0.5
    x[0, 0, 0, :] = bfx(60.0 * (k > 0))                                    # a saturated pixel: p == 1, the clip path
    t = (np.round(rng.random((n, h, w, 1)) ** 2 * 255) / 255).astype(np.float32)
    return x, k, b, t


def head_iters(pixels, cin, det, fwd=True):
    lpp = cin // 4
    if not fwd:
        grid = min(grid_for(pixels * lpp // 4), HEAD_BWD_BLOCKS)
        return cdiv(pixels, grid * TPB // lpp), grid
    if cin == 32:
        grid = max(1, min(cdiv(pixels, TPB * 2), SLOTS_DET if det else HEAD_LPP_BLOCKS))
        return cdiv(pixels, grid * TPB), grid
    grid = max(1, min(cdiv(pixels * lpp // 4, TPB), SLOTS_DET if det else HEAD_BLOCKS))
    return cdiv(pixels, grid * TPB // lpp), grid


def bce_terms(p, t):
    """float64 BCE per element on the fp32 clip bounds, and the logit it goes through"""
    pc = np.clip(p, LO32, HI32)
    z = np.log(pc / (1.0 - pc))
    return np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z))), z


def loss64(name, al, be, t, p, w):
    """the selected loss in float64 (tests/loss_family_oracle.py), the weighted one with the device's weight map w"""
    if name != "weighted_bce_dice_loss":
        return LF.loss_fn(name, al, be)(t, p)
    pc = torch.clamp(p, O.BCE_EPS, 1.0 - O.BCE_EPS)
    z = torch.log(pc / (1.0 - pc))
    l = torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-torch.abs(z)))
    return 0.5 * (w * l).sum() / w.sum() + 0.5 * LF.dice_loss(t, p)


def head_run(ops, E, dt, x, k, b, t, sel, relu_mask, handle=None, use_ex=None):
    """forward (p, loss sums) and backward (dx, dw, db) of the head; returns everything checked, plus the raw device outputs for rerun comparisons"""
    n, h, w, cin = x.shape
    pixels = n * h * w
    name, al, be = sel
    kind = _lib.LOSSES[name]
    ex = use_ex if use_ex is not None else name != "bce_dice_loss"
    xd, kd, bd, td = dev(x, dt), ops.d(k), ops.d(b), ops.d(t)
    wm = None
    if name == "weighted_bce_dice_loss":
        wm = ops.z(n, h, w, 1)
        ck(ops, ops.lib.unet_loss_weight_map(ops.h, td.data_ptr(), wm.data_ptr(), n, h, w, ops.s), "weight map")
    wmp = None if wm is None else wm.data_ptr()
    p = ops.z(n, h, w, 1); sums = ops.z(5, dtype=torch.float64)
    if ex:
        ck(ops, E.head_fwd_ex(xd.data_ptr(), kd.data_ptr(), bd.data_ptr(), p.data_ptr(), td.data_ptr(), wmp, sums.data_ptr(), pixels, cin), "head_fwd_ex", handle)
    else:
        ck(ops, E.head_fwd(xd.data_ptr(), kd.data_ptr(), bd.data_ptr(), p.data_ptr(), td.data_ptr(), sums.data_ptr(), pixels, cin), "head_fwd", handle)
    pg = p.cpu().numpy().astype(np.float64).reshape(-1)
    t64 = t.astype(np.float64).reshape(-1)
    w64 = np.ones_like(t64) if wm is None else wm.cpu().numpy().astype(np.float64).reshape(-1)
    ns = 5 if wm is not None else 4
    # backward on the float64 sums of the kernel's own p
    l, z = bce_terms(pg, t64)
    sref = np.array([(w64 * l).sum(), (t64 * pg).sum(), t64.sum(), pg.sum(), w64.sum()])
    dx = ops.z(n, h, w, cin, dtype=torch.bfloat16 if dt == "bf16" else torch.float32); dw = ops.z(cin); db = ops.z(1)
    if ex:
        ck(ops, E.head_bwd_ex(xd.data_ptr(), kd.data_ptr(), p.data_ptr(), td.data_ptr(), d64(sref).data_ptr(), float(pixels), kind, al, be, wmp, dx.data_ptr(),
                              dw.data_ptr(), db.data_ptr(), pixels, cin, relu_mask), "head_bwd_ex", handle)
    else:
        ck(ops, E.head_bwd(xd.data_ptr(), kd.data_ptr(), p.data_ptr(), td.data_ptr(), d64(sref).data_ptr(), float(pixels), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                           pixels, cin, relu_mask), "head_bwd", handle)
    return dict(p=pg, sums=sums.cpu().numpy()[:ns], sref=sref[:ns], l=l, z=z, t=t64, w=w64, dx=dx, dw=dw.cpu().numpy(), db=db.cpu().numpy())


def head_check(r, x, k, b, sel, relu_mask, dt, det=False, tag=""):
    n, h, w, cin = x.shape
    pixels = n * h * w
    name, al, be = sel
    lpp = cin // 4
    x64 = x.reshape(-1, cin).astype(np.float64); k64 = k.astype(np.float64)
    # p: z = x . k + b over 4 products per lane and a log2(lpp) shuffle tree, then sigmoid (expf, add, divide): |dp| <= p (1 - p) |dz| + 8 u p
    zr = x64 @ k64 + float(b[0])
    pr = O.conv1x1_sigmoid(torch.from_numpy(x64.reshape(n, h, w, cin)), torch.from_numpy(k64.reshape(1, 1, cin, 1)), torch.from_numpy(b.astype(np.float64))).numpy().reshape(-1)
    az = np.abs(x64) @ np.abs(k64) + abs(float(b[0]))
    bp = U * (pr * (1 - pr) * (6 + np.log2(lpp)) * az + 8 * pr)
    check_sum(r["p"], pr, bp, f"head p cin={cin}{tag}", dt)
    assert r["p"][0] == 1.0, "the saturated pixel must hit the clip path"
    # loss sums on the kernel's p: the BCE term through logf / log1pf / expf: <= 8 u (|z| + 1) per element; every sum (n1 + 12) u sum|terms|
    it, _ = head_iters(pixels, cin, det)
    terms = [r["w"] * r["l"], r["t"] * r["p"], r["t"], r["p"], r["w"]][:len(r["sums"])]
    bound = np.array([U * ((it + 12) * np.abs(tm).sum()) for tm in terms])
    bound[0] += U * 8 * (r["w"] * (np.abs(r["z"]) + 1)).sum()
    check_sum(r["sums"], r["sref"], bound, f"head loss sums cin={cin}{tag}", dt)
    # dz by autograd of the selected loss at the kernel's p (float64), times p (1 - p): the logit gradient
    pt = torch.from_numpy(r["p"].copy()).requires_grad_(True)
    loss64(name, al, be, torch.from_numpy(r["t"]), pt, torch.from_numpy(r["w"])).backward()
    dz = pt.grad.numpy() * r["p"] * (1.0 - r["p"])
    cb, A_, B_ = LF.coefs(name, r["t"].reshape(n, h, w, 1), r["p"].reshape(n, h, w, 1), al, be)
    inr = (r["p"] >= LO32) & (r["p"] <= HI32)
    # fp32 dz: coefficients rounded to fp32, ~8 roundings on the chain: DA = |cb w (p - t)| [in range] + p (1 - p) (|A t| + |B|), k = 10 for dx = dz k_c (mask)
    DA = np.where(inr, np.abs(cb * r["w"] * (r["p"] - r["t"])), 0.0) + r["p"] * (1 - r["p"]) * (np.abs(A_ * r["t"]) + abs(B_))
    mask = (x64 > 0) if relu_mask else np.ones_like(x64)
    ref = dz[:, None] * k64[None, :] * mask
    check_store(host(r["dx"]).reshape(-1, cin), ref, DA[:, None] * np.abs(k64)[None, :], 10, dt, f"head dx cin={cin} {name} relu={relu_mask}{tag}")
    itb, gridb = head_iters(pixels, cin, det, fwd=False)
    red = itb + 6 + 4 + gridb + 1                                          # per thread, shuffle levels, waves, fp32 atomics of the workgroups
    check_sum(r["dw"], dz @ x64, U * (10 * (DA @ np.abs(x64)) + red * (np.abs(dz) @ np.abs(x64))), f"head dw cin={cin} {name}{tag}", dt)
    check_sum(r["db"], [dz.sum()], [U * (10 * DA.sum() + red * np.abs(dz).sum())], f"head db cin={cin} {name}{tag}", dt)


@pytest.mark.parametrize("cin", [4, 8, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("dt", DTYPES)
def test_head_widths(ops, dt, cin):
    """every cin the head takes (cin = 32: head_fwd_lpp_kernel; the others: head_fwd_kernel; head_bwd_kernel for all), relu_mask 0 and 1, the default loss
    through the plain entries; and the p-only predict call (no labels): the same p bit for bit.  Bounds in head_check: p (dot product + sigmoid),
    the loss sums (reduction), dx (per element, k = 10), dw / db (reduction of the fp32 dz x)."""
    rng = np.random.default_rng(cin)
    x, k, b, t = head_case(rng, (2, 24, 41), cin)
    E = Ent(ops, dt)
    for relu_mask in (0, 1):
        r = head_run(ops, E, dt, x, k, b, t, SEL[0], relu_mask)
        head_check(r, x, k, b, SEL[0], relu_mask, dt)
    # the oracle's loss value on the same p: bce_dice_loss from the four sums
    pr = torch.from_numpy(r["p"]); tt = torch.from_numpy(r["t"])
    s = r["sums"]
    assert abs((0.5 * s[0] / len(r["p"]) + 0.5 * (1 - (2 * s[1] + 1) / (s[2] + s[3] + 1))) - float(O.bce_dice_loss(tt, torch.clamp(pr, LO32, HI32)))) < 1e-5
    p2 = ops.z(*x.shape[:3], 1)
    pixels = int(np.prod(x.shape[:3]))
    ck(ops, E.head_fwd(dev(x, dt).data_ptr(), ops.d(k).data_ptr(), ops.d(b).data_ptr(), p2.data_ptr(), None, None, pixels, cin), "head_fwd predict")
    assert np.array_equal(p2.cpu().numpy().reshape(-1), r["p"].astype(np.float32))


@pytest.mark.parametrize("cin", [16, 32])
@pytest.mark.parametrize("sel", SEL, ids=SEL_IDS)
@pytest.mark.parametrize("dt", DTYPES)
def test_head_losses(ops, dt, sel, cin):
    """every UNET_LOSS_* selection through the _ex entries (the weighted loss with unet_loss_weight_map's map), on both forward kernels"""
    rng = np.random.default_rng(cin + len(sel[0]))
    x, k, b, t = head_case(rng, (2, 64, 72), cin)
    t[1, :20] = 1.0                                                          # a blob: the weight map varies
    E = Ent(ops, dt)
    r = head_run(ops, E, dt, x, k, b, t, sel, 1, use_ex=True)
    head_check(r, x, k, b, sel, 1, dt)


# ---- slices ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_copy_and_accum_slices(ops, dt):
    """copy_slice: bit-exact into a slice, sentinels around it.  accum_slices, nsrc 1-4 with mixed source strides, accumulate 0 / 1: the fp32 sum of <= 5 bf16
    values with exponents in [-3, 3] is exact, so the result is the float64 sum (fp32) or ONE bf16 rounding of it (bf16) -- rounding after each add would
    differ on a share of these elements (asserted).  nsrc 0 and 5 are refused."""
    rng = np.random.default_rng(61)
    n, h, w, c = 2, 9, 13, 48
    pixels = n * h * w
    E = Ent(ops, dt)
    a = narrow(rng, (n, h, w, c))
    src = wide(a, c + 20, 12, dt, BAD_IN)
    dst = wide(np.zeros_like(a), 2 * c + 8, c, dt, SENT)
    ck(ops, E.copy_slice(ptr(src, 12), c + 20, ptr(dst, c), 2 * c + 8, pixels, c), "copy_slice")
    sentinels_kept(dst, c, c, "copy_slice")
    assert np.array_equal(host(dst)[..., c:2 * c], a.astype(np.float64))
    lds_all = [c, c + 4, 3 * c, c + 36]
    offs = [0, 4, c, 36]
    srcs = [narrow(rng, (n, h, w, c)) for _ in range(4)]
    devs = [wide(s, ld, off, dt, BAD_IN) for s, ld, off in zip(srcs, lds_all, offs)]
    for nsrc in (1, 2, 3, 4):
        for acc in (0, 1):
            old = narrow(rng, (n, h, w, c))
            dst = wide(old, c + 8, 4, dt, SENT)
            sp = (ctypes.c_void_p * 4)(*[ptr(d, o) for d, o in zip(devs, offs)]); lp = (ctypes.c_int32 * 4)(*lds_all)
            ck(ops, E.accum_slices(sp, lp, nsrc, ptr(dst, 4), c + 8, pixels, c, acc), f"accum_slices nsrc={nsrc} acc={acc}")
            sentinels_kept(dst, 4, c, "accum_slices")
            terms = ([old] if acc else []) + srcs[:nsrc]
            exact = np.sum([tm.astype(np.float64) for tm in terms], 0)
            got = host(dst)[..., 4:4 + c]
            assert np.array_equal(got, exact if dt == "fp32" else rne_bf16(exact)), f"accum_slices nsrc={nsrc} acc={acc}: not one rounding of the float64 sum"
            if len(terms) >= 3:
                step = terms[0].astype(np.float64)
                for tm in terms[1:]:
                    step = rne_bf16(step + tm)
                assert (step != rne_bf16(exact)).mean() > 0.05, "the data must tell one rounding from rounding after every add"
    sp = (ctypes.c_void_p * 5)(*([ptr(devs[0])] * 5)); lp = (ctypes.c_int32 * 5)(*([c] * 5))
    for bad in (0, 5):
        assert E.accum_slices(sp, lp, bad, ptr(dst, 4), c + 8, pixels, c, 0) == -1, f"nsrc={bad} must be refused"


# ---- full size, default and deterministic mode -----------------------------------------------------------------------------------------------
FULL_BN = (4, 256, 256)          # x 64 channels: 16.8 M elements; every statistics grid at its cap, bn_apply's grid-stride loop at MAX_BLOCKS
FULL_HEAD = (4, 512, 520)        # x 32 channels: > 2048 x 512 pixels, head_fwd_lpp_kernel at its cap


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("dt", DTYPES)
def test_full_size_statistics(ops, dt, det):
    """Every statistics-producing entry at the full-size shape: bn_stats, bn_stats_concat, bn_bwd_stats, maxpool2x2_dropout_bwd_bnstats,
    maxpool2x2_dropout_bwd_sums, the head's loss sums and its dw / db -- within the float64 bounds of the small-shape tests (whose term counts follow the capped
    grids), and bn_apply per element.  Deterministic mode (a private context, UNET_BN_SLOTS_DET slot copies with one writer each): each entry twice, bit-identical."""
    c = 64
    rng = np.random.default_rng(2024 + det)
    n, h, w = FULL_BN
    pixels = n * h * w
    x, gamma, beta = bn_inputs(rng, FULL_BN, c)
    ctx = _lib.Context.get(0, {"deterministic": 1}, private=True) if det else None
    handle = ctx.handle if ctx else ops.h
    try:
        E = Ent(ops, dt, handle)
        reps = 2 if det else 1
        runs = []
        for _ in range(reps):
            runs.append(bn_stats_checks(E, ops, dt, x, c, pixels, "full bn_stats", handle))
        # concat, bwd stats
        x64 = x.reshape(-1, c).astype(np.float64)
        src = np.concatenate([x64.sum(0), (x64 * x64).sum(0)])
        xd = dev(x, dt)
        outs = {"bn_stats": [r.tobytes() for r in runs]}
        for _ in range(reps):
            s = ops.z(4 * c, dtype=torch.float64)
            ck(ops, E.bn_stats_concat(xd.data_ptr(), c, d64(src).data_ptr(), float(pixels), ops.d(gamma).data_ptr(), ops.d(beta).data_ptr(), s.data_ptr(), pixels, c, c),
               "full bn_stats_concat", handle)
            sn = s.cpu().numpy()
            nt = stats_terms(pixels, c, BN_STATS_BLOCKS)
            check_sum(sn[:c], x64.sum(0), (nt + 2) * U * np.abs(x64).sum(0), "full bn_stats_concat", dt)
            outs.setdefault("concat", []).append(sn.tobytes())
        bnp = bn_params(x, gamma, beta)
        sc, sh, mean, istd = (bnp[i * c:(i + 1) * c].astype(np.float64) for i in range(4))
        y = ops.z(n, h, w, c, dtype=torch.bfloat16 if dt == "bf16" else torch.float32)
        ck(ops, E.bn_apply(xd.data_ptr(), c, ops.d(bnp).data_ptr(), y.data_ptr(), c, pixels, c), "full bn_apply", handle)
        check_store(host(y).reshape(-1, c), x64 * sc + sh, np.abs(x64 * sc) + np.abs(sh), 2, dt, "full bn_apply")
        del y
        dy = bfx(rng.standard_normal(FULL_BN + (c,)))
        g64 = dy.reshape(-1, c).astype(np.float64)
        xh = (x64 - mean) * istd
        ppb = TPB // (c // 4)
        ntb = cdiv(pixels, max(1, min(cdiv(pixels, ppb * 16), BN_BWD_STATS_BLOCKS)) * ppb) + ppb
        dyd = dev(dy, dt)
        for _ in range(reps):
            s = ops.z(2 * c, dtype=torch.float64)
            ck(ops, E.bn_bwd_stats(dyd.data_ptr(), c, xd.data_ptr(), c, ops.d(bnp).data_ptr(), s.data_ptr(), pixels, c), "full bn_bwd_stats", handle)
            sn = s.cpu().numpy()
            check_sum(sn[:c], g64.sum(0), (ntb + 2) * U * np.abs(g64).sum(0), "full bn_bwd_stats sum dy", dt)
            check_sum(sn[c:], (g64 * xh).sum(0), (ntb + 5) * U * np.abs(g64 * xh).sum(0), "full bn_bwd_stats sum dy xhat", dt)
            outs.setdefault("bwd_stats", []).append(sn.tobytes())
        del dyd
        # pooled statistics at rate 0.25
        rate, seed = 0.25, 99
        ho, wo = h // 2, w // 2
        total = n * ho * wo * (c // 4)
        dyp = bfx(rng.standard_normal((n, ho, wo, c)))
        ks = PX.keep_scale_dense(dyp.shape, rate, seed).astype(np.float64)
        g = dyp.astype(np.float64) * ks
        ig = (np.float32(1.0) / gamma).astype(np.float64)
        p = bfx(rng.standard_normal((n, ho, wo, c)))
        unkeep = float(np.float32(1.0) - np.float32(rate))
        grid2 = max(1, min(cdiv(total, TPB * 4), BN_STATS_BLOCKS))
        nt2 = cdiv(total, grid2 * TPB) + TPB // (c // 4)
        u2 = g * (p.astype(np.float64) * unkeep - beta) * ig
        for _ in range(reps):
            s = ops.z(2 * c, dtype=torch.float64)
            ck(ops, E.pool_bwd_sums(dev(p, dt).data_ptr(), dev(dyp, dt).data_ptr(), ops.d(gamma).data_ptr(), ops.d(beta).data_ptr(), s.data_ptr(), n, h, w, c, rate, seed),
               "full pool_bwd_sums", handle)
            sn = s.cpu().numpy()
            check_sum(sn[:c], g.reshape(-1, c).sum(0), (nt2 + 3) * U * np.abs(g).reshape(-1, c).sum(0), "full pool_bwd_sums sum g", dt)
            check_sum(sn[c:], u2.reshape(-1, c).sum(0), (nt2 + 6) * U * (np.abs(g) * (np.abs(p * unkeep) + np.abs(beta)) * np.abs(ig)).reshape(-1, c).sum(0),
                      "full pool_bwd_sums sum g xhat", dt)
            outs.setdefault("pool_sums", []).append(sn.tobytes())
        yv = x                                                                   # any tensor: the pooled routing reads it as y
        arg = np.argmax(windows(yv.astype(np.float64)), 0)
        routed = unwindows(np.stack([np.where(arg == k, g, 0.0) for k in range(4)]))
        v = routed                                                               # (no skip gradient: dx starts at zero)
        grid = max(1, min(cdiv(total, TPB), POOL_BWD_STATS_BLOCKS))
        nt = 4 * cdiv(total, grid * TPB) + TPB // (c // 4)
        y64 = yv.astype(np.float64)
        yd = dev(yv, dt); dypd = dev(dyp, dt)
        for _ in range(reps):
            dx = ops.z(n, h, w, c, dtype=torch.bfloat16 if dt == "bf16" else torch.float32); s = ops.z(2 * c, dtype=torch.float64)
            ck(ops, E.pool_bwd_bnstats(yd.data_ptr(), c, dypd.data_ptr(), dx.data_ptr(), c, ops.d(gamma).data_ptr(), ops.d(beta).data_ptr(), s.data_ptr(), n, h, w, c,
                                       rate, seed), "full pool_bwd_bnstats", handle)
            sn = s.cpu().numpy()
            check_sum(sn[:c], v.reshape(-1, c).sum(0), (nt + 3) * U * np.abs(v).reshape(-1, c).sum(0), "full pool_bwd_bnstats sum v", dt)
            check_sum(sn[c:], (v * (y64 - beta) * ig).reshape(-1, c).sum(0), (nt + 6) * U * (np.abs(v) * (np.abs(y64) + np.abs(beta)) * np.abs(ig)).reshape(-1, c).sum(0),
                      "full pool_bwd_bnstats sum v xhat", dt)
            outs.setdefault("pool_bnstats", []).append(sn.tobytes())
            del dx
        del yd, dypd, xd
        # head at the U-Net's width
        hx, hk, hb, ht = head_case(rng, FULL_HEAD, 32)
        for _ in range(reps):
            r = head_run(ops, E, dt, hx, hk, hb, ht, SEL[0], 1, handle=handle)
            outs.setdefault("head", []).append(r["sums"].tobytes() + r["dw"].tobytes() + r["db"].tobytes() + r["p"].tobytes())
        head_check(r, hx, hk, hb, SEL[0], 1, dt, det=bool(det), tag=" full")
        if det:
            for key, pair in outs.items():
                assert pair[0] == pair[1], f"deterministic mode: {key} differs between two runs"
    finally:
        if ctx is not None:
            ctx.close()

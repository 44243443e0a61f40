"""References, bounds and check functions of the BatchNorm-folded conv3x3's three launches, shared by test_gpu_bnfold_elem.py (the device
against them) and test_bnfold_bounds_host.py (a defective result must fail them).  Everything is torch float64 on the device of its inputs (CPU here, the GPU in
the -m gpu file: nine shifted matrix products per convolution, no convolution library involved), NHWC / HWIO as the C ABI.

Notation: u = 2^-24 (gpu_util.U), EPS_SPLIT = 16 u the h2 product bound per unit of A1 = sum |a| |b|; a chain of k fp32 roundings over terms t costs k u sum |t|.
The derivations are in the docstrings of the functions that build each bound; the launch geometry they mirror is kernels_bnfold.hip's."""
import numpy as np
import torch

from gpu_util import EPS_SPLIT, U

F64 = torch.float64


def cdiv(a, b):
    return -(-int(a) // int(b))


def t64(a, dev="cpu"):
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=F64)
    return torch.as_tensor(np.asarray(a), dtype=F64).to(dev)


# ---- float64 convolutions as shifted matrix products -------------------------------------------------------------------------------------------------------------
def shifted(t, a, b):
    """s[n, i, j] = t[n, i + a - 1, j + b - 1], zero outside the image (t NHWC)"""
    n, h, w, c = t.shape
    p = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
    return p[:, a:a + h, b:b + w]


def conv64(z, k):
    """y[n,i,j,o] = sum_{a,b,c} z[n,i+a-1,j+b-1,c] k[a,b,c,o]  (zero padding of z)"""
    y = None
    for a in range(3):
        for b in range(3):
            t = shifted(z, a, b) @ k[a, b]
            y = t if y is None else y + t
    return y


def dgrad64(dy, k):
    """dz[n,i,j,c] = sum_{a,b,o} dy[n,i-a+1,j-b+1,o] k[a,b,c,o]"""
    dz = None
    for a in range(3):
        for b in range(3):
            t = shifted(dy, 2 - a, 2 - b) @ k[a, b].T
            dz = t if dz is None else dz + t
    return dz


def wgrad64(z, dy):
    """dw[a,b,c,o] = sum_p z[p + (a-1, b-1), c] dy[p, o]"""
    ci, co = z.shape[-1], dy.shape[-1]
    d2 = dy.reshape(-1, co)
    return torch.stack([torch.stack([shifted(z, a, b).reshape(-1, ci).T @ d2 for b in range(3)]) for a in range(3)])


def border_classes(h, w):
    """the kernel's class index of pixel (py, px): 4 * (py == 0 | (py == H-1) << 1) + (px == 0 | (px == W-1) << 1)"""
    rowc = (np.arange(h) == 0).astype(int) | ((np.arange(h) == h - 1).astype(int) << 1)
    colc = (np.arange(w) == 0).astype(int) | ((np.arange(w) == w - 1).astype(int) << 1)
    return (rowc[:, None] << 2) | colc[None, :]


def tap_inside(cls, a, b):
    """whether tap (a, b) of a pixel of border class cls stays inside the image (bn_fold_table_kernel's `out`, negated)"""
    rs, cs = cls >> 2, cls & 3
    return not ((a == 0 and (rs & 1)) or (a == 2 and (rs & 2)) or (b == 0 and (cs & 1)) or (b == 2 and (cs & 2)))


def bias_table64(k, b, shift):
    """table[cls][o] = b[o] + sum over the taps inside of T[a][b][o],  T = sum_c shift_c w[a][b][c][o]: float64 [16, cout]"""
    T = torch.einsum("abco,c->abo", k, shift)
    rows = []
    for cls in range(16):
        v = b.clone()
        for a in range(3):
            for bb in range(3):
                if tap_inside(cls, a, bb):
                    v = v + T[a, bb]
        rows.append(v)
    return torch.stack(rows)


# ---- the dispatch of k_conv3x3_h2_fwd (no K slices armed) -----------------------------------------------------------------------------------------------------------
ARMS = ("1,1,4", "1,2,4 inb=1", "1,2,4 inb=2", "2,4,2", "2,2,2")          # launch_h2<0, RW, NB, WAVES-rows>: the template arguments after MODE


def h2_arm(cu, n, h, w, M):
    """which instance of conv_h2_kernel a forward / data-gradient launch with M output channels takes on a device of cu compute units (the arithmetic at the end of
    k_conv3x3_h2_fwd, transcribed)"""
    inb = 2 if M % 64 == 0 else 1
    t8 = cdiv(w, 32) * cdiv(h, 8) * n
    if t8 * cdiv(M, 32) < cu:
        return ARMS[0]
    if inb == 1:
        return ARMS[1]
    if t8 * cdiv(M, 64) < 2 * cu:
        return ARMS[2]
    wgs16 = cdiv(w, 32) * cdiv(h, 16) * n * cdiv(M, 64)
    if h <= 128 and wgs16 >= 512:
        return ARMS[3]
    return ARMS[4]


ARM_CASES = {ARMS[1]: (32, 64, 64), ARMS[2]: (128, 64, 64), ARMS[4]: (128, 136, 32), ARMS[3]: (128, 128, 64)}          # arm -> (M, h, w); the batch follows the CU count


def arm_shape(cu, arm):
    """(n, h, w, M) of the smallest batch at which the launch takes `arm` on cu compute units (256 CUs: 16, 4, 16, 16 images)"""
    M, h, w = ARM_CASES[arm]
    for n in range(1, 1025):
        if h2_arm(cu, n, h, w, M) == arm:
            return n, h, w, M
    raise AssertionError(f"no batch up to 1024 reaches arm {arm} at {cu} CUs")


# ---- data ------------------------------------------------------------------------------------------------------------------------------------------------------------
def make_case(n, h, w, ci, co, regime, seed, producer="none", rate=0.0, drop_seed=0):
    """fp32 inputs of one BatchNorm -> conv3x3 site.  regime "indep": scale / shift drawn independently of x (mean / invstd still x's own); regime "bn": training-mode
    BatchNorm of x itself (eps 1e-3, gamma in [0.5, 1.5], beta in [-0.5, 0.5]) where every fourth channel has mean = 30 std, so sum w scale x and the table cancel to
    a thirtieth of their size.  producer: what made x -- "none", "relu", "elu", "elu_drop" (x = keep_scale * elu(.), the mask of philox_ref at rate / drop_seed)."""
    rng = np.random.default_rng(seed)
    cnt = n * h * w
    r = rng.standard_normal((n, h, w, ci))
    sig = rng.uniform(0.5, 2.0, ci)
    if regime == "bn":
        assert cnt >= 2
        r = (r - r.mean((0, 1, 2))) / r.std((0, 1, 2))
        mu = np.where(np.arange(ci) % 4 == 0, 30.0, rng.uniform(-1.5, 1.5, ci))
        x = sig * (r + mu)
    else:
        x = r * sig + rng.uniform(-1.5, 1.5, ci)
    if producer == "relu":
        x = np.maximum(x, 0.0)
    elif producer in ("elu", "elu_drop"):
        x = np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    x = x.astype(np.float32)
    if producer == "elu_drop":
        import philox_ref as PX
        x = (x * PX.keep_scale_dense((n, h, w, ci), rate, drop_seed)).astype(np.float32)
    k = (rng.standard_normal((3, 3, ci, co)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
    b = (rng.standard_normal(co) * 0.1).astype(np.float32)
    dy = rng.standard_normal((n, h, w, co)).astype(np.float32)
    x64 = x.astype(np.float64)
    mean = x64.mean((0, 1, 2)); var = x64.var((0, 1, 2)); istd = 1.0 / np.sqrt(var + 1e-3)
    if regime == "bn":
        gamma = rng.uniform(0.5, 1.5, ci); beta = rng.uniform(-0.5, 0.5, ci)
        scale = gamma * istd; shift = beta - mean * scale
    else:
        scale = rng.uniform(0.4, 1.6, ci); shift = rng.standard_normal(ci) * 0.7
    out = dict(x=x, k=k, b=b, dy=dy, scale=scale.astype(np.float32), shift=shift.astype(np.float32), mean=mean.astype(np.float32), istd=istd.astype(np.float32),
               std=np.sqrt(var), shape=(n, h, w, ci, co), regime=regime)
    if regime == "bn" and producer == "none":
        hi = np.arange(ci) % 4 == 0                          # the regime is real: the shift dwarfs the spread of the scaled data
        assert (np.abs(out["shift"][hi]) > 20.0 * np.abs(out["scale"][hi]) * out["std"][hi]).all()
    return out


def bnp_of(case):
    return np.concatenate([case["scale"], case["shift"], case["mean"], case["istd"]]).astype(np.float32)


# ---- the common comparison ---------------------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (an element whose bound is 0 must be exact: its ratio is 0 then, inf otherwise); also the index of the worst"""
    ref = t64(ref, ref.device if isinstance(ref, torch.Tensor) else "cpu")
    got = t64(got, ref.device); bound = t64(bound, ref.device).expand_as(ref)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    if r.numel() == 0:
        return 0.0, ()
    i = int(torch.argmax(r))
    return float(r.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))


def check_elem(got, ref, bound, what, limit=1.0):
    r, at = worst_ratio(got, ref, bound)
    print(f"bound-ratio {what} {r:.3g}")
    assert r <= limit, f"{what}: worst error / bound {r:.3g} at {at}"
    return r


# ---- (a) forward ---------------------------------------------------------------------------------------------------------------------------------------------------
def k_tab(cin):
    """roundings on the longest chain of a table entry as the epilogue adds it: bn_fold_taps_kernel runs 8 fma per channel sub-slice (32 channels / 4) and 2 pairwise
    additions; bn_fold_table_kernel adds the ceil(cin / 32) slices in sequence, then up to 9 taps, then the bias; the conv's epilogue adds the entry: 21 + ceil(cin / 32)"""
    return 8 + 2 + cdiv(cin, 32) + 9 + 1 + 1


def fwd_problem(case, dev="cpu"):
    """reference and bound of unet_conv3x3_bnfold_fwd before the activation.  ref = conv3x3(zero-padded scale x + shift) + b.
    |y - ref| <= EPS_SPLIT A1 (1 + 1/16) + k_tab u (|b| + T1):  A1 = sum |x| |scale w| carries the h2 product bound and u A1 (= EPS_SPLIT A1 / 16) for the fp32 product
    scale * w the image is split from;  T1 = sum over the taps inside the image of |shift_c| |w| are the terms of the table entry (k_tab)."""
    n, h, w, ci, co = case["shape"]
    x, k, b, sc, sh = (t64(case[v], dev) for v in ("x", "k", "b", "scale", "shift"))
    pre = conv64(x * sc + sh, k) + b
    a1 = conv64(x.abs(), (k * sc[None, None, :, None]).abs())
    t1 = conv64(sh.abs().expand(1, h, w, ci), k.abs())
    bound = EPS_SPLIT * a1 * (1.0 + 1.0 / 16.0) + k_tab(ci) * U * (b.abs() + t1)
    return dict(pre=pre, bound=bound, cls=border_classes(h, w), a1=a1, t1=t1)


def check_fwd(got, P, act, what):
    """the whole tensor, then every border class on its own (so the message names the class); act 1 = ReLU (1-Lipschitz: the same bound)"""
    want = P["pre"].clamp_min(0.0) if act else P["pre"]
    got = t64(got, want.device)
    worst = {}
    for c_ in np.unique(P["cls"]):
        sel = torch.as_tensor(P["cls"] == c_, device=want.device)
        worst[int(c_)], _ = worst_ratio(got[:, sel], want[:, sel], P["bound"][:, sel])
    print(f"bound-ratio {what} act={act} per border class {({c_: round(v, 3) for c_, v in worst.items()})}")
    r = check_elem(got, want, P["bound"], f"{what} act={act}")
    assert max(worst.values()) <= 1.0, (what, worst)
    return r


# ---- (b) weight gradient, bias gradient, the BatchNorm's backward sums ------------------------------------------------------------------------------------------------
def tap_terms64(dy, images=None, corner=True, swap_rows=False):
    """float64 (db, kr, kc, kk, S) of fold_tap_sums_kernel: per tap the sums of dy over the border row / column the tap excludes and the corner both exclude;
    S = db - kr - kc + kk.  images / corner / swap_rows reproduce defects (a slice of the images only in the border sums; no corner term; first <-> last row)."""
    co = dy.shape[-1]
    db = dy.sum((0, 1, 2))
    d = dy if images is None else dy[images]
    z = torch.zeros(co, dtype=F64, device=dy.device)
    kr = torch.zeros(3, 3, co, dtype=F64, device=dy.device); kc = torch.zeros_like(kr); kk = torch.zeros_like(kr)
    for a in range(3):
        for b in range(3):
            er = {0: 0, 2: -1}.get(a); ec = {0: 0, 2: -1}.get(b)
            if swap_rows and er is not None:
                er = -1 - er
            kr[a, b] = d[:, er].sum((0, 1)) if er is not None else z
            kc[a, b] = d[:, :, ec].sum((0, 1)) if ec is not None else z
            kk[a, b] = d[:, er, ec].sum(0) if (er is not None and ec is not None and corner) else z
    return db, kr, kc, kk, db[None, None] - kr - kc + kk


def k_border(n, h, w, co):
    """roundings behind one of kr / kc / kk: border_sums_kernel gives a thread ceil(ceil(len / 4) / nsl) terms of its segment (nsl = 256 / cout threads per channel), then
    adds the nsl partials; fold_tap_sums_kernel gives each of 16 slices ceil(NS / 16) of the NS = 4 n entries, then adds the 16"""
    nsl = 256 // co
    return cdiv(cdiv(max(h, w), 4), nsl) + nsl + cdiv(4 * n, 16) + 16


def wgrad_problem(case, dev="cpu"):
    """references and bounds of unet_conv3x3_bnfold_bwd_weights.

    db: the plain weight gradient's own bias sum, one split operand against 1: |db - ref| <= e_db = EPS_SPLIT D, D = sum_p |dy_o|.
    S = ((db - kr) - kc) + kk:  e_S = e_db + k_border u (R_r + R_c + R_k) + 3 u (D + R_r + R_c + R_k), R = the sums of |dy| behind kr, kc, kk (k_border), 3 for the
    three operations of the expression.
    dw = fmaf(scale, dw_raw, shift * S): |dw - ref| <= |scale| EPS_SPLIT A1_raw + 3 u (|scale dw_raw| + |shift S|) + |shift| e_S  (two roundings, one to spare;
    A1_raw = sum_p |x| |dy| of the tap).  A tap wholly outside a one-row / one-column image has A1_raw = 0 and S = 0 exactly: what may remain is |shift| e_S.
    sums[c] += sum_{tap,o} W S: ceil(9 cout / 256) fma per thread, then double: (ceil(9 cout / 256) + 1) u sum |W| |S| + sum |W| e_S.
    sums[cin + c] += istd (sum W dW_raw - mean sum W S): istd (e_dzx + |mean| e_dz), e_dzx = (ceil(9 cout / 256) + 1) u sum |W| |dW_raw| + sum |W| EPS_SPLIT A1_raw."""
    n, h, w, ci, co = case["shape"]
    x, k, dy, sc, sh, mean, istd = (t64(case[v], dev) for v in ("x", "k", "dy", "scale", "shift", "mean", "istd"))
    dw_raw = wgrad64(x, dy); a1_raw = wgrad64(x.abs(), dy.abs())
    db, kr, kc, kk, S = tap_terms64(dy)
    D, Rr, Rc, Rk, _ = tap_terms64(dy.abs())
    e_db = EPS_SPLIT * D
    e_S = e_db[None, None] + k_border(n, h, w, co) * U * (Rr + Rc + Rk) + 3 * U * (D[None, None] + Rr + Rc + Rk)
    sc4, sh4 = sc[None, None, :, None], sh[None, None, :, None]
    dw = sc4 * dw_raw + sh4 * S[:, :, None, :]
    dw_bound = sc4.abs() * EPS_SPLIT * a1_raw + 3 * U * ((sc4 * dw_raw).abs() + (sh4 * S[:, :, None, :]).abs()) + sh4.abs() * e_S[:, :, None, :]
    outside = np.zeros((3, 3), bool)
    if h == 1:
        outside[0] = outside[2] = True
    if w == 1:
        outside[:, 0] = outside[:, 2] = True
    kf = cdiv(9 * co, 256) + 1
    ka = k.abs()
    dz = dgrad64(dy, k)
    xhat = (x - mean) * istd
    s1 = dz.sum((0, 1, 2)); s2 = (dz * xhat).sum((0, 1, 2))
    e_dz = kf * U * torch.einsum("abco,abo->c", ka, S.abs()) + torch.einsum("abco,abo->c", ka, e_S)
    e_dzx = kf * U * torch.einsum("abco,abco->c", ka, dw_raw.abs()) + EPS_SPLIT * torch.einsum("abco,abco->c", ka, a1_raw)
    return dict(dw=dw, dw_bound=dw_bound, db=db, db_bound=e_db, outside=outside, dz=dz, sums=torch.cat([s1, s2]), sums_bound=torch.cat([e_dz, istd * (e_dzx + mean.abs() * e_dz)]),
                S=S, dw_raw=dw_raw, count=float(n * h * w))


def check_wgrad(dw, db, P, what):
    dev = P["dw"].device
    dw = t64(dw, dev)
    rb = check_elem(db, P["db"], P["db_bound"], f"{what} db")
    inside = torch.as_tensor(~P["outside"], device=dev)
    r = check_elem(dw[inside], P["dw"][inside], P["dw_bound"][inside], f"{what} dw")
    ro = 0.0
    if P["outside"].any():
        out = torch.as_tensor(P["outside"], device=dev)
        assert float(P["dw"][out].abs().max()) == 0.0
        ro = check_elem(dw[out], P["dw"][out], P["dw_bound"][out], f"{what} dw of the taps wholly outside the image (exactly 0; |shift| e_S allowed)")
    return r, ro, rb


def check_bn_sums(got, prefill, P, what):
    """got = prefill + the kernel's sums (double accumulators: the addition itself costs 2^-52 of the operands, allowed for)"""
    from gpu_util import check_sum
    ci = P["sums"].numel() // 2
    got, prefill = t64(got, P["sums"].device), t64(prefill, P["sums"].device)
    bound = P["sums_bound"] + 2.0 ** -50 * (prefill.abs() + P["sums"].abs())
    d = (got - prefill).cpu().numpy(); ref = P["sums"].cpu().numpy(); bd = bound.cpu().numpy()
    return check_sum(d[:ci], ref[:ci], bd[:ci], f"{what} sum dz"), check_sum(d[ci:], ref[ci:], bd[ci:], f"{what} sum dz xhat")


# ---- (c) data gradient with the BatchNorm backward in the epilogue --------------------------------------------------------------------------------------------------
def bn_coef64(scale, mean, istd, sums, count):
    """bn_bwd_coef_kernel in float64: dx = sc (dz - k1 - xhat k2) = K0 dz + K1 x + K2"""
    ci = scale.numel()
    k1, k2 = sums[:ci] / count, sums[ci:] / count
    return scale, -scale * istd * k2, scale * (mean * istd * k2 - k1)


def mask_factor64(x, mode, rate=0.0, seed=0):
    """common.h mask_factor: UNET_MASK_NONE 1, _RELU [x > 0], _ELU x > 0 ? 1 : x + 1, _ELU_DROP ks (a > 0 ? 1 : a + 1) with a = x (1 - rate), ks the keep factor"""
    if mode == 0:
        return torch.ones_like(x)
    if mode == 1:
        return (x > 0).to(F64)
    if mode == 2:
        return torch.where(x > 0, torch.ones_like(x), x + 1.0)
    import philox_ref as PX
    ks = t64(PX.keep_scale_dense(tuple(x.shape), rate, seed), x.device)
    a = x * (1.0 - float(np.float32(rate)))
    return ks * torch.where(a > 0, torch.ones_like(a), a + 1.0)


def dgrad_problem(case, sums, mode=0, rate=0.0, seed=0, x_channels=None, dev="cpu", drop_k2=False, ignore_limit=False):
    """reference and bound of unet_conv3x3_bnfold_bwd_data: ref = f(x) (K0 dz + K1 x + K2); channels >= x_channels: K0 dz + K2 (x is not read there).
    |dx - ref| <= |f| (|K0| EPS_SPLIT A1 + 4 u (|K0 dz| + |K1 x| + |K2|)) + 3 u |ref|:  A1 = sum |dy| |w|;  K1 and K2 are rounded to fp32 once, fmaf(K1, x, K2) and
    fmaf(K0, dz, .) round once each -- three roundings on the K1 x and K2 terms, one on K0 dz, one to spare;  the factor costs up to three (a = x (1 - rate), a + 1,
    the product with the keep factor) -- the last multiplication is inside the spare."""
    n, h, w, ci, co = case["shape"]
    x, k, dy, sc, mean, istd = (t64(case[v], dev) for v in ("x", "k", "dy", "scale", "mean", "istd"))
    sums = t64(sums, dev)
    K0, K1, K2 = bn_coef64(sc, mean, istd, sums, float(n * h * w))
    if drop_k2:
        K2 = torch.zeros_like(K2)
    dz = dgrad64(dy, k); a1 = dgrad64(dy.abs(), k.abs())
    lim = ci if x_channels is None else x_channels
    assert lim == ci or mode == 0
    xs = x.clone()
    if lim < ci and not ignore_limit:
        xs[..., lim:] = 0.0
    f = mask_factor64(xs, mode, rate, seed)
    inner = K0 * dz + K1 * xs + K2
    ref = f * inner
    bound = f.abs() * (K0.abs() * EPS_SPLIT * a1 + 4 * U * ((K0 * dz).abs() + (K1 * xs).abs() + K2.abs())) + 3 * U * ref.abs()
    return dict(ref=ref, bound=bound, dz=dz, lim=lim, K=(K0, K1, K2))


def check_dgrad(got, P, what):
    got = t64(got, P["ref"].device)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    lim, ci = P["lim"], P["ref"].shape[-1]
    r = check_elem(got[..., :lim], P["ref"][..., :lim], P["bound"][..., :lim], f"{what} dx")
    if lim < ci:
        r = max(r, check_elem(got[..., lim:], P["ref"][..., lim:], P["bound"][..., lim:], f"{what} dx of the channels from x_channels = {lim} on (K0 dz + K2)"))
    return r


def bn_train_dx_autograd(case, gamma_from_scale=True):
    """torch.autograd's gradient of <dy, conv3x3(BN_train(x))> with respect to x, float64 throughout (mean / variance of x itself, eps 1e-3, gamma = scale / invstd
    of the case's fp32 scale so that the float64 scale equals the case's), and the float64 (scale, mean, invstd) it ran with"""
    x, k, dy = (t64(case[v]) for v in ("x", "k", "dy"))
    xr = x.clone().requires_grad_(True)
    mean = xr.mean((0, 1, 2)); var = xr.var((0, 1, 2), unbiased=False); istd = 1.0 / torch.sqrt(var + 1e-3)
    gamma = (t64(case["scale"]) / istd).detach()
    z = (xr - mean) * istd * gamma + 0.25
    (conv64(z, k) * dy).sum().backward()
    return xr.grad, (gamma * istd).detach(), mean.detach(), istd.detach()


def exact_sums(dz, x, mean, istd):
    xhat = (x - mean) * istd
    return torch.cat([dz.sum((0, 1, 2)), (dz * xhat).sum((0, 1, 2))])

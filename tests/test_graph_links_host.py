"""No GPU: tests/graph_links.py has to be shown to bite.  A stand-in engine is made from the oracle in float64 with store=O.store_bf16 (oracle/unet_oracle.py rounds at
exactly the tensors the bf16 engine materialises, accumulates a multiply-written gradient buffer launch by launch and folds a BatchNorm the engine's way); its
activations, gradients and parameter gradients are taken as if they were taps.  Where an engine gradient tap holds the masked pre-activation gradient (every conv
output; the 32 hidden units) the oracle's gradient of the stored OUTPUT is converted to that convention: times the producer's derivative from the stored output
(and the keep factor), stored once.  Then
  * the stand-in passes every link at the derived allowances, with the keep masks of tests/philox_ref.py (U-Net++ with dropout on, classifier with dropout on);
  * each planted error, applied to the stand-in's outputs, fails the link named beside it (PLANTED) -- an error that went unnoticed would show as a missing name.
The classifier stand-in runs the unfused encoder tail (pool backward, then the BatchNorm backward on float64 statistics): autograd knows nothing of sums taken from
the pooled tensors.  The fused tail's link is exercised on its own, on a gradient formed by that kernel's formula in this file."""
import numpy as np
import pytest
import torch

import graph_links as G
import philox_ref as PX
from gpu_util import rne_bf16, trunc_bf16
from oracle import unet_oracle as O

f64 = np.float64
DROP_SEED = 0x1234567890ABCDEF
PP_FOLD = tuple(n[0] + "b" for n in O.PP_NODES)
CLS_FOLD = ("c2b", "c3b")


weights_of = G.case_weights


def keep_of(table, shape, conv, rate, drop_seed=DROP_SEED):
    sd = G.FC_SEED if conv == "fc1" else G.seed_of(table, conv)
    return PX.keep_scale_dense(shape, rate, (drop_seed + sd) & G.M64).astype(f64)


def elu_factor(y, ks, rate):
    """the producer's derivative from the stored output; ks: keep factors (any non-zero value marks a kept element; the oracle scales by the float64 1 / (1 - rate))"""
    if ks is None:
        return np.where(y > 0, 1.0, y + 1.0)
    a = y * (1.0 - rate)
    return np.where(a > 0, 1.0, a + 1.0) * (ks != 0) * (1.0 / (1.0 - rate))          # (the oracle's order of operations: the same bits)


class StandIn:
    """activations / gradients / parameter gradients of the storage-emulating oracle, keyed like the engine's taps; .act / .grad / .pgrads may be edited (planted errors)"""

    def __init__(self, arch, n, h, w, drop, seed=3):
        self.arch, self.drop = arch, drop
        rng = np.random.default_rng(seed)
        self.w = weights_of(arch, seed, (h, w))
        self.x = rng.random((n, h, w, 1)).astype(np.float32)
        self.ks = {}
        if arch == "unetpp":
            self.table = O.pp_layer_table(1)
            self.y = (np.round(rng.random((n, h, w, 1)) ** 4 * 255) / 255).astype(np.float32)
            if drop:
                for k in (1, 2, 3, 4):
                    self.ks[f"c{k}a"] = keep_of(self.table, (n, h >> (k - 1), w >> (k - 1), O.ENC[k - 1]), f"c{k}a", O.PP_ENC_DROP)
                for nm, c, _, _ in O.PP_NODES:
                    lv = int(nm[1]) - 1
                    for ab in "ab":
                        self.ks[nm + ab] = keep_of(self.table, (n, h >> lv, w >> lv, c), nm + ab, O.PP_BLOCK_DROP)
            r = O.pp_loss_and_grads(self.w, self.x, self.y, {k: (v != 0).astype(f64) for k, v in self.ks.items()} if drop else None, dtype=torch.float64, want_acts=True,
                                    store=O.store_bf16, fold=PP_FOLD)
            self.folded, self.loss = set(PP_FOLD), np.array([r["loss"], r["dice"]])
            alias = {f"c{k}": f"bn{k}" for k in (1, 2, 3, 4)}
            alias.update({nm[0]: nm[0] + "bbn" for nm in O.PP_NODES})
            convs = [f"c{k}{ab}" for k in (1, 2, 3, 4) for ab in "ab"] + [nm[0] + ab for nm in O.PP_NODES for ab in "ab"]
            rate_of = lambda cn: O.PP_ENC_DROP if cn[0] == "c" else O.PP_BLOCK_DROP
        else:
            self.table = O.cls_layer_table(1, (h, w))
            self.y = (rng.random(n) > 0.5).astype(np.float32)
            if drop:
                self.ks["fc1"] = keep_of(self.table, (n, O.CLS_HIDDEN), "fc1", O.CLS_DROP)
            r = O.cls_loss_and_grads(self.w, self.x, self.y, (self.ks["fc1"] != 0).astype(f64) if drop else None, (0.8, 1.4), dtype=torch.float64, want_acts=True,
                                     store=O.store_bf16, fold=CLS_FOLD)
            self.folded, self.loss = set(CLS_FOLD), np.array([r["loss"], r["f1"]])
            alias, convs = {}, [f"c{k}{ab}" for k in (1, 2, 3) for ab in "ab"]
        self.raw_grad = {k: v for k, v in r["act_grads"].items() if v is not None}          # gradients of the stored OUTPUTS, not yet stored themselves
        self.act = {k: np.asarray(v, f64) for k, v in r["acts"].items()}
        self.grad = {}
        for k, g in self.raw_grad.items():
            if k == "out":
                continue
            y = self.act[k]
            if arch == "unetpp" and k in convs:
                g = g * elu_factor(y, self.ks.get(k), rate_of(k))
            elif k in convs:
                g = g * (y > 0)
            if k == "h1":
                self.grad[k] = g * (y > 0) * (1.0 / (1.0 - O.CLS_DROP) if drop else 1.0)          # fp32 on the engine: kept in float64
            else:
                self.grad[k] = O.store_bf16(torch.from_numpy(np.ascontiguousarray(g))).numpy()          # (the oracle's own store: through fp32, as the engine's values are)
        for a, b in alias.items():
            self.act[a] = self.act[b]; self.grad[a] = self.grad[b]
        self.pgrads = {k: np.asarray(v, f64) for k, v in r["grads"].items()}
        self.p = r["p"]

    def src(self, fused_tail=False):
        return G.Src(self.arch, "bf16", self.x, self.y, self.w, lambda nm: self.act[nm], lambda nm: self.grad.get(nm), self.pgrads, self.p, self.loss,
                     drop_seed=DROP_SEED if self.drop else None, folded=self.folded, fused_tail=fused_tail, class_weights=(0.8, 1.4))


@pytest.fixture(scope="module")
def pp():
    return StandIn("unetpp", 2, 16, 24, drop=True)


@pytest.fixture(scope="module")
def cls():
    return StandIn("classifier", 3, 16, 24, drop=True)


def failed_links(si, **kw):
    return G.Links(si.src(**kw), collect=True).run().failed


@pytest.mark.parametrize("arch", ["unetpp", "classifier"])
def test_the_stand_in_passes_every_link(arch, pp, cls, capsys):
    si = pp if arch == "unetpp" else cls
    L = G.Links(si.src()).run()                                  # (raises at the first link that fails)
    out = capsys.readouterr().out
    assert set(si.pgrads) == L.params, sorted(set(si.pgrads) - L.params)
    assert out.count("bound-ratio link") > len(L.params)          # one line per compared link, as the per-op tests print them
    print(out)


def test_the_stand_in_passes_without_dropout():
    for arch, shape in (("unetpp", (2, 16, 16)), ("classifier", (2, 16, 16))):
        G.Links(StandIn(arch, *shape, drop=False, seed=5).src()).run()


def _edit(si, kind, name, value):
    """context: the stand-in with one tap replaced"""
    class Ctx:
        def __enter__(self_):
            self_.d = getattr(si, kind); self_.old = self_.d[name]; self_.d[name] = value
        def __exit__(self_, *a):
            self_.d[name] = self_.old
    return Ctx()


def bn_bwd_restated(si, bn, dy_name, x_name, factor, count_scale=1.0):
    dy, x = si.grad[dy_name], si.act[x_name]
    c = x.shape[-1]
    x2 = x.reshape(-1, c)
    mean, var = x2.mean(0), x2.var(0)
    istd = 1.0 / np.sqrt(var + O.BN_EPS)
    xh = (x - mean) * istd
    cnt = x2.shape[0] * count_scale
    k1, k2 = dy.reshape(-1, c).sum(0) / cnt, (dy * xh).reshape(-1, c).sum(0) / cnt
    return rne_bf16(si.w[bn + "/gamma"].astype(f64) * istd * (dy - k1 - xh * k2) * factor)


def route_first(dyp):
    out = np.zeros((dyp.shape[0], dyp.shape[1] * 2, dyp.shape[2] * 2, dyp.shape[3]))
    out[:, 0::2, 0::2] = dyp
    return out


def planted_pp(si):
    """(what, kind, tap, wrong value, the link that has to fail) for the U-Net++ stand-in"""
    out = []
    g = si.grad
    # 1. one source left out of accum_slice:x1_4+x1_3+x1_2>c1 (the x1_2 slice; the pool backward of p1 wrote the buffer first)
    first = rne_bf16(G.route(g["p1"], si.act["c1"]))
    out.append(("1 accum_slice source dropped", "grad", "c1", rne_bf16(first + g["cat_x1_4"][..., 32:64] + g["cat_x1_3"][..., 32:64]), "bwd sum >c1"))
    # 2. the c1 and x1_2 slices of cat_x1_4 swapped
    cat = si.act["cat_x1_4"].copy(); cat[..., 32:64], cat[..., 64:96] = si.act["cat_x1_4"][..., 64:96], si.act["cat_x1_4"][..., 32:64]
    out.append(("2 skip slices swapped", "act", "cat_x1_4", cat, "fwd c1 = cat_x1_4[32:64]"))
    # 3. one tensor stored by truncation: c1a from the image, restated here
    z = torch.nn.functional.conv2d(torch.from_numpy(si.x.astype(f64)).permute(0, 3, 1, 2), torch.from_numpy(si.w["c1a/kernel"].astype(f64)).permute(3, 2, 0, 1),
                                   torch.from_numpy(si.w["c1a/bias"].astype(f64)), padding=1).permute(0, 2, 3, 1).numpy()
    e = np.where(z > 0, z, np.expm1(np.minimum(z, 0))) * si.ks["c1a"]
    assert np.array_equal(rne_bf16(e), si.act["c1a"])
    out.append(("3 truncating store", "act", "c1a", trunc_bf16(e), "fwd c1a"))
    # 4. ELU's derivative replaced by ReLU's on one conv
    out.append(("4 ReLU derivative for ELU", "grad", "c2b", rne_bf16(si.raw_grad["c2b"] * (si.act["c2b"] > 0)), "bwd bn2: c2>c2b"))
    # 5. the keep scale left off one conv's gradient; a dropout mask from the wrong seed
    y = si.act["x1_2b"]
    out.append(("5a keep scale left off", "grad", "x1_2b", rne_bf16(si.raw_grad["x1_2b"] * elu_factor(y, si.ks["x1_2b"], O.PP_BLOCK_DROP) * (1.0 - O.PP_BLOCK_DROP)), "bwd x1_2bbn: x1_2>x1_2b"))
    out.append(("5b mask of another conv's seed", "grad", "x1_2b", rne_bf16(si.raw_grad["x1_2b"] * elu_factor(y, si.ks["x1_2a"], O.PP_BLOCK_DROP)), "bwd x1_2bbn: x1_2>x1_2b"))
    # 6. one BatchNorm backward with its pixel count off by a factor of two
    out.append(("6 BatchNorm backward count x 2", "grad", "c3b", bn_bwd_restated(si, "bn3", "c3", "c3b", elu_factor(si.act["c3b"], None, 0.0), 2.0), "bwd bn3: c3>c3b"))
    # 9. one bias gradient summed over n - 1 images
    out.append(("9 bias gradient over n - 1 images", "pgrads", "c2a/bias", g["c2a"][:-1].sum((0, 1, 2)), "param c2a/bias"))
    # 10. the folded conv's weight-gradient correction omitted: the raw correlation
    out.append(("10 fold correction omitted", "pgrads", "x1_2b/kernel", G.wgrad64(si.act["x1_2a"], g["x1_2b"]), "param x1_2b/kernel (folded)"))
    return out


def planted_cls(si):
    g = si.grad
    n = si.x.shape[0]
    out = [("7 pool gradient to the first element", "grad", "bn3b", route_first(g["p3"]), "bwd pool p3>bn3b"),
           ("8 (c, h, w) flatten in fc1's weight gradient", "pgrads", "fc1/kernel", si.act["p3"].transpose(0, 3, 1, 2).reshape(n, -1).T @ g["h1"].reshape(n, -1), "param fc1/kernel"),
           ("9 bias gradient over n - 1 images", "pgrads", "c2a/bias", g["c2a"][:-1].sum((0, 1, 2)), "param c2a/bias"),
           ("10 fold correction omitted", "pgrads", "c2b/kernel", G.wgrad64(si.act["c2a"], g["c2b"]), "param c2b/kernel (folded)"),
           ("6 BatchNorm backward count x 2", "grad", "c1a", bn_bwd_restated(si, "bn1a", "bn1a", "c1a", (si.act["c1a"] > 0), 2.0), "bwd bn1a: bn1a>c1a")]
    return out


PLANTED = ["1 accum_slice source dropped", "2 skip slices swapped", "3 truncating store", "4 ReLU derivative for ELU", "5a keep scale left off",
           "5b mask of another conv's seed", "6 BatchNorm backward count x 2", "9 bias gradient over n - 1 images", "10 fold correction omitted"]


@pytest.mark.parametrize("what", PLANTED)
def test_planted_error_in_unetpp_fails_its_link(what, pp):
    (_, kind, tap, wrong, link), = [p for p in planted_pp(pp) if p[0] == what]
    with _edit(pp, kind, tap, wrong):
        failed = failed_links(pp)
    hit = [k for k in failed if k.startswith(link)]
    print(f"planted {what}: failing links {sorted(failed)}")
    assert hit, f"planted error '{what}' went unnoticed by link '{link}'; failing links: {sorted(failed)}"


@pytest.mark.parametrize("what", ["7 pool gradient to the first element", "8 (c, h, w) flatten in fc1's weight gradient", "9 bias gradient over n - 1 images",
                                  "10 fold correction omitted", "6 BatchNorm backward count x 2"])
def test_planted_error_in_classifier_fails_its_link(what, cls):
    (_, kind, tap, wrong, link), = [p for p in planted_cls(cls) if p[0] == what]
    with _edit(cls, kind, tap, wrong):
        failed = failed_links(cls)
    hit = [k for k in failed if k.startswith(link)]
    print(f"planted {what}: failing links {sorted(failed)}")
    assert hit, f"planted error '{what}' went unnoticed by link '{link}'; failing links: {sorted(failed)}"


def fused_tail_restated(si, k, first=False):
    """bn_maxpool_bwd_apply's result from the kernel's formula: sums over the pooled tensors, routing to the first maximum of y"""
    cb, bb, pk = f"c{k}b", f"bn{k}b", f"p{k}"
    x, gp, pv = si.act[cb], si.grad[pk], si.act[pk]
    c = x.shape[-1]
    x2 = x.reshape(-1, c)
    mean, var = x2.mean(0), x2.var(0)
    istd = 1.0 / np.sqrt(var + O.BN_EPS)
    gamma, beta = si.w[bb + "/gamma"].astype(f64), si.w[bb + "/beta"].astype(f64)
    sc = gamma * istd
    y = x * sc + (beta - mean * sc)
    t = route_first(gp) if first else G.route(gp, y)
    k1 = gp.reshape(-1, c).sum(0) / x2.shape[0]; k2 = (gp * (pv - beta) / gamma).reshape(-1, c).sum(0) / x2.shape[0]
    return rne_bf16(np.where(x > 0, sc * (t - k1 - (x - mean) * istd * k2), 0.0)), gp.reshape(-1, c).sum(0), (gp * (pv - beta) / gamma).reshape(-1, c).sum(0)


@pytest.mark.parametrize("k", [1, 3])
def test_the_fused_tail_link_on_its_own(k, cls):
    """the link of pool_bwd_sums + bn_maxpool_bwd_apply passes on a gradient formed by the kernel's formula and fails when the pool gradient goes to the first element"""
    cb, bb = f"c{k}b", f"bn{k}b"
    for first in (False, True):
        dx, s1, s2 = fused_tail_restated(cls, k, first)
        with _edit(cls, "grad", cb, dx), _edit(cls, "pgrads", bb + "/beta", s1), _edit(cls, "pgrads", bb + "/gamma", s2):
            L = G.Links(cls.src(fused_tail=True), collect=True)
            L.cls_fused_tail(k)
        assert bool(L.failed) == first, (first, L.failed)
        if first:
            assert [n for n in L.failed if n.startswith(f"bwd fused tail p{k}>{cb}")], L.failed


def test_the_oracle_defaults_are_unchanged_by_the_storage_arguments():
    """store=None, fold=() is the plain graph: a fold alone (float64, nothing stored) changes values only by round-off -- the folded expression is the same function"""
    w = weights_of("unetpp", 1, (16, 16)); rng = np.random.default_rng(0)
    x = rng.random((2, 16, 16, 1)).astype(np.float32); y = (rng.random((2, 16, 16, 1)) > 0.6).astype(np.float32)
    a = O.pp_loss_and_grads(w, x, y, dtype=torch.float64); b = O.pp_loss_and_grads(w, x, y, dtype=torch.float64, fold=PP_FOLD)
    assert abs(a["loss"] - b["loss"]) < 1e-12
    for k in a["grads"]:
        assert np.abs(a["grads"][k] - b["grads"][k]).max() <= 1e-10 * (np.abs(a["grads"][k]).max() + 1e-30) + 1e-14, k
    w = weights_of("classifier", 1, (16, 16)); yc = (rng.random(2) > 0.5).astype(np.float32)
    a = O.cls_loss_and_grads(w, x, yc, dtype=torch.float64); b = O.cls_loss_and_grads(w, x, yc, dtype=torch.float64, fold=("c1b", "c2b", "c3b"))
    assert abs(a["loss"] - b["loss"]) < 1e-12
    for k in a["grads"]:
        assert np.abs(a["grads"][k] - b["grads"][k]).max() <= 1e-10 * (np.abs(a["grads"][k]).max() + 1e-30) + 1e-14, k

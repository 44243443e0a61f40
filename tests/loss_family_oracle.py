"""float64 torch restatements of the selectable segmentation losses (T1:784-805 and Keras' binary_crossentropy, T1:60) on the probabilities of
oracle.unet_oracle.forward / pp_forward, usable with autograd; their closed-form logit gradients (the form the engine computes,
include/unet_hip.h UNET_LOSS_*); and a loss-selectable training step on top of the oracle's graphs (whose own loss_and_grads is fixed to
bce_dice_loss).  Test-only.

Every loss is a function of the batch sums I = sum t p, St = sum t, Sp = sum p and of the mean clipped BCE, and its gradient at the head's logit is
    dz = cb a + q (A t + B),   a = dBCE/dz = p_clipped - t inside the clip range (0 outside), q = p (1 - p)
with batch scalars (cb, A, B): coefs() below.  tests/golden/loss_family_goldens.npz pins dice_loss / tversky_loss to the reference's own
functions (tests/golden/make_loss_family_goldens.py)."""
import numpy as np
import torch

from oracle import unet_oracle as O

LOSSES = ("bce_dice_loss", "binary_crossentropy", "dice_loss", "tversky_loss", "weighted_bce_dice_loss")
POOL, POOL_BEFORE = 50, 24          # K.pool2d(y, (50, 50), strides=(1, 1), padding='same', pool_mode='avg'): TF's SAME pads 24 before, 25 after


def dice_loss(t, p):
    """T1:792-794: 1 - dice_coeff"""
    return 1.0 - O.dice_coeff(t, p)


def tversky_loss(t, p, alpha=0.5, beta=0.5):
    """T1:801-816: Ncl - sum over classes of num / den, one class (the masks are [n, h, w, 1]): the sums run over every element"""
    num = (p * t).sum()
    den = num + alpha * (p * (1.0 - t)).sum() + beta * ((1.0 - p) * t).sum()
    return 1.0 - num / den


def avg_pool_same(t):
    """TF avg_pool with SAME padding, window 50 x 50, stride 1 (restated from TF's published semantics; TF is not a dependency here): output (r, c) averages
    rows r - 24 ... r + 25 and columns c - 24 ... c + 25 clipped to the image, divided by the number of in-image cells.  t: [n, h, w, 1] float64 tensor."""
    x = t.permute(0, 3, 1, 2)
    ones = torch.ones_like(x)
    pad = (POOL_BEFORE, POOL - 1 - POOL_BEFORE, POOL_BEFORE, POOL - 1 - POOL_BEFORE)
    k = torch.ones((1, 1, POOL, POOL), dtype=t.dtype)
    s = torch.nn.functional.conv2d(torch.nn.functional.pad(x, pad), k)
    c = torch.nn.functional.conv2d(torch.nn.functional.pad(ones, pad), k)
    return (s / c).permute(0, 2, 3, 1)


def weight_map(t):
    """T1:843 before the rescale: 5 exp(-5 |avg - 0.5|)"""
    return 5.0 * torch.exp(-5.0 * torch.abs(avg_pool_same(t) - 0.5))


def weighted_bce_dice_loss(t, p):
    """T1:835-847, with T1's w0 / w1 rescale of the map kept (weighted_bce_loss T1:861-867 divides it out again)"""
    w = weight_map(t)
    w = w * (float(w.numel()) / w.sum())
    pc = torch.clamp(p, O.BCE_EPS, 1.0 - O.BCE_EPS)
    z = torch.log(pc / (1.0 - pc))
    l = w * (z * (1.0 - t) + torch.log1p(torch.exp(-torch.abs(z))) + torch.clamp(-z, min=0))
    return 0.5 * l.sum() / w.sum() + 0.5 * dice_loss(t, p)


def loss_fn(name, alpha=0.5, beta=0.5):
    return {"bce_dice_loss": O.bce_dice_loss, "binary_crossentropy": O.binary_crossentropy_mean, "dice_loss": dice_loss,
            "tversky_loss": lambda t, p: tversky_loss(t, p, alpha, beta), "weighted_bce_dice_loss": weighted_bce_dice_loss}[name]


def coefs(name, t, p, alpha=0.5, beta=0.5):
    """(cb, A, B) of dz = cb a + q (A t + B) from the float64 batch sums"""
    t, p = (np.asarray(a, np.float64) for a in (t, p))
    n = t.size
    i, st, sp = float((t * p).sum()), float(t.sum()), float(p.sum())
    s = st + sp + 1.0
    d = (2.0 * i + 1.0) / s
    if name == "bce_dice_loss":
        return 0.5 / n, -1.0 / s, 0.5 * d / s
    if name == "binary_crossentropy":
        return 1.0 / n, 0.0, 0.0
    if name == "dice_loss":
        return 0.0, -2.0 / s, d / s
    if name == "weighted_bce_dice_loss":                          # cb multiplies w a: 0.5 / sum w (the map without T1's rescale, which cancels)
        return 0.5 / float(weight_map(torch.as_tensor(t)).sum()), -1.0 / s, 0.5 * d / s
    den = i + alpha * (sp - i) + beta * (st - i)
    return 0.0, -(den - i * (1.0 - alpha - beta)) / den ** 2, alpha * i / den ** 2


def closed_form_dz(name, t, p, alpha=0.5, beta=0.5):
    """dL/dz per element by the closed form (z = the head's logit, p = sigmoid(z))"""
    t, p = (np.asarray(a, np.float64) for a in (t, p))
    cb, a_, b_ = coefs(name, t, p, alpha, beta)
    inr = (p >= O.BCE_EPS) & (p <= 1.0 - O.BCE_EPS)
    a = np.where(inr, np.clip(p, O.BCE_EPS, 1.0 - O.BCE_EPS) - t, 0.0)
    if name == "weighted_bce_dice_loss":
        a = a * weight_map(torch.as_tensor(t)).numpy()
    return cb * a + p * (1.0 - p) * (a_ * t + b_)


def loss_and_grads(weights, x, y, loss="bce_dice_loss", alpha=0.5, beta=0.5, arch="unet", dtype=torch.float64, want_acts=False, relu_masks=None,
                   pool_sel=None):
    """oracle.unet_oracle.loss_and_grads / pp_loss_and_grads with the loss selectable.  Returns dict(loss, dice, grads, bn_stats, p[, acts])."""
    in_ch = np.asarray(x).shape[-1]
    names = O.trainable_names(in_ch) if arch == "unet" else O.pp_trainable_names(in_ch)
    W = {k: O._t(v, dtype).clone() for k, v in weights.items()}
    for k in names:
        W[k].requires_grad_(True)
    if arch == "unet":
        p, acts, stats = O.forward(W, x, training=True, dtype=dtype, want_acts=want_acts, relu_masks=relu_masks, pool_sel=pool_sel)
    else:
        p, acts, stats = O.pp_forward(W, x, training=True, dtype=dtype, want_acts=want_acts)
    t = O._t(y, dtype)
    lv = loss_fn(loss, alpha, beta)(t, p)
    dice = O.dice_coeff(t, p)
    lv.backward()
    out = dict(loss=float(lv.detach()), dice=float(dice.detach()), p=p.detach().numpy(), grads={k: W[k].grad.numpy() for k in names},
               bn_stats={k: (m.detach().numpy(), v.detach().numpy(), n) for k, (m, v, n) in stats.items()})
    if want_acts:
        out["acts"] = {k: v.detach().numpy() for k, v in acts.items()}
    return out


class Trainer(O.OracleTrainer):
    """oracle.unet_oracle.OracleTrainer on a selectable loss"""

    def __init__(self, weights, loss="bce_dice_loss", alpha=0.5, beta=0.5, dtype=torch.float64, arch="unet"):
        super().__init__(weights, dtype, arch)
        self.loss, self.alpha, self.beta = loss, alpha, beta

    def train_step(self, x, y, keep_masks=None):
        assert keep_masks is None
        r = loss_and_grads(self.w, x, y, self.loss, self.alpha, self.beta, self.arch, self.dtype)
        for k, (mu, va, n) in r["bn_stats"].items():
            nm, nv = O.bn_moving_update(self.w[k + "/mean"], self.w[k + "/var"], mu, va, n)
            self.w[k + "/mean"] = nm.astype(self.w[k + "/mean"].dtype)
            self.w[k + "/var"] = nv.astype(self.w[k + "/var"].dtype)
        self.t += 1
        O.adam_keras(self.w, r["grads"], self.m, self.v, self.t)
        return r["loss"], r["dice"]

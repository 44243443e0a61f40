"""-m gpu: the U-Net in bf16-storage mode (HipUNet(dtype="bf16"): activations / activation gradients bf16, the rest fp32) against
the oracle run with the SAME storage rounding (oracle.unet_oracle.store_bf16 at every tensor the engine materialises), so the
comparison stays per-tensor tight instead of accumulating 23 layers of rounding; and against the fp32 path for the end metrics.

Tolerances (measured values in brackets, tools/debug_bf16.py):
  * forward tensors: both sides round at the same points, but an element whose fp32-accumulated value (engine) and fp64 value
    (oracle) fall on different sides of a bf16 rounding boundary differs by one bf16 ulp (2^-8), and that difference feeds the
    next layer: the two computations drift apart to the bf16 noise floor within ~10 layers [3e-5 at bn3 -> 6e-3 at c9b].
    Bound: 1e-2 relative L2 per tensor; probabilities 2e-2 absolute; loss / dice_coeff 2e-3.
  * backward tensors: a 6e-3 activation error flips the ReLU mask (and the max-pool argmax) of the ~0.2 % of elements that sit
    that close to zero; a flipped element is a 100 % error of that gradient element, i.e. sqrt(0.002/0.5) = 6e-2 relative L2
    at the first masked tensor, growing upstream [6e-2 at c9b -> 0.17 at c3a].  This is a property of comparing ANY two bf16
    evaluations of a ReLU network (the fp32 test counts the same flips, there they are 0..8 elements), not a kernel error:
    on the elements whose mask agrees the head gradient is checked to 1e-2, and each kernel is pinned on identical inputs at the
    op level: the conv / ConvT / dense kernels to 4e-3 relative L2 in test_gpu_bf16_ops.py; the BatchNorm, pooling / dropout, head
    and slice kernels per element (every stored value the nearest-even bf16 of the float64 result, keep masks exact) in
    test_gpu_storage_ops.py.  Bound here: 0.25 relative L2 and cosine >= 0.97 (a wiring error -- wrong slice, a missing
    skip / pool contribution -- is an O(1) error).
"""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
TOL_T, TOL_G, TOL_L = 1e-2, 0.25, 2e-3


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(max(np.linalg.norm(a - b) - 1e-8 * np.sqrt(a.size), 0.0) / (np.linalg.norm(b) + 1e-30))


def cosine(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def make(h, w=None, **kw):
    from covidseg_amd.engine import HipUNet
    return HipUNet(h, w or h, 1, **kw)


def _case(h, w_, n, seed):
    rng = np.random.default_rng(seed)
    wts = O.init_weights(seed=seed)
    for k in wts:
        if k.endswith("/bias") or k.endswith("/beta"):
            wts[k] = (rng.standard_normal(wts[k].shape) * 0.1).astype(np.float32)
        if k.endswith("/gamma"):
            wts[k] = rng.uniform(0.5, 1.5, wts[k].shape).astype(np.float32)
    # the engine rounds the conv / ConvT kernels to bf16 when it lays them out for the MFMA: give the oracle the same values
    # (c1a and the 1x1 head run on fp32 weights)
    for k in wts:
        if k.endswith("/kernel") and k not in ("c1a/kernel", "out/kernel"):
            wts[k] = bf16(wts[k])
    x = rng.random((n, h, w_, 1)).astype(np.float32)
    y = (np.round(rng.random((n, h, w_, 1)) ** 4 * 255) / 255).astype(np.float32)
    return wts, x, y


@pytest.mark.parametrize("hw,n", [((64, 48), 2), ((32, 64), 3)])
def test_bf16_fwd_bwd_matches_storage_emulating_oracle(hw, n):
    h, w_ = hw
    wts, x, y = _case(h, w_, n, seed=h)
    r = O.loss_and_grads(wts, x, y, dtype=torch.float64, want_acts=True, store=O.store_bf16)
    eng = make(h, w_, dropout_rate=0.0, dtype="bf16")
    eng.set_weights(wts)
    ld = eng.forward_backward(x, y).cpu().numpy()
    assert abs(ld[0] - r["loss"]) < TOL_L and abs(ld[1] - r["dice"]) < TOL_L
    for name in ("c1a", "c1b", "bn1", "p1", "c2a", "c3b", "bn4", "p4", "c5a", "c5b", "u6", "bn6", "c6a", "u9", "bn9", "c9a", "c9b"):
        assert relerr(eng.tap(n, name), r["acts"][name]) < TOL_T, name
    assert np.abs(eng._p_train.cpu().numpy().reshape(r["p"].shape) - r["p"]).max() < 2e-2
    bwd = [o[0] for o in eng.op_profile(n, 1)]
    assert "conv3x3_dgrad_bn_bwd:c9a" in bwd and "bn_bwd_apply:bn9" not in bwd          # the folded decoder BatchNorm is the path under test
    with pytest.raises(Exception):
        eng.tap(n, "bn9", grad=True)                                                      # ... whose output gradient is never stored
    for name, masked in (("c9b", True), ("c9a", True), ("u9", False), ("c6a", True), ("c5b", True), ("c5a", True), ("p4", False),
                         ("c4b", True), ("c2a", True), ("c1a", True)):      # (bn4's total gradient only exists inside the fused encoder-tail pass; c4b is its result)
        want = r["act_grads"][name] * ((r["acts"][name] > 0) if masked else 1.0)
        got = eng.tap(n, name, grad=True)
        assert relerr(got, want) < TOL_G and cosine(got, want) > 0.97, name
    # head backward, flip-free: where the engine's and the oracle's ReLU masks of c9b agree the stored gradient is the oracle's
    # up to its own bf16 rounding and the 2e-2 error of p
    agree = (eng.tap(n, "c9b") > 0) == (r["acts"]["c9b"] > 0)
    assert agree.mean() > 0.99
    got, want = eng.tap(n, "c9b", grad=True), r["act_grads"]["c9b"] * (r["acts"]["c9b"] > 0)
    assert relerr(got * agree, want * agree) < TOL_T
    g = eng.get_grads()
    for k in g:
        if k.startswith("u") and k.endswith("/bias"):
            continue                       # a ConvT bias sits in front of a BatchNorm: its true gradient is 0, both sides return noise
        # (per-channel sums with cancellation -- biases, gamma, beta -- are the noisiest: up to 0.3 measured on 32-element vectors)
        assert relerr(g[k], r["grads"][k]) < 0.4 and cosine(g[k], r["grads"][k]) > 0.92, k


def test_bf16_close_to_fp32_path_end_metrics():
    """What the precision change costs at the outputs the reference reports (Dice / IoU tables): same weights, same batch."""
    from covidseg_amd.data import synthetic_ct
    wts = O.init_weights(seed=11); x, y = synthetic_ct(4, 64, seed=3)
    a, b = make(64, dropout_rate=0.0), make(64, dropout_rate=0.0, dtype="bf16")
    a.set_weights(wts); b.set_weights(wts)
    la = np.array([a.train_batch(x, y).cpu().numpy() for _ in range(6)]); lb = np.array([b.train_batch(x, y).cpu().numpy() for _ in range(6)])
    assert np.abs(la - lb).max() < 2e-2                                    # loss / dice_coeff trajectories stay together
    assert lb[-1, 0] < lb[0, 0]                                            # and the bf16 run learns
    pa, _ = a.predict_batch(x, y); pb, _ = b.predict_batch(x, y)
    th = np.array([0.3, 0.5, 0.547], np.float32)
    sa = a.threshold_sums(pa, y, th).cpu().numpy(); sb = b.threshold_sums(pb, y, th).cpu().numpy()
    ca, cb = O.sm_scores(sa[:, 0], sa[:, 1], sa[:, 2]), O.sm_scores(sb[:, 0], sb[:, 1], sb[:, 2])
    for k in ("dice", "iou"):
        assert np.abs(ca[k] - cb[k]).max() < 2e-2, k


def test_bf16_workspace_is_smaller_and_modes_are_rejected_loudly():
    from covidseg_amd import _lib
    a, b = make(64), make(64, dtype="bf16")
    wa = a.lib.unet_model_workspace_bytes(a._plan(2)["m"], 1); wb = b.lib.unet_model_workspace_bytes(b._plan(2)["m"], 1)
    assert wb < 0.75 * wa                                                  # activations + gradients halve, the split-K scratch does not (it dominates at 64 x 64)
    with pytest.raises(_lib.UNetHipError):
        from covidseg_amd.engine import HipUNet
        HipUNet(60, 64, 1, dtype="bf16")                                   # (any storage: the image must pool four times)


@pytest.mark.parametrize("arch", ["unet", "classifier"])
def test_bf16_storage_takes_a_three_channel_image(arch):
    """BASELINE.json configs[4] writes 224 x 224 x 3: in bf16 storage the first conv of a multi-channel image runs on the fp32 VALU kernels through an fp32 staging
    tensor (the 1-channel kernels keep the image fp32 themselves).  Against the fp32 engine on the same weights / batch: loss, probabilities, the first conv's
    output and its weight gradient."""
    from covidseg_amd.engine import HipUNet
    rng = np.random.default_rng(5)
    n, h, w_ = 4, 32, 48
    x = rng.random((n, h, w_, 3)).astype(np.float32)
    if arch == "classifier":
        wts = O.cls_init_weights(3, 3, (h, w_)); y = (rng.random(n) > 0.5).astype(np.float32)
    else:
        wts = O.init_weights(seed=3, in_ch=3); y = (rng.random((n, h, w_, 1)) > 0.7).astype(np.float32)
    a, b = HipUNet(h, w_, 3, arch=arch, dropout_rate=0.0), HipUNet(h, w_, 3, arch=arch, dropout_rate=0.0, dtype="bf16")
    a.set_weights(wts); b.set_weights(wts)
    la, lb = a.forward_backward(x, y).cpu().numpy(), b.forward_backward(x, y).cpu().numpy()
    assert abs(la[0] - lb[0]) < 3e-2
    assert relerr(b.tap(n, "c1a"), a.tap(n, "c1a")) < 5e-3                # one bf16 rounding of the same fp32 sums
    assert np.abs(a._p_train.cpu().numpy() - b._p_train.cpu().numpy()).max() < 1e-1
    # the first conv's weight / bias gradient IS the correlation of the image with the (bf16) output gradient the engine stored: checked against torch in float64
    # on exactly those tensors (end-to-end bf16 gradients of a 32 x 48 net are too noisy to compare engine against engine)
    dy = torch.from_numpy(b.tap(n, "c1a", grad=True).astype(np.float64)).permute(0, 3, 1, 2)
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    kt = torch.zeros(dy.shape[1], 3, 3, 3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xt, kt, padding=1).backward(dy)
    gb = b.get_grads()
    assert relerr(gb["c1a/kernel"], kt.grad.permute(2, 3, 1, 0).numpy()) < 1e-5
    assert relerr(gb["c1a/bias"], dy.sum((0, 2, 3)).numpy()) < 1e-5


@pytest.mark.parametrize("dropout", [0.0, 0.3])
def test_unetpp_bf16_against_the_fp32_engine(dropout):
    """U-Net++ (BASELINE.json configs[3] names bf16): the nested-skip graph in bf16 storage against the fp32 engine, which
    test_gpu_unetpp.py pins to the oracle.  Same weights, batch and dropout streams (the counter-based RNG indexes elements, not
    bytes).  Forward tensors drift to the bf16 noise floor (<= 3e-2 by the last node), gradients carry the mask / argmax flips
    explained at the top of this file."""
    from covidseg_amd.engine import HipUNet
    from covidseg_amd import weights as W
    from covidseg_amd.data import synthetic_ct
    x, y = synthetic_ct(4, 64, seed=5)
    wts = W.init_weights(3, 1, "unetpp", (64, 64))
    a = HipUNet(64, 64, 1, arch="unetpp", dropout_rate=dropout, seed=9); b = HipUNet(64, 64, 1, arch="unetpp", dropout_rate=dropout, seed=9, dtype="bf16")
    a.set_weights(wts); b.set_weights(wts)
    la, lb = a.forward_backward(x, y).cpu().numpy(), b.forward_backward(x, y).cpu().numpy()
    assert np.abs(la - lb).max() < 2e-2
    for name in ("c1a", "c1", "p1", "c3", "x3_2", "x2_3", "cat_x1_4", "x1_4"):
        assert relerr(b.tap(4, name), a.tap(4, name)) < 3e-2, name
    if dropout:
        assert ((b.tap(4, "x1_4a") == 0) == (a.tap(4, "x1_4a") == 0)).mean() > 0.999            # same keep masks
    ga, gb = a.get_grads(), b.get_grads()
    for k in ga:
        if k.startswith("u") and k.endswith("/bias"):
            continue
        assert cosine(gb[k], ga[k]) > 0.9, k
    ta = np.array([a.train_batch(x, y).cpu().numpy() for _ in range(5)]); tb = np.array([b.train_batch(x, y).cpu().numpy() for _ in range(5)])
    assert np.abs(ta - tb).max() < 3e-2 and tb[-1, 0] < tb[0, 0]
    a.set_weights(wts); b.set_weights(wts)
    pa, _ = a.predict_batch(x, y); pb, _ = b.predict_batch(x, y)
    assert np.abs(pa.cpu().numpy() - pb.cpu().numpy()).max() < 3e-2


def test_classifier_bf16_against_the_fp32_engine():
    """task-2 classifier (BASELINE.json configs[4] names bf16) in bf16 storage against the fp32 engine (pinned to the oracle in
    test_gpu_classifier.py): 16-channel layers run the 32-row MFMA tiles half empty, the 32 hidden units stay fp32."""
    from covidseg_amd.engine import HipUNet
    from covidseg_amd import weights as W
    from covidseg_amd.data import synthetic_classification
    x, y = synthetic_classification(12, 64, seed=2); y = y.astype(np.float32)
    wts = W.init_weights(4, 1, "classifier", (64, 64))
    a = HipUNet(64, 64, 1, arch="classifier", dropout_rate=0.0); b = HipUNet(64, 64, 1, arch="classifier", dropout_rate=0.0, dtype="bf16")
    a.set_weights(wts); b.set_weights(wts)
    la, lb = a.forward_backward(x, y).cpu().numpy(), b.forward_backward(x, y).cpu().numpy()
    assert abs(la[0] - lb[0]) < 2e-2
    for name in ("c1a", "bn1b", "p1", "c2b", "p3", "h1"):
        assert relerr(b.tap(12, name), a.tap(12, name)) < 3e-2, name
    ga, gb = a.get_grads(), b.get_grads()
    for k in ga:
        if k.startswith("c") and k.endswith("/bias"):
            continue                       # a conv bias in front of a BatchNorm: true gradient 0
        assert cosine(gb[k], ga[k]) > 0.9, k
    ta = np.array([a.train_batch(x, y).cpu().numpy() for _ in range(6)]); tb = np.array([b.train_batch(x, y).cpu().numpy() for _ in range(6)])
    assert np.abs(ta[:, 0] - tb[:, 0]).max() < 5e-2 and tb[-1, 0] < tb[0, 0]

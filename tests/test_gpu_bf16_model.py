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

U-Net++ and the classifier (test_*_bf16_matches_storage_emulating_oracle) get the same comparison: the engine against pp_loss_and_grads / cls_loss_and_grads at
store=O.store_bf16 in float64, with the engine's pool selections, folds and (classifier) ReLU masks fed in, on (4, 64, 64) resp. (8, 64, 64) with class weights
(0.8, 1.4).  Their bounds are not chosen: the SAME oracle run in float32 is a second correct evaluation that differs from the float64 one only in arithmetic precision
-- the engine's situation -- and its relative L2 distance from the float64 run was measured on the CPU per stored tensor and per parameter gradient (D32_* below hold
every value); the bound of each is 4 x that distance, the margin for another summation order and other rounding-boundary crossings.  Measured distances [bounds]:
  * U-Net++ tensors: 6.4e-6 at c1a (one or two elements across a bf16 boundary in 524 k) -> 3.7e-5 p1 -> 5.7e-4 bn2 -> 2.9e-3 bn3 -> 6.0e-3 bn4 -> 6.5e-3 u2_3
    -> 5.3e-3 x1_4, probabilities 2.5e-3  [2.5e-5 ... 2.6e-2];  parameter gradients 1.8e-5 (out/bias), 3.0e-5 (x1_4bbn/beta), 4.1e-4 ... 1.8e-2 elsewhere
    (largest: x2_3a/bias)  [7e-5 ... 7.1e-2].  ELU has no mask flips: the gradients stay two orders below the plain U-Net's.
  * classifier tensors: 2.3e-5 c1a -> 1.3e-4 p1 -> 1.3e-3 p2 -> 5.0e-3 p3, h1 4.2e-3, probabilities 5.9e-3  [9e-5 ... 2.4e-2];  parameter gradients 1.3e-3
    (fc2/bias), 3.4e-3 (fc2/kernel), 5.2e-2 ... 2.6e-1 for everything in front of the head  [5e-3 ... 1.04]: dz = cw (p - t) / n cancels where p is close
    to t, so a 6e-3 change of p is a change of tens of per cent of some rows' gradient even with every mask and arg-max held fixed.  Loss 4.0e-3 [1.6e-2].
  * the engine, on an MI355X: every figure inside its bound; the nearest are U-Net++ p1 at 0.79 of its bound (1.17e-4 against 1.48e-4), c2a 0.50, bn1 0.41,
    u1_3/bias 0.40; the classifier's all below 0.35.  Each figure is printed before the assertion (-s).
tests/test_gpu_graph_links.py removes the pile-up altogether: there every tensor is compared with the float64 function of the engine's OWN stored inputs.
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


# ---- U-Net++ and classifier against the storage-emulating oracle (the comparison the plain U-Net has at the top of this file) ---------------------------------
E2E_SHAPE = {"unetpp": (4, 64, 64), "classifier": (8, 64, 64)}
E2E_CW = (0.8, 1.4)
# relative L2 distance between the storage-emulating oracle in float32 and in float64 on the e2e inputs (both with the float64 run's pool selections / ReLU masks, every
# second conv folded), per stored tensor and per parameter gradient; measured on the CPU (_e2e_oracles(arch, None)).  (p4, which the oracle
# computes and the reference never uses, is no tensor of the engine.)  The bounds are 4 x these.
D32_UNETPP_T = {
    "c1a": 6.36e-06, "c1b": 3.59e-05, "bn1": 6.52e-05, "p1": 3.70e-05, "c2a": 1.19e-04, "c2b": 2.75e-04, "bn2": 5.74e-04, "u1_2": 8.71e-04,
    "cat_x1_2": 4.45e-04, "x1_2a": 9.66e-04, "x1_2b": 1.82e-03, "x1_2bbn": 2.14e-03, "p2": 5.86e-04, "c3a": 1.20e-03, "c3b": 1.98e-03, "bn3": 2.94e-03,
    "u2_2": 3.60e-03, "cat_x2_2": 1.93e-03, "x2_2a": 2.76e-03, "x2_2b": 3.65e-03, "x2_2bbn": 4.06e-03, "u1_3": 4.63e-03, "cat_x1_3": 2.29e-03,
    "x1_3a": 3.09e-03, "x1_3b": 3.95e-03, "x1_3bbn": 4.39e-03, "p3": 2.82e-03, "c4a": 3.65e-03, "c4b": 4.28e-03, "bn4": 6.01e-03, "u3_2": 6.34e-03,
    "cat_x3_2": 4.06e-03, "x3_2a": 4.74e-03, "x3_2b": 5.62e-03, "x3_2bbn": 6.08e-03, "u2_3": 6.45e-03, "cat_x2_3": 3.70e-03, "x2_3a": 4.41e-03,
    "x2_3b": 5.26e-03, "x2_3bbn": 5.71e-03, "u1_4": 6.10e-03, "cat_x1_4": 3.33e-03, "x1_4a": 4.10e-03, "x1_4b": 4.90e-03, "x1_4bbn": 5.31e-03,
    "out": 2.50e-03,
}
D32_UNETPP_G = {
    "c1a/kernel": 3.96e-03, "c1a/bias": 5.14e-03, "c1b/kernel": 3.51e-03, "c1b/bias": 1.30e-02, "bn1/gamma": 2.74e-03, "bn1/beta": 1.21e-02,
    "c2a/kernel": 1.04e-02, "c2a/bias": 1.24e-02, "c2b/kernel": 9.31e-03, "c2b/bias": 1.33e-02, "bn2/gamma": 8.19e-03, "bn2/beta": 5.83e-03,
    "u1_2/kernel": 6.03e-03, "u1_2/bias": 5.08e-03, "x1_2a/kernel": 2.41e-03, "x1_2a/bias": 5.94e-03, "x1_2abn/gamma": 1.80e-03,
    "x1_2abn/beta": 7.66e-03, "x1_2b/kernel": 2.14e-03, "x1_2b/bias": 6.25e-03, "x1_2bbn/gamma": 1.91e-03, "x1_2bbn/beta": 1.07e-02,
    "c3a/kernel": 1.19e-02, "c3a/bias": 1.17e-02, "c3b/kernel": 1.18e-02, "c3b/bias": 1.50e-02, "bn3/gamma": 1.02e-02, "bn3/beta": 1.23e-02,
    "u2_2/kernel": 9.97e-03, "u2_2/bias": 1.10e-02, "x2_2a/kernel": 8.42e-03, "x2_2a/bias": 1.68e-02, "x2_2abn/gamma": 7.82e-03,
    "x2_2abn/beta": 8.39e-03, "x2_2b/kernel": 8.29e-03, "x2_2b/bias": 1.01e-02, "x2_2bbn/gamma": 8.18e-03, "x2_2bbn/beta": 5.92e-03,
    "u1_3/kernel": 6.98e-03, "u1_3/bias": 6.63e-03, "x1_3a/kernel": 2.18e-03, "x1_3a/bias": 9.39e-03, "x1_3abn/gamma": 1.63e-03,
    "x1_3abn/beta": 8.65e-03, "x1_3b/kernel": 2.18e-03, "x1_3b/bias": 7.94e-03, "x1_3bbn/gamma": 2.06e-03, "x1_3bbn/beta": 6.30e-03,
    "c4a/kernel": 1.33e-02, "c4a/bias": 1.45e-02, "c4b/kernel": 1.26e-02, "c4b/bias": 1.37e-02, "bn4/gamma": 1.27e-02, "bn4/beta": 1.18e-02,
    "u3_2/kernel": 1.23e-02, "u3_2/bias": 1.35e-02, "x3_2a/kernel": 1.12e-02, "x3_2a/bias": 1.46e-02, "x3_2abn/gamma": 1.18e-02,
    "x3_2abn/beta": 1.03e-02, "x3_2b/kernel": 1.10e-02, "x3_2b/bias": 1.31e-02, "x3_2bbn/gamma": 1.12e-02, "x3_2bbn/beta": 1.12e-02,
    "u2_3/kernel": 1.05e-02, "u2_3/bias": 1.12e-02, "x2_3a/kernel": 7.87e-03, "x2_3a/bias": 1.78e-02, "x2_3abn/gamma": 9.21e-03,
    "x2_3abn/beta": 1.23e-02, "x2_3b/kernel": 7.16e-03, "x2_3b/bias": 1.67e-02, "x2_3bbn/gamma": 5.95e-03, "x2_3bbn/beta": 3.35e-03,
    "u1_4/kernel": 6.36e-03, "u1_4/bias": 8.31e-03, "x1_4a/kernel": 1.67e-03, "x1_4a/bias": 6.43e-03, "x1_4abn/gamma": 6.35e-04,
    "x1_4abn/beta": 7.19e-03, "x1_4b/kernel": 1.17e-03, "x1_4b/bias": 8.73e-03, "x1_4bbn/gamma": 4.13e-04, "x1_4bbn/beta": 2.96e-05,
    "out/kernel": 4.70e-04, "out/bias": 1.78e-05,
}
D32_CLASSIFIER_T = {
    "c1a": 2.32e-05, "c1b": 7.51e-05, "bn1b": 1.19e-04, "p1": 1.26e-04, "c2a": 3.01e-04, "c2b": 8.92e-04, "bn2b": 1.32e-03, "p2": 1.35e-03,
    "c3a": 2.18e-03, "c3b": 4.19e-03, "bn3b": 5.26e-03, "p3": 4.98e-03, "h1": 4.22e-03, "out": 5.92e-03,
}
D32_CLASSIFIER_G = {
    "c1a/kernel": 1.89e-01, "c1a/bias": 2.60e-01, "bn1a/gamma": 1.14e-01, "bn1a/beta": 2.12e-01, "c1b/kernel": 1.35e-01, "c1b/bias": 2.22e-01,
    "bn1b/gamma": 1.38e-01, "bn1b/beta": 1.16e-01, "c2a/kernel": 1.36e-01, "c2a/bias": 1.22e-01, "bn2a/gamma": 1.77e-01, "bn2a/beta": 1.55e-01,
    "c2b/kernel": 1.40e-01, "c2b/bias": 1.48e-01, "bn2b/gamma": 1.25e-01, "bn2b/beta": 1.92e-01, "c3a/kernel": 1.46e-01, "c3a/bias": 1.83e-01,
    "bn3a/gamma": 1.17e-01, "bn3a/beta": 1.47e-01, "c3b/kernel": 1.27e-01, "c3b/bias": 1.94e-01, "bn3b/gamma": 8.77e-02, "bn3b/beta": 5.23e-02,
    "fc1/kernel": 8.88e-02, "fc1/bias": 7.30e-02, "fc2/kernel": 3.42e-03, "fc2/bias": 1.33e-03,
}


def _e2e_inputs(arch):
    import graph_links as G
    n, h, w_ = E2E_SHAPE[arch]
    rng = np.random.default_rng(100 * n + h + w_)
    wts = G.case_weights(arch, 11, (h, w_))
    x = rng.random((n, h, w_, 1)).astype(np.float32)
    y = (np.round(rng.random((n, h, w_, 1)) ** 4 * 255) / 255).astype(np.float32) if arch == "unetpp" else (rng.random(n) > 0.5).astype(np.float32)
    return wts, x, y


def _e2e_oracles(arch, eng_sel, dtypes=(torch.float64, torch.float32)):
    """the storage-emulating oracle on the e2e inputs in each of `dtypes`.  eng_sel: (pool selections, ReLU masks or None, folded convs) read from the engine; None:
    those of the float64 oracle itself with every second conv folded (the default graphs) -- how the D32_* tables were measured, on the CPU"""
    wts, x, y = _e2e_inputs(arch)
    pp = arch == "unetpp"
    if eng_sel is None:
        fold = tuple(nd[0] + "b" for nd in O.PP_NODES) if pp else ("c1b", "c2b", "c3b")
        if pp:
            r0 = O.pp_loss_and_grads(wts, x, y, dtype=torch.float64, want_acts=True, store=O.store_bf16, fold=fold)
            eng_sel = ({f"p{k}": O.pool_selection(r0["acts"][f"bn{k}"]) for k in (1, 2, 3)}, None, fold)
        else:
            r0 = O.cls_loss_and_grads(wts, x, y, None, E2E_CW, dtype=torch.float64, want_acts=True, store=O.store_bf16, fold=fold)
            eng_sel = ({f"p{k}": O.pool_selection(r0["acts"][f"bn{k}b"]) for k in (1, 2, 3)},
                       {f"c{k}{ab}": (r0["acts"][f"c{k}{ab}"] > 0).astype(np.float64) for k in (1, 2, 3) for ab in "ab"}, fold)
    sel, rm, fold = eng_sel
    if pp:
        return [O.pp_loss_and_grads(wts, x, y, dtype=dt, want_acts=True, store=O.store_bf16, pool_sel=sel, fold=fold) for dt in dtypes]
    return [O.cls_loss_and_grads(wts, x, y, None, E2E_CW, dtype=dt, want_acts=True, store=O.store_bf16, pool_sel=sel, relu_masks=rm, fold=fold) for dt in dtypes]


def _e2e_compare(eng, n, r, d32_t, d32_g, tap_name):
    bad = []
    for name, d in d32_t.items():
        if name not in r["acts"]:
            continue
        got = eng._p_train.cpu().numpy().reshape(r["p"].shape) if name == "out" else eng.tap(n, tap_name(name))
        e = relerr(got.reshape(r["acts"][name].shape), r["acts"][name])
        print(f"e2e tensor {name}: engine {e:.2e}  float32 oracle {d:.2e}  bound {4 * d:.2e}")
        if not e <= 4 * d:
            bad.append((name, e, 4 * d))
    g = eng.get_grads()
    assert set(g) == set(d32_g)
    for k, d in d32_g.items():
        e = relerr(g[k], r["grads"][k])
        print(f"e2e gradient {k}: engine {e:.2e}  float32 oracle {d:.2e}  bound {4 * d:.2e}")
        if not e <= 4 * d:
            bad.append((k, e, 4 * d))
    assert not bad, f"{len(bad)} beyond 4 x the float32 oracle's distance: {bad}"


def test_unetpp_bf16_matches_storage_emulating_oracle():
    """bf16 U-Net++ against pp_loss_and_grads(store=O.store_bf16) in float64 with the engine's pool selections and folds: every stored tensor and every parameter
    gradient within 4 x D32_UNETPP_* (module docstring)."""
    from covidseg_amd.engine import HipUNet
    n, h, w_ = E2E_SHAPE["unetpp"]
    wts, x, y = _e2e_inputs("unetpp")
    eng = HipUNet(h, w_, 1, arch="unetpp", dropout_rate=0.0, dtype="bf16")
    eng.set_weights(wts)
    ld = eng.forward_backward(x, y).cpu().numpy()
    fold = tuple(o[0].split(":")[1] for o in eng.op_profile(n, 0) if o[0].startswith("bn_fold_prepare:"))
    sel = {f"p{k}": O.pool_selection(eng.tap(n, f"c{k}")) for k in (1, 2, 3)}          # pool backward routes to the first maximum of the stored tensor
    r, = _e2e_oracles("unetpp", (sel, None, fold), dtypes=(torch.float64,))
    assert abs(ld[0] - r["loss"]) < TOL_L and abs(ld[1] - r["dice"]) < TOL_L
    alias = {f"bn{k}": f"c{k}" for k in (1, 2, 3, 4)}
    _e2e_compare(eng, n, r, D32_UNETPP_T, D32_UNETPP_G, lambda nm: alias.get(nm, nm[:-3] if nm.endswith("bbn") else nm))


def test_classifier_bf16_matches_storage_emulating_oracle():
    """bf16 classifier against cls_loss_and_grads(store=O.store_bf16) in float64 with the engine's ReLU masks, pool selections (the fused encoder tail routes to the first
    maximum of y = fma(x, scale, shift) recomputed in fp32: taken from the stored c{k}b and float64 statistics, graph_links.Links.bn_params) and folds: every stored
    tensor and every parameter gradient within 4 x D32_CLASSIFIER_* (module docstring)."""
    import graph_links as G
    from covidseg_amd.engine import HipUNet
    n, h, w_ = E2E_SHAPE["classifier"]
    wts, x, y = _e2e_inputs("classifier")
    eng = HipUNet(h, w_, 1, arch="classifier", dropout_rate=0.0, dtype="bf16")
    eng.set_class_weights(*E2E_CW)
    eng.set_weights(wts)
    src = G.engine_src(eng, x, y, wts, E2E_CW)
    L = G.Links(src)
    sel = {}
    for k in (1, 2, 3):
        xk = src.act(f"c{k}b"); P = L.bn_params(f"bn{k}b", xk)
        sel[f"p{k}"] = O.pool_selection(xk * P["sc"] + P["sh"])
    rm = {f"c{k}{ab}": (src.act(f"c{k}{ab}") > 0).astype(np.float64) for k in (1, 2, 3) for ab in "ab"}
    r, = _e2e_oracles("classifier", (sel, rm, tuple(sorted(src.folded))), dtypes=(torch.float64,))
    assert abs(src.loss[0] - r["loss"]) < 1.6e-2                          # (4 x the 4.0e-3 between the float32 and the float64 oracle)
    _e2e_compare(eng, n, r, D32_CLASSIFIER_T, D32_CLASSIFIER_G, lambda nm: nm)

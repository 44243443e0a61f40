"""-m gpu: the selectable segmentation losses (include/unet_hip.h UNET_LOSS_*, HipUNet.set_loss, UNetModel.compile(loss=...)) against float64 autograd of
their restatements (tests/loss_family_oracle.py): the op-level entries (unfused head, fused conv3x3 + head with its dy / {dz, mask} backward), the whole U-Net /
U-Net++ step in every head arrangement, and the Keras surface.  Tolerances as tests/test_gpu_ops.py / test_gpu_model.py hold bce_dice_loss."""
import numpy as np
import pytest
import torch

import loss_family_oracle as LF
from covidseg_amd import _lib
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
SEL = [("bce_dice_loss", 0.5, 0.5), ("binary_crossentropy", 0.5, 0.5), ("dice_loss", 0.5, 0.5), ("tversky_loss", 0.5, 0.5), ("tversky_loss", 0.7, 0.3),
       ("weighted_bce_dice_loss", 0.5, 0.5)]
IDS = ["bce_dice", "bce", "dice", "tversky", "tversky_0.7_0.3", "weighted"]


def _wmap(ops, t, loss):
    """the weighted loss's map of labels t [n, h, w, 1] on the device (unet_loss_weight_map), else None"""
    if loss != "weighted_bce_dice_loss":
        return None
    n, h, w = t.shape[:3]
    wm = ops.z(n, h, w, 1)
    ops.ck(ops.lib.unet_loss_weight_map(ops.h, ops.d(t).data_ptr(), wm.data_ptr(), n, h, w, ops.s), "weight map")
    return wm


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("shape", [(1, 16, 16), (2, 64, 64), (1, 200, 136), (2, 512, 512)])
def test_weight_map_against_float64_pool(ops, shape):
    """weighted_bce_dice_loss's map (TF SAME 50 x 50 average pool, clipped windows counted in-image only) against the float64 restatement"""
    n, h, w = shape
    rng = np.random.default_rng(h + w)
    t = (rng.random((n, h, w, 1)) > 0.7).astype(np.float32)
    t[:, : h // 3, : w // 4] = (np.round(rng.random((n, h // 3, w // 4, 1)) * 255) / 255).astype(np.float32)          # soft labels
    got = _wmap(ops, t, "weighted_bce_dice_loss").cpu().numpy()
    want = LF.weight_map(T64(t)).numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), np.abs(got - want).max()
    assert (np.abs(got - want) <= 1e-5 * np.abs(want)).all()


@pytest.fixture(scope="module")
def ops():
    from gpu_util import Ops
    return Ops()


def T64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


@pytest.mark.parametrize("sel", SEL, ids=IDS)
def test_unfused_head_fwd_bwd(ops, sel):
    from gpu_util import relerr
    loss, al, be = sel
    kind = _lib.LOSSES[loss]
    n, h, w, c = 2, 16, 24, 32
    pixels = n * h * w
    rng = np.random.default_rng(9)
    x = np.maximum(rng.standard_normal((n, h, w, c)), 0).astype(np.float32)
    k = (rng.standard_normal((1, 1, c, 1)) * 0.5).astype(np.float32); b = np.array([0.1], np.float32)
    x[0, 0, 0, :] = 60.0 * np.sign(k[0, 0, :, 0]).clip(0)              # one saturated pixel: the clip path of the BCE
    t = (np.round(rng.random((n, h, w, 1)) ** 2 * 255) / 255).astype(np.float32)
    p = ops.z(n, h, w, 1); sums = ops.z(5, dtype=torch.float64); out = ops.z(2)
    wm = _wmap(ops, t, loss)
    ops.ck(ops.lib.unet_head_fwd_ex(ops.h, ops.d(x).data_ptr(), ops.d(k).data_ptr(), ops.d(b).data_ptr(), p.data_ptr(), ops.d(t).data_ptr(), _ptr(wm), sums.data_ptr(), pixels, c, ops.s), "head fwd")
    ops.ck(ops.lib.unet_loss_finalize_ex(ops.h, sums.data_ptr(), float(pixels), kind, al, be, out.data_ptr(), ops.s), "loss fin")
    xt, kt, bt = T64(x).requires_grad_(True), T64(k).requires_grad_(True), T64(b).requires_grad_(True)
    pt = O.conv1x1_sigmoid(xt, kt, bt)
    lv = LF.loss_fn(loss, al, be)(T64(t), pt)
    lo = out.cpu().numpy()
    # (loss value against the fp32 restatement where the BCE enters: its clip bound 1 - 1e-7 is 1 - 1.19e-7 in fp32, which matters for the saturated pixel)
    T32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    ref = LF.loss_fn(loss, al, be)(T32(t), O.conv1x1_sigmoid(T32(x), T32(k), T32(b))) if loss in ("bce_dice_loss", "binary_crossentropy", "weighted_bce_dice_loss") else lv
    assert abs(lo[0] - float(ref)) < 5e-6 and abs(lo[1] - float(O.dice_coeff(T64(t), pt))) < 2e-6
    lv.backward()
    dx = ops.z(n, h, w, c); dw = ops.z(c); db = ops.z(1)
    ops.ck(ops.lib.unet_head_bwd_ex(ops.h, ops.d(x).data_ptr(), ops.d(k).data_ptr(), p.data_ptr(), ops.d(t).data_ptr(), sums.data_ptr(), float(pixels), kind, al, be,
                                    _ptr(wm), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), pixels, c, 1, ops.s), "head bwd")
    assert relerr(dx.cpu().numpy(), xt.grad.numpy() * (x > 0)) < 2e-5
    assert relerr(dw.cpu().numpy(), kt.grad.numpy().ravel()) < 2e-5 and relerr(db.cpu().numpy(), bt.grad.numpy()) < 2e-5
    if loss == "bce_dice_loss":                                         # the default selection is the call without the suffix, bit for bit
        dx2 = ops.z(n, h, w, c); dw2 = ops.z(c); db2 = ops.z(1); out2 = ops.z(2)
        ops.ck(ops.lib.unet_head_bwd(ops.h, ops.d(x).data_ptr(), ops.d(k).data_ptr(), p.data_ptr(), ops.d(t).data_ptr(), sums.data_ptr(), float(pixels),
                                     dx2.data_ptr(), dw2.data_ptr(), db2.data_ptr(), pixels, c, 1, ops.s), "head bwd")
        ops.ck(ops.lib.unet_loss_finalize(ops.h, sums.data_ptr(), float(pixels), out2.data_ptr(), ops.s), "loss fin")
        assert torch.equal(dx, dx2) and torch.equal(out, out2)


def test_bad_loss_selections_are_refused(ops):
    sums = ops.z(4, dtype=torch.float64); out = ops.z(2)
    for kind, al, be in ((5, 0.5, 0.5), (-1, 0.5, 0.5), (3, -0.1, 0.5), (3, 0.0, 0.5), (3, 0.5, 0.0), (3, float("nan"), 0.5)):
        assert ops.lib.unet_loss_finalize_ex(ops.h, sums.data_ptr(), 16.0, kind, al, be, out.data_ptr(), ops.s) == -1, (kind, al, be)


@pytest.mark.parametrize("sel", SEL, ids=IDS)
def test_fused_head_dy_and_dzm(ops, sel):
    """unet_conv3x3_head_fwd (the loss sums and the head's 99 weight-gradient sums are the same for every loss) + unet_head_dy_ex / unet_head_dzm_ex"""
    from gpu_util import relerr
    loss, al, be = sel
    kind = _lib.LOSSES[loss]
    n, h, w, cin, c = 2, 16, 24, 32, 32
    pixels = n * h * w
    rng = np.random.default_rng(21)
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(np.float32)
    k3 = (rng.standard_normal((3, 3, cin, c)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32); b3 = (rng.standard_normal(c) * 0.1).astype(np.float32)
    k = (rng.standard_normal((1, 1, c, 1)) * 0.8).astype(np.float32); b = np.array([-0.2], np.float32)
    t = (np.round(rng.random((n, h, w, 1)) ** 2 * 255) / 255).astype(np.float32)
    y = ops.z(n, h, w, c); p = ops.z(n, h, w, 1); sums = ops.z(5, dtype=torch.float64); hs = ops.z(99, dtype=torch.float64); out = ops.z(2)
    wm = _wmap(ops, t, loss)
    bits = torch.zeros(pixels * c // 8, dtype=torch.uint8, device="cuda")
    ops.ck(ops.lib.unet_request_relu_bits(ops.h, bits.data_ptr()), "arm")
    ops.ck(ops.lib.unet_conv3x3_head_fwd_ex(ops.h, ops.d(x).data_ptr(), ops.d(k3).data_ptr(), ops.d(b3).data_ptr(), y.data_ptr(), ops.d(k).data_ptr(), ops.d(b).data_ptr(), p.data_ptr(),
                                            ops.d(t).data_ptr(), _ptr(wm), sums.data_ptr(), hs.data_ptr(), n, h, w, cin, ops.wws(cin, c), ops.s), "conv + head fwd")
    ops.ck(ops.lib.unet_loss_finalize_ex(ops.h, sums.data_ptr(), float(pixels), kind, al, be, out.data_ptr(), ops.s), "loss fin")
    yt = O.conv3x3_bias_relu(T64(x), T64(k3), T64(b3)).detach().requires_grad_(True)
    kt, bt = T64(k).requires_grad_(True), T64(b).requires_grad_(True)
    zt = (yt.reshape(-1, c) @ kt.reshape(c, 1) + bt).reshape(n, h, w, 1)
    zt.retain_grad()
    pt = torch.sigmoid(zt)
    lv = LF.loss_fn(loss, al, be)(T64(t), pt)
    lo = out.cpu().numpy()
    assert abs(lo[0] - float(lv)) < 1e-5 and abs(lo[1] - float(O.dice_coeff(T64(t), pt))) < 2e-6
    lv.backward()
    yn = y.cpu().numpy()
    dy = ops.z(n, h, w, c); dw = ops.z(c); db = ops.z(1)
    for use_bits in (1, 0):
        dy.zero_(); dw.zero_(); db.zero_()
        ops.ck(ops.lib.unet_head_dy_ex(ops.h, p.data_ptr(), ops.d(t).data_ptr(), sums.data_ptr(), float(pixels), hs.data_ptr(), kind, al, be, _ptr(wm), ops.d(k).data_ptr(),
                                       bits.data_ptr() if use_bits else None, y.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), n, h, w, ops.s), "head dy")
        assert relerr(dy.cpu().numpy(), yt.grad.numpy() * (yn > 0)) < 2e-5
        assert relerr(dw.cpu().numpy(), kt.grad.numpy().ravel()) < 3e-5 and relerr(db.cpu().numpy(), bt.grad.numpy()) < 3e-5
    dzm = torch.zeros(pixels * 2, dtype=torch.int32, device="cuda"); dw.zero_(); db.zero_()
    ops.ck(ops.lib.unet_head_dzm_ex(ops.h, p.data_ptr(), ops.d(t).data_ptr(), sums.data_ptr(), float(pixels), hs.data_ptr(), kind, al, be, _ptr(wm), bits.data_ptr(), dzm.data_ptr(),
                                    dw.data_ptr(), db.data_ptr(), n, h, w, ops.s), "head dzm")
    dz = dzm.view(pixels, 2)[:, 0].contiguous().view(torch.float32).cpu().numpy()
    assert relerr(dz, zt.grad.numpy().ravel()) < 2e-5
    assert relerr(dw.cpu().numpy(), kt.grad.numpy().ravel()) < 3e-5 and relerr(db.cpu().numpy(), bt.grad.numpy()) < 3e-5


def _weights(seed, arch="unet"):
    rng = np.random.default_rng(seed)
    wts = O.init_weights(seed=seed) if arch == "unet" else O.pp_init_weights(seed=seed)
    for k in wts:
        if k.endswith("/bias") or k.endswith("/beta"):
            wts[k] = (rng.standard_normal(wts[k].shape) * 0.1).astype(np.float32)
        if k.endswith("/gamma"):
            wts[k] = rng.uniform(0.5, 1.5, wts[k].shape).astype(np.float32)
    return wts


def _data(seed, n, h):
    rng = np.random.default_rng(seed)
    x = rng.random((n, h, h, 1)).astype(np.float32)
    y = (np.round(rng.random((n, h, h, 1)) ** 4 * 255) / 255).astype(np.float32)
    return x, y


def _check_grads(g, want, tol=3e-4):
    """relative L2 per tensor; a tensor whose exact gradient vanishes (the ConvT biases right in front of a BatchNorm, which removes any per-channel
    constant: float64 leaves ~1e-19) is held to an absolute bound beside the largest gradient instead"""
    from gpu_util import relerr
    top = max(float(np.linalg.norm(v)) for v in want.values())
    for k in g:
        if np.linalg.norm(want[k]) < 1e-12 * top:
            assert np.linalg.norm(g[k]) < 1e-5 * top, k
        else:
            assert relerr(g[k], want[k]) < tol, k


def _engine(h, loss, al, be, **kw):
    from covidseg_amd.engine import HipUNet
    eng = HipUNet(h, h, 1, dropout_rate=0.0, **kw)
    eng.set_loss(loss, al, be)
    return eng


@pytest.mark.parametrize("options", [None, {"head_fused": 0}, {"deterministic": 1}], ids=["fused", "unfused", "det"])
@pytest.mark.parametrize("sel", SEL, ids=IDS)
def test_unet_step_all_grads(sel, options):
    """the whole U-Net step on each loss against float64 autograd on the engine's ReLU sign pattern and pooling choices (test_gpu_model.py)"""
    loss, al, be = sel
    h, n = 64, 2
    wts = _weights(h)
    x, y = _data(h + 1, n, h)
    eng = _engine(h, loss, al, be, options=options)
    eng.set_weights(wts)
    ld = eng.forward_backward(x, y).cpu().numpy()
    bwd = [o[0] for o in eng.op_profile(n, 1)]
    assert ("head_bwd" in bwd) == (options == {"head_fused": 0}), bwd
    convs = [f"c{k}{ab}" for k in range(1, 10) for ab in "ab"]
    emasks = {name: (eng.tap(n, name) > 0).astype(np.float64) for name in convs}
    r = LF.loss_and_grads(wts, x, y, loss, al, be, relu_masks=emasks, pool_sel={f"p{k}": O.pool_selection(eng.tap(n, f"bn{k}")) for k in (1, 2, 3, 4)})
    assert abs(ld[0] - r["loss"]) < 1e-5 and abs(ld[1] - r["dice"]) < 1e-5
    _check_grads(eng.get_grads(), r["grads"])


@pytest.mark.parametrize("sel", [SEL[3], SEL[4], SEL[2], SEL[5]], ids=["tversky", "tversky_0.7_0.3", "dice", "weighted"])
def test_unetpp_step_all_grads(sel):
    from covidseg_amd.engine import HipUNet
    loss, al, be = sel
    h, n = 64, 2
    wts = _weights(h, "unetpp")
    x, y = _data(h + 2, n, h)
    eng = HipUNet(h, h, 1, arch="unetpp", dropout_rate=0.0)
    eng.set_loss(loss, al, be)
    eng.set_weights(wts)
    ld = eng.forward_backward(x, y).cpu().numpy()
    r = LF.loss_and_grads(wts, x, y, loss, al, be, arch="unetpp")
    assert abs(ld[0] - r["loss"]) < 1e-5 and abs(ld[1] - r["dice"]) < 1e-5
    _check_grads(eng.get_grads(), r["grads"])                   # (ELU: no sign-flip discontinuities -- tests/test_gpu_unetpp.py)


@pytest.mark.parametrize("sel", [SEL[2], SEL[4]], ids=["dice", "tversky_0.7_0.3"])
def test_bf16_storage_follows_the_loss(sel):
    """bf16 storage (unet_head_bwd_bf16_ex) on a non-default loss: its gradient is the fp32 engine's on the same loss up to bf16 noise
    (tests/test_gpu_bf16_model.py bounds: 0.25 relative L2, cosine >= 0.97) at the head and the conv in front of it -- further upstream the
    two drift apart as every bf16 comparison does (c8a: cosine 0.970 measured for tversky 0.7 / 0.3) -- and clearly not the default loss's"""
    from gpu_util import relerr
    loss, al, be = sel
    h, n = 64, 2
    wts = _weights(h)
    x, y = _data(h + 3, n, h)
    outs = {}
    for key, dt, ls in (("bf16", "bf16", sel), ("fp32", "fp32", sel), ("bf16_default", "bf16", ("bce_dice_loss", 0.5, 0.5))):
        eng = _engine(h, *ls, dtype=dt)
        eng.set_weights(wts)
        outs[key] = (eng.forward_backward(x, y).cpu().numpy(), eng.get_grads())
        del eng
    (la, ga), (lb, gb), (lc, gc) = outs["bf16"], outs["fp32"], outs["bf16_default"]
    assert abs(la[0] - lb[0]) < 2e-2 * max(1.0, abs(lb[0]))
    for k in ("out/kernel", "out/bias", "c9b/kernel"):
        cos = float((ga[k] * gb[k]).sum() / (np.linalg.norm(ga[k]) * np.linalg.norm(gb[k])))
        assert relerr(ga[k], gb[k]) < 0.25 and cos >= 0.97, (k, cos)
    assert relerr(ga["out/kernel"], gc["out/kernel"]) > 0.3


def test_adam_trajectory_tversky():
    """10 steps of Adam on tversky_loss (0.7, 0.3) against the float64 trainer"""
    h, n = 32, 2
    wts = O.init_weights(seed=5)
    rng = np.random.default_rng(3)
    x = rng.random((n, h, h, 1)).astype(np.float32); y = (rng.random((n, h, h, 1)) > 0.8).astype(np.float32)
    tr = LF.Trainer({k: v.astype(np.float64) for k, v in wts.items()}, "tversky_loss", 0.7, 0.3)
    eng = _engine(h, "tversky_loss", 0.7, 0.3, options={"deterministic": 1})
    eng.set_weights(wts)
    first = None
    for _ in range(10):
        a = eng.train_batch(x, y).cpu().numpy(); b = tr.train_step(x, y)
        assert abs(a[0] - b[0]) < 1e-3 and abs(a[1] - b[1]) < 1e-3
        first = a[0] if first is None else first
    assert a[0] < first                                                  # (and it learns)


def test_default_compile_is_bit_identical_and_losses_switch_on_a_live_model():
    """compile(loss="bce_dice_loss") and no argument run the same program bit for bit (deterministic mode); a model switched to another loss and back
    equals one that never left the default; the program's op list does not depend on the loss"""
    from covidseg_amd.keras_like import UNetModel
    x, y = _data(11, 2, 64)
    runs = []
    for how in ("none", "named", "switched"):
        m = UNetModel(64, seed=2, dropout_rate=0.0, options={"deterministic": 1})
        if how == "none":
            m.compile()
        elif how == "named":
            m.compile(loss="bce_dice_loss")
        else:
            m.compile(loss="tversky_loss", loss_kwargs={"alpha": 0.7, "beta": 0.3})
            w0 = m.get_weights()
            other = m.backend.forward_backward(x, y).cpu().numpy()
            m.set_weights(w0)                                          # (that training-mode forward moved the BatchNorm statistics)
            m.compile(loss="bce_dice_loss")
        ls = [m.backend.train_batch(x, y).cpu().numpy() for _ in range(3)]
        runs.append((np.stack(ls), m.get_weights(), [o[0] for o in m.backend.op_profile(2, 0)] + [o[0] for o in m.backend.op_profile(2, 1)]))
        del m
    for ls, w, names in runs[1:]:
        assert np.array_equal(ls, runs[0][0]) and names == runs[0][2]
        assert all(np.array_equal(w[k], runs[0][1][k]) for k in w)
    assert abs(other[0] - runs[0][0][0][0]) > 1e-3                      # (the Tversky step did compute another loss)


def test_save_load_tversky_resumes_bit_for_bit(tmp_path):
    from covidseg_amd.keras_like import UNetModel, load_model
    x, y = _data(12, 2, 64)
    kw = dict(dropout_rate=0.0, options={"deterministic": 1})
    a = UNetModel(64, seed=3, **kw); a.verbose = 0
    a.compile(loss="tversky_loss", loss_kwargs={"alpha": 0.7, "beta": 0.3})
    for _ in range(2):
        a.backend.train_batch(x, y)
    f = str(tmp_path / "tversky.hdf5")
    a.save(f)
    b = load_model(f, **kw)
    assert b.loss == "tversky_loss" and b.backend.loss == ("tversky_loss", 0.7, 0.3)
    for _ in range(2):
        la = a.backend.train_batch(x, y).cpu().numpy(); lb = b.backend.train_batch(x, y).cpu().numpy()
        assert np.array_equal(la, lb)
    wa, wb = a.get_weights(), b.get_weights()
    assert all(np.array_equal(wa[k], wb[k]) for k in wa)


def test_classifier_keeps_binary_crossentropy():
    from covidseg_amd.engine import HipUNet
    eng = HipUNet(32, 32, 1, arch="classifier")
    with pytest.raises(ValueError):
        eng.set_loss("dice_loss")
    m = eng._plan(2)["m"]
    assert eng.lib.unet_model_set_loss(m, _lib.LOSSES["dice_loss"], 0.5, 0.5) == -1
    assert eng.lib.unet_model_set_loss(m, _lib.LOSSES["binary_crossentropy"], 0.5, 0.5) == 0


def test_weighted_deterministic_reruns_are_bit_identical_and_program_reshapes():
    """weighted_bce_dice_loss in deterministic mode: two engines, three steps each, the same bits; the weight-map op and the 5-double sync point appear with the
    loss and leave with it (the default program's op list is restored)"""
    x, y = _data(13, 2, 64)
    runs = []
    for _ in range(2):
        eng = _engine(64, "bce_dice_loss", 0.5, 0.5, options={"deterministic": 1})
        eng.set_weights(_weights(64))
        base = [o[0] for o in eng.op_profile(2, 0)]
        eng.set_loss("weighted_bce_dice_loss")
        ops_w = [o[0] for o in eng.op_profile(2, 0)]
        assert "loss_weight_map" in ops_w and "loss_weight_map" not in base
        ls = np.stack([eng.train_batch(x, y).cpu().numpy() for _ in range(3)])
        p = eng._plan(2)
        assert [sp[3] for sp in p["sync"][0] if sp[1] == 1] == [5]
        runs.append((ls, eng.get_weights()))
        eng.set_loss("bce_dice_loss")
        assert [o[0] for o in eng.op_profile(2, 0)] == base and [sp[3] for sp in eng._plan(2)["sync"][0] if sp[1] == 1] == [4]
        del eng
    assert np.array_equal(runs[0][0], runs[1][0]) and all(np.array_equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])

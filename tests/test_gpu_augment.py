"""-m gpu: on-device flip + affine augmentation (include/unet_hip.h unet_augment_samples, csrc/kernels_augment.hip; HipUNet.take_augmented / augment_batch;
UNetModel.fit(augment=...) / UNetModel.augment) against the float64 restatement of tests/augment_oracle.py, which reads the same float32 table."""
import os
import socket

import numpy as np
import pytest
import torch

import augment_oracle as AO
from covidseg_amd import augment as AUG
from covidseg_amd.data import synthetic_ct

pytestmark = pytest.mark.gpu
UNET_E_ARG = -1                                                          # include/unet_hip.h


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _kernel(ops, img, mask, idx, mats):
    """unet_augment_samples on host inputs; outputs are pre-filled with NaN so an unwritten pixel shows"""
    n = len(mats)
    h, w, c = img.shape[1:]
    si, dm = ops.d(img), ops.d(mats)
    sm = ops.d(mask) if mask is not None else None
    di = ops.d(idx, np.int64) if idx is not None else None
    oi = torch.full((n, h, w, c), float("nan"), device="cuda")
    om = torch.full((n, h, w, 1), float("nan"), device="cuda") if mask is not None else None
    ops.ck(ops.lib.unet_augment_samples(ops.h, si.data_ptr(), sm.data_ptr() if sm is not None else None, di.data_ptr() if di is not None else None,
                                        dm.data_ptr(), oi.data_ptr(), om.data_ptr() if om is not None else None, n, h, w, c, ops.s), "augment_samples")
    return oi.cpu().numpy(), (om.cpu().numpy() if om is not None else None)


def _tables(n, h, w, seed):
    """n rows: the reference's policy with the affine step always on, then identity, a flip of each kind and one row that maps everything out of frame"""
    t = AUG.AffineAugment(p_affine=1.0).matrices(n, seed, 0, h, w)
    t[1] = [1, 0, 0, 0, 1, 0]
    t[2] = [-1, 0, w - 1, 0, 1, 0]
    t[3] = [1, 0, 0, 0, -1, h - 1]
    t[4] = [1, 0, 4 * w, 0, 1, -3 * h]
    return t


@pytest.mark.parametrize("hw,c,idx_kind", [((224, 224), 1, "repeat"), ((224, 224), 3, "reverse"), ((512, 512), 1, "null"),
                                           ((61, 97), 1, "reverse"), ((61, 97), 3, "repeat"), ((97, 61), 1, "null"), ((512, 512), 3, "repeat")])
def test_kernel_matches_the_float64_restatement(hw, c, idx_kind):
    from gpu_util import Ops
    ops = Ops()
    h, w = hw
    rng = np.random.default_rng(h * 7 + w + c)
    nsrc, n = 5, 7
    img = (rng.standard_normal((nsrc, h, w, c)) * 3).astype(np.float32)
    mask = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(nsrc, h, w, 1))
    idx = {"repeat": np.array([3, 3, 0, 4, 1, 2, 3]), "reverse": np.arange(n)[::-1] % nsrc, "null": None}[idx_kind]
    if idx is None:
        img, mask = np.concatenate([img, img[:2]]), np.concatenate([mask, mask[:2]])
    src = np.arange(n) if idx is None else idx
    mats = _tables(n, h, w, seed=h + c)
    gi, gm = _kernel(ops, img, mask, idx, mats)
    bound = 3e-4 * float(np.abs(img).max())
    for k in range(n):
        want = AO.warp_bilinear(img[src[k]], mats[k])
        err = float(np.abs(gi[k] - want).max())
        assert err <= bound, (k, err, bound)
        wm = AO.warp_nearest(mask[src[k]], mats[k])
        near = AO.near_rounding_boundary(mats[k], h, w)
        diff = (gm[k] != wm)[..., 0]
        assert not np.any(diff & ~near), (k, int((diff & ~near).sum()))
        assert near.mean() < 0.01 and diff.sum() <= near.sum()
        assert set(np.unique(gm[k])) <= set(np.unique(mask[src[k]])) | {0.0}
    # the exact rows: identity copies, flips reverse, bit for bit; the out-of-frame row is all zeros
    assert np.array_equal(gi[1], img[src[1]]) and np.array_equal(gm[1], mask[src[1]])
    assert np.array_equal(gi[2], img[src[2]][:, ::-1]) and np.array_equal(gm[2], mask[src[2]][:, ::-1])
    assert np.array_equal(gi[3], img[src[3]][::-1]) and np.array_equal(gm[3], mask[src[3]][::-1])
    assert not np.any(gi[4]) and not np.any(gm[4])


def test_flip_only_policy_is_bit_exact_and_images_only_call():
    from gpu_util import Ops
    ops = Ops()
    h, w = 61, 97
    rng = np.random.default_rng(3)
    img = rng.standard_normal((6, h, w, 3)).astype(np.float32)
    pol = AUG.AffineAugment(fliplr=0.5, flipud=0.5, p_affine=0.0)
    d, mats = pol.sample(6, 2, 0), pol.matrices(6, 2, 0, h, w)
    gi, gm = _kernel(ops, img, None, None, mats)
    assert gm is None
    for k in range(6):
        want = img[k][::-1] if d.flipud[k] else img[k]
        want = want[:, ::-1] if d.fliplr[k] else want
        assert np.array_equal(gi[k], want), k


def test_bad_arguments_are_refused():
    from gpu_util import Ops
    ops = Ops()
    a, m, o = ops.z(2, 8, 8, 1), ops.z(2, 6), ops.z(2, 8, 8, 1)
    p = lambda t: t.data_ptr()
    ok = (p(a), p(a), None, p(m), p(o), p(o), 2, 8, 8, 1)
    assert ops.lib.unet_augment_samples(ops.h, *ok, ops.s) == 0
    torch.cuda.synchronize()
    # null image / table / output; a mask in without a mask out and the other way round; n, h, w, c out of range
    for k, v in ((0, None), (3, None), (4, None), (1, None), (5, None), (6, 0), (7, 0), (8, -1), (9, 0), (9, 5000)):
        bad = list(ok); bad[k] = v
        assert ops.lib.unet_augment_samples(ops.h, *bad, ops.s) == UNET_E_ARG, (k, v)
    assert ops.lib.unet_augment_samples(ops.h, p(a), None, None, p(m), p(o), None, 2, 8, 8, 1, ops.s) == 0     # images only
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- engine and model
def test_take_augmented_equals_augment_batch_and_the_restatement():
    from covidseg_amd.engine import HipUNet
    eng = HipUNet(64, 64, 1, dropout_rate=0.0)
    x, y = synthetic_ct(10, 64, seed=4)
    dx, dy = eng.resident(x, max_fraction=1.0), eng.resident(y, max_fraction=1.0)
    mats = AUG.AffineAugment().matrices(10, 1, 0, 64, 64)
    table = eng.augment_table(mats)
    for idx, rows in ((np.array([7, 2, 2, 9]), slice(0, 4)), (np.arange(3, 8), slice(5, 10))):
        xa, ya = eng.take_augmented(dx, dy, idx, table[rows])
        xb, yb = eng.augment_batch(x[idx], y[idx], table[rows])
        xa, ya, xb, yb = (t.cpu().numpy() for t in (xa, ya, xb, yb))
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
        for k, j in enumerate(idx):
            r = mats[rows][k]
            assert np.abs(xa[k] - AO.warp_bilinear(x[j], r)).max() <= 3e-4 * np.abs(x).max()
    with pytest.raises(IndexError):
        eng.take_augmented(dx, dy, np.array([0, 10]), table[:2])
    with pytest.raises(ValueError):
        eng.take_augmented(dx, dy, np.array([0, 1]), table[:3])


def _model(arch="unet", **kw):
    from covidseg_amd.keras_like import UNetModel
    m = UNetModel(32, 1, seed=2, arch=arch, **kw)
    m.verbose = 0
    m.compile(lr=0.0005)
    return m


def test_resident_and_staged_augmented_fits_are_bit_identical():
    x, y = synthetic_ct(20, 32, seed=6)
    hists, weights = [], []
    for resident in (True, False):
        m = _model(dropout_rate=0.25, options={"deterministic": 1})
        hists.append(m.fit(x, y, batch_size=6, epochs=2, shuffle_seed=1, augment=True, device_resident=resident).history)
        weights.append(m.get_weights())
    assert hists[0] == hists[1]
    for k in weights[0]:
        assert np.array_equal(weights[0][k], weights[1][k]), k


def test_augmented_fits_are_deterministic_and_differ_from_plain():
    x, y = synthetic_ct(16, 32, seed=7)
    runs = []
    for aug in (True, True, None):
        m = _model(options={"deterministic": 1})
        m.fit(x, y, batch_size=8, epochs=2, shuffle_seed=3, augment=aug, validation_data=(x[:4], y[:4]))
        runs.append(m.get_weights())
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert any(not np.array_equal(runs[0][k], runs[2][k]) for k in runs[0] if k.endswith("/kernel"))


def test_fit_equals_a_manual_loop_of_augment_and_train_batch():
    x, y = synthetic_ct(14, 32, seed=8)
    pol = AUG.AffineAugment(p_affine=0.9)
    m1 = _model(options={"deterministic": 1})
    m1.fit(x, y, batch_size=5, epochs=2, shuffle_seed=4, augment=pol, augment_seed=17)
    m2 = _model(options={"deterministic": 1})
    rng, eng = np.random.RandomState(4), m2.backend
    for ep in range(2):
        order = rng.permutation(14)
        table = eng.augment_table(pol.matrices(14, 17, ep, 32, 32))
        for i in range(0, 14, 5):
            idx = order[i:i + 5]
            xa, ya = eng.augment_batch(x[idx], y[idx], table[i:i + len(idx)])
            eng.train_batch(xa, ya, True)
    w1, w2 = m1.get_weights(), m2.get_weights()
    for k in w1:
        assert np.array_equal(w1[k], w2[k]), k
    # UNetModel.augment is the epoch-0 table of the same policy and seed
    xo, yo = m2.augment(x, y, seed=17, policy=pol)
    t0 = pol.matrices(14, 17, 0, 32, 32)
    xb, yb = eng.augment_batch(x, y, eng.augment_table(t0))
    assert np.array_equal(xo, xb.cpu().numpy()) and np.array_equal(yo, yb.cpu().numpy())


def test_weighted_loss_sees_the_augmented_labels():
    import loss_family_oracle as LF
    from covidseg_amd import weights as W
    from covidseg_amd.engine import HipUNet
    h, n = 64, 2
    x, y = synthetic_ct(4, h, seed=9)
    wts = W.init_weights(5, 1, "unet", (h, h))
    eng = HipUNet(h, h, 1, dropout_rate=0.0)
    eng.set_loss("weighted_bce_dice_loss")
    eng.set_weights(wts)
    dx, dy = eng.resident(x, max_fraction=1.0), eng.resident(y, max_fraction=1.0)
    mats = AUG.AffineAugment(p_affine=1.0).matrices(n, 3, 0, h, h)
    xa, ya = eng.take_augmented(dx, dy, np.array([2, 0]), mats)
    ld = eng.forward_backward(xa, ya).cpu().numpy()
    xh, yh = xa.cpu().numpy(), ya.cpu().numpy()
    assert not np.array_equal(yh, y[[2, 0]])
    r = LF.loss_and_grads(wts, xh, yh, "weighted_bce_dice_loss")
    plain = LF.loss_and_grads(wts, x[[2, 0]], y[[2, 0]], "weighted_bce_dice_loss")
    assert abs(ld[0] - r["loss"]) < 1e-5 and abs(ld[1] - r["dice"]) < 1e-5
    assert abs(plain["loss"] - r["loss"]) > 1e-4


@pytest.mark.parametrize("arch,dtype", [("unetpp", "fp32"), ("unet", "bf16")])
def test_unetpp_and_bf16_augmented_fits_run(arch, dtype):
    x, y = synthetic_ct(12, 32, seed=10)
    m = _model(arch=arch, dtype=dtype)
    h = m.fit(x, y, batch_size=6, epochs=2, shuffle_seed=2, augment=True, validation_data=(x[:4], y[:4])).history
    assert all(np.isfinite(v) for k in h for v in h[k])
    assert all(np.all(np.isfinite(v)) for v in m.get_weights().values())


# ----------------------------------------------------------------------------------------------- data parallel: 2 ranks on one GPU
def _dp_worker(rank, world, port, x, y, out):
    import torch.distributed as dist
    from covidseg_amd.keras_like import UNetModel, dp_shard
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    m = UNetModel(32, 1, seed=2, dropout_rate=0.0, process_group=dist.group.WORLD, device=0)
    m.verbose = 0
    m.compile(lr=0.0005)
    eng = m.backend
    # this rank's shard of the first batch of epoch 0, augmented: rows = its positions
    order = np.random.RandomState(5).permutation(len(x))
    sel, _ = dp_shard(order[:4], world, rank)
    pos, _ = dp_shard(np.arange(4), world, rank)
    table = eng.augment_table(AUG.AffineAugment().matrices(len(x), 5, 0, 32, 32))
    xa, ya = eng.take_augmented(eng.resident(x, max_fraction=1.0), eng.resident(y, max_fraction=1.0), sel, table[int(pos[0]):int(pos[0]) + len(pos)])
    hist = m.fit(x, y, batch_size=4, epochs=1, shuffle_seed=5, augment=True).history
    np.savez(out + f".{rank}.npz", xa=xa.cpu().numpy(), ya=ya.cpu().numpy(), loss=hist["loss"], dice=hist["dice_coeff"])
    dist.barrier(); dist.destroy_process_group()


def test_two_ranks_reproduce_the_single_process_augmented_fit(tmp_path):
    import torch.multiprocessing as mp
    from covidseg_amd.keras_like import UNetModel
    x, y = synthetic_ct(8, 32, seed=5)
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(2, _free_port(), x, y, out), nprocs=2, join=True)
    m = UNetModel(32, 1, seed=2, dropout_rate=0.0)
    m.verbose = 0
    m.compile(lr=0.0005)
    eng = m.backend
    order = np.random.RandomState(5).permutation(8)
    table = eng.augment_table(AUG.AffineAugment().matrices(8, 5, 0, 32, 32))
    xa, ya = eng.augment_batch(x[order[:4]], y[order[:4]], table[0:4])
    hist = m.fit(x, y, batch_size=4, epochs=1, shuffle_seed=5, augment=True).history
    for r in (0, 1):
        got = np.load(out + f".{r}.npz")
        assert np.array_equal(got["xa"], xa.cpu().numpy()[2 * r:2 * r + 2]) and np.array_equal(got["ya"], ya.cpu().numpy()[2 * r:2 * r + 2])
        assert abs(float(got["loss"][0]) - hist["loss"][0]) < 2e-5 and abs(float(got["dice"][0]) - hist["dice_coeff"][0]) < 2e-5

"""CPU: the augmentation policy (augment.py) and its wiring into UNetModel.fit / UNetModel.augment, without a GPU.
The matrices against explicit 3x3 products, the draw statistics, determinism, the float64 bilinear restatement against scipy.ndimage, a numpy backend that
implements the augmentation hook (fit augments exactly the training batches, with the rows of their positions), a 2-rank gloo fit, and the refusals."""
import json
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import augment_oracle as AO
from covidseg_amd import augment as AUG
from covidseg_amd import keras_like as KL
from test_dp_fit_cpu import ToyDPBackend, _data, _free_port


# ----------------------------------------------------------------------------------------------- policy and matrices
def test_defaults_are_the_reference_literals():
    p = AUG.AffineAugment()                                           # T1:547-583: Fliplr(0.5), Flipud(0.2), sometimes = Sometimes(0.5, ...)
    assert (p.fliplr, p.flipud, p.p_affine) == (0.5, 0.2, 0.5)
    assert p.scale == (0.8, 1.2) and p.translate == (-0.2, 0.2) and p.rotate == (-40.0, 40.0) and p.shear == (-16.0, 16.0)
    assert AUG.resolve(True).config() == p.config() and AUG.resolve(None) is None
    assert AUG.resolve(p.config()).config() == p.config()


@pytest.mark.parametrize("hw", [(224, 224), (61, 97)])
def test_matrices_are_the_explicit_products_for_every_order(hw):
    h, w = hw
    for pol in (AUG.AffineAugment(fliplr=1, flipud=1, p_affine=1), AUG.AffineAugment()):
        d = pol.sample(600, 11, 2)
        t = pol.matrices(600, 11, 2, h, w)
        assert t.dtype == np.float32 and t.shape == (600, 6)
        if pol.fliplr == 1:
            assert len({tuple(o) for o in d.order}) == 6                # every order of the three steps occurs
        for k in range(600):
            want = AO.sample_inverse(d, k, h, w).reshape(6)
            assert np.all(np.abs(t[k].astype(np.float64) - want) <= 1.2e-7 * np.abs(want) + 1e-9), (k, t[k], want)


def test_flip_rows_are_exact_integers():
    pol = AUG.AffineAugment(fliplr=0.5, flipud=0.5, p_affine=0.0)
    d, t = pol.sample(64, 3, 0), pol.matrices(64, 3, 0, 61, 97)
    for k in range(64):
        sx, ox = (-1.0, 96.0) if d.fliplr[k] else (1.0, 0.0)
        sy, oy = (-1.0, 60.0) if d.flipud[k] else (1.0, 0.0)
        assert np.array_equal(t[k], np.array([sx, 0, ox, 0, sy, oy], np.float32)), (k, t[k])


def test_draw_statistics():
    n = 200_000
    pol = AUG.AffineAugment()
    d = pol.sample(n, 7, 0)
    for got, p in ((d.fliplr.mean(), 0.5), (d.flipud.mean(), 0.2), (d.affine.mean(), 0.5)):
        assert abs(got - p) <= 4 * np.sqrt(p * (1 - p) / n), (got, p)
    for arr, (lo, hi) in ((d.scale_x, pol.scale), (d.scale_y, pol.scale), (d.translate_x, pol.translate), (d.translate_y, pol.translate),
                          (d.rotate, pol.rotate), (d.shear, pol.shear)):
        assert arr.min() >= lo and arr.max() <= hi
        assert abs(arr.mean() - (lo + hi) / 2) <= 4 * (hi - lo) / np.sqrt(12 * n)
    assert np.array_equal(np.sort(d.order, axis=1), np.broadcast_to(np.arange(3), (n, 3)))
    counts = np.unique(d.order[:, 0] * 9 + d.order[:, 1] * 3 + d.order[:, 2], return_counts=True)[1]
    assert len(counts) == 6 and np.all(np.abs(counts / n - 1 / 6) <= 4 * np.sqrt((1 / 6) * (5 / 6) / n))


def test_tables_are_deterministic_and_independent_of_batch_and_world():
    pol = AUG.AffineAugment()
    a, b = pol.matrices(100, 5, 3, 64, 64), pol.matrices(100, 5, 3, 64, 64)
    assert np.array_equal(a, b)
    assert np.array_equal(pol.matrices(37, 5, 3, 64, 64), a[:37])    # row k does not depend on how many rows are drawn
    assert not np.array_equal(pol.matrices(100, 5, 4, 64, 64), a) and not np.array_equal(pol.matrices(100, 6, 3, 64, 64), a)
    for world in (1, 2, 4):                                           # the rows the ranks use for one global batch are that batch's positions
        for i, bs in ((0, 8), (8, 8), (96, 4), (90, 10)):
            parts = [KL.dp_shard(np.arange(i, i + bs), world, r)[0] for r in range(world)]
            kw = KL.dp_shard(np.arange(i, i + bs), world, 0)[1]
            got = parts[0] if kw else np.concatenate(parts)
            assert np.array_equal(a[got], a[i:i + bs])


def test_policy_travels_to_data_parallel_ranks():
    from covidseg_amd import dp_launch
    pol = AUG.AffineAugment(fliplr=0.3, rotate=10)
    cfg = json.loads(json.dumps(dp_launch._jsonable({"augment": pol})))["augment"]
    assert AUG.resolve(cfg).config() == pol.config() and pol.rotate == (-10.0, 10.0)


@pytest.mark.parametrize("bad", [dict(fliplr=1.5), dict(flipud=-0.1), dict(p_affine=2), dict(scale=(1.2, 0.8)), dict(scale=(0.0, 1.0)),
                                 dict(translate=(0.2, -0.2)), dict(rotate=(10, -10)), dict(shear=(-90, 10)), dict(shear=(0, float("nan")))])
def test_bad_policy_arguments_raise(bad):
    with pytest.raises(ValueError):
        AUG.AffineAugment(**bad)
    with pytest.raises(ValueError):
        AUG.resolve("yes")


# ----------------------------------------------------------------------------------------------- the restated warps
def test_bilinear_restatement_matches_scipy_grid_constant():
    from scipy import ndimage
    rng = np.random.default_rng(0)
    pol = AUG.AffineAugment(fliplr=0.5, flipud=0.5, p_affine=1.0, translate=(-0.4, 0.4))
    for (h, w) in ((33, 33), (61, 97)):
        img = rng.standard_normal((h, w))
        for row in pol.matrices(12, 9, 0, h, w):
            m = row.astype(np.float64)
            want = ndimage.affine_transform(img, np.array([[m[4], m[3]], [m[1], m[0]]]), offset=(m[5], m[2]), output_shape=(h, w), order=1,
                                            mode="grid-constant", cval=0.0, prefilter=False)
            got = AO.warp_bilinear(img, row)[..., 0]
            assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


def test_nearest_restatement_reads_only_source_values():
    rng = np.random.default_rng(1)
    mask = (rng.random((40, 50)) > 0.5).astype(np.float32) * 3
    for row in AUG.AffineAugment(p_affine=1.0).matrices(8, 2, 0, 40, 50):
        out = AO.warp_nearest(mask, row)
        assert set(np.unique(out)) <= {0.0, 3.0}


# ----------------------------------------------------------------------------------------------- fit wiring on a numpy backend
class ToyAugBackend(ToyDPBackend):
    """ToyDPBackend plus the augmentation hook in numpy (augment_oracle's warps): records every table, every augmented batch and what train_batch got."""

    def __init__(self, pg=None):
        super().__init__(pg)
        self.tables, self.aug_calls, self.trained = [], [], []

    def augment_table(self, mats):
        t = np.array(mats, np.float32)
        self.tables.append(t)
        return t

    def augment_batch(self, xb, yb, mats):
        mats = np.asarray(mats)
        self.aug_calls.append((len(xb), mats.copy()))
        xa = np.stack([AO.warp_bilinear(xb[k], mats[k]).reshape(np.shape(xb)[1:]) for k in range(len(xb))]).astype(np.float32)
        ya = None if yb is None else np.stack([AO.warp_nearest(yb[k], mats[k]) for k in range(len(yb))]).astype(np.float32)
        return xa, ya

    def train_batch(self, x, y, training_dropout=True, replicated=False):
        self.trained.append((np.array(x), np.array(y)))
        return super().train_batch(x, y, training_dropout, replicated)


def _model(backend):
    m = KL.UNetModel.__new__(KL.UNetModel)
    m.h = m.w = 8; m.in_ch = 1; m.arch = "unet"; m.backend = backend; m.compiled = False; m.verbose = 0
    m.compile(lr=0.0005)
    backend.lr = 0.5
    return m


def test_fit_augments_exactly_the_training_batches_with_their_rows():
    x, y = _data()
    be = ToyAugBackend()
    m = _model(be)
    pol = AUG.AffineAugment(p_affine=0.8)
    m.fit(x[:16], y[:16], batch_size=6, epochs=2, validation_data=(x[16:], y[16:]), shuffle_seed=3, augment=pol, augment_seed=21)
    assert len(be.tables) == 2 and len(be.aug_calls) == len(be.trained) == 6           # one table per epoch; validation never augmented
    rng = np.random.RandomState(3)                                    # the shuffle is the one fit draws without augmentation
    c = 0
    for ep in range(2):
        order = rng.permutation(16)
        table = pol.matrices(16, 21, ep, 8, 8)
        assert np.array_equal(be.tables[ep], table)
        for i in range(0, 16, 6):
            idx = order[i:i + 6]
            n, rows = be.aug_calls[c]
            assert n == len(idx) and np.array_equal(rows, table[i:i + len(idx)])
            xt, yt = be.trained[c]
            want_x = np.stack([AO.warp_bilinear(x[j], table[i + k]) for k, j in enumerate(idx)]).astype(np.float32)
            want_y = np.stack([AO.warp_nearest(y[j], table[i + k]) for k, j in enumerate(idx)]).astype(np.float32)
            assert np.array_equal(xt, want_x) and np.array_equal(yt, want_y)
            c += 1
    assert [k for k, *_ in be.calls].count("predict") > 0


def test_augment_seed_defaults_to_shuffle_seed_and_none_never_calls_the_hook():
    x, y = _data()
    be = ToyAugBackend()
    _model(be).fit(x[:16], y[:16], batch_size=8, epochs=1, shuffle_seed=5, augment=True)
    assert np.array_equal(be.tables[0], AUG.AffineAugment().matrices(16, 5, 0, 8, 8))
    be2, plain = ToyAugBackend(), ToyDPBackend()
    h2 = _model(be2).fit(x[:16], y[:16], batch_size=8, epochs=2, shuffle_seed=5, validation_data=(x[16:], y[16:])).history
    h3 = _model(plain).fit(x[:16], y[:16], batch_size=8, epochs=2, shuffle_seed=5, validation_data=(x[16:], y[16:])).history
    assert be2.tables == [] and be2.aug_calls == [] and h2 == h3


def test_offline_augment_is_the_epoch_zero_table():
    x, y = _data()
    be = ToyAugBackend()
    m = _model(be)
    xa, ya = m.augment(x, y, seed=4, batch_size=5)
    t = AUG.AffineAugment().matrices(len(x), 4, 0, 8, 8)
    assert xa.shape == x.shape and ya.shape == y.shape and xa.dtype == np.float32
    for k in range(len(x)):
        assert np.array_equal(xa[k], AO.warp_bilinear(x[k], t[k]).astype(np.float32))
        assert np.array_equal(ya[k], AO.warp_nearest(y[k], t[k]).astype(np.float32))
    assert np.array_equal(m.augment(x, seed=4, batch_size=7), xa)     # images only, other chunking: the same rows


def test_backend_without_the_hook_is_refused():
    x, y = _data()
    m = _model(ToyDPBackend())
    with pytest.raises(ValueError, match="augmentation hook"):
        m.fit(x, y, batch_size=8, epochs=1, augment=True)
    with pytest.raises(ValueError, match="augmentation hook"):
        m.augment(x, y)
    with pytest.raises(ValueError):
        _model(ToyAugBackend()).fit(x, y, batch_size=8, epochs=1, augment="imgaug")


# ----------------------------------------------------------------------------------------------- data parallel (gloo, 2 ranks)
def _aug_fit(backend):
    x, y = _data()
    m = _model(backend)
    pol = AUG.AffineAugment(p_affine=0.7)
    # 16 samples, batch 6 -> 6, 6, 4 (2 ranks: 3 + 3, 3 + 3, 2 + 2); batch 5 -> 5, 5, 5, 1 (replicated)
    h1 = m.fit(x[:16], y[:16], batch_size=6, epochs=2, validation_data=(x[16:], y[16:]), shuffle_seed=3, augment=pol).history
    h2 = m.fit(x[:16], y[:16], batch_size=5, epochs=1, shuffle_seed=4, augment=pol, augment_seed=9).history
    return {"h1": h1, "h2": h2, "w": backend.w.tolist()}


def _worker(rank, world, port, workdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = _aug_fit(ToyAugBackend(dist.group.WORLD))
    with open(os.path.join(workdir, f"aug_rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier(); dist.destroy_process_group()


def test_two_rank_augmented_fit_equals_single_process_fit(tmp_path):
    single = _aug_fit(ToyAugBackend(None))
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in (0, 1):
        got = json.load(open(tmp_path / f"aug_rank{r}.json"))
        for hk in ("h1", "h2"):
            for k in single[hk]:
                np.testing.assert_allclose(got[hk][k], single[hk][k], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got["w"], single["w"], rtol=1e-12)

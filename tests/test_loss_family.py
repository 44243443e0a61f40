"""CPU tests of the selectable segmentation losses (compile(loss=...): bce_dice_loss, binary_crossentropy, dice_loss, tversky_loss): the float64
restatements against the reference's own functions (tests/golden/loss_family_goldens.npz), the closed-form logit gradients the engine computes
against autograd, and the Keras surface -- compile's names, training_config through save / load_model -- on an oracle-backed stub backend."""
import json
import os

import numpy as np
import pytest
import torch

import loss_family_oracle as LF
from covidseg_amd import _lib
from covidseg_amd import weights as W
from covidseg_amd.data import synthetic_ct
from covidseg_amd.keras_like import LOSSES, UNetModel, load_model
from oracle import unet_oracle as O
from oracle_backend import OracleBackend

HERE = os.path.dirname(os.path.abspath(__file__))


def T64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def test_restatements_reproduce_reference_goldens():
    z = np.load(os.path.join(HERE, "golden", "loss_family_goldens.npz"))
    for i in range(int(z["n_cases"])):
        t, p = T64(z[f"t{i}"]), T64(z[f"p{i}"])
        assert float(LF.dice_loss(t, p)) == pytest.approx(float(z[f"dice_loss{i}"]), rel=1e-10, abs=1e-14), i
        assert float(LF.tversky_loss(t, p)) == pytest.approx(float(z[f"tversky_loss{i}"]), rel=1e-10, abs=1e-14), i
        assert float(LF.weighted_bce_dice_loss(t, p)) == pytest.approx(float(z[f"weighted_bce_dice_loss{i}"]), rel=1e-10), i
        np.testing.assert_allclose(LF.avg_pool_same(t).numpy(), z[f"avg_pool{i}"], rtol=1e-12, atol=1e-15)


def test_loss_names_match_the_engine_enum():
    assert tuple(LOSSES) == tuple(LF.LOSSES) and set(_lib.LOSSES) == set(LOSSES) and _lib.LOSSES["bce_dice_loss"] == 0


def _cases(rng):
    out = []
    for shape in [(2, 8, 8, 1), (1, 24, 16, 1)]:
        t = np.round(rng.random(shape) ** 3 * 255) / 255.0
        t[rng.random(shape) < 0.5] = 0.0
        out.append((t, rng.standard_normal(shape) * 3))
    t = (rng.random((2, 8, 8, 1)) > 0.9).astype(np.float64)
    z = rng.standard_normal(t.shape) * 2
    z.flat[:3] = [40.0, -40.0, 16.5]                                  # logits whose p leaves the clip range (a = 0 there)
    out.append((t, z))
    out.append((np.zeros((1, 8, 8, 1)), rng.standard_normal((1, 8, 8, 1))))   # empty mask
    return out


@pytest.mark.parametrize("loss,ab", [("bce_dice_loss", (0.5, 0.5)), ("binary_crossentropy", (0.5, 0.5)), ("dice_loss", (0.5, 0.5)),
                                     ("tversky_loss", (0.5, 0.5)), ("tversky_loss", (0.7, 0.3)), ("tversky_loss", (0.2, 0.9)),
                                     ("weighted_bce_dice_loss", (0.5, 0.5))])
def test_closed_form_logit_gradient_matches_autograd(loss, ab):
    """dz = cb a + q (A t + B) with the batch scalars of include/unet_hip.h UNET_LOSS_* equals d loss / d logit of the float64 restatement"""
    rng = np.random.default_rng(7)
    for t, z in _cases(rng):
        zt = T64(z).requires_grad_(True)
        p = torch.sigmoid(zt)
        LF.loss_fn(loss, *ab)(T64(t), p).backward()
        got = LF.closed_form_dz(loss, t, p.detach().numpy(), *ab)
        want = zt.grad.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max() * want.size), (loss, ab)


def test_loss_values_of_the_selectable_losses():
    rng = np.random.default_rng(3)
    t = (rng.random((2, 8, 8, 1)) > 0.7).astype(np.float64); p = rng.random(t.shape)
    tt, pp = T64(t), T64(p)
    i, st, sp = (t * p).sum(), t.sum(), p.sum()
    assert float(LF.tversky_loss(tt, pp, 0.7, 0.3)) == pytest.approx(1 - i / (i + 0.7 * (sp - i) + 0.3 * (st - i)), rel=1e-12)
    assert float(LF.loss_fn("binary_crossentropy")(tt, pp)) == pytest.approx(float(O.binary_crossentropy_mean(tt, pp)), rel=1e-15)
    assert float(LF.loss_fn("bce_dice_loss")(tt, pp)) == pytest.approx(0.5 * float(O.binary_crossentropy_mean(tt, pp)) + 0.5 * float(LF.dice_loss(tt, pp)), rel=1e-12)


class LossOracleBackend(OracleBackend):
    """OracleBackend with set_loss: the oracle's step on the selected loss (tests/loss_family_oracle.py)"""

    def __init__(self, h, w, in_ch=1, dtype=torch.float64, arch="unet"):
        super().__init__(h, w, in_ch, dtype, arch)
        self.loss = ("bce_dice_loss", 0.5, 0.5)

    def set_weights(self, w):
        if self.tr is None:
            self.tr = LF.Trainer(w, *self.loss, dtype=self.dtype, arch=self.arch)
        else:
            super().set_weights(w)

    def set_loss(self, name, alpha=0.5, beta=0.5):
        if name not in LF.LOSSES:
            raise ValueError(name)
        self.loss = (name, float(alpha), float(beta))
        self.tr.loss, self.tr.alpha, self.tr.beta = self.loss

    def predict_batch(self, x, y=None):
        p, ld = super().predict_batch(x, y)
        if y is not None:
            ld[0] = float(LF.loss_fn(*self.loss)(T64(y), T64(p)))
        return p, ld


def small(backend_cls=LossOracleBackend, size=16):
    m = UNetModel(size, backend=backend_cls(size, size), seed=1)
    m.verbose = 0
    return m


def test_compile_accepts_the_loss_names_and_refuses_the_rest():
    m = small()
    for name in LOSSES:
        m.compile(loss=name)
        assert m.backend.loss[0] == name and m.loss == name and m.loss_config is None

    def tversky_loss(y_true, y_pred):                                  # a Keras-style callable: selected by its name
        raise AssertionError("never called")
    m.compile(loss=tversky_loss, loss_kwargs={"alpha": 0.7, "beta": 0.3})
    assert m.backend.loss == ("tversky_loss", 0.7, 0.3) and m.loss_config == {"alpha": 0.7, "beta": 0.3}
    m.compile()
    assert m.backend.loss == ("bce_dice_loss", 0.5, 0.5) and m.loss == "bce_dice_loss"
    for bad in ("mean_squared_error", "weighted_dice_loss", "focal", lambda a, b: a):
        with pytest.raises(ValueError):
            m.compile(loss=bad)
    with pytest.raises(ValueError):
        m.compile(loss="dice_loss", loss_kwargs={"alpha": 0.7})
    with pytest.raises(ValueError):
        m.compile(loss="tversky_loss", loss_kwargs={"gamma": 0.7})
    # a backend without set_loss (the plain oracle backend) keeps working for the default loss and refuses the others
    d = small(OracleBackend)
    d.compile(loss="bce_dice_loss")
    assert d.compiled
    with pytest.raises(ValueError, match="set_loss"):
        d.compile(loss="dice_loss")


def test_fit_reports_the_selected_loss():
    x, y = synthetic_ct(4, 16, seed=4)
    m = small()
    m.compile(loss="dice_loss")
    h = m.fit(x[:2], y[:2], batch_size=2, epochs=1, validation_data=(x[2:], y[2:]), shuffle=False)
    ref = LF.Trainer(small().get_weights(), "dice_loss")
    lv, dv = ref.train_step(x[:2], y[:2])
    assert h.history["loss"][0] == pytest.approx(lv, rel=1e-12) and h.history["dice_coeff"][0] == pytest.approx(dv, rel=1e-12)
    p = ref.predict(x[2:])
    assert h.history["val_loss"][0] == pytest.approx(float(LF.dice_loss(T64(y[2:]), T64(p))), rel=1e-9)


def test_training_config_round_trip(tmp_path):
    from covidseg_amd import hdf5_min as H5
    x, y = synthetic_ct(4, 16, seed=1)
    a = small()
    a.compile(lr=0.0005, loss="tversky_loss", loss_kwargs={"alpha": 0.7, "beta": 0.3})
    for _ in range(2):
        a.backend.train_batch(x, y)
    f = str(tmp_path / "tversky.hdf5")
    a.save(f)
    tc = json.loads(H5._strs(H5.read_file(f).attrs["training_config"])[0])
    assert tc["loss"] == "tversky_loss" and tc["loss_config"] == {"alpha": 0.7, "beta": 0.3}
    b = load_model(f, backend=LossOracleBackend(16, 16))
    assert b.compiled and b.loss == "tversky_loss" and b.backend.loss == ("tversky_loss", 0.7, 0.3) and b.backend.tr.t == 2
    for _ in range(2):
        a.backend.train_batch(x, y); b.backend.train_batch(x, y)
    wa, wb = a.get_weights(), b.get_weights()
    assert all(np.array_equal(wa[k], wb[k]) for k in wa)
    # every selectable name loads and resumes on that loss; the default Tversky weights write no loss_config
    for name in LOSSES:
        a.compile(loss=name); a.save(f)
        tc = json.loads(H5._strs(H5.read_file(f).attrs["training_config"])[0])
        assert tc["loss"] == name and "loss_config" not in tc
        assert load_model(f, backend=LossOracleBackend(16, 16)).backend.loss == (name, 0.5, 0.5)
    # a file naming any other loss is still refused unless compile=False
    opt = a.backend.get_optimizer_state()
    W.save_weights(f, a.get_weights(), 1, "unet", (16, 16), full_model=True, optimizer=dict(opt, loss="weighted_dice_loss"))
    with pytest.raises(ValueError, match="weighted_dice_loss"):
        load_model(f, backend=LossOracleBackend(16, 16))
    assert not load_model(f, backend=LossOracleBackend(16, 16), compile=False).compiled

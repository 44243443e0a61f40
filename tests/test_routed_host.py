"""CPU: the host halves of the routed two-model system (routed.py, cluster.Router) on the CPU oracle backend, with the float64 routing oracle
(tests/route_oracle.py) as the backend's route hook; the (C, H, W) -> (H, W, C) component permutation; Keras' binary accuracy in evaluate."""
import contextlib
import io
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from covidseg_amd import cluster  # noqa: E402
from covidseg_amd.data import synthetic_ct  # noqa: E402
from covidseg_amd.keras_like import UNetModel, binary_matches  # noqa: E402
from covidseg_amd.routed import ClusterRoutedModel  # noqa: E402
from tests import cluster_oracle as CO  # noqa: E402
from tests import route_oracle as RO  # noqa: E402
from tests.oracle_backend import OracleBackend  # noqa: E402

try:
    from sklearn.cluster import KMeans as SKKMeans
    from sklearn.decomposition import PCA as SKPCA
    HAVE_SK = True
except ImportError:
    HAVE_SK = False

S = 16                                                    # c5a of a 16 x 16 U-Net: 1 x 1 x 512


class RoutedOracleBackend(OracleBackend):
    """OracleBackend plus the two hooks routed.py asks of a backend: spawn (an expert's backend) and route_taps (here the float64 oracle of
    unet_cluster_route on the last forward's tap).  `forced`: labels to return instead (a callable of n), for the grouping cases."""

    forced = None

    def spawn(self, seed=0):
        return RoutedOracleBackend(self.h, self.w, self.in_ch, self.dtype, self.arch)

    def route_taps(self, router, n, name):
        if self.forced is not None:
            return self.forced(n)
        taps = self._last_acts[name]
        assert len(taps) == n
        return RO.route(taps, router.components_chw(), router.mean64, router.centres.cpu().numpy())[1]


def _base(seed=1, arch="unet"):
    m = UNetModel(S, 1, backend=RoutedOracleBackend(S, S, arch=arch), seed=seed, arch=arch)
    m.compile(lr=0.0005)
    m.verbose = 0
    return m


def _routed(base, x, k=4):
    rm = ClusterRoutedModel(base, n_components=k)
    f = base.feature_matrix("conv2d_9", x).numpy()
    pca = RO.OraclePCA(k).fit(f)
    km = RO.OracleKMeans(2, 0).fit(pca.transform(f))
    hwc = base.intermediate_output("conv2d_9", x[:1]).shape[1:]
    return rm.set_router(pca, km, hwc, device="cpu"), pca, km


def _distinct_experts(rm):
    """experts with weights of their own (fresh seeds) without training"""
    for j in range(rm.n_clusters):
        rm.experts[j] = rm._new_expert(j, "fresh")
        rm.expert_source[j] = "trained-from-fresh"


def test_component_permutation_equals_rollaxis_flatten():
    r = np.random.RandomState(0)
    n, h, w, c, k = 5, 3, 4, 6, 7
    taps = r.randn(n, h, w, c)
    comps = r.randn(k, c * h * w)
    flat = RO.flatten_chw(taps)
    np.testing.assert_array_equal(cluster.chw_to_hwc(flat, (h, w, c)), taps.reshape(n, -1))
    np.testing.assert_array_equal(cluster.hwc_to_chw(cluster.chw_to_hwc(comps, (h, w, c)), (h, w, c)), comps)
    got = taps.reshape(n, -1) @ cluster.chw_to_hwc(comps, (h, w, c)).T
    np.testing.assert_allclose(got, flat @ comps.T, rtol=1e-13, atol=1e-13)
    t = torch.from_numpy(comps)
    np.testing.assert_array_equal(cluster.chw_to_hwc(t, (h, w, c)).numpy(), cluster.chw_to_hwc(comps, (h, w, c)))
    np.testing.assert_array_equal(cluster.hwc_to_chw(cluster.chw_to_hwc(t, (h, w, c)), (h, w, c)).numpy(), comps)


def test_router_oracle_equals_kmeans_predict_of_pca_transform():
    r = np.random.RandomState(3)
    h, w, c, k = 2, 3, 8, 5
    fit = np.concatenate([r.randn(40, h, w, c) + 2.0, r.randn(30, h, w, c) - 1.0])
    new = r.randn(25, h, w, c) * 1.5 + 0.5
    X, Y = RO.flatten_chw(fit), RO.flatten_chw(new)
    if HAVE_SK:
        pca = SKPCA(k, svd_solver="full").fit(X)
        km = SKKMeans(2, random_state=0).fit(pca.transform(X))
        want = km.predict(pca.transform(Y))
        comps, mean, cen = pca.components_, pca.mean_, km.cluster_centers_
    else:
        o = CO.pca(X, k)
        comps, mean = o["components_"], o["mean_"]
        km = RO.OracleKMeans(2, 0).fit(o["transform"])
        cen = km._centres64
        want = km.predict((Y - mean) @ comps.T)
    proj, lab, dist = RO.route(new, comps, mean, cen)
    np.testing.assert_array_equal(lab, want)
    np.testing.assert_allclose(dist, ((proj - cen[lab]) ** 2).sum(1), rtol=1e-12)


def test_router_arrays_round_trip_on_host():
    r = np.random.RandomState(1)
    h, w, c, k = 2, 2, 4, 3
    comps, mean, cen = r.randn(k, h * w * c).astype(np.float32), r.randn(h * w * c), r.randn(2, k)
    ro = cluster.Router.from_arrays(comps, mean, cen, (h, w, c), "conv2d_9", np.array([0.5, 0.2, 0.1]), device="cpu")
    np.testing.assert_array_equal(ro.comps_hwc.numpy(), cluster.chw_to_hwc(comps, (h, w, c)))
    np.testing.assert_array_equal(ro.mu_hwc.numpy(), cluster.chw_to_hwc(mean, (h, w, c)).astype(np.float32))
    a = ro.arrays()
    np.testing.assert_array_equal(a["components"], comps)
    np.testing.assert_array_equal(a["mean"], mean)
    np.testing.assert_array_equal(a["centres"], cen)
    assert tuple(a["tap_shape"]) == (h, w, c) and str(a["layer"]) == "conv2d_9" and int(a["format"]) == 1
    with pytest.raises(ValueError):
        cluster.Router.from_arrays(comps, mean, r.randn(17, k), (h, w, c), device="cpu")
    with pytest.raises(ValueError):
        cluster.Router.from_arrays(comps, mean, cen, (h, w, c + 1), device="cpu")


def test_routed_predict_groups_and_scatters_in_input_order():
    x, _ = synthetic_ct(11, S, seed=4)
    base = _base()
    rm, _, _ = _routed(base, x)
    _distinct_experts(rm)
    got = rm.predict(x, batch_size=4)
    assert got.shape == base.predict(x).shape
    labels = rm.route(x, batch_size=4)
    assert set(labels.tolist()) == {0, 1}
    want = np.empty_like(got)
    for i in range(0, len(x), 4):
        xb, lb = x[i:i + 4], labels[i:i + 4]
        for j in (0, 1):
            idx = np.where(lb == j)[0]
            if len(idx):
                want[i + idx] = rm.experts[j].predict(xb[idx], batch_size=len(idx))
    np.testing.assert_array_equal(got, want)
    assert np.abs(got - base.predict(x)).max() > 0


def test_forced_labels_interleaved_groups():
    x, _ = synthetic_ct(7, S, seed=5)
    base = _base()
    rm, _, _ = _routed(base, x)
    _distinct_experts(rm)
    pattern = np.array([1, 0, 0, 1, 0, 1, 1], np.int32)
    base.backend.forced = lambda n: pattern[:n]
    got = rm.predict(x, batch_size=7)
    p0, p1 = rm.experts[0].predict(x[pattern == 0], 7), rm.experts[1].predict(x[pattern == 1], 7)
    np.testing.assert_array_equal(got[pattern == 0], p0)
    np.testing.assert_array_equal(got[pattern == 1], p1)


def test_all_one_cluster_batch_and_empty_cluster_falls_back_to_base(capsys):
    x, y = synthetic_ct(6, S, seed=6)
    base = _base()
    rm, _, _ = _routed(base, x)
    base.backend.forced = lambda n: np.ones(n, np.int32)
    hists = rm.fit(x, y, init="fresh", batch_size=3, epochs=1, validation_data=(x[:2], y[:2]))
    assert "cluster 0 has no training rows" in capsys.readouterr().out
    assert hists[0] is None and hists[1] is not None
    assert rm.experts[0] is base and rm.expert_source == ["base", "trained-from-fresh"]
    np.testing.assert_array_equal(rm.predict(x, batch_size=4), rm.experts[1].predict(x, batch_size=4))
    ev = rm.evaluate(x, y, batch_size=4)
    assert ev["per_cluster"][0] is None and ev["counts"] == [0, 6]


def test_fit_trains_each_expert_on_its_rows_with_prefixed_checkpoints(tmp_path):
    x, y = synthetic_ct(8, S, seed=7)
    base = _base()
    rm, _, _ = _routed(base, x)
    pattern = np.array([0, 1, 1, 0, 1, 0, 0, 1], np.int32)
    base.backend.forced = lambda n: pattern[:n]
    w0 = base.get_weights()
    fd, fl = str(tmp_path / "d.hdf5"), str(tmp_path / "l.hdf5")
    rm.fit(x, y, init="base", batch_size=8, epochs=1, validation_data=(x, y), checkpoint_dice=fd, checkpoint_loss=fl)
    assert rm.expert_source == ["trained-from-base", "trained-from-base"]
    for j in (0, 1):
        assert os.path.exists(tmp_path / f"cluster{j}_d.hdf5") and os.path.exists(tmp_path / f"cluster{j}_l.hdf5")
        ref = UNetModel(S, 1, backend=RoutedOracleBackend(S, S), seed=0)
        ref.set_weights(w0)
        ref.compile(lr=0.0005)
        ref.verbose = 0
        ref.fit(x[pattern == j], y[pattern == j], batch_size=8, epochs=1)
        for name, v in ref.get_weights().items():
            np.testing.assert_array_equal(rm.experts[j].get_weights()[name], v, err_msg=name)
    for name, v in base.get_weights().items():                                      # the base is untouched
        np.testing.assert_array_equal(v, w0[name])
    with pytest.raises(ValueError):
        rm.fit(x, y, init="other")


def test_refusals():
    base = _base()
    base.backend._dp, base.backend.world, base.backend.rank = True, 2, 0
    with pytest.raises(ValueError, match="world size"):
        ClusterRoutedModel(base)
    base.backend._dp = False
    cls = type("Cls", (), {"arch": "classifier", "backend": base.backend})()
    with pytest.raises(ValueError, match="U-Net"):
        ClusterRoutedModel(cls)
    with pytest.raises(RuntimeError):
        ClusterRoutedModel(base).predict(np.zeros((1, S, S, 1), np.float32))


def test_save_load_round_trip(tmp_path):
    x, y = synthetic_ct(9, S, seed=8)
    base = _base()
    rm, pca, km = _routed(base, x)
    _distinct_experts(rm)
    rm.save(str(tmp_path / "m"))
    for f in ("base.h5", "expert_0.h5", "expert_1.h5", "router.npz", "manifest.json"):
        assert os.path.exists(tmp_path / "m" / f), f
    z = np.load(tmp_path / "m" / "router.npz")
    np.testing.assert_array_equal(z["components"], np.asarray(pca.components_, np.float32))
    np.testing.assert_array_equal(z["mean"], pca.mean_)
    np.testing.assert_array_equal(z["centres"], km._centres64)
    back = ClusterRoutedModel.load(str(tmp_path / "m"), backend=lambda: RoutedOracleBackend(S, S))
    assert back.expert_source == rm.expert_source and back.router.tap_shape == rm.router.tap_shape
    np.testing.assert_array_equal(back.route(x, 4), rm.route(x, 4))
    np.testing.assert_array_equal(back.predict(x, 4), rm.predict(x, 4))


def test_routed_evaluate_whole_set_and_per_cluster():
    x, y = synthetic_ct(10, S, seed=9)
    base = _base()
    rm, _, _ = _routed(base, x)
    _distinct_experts(rm)
    ev = rm.evaluate(x, y, batch_size=4, thresholds=(0.3, 0.547))
    assert "loss" not in ev["whole"]
    p = rm.predict(x, batch_size=4)
    from oracle import unet_oracle as O
    from covidseg_amd.keras_like import sm_scores
    sc = [sm_scores(*(O.threshold_sums(y[i:i + 4], p[i:i + 4], [0.3, 0.547]).T)) for i in range(0, 10, 4)]
    for key in ("dice", "iou", "precision", "recall"):
        np.testing.assert_allclose(ev["whole"][key], np.mean([s[key] for s in sc], axis=0), rtol=1e-12)
    assert ev["whole"]["accuracy"] == RO.binary_accuracy([p], [y])
    labels = rm.route(x, 4)
    np.testing.assert_array_equal(ev["labels"], labels)
    for j in (0, 1):
        sel = np.where(labels == j)[0]
        e = rm.experts[j].evaluate(x[sel], y[sel], batch_size=4, thresholds=[0.3], accuracy=True)
        assert ev["per_cluster"][j] == [float(e["loss"]), float(e["dice"][0]), float(e["iou"][0]), float(e["accuracy"])]


# ---- Keras' binary accuracy ------------------------------------------------------------------------------------------------------------------

class _FixedP:
    """a backend whose prediction of a row is a fixed array, the row picked by the id written in pixel [0, 0, 0] of the input"""

    def __init__(self, p):
        self.p = p
        self.lr = 0.0005

    def set_weights(self, w):
        pass

    def reset_optimizer(self):
        pass

    def predict_batch(self, x, y=None):
        p = self.p[np.asarray(x)[:, 0, 0, 0].astype(int)]
        return p, np.array([0.25, 0.5])


def test_binary_matches_crafted_cases():
    p = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.2, 0.9, 0.9, 0.1], np.float32)
    y = np.array([0.0, 1.0, 0.0, 1.0, 0.7, 0.3], np.float32)
    assert binary_matches(p, y) == 4                                               # p = 0.5 is "0"; fractional y never matches
    assert binary_matches(torch.from_numpy(p), y).item() == 4
    assert binary_matches(torch.from_numpy(p), torch.from_numpy(y)).item() == 4


def test_evaluate_accuracy_is_a_pixel_mean_over_the_set():
    r = np.random.RandomState(2)
    n = 5
    p = r.rand(n, S, S, 1).astype(np.float32)
    p[0, :4, :4] = 0.5
    y = (r.rand(n, S, S, 1) > 0.5).astype(np.float32)
    y[1, :3] = 0.5
    y[4] = (p[4] > 0.5)                                                            # a batch of its own, all matching
    x = np.zeros((n, S, S, 1), np.float32)
    x[:, 0, 0, 0] = np.arange(n)
    m = UNetModel(S, 1, backend=_FixedP(p), seed=0)
    plain = m.evaluate(x, y, batch_size=2)
    ev = m.evaluate(x, y, batch_size=2, accuracy=True)
    assert set(plain) == {"loss", "dice_coeff"} and set(ev) == {"loss", "dice_coeff", "accuracy"}
    want = RO.binary_accuracy([p[0:2], p[2:4], p[4:5]], [y[0:2], y[2:4], y[4:5]])
    assert ev["accuracy"] == want
    per_batch = np.mean([RO.binary_accuracy([p[i:i + 2]], [y[i:i + 2]]) for i in (0, 2, 4)])
    assert abs(per_batch - want) > 1e-3                                            # unequal batches: not a mean of batch means
    assert ev["accuracy"] == m.evaluate(x, y, batch_size=5, accuracy=True)["accuracy"]


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------

def _run(tmp, monkeypatch, **kw):
    from covidseg_amd.runners import holdout_runner_unet_infection_segmentation
    monkeypatch.setattr(cluster, "PCA", RO.OraclePCA)
    monkeypatch.setattr(cluster, "KMeans", RO.OracleKMeans)
    x, y = synthetic_ct(12, S, seed=3)
    os.makedirs(tmp, exist_ok=True)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = holdout_runner_unet_infection_segmentation(data=(x, y), epochs=1, batch_size=4, workdir=str(tmp), verbose=0,
                                                         backend=RoutedOracleBackend(S, S), **kw)
    return out, buf.getvalue()


def test_runner_route_true(tmp_path, monkeypatch):
    out, txt = _run(tmp_path, monkeypatch, route=True, cluster_components=4)
    assert "cluster" in out and "routed" in out
    ro = out["routed"]
    for s in ("Routed training rows per cluster:", "routed test dice coefficient, test iou, test accuracy:"):
        assert s in txt, s
    assert sum(ro["label_counts"]) == 8 and sum(ro["valid_label_counts"]) == 4
    assert len(ro["expert_source"]) == 2 and len(ro["whole"]) == 3
    rm = ro["model"]
    from covidseg_amd.data import train_test_split
    x, y = synthetic_ct(12, S, seed=3)
    _, xv, _, yv = train_test_split(x, y, test_size=0.3, random_state=42)
    np.testing.assert_array_equal(ro["valid_labels"], rm.route(xv))
    for j, sc in enumerate(ro["scores"]):
        sel = np.where(ro["valid_labels"] == j)[0]
        if len(sel) == 0:
            assert sc is None
            continue
        e = rm.experts[j].evaluate(xv[sel], yv[sel], batch_size=32, thresholds=[0.547], accuracy=True)
        assert sc == [float(e["loss"]), float(e["dice"][0]), float(e["iou"][0]), float(e["accuracy"])]
        assert f"routed cluster {j} test loss, test dice coefficient, test iou, test accuracy:" in txt
    for j, src in enumerate(ro["expert_source"]):
        if src != "base":
            assert os.path.exists(tmp_path / f"cluster{j}_unet_covid_weights_dice_coeff.hdf5")


def test_runner_route_false_is_unchanged(tmp_path, monkeypatch):
    a, ta = _run(tmp_path / "a", monkeypatch, cluster=True, cluster_components=4)
    b, tb = _run(tmp_path / "b", monkeypatch, cluster=True, cluster_components=4, route=False)
    assert ta == tb and "routed" not in ta and "Routed" not in ta
    assert set(a) == set(b) and "routed" not in a
    assert all(s is None or len(s) == 3 for s in a["cluster"]["scores"])
    assert a["cluster"]["scores"] == b["cluster"]["scores"] and a["score"] == b["score"]
    c, tc = _run(tmp_path / "c", monkeypatch)
    assert "cluster" not in c and "routed" not in c and "Extracted feature shape" not in tc

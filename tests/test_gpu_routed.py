"""GPU: unet_cluster_route (csrc/kernels_cluster.hip) through cluster.Router against float64, its batch independence, its agreement with the
fit path, and the routed two-model system (routed.ClusterRoutedModel): predict, save / load, evaluate(accuracy=True) and the runner."""
import contextlib
import io
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from covidseg_amd import cluster  # noqa: E402
from covidseg_amd.data import synthetic_ct  # noqa: E402
from covidseg_amd.keras_like import UNetModel  # noqa: E402
from covidseg_amd.routed import ClusterRoutedModel  # noqa: E402
from tests import cluster_oracle as CO  # noqa: E402
from tests import route_oracle as RO  # noqa: E402
from tests.gpu_util import elem_ratio  # noqa: E402


def _case(n, h, w, c, ld, k, nc, bf16, seed, big=False):
    """a strided NHWC tap view (pixel stride ld), and a Router of random components / mean / centres"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = h * w * c
    buf = torch.randn((n, h, w, ld), generator=g, device="cuda", dtype=torch.float32).relu_() * 2.0
    tap = buf.to(torch.bfloat16)[..., :c] if bf16 else buf[..., :c]
    comps = torch.randn((k, d), generator=g, device="cuda", dtype=torch.float32)
    if not big:
        comps = comps.cpu().numpy()
    mean = np.random.RandomState(seed).rand(d) * 1.5
    r = np.random.RandomState(seed + 1)
    centres = r.randn(nc, k) * 3.0
    router = cluster.Router.from_arrays(comps, mean, centres, (h, w, c), device="cuda")
    return tap, router


def _want(tap, router):
    """float64 projections of the kernel's operands (tap widened to fp32, the fp32 mean subtracted in fp32) and A1 = sum |x - mu| |w|"""
    x = (tap.float().reshape(tap.shape[0], -1) - router.mu_hwc[None, :]).double()
    w = router.comps_hwc.double()
    return (x @ w.T).cpu().numpy(), (x.abs() @ w.abs().T).cpu().numpy()


CASES = [  # n, h, w, c, ld, k, nc, bf16
    (1, 14, 14, 32, 32, 1, 2, False),
    (7, 14, 14, 32, 36, 17, 3, False),
    (32, 14, 14, 32, 32, 1000, 2, False),
    (33, 7, 7, 64, 64, 1000, 8, False),
    (32, 14, 14, 32, 32, 1000, 2, True),
    (33, 14, 14, 32, 40, 17, 3, True),
    (7, 5, 7, 5, 7, 17, 8, False),                                                  # c % 16 != 0: the element-wise path
    (32, 6, 6, 48, 51, 1000, 2, False),                                             # odd pixel stride
]


@pytest.mark.parametrize("n,h,w,c,ld,k,nc,bf16", CASES)
def test_route_projections_labels_distances(n, h, w, c, ld, k, nc, bf16):
    tap, router = _case(n, h, w, c, ld, k, nc, bf16, seed=n + k + c)
    assert tap.stride(2) == ld
    labels, dist, proj = router.assign(tap, want_proj=True)
    want, a1 = _want(tap, router)
    assert elem_ratio(proj.cpu().numpy(), want, a1) <= 1.0
    p64 = proj.double().cpu().numpy()
    wl, wd = CO.assign(p64, router.centres.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), wl)
    np.testing.assert_allclose(dist.cpu().numpy(), wd, rtol=1e-12)
    l2, d2, p2 = router.assign(tap)
    assert p2 is None
    np.testing.assert_array_equal(l2.cpu().numpy(), labels.cpu().numpy())
    np.testing.assert_array_equal(d2.cpu().numpy(), dist.cpu().numpy())


@pytest.mark.parametrize("bf16", [False, True])
def test_route_rows_are_batch_independent_and_reruns_bitwise(bf16):
    tap, router = _case(33, 14, 14, 32, 36, 1000, 2, bf16, seed=5)
    lab, dist, proj = (t.cpu().numpy() for t in router.assign(tap, want_proj=True))
    again = [t.cpu().numpy() for t in router.assign(tap, want_proj=True)]
    for a, b in zip((lab, dist, proj), again):
        np.testing.assert_array_equal(a, b)
    for i in range(33):
        li, di, pi = (t.cpu().numpy() for t in router.assign(tap[i:i + 1], want_proj=True))
        assert li[0] == lab[i] and di[0] == dist[i]
        np.testing.assert_array_equal(pi[0], proj[i])
    li, di, pi = (t.cpu().numpy() for t in router.assign(tap[5:12], want_proj=True))
    np.testing.assert_array_equal(pi, proj[5:12])


def test_route_components_over_2gib():
    k, h, w, c = 17, 256, 256, 512                                                   # comps_hwc 17 x 2^25 fp32 = 2.28 GB
    tap, router = _case(2, h, w, c, c, k, 2, False, seed=9, big=True)
    assert router.comps_hwc.numel() * 4 > 2 ** 31
    labels, dist, proj = router.assign(tap, want_proj=True)
    want, a1 = _want(tap, router)
    assert elem_ratio(proj.cpu().numpy(), want, a1) <= 1.0
    wl, wd = CO.assign(proj.double().cpu().numpy(), router.centres.cpu().numpy())
    np.testing.assert_array_equal(labels.cpu().numpy(), wl)


def test_route_bad_arguments():
    from covidseg_amd import _lib
    tap, router = _case(4, 4, 4, 16, 16, 5, 2, False, seed=1)
    lib, ctx = _lib.load(), _lib.Context.get(torch.cuda.current_device())
    lab = torch.empty(4, dtype=torch.int32, device="cuda"); dist = torch.empty(4, dtype=torch.float64, device="cuda")
    need = lib.unet_cluster_route_workspace(4, 256, 5)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nc=2, k=5, ld=16, nbytes=need):
        return lib.unet_cluster_route(ctx.handle, tap.data_ptr(), 0, 4, 4, 4, 16, ld, router.comps_hwc.data_ptr(), router.mu_hwc.data_ptr(), k,
                                      router.centres.data_ptr(), nc, None, lab.data_ptr(), dist.data_ptr(), ws.data_ptr(), nbytes, s)
    assert call() == 0
    for bad in (dict(nc=0), dict(nc=17), dict(k=0), dict(ld=15), dict(nbytes=need - 8)):
        assert call(**bad) == -1, bad


def _small_model(arch="unet", bf16=False, seed=2, size=64):
    kw = {"dtype": "bf16"} if bf16 else {}
    m = UNetModel(size, 1, seed=seed, arch=arch, **kw)
    m.compile(lr=0.0005)
    m.verbose = 0
    return m


def test_routed_labels_agree_with_the_fit_path():
    x, _ = synthetic_ct(64, 64, seed=3)
    m = _small_model()
    rm = ClusterRoutedModel(m, n_components=40).fit_router(x)
    data = m.feature_matrix("conv2d_9", x)
    pca = cluster.PCA(40).fit(data)
    km = cluster.KMeans(2, random_state=0).fit(pca.transform(data))
    got = rm.route(x, batch_size=16)
    pts = pca.transform(data).double().cpu().numpy()
    d = ((pts[:, None, :] - km._centres64[None]) ** 2).sum(2)
    margin = np.abs(d[:, 0] - d[:, 1]) / d.max(1)
    differ = got != km.labels_
    assert not np.any(differ & (margin >= 1e-4)), np.where(differ)[0]
    assert len(set(got.tolist())) == 2


@pytest.mark.parametrize("arch,bf16", [("unet", False), ("unet", True), ("unetpp", False)])
def test_routed_predict_equals_experts_on_their_groups(arch, bf16):
    x, _ = synthetic_ct(40, 64, seed=4)
    m = _small_model(arch, bf16)
    rm = ClusterRoutedModel(m, n_components=30).fit_router(x[:32])
    for j in range(2):
        rm.experts[j] = rm._new_expert(j, "fresh")
    got = rm.predict(x, batch_size=16)
    labels = rm.route(x, batch_size=16)
    want = np.empty_like(got)
    for i in range(0, len(x), 16):
        xb, lb = x[i:i + 16], labels[i:i + 16]
        for j in range(2):
            idx = np.where(lb == j)[0]
            if len(idx):
                want[i + idx] = rm.experts[j].predict(xb[idx], batch_size=len(idx))
    np.testing.assert_array_equal(got, want)
    assert got.shape == m.predict(x).shape
    assert np.abs(got - m.predict(x)).max() > 1e-4


def test_save_and_reload_are_bit_identical():
    x, y = synthetic_ct(24, 64, seed=5)
    m = _small_model()
    rm = ClusterRoutedModel(m, n_components=20).fit_router(x)
    rm.fit(x, y, init="fresh", batch_size=8, epochs=1)
    d = tempfile.mkdtemp()
    rm.save(d)
    back = ClusterRoutedModel.load(d)
    np.testing.assert_array_equal(back.route(x), rm.route(x))
    np.testing.assert_array_equal(back.predict(x), rm.predict(x))


def test_evaluate_accuracy_equals_the_keras_restatement():
    x, y = synthetic_ct(21, 64, seed=6)
    m = _small_model()
    plain = m.evaluate(x, y, batch_size=8, thresholds=[0.5])
    ev = m.evaluate(x, y, batch_size=8, thresholds=[0.5], accuracy=True)
    assert set(plain) == {"loss", "dice_coeff", "dice", "iou", "precision", "recall"}
    assert set(m.evaluate(x, y, batch_size=8)) == {"loss", "dice_coeff"}
    p = m.predict(x, batch_size=8)
    assert ev["accuracy"] == RO.binary_accuracy([p[i:i + 8] for i in range(0, 21, 8)], [y[i:i + 8] for i in range(0, 21, 8)])
    for key in plain:
        np.testing.assert_array_equal(plain[key], ev[key])


def test_runner_route_option():
    from covidseg_amd import runners
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = runners.holdout_runner_unet_infection_segmentation(input_size=64, epochs=1, n_samples=48, batch_size=8, verbose=0, route=True,
                                                                 workdir=tempfile.mkdtemp())
    text = buf.getvalue()
    assert "Label count for Kmeans on cts:" in text and "routed test dice coefficient, test iou, test accuracy:" in text
    ro = out["routed"]
    assert sum(ro["label_counts"]) == 33 and sum(ro["valid_label_counts"]) == 15
    assert len(ro["scores"]) == 2 and len(ro["expert_source"]) == 2
    for j, sc in enumerate(ro["scores"]):
        if ro["valid_label_counts"][j]:
            assert len(sc) == 4 and 0.0 <= sc[3] <= 1.0
        else:
            assert sc is None
    assert 0.0 <= ro["whole"][2] <= 1.0

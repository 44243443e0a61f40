"""GPU: the feature-tap PCA / KMeans kernels (csrc/kernels_cluster.hip) against float64, cluster.PCA / cluster.KMeans against the float64 oracle
(tests/cluster_oracle.py), UNetModel.feature_matrix, and the runner's cluster=True path."""
import io
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from covidseg_amd import cluster  # noqa: E402
from tests import cluster_oracle as CO  # noqa: E402
from tests.gpu_util import elem_ratio  # noqa: E402


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _nt_ref(a, b, mu_a, mu_b):
    """float64 product and A1 = sum |a - mu_a| |b - mu_b| on the device (the operands as the kernel sees them: fp32 values, fp64 means)"""
    ac = a.double() - (mu_a[None, :] if mu_a is not None else 0.0)
    bc = b.double() - (mu_b[None, :] if mu_b is not None else 0.0)
    return (ac @ bc.T).cpu().numpy(), (ac.abs() @ bc.abs().T).cpu().numpy()


def test_col_mean_matches_float64():
    r = np.random.RandomState(0)
    for n, d in ((1, 7), (37, 1000), (300, 5003)):
        x = (r.randn(n, d) * 3 + 1).astype(np.float32)
        got = cluster.col_mean(_dev(x)).cpu().numpy()
        want = x.astype(np.float64).mean(axis=0)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(x).mean()


@pytest.mark.parametrize("m,p,d", [(1, 1, 7), (37, 53, 7), (129, 200, 1000), (130, 67, 100352), (300, 300, 1000)])
@pytest.mark.parametrize("means", [False, True])
def test_gemm_nt_cross_matches_float64(m, p, d, means):
    r = np.random.RandomState(m + p + d)
    a, b = _dev(r.randn(m, d) + 0.5), _dev(r.randn(p, d) - 0.25)
    mu_a = cluster.col_mean(a) if means else None
    mu_b = cluster.col_mean(b) if means else None
    got = cluster.gemm_nt(a, b, mu_a, mu_b, out_dtype=torch.float64).cpu().numpy()
    want, a1 = _nt_ref(a, b, mu_a, mu_b)
    assert elem_ratio(got, want, a1) <= 1.0
    got32 = cluster.gemm_nt(a, b, mu_a, mu_b).cpu().numpy()
    assert elem_ratio(got32, want, a1) <= 1.0
    again = cluster.gemm_nt(a, b, mu_a, mu_b, out_dtype=torch.float64).cpu().numpy()
    np.testing.assert_array_equal(again, got)                                       # bit-identical rerun


@pytest.mark.parametrize("n,d", [(5, 7), (261, 1000), (150, 100352)])
def test_gemm_nt_gram_is_exactly_symmetric(n, d):
    r = np.random.RandomState(n)
    x = _dev(r.randn(n, d) * 2 + 1)
    mu = cluster.col_mean(x)
    g = cluster.gemm_nt(x, x, mu, mu, sym=True, out_dtype=torch.float64).cpu().numpy()
    want, a1 = _nt_ref(x, x, mu, mu)
    assert elem_ratio(g, want, a1) <= 1.0
    np.testing.assert_array_equal(g, g.T)
    np.testing.assert_array_equal(cluster.gemm_nt(x, x, mu, mu, sym=True, out_dtype=torch.float64).cpu().numpy(), g)


def test_gemm_nt_over_2gib():
    n, d = 40, (1 << 31) // (4 * 40) + 4099                                         # 2^31 bytes + a ragged tail
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    mu = cluster.col_mean(x)
    got = cluster.gemm_nt(x, x, mu, mu, sym=True, out_dtype=torch.float64).cpu().numpy()
    xc = x.double() - mu[None, :]
    want = (xc @ xc.T).cpu().numpy(); a1 = (xc.abs() @ xc.abs().T).cpu().numpy()
    del xc
    assert elem_ratio(got, want, a1) <= 1.0
    np.testing.assert_array_equal(got, got.T)
    w = torch.randn((n, 3), generator=g, device="cuda", dtype=torch.float32)
    out = cluster.gemm_tn(w, x, mu, out_dtype=torch.float64)
    xcd = x.double() - mu[None, :]
    want = (w.double().T @ xcd); a1 = (w.double().abs().T @ xcd.abs())
    r = ((out - want).abs() / (a1 * 4.0 * 2.0 ** -22 + 1e-300)).max().item()
    assert r <= 1.0


@pytest.mark.parametrize("n,k,d", [(1, 1, 7), (37, 5, 7), (300, 50, 1000), (97, 130, 5003), (200, 3, 100352)])
@pytest.mark.parametrize("means", [False, True])
def test_gemm_tn_matches_float64(n, k, d, means):
    r = np.random.RandomState(n + k + d)
    w, x = _dev(r.randn(n, k)), _dev(r.randn(n, d) + 0.5)
    mu = cluster.col_mean(x) if means else None
    got = cluster.gemm_tn(w, x, mu, out_dtype=torch.float64).cpu().numpy()
    xc = x.double() - (mu[None, :] if mu is not None else 0.0)
    want, a1 = (w.double().T @ xc).cpu().numpy(), (w.double().abs().T @ xc.abs()).cpu().numpy()
    assert elem_ratio(got, want, a1) <= 1.0
    np.testing.assert_array_equal(cluster.gemm_tn(w, x, mu, out_dtype=torch.float64).cpu().numpy(), got)


def test_kmeans_step_matches_float64():
    r = np.random.RandomState(3)
    for n, p, k in ((1, 1, 1), (300, 7, 3), (1615, 1000, 2), (500, 33, 9)):
        x = (r.randn(n, p) + np.repeat(r.randn(1, p), n, 0)).astype(np.float32)
        c = r.randn(k, p) * 0.5
        lab, dist, sums, cnt, inertia = (t.cpu().numpy() for t in cluster.kmeans_step(_dev(x), torch.from_numpy(c)))
        x64 = x.astype(np.float64)
        want_lab, want_dist = CO.assign(x64, c)
        np.testing.assert_array_equal(lab, want_lab)
        np.testing.assert_allclose(dist, want_dist, rtol=1e-12)
        np.testing.assert_array_equal(cnt, np.bincount(want_lab, minlength=k))
        for j in range(k):
            np.testing.assert_allclose(sums[j], x64[want_lab == j].sum(axis=0), rtol=1e-12, atol=1e-12 * np.abs(x64).sum(axis=0).max())
        assert abs(inertia[0] - want_dist.sum()) <= 1e-12 * want_dist.sum()


def _check_pca(x, k, pca, o, tr):
    np.testing.assert_allclose(pca.explained_variance_ratio_, o["explained_variance_ratio_"], atol=1e-6)
    ev = o["eigvals"]
    sep = []                                                                        # components with a relative eigengap >= 1e-3 (the others are
    for i in range(k):                                                              # any rotation within a near-degenerate block)
        gap = min(abs(ev[i] - ev[i - 1]) if i else np.inf, abs(ev[i] - ev[i + 1]) if i + 1 < len(ev) else np.inf) / ev[0]
        if gap < 1e-3:
            continue
        sep.append(i)
        cos = float(pca.components_[i].astype(np.float64) @ o["components_"][i]) / np.linalg.norm(pca.components_[i]) / np.linalg.norm(o["components_"][i])
        assert cos > 0 and 1 - cos <= 1e-5, (i, cos)
    assert sep
    assert np.linalg.norm(tr[:, sep] - o["transform"][:, sep]) / np.linalg.norm(o["transform"][:, sep]) <= 1e-5


def test_pca_low_rank_plus_noise_matches_oracle():
    r = np.random.RandomState(11)
    n, d, k = 300, 5000, 50
    x = (r.randn(n, 20) * np.linspace(10, 1, 20)) @ r.randn(20, d) + 0.05 * r.randn(n, d) + 2.0
    x = x.astype(np.float32)
    pca = cluster.PCA(k).fit(x)
    tr = pca.transform(x)
    assert tr.dtype == np.float32 and tr.shape == (n, k) and pca.components_.shape == (k, d)
    o = CO.pca(x.astype(np.float64), k)
    _check_pca(x, k, pca, o, tr)
    np.testing.assert_allclose(pca.mean_, o["mean_"], rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        cluster.PCA(n).fit(x)
    td = pca.transform(_dev(x))                                                     # device in, device out
    assert isinstance(td, torch.Tensor) and td.is_cuda
    np.testing.assert_array_equal(td.cpu().numpy(), tr)


def test_kmeans_device_matches_oracle_from_same_seeding():
    r = np.random.RandomState(4)
    for k, x in ((2, np.concatenate([r.randn(120, 40), r.randn(80, 40) + 1.5])), (3, r.randn(400, 12) + np.repeat(r.randn(4, 12), 100, 0))):
        x = x.astype(np.float32)
        km = cluster.KMeans(k, random_state=0).fit(x)
        x64 = x.astype(np.float64)
        mu = x64.mean(axis=0)
        c0, _ = cluster.kmeans_plusplus(x64 - mu, k, np.random.RandomState(0))
        lab, inertia, cen, n_iter = CO.lloyd(x64, c0 + mu)
        np.testing.assert_array_equal(km.labels_, lab)
        assert km.n_iter_ == n_iter
        np.testing.assert_allclose(km._centres64, cen, rtol=1e-10, atol=1e-10 * np.abs(x64).max())
        assert abs(km.inertia_ - inertia) <= 1e-10 * inertia
        y = (r.randn(50, x.shape[1]) + x64.mean(axis=0)).astype(np.float32)
        np.testing.assert_array_equal(km.predict(y), CO.assign(y.astype(np.float64), km._centres64)[0])


@pytest.mark.parametrize("bf16", [False, True])
def test_pca_on_c5a_taps_of_a_small_unet(bf16):
    from covidseg_amd.data import synthetic_ct
    from covidseg_amd.keras_like import UNetModel
    x, _ = synthetic_ct(96, 128, seed=9)
    kw = {"dtype": "bf16"} if bf16 else {}
    m = UNetModel(128, 1, seed=2, **kw)
    f = m.feature_matrix("conv2d_9", x, batch_size=32)
    assert f.dtype == torch.float32 and tuple(f.shape) == (96, 32768) and f.is_cuda
    inter = m.intermediate_output("conv2d_9", x, batch_size=32)
    np.testing.assert_array_equal(f.cpu().numpy(), np.transpose(inter, (0, 3, 1, 2)).reshape(96, -1).astype(np.float32))
    if bf16:
        return
    k = 40
    pca = cluster.PCA(k).fit(f)
    tr = pca.transform(f).cpu().numpy()
    o = CO.pca(f.cpu().numpy().astype(np.float64), k)
    _check_pca(f, k, pca, o, tr)


def test_reference_shape_1615_x_224():
    from covidseg_amd.data import synthetic_ct
    from covidseg_amd.keras_like import UNetModel
    n, k = 1615, 1000
    x, _ = synthetic_ct(n, 224, seed=1)
    m = UNetModel(224, 1, seed=0)
    f = m.feature_matrix("conv2d_9", x, batch_size=32)
    assert tuple(f.shape) == (n, 100352)
    mu = cluster.col_mean(f)
    g = cluster.gemm_nt(f, f, mu, mu, sym=True, out_dtype=torch.float64)
    r = np.random.RandomState(0)
    ii, jj = r.randint(0, n, 256), r.randint(0, n, 256)
    fc = f.double() - mu[None, :]
    a, b = fc[torch.from_numpy(ii).cuda()], fc[torch.from_numpy(jj).cuda()]
    want = (a * b).sum(1).cpu().numpy(); a1 = (a.abs() * b.abs()).sum(1).cpu().numpy()
    got = g.cpu().numpy()[ii, jj]
    assert elem_ratio(got, want, a1) <= 1.0
    var = float((fc * fc).sum() / (n - 1))
    del fc, a, b
    assert abs(float(torch.trace(g)) / (n - 1) - var) <= 1e-9 * var
    pca = cluster.PCA(k).fit(f)
    tr = pca.transform(f).double()
    lam, u = torch.linalg.eigh(g)
    lam, u = lam.flip(0)[:k], u.flip(1)[:, :k]
    us = u * lam.clamp(min=0).sqrt()
    sg = torch.sign((tr * us).sum(0))                                               # U's sign convention is the eigensolver's
    keep = (lam >= 1e-6 * lam[0])
    assert float(torch.linalg.norm((tr - us * sg)[:, keep]) / torch.linalg.norm(us[:, keep])) <= 1e-5
    c = torch.from_numpy(pca.components_[keep.cpu().numpy()].astype(np.float64)).cuda()
    assert float((c @ c.T - torch.eye(c.shape[0], device="cuda", dtype=torch.float64)).abs().max()) <= 1e-4


def test_runner_cluster_option():
    from covidseg_amd import runners
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = runners.holdout_runner_unet_infection_segmentation(input_size=64, epochs=1, n_samples=48, batch_size=8, verbose=0, cluster=True,
                                                                 workdir=_tmp())
    text = buf.getvalue()
    order = ["Extracted feature shape:", "Flattened features for the input of PCA:", "Total variance explained:", "Input data shape for Clustering:",
             "Label count for Kmeans on cts:", "Extracted feature shape:", "Flattened features for the input of PCA:", "Label count for Kmeans on valid:"]
    pos = 0
    for s in order:
        pos = text.index(s, pos) + len(s)
    cl = out["cluster"]
    assert sum(cl["label_counts"]) == 48
    nv = len(cl["valid_labels"])
    assert sum(cl["valid_label_counts"]) == nv
    assert cl["n_components"] == 47
    model = out["model"]
    from covidseg_amd.data import train_test_split
    cts, masks = runners._get_data(None, 64, 48, 0)
    _, xv, _, yv = train_test_split(cts, masks, test_size=0.3, random_state=42)
    assert nv == len(xv)
    for j, sc in enumerate(cl["scores"]):
        sel = np.arange(nv) if j == 0 else np.where(cl["valid_labels"] == j - 1)[0]
        if len(sel) == 0:
            assert sc is None
            continue
        ev = model.evaluate(xv[sel], yv[sel], batch_size=32, thresholds=[0.547])
        assert sc == [float(ev["loss"]), float(ev["dice"][0]), float(ev["iou"][0])]
    out2 = runners.holdout_runner_unet_infection_segmentation(input_size=64, epochs=1, n_samples=48, batch_size=8, verbose=0, workdir=_tmp())
    assert "cluster" not in out2


def _tmp():
    import tempfile
    return tempfile.mkdtemp()

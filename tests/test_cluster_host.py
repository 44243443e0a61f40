"""CPU: the host halves of cluster.py (k-means++ seeding, the n_components rules, the sign flip), the float64 oracle against scikit-learn, and
UNetModel.feature_matrix on the CPU oracle backend."""
import numpy as np
import pytest

from covidseg_amd import cluster
from tests import cluster_oracle as CO

try:
    import sklearn  # noqa: F401
    from sklearn.cluster import KMeans as SKKMeans, kmeans_plusplus as sk_kpp
    from sklearn.decomposition import PCA as SKPCA
    HAVE_SK = True
except ImportError:
    HAVE_SK = False
need_sk = pytest.mark.skipif(not HAVE_SK, reason="scikit-learn not installed")


def _sets():
    r = np.random.RandomState(7)
    sep = np.concatenate([r.randn(60, 5) + 6.0 * c for c in range(3)])
    over = r.randn(150, 8) + np.repeat(r.randn(3, 8) * 0.7, 50, axis=0)
    wide = r.rand(90, 20) * np.linspace(0.1, 4.0, 20)
    return [sep, over, wide]


@need_sk
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_kmeans_plusplus_equals_sklearn(k, which):
    X = _sets()[which]
    for seed in (0, 3):
        want_c, want_i = sk_kpp(X, k, random_state=seed)
        got_c, got_i = cluster.kmeans_plusplus(X, k, np.random.RandomState(seed))
        np.testing.assert_array_equal(got_i, want_i)
        np.testing.assert_array_equal(got_c, want_c)


@need_sk
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("k", [2, 3])
def test_seeding_plus_oracle_lloyd_equals_sklearn_kmeans(which, k):
    X = _sets()[which]
    sk = SKKMeans(k, random_state=0).fit(X)
    mu = X.mean(axis=0)
    c0, _ = cluster.kmeans_plusplus(X - mu, k, np.random.RandomState(0))          # KMeans.fit seeds on the centred data
    labels, inertia, cen, n_iter = CO.lloyd(X, c0 + mu)
    np.testing.assert_array_equal(labels, sk.labels_)
    assert n_iter == sk.n_iter_
    np.testing.assert_allclose(cen, sk.cluster_centers_, rtol=1e-10, atol=1e-10 * np.abs(X).max())
    assert abs(inertia - sk.inertia_) <= 1e-10 * sk.inertia_


@need_sk
@pytest.mark.parametrize("k", [1, 4, 9])
def test_pca_oracle_equals_sklearn_full(k):
    r = np.random.RandomState(1)
    X = r.randn(40, 12) @ r.randn(12, 30) + 0.1 * r.randn(40, 30) + 3.0
    sk = SKPCA(k, svd_solver="full").fit(X)
    o = CO.pca(X, k)
    for name in ("components_", "mean_", "explained_variance_", "explained_variance_ratio_", "singular_values_"):
        np.testing.assert_allclose(o[name], getattr(sk, name), rtol=1e-8, atol=1e-8, err_msg=name)
    np.testing.assert_allclose(o["transform"], sk.transform(X), rtol=1e-8, atol=1e-8)


def test_n_components_rules():
    assert cluster.check_n_components(9, 10, 100) == 9
    assert cluster.check_n_components(5, 100, 5) == 5
    for bad in (0, 10, -1):
        with pytest.raises(ValueError):
            cluster.check_n_components(bad, 10, 100)
    with pytest.raises(ValueError):
        cluster.check_n_components(6, 100, 5)
    with pytest.raises(ValueError):
        cluster.check_n_components(2.0, 10, 100)


def test_sign_flip_takes_the_first_of_a_tie():
    v = np.array([[1.0, -1.0, 0.5], [-2.0, 2.0, 0.0], [0.1, -0.3, 0.3]])
    np.testing.assert_array_equal(cluster.flip_signs(v), [1.0, -1.0, -1.0])


def test_feature_matrix_equals_reference_flatten_loop():
    torch = pytest.importorskip("torch")
    from covidseg_amd.keras_like import UNetModel
    from covidseg_amd.data import synthetic_ct
    from tests.oracle_backend import OracleBackend
    x, _ = synthetic_ct(5, 32, seed=2)
    m = UNetModel(32, 1, backend=OracleBackend(32, 32, 1, dtype=torch.float32), seed=0)
    got = m.feature_matrix("conv2d_9", x, batch_size=2)
    inter = m.intermediate_output("conv2d_9", x, batch_size=2)
    want = []
    for i in range(len(inter)):                                                     # T1:1403-1411
        cur = inter[i]
        want.append(np.reshape(np.rollaxis(cur, 2), (cur.shape[2], cur.shape[0], cur.shape[1])).flatten())
    want = np.array(want)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    np.testing.assert_array_equal(got.numpy(), want)

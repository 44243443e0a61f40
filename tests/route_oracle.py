"""Float64 restatements behind the routing tests: the reference's two-step assignment (np.rollaxis flatten -> PCA.transform -> KMeans.predict,
T1:1403-1450) and Keras' binary accuracy as model.evaluate reports it."""
import numpy as np

from tests import cluster_oracle as CO


def flatten_chw(taps):
    """[n, h, w, c] -> [n, c*h*w] in the reference's order: np.rollaxis(curr_img, 2).flatten() per slice (T1:1403-1411)"""
    return np.stack([np.rollaxis(np.asarray(t), 2).flatten() for t in taps]) if len(taps) else np.zeros((0, 0))


def route(taps, components, mean, centres):
    """(projections, labels, squared distances), float64: kmeans.predict(pca.transform(flatten_chw(taps))) with components / mean in (C, H, W)
    order; the lowest index wins a tie"""
    x = flatten_chw(taps).astype(np.float64)
    proj = (x - np.asarray(mean, np.float64)) @ np.asarray(components, np.float64).T
    lab, dist = CO.assign(proj, np.asarray(centres, np.float64))
    return proj, lab, dist


def binary_accuracy(p_batches, y_batches):
    """Keras' 'accuracy' for a sigmoid output (binary_accuracy, threshold 0.5) as evaluate reports it: MeanMetricWrapper averages the per-pixel
    values equal(y, p > 0.5) over every pixel of every batch -- not a mean of per-batch means"""
    vals = [np.equal(np.asarray(y, np.float32), (np.asarray(p, np.float32) > 0.5).astype(np.float32)).reshape(-1) for p, y in zip(p_batches, y_batches)]
    return float(np.concatenate(vals).astype(np.float64).mean())


class OraclePCA:
    """PCA(n_components) restated in float64 (cluster_oracle.pca) with the attributes the runner and the router read"""

    def __init__(self, n_components):
        self.n_components = n_components

    def fit(self, X):
        X = np.asarray(X, np.float64)
        o = CO.pca(X, self.n_components)
        self.components_, self.mean_ = o["components_"], o["mean_"]
        self.explained_variance_ratio_ = o["explained_variance_ratio_"]
        self.n_components_ = self.n_components
        return self

    def transform(self, X):
        return (np.asarray(X, np.float64) - self.mean_) @ self.components_.T


class OracleKMeans:
    """KMeans(n_clusters, random_state) restated in float64: k-means++ on the centred data, then cluster_oracle.lloyd"""

    def __init__(self, n_clusters=2, random_state=0):
        self.n_clusters, self.random_state = n_clusters, random_state

    def fit(self, X):
        from covidseg_amd.cluster import kmeans_plusplus
        X = np.asarray(X, np.float64)
        mu = X.mean(axis=0)
        c0, _ = kmeans_plusplus(X - mu, self.n_clusters, np.random.RandomState(self.random_state))
        self.labels_, self.inertia_, self._centres64, self.n_iter_ = CO.lloyd(X, c0 + mu)
        self.cluster_centers_ = self._centres64
        return self

    def predict(self, X):
        return CO.assign(np.asarray(X, np.float64), self._centres64)[0]

"""Float64 restatements behind the cluster tests: PCA by SVD of the centred data (sklearn's svd_solver="full") and Lloyd with direct differences
(sklearn's _kmeans_single_lloyd control flow)."""
import numpy as np


def pca(X, k):
    """dict of components_ (signs as svd_flip(u_based_decision=False)), mean_, explained_variance_, explained_variance_ratio_, singular_values_,
    and transform(X), all float64"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    mu = X.mean(axis=0)
    U, S, Vt = np.linalg.svd(X - mu, full_matrices=False)
    idx = np.argmax(np.abs(Vt), axis=1)
    sg = np.sign(Vt[np.arange(Vt.shape[0]), idx])
    U, Vt = U * sg, Vt * sg[:, None]
    ev = S ** 2 / (n - 1)
    return {"components_": Vt[:k], "mean_": mu, "explained_variance_": ev[:k], "explained_variance_ratio_": ev[:k] / ev.sum(),
            "singular_values_": S[:k], "transform": (X - mu) @ Vt[:k].T, "eigvals": S ** 2}


def assign(X, C):
    """labels (lowest index on a tie) and squared distances by direct differences"""
    d = ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2)
    lab = np.argmin(d, axis=1).astype(np.int32)
    return lab, d[np.arange(len(X)), lab]


def lloyd(X, centres, max_iter=300, tol=1e-4):
    """(labels, inertia, centres, n_iter) from the given initial centres; tol relative as KMeans(tol=...)"""
    X = np.asarray(X, np.float64)
    tol = float(np.mean(np.var(X, axis=0))) * tol
    cen = np.asarray(centres, np.float64).copy()
    k = len(cen)
    labels_old = np.full(len(X), -1, np.int32)
    strict = False
    for it in range(max_iter):
        labels, dist = assign(X, cen)
        cnt = np.bincount(labels, minlength=k).astype(np.float64)
        sums = np.zeros_like(cen)
        for j in range(k):
            sums[j] = X[labels == j].sum(axis=0)
        empty = np.where(cnt == 0)[0]
        if len(empty):
            far = np.argpartition(dist, -len(empty))[: -len(empty) - 1: -1]
            for e, f in zip(empty, far):
                sums[labels[f]] -= X[f]; sums[e] = X[f]; cnt[e] = 1; cnt[labels[f]] -= 1
        new = sums * (1.0 / np.maximum(cnt, 1))[:, None]
        shift = np.sqrt(((new - cen) ** 2).sum(axis=1))
        cen = new
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if (shift ** 2).sum() <= tol:
            break
        labels_old = labels
    if not strict:
        labels, _ = assign(X, cen)
    return labels, float(((X - cen[labels]) ** 2).sum()), cen, it + 1

"""Bottleneck-feature PCA and KMeans on the device: the reference's clustering of the conv2d_9 taps (T1:1386-1496),
`PCA(n_components=1000)` then `KMeans(n_clusters=2, random_state=0)`.

scikit-learn is not a dependency: this module restates what the runner needs (as data.train_test_split does), and the tests pin the
restatement against scikit-learn 1.7.

PCA.fit(X), X n x d (fp32 on the device):
  mean_        unet_feat_col_mean (fp64)
  G            unet_feat_gemm_nt, symmetric form: the centred Gram matrix Xc Xc^T, n x n fp64 (fp32 MFMA products, fp64 accumulation)
  eigh(G)      torch.linalg.eigh in float64 on the device; the top k eigenpairs (lambda, U) in descending order
  components_  diag(1/s) U^T Xc through unet_feat_gemm_tn, s = sqrt(lambda); signs as sklearn's svd_flip(u_based_decision=False): the
               largest-|.| entry of each row positive (the first one on a tie, as np.argmax)
  explained_variance_ = lambda / (n - 1), explained_variance_ratio_ = lambda / trace(G) (the variance of ALL components, as sklearn)
PCA.transform(Y) = (Y - mean_) components_^T through unet_feat_gemm_nt.  This is the exact (svd_solver="full") PCA; the reference's default
solver for its shape is sklearn's randomized SVD, which approximates the same subspace.

KMeans: k-means++ seeding on the host in float64, draw for draw sklearn's `_kmeans_plusplus` on the centred data; Lloyd on the device, one
unet_kmeans_step per iteration, with sklearn's stopping rules, empty-cluster relocation and final E-step.
"""
from __future__ import annotations

import numbers

import numpy as np

from . import _lib


def _torch():
    import torch
    return torch


def _ctx():
    torch = _torch()
    if not torch.cuda.is_available():
        raise _lib.UNetHipError("cluster: no GPU visible to torch; the kernels have no CPU fallback")
    return _lib.load(), _lib.Context.get(torch.cuda.current_device())


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _to_device(x):
    """(fp32 contiguous [n, d] tensor on the current device, input was NumPy, input dtype)"""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        dt = np.float64 if x.dtype == torch.float64 else np.float32
        return x.detach().to(device="cuda", dtype=torch.float32).contiguous(), False, dt
    a = np.asarray(x)
    dt = np.float64 if a.dtype == np.float64 else np.float32
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda(), True, dt


def _workspace(nbytes):
    return _torch().empty(max(int(nbytes), 16), dtype=_torch().uint8, device="cuda")


def col_mean(x):
    """mu[j] = mean_i x[i, j] in fp64 (unet_feat_col_mean); x: fp32 [n, d] on the device."""
    torch = _torch(); lib, ctx = _ctx()
    n, d = x.shape
    mu = torch.empty(d, dtype=torch.float64, device=x.device)
    ctx.check(lib.unet_feat_col_mean(ctx.handle, x.data_ptr(), x.stride(0), n, d, mu.data_ptr(), _stream()), "feat_col_mean")
    return mu


def gemm_nt(a, b, mu_a=None, mu_b=None, sym=False, out_dtype=None):
    """(a - mu_a)(b - mu_b)^T (unet_feat_gemm_nt): a [m, d], b [p, d] fp32 on the device, means fp64 [d] or None; sym: the Gram form (b is a)."""
    torch = _torch(); lib, ctx = _ctx()
    out_dtype = out_dtype or torch.float32
    m, d = a.shape
    p = b.shape[0]
    c = torch.empty((m, p), dtype=out_dtype, device=a.device)
    ws = _workspace(lib.unet_feat_gemm_nt_workspace(m, p, d, int(sym)))
    ctx.check(lib.unet_feat_gemm_nt(ctx.handle, a.data_ptr(), a.stride(0), mu_a.data_ptr() if mu_a is not None else None, b.data_ptr(), b.stride(0),
                                    mu_b.data_ptr() if mu_b is not None else None, m, p, d, int(sym), c.data_ptr(), c.stride(0),
                                    int(out_dtype == torch.float64), ws.data_ptr(), ws.numel(), _stream()), "feat_gemm_nt")
    return c


def gemm_tn(w, x, mu=None, out_dtype=None):
    """w^T (x - mu) (unet_feat_gemm_tn): w [n, k], x [n, d] fp32 on the device, mu fp64 [d] or None -> [k, d]."""
    torch = _torch(); lib, ctx = _ctx()
    out_dtype = out_dtype or torch.float32
    n, k = w.shape
    d = x.shape[1]
    out = torch.empty((k, d), dtype=out_dtype, device=x.device)
    ws = _workspace(lib.unet_feat_gemm_tn_workspace(k, d, n))
    ctx.check(lib.unet_feat_gemm_tn(ctx.handle, w.data_ptr(), w.stride(0), x.data_ptr(), x.stride(0), mu.data_ptr() if mu is not None else None, n, k, d,
                                    out.data_ptr(), out.stride(0), int(out_dtype == torch.float64), ws.data_ptr(), ws.numel(), _stream()), "feat_gemm_tn")
    return out


def kmeans_step(pts, centres):
    """One Lloyd E-step plus the sums of the M-step (unet_kmeans_step): pts fp32 [n, p], centres fp64 [k, p] on the device ->
    (labels int32 [n], squared distances fp64 [n], sums fp64 [k, p], counts int64 [k], inertia fp64 [1])."""
    torch = _torch(); lib, ctx = _ctx()
    n, p = pts.shape
    centres = centres.to(device=pts.device, dtype=torch.float64).contiguous()
    k = centres.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=pts.device)
    dist = torch.empty(n, dtype=torch.float64, device=pts.device)
    sums = torch.empty((k, p), dtype=torch.float64, device=pts.device)
    counts = torch.empty(k, dtype=torch.int64, device=pts.device)
    inertia = torch.empty(1, dtype=torch.float64, device=pts.device)
    ctx.check(lib.unet_kmeans_step(ctx.handle, pts.data_ptr(), pts.stride(0), n, p, centres.data_ptr(), k, labels.data_ptr(), dist.data_ptr(),
                                   sums.data_ptr(), counts.data_ptr(), inertia.data_ptr(), _stream()), "kmeans_step")
    return labels, dist, sums, counts, inertia


def flip_signs(v):
    """sklearn 1.7 svd_flip(u_based_decision=False) on the rows of v: the largest-|.| entry of each row becomes positive (the first one on a tie)."""
    v = np.asarray(v)
    idx = np.argmax(np.abs(v), axis=1)
    return np.sign(v[np.arange(v.shape[0]), idx])


def check_n_components(k, n_samples, n_features):
    """Centred data has rank <= n - 1: 1 <= k <= min(n - 1, d), else ValueError."""
    if not isinstance(k, numbers.Integral) or isinstance(k, bool):
        raise ValueError(f"n_components={k!r} must be an integer")
    lim = min(n_samples - 1, n_features)
    if not 1 <= k <= lim:
        raise ValueError(f"n_components={k} must be between 1 and min(n_samples - 1, n_features)={lim} (n_samples={n_samples}, n_features={n_features})")
    return int(k)


class PCA:
    """sklearn.decomposition.PCA(n_components) on the device (exact solver, module docstring).  fit / transform / fit_transform take a NumPy
    array or a device tensor and return the same kind (float32 for float32 input)."""

    def __init__(self, n_components):
        self.n_components = n_components

    def fit(self, X):
        torch = _torch()
        x, _, dt = _to_device(X)
        n, d = x.shape
        k = check_n_components(self.n_components, n, d)
        mu = col_mean(x)
        g = gemm_nt(x, x, mu, mu, sym=True, out_dtype=torch.float64)
        lam, u = torch.linalg.eigh(g)
        lam, u = lam.flip(0), u.flip(1)
        total = torch.trace(g)
        lam_k, u_k = lam[:k].clamp(min=0.0), u[:, :k]
        s = lam_k.sqrt()
        inv = torch.where(s > 0, 1.0 / s, torch.zeros_like(s))
        comps = gemm_tn((u_k * inv).to(torch.float32).contiguous(), x, mu)
        signs = flip_signs(comps.cpu().numpy())
        comps = comps * torch.from_numpy(signs.astype(np.float32)).to(comps.device)[:, None]
        self._mean_dev, self._comps_dev = mu, comps.contiguous()
        lam_h, tot = lam_k.cpu().numpy(), float(total)
        self.components_ = comps.cpu().numpy().astype(dt, copy=False)
        self.mean_ = mu.cpu().numpy().astype(dt)
        self.explained_variance_ = (lam_h / (n - 1)).astype(dt)
        self.explained_variance_ratio_ = (lam_h / tot).astype(dt)
        self.singular_values_ = np.sqrt(lam_h).astype(dt)
        self.n_components_, self.n_samples_, self.n_features_in_ = k, n, d
        return self

    def transform(self, X):
        if not hasattr(self, "_comps_dev"):
            raise RuntimeError("PCA.transform before fit")
        x, is_np, dt = _to_device(X)
        if x.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {x.shape[1]} features, PCA was fitted with {self.n_features_in_}")
        y = gemm_nt(x, self._comps_dev, self._mean_dev, None)
        if is_np:
            return y.cpu().numpy().astype(dt, copy=False)
        return y if dt == np.float32 else y.double()

    def fit_transform(self, X):
        return self.fit(X).transform(X)


def kmeans_plusplus(X, n_clusters, random_state, n_local_trials=None):
    """sklearn.cluster._kmeans._kmeans_plusplus (1.7), unit sample weights, float64 on the host: (centres [k, p], indices [k])."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    w = np.ones(n, np.float64)
    xx = np.einsum("ij,ij->i", X, X)

    def sqdist(a):                                                     # sklearn _euclidean_distances(a, X, Y_norm_squared=xx, squared=True)
        aa = np.einsum("ij,ij->i", a, a)[:, None]
        dd = -2 * (a @ X.T)
        dd += aa
        dd += xx[None, :]
        np.maximum(dd, 0, out=dd)
        return dd

    if n_local_trials is None:
        n_local_trials = 2 + int(np.log(n_clusters))
    centres = np.empty((n_clusters, X.shape[1]), np.float64)
    cid = rs.choice(n, p=w / w.sum())
    idx = np.full(n_clusters, -1, dtype=int)
    centres[0] = X[cid]; idx[0] = cid
    closest = sqdist(centres[0, None])
    pot = closest @ w
    for c in range(1, n_clusters):
        rv = rs.uniform(size=n_local_trials) * pot
        cand = np.searchsorted(np.cumsum(w * closest, dtype=np.float64), rv)
        np.clip(cand, None, closest.size - 1, out=cand)
        dc = sqdist(X[cand])
        np.minimum(closest, dc, out=dc)
        cpot = dc @ w.reshape(-1, 1)
        best = np.argmin(cpot)
        pot = cpot[best]
        closest = dc[best]
        centres[c] = X[cand[best]]; idx[c] = cand[best]
    return centres, idx


def _same_clustering(l1, l2, k):
    """sklearn _is_same_clustering: the two labelings are equal up to a permutation"""
    mapping = np.full(k, -1, dtype=np.int64)
    for a, b in zip(l1, l2):
        if mapping[a] == -1:
            mapping[a] = b
        elif mapping[a] != b:
            return False
    return True


class KMeans:
    """sklearn.cluster.KMeans (1.7 semantics, dense data, unit weights): k-means++ on the host, Lloyd on the device (module docstring)."""

    def __init__(self, n_clusters=8, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, random_state=None):
        self.n_clusters, self.init, self.n_init, self.max_iter, self.tol, self.random_state = n_clusters, init, n_init, max_iter, tol, random_state

    def _lloyd(self, pts, xh, centres, tol):
        """_kmeans_single_lloyd: pts fp32 on the device, xh the same points float64 on the host, centres float64 [k, p] -> (labels, inertia, centres, n_iter)"""
        torch = _torch()
        k = self.n_clusters
        labels_old = np.full(len(xh), -1, np.int32)
        strict = False
        cen = centres.copy()
        for it in range(self.max_iter):
            lab_d, dist_d, sums_d, cnt_d, _ = kmeans_step(pts, torch.from_numpy(cen))
            labels, dist, sums, cnt = lab_d.cpu().numpy(), dist_d.cpu().numpy(), sums_d.cpu().numpy(), cnt_d.cpu().numpy().astype(np.float64)
            empty = np.where(cnt == 0)[0]
            if len(empty):                                             # _relocate_empty_clusters_dense
                far = np.argpartition(dist, -len(empty))[: -len(empty) - 1: -1]
                for e, f in zip(empty, far):
                    old = labels[f]
                    sums[old] -= xh[f]
                    sums[e] = xh[f]
                    cnt[e] = 1.0
                    cnt[old] -= 1.0
            new = sums.copy()
            big = int(np.argmax(cnt))
            for j in range(k):                                         # _average_centers
                if cnt[j] > 0:
                    new[j] *= 1.0 / cnt[j]
                else:
                    new[j] = new[big]
            shift = np.sqrt(((new - cen) ** 2).sum(axis=1))
            cen = new
            if np.array_equal(labels, labels_old):
                strict = True
                break
            if (shift ** 2).sum() <= tol:
                break
            labels_old = labels
        if not strict:
            labels = kmeans_step(pts, torch.from_numpy(cen))[0].cpu().numpy()
        inertia = float(((xh - cen[labels]) ** 2).sum())
        return labels, inertia, cen, it + 1

    def fit(self, X, y=None):
        torch = _torch()
        pts, _, dt = _to_device(X)
        xh = pts.double().cpu().numpy()
        n = xh.shape[0]
        if n < self.n_clusters:
            raise ValueError(f"n_samples={n} should be >= n_clusters={self.n_clusters}")
        rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else np.random.RandomState(self.random_state)
        tol = float(np.mean(np.var(xh, axis=0))) * self.tol
        x_mean = xh.mean(axis=0)
        xc = xh - x_mean
        if isinstance(self.init, str) and self.init == "k-means++":
            n_init = 1 if self.n_init == "auto" else int(self.n_init)
        elif isinstance(self.init, np.ndarray):
            n_init = 1
        else:
            raise ValueError(f"init={self.init!r}: k-means++ or an array of centres")
        best = None
        for _ in range(n_init):
            if isinstance(self.init, np.ndarray):
                c0 = np.asarray(self.init, np.float64) - x_mean
            else:
                c0, _idx = kmeans_plusplus(xc, self.n_clusters, rs)
            labels, inertia, cen, n_iter = self._lloyd(pts, xh, c0 + x_mean, tol)
            if best is None or (inertia < best[1] and not _same_clustering(labels, best[0], self.n_clusters)):
                best = (labels, inertia, cen, n_iter)
        self.labels_ = best[0].astype(np.int32)
        self.inertia_ = best[1]
        self.cluster_centers_ = best[2].astype(dt)
        self._centres64 = best[2]
        self.n_iter_ = best[3]
        return self

    def predict(self, X):
        pts, _, _ = _to_device(X)
        return kmeans_step(pts, _torch().from_numpy(self._centres64))[0].cpu().numpy().astype(np.int32)

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


ROUTER_FORMAT = 1


def chw_to_hwc(a, tap_shape):
    """Rows flattened in the reference's (C, H, W) order (np.rollaxis(curr_img, 2).flatten(), T1:1403-1411) -> the same rows in tap order (H, W, C).
    a: [k, C*H*W] (or [C*H*W]) torch tensor or array; tap_shape (h, w, c)."""
    h, w, c = (int(v) for v in tap_shape)
    lead = tuple(a.shape[:-1])
    if hasattr(a, "permute"):
        return a.reshape(lead + (c, h, w)).movedim(-3, -1).reshape(lead + (h * w * c,))
    return np.moveaxis(np.asarray(a).reshape(lead + (c, h, w)), -3, -1).reshape(lead + (h * w * c,))


def hwc_to_chw(a, tap_shape):
    """The inverse of chw_to_hwc."""
    h, w, c = (int(v) for v in tap_shape)
    lead = tuple(a.shape[:-1])
    if hasattr(a, "permute"):
        return a.reshape(lead + (h, w, c)).movedim(-1, -3).reshape(lead + (c * h * w,))
    return np.moveaxis(np.asarray(a).reshape(lead + (h, w, c)), -1, -3).reshape(lead + (c * h * w,))


class Router:
    """The assignment step of the routed two-model system (routed.py): a tap of `layer` -> PCA projection -> nearest KMeans centre, for one batch
    at a time, through unet_cluster_route.  Built once from a fitted PCA and KMeans: the components and the mean are permuted into tap order
    (h, w, c) so that the kernel reads the engine's NHWC tap in place; the mean is rounded to fp32 (as PCA.transform stages it) and the centres
    stay fp64.

    Attributes: comps_hwc [k, d] fp32, mu_hwc [d] fp32, centres [nc, k] fp64 (torch, on `device`), mean64 [d] fp64 in (C, H, W) order (host),
    explained_variance_ratio (host), tap_shape (h, w, c), layer."""

    def __init__(self, pca, kmeans, tap_shape, layer="conv2d_9", device="cuda"):
        comps = getattr(pca, "_comps_dev", None)
        if comps is None or str(device) == "cpu":
            comps = np.asarray(pca.components_, np.float32)
        centres = getattr(kmeans, "_centres64", None)
        if centres is None:
            centres = np.asarray(kmeans.cluster_centers_, np.float64)
        self._build(comps, np.asarray(pca.mean_, np.float64), centres, tap_shape, layer, np.asarray(pca.explained_variance_ratio_), device)

    @classmethod
    def from_arrays(cls, components, mean, centres, tap_shape, layer="conv2d_9", explained_variance_ratio=None, device="cuda"):
        """components [k, d] and mean [d] in the reference's (C, H, W) flatten order, centres [nc, k]."""
        r = cls.__new__(cls)
        r._build(components, np.asarray(mean, np.float64), centres, tap_shape, layer, explained_variance_ratio, device)
        return r

    def _build(self, comps, mean, centres, tap_shape, layer, evr, device):
        torch = _torch()
        self.tap_shape = tuple(int(v) for v in tap_shape)
        self.layer = layer
        h, w, c = self.tap_shape
        d = h * w * c
        k = int(comps.shape[0])
        if tuple(comps.shape) != (k, d) or mean.shape != (d,):
            raise ValueError(f"Router: components {tuple(comps.shape)} / mean {mean.shape} do not match the tap shape {self.tap_shape} (d = {d})")
        centres = torch.as_tensor(np.asarray(centres.cpu() if hasattr(centres, "cpu") else centres, np.float64))
        if centres.ndim != 2 or centres.shape[1] != k or not 1 <= centres.shape[0] <= 16:
            raise ValueError(f"Router: centres {tuple(centres.shape)} must be [nc, {k}] with 1 <= nc <= 16")
        if not isinstance(comps, torch.Tensor):
            comps = torch.from_numpy(np.ascontiguousarray(comps, np.float32))
        self.comps_hwc = chw_to_hwc(comps.to(device=device, dtype=torch.float32), self.tap_shape).contiguous()
        self.mean64 = mean
        self.mu_hwc = torch.from_numpy(np.ascontiguousarray(chw_to_hwc(mean, self.tap_shape), np.float32)).to(device)
        self.centres = centres.to(device).contiguous()
        self.explained_variance_ratio = None if evr is None else np.asarray(evr)
        self.n_components, self.n_clusters, self.n_features = k, int(centres.shape[0]), d

    def components_chw(self):
        """The components in the reference's (C, H, W) order, fp32 numpy [k, d]."""
        return hwc_to_chw(self.comps_hwc, self.tap_shape).cpu().numpy()

    def assign(self, tap, want_proj=False):
        """One batch of taps [n, h, w, c] -- the engine's tap_device view (pixel stride >= c, fp32 or bf16), or any fp32 / bf16 tensor of that shape
        on the device -> (labels int32 [n], squared distances fp64 [n], projections fp32 [n, k] or None), device tensors."""
        torch = _torch(); lib, ctx = _ctx()
        if tuple(tap.shape[1:]) != self.tap_shape:
            raise ValueError(f"Router.assign: tap shape {tuple(tap.shape[1:])}, the router was built for {self.tap_shape}")
        if tap.dtype not in (torch.float32, torch.bfloat16):
            tap = tap.to(torch.float32)
        n, h, w, c = tap.shape
        ld = tap.stride(2)
        if not (tap.stride(3) == 1 and ld >= c and tap.stride(1) == w * ld and tap.stride(0) == h * w * ld) or not tap.is_cuda:
            tap = tap.to(device=self.comps_hwc.device).contiguous()
            ld = c
        k = self.n_components
        labels = torch.empty(n, dtype=torch.int32, device=tap.device)
        dist = torch.empty(n, dtype=torch.float64, device=tap.device)
        proj = torch.empty((n, k), dtype=torch.float32, device=tap.device) if want_proj else None
        ws = _workspace(lib.unet_cluster_route_workspace(n, h * w * c, k))
        ctx.check(lib.unet_cluster_route(ctx.handle, tap.data_ptr(), int(tap.dtype == torch.bfloat16), n, h, w, c, ld, self.comps_hwc.data_ptr(),
                                         self.mu_hwc.data_ptr(), k, self.centres.data_ptr(), self.n_clusters,
                                         proj.data_ptr() if proj is not None else None, labels.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream()), "cluster_route")
        return labels, dist, proj

    def arrays(self):
        """What router.npz holds (routed.ClusterRoutedModel.save)."""
        return {"format": np.int64(ROUTER_FORMAT), "components": self.components_chw(), "mean": self.mean64,
                "centres": self.centres.cpu().numpy(), "tap_shape": np.asarray(self.tap_shape, np.int64), "layer": np.asarray(self.layer),
                "explained_variance_ratio": (np.asarray([], np.float64) if self.explained_variance_ratio is None
                                             else np.asarray(self.explained_variance_ratio))}

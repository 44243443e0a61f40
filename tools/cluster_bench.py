"""Feature-tap PCA + KMeans at the reference's shape (T1:1386-1496): 1615 synthetic slices at 224^2 through a random-init U-Net, conv2d_9 taps
(d = 14 * 14 * 512 = 100,352), PCA(1000), KMeans(2).  Prints one JSON line: ms per stage, the achieved TFLOP/s of the NT (Gram, transform) and TN
(components) kernels against the 157 TFLOP/s fp32 matrix peak, and -- when scikit-learn is importable -- its CPU PCA(1000) + KMeans(2) time.
    python tools/cluster_bench.py [--n 1615] [--size 224] [--k 1000] [--reps 3] [--no-sklearn]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from covidseg_amd import cluster  # noqa: E402
from covidseg_amd.data import synthetic_ct  # noqa: E402
from covidseg_amd.keras_like import UNetModel  # noqa: E402

PEAK = 157.0


def timed(fn, reps):
    """median ms of `reps` runs after one warm-up"""
    out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1615); ap.add_argument("--size", type=int, default=224); ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    x, _ = synthetic_ct(a.n, a.size, seed=1)
    m = UNetModel(a.size, 1, seed=0)
    ms_feat, f = timed(lambda: m.feature_matrix("conv2d_9", x, batch_size=32), 1)
    n, d = f.shape
    k = min(a.k, n - 1, d)
    ms_mean, mu = timed(lambda: cluster.col_mean(f), a.reps)
    ms_gram, g = timed(lambda: cluster.gemm_nt(f, f, mu, mu, sym=True, out_dtype=torch.float64), a.reps)
    ms_eigh, (lam, u) = timed(lambda: torch.linalg.eigh(g), a.reps)
    w = (u.flip(1)[:, :k] / lam.flip(0)[:k].clamp(min=1e-30).sqrt()).float().contiguous()
    ms_comp, comps = timed(lambda: cluster.gemm_tn(w, f, mu), a.reps)
    ms_tr, tr = timed(lambda: cluster.gemm_nt(f, comps, mu, None), a.reps)
    ms_pca, pca = timed(lambda: cluster.PCA(k).fit(f), 1)
    pts = pca.transform(f)
    ms_km, km = timed(lambda: cluster.KMeans(2, random_state=0).fit(pts), 1)
    # useful flops: the Gram's upper triangle (the kernel computes whole diagonal tiles), components 2 k n d, transform 2 n k d
    fl_gram, fl_tn, fl_tr = n * (n + 1) * d, 2.0 * k * n * d, 2.0 * n * k * d
    res = {"n": n, "d": d, "k": k, "ms": {"features": round(ms_feat, 2), "mean": round(ms_mean, 3), "gram": round(ms_gram, 3),
                                          "mean_plus_gram": round(ms_mean + ms_gram, 3), "eigh": round(ms_eigh, 2), "components": round(ms_comp, 3),
                                          "transform": round(ms_tr, 3), "pca_fit_total": round(ms_pca, 2), "kmeans": round(ms_km, 2)},
           "tflops": {"gram_nt": round(fl_gram / ms_gram / 1e9, 1), "components_tn": round(fl_tn / ms_comp / 1e9, 1),
                      "transform_nt": round(fl_tr / ms_tr / 1e9, 1), "peak": PEAK},
           "kmeans_n_iter": int(km.n_iter_), "explained_variance": float(np.sum(pca.explained_variance_ratio_))}
    if not a.no_sklearn:
        try:
            from sklearn.cluster import KMeans as SKK
            from sklearn.decomposition import PCA as SKP
            fh = f.cpu().numpy()
            t0 = time.perf_counter(); sp = SKP(k).fit(fh); t1 = time.perf_counter(); SKK(2, random_state=0).fit(sp.transform(fh)); t2 = time.perf_counter()
            res["sklearn_cpu_ms"] = {"pca": round((t1 - t0) * 1e3, 1), "kmeans": round((t2 - t1) * 1e3, 1), "threads": torch.get_num_threads()}
        except ImportError:
            res["sklearn_cpu_ms"] = None
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The routing step of the routed two-model system at the reference's shape: a random-init U-Net at 224^2, the Router fitted on 1615 synthetic slices
(conv2d_9 taps, d = 14 * 14 * 512 = 100,352, PCA(1000), KMeans(2)), one batch of n = 32.  Prints one JSON line:
  route      unet_cluster_route alone, its floor max(bytes / 8 TB/s, 2 n k d / 157 TFLOP/s) and the fraction of that floor it reaches
  composed   the same batch through the pieces that existed before it: permute-copy of the tap, unet_feat_gemm_nt, unet_kmeans_step
  predict    routed predict of 32 slices against plain predict
Kernel times: hip events around `--inner` back-to-back launches, after warm-up; the median of `--reps` such groups.
    python tools/route_bench.py [--n-fit 1615] [--size 224] [--k 1000] [--n 32] [--reps 7] [--inner 20]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from covidseg_amd import _lib, cluster  # noqa: E402
from covidseg_amd.data import synthetic_ct  # noqa: E402
from covidseg_amd.keras_like import UNetModel  # noqa: E402
from covidseg_amd.routed import ClusterRoutedModel  # noqa: E402

PEAK_TFLOPS, PEAK_TBS = 157.0, 8.0


def timed_us(fn, reps, inner):
    """median over `reps` groups of the mean per-call time (us) of `inner` back-to-back calls, after 3 warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-fit", type=int, default=1615); ap.add_argument("--size", type=int, default=224); ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--n", type=int, default=32); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    x, _ = synthetic_ct(a.n_fit, a.size, seed=1)
    m = UNetModel(a.size, 1, seed=0)
    rm = ClusterRoutedModel(m, n_components=a.k).fit_router(x)
    ro = rm.router
    h, w, c = ro.tap_shape
    d, k, nc, n = ro.n_features, ro.n_components, ro.n_clusters, a.n
    for j in range(nc):
        rm.experts[j] = rm._new_expert(j, "fresh")
    xb = x[:n]
    m.backend.predict_batch(xb)
    tap = m.backend.tap_device(n, "c5a")
    lib, ctx = _lib.load(), _lib.Context.get(torch.cuda.current_device())
    s = torch.cuda.current_stream().cuda_stream
    lab = torch.empty(n, dtype=torch.int32, device="cuda"); dist = torch.empty(n, dtype=torch.float64, device="cuda")
    proj = torch.empty((n, k), dtype=torch.float32, device="cuda")
    ws = torch.empty(max(lib.unet_cluster_route_workspace(n, d, k), 16), dtype=torch.uint8, device="cuda")
    bf16 = int(tap.dtype == torch.bfloat16)

    def route():
        ctx.check(lib.unet_cluster_route(ctx.handle, tap.data_ptr(), bf16, n, h, w, c, tap.stride(2), ro.comps_hwc.data_ptr(), ro.mu_hwc.data_ptr(), k,
                                         ro.centres.data_ptr(), nc, proj.data_ptr(), lab.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(), s),
                  "cluster_route")
    us_route = timed_us(route, a.reps, a.inner)
    bytes_ = k * d * 4 + n * d * tap.element_size() + d * 4
    floor = max(bytes_ / (PEAK_TBS * 1e12), 2.0 * n * k * d / (PEAK_TFLOPS * 1e12)) * 1e6

    comps_chw = cluster.hwc_to_chw(ro.comps_hwc, ro.tap_shape).contiguous()
    mu64 = torch.from_numpy(ro.mean64).cuda()
    flat = torch.empty((n, d), dtype=torch.float32, device="cuda")
    us_perm = timed_us(lambda: flat.view(n, c, h, w).copy_(tap.permute(0, 3, 1, 2)), a.reps, a.inner)
    us_gemm = timed_us(lambda: cluster.gemm_nt(flat, comps_chw, mu64, None), a.reps, a.inner)
    pts = cluster.gemm_nt(flat, comps_chw, mu64, None)
    us_km = timed_us(lambda: cluster.kmeans_step(pts, ro.centres), a.reps, a.inner)
    agree = bool(torch.equal(cluster.kmeans_step(pts, ro.centres)[0], lab))

    ms_plain = timed_us(lambda: m.predict(xb, batch_size=n), a.reps, 1) / 1e3
    ms_routed = timed_us(lambda: rm.predict(xb, batch_size=n), a.reps, 1) / 1e3
    res = {"shape": {"size": a.size, "n_fit": a.n_fit, "n": n, "d": d, "k": k, "nc": nc, "tap_dtype": str(tap.dtype).split(".")[-1]},
           "route": {"us": round(us_route, 1), "floor_us": round(floor, 1), "fraction_of_floor": round(floor / us_route, 3),
                     "x_floor": round(us_route / floor, 2), "gb_per_s": round(bytes_ / us_route / 1e3, 1)},
           "composed_us": {"permute_copy": round(us_perm, 1), "feat_gemm_nt": round(us_gemm, 1), "kmeans_step": round(us_km, 1),
                           "total": round(us_perm + us_gemm + us_km, 1)},
           "labels_agree_with_composed": agree,
           "predict_ms": {"plain": round(ms_plain, 2), "routed": round(ms_routed, 2), "ratio": round(ms_routed / ms_plain, 2)},
           "batch_labels": np.bincount(lab.cpu().numpy(), minlength=nc).tolist()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

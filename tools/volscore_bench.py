"""Times the volume score (unet_vol_confusion / unet_vol_surface / unet_vol_edt_sq / unet_vol_surface_distances / unet_vol_lesion_overlap and score_volume as a
whole) on a 512 x 512 x 301 pair at spacing (0.7, 0.7, 1.25) -- 300 random ellipsoids against their roll by (3, -2, 1) plus 20 more -- and the host path it
replaces on the same box: masks device -> host, two scipy erosions, two scipy.ndimage.distance_transform_edt, the reductions.  tools/components_bench.py's
method: warm-up, median of `--runs`, device events around the entries.  Writes profiles/volume_score.json.

    python tools/volscore_bench.py [--runs 10] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
    python tools/volscore_bench.py --trace-call                            three score_volume calls and nothing else (for a kernel trace: per-launch times)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12
PIXDIM = (0.7, 0.7, 1.25)


def event_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def entry(ms, byts):
    return {"ms": ms, "bytes": int(byts), "TBps": byts / ms / 1e9, "of_8TBps": byts / (ms * 1e-3) / HBM}


def pair(shape):
    import components_oracle as CO
    pred = CO.ellipsoids(shape, 300, 0, 5)
    return pred, np.roll(pred, (3, -2, 1), axis=(0, 1, 2)) | CO.ellipsoids(shape, 20, 0, 9)


def bench(shape, runs, host):
    import torch
    from covidseg_amd import volume as V
    lib, ctx = V._ctx()
    X, Y, Z = shape
    N = X * Y * Z
    pred, truth = pair(shape)
    pd, _ = V._mask_to_device(pred); td, _ = V._mask_to_device(truth)
    s = V._stream()
    out = {"shape": list(shape), "pixdim": list(PIXDIM)}
    counts = torch.empty((Z, 3), dtype=torch.int64, device="cuda")
    out["vol_confusion"] = entry(event_ms(lambda: ctx.check(lib.unet_vol_confusion(ctx.handle, pd.data_ptr(), td.data_ptr(), X, Y, Z, counts.data_ptr(), s)), runs), 2 * N)
    sa = torch.empty(N, dtype=torch.uint8, device="cuda"); sb = torch.empty(N, dtype=torch.uint8, device="cuda"); cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    surf = lambda m, o: ctx.check(lib.unet_vol_surface(ctx.handle, m.data_ptr(), X, Y, Z, 1, o.data_ptr(), cnt.data_ptr(), s))
    out["vol_surface"] = entry(event_ms(lambda: surf(pd, sa), runs), 2 * N)          # (the eight neighbour rows are re-reads of lines the same workgroups hold)
    surf(td, sb); nb = int(cnt.item()); surf(pd, sa); na = int(cnt.item())
    out["surface_voxels"] = [na, nb]
    d2 = torch.empty(N, dtype=torch.float64, device="cuda")
    w = np.ascontiguousarray(np.asarray(PIXDIM, np.float64) ** 2)
    edt = lambda f: ctx.check(lib.unet_vol_edt_sq(ctx.handle, f.data_ptr(), X, Y, Z, 1, w.ctypes.data, d2.data_ptr(), None, 0, s))
    ms = event_ms(lambda: edt(sb), runs)
    # x pass: N read, 8 N written; y and z pass: 8 N read and written each.  Line passes: 5 fp64 operations per (output, candidate) pair, every candidate scanned at most
    out["vol_edt_sq"] = dict(entry(ms, N + 8 * N + 2 * 16 * N), fp64_ops_upper_bound=5.0 * N * (Y + Z), Tops_upper_bound=5.0 * N * (Y + Z) / ms / 1e9)
    res = torch.zeros(3, dtype=torch.int64, device="cuda"); gath = torch.empty(max(na, 1), dtype=torch.float64, device="cuda")
    ws = torch.empty(32768, dtype=torch.uint8, device="cuda")
    sd = lambda: ctx.check(lib.unet_vol_surface_distances(ctx.handle, sa.data_ptr(), d2.data_ptr(), X, Y, Z, res.data_ptr(), gath.data_ptr(), na, ws.data_ptr(), ws.numel(), s))
    out["vol_surface_distances"] = entry(event_ms(sd, runs), N + 16 * na)
    lt, nt = V.label_device(td, shape, 1); lp, npred = V.label_device(pd, shape, 1)
    ct = torch.zeros(max(nt, 1), dtype=torch.int64, device="cuda"); cp = torch.zeros(max(npred, 1), dtype=torch.int64, device="cuda")
    ov = lambda: ctx.check(lib.unet_vol_lesion_overlap(ctx.handle, lt.data_ptr(), nt, lp.data_ptr(), npred, X, Y, Z, ct.data_ptr(), cp.data_ptr(), s))
    out["vol_lesion_overlap"] = entry(event_ms(ov, runs), 8 * N)
    del lt, lp, d2, gath
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        score = V.score_volume(pd, td, PIXDIM, shape=shape)
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    out["score_volume_ms"] = statistics.median(ts)
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        V.score_volume(pd, td, PIXDIM, shape=shape, lesions=False)
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    out["score_volume_no_lesions_ms"] = statistics.median(ts)
    out["score"] = {k: getattr(score, k) for k in ("dice", "hd", "hd95", "assd", "lesion_recall", "lesion_precision")}
    if not host:
        return out
    try:
        from scipy import ndimage as ndi
    except ImportError:
        out["host_path"] = "scipy does not import here: the host path was not timed"
        return out
    torch.cuda.synchronize(); t0 = time.perf_counter()
    hp = pd.cpu().numpy().reshape(shape, order="F") != 0; ht = td.cpu().numpy().reshape(shape, order="F") != 0; t1 = time.perf_counter()
    ha, hb = hp ^ ndi.binary_erosion(hp), ht ^ ndi.binary_erosion(ht); t2 = time.perf_counter()
    da = ndi.distance_transform_edt(~hb, sampling=PIXDIM)[ha]; t3 = time.perf_counter()
    db = ndi.distance_transform_edt(~ha, sampling=PIXDIM)[hb]; t4 = time.perf_counter()
    hd, hd95 = float(max(da.max(), db.max())), float(np.percentile(np.concatenate([da, db]), 95.0))
    assd = (math.fsum(da) / len(da) + math.fsum(db) / len(db)) / 2.0
    tp = int(np.count_nonzero(hp & ht)); t5 = time.perf_counter()
    out["host_path"] = {"copy_out_ms": (t1 - t0) * 1e3, "erosions_ms": (t2 - t1) * 1e3, "edt_ms": [(t3 - t2) * 1e3, (t4 - t3) * 1e3], "reductions_ms": (t5 - t4) * 1e3,
                        "total_ms": (t5 - t0) * 1e3, "hd": hd, "hd95": hd95, "assd": assd}
    out["host_over_device"] = out["host_path"]["total_ms"] / out["score_volume_no_lesions_ms"]
    ulp = 2.0 ** -53
    assert tp == score.tp and (len(da), len(db)) == (score.n_surface_pred, score.n_surface_truth), "the host path and the device disagree on the counts"
    import volscore_oracle as SO
    for got, want, k in ((score.hd, hd, 4), (score.hd95, hd95, 4), (score.assd, assd, SO.sum_chain(N) + 5)):          # (scipy orders the three products differently; the sum's chain: DESIGN 4q)
        assert abs(got - want) <= k * ulp * abs(want), f"the host path and the device disagree: {got!r} against {want!r}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_score.json"))
    a = ap.parse_args()
    import torch
    shape = (128, 128, 64) if a.small else (512, 512, 301)
    if a.trace_call:
        from covidseg_amd import volume as V
        pred, truth = pair(shape)
        pd, _ = V._mask_to_device(pred); td, _ = V._mask_to_device(truth)
        for _ in range(3):
            sc = V.score_volume(pd, td, PIXDIM, shape=shape)
        torch.cuda.synchronize()
        print(sc)
        return
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "case": bench(shape, a.runs, not a.no_host)}
    try:
        import subprocess
        res["clocks"] = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip().splitlines()[-12:]
    except Exception as e:                                           # noted, not needed
        res["clocks"] = f"unavailable: {e}"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

"""Times the component step (unet_vol_label / unet_vol_component_stats / unet_vol_filter_components) on a 512 x 512 x 301 mask -- 300 random ellipsoids with and
without 0.2 % salt noise -- and the host path it replaces on the same box: mask device -> host, scipy.ndimage.label (the numpy oracle where scipy is absent),
labels host -> device.  tools/volume_bench.py's method: warm-up, median of `--runs`, device events around the entries.  Writes profiles/components.json.

    python tools/components_bench.py [--runs 10] [--small]        (--small: 128 x 128 x 64, a functional check of the tool)
    python tools/components_bench.py --trace-call [--noise 0.002]  three label + stats + filter calls and nothing else (for a kernel trace: per-launch times)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12


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


def bench_case(shape, noise, runs):
    import torch
    import components_oracle as CO
    from covidseg_amd import volume as V
    lib, ctx = V._ctx()
    X, Y, Z = shape
    N = X * Y * Z
    m = CO.ellipsoids(shape, 300, noise, 5)
    dev, _ = V._mask_to_device(m)
    labels = torch.empty(N, dtype=torch.int32, device="cuda")
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.unet_vol_label_ws_bytes(X, Y, Z)), dtype=torch.uint8, device="cuda")
    s = V._stream()
    run_label = lambda: ctx.check(lib.unet_vol_label(ctx.handle, dev.data_ptr(), X, Y, Z, 1, labels.data_ptr(), n_dev.data_ptr(), ws.data_ptr(), ws.numel(), s))
    out = {"shape": list(shape), "noise": noise, "foreground": int(np.count_nonzero(m))}
    # the least the seven launches move: mask in + labels out (local), labels in + out twice (flatten, final), the flags zeroed, written and read twice
    out["vol_label"] = entry(event_ms(run_label, runs), N * (1 + 4) + 2 * N * 8 + 3 * N)
    n = int(n_dev.item())
    out["components"] = n
    st = torch.empty(max(n, 1) * 64, dtype=torch.uint8, device="cuda")
    run_stats = lambda: ctx.check(lib.unet_vol_component_stats(ctx.handle, labels.data_ptr(), X, Y, Z, n, st.data_ptr(), s))
    out["vol_component_stats"] = entry(event_ms(run_stats, runs), N * 4 + n * 64)
    keep = torch.ones(n + 1, dtype=torch.uint8, device="cuda"); keep[0] = 0
    mask2 = torch.empty(N, dtype=torch.uint8, device="cuda"); counts = torch.empty(Z, dtype=torch.int64, device="cuda")
    run_filter = lambda: ctx.check(lib.unet_vol_filter_components(ctx.handle, labels.data_ptr(), keep.data_ptr(), n, X, Y, Z, 0, Z, mask2.data_ptr(), counts.data_ptr(), s))
    out["vol_filter_components"] = entry(event_ms(run_filter, runs), N * 5)
    out["label_stats_filter_ms"] = event_ms(lambda: (run_label(), run_stats(), run_filter()), runs)
    try:
        from scipy import ndimage as ndi
        host_label, how = (lambda a: ndi.label(a)[0]), "scipy.ndimage.label"
    except ImportError:
        host_label, how = (lambda a: CO.label(a, 1)[0]), "numpy oracle"
    ts = []
    for _ in range(max(2, runs // 3)):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        h = dev.cpu().numpy().reshape(shape, order="F"); t1 = time.perf_counter()
        lab = host_label(h); t2 = time.perf_counter()
        back = torch.from_numpy(np.asfortranarray(lab.astype(np.int32)).reshape(-1, order="F")).cuda(); torch.cuda.synchronize(); t3 = time.perf_counter()
        ts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    out["host_path"] = {"labeller": how, "copy_out_ms": statistics.median(t[0] for t in ts), "label_ms": statistics.median(t[1] for t in ts),
                        "copy_back_ms": statistics.median(t[2] for t in ts), "total_ms": statistics.median(sum(t) for t in ts)}
    assert torch.equal(back, labels), "the host labeller and the device disagree"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--trace-call", action="store_true")
    ap.add_argument("--noise", type=float, default=0.002)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.json"))
    a = ap.parse_args()
    import torch
    shape = (128, 128, 64) if a.small else (512, 512, 301)
    if a.trace_call:
        import components_oracle as CO
        from covidseg_amd import volume as V
        dev, _ = V._mask_to_device(CO.ellipsoids(shape, 300, a.noise, 5))
        for _ in range(3):
            labels, n = V.label_device(dev, shape, 1)
            stt = V.component_stats_device(labels, shape, n)
            V.filter_components(labels, np.ones(n + 1, bool), n, shape)
        torch.cuda.synchronize()
        print("components:", n, "voxels in components:", int(stt["voxels"].sum()))
        return
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"),
           "cases": [bench_case(shape, noise, a.runs) for noise in (0.002, 0.0)]}
    try:
        import subprocess
        res["clocks"] = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip().splitlines()[-12:]
    except Exception as e:                                           # noted, not needed
        res["clocks"] = f"unavailable: {e}"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

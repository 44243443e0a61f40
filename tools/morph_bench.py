"""Times the binary morphology (unet_vol_morph / unet_vol_ball / unet_vol_label_planar / unet_vol_fill_holes) on the 512 x 512 x 301 test volume -- 300 random
ellipsoids + 0.2 % salt noise, spacing (0.7, 0.7, 1.25) --, the chain close(2) -> fill_holes -> remove_small on the device, and the host path that chain replaces on
the same box: mask device -> host, scipy.ndimage.binary_closing / binary_fill_holes, a scipy label + bincount filter, host -> device.  The two paths must give equal
masks.  tools/volscore_bench.py's method: warm-up, median of `--runs`, device events around the entries.  Writes profiles/volume_morph.json.

    python tools/morph_bench.py [--runs 10] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
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
PIXDIM = (0.7, 0.7, 1.25)
MIN_VOXELS = 30


def event_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def wall_ms(fn, runs, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def entry(ms, byts, **kw):
    return dict({"ms": ms, "bytes": int(byts), "TBps": byts / ms / 1e9, "of_8TBps": byts / (ms * 1e-3) / HBM}, **kw)


def bench(shape, runs, host):
    import torch
    import components_oracle as CO
    from covidseg_amd import _lib, volume as V
    lib, ctx = V._ctx()
    X, Y, Z = shape
    N = X * Y * Z
    m = CO.ellipsoids(shape, 300, 0.002, 5)
    dev, _ = V._mask_to_device(m)
    s = V._stream()
    out = {"shape": list(shape), "pixdim": list(PIXDIM), "foreground_voxels": int(m.sum())}
    res = torch.empty(N, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(Z, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_morph_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    packed = ((X + 63) // 64) * 8 * Y * Z                            # bytes of one packed volume

    def morph(op, c, planar, it):
        return lambda: ctx.check(lib.unet_vol_morph(ctx.handle, dev.data_ptr(), X, Y, Z, _lib.MORPH_OPS[op], c, planar, it, 0, res.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), s))
    # bytes: the byte volume in and out, one packed volume written by the pack and read by the unpack, one read and one written per step
    for name, op, c, planar, it in (("dilate_c1_x1", "dilate", 1, 0, 1), ("erode_c1_x1", "erode", 1, 0, 1), ("dilate_c3_x1", "dilate", 3, 0, 1), ("close_c1_x2", "close", 1, 0, 2),
                                    ("open_c3_x2", "open", 3, 0, 2), ("close_c2_x2_planar", "close", 2, 1, 2), ("dilate_c1_x16", "dilate", 1, 0, 16), ("dilate_c1_x64", "dilate", 1, 0, 64)):
        steps = it * (2 if op in ("open", "close") else 1)
        out["vol_morph_" + name] = entry(event_ms(morph(op, c, planar, it), runs), 2 * N + 2 * packed + steps * 2 * packed, launches=2 + steps)
    e1, e64 = out["vol_morph_dilate_c1_x1"]["ms"], out["vol_morph_dilate_c1_x64"]["ms"]
    out["ms_per_step"] = (e64 - e1) / 63.0
    d2 = V.edt_sq_device(dev, shape, PIXDIM, True)
    out["vol_ball"] = entry(event_ms(lambda: ctx.check(lib.unet_vol_ball(ctx.handle, d2.data_ptr(), X, Y, Z, 4.0, 1, res.data_ptr(), counts.data_ptr(), s)), runs), 9 * N)
    del d2
    out["dilate_mm_2mm_ms"] = wall_ms(lambda: V.ball_device(dev, shape, 2.0, PIXDIM, True), runs)
    out["close_mm_2mm_ms"] = wall_ms(lambda: V.ball_device(V.ball_device(dev, shape, 2.0, PIXDIM, True)[0], shape, 2.0, PIXDIM, False), runs)
    labels = torch.empty(N, dtype=torch.int32, device="cuda"); n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    lws = torch.empty(max(int(lib.unet_vol_label_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    for name, fn, c in (("vol_label_c1", lib.unet_vol_label, 1), ("vol_label_planar_c1", lib.unet_vol_label_planar, 1), ("vol_label_planar_c2", lib.unet_vol_label_planar, 2)):
        out[name] = {"ms": event_ms(lambda: ctx.check(fn(ctx.handle, dev.data_ptr(), X, Y, Z, c, labels.data_ptr(), n_dev.data_ptr(), lws.data_ptr(), lws.numel(), s)), runs),
                     "components": int(n_dev.item())}
    del labels, lws
    fws = torch.empty(max(int(lib.unet_vol_fill_holes_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    for name, c, planar in (("vol_fill_holes_c1", 1, 0), ("vol_fill_holes_c1_planar", 1, 1)):
        fh = lambda: ctx.check(lib.unet_vol_fill_holes(ctx.handle, dev.data_ptr(), X, Y, Z, c, planar, res.data_ptr(), counts.data_ptr(), fws.data_ptr(), fws.numel(), s))
        out[name] = {"ms": event_ms(fh, runs), "filled_voxels": int(counts.sum().item()) - int(m.sum())}
    del fws
    steps = [("close", {"iterations": 2}), ("fill_holes", {}), ("remove_small", {"min_voxels": MIN_VOXELS})]
    chain = lambda: V.postprocess_device(dev, shape, steps, PIXDIM)
    out["chain_close2_fill_remove_small_ms"] = wall_ms(chain, runs)
    got = chain()[0].cpu().numpy().reshape(shape, order="F")
    out["chain_voxels"] = int(got.sum())
    if not host:
        return out
    try:
        from scipy import ndimage as ndi
    except ImportError:
        out["host_path"] = "scipy does not import here: the host path was not timed"
        return out
    torch.cuda.synchronize(); t0 = time.perf_counter()
    h = dev.cpu().numpy().reshape(shape, order="F") != 0; t1 = time.perf_counter()
    closed = ndi.binary_closing(h, iterations=2); t2 = time.perf_counter()
    filled = ndi.binary_fill_holes(closed); t3 = time.perf_counter()
    lab, n = ndi.label(filled)
    keep = np.bincount(lab.reshape(-1), minlength=n + 1) >= MIN_VOXELS; keep[0] = False
    kept = keep[lab]; t4 = time.perf_counter()
    back = torch.from_numpy(np.asfortranarray(kept.astype(np.uint8)).reshape(-1, order="F")).cuda(); torch.cuda.synchronize(); t5 = time.perf_counter()
    del back
    out["host_path"] = {"copy_out_ms": (t1 - t0) * 1e3, "binary_closing_ms": (t2 - t1) * 1e3, "binary_fill_holes_ms": (t3 - t2) * 1e3, "remove_small_ms": (t4 - t3) * 1e3,
                        "copy_back_ms": (t5 - t4) * 1e3, "total_ms": (t5 - t0) * 1e3}
    out["host_over_device"] = out["host_path"]["total_ms"] / out["chain_close2_fill_remove_small_ms"]
    assert np.array_equal(got, kept), f"the host path and the device disagree on {np.count_nonzero(got != kept)} voxels"
    out["host_equals_device"] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_morph.json"))
    a = ap.parse_args()
    import torch
    shape = (128, 128, 64) if a.small else (512, 512, 301)
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

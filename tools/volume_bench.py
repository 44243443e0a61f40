"""Times the volume path: load_volume(kind="cts") and segment_volume for an int16 512 x 512 x 301 and a 630 x 630 x 45 volume (.nii.gz input), per kernel the
achieved bytes per second against the 8 TB/s of HBM, and the same steps on the CPU (the vectorised restatement of tests/volume_oracle.py and the numpy-in /
numpy-out preprocess wrappers).  Warm-up first, median of `--runs` timed runs, device events around the kernels.  Writes profiles/volume_pipeline.json.

    python tools/volume_bench.py [--runs 10] [--small]        (--small: 128 x 128 x 40, a functional check of the tool)
    python tools/volume_bench.py --trace-call                 one load_volume(kind="cts") call and nothing else (for a memory-copy trace)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12


def make_volume(X, Y, Z, seed=0):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    base = 1200 * np.exp(-(((x - X / 2) / (X / 3)) ** 2 + ((y - Y / 2) / (Y / 3)) ** 2))
    vol = np.empty((X, Y, Z), np.int16, order="F")
    for z in range(Z):
        vol[:, :, z] = (base * (0.8 + 0.2 * np.sin(z / 9.0)) + rng.normal(0, 40, (X, Y))).astype(np.int16)
    return vol


def write_ct(path, vol):
    import gzip, struct
    from covidseg_amd import nifti_min
    h = bytearray(nifti_min.default_header(vol.shape, (0.7, 0.7, 1.0)))
    struct.pack_into("<2h", h, 70, 4, 16); struct.pack_into("<3f", h, 108, 352.0, 1.0, -1024.0)
    with open(path, "wb") as f:
        f.write(gzip.compress(bytes(h) + b"\0\0\0\0" + vol.tobytes(order="F"), 1))


def median_ms(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def event_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def bench_case(X, Y, Z, S, d, runs, model):
    import torch
    from covidseg_amd import nifti_min, volume as V, preprocess as PRE
    import volume_oracle as VO
    vol_np = make_volume(X, Y, Z)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "ct.nii.gz")
    write_ct(path, vol_np)
    z0, z1 = V.trim_range(Z); n = z1 - z0
    r1, r2 = V.whole_frame_rects(n, S); rects = (r1, r2, list(range(n)))
    out = {"shape": [X, Y, Z], "kept_slices": n, "img_size": S, "model_size": d}
    out["decode_gzip_ms"] = median_ms(lambda: nifti_min.read(path), runs, 1)
    vol = nifti_min.read(path)
    out["upload_ms"] = median_ms(lambda: (V.upload(vol), torch.cuda.synchronize()), runs)
    dev = V.upload(vol)
    item = vol.raw.dtype.itemsize
    ms = event_ms(lambda: V.slices_f64(vol, dev, z0, z1, S, ("u8",)), runs)
    byts = n * (X * Y * item * 2 + S * S * (8 + 8 + 1))                # voxels twice (resize + uniform test), float64 stage written and read, uint8 out
    out["vol_slices_f64"] = {"ms": ms, "bytes": byts, "TBps": byts / ms / 1e9, "of_8TBps": byts / (ms * 1e-3) / HBM}
    prob = torch.rand((n, d, d), device="cuda")
    R1 = np.asarray(r1, np.int32); R2 = np.asarray(r2, np.int32)
    ms = event_ms(lambda: V.paste_back(prob, R1, R2, S), runs)
    byts = n * (d * d * 4 + S * S * 4)
    out["vol_paste_back"] = {"ms": ms, "bytes": byts, "TBps": byts / ms / 1e9, "of_8TBps": byts / (ms * 1e-3) / HBM}
    canvas = V.paste_back(prob, R1, R2, S)
    ms = event_ms(lambda: V.unslice(canvas, 0.5, (X, Y, Z), z0, z1), runs)
    byts = n * S * S * 4 + X * Y * Z + X * Y * n
    out["vol_unslice"] = {"ms": ms, "bytes": byts, "TBps": byts / ms / 1e9, "of_8TBps": byts / (ms * 1e-3) / HBM}
    out["load_volume_cts_ms"] = median_ms(lambda: (V.load_volume(path, "cts", S, rects=rects, box_indexing="slice", new_dim=d), torch.cuda.synchronize()), runs)
    out["load_volume_cts_device_part_ms"] = median_ms(lambda: (V.load_volume(vol, "cts", S, rects=rects, box_indexing="slice", new_dim=d), torch.cuda.synchronize()), runs)
    seg = []
    def run_seg():
        seg.append(V.segment_volume(path, model, batch_size=32, img_size=S).seconds)
    out["segment_volume_ms"] = median_ms(run_seg, max(3, runs // 3), 1)
    out["segment_volume_split_ms"] = {k: statistics.median(s[k] for s in seg[1:]) * 1e3 for k in seg[0]}
    # CPU, same box: the vectorised restatement (decode + rot90 + resize + min-max) and the composed path through the numpy-in / numpy-out wrappers
    few = min(n, 8)
    t0 = time.perf_counter(); st = VO.slices_f64(vol.raw, vol.slope, vol.inter, z0, z0 + few, S); t_cpu = (time.perf_counter() - t0) / few * n * 1e3
    out["cpu_restatement_slices_ms_extrapolated"] = t_cpu
    raw_f32 = np.stack([st["img64"][i] for i in range(few)]).astype(np.float32)
    t0 = time.perf_counter(); PRE.prepare_cts(raw_f32, r1[:few], r2[:few], new_dim=d); out["numpy_wrappers_prepare_cts_ms_extrapolated"] = (time.perf_counter() - t0) / few * n * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--trace-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_pipeline.json"))
    a = ap.parse_args()
    import torch
    from covidseg_amd import volume as V
    if a.trace_call:
        vol = make_volume(512, 512, 40)
        n = 24
        r1, r2 = V.whole_frame_rects(n, 512)
        x = V.load_volume(vol, "cts", 512, rects=(r1, r2, list(range(n))), box_indexing="slice", new_dim=224)
        torch.cuda.synchronize()
        print("load_volume(cts):", tuple(x.shape), x.device, "voxel buffer bytes", vol.nbytes)
        return
    from covidseg_amd.keras_like import UNetModel
    d = 64 if a.small else 224
    model = UNetModel(d, 1, seed=0); model.verbose = 0
    cases = [(128, 128, 40, 128)] if a.small else [(512, 512, 301, 512), (630, 630, 45, 512)]
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "cases": [bench_case(X, Y, Z, S, d, a.runs, model) for X, Y, Z, S in cases]}
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

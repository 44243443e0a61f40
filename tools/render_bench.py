"""Times volume.render_planes for six axial planes plus one coronal maximum projection of a synthetic 512 x 512 x 301 int16 volume (slope 0.5, inter -1024, spacing
(0.7, 0.7, 1.25)) with a lesion mask and a lung mask as layers, both already on the device, and the host route it replaces: the download of the mask plus the numpy
drawing of the same sheet (tests/render_oracle.py) on the box's threads, timed once.  Method: two warm runs, then the median of `--runs` wall times with a device
synchronisation on both sides of the clock; the projection and the canvas kernel alone with device events.  Writes profiles/volume_render.json.

    python tools/render_bench.py [--runs 5] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
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
PIXDIM = (0.7, 0.7, 1.25)


def wall_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def event_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def bench(shape, runs, host):
    import torch
    import components_oracle as CO
    import render_oracle as RO
    from covidseg_amd import nifti_min, volume as V
    X, Y, Z = shape
    rng = np.random.default_rng(3)
    raw = np.asfortranarray(rng.integers(0, 3000, shape).astype(np.int16))
    vol = nifti_min.NiftiVolume(raw, 0.5, -1024.0, PIXDIM, nifti_min.default_header(shape, PIXDIM), "<")
    inf = np.asfortranarray(CO.ellipsoids(shape, 200, 0.0, 7).astype(np.uint8))
    lung = np.asfortranarray(CO.ellipsoids(shape, 2, 0.0, 9).astype(np.uint8))
    inf_dev, _ = V._mask_to_device(inf)
    lung_dev, _ = V._mask_to_device(lung)
    dev = V.upload(vol)
    counts = inf.sum(axis=(0, 1))
    planes = [("axial", z) for z in (V.key_slices(counts, 6) or [Z // 2])] + [("mip", "coronal", 0, Y)]
    layers = [V.Layer(inf_dev), V.Layer(lung_dev, V.PALETTE_LUNG, 0, 255)]
    out = {"shape": list(shape), "pixdim": list(PIXDIM), "planes": [list(p) for p in planes]}

    def device():
        return V.render_planes(vol, planes, layers, shape=shape, _dev=dev)
    med, ts = wall_ms(device, runs)
    sheet = device()
    out.update(render_planes_ms=med, all_ms=ts, sheet=list(sheet.image.shape), launches=sheet.launches)
    out["render_planes_with_upload_ms"], _ = wall_ms(lambda: V.render_planes(vol, planes, layers, shape=shape), runs, 1)
    vargs = V._vox_args(vol)
    ldev = [(inf_dev, 2), (lung_dev, 2)]
    ms = event_ms(lambda: V.project_device(vargs, dev, 1, 0, Y, 0, ldev), runs)
    byts = X * Y * Z * (raw.itemsize + 2)
    out["vol_project_coronal"] = {"ms": ms, "bytes": byts, "TBps": byts / ms / 1e9}
    ms = event_ms(lambda: V.project_device(vargs, dev, 0, 0, X, 0, ldev), runs)
    out["vol_project_sagittal"] = {"ms": ms, "bytes": byts, "TBps": byts / ms / 1e9}
    if not host:
        return out
    t0 = time.perf_counter()
    mask_host = inf_dev.cpu().numpy().reshape(shape, order="F")     # the download the host route begins with
    t1 = time.perf_counter()
    fd = vol.get_fdata()
    want, _ = RO.sheet(fd, PIXDIM, planes, [(mask_host, V.PALETTE_INFECTION, 128, 255), (lung, V.PALETTE_LUNG, 0, 255)], V.WINDOWS["lung"], V.BONE)
    t2 = time.perf_counter()
    out["host_path"] = {"mask_download_ms": (t1 - t0) * 1e3, "numpy_sheet_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}
    out["host_over_device"] = out["host_path"]["total_ms"] / out["render_planes_ms"]
    out["sheets_equal"] = bool(np.array_equal(sheet.image, want))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_render.json"))
    a = ap.parse_args()
    import torch
    shape = (128, 128, 64) if a.small else (512, 512, 301)
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "case": bench(shape, a.runs, not a.no_host)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

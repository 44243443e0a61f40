"""Times volume.resample_volume on a synthetic 512 x 512 x 301 int16 volume (slope 0.5, inter -1024, spacing (0.7, 0.7, 1.25), stored "LPS"): (a) to 1 mm isotropic,
trilinear, float32; (b) reoriented "LPS" -> "RAS" with the stored elements kept (volume.reorient_volume); and the host route they replace,
scipy.ndimage.affine_transform(order=1) of the decoded volume on the box's threads, timed once.  Method: two warm runs, then the median of `--runs` wall times with a
device synchronisation on both sides of the clock; the kernels alone (the voxels already uploaded) with device events.  Writes profiles/volume_resample.json.

    python tools/resample_bench.py [--runs 5] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
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
    from covidseg_amd import nifti_min, volume as V
    rng = np.random.default_rng(3)
    raw = np.asfortranarray(rng.integers(0, 3000, shape).astype(np.int16))
    A = nifti_min.affine_from_axcodes("LPS", PIXDIM)
    vol = nifti_min.NiftiVolume(raw, 0.5, -1024.0, PIXDIM, nifti_min.header_with_affine(shape, A), "<")
    dev = V.upload(vol)
    vargs = V._vox_args(vol)
    target, M = V.resample_target(V.Grid.of(vol), spacing=(1.0, 1.0, 1.0))
    n_out = int(np.prod(target.shape))
    out = {"shape": list(shape), "pixdim": list(PIXDIM), "isotropic_shape": list(target.shape)}
    med, ts = wall_ms(lambda: V.resample_volume(vol, spacing=(1.0, 1.0, 1.0), return_device=True), runs)
    out["resample_volume_1mm_linear_ms"], out["all_ms"] = med, ts
    ms = event_ms(lambda: V.resample_linear_device(dev, vargs, M, 0, 0.0, target.shape, 16), runs)
    byts = raw.nbytes + 4 * n_out                                    # every source voxel once, every output once
    out["vol_resample_linear"] = {"ms": ms, "bytes": byts, "TBps": byts / ms / 1e9}
    Mr, rshape = V.reorient_matrix(shape, "LPS", "RAS")
    med, _ = wall_ms(lambda: V.reorient_volume(vol, "RAS", return_device=True), runs)
    out["reorient_LPS_to_RAS_ms"] = med
    ms = event_ms(lambda: V.resample_nearest_device(dev, 2, shape, Mr, 0, 0, rshape), runs)
    out["vol_resample_nearest_LPS_to_RAS"] = {"ms": ms, "bytes": 2 * raw.nbytes, "TBps": 2 * raw.nbytes / ms / 1e9}
    Mp, pshape = V.reorient_matrix(shape, "LPS", "PSR")             # source x feeds output z: the transposing kernel
    ms = event_ms(lambda: V.resample_nearest_device(dev, 2, shape, Mp, 0, 0, pshape), runs)
    out["vol_resample_nearest_LPS_to_PSR"] = {"ms": ms, "bytes": 2 * raw.nbytes, "TBps": 2 * raw.nbytes / ms / 1e9}
    if not host:
        return out
    import scipy.ndimage as ndi
    got = V.resample_volume(vol, spacing=(1.0, 1.0, 1.0), dtype="float64").data
    t0 = time.perf_counter()
    fd = vol.get_fdata()
    want = ndi.affine_transform(fd, M[:, :3], M[:, 3], target.shape, order=1, mode="nearest")
    t1 = time.perf_counter()
    out["host_path"] = {"scipy_affine_transform_ms": (t1 - t0) * 1e3}
    out["host_over_device"] = out["host_path"]["scipy_affine_transform_ms"] / out["resample_volume_1mm_linear_ms"]
    out["max_abs_difference_to_scipy"] = float(np.abs(got - want).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_resample.json"))
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

"""Times the rank filter (unet_vol_rank_filter) and filters.gaussian_filter on a synthetic 512 x 512 x 301 int16 CT: the 7-voxel cross, the 27-box and the 125-box at the
median, the minimum and the maximum, and the Gaussian at sigma = 1, and sets them against scipy.ndimage on the same box where it is installed (tests/filter_oracle.py
otherwise) -- the reference, never the code under test; where the reference ran, the device result is also compared with it for equality.
tools/texture_bench.py's method: warm-up, median of `--runs`, device events around the entry (the voxels already uploaded), the clocks noted.  Per case: voxels / s, and
the staged bytes per voxel -- the keys' source elements a workgroup reads for a brick and its halo over the brick's 2,048 voxels, plus the element written.
Writes profiles/filters.json.

    python tools/filter_bench.py [--runs 10] [--small] [--no-host] [--host-max-n 125]      (--small: 128 x 128 x 64, a functional check of the tool;
                                                                                            --host-max-n: the largest footprint the reference is run on)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
BRICK = (32, 8, 8)


def note(msg):
    print(f"[filter_bench] {msg}", file=sys.stderr, flush=True)


def event_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def synthetic_ct(shape, seed=1):
    """tools/texture_bench.py's volume: a slow Hounsfield-like wave plus noise"""
    rng = np.random.default_rng(seed)
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    wave = (-650.0 + 250.0 * np.sin(x / 9.0) * np.cos(y / 11.0) + 120.0 * np.sin(z / 5.0)).astype(np.float32)
    return np.asfortranarray((wave + 60.0 * rng.standard_normal(shape, dtype=np.float32)).astype(np.int16))


def staged_bytes_per_voxel(R, elem_bytes):
    staged = np.prod([b + 2 * R for b in BRICK])
    return float(staged * elem_bytes / np.prod(BRICK) + elem_bytes)


def bench(shape, runs, host, host_max_n):
    import torch
    import filter_oracle as FO
    from covidseg_amd import filters as F, volume as V
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    ct = synthetic_ct(shape)
    N = int(np.prod(shape))
    dev = torch.from_numpy(np.ascontiguousarray(ct.reshape(-1, order="F"))).cuda()
    out = {"reference": ("scipy.ndimage " + __import__("scipy").__version__) if ndi is not None else "tests/filter_oracle.py", "cases": {}}
    for fname, fp in (("cross7", F.structure(1)), ("box27", np.ones((3, 3, 3), bool)), ("box125", np.ones((5, 5, 5), bool))):
        R, lo, hi = F.footprint_bits(fp)
        n = int(fp.sum())
        for rname, rank in (("median", n // 2), ("minimum", 0), ("maximum", n - 1)):
            call = lambda: F.rank_filter_device(dev, 4, shape, R, lo, hi, rank, F.MODES["reflect"], 0)
            ms = event_ms(call, runs)
            res = {"ms": ms, "voxels_per_s": N / (ms * 1e-3), "staged_bytes_per_voxel": staged_bytes_per_voxel(R, 2), "n": n, "rank": rank, "mode": "reflect"}
            if host and n <= host_max_n:
                t0 = time.perf_counter()
                want = ndi.rank_filter(ct, rank, footprint=fp, mode="reflect") if ndi is not None else FO.rank_filter(ct, rank, fp, "reflect")
                res["reference_s"] = time.perf_counter() - t0
                got = V._host_of(call(), np.int16, shape)
                assert np.array_equal(got, want), f"{fname} {rname}: the device and the reference disagree"
                res["reference_over_device"] = res["reference_s"] * 1e3 / ms
                del want, got
            out["cases"][f"{fname} {rname}"] = res
            note(f"{fname} {rname}: {ms:.3f} ms" + (f", reference {res['reference_s']:.1f} s" if "reference_s" in res else ""))
    gms = event_ms(lambda: F.gaussian_filter(dev, sigma=1.0, return_device=True, src_shape=shape), runs)
    res = {"ms": gms, "voxels_per_s": N / (gms * 1e-3), "sigma": 1.0, "note": "the int16 -> float32 decode and three passes of unet_vol_smooth_axis"}
    if host:
        a32 = ct.astype(np.float32)
        t0 = time.perf_counter()
        want = ndi.gaussian_filter(a32, 1.0, mode="nearest", radius=3) if ndi is not None else FO.gaussian_filter(a32, (1.0, 1.0, 1.0))
        res["reference_s"] = time.perf_counter() - t0
        got = F.gaussian_filter(dev, sigma=1.0, src_shape=shape)
        res["max_abs_difference_to_reference"] = float(np.abs(got.astype(np.float64) - want).max())
        res["reference_over_device"] = res["reference_s"] * 1e3 / gms
    out["cases"]["gaussian sigma=1"] = res
    note(f"gaussian: {gms:.3f} ms")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-max-n", type=int, default=125)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filters.json"))
    a = ap.parse_args()
    shape = (128, 128, 64) if a.small else (512, 512, 301)
    import torch
    res = {"shape": list(shape), "dtype": "int16", "runs": a.runs, "device": torch.cuda.get_device_name(0), "threads": os.environ.get("OMP_NUM_THREADS")}
    res.update(bench(shape, a.runs, not a.no_host, a.host_max_n))
    try:
        res["clocks"] = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip().splitlines()[-12:]
    except Exception as e:                                              # noqa: BLE001
        res["clocks"] = f"unavailable: {e}"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

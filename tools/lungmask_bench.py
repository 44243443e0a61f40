"""Times the lung mask found from the CT itself (unet_vol_threshold, unet_vol_geodesic_begin / _steps, lungs.lung_mask) on a synthetic 512 x 512 x 301 chest -- the
phantom of tests/lungmask_oracle.py sampled on a 128 x 128 x 76 grid, every voxel repeated 4 x 4 x 4, cropped to 301 slices, Gaussian noise of sigma = 35 HU added at
full size, int16 --: the two kernels under device events, lung_mask end to end, and a scipy restatement of its steps on the same box, timed once: the threshold, the
body (label, largest component, binary_fill_holes slice by slice) and `--host-steps` steps of the growth as masked binary_dilation (the growth's per-step cost is what
the host path is compared by; its whole loop is not run).  tools/morph_bench.py's method: warm-up, median of `--runs`, device events around the entries.  The figures are
a record, not pass marks.  Writes profiles/volume_lungmask.json.

    python tools/lungmask_bench.py [--runs 10] [--small] [--no-host] [--host-steps 8]      (--small: 128 x 128 x 76, a functional check of the tool)
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
COARSE = (128, 128, 76)
FOV_MM = (168.0, 144.0, 168.0)


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


def chest(small):
    """-> (int16 HU [X, Y, Z], pixdim): the phantom on the coarse grid, repeated to full size, noise added at full size"""
    import lungmask_oracle as LO
    cp = tuple(f / n for f, n in zip(FOV_MM, COARSE))
    ph = LO.phantom(leak=False, superior="z-", shape=COARSE, pixdim=cp, noise=0.0)
    hu, rep = ph["hu"], (1 if small else 4)
    if rep > 1:
        hu = np.repeat(np.repeat(np.repeat(hu, rep, axis=0), rep, axis=1), rep, axis=2)[:, :, :301]
    rng = np.random.default_rng(7)
    out = np.empty(hu.shape, np.int16, order="F")
    for z in range(hu.shape[2]):                                     # slice by slice: no float64 copy of the whole volume
        out[:, :, z] = np.rint(hu[:, :, z] + rng.normal(0.0, 35.0, hu.shape[:2])).astype(np.int16)
    return out, tuple(p / rep for p in cp)


def bench(small, runs, host, host_steps):
    import torch
    from covidseg_amd import lungs as L, volume as V
    lib, ctx = V._ctx()
    hu, pixdim = chest(small)
    shape = hu.shape
    X, Y, Z = shape
    N = X * Y * Z
    s = V._stream()
    out = {"shape": list(shape), "pixdim": list(pixdim)}
    src = V._resample_source(hu, pixdim=pixdim)
    dev = V.upload(src.vol)
    mask = torch.empty(N, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(Z, dtype=torch.int64, device="cuda")
    body = L._body_device(dev, src, L.BODY_HU)

    def threshold(region, cnt):
        return lambda: ctx.check(lib.unet_vol_threshold(ctx.handle, dev.data_ptr(), 4, X, Y, Z, 0, 1.0, 0.0, float("-inf"), L.AIR_HU, V._ptr(region), mask.data_ptr(), V._ptr(cnt), s))
    # bytes: the int16 volume in, the mask out, the region in when given
    out["vol_threshold"] = entry(event_ms(threshold(None, None), runs), 3 * N)
    out["vol_threshold_counts"] = entry(event_ms(threshold(None, counts), runs), 3 * N)
    out["vol_threshold_region_counts"] = entry(event_ms(threshold(body, counts), runs), 4 * N)
    cand = L.threshold_device(dev, src.vargs, float("-inf"), L.AIR_HU, body)[0]
    out["candidate_voxels"] = int(cand.sum(dtype=torch.int64).item())
    seed = L._find_trachea_device(cand, shape, pixdim, "z-", L._check_trachea_args())
    if seed is None:
        raise SystemExit("the bench chest has no trachea: the phantom or find_trachea changed")
    within = L._reconstruct_device(cand, seed.mask, shape, 1)
    constraint = L.threshold_device(dev, src.vargs, float("-inf"), L.AIRWAY_HU, within)[0]
    arrival = torch.empty(2 * N, dtype=torch.uint8, device="cuda")
    steps_counts = torch.zeros(L.MAX_STEP + 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.unet_vol_geodesic_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    packed = ((X + 63) // 64) * 8 * Y * Z                            # bytes of one packed volume

    def begin():
        ctx.check(lib.unet_vol_geodesic_begin(ctx.handle, seed.mask.data_ptr(), constraint.data_ptr(), X, Y, Z, arrival.data_ptr(), steps_counts.data_ptr(), ws.data_ptr(), ws.numel(), s))

    def begin_and(n):
        def fn():
            begin()
            ctx.check(lib.unet_vol_geodesic_steps(ctx.handle, X, Y, Z, 1, n, 1, 0, arrival.data_ptr(), steps_counts.data_ptr(), ws.data_ptr(), ws.numel(), s))
        return fn
    # bytes of _begin: two byte volumes in, the uint16 arrival out, three packed volumes out; of a step at least: constraint and reached in, a frontier out
    out["vol_geodesic_begin"] = entry(event_ms(begin, runs), 4 * N + 3 * packed)
    b0, b32 = out["vol_geodesic_begin"]["ms"], event_ms(begin_and(32), runs)
    out["vol_geodesic_first_32_steps_ms"] = b32 - b0
    out["ms_per_step_first_32"] = (b32 - b0) / 32.0
    out["step_min_bytes"] = 3 * packed
    t0 = time.perf_counter()
    arr, grown_counts = L.geodesic_device(seed.mask, constraint, shape, 1, False, 2000)
    torch.cuda.synchronize()
    out["growth"] = {"steps": int(grown_counts.size - 1), "voxels": int(grown_counts.sum()), "wall_ms": (time.perf_counter() - t0) * 1e3,
                     "leak_rule": list(L.leak_rule(grown_counts))}
    del arr
    res = L.lung_mask(hu, pixdim=pixdim, orientation="LPI")
    out["lung_mask"] = {"wall_ms": wall_ms(lambda: L.lung_mask(hu, pixdim=pixdim, orientation="LPI"), max(1, runs // 3)), "lung_ml": res.lung_ml, "components": len(res.components),
                        "airway_steps": int(res.airways.counts.size - 1), "leak_step": res.airways.leak_step, "stop_step": res.airways.stop_step,
                        "seconds": {k: float(v) for k, v in res.seconds.items() if not isinstance(v, list)}}
    out["lung_mask_on_device_ms"] = wall_ms(lambda: L.lung_mask(dev.view(torch.int16), src_shape=shape, pixdim=pixdim, orientation="LPI", return_device=True), max(1, runs // 3))
    if not host:
        return out
    try:
        from scipy import ndimage as ndi
    except ImportError:
        out["host_path"] = "scipy does not import here: the host path was not timed"
        return out
    t0 = time.perf_counter()
    solid = hu >= L.BODY_HU; t1 = time.perf_counter()
    lab, n = ndi.label(solid)
    big = lab == (1 + int(np.argmax(np.bincount(lab.reshape(-1), minlength=n + 1)[1:]))); t2 = time.perf_counter()
    filled = np.empty(shape, bool)
    for z in range(Z):
        filled[:, :, z] = ndi.binary_fill_holes(big[:, :, z])
    t3 = time.perf_counter()
    air = (hu < L.AIR_HU) & filled; t4 = time.perf_counter()
    hc = constraint.cpu().numpy().reshape(shape, order="F") != 0
    reached = (seed.mask.cpu().numpy().reshape(shape, order="F") != 0) & hc
    t5 = time.perf_counter()
    for _ in range(host_steps):
        reached = ndi.binary_dilation(reached, mask=hc)
    t6 = time.perf_counter()
    assert np.array_equal(air, cand.cpu().numpy().reshape(shape, order="F") != 0), "the host path and the device disagree on the candidates"
    out["host_path"] = {"threshold_ms": (t1 - t0) * 1e3, "label_largest_ms": (t2 - t1) * 1e3, "fill_holes_per_slice_ms": (t3 - t2) * 1e3, "air_in_body_ms": (t4 - t3) * 1e3,
                        "growth_steps_timed": host_steps, "growth_ms_per_step": (t6 - t5) * 1e3 / max(1, host_steps), "candidates_equal_device": True}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-steps", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_lungmask.json"))
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "case": bench(a.small, a.runs, not a.no_host, a.host_steps)}
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

"""Times the surface extraction (csrc/kernels_mesh.hip) on a synthetic 512 x 512 x 301 volume: a lung mask of two ellipsoids and an infection mask of
a few dozen blobs.  Per launch: the milliseconds (device events, warm-up first, median of `--runs`) and the achieved GB/s against the ALGORITHMIC bytes -- samples read once,
flag and count bytes written once and read once, outputs written once --, then extract_surface end to end, the shader clock and socket power of the timed region (bench.py's
sampler), and tests/mesh_oracle.py on a z-slab of the same mask on this box's CPU threads, extrapolated to the whole volume.  Writes profiles/mesh_bench.json.

    python tools/mesh_bench.py [--runs 10] [--small]        (--small: 128 x 128 x 40, a functional check of the tool)
    COVIDSEG_AMD_LIB=build/exp/libunet_mesh_loads.so python tools/mesh_bench.py --no-cpu      the count kernel with overlapping loads instead of LDS staging (make -C <package>/csrc mesh_loads)
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


def make_masks(X, Y, Z, blobs=36, seed=0):
    """-> (lungs uint8, lesions uint8) [X, Y, Z] in Fortran order: two ellipsoids, and `blobs` balls of 3..12 voxels radius inside them"""
    rng = np.random.default_rng(seed)
    x = np.arange(X, dtype=np.float32)[:, None, None]; y = np.arange(Y, dtype=np.float32)[None, :, None]; z = np.arange(Z, dtype=np.float32)[None, None, :]
    lungs = np.zeros((X, Y, Z), np.uint8, order="F")
    for cx in (0.30, 0.70):
        lungs |= (((x - cx * X) / (0.16 * X)) ** 2 + ((y - 0.5 * Y) / (0.30 * Y)) ** 2 + ((z - 0.5 * Z) / (0.42 * Z)) ** 2 < 1).astype(np.uint8)
    lesions = np.zeros((X, Y, Z), np.uint8, order="F")
    pts = np.argwhere(lungs)
    for c in pts[rng.choice(len(pts), blobs, replace=False)]:
        r = float(rng.uniform(3, 12)) * min(1.0, X / 512)
        lo = np.maximum(c - int(r) - 1, 0); hi = np.minimum(c + int(r) + 2, (X, Y, Z))
        sub = (slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
        lesions[sub] |= ((x[lo[0]:hi[0]] - c[0]) ** 2 + (y[:, lo[1]:hi[1]] - c[1]) ** 2 + (z[:, :, lo[2]:hi[2]] - c[2]) ** 2 < r * r).astype(np.uint8)
    return lungs, lesions & lungs


def event_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def rate(ms, byts):
    return {"ms": round(ms, 4), "bytes": int(byts), "GBps": round(byts / ms / 1e6, 1), "of_8TBps": round(byts / (ms * 1e-3) / HBM, 4)}


def bench_mask(name, mask, runs, pixdim=(0.7, 0.7, 1.0)):
    import torch
    from covidseg_amd import volume as V
    lib, ctx = V._ctx()
    X, Y, Z = mask.shape
    dev = torch.from_numpy(mask.reshape(-1, order="F")).cuda()
    vargs = (2, X, Y, Z, 0, 1.0, 0.0)
    M = np.diag(pixdim + (1.0,))[:3].copy(); m12 = np.ascontiguousarray(M).reshape(12)
    NP = (X + 2) * (Y + 2) * (Z + 2)
    nv, nt, ws = V.mesh_count_device(dev, "mask", vargs, 0.5, 0, True, 0.0)
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = {"mask": name, "shape": [X, Y, Z], "lattice_points": NP, "n_vertices": nv, "n_triangles": nt}

    def count():
        ctx.check(lib.unet_vol_mesh_count(ctx.handle, dev.data_ptr(), 0, *vargs, 0.5, 0, 1, 0.0, ws.data_ptr(), ws.numel(), totals.data_ptr(), V._stream()), "count")
    v = torch.empty((nv, 3), dtype=torch.float32, device="cuda"); t = torch.empty((nt, 3), dtype=torch.int32, device="cuda"); g = torch.empty(nt, dtype=torch.int32, device="cuda")

    def emit(cv, ct):
        ctx.check(lib.unet_vol_mesh_emit(ctx.handle, dev.data_ptr(), 0, *vargs, 0.5, 0, 1, 0.0, m12.ctypes.data, ws.data_ptr(), ws.numel(), v.data_ptr(), cv, t.data_ptr(),
                                         g.data_ptr(), ct, V._stream()), "emit")
    out["count_and_scan"] = rate(event_ms(count, runs), X * Y * Z + 2 * NP)                    # samples read once, flag and count bytes written once
    out["vertices"] = rate(event_ms(lambda: emit(nv, 0), runs), NP + 12 * nv)                   # flag bytes read once, vertices written once
    out["triangles"] = rate(event_ms(lambda: emit(0, nt), runs), NP + 16 * nt)                  # count bytes read once, triangles and groups written once
    emit(nv, nt)
    out["measure"] = rate(event_ms(lambda: V.mesh_measure_device(v, t), runs), 12 * nv + 12 * nt + 16 * nt)
    ts = []
    for _ in range(max(3, runs // 2)):
        torch.cuda.synchronize(); t0 = time.perf_counter(); mesh = V.extract_surface(dev, shape=(X, Y, Z), pixdim=pixdim, return_device=True); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["extract_surface_device_ms"] = round(statistics.median(ts), 3)
    out["area_mm2"], out["volume_ml"], out["euler"] = mesh.area_mm2, mesh.volume_ml, mesh.euler
    return out


def cpu_oracle_ms(mask, slab=24):
    """tests/mesh_oracle.py on the middle z-slab, extrapolated by the slice count (its intermediates need ~60 bytes per lattice point)"""
    import mesh_oracle as MO
    Z = mask.shape[2]
    k = min(slab, Z)
    z0 = (Z - k) // 2
    t0 = time.perf_counter(); r = MO.extract(mask=mask[:, :, z0:z0 + k], closed=True); MO.measure(r.vertices, r.triangles)
    return {"slab_slices": k, "slab_ms": round((time.perf_counter() - t0) * 1e3, 1), "extrapolated_ms": round((time.perf_counter() - t0) * 1e3 / k * Z, 1), "slab_triangles": len(r.triangles)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU oracle")
    a = ap.parse_args()
    import torch
    from bench import _SmiSampler
    shape = (128, 128, 40) if a.small else (512, 512, 301)
    lungs, lesions = make_masks(*shape)
    smi = _SmiSampler(0).start()
    cases = [bench_mask("lungs", lungs, a.runs), bench_mask("lesions", lesions, a.runs)]
    op = smi.stop()
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "sclk_mhz": op["sclk_mhz"], "power_w": op["power_w"],
           "library": os.environ.get("COVIDSEG_AMD_LIB") or "product", "cases": cases,
           "cpu_oracle": None if a.no_cpu else {"lungs": cpu_oracle_ms(lungs), "lesions": cpu_oracle_ms(lesions)}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

"""Times one volume.split_lungs + volume.lung_burden on a synthetic 512 x 512 x 301 fused-lung mask (two ellipsoids joined by a bar of 3.2 mm radius, spacing
(0.7, 0.7, 1.25), LPS) with 200 random ellipsoid lesions, and the same procedure restated with scipy.ndimage on the same box, timed once.  Method: two warm runs, then
the median of `--runs` wall times with a device synchronisation on both sides of the clock; the two kernels of csrc/kernels_lungside.hip alone with device events.
Writes profiles/volume_lungside.json.

    python tools/lungside_bench.py [--runs 5] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
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


def fused_mask(shape, bridge_mm=3.2):
    """slice by slice (no full-size float grids): two ellipsoids side by side along x, a few millimetres apart, joined by a round bar of radius bridge_mm between
    their centres -- the anterior junction; eroding by the first radius above bridge_mm separates them"""
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8, order="F")
    x, y = np.meshgrid(np.arange(X) / X, np.arange(Y) / Y, indexing="ij")
    bar_x = (x > 0.27) & (x < 0.735)
    for z in range(Z):
        zz = (z / Z - 0.5) / 0.45
        a = ((x - 0.27) / 0.225) ** 2 + ((y - 0.5) / 0.38) ** 2 + zz * zz <= 1.0
        b = ((x - 0.735) / 0.23) ** 2 + ((y - 0.5) / 0.40) ** 2 + zz * zz <= 1.0
        bar = bar_x & (((y - 0.5) * Y * PIXDIM[1]) ** 2 + ((z - Z // 2) * PIXDIM[2]) ** 2 <= bridge_mm ** 2)
        m[:, :, z] = a | b | bar
    return m


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


def scipy_split(m, inf, pixdim, min_ratio, radii):
    """the procedure of volume.split_lungs / lung_burden with scipy.ndimage (rounded distances: not bit for bit the device's on exact ties)"""
    from scipy import ndimage as ndi
    d_bg = ndi.distance_transform_edt(m, sampling=pixdim)
    for r in (0,) + tuple(radii):
        cand = m if r == 0 else d_bg > r
        lab, n = ndi.label(cand)
        cnt = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
        order = np.lexsort((np.arange(n), -cnt))[:2]
        if n >= 2 and cnt[order[1]] >= min_ratio * cnt[order[0]]:
            break
    else:
        raise RuntimeError("scipy: no radius separates the lungs")
    cx = [ndi.center_of_mass(lab == k + 1)[0] for k in order]
    left, right = (order[0], order[1]) if -pixdim[0] * cx[0] < -pixdim[0] * cx[1] else (order[1], order[0])          # LPS: world x = -pixdim x
    dl = ndi.distance_transform_edt(lab != left + 1, sampling=pixdim)
    dr = ndi.distance_transform_edt(lab != right + 1, sampling=pixdim)
    sides = np.where(m, np.where(dl <= dr, 1, 2), 0).astype(np.uint8)
    ll, ln = ndi.label(inf)
    table = np.zeros((ln + 1, 3), np.int64)
    np.add.at(table, (ll.reshape(-1), sides.reshape(-1)), 1)
    return r, sides, table[1:]


def bench(shape, runs, host):
    import torch
    import components_oracle as CO
    from covidseg_amd import volume as V
    lib, ctx = V._ctx()
    X, Y, Z = shape
    N = X * Y * Z
    m = fused_mask(shape)
    inf = np.asfortranarray(CO.ellipsoids(shape, 200, 0.0, 7).astype(np.uint8))
    dev, _ = V._mask_to_device(m)
    inf_dev, _ = V._mask_to_device(inf)
    out = {"shape": list(shape), "pixdim": list(PIXDIM), "lung_voxels": int(m.sum()), "infected_voxels": int(inf.sum())}

    def device():
        ls = V.split_lungs(dev, orientation="LPS", pixdim=PIXDIM, shape=shape, return_device=True)
        return ls, V.lung_burden(inf_dev, ls, pixdim=PIXDIM, shape=shape)
    med, ts = wall_ms(device, runs)
    ls, b = device()
    out.update(split_plus_burden_ms=med, all_ms=ts, radius_mm=ls.radius_mm, voxels=list(ls.voxels), lesions=len(b.lesions), left_fraction=b.left.fraction,
               right_fraction=b.right.fraction)
    out["split_lungs_ms"], _ = wall_ms(lambda: V.split_lungs(dev, orientation="LPS", pixdim=PIXDIM, shape=shape, return_device=True), runs, 1)
    out["lung_burden_ms"], _ = wall_ms(lambda: V.lung_burden(inf_dev, ls, pixdim=PIXDIM, shape=shape), runs, 1)
    # the two kernels alone: the assignment of the lung mask between two distance volumes, and the table
    seed = torch.zeros(N, dtype=torch.uint8, device="cuda"); seed[0] = 1
    d2a = V.edt_sq_device(seed, shape, PIXDIM, True); seed[0] = 0; seed[N - 1] = 1
    d2b = V.edt_sq_device(seed, shape, PIXDIM, True)
    sides = torch.empty(N, dtype=torch.uint8, device="cuda"); counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    s = V._stream()
    ms = event_ms(lambda: ctx.check(lib.unet_vol_side_assign(ctx.handle, dev.data_ptr(), d2a.data_ptr(), d2b.data_ptr(), X, Y, Z, 1, 2, sides.data_ptr(), counts.data_ptr(), s)), runs)
    byts = 2 * N + 16 * int(m.sum())                                 # the mask in, sides out, both distances where a wave holds a mask voxel (at least the mask's own)
    out["vol_side_assign"] = {"ms": ms, "bytes_at_least": byts, "TBps_at_least": byts / ms / 1e9, "of_8TBps_at_least": byts / (ms * 1e-3) / HBM}
    del d2a, d2b, seed
    labels, n = V.label_device(inf_dev, shape, 1)
    tot = torch.zeros(6, dtype=torch.int64, device="cuda"); les = torch.zeros(max(n, 1) * 3, dtype=torch.int64, device="cuda"); ps = torch.zeros(Z * 6, dtype=torch.int64, device="cuda")
    ms = event_ms(lambda: ctx.check(lib.unet_vol_side_table(ctx.handle, ls.sides.data_ptr(), inf_dev.data_ptr(), labels.data_ptr(), n, X, Y, Z, tot.data_ptr(), les.data_ptr(),
                                                            ps.data_ptr(), s)), runs)
    out["vol_side_table"] = {"ms": ms, "bytes": 6 * N, "TBps": 6 * N / ms / 1e9, "of_8TBps": 6 * N / (ms * 1e-3) / HBM, "lesions": n}
    if not host:
        return out
    try:
        import scipy.ndimage  # noqa: F401
    except ImportError:
        out["host_path"] = "scipy does not import here: the host path was not timed"
        return out
    t0 = time.perf_counter()
    r, hs, table = scipy_split(m != 0, inf != 0, PIXDIM, V.LUNG_MIN_RATIO, V.LUNG_ERODE_MM)
    out["host_path"] = {"total_ms": (time.perf_counter() - t0) * 1e3, "radius_mm": float(r)}
    out["host_over_device"] = out["host_path"]["total_ms"] / out["split_plus_burden_ms"]
    got = ls.sides.cpu().numpy().reshape(shape, order="F")
    out["host_differs_on_voxels"] = int(np.count_nonzero(got != hs))          # exact ties that scipy's rounded distances break the other way
    out["host_lesion_rows_equal"] = bool(np.array_equal(table, np.stack([b.lesions["voxels_outside"], b.lesions["voxels_left"], b.lesions["voxels_right"]], 1))) if out["host_differs_on_voxels"] == 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_lungside.json"))
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

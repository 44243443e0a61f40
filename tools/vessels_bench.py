"""Times the vesselness of a CT (unet_vol_hessian_eig, unet_vol_vesselness, vessels.vessel_mask) on the synthetic 512 x 512 x 301 chest of tools/lungmask_bench.py: per
scale the kernel under device events with and without a lung-sized region (the eroded lung mask of lungs.lung_mask), the eigenvalue entry, the Gaussian beside them
(filters.gaussian_filter on the decoded device volume), vessel_mask end to end, and the numpy restatement of one scale (tests/vessel_oracle.response) on `--host-slices`
slices of the smoothed volume, cut into slabs over 16 threads, scaled to the whole volume by the slice count.  tools/lungmask_bench.py's method: warm-up, median of
`--runs`, device events around the entries.  One run, reported as measured: there is no threshold to meet.  Writes profiles/volume_vessels.json.

    python tools/vessels_bench.py [--runs 5] [--small] [--no-host] [--host-slices 32]      (--small: 128 x 128 x 76, a functional check of the tool)
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
THREADS = 16


def host_response_ms(L32, k, dens, slices, slab=2):
    """vessel_oracle.response on the middle `slices` slices, in slabs of `slab` slices with a halo of one, over THREADS threads -> (ms, slices timed)"""
    import vessel_oracle as VO
    Z = L32.shape[2]
    n = min(int(slices), Z)
    z0 = (Z - n) // 2
    parts = [(z, min(z + slab, z0 + n)) for z in range(z0, z0 + n, slab)]

    def one(p):
        a, b = max(p[0] - 1, 0), min(p[1] + 1, Z)
        return VO.response(L32[:, :, a:b], k, dens)[:, :, p[0] - a:p[0] - a + (p[1] - p[0])]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        out = list(ex.map(one, parts))
    return (time.perf_counter() - t0) * 1e3, n, np.concatenate(out, axis=2), z0


def bench(small, runs, host, host_slices):
    import torch
    import lungmask_bench as LB
    from covidseg_amd import filters as F, lungs as L, vessels as VS, volume as V
    lib, ctx = V._ctx()
    hu, pixdim = LB.chest(small)
    shape = hu.shape
    X, Y, Z = shape
    N = X * Y * Z
    s = V._stream()
    out = {"shape": list(shape), "pixdim": list(pixdim), "sigmas_mm": list(VS.SIGMAS_MM)}
    src = V._resample_source(hu, pixdim=pixdim)
    x32 = VS._decoded_device(src)
    lungs = L.lung_mask(hu, pixdim=pixdim, orientation="LPI", return_device=True).mask
    region = V.ball_device(lungs, shape, 2.0, pixdim, False)[0]
    out["lung_voxels"], out["region_voxels"] = int(lungs.sum(dtype=torch.int64).item()), int(region.sum(dtype=torch.int64).item())
    dens = VS.denominators()
    best = torch.empty(N, dtype=torch.float32, device="cuda")
    scale = torch.empty(N, dtype=torch.uint8, device="cuda")
    eig = torch.empty(3 * N, dtype=torch.float32, device="cuda")
    per_scale = []
    for i, sigma in enumerate(VS.SIGMAS_MM):
        k = VS.hessian_factors(sigma, pixdim)
        sm = VS._smoothed(x32, shape, pixdim, sigma)

        def vess(reg, index):
            return lambda: ctx.check(lib.unet_vol_vesselness(ctx.handle, sm.data_ptr(), X, Y, Z, k.ctypes.data, V._ptr(reg), dens[0], dens[1], dens[2], 1, index, best.data_ptr(),
                                                             scale.data_ptr(), s))

        def eigen(reg):
            return lambda: ctx.check(lib.unet_vol_hessian_eig(ctx.handle, sm.data_ptr(), X, Y, Z, k.ctypes.data, V._ptr(reg), eig.data_ptr(), s))
        # bytes: the smoothed volume in; best and scale out (index 0), the three eigenvalue volumes out; under a region its byte per voxel in
        row = {"sigma_mm": sigma, "radius_voxels": [int(np.ceil(3.0 * sigma / p)) for p in pixdim],
               "gaussian_ms": LB.event_ms(lambda: F.gaussian_filter(x32, sigma_mm=sigma, pixdim=pixdim, return_device=True, src_shape=shape), runs),
               "vol_vesselness": LB.entry(LB.event_ms(vess(None, 0), runs), 9 * N),
               "vol_vesselness_region": LB.entry(LB.event_ms(vess(region, 0), runs), 10 * N),
               "vol_hessian_eig": LB.entry(LB.event_ms(eigen(None), runs), 16 * N),
               "vol_hessian_eig_region": LB.entry(LB.event_ms(eigen(region), runs), 17 * N)}
        for key in ("vol_vesselness", "vol_vesselness_region", "vol_hessian_eig", "vol_hessian_eig_region"):
            row[key]["ns_per_voxel"] = row[key]["ms"] * 1e6 / N
        row["vol_vesselness_region"]["ns_per_region_voxel"] = row["vol_vesselness_region"]["ms"] * 1e6 / max(1, out["region_voxels"])
        vess(None, 0)()
        row["responding_voxels"] = int((best > 0).sum(dtype=torch.int64).item())
        if host and i == 1:
            host_l = V._host_of(sm, np.float32, shape)
            ms, n, want, z0 = host_response_ms(host_l, [float(v) for v in k], dens, host_slices)
            got = V._host_of(best, np.float32, shape)[:, :, z0:z0 + n]
            row["numpy_restatement"] = {"threads": THREADS, "slices_timed": n, "ms": ms, "ms_scaled_to_the_volume": ms * Z / n, "equals_device": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))}
            del host_l, got, want
        per_scale.append(row)
        del sm
    out["scales"] = per_scale
    del best, scale, eig
    res = VS.vessel_mask(hu, lungs, pixdim=pixdim, return_device=True)
    out["vessel_mask"] = {"wall_ms": LB.wall_ms(lambda: VS.vessel_mask(hu, lungs, pixdim=pixdim, return_device=True), max(1, runs // 3)), "ml": res.ml, "n_components": res.n_components}
    out["vessel_mask_on_device_ms"] = LB.wall_ms(lambda: VS.vessel_mask(x32, lungs, pixdim=pixdim, src_shape=shape, return_device=True), max(1, runs // 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-slices", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_vessels.json"))
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "case": bench(a.small, a.runs, not a.no_host, a.host_slices)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

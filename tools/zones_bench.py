"""Times the zone kernels (unet_vol_side_extents / unet_vol_zone_table) and zones.lung_zones / lung_distribution as a whole on a synthetic 512 x 512 x 301 volume -- two
ellipsoid lungs (about a sixth of the volume), a few hundred ellipsoid lesions labelled on the device, the exact distance transform of the lungs -- and sets them against
the numpy restatement (tests/zones_oracle.py) on the same box, run over z slabs on 16 threads and summed: the restatement, never the code under test.
tools/components_bench.py's method: warm-up, median of `--runs`, device events around the entries.  The bandwidth figure is the bytes the pass has to read once -- sides
and infection (or the zone map written) everywhere (1 + 1), distances and labels under the lungs (8 + 4) -- over its time, as a share of 8 TB/s.
Writes profiles/volume_zones.json.

    python tools/zones_bench.py [--runs 10] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM = 8.0e12
PIX = (0.75, 0.75, 1.0)


def note(msg):
    print(f"[zones_bench] {msg}", file=sys.stderr, flush=True)


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


def phantom(shape, lesions, seed=1):
    """-> (sides uint8: two ellipsoids along x, infection uint8: `lesions` random ellipsoids, most of them in the lungs)"""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    x, y, z = np.ogrid[0:X, 0:Y, 0:Z]
    sides = np.zeros(shape, np.uint8)
    sides[((x - 0.27 * X) / (0.2 * X)) ** 2 + ((y - 0.5 * Y) / (0.33 * Y)) ** 2 + ((z - 0.5 * Z) / (0.44 * Z)) ** 2 < 1] = 2
    sides[((x - 0.73 * X) / (0.2 * X)) ** 2 + ((y - 0.5 * Y) / (0.33 * Y)) ** 2 + ((z - 0.5 * Z) / (0.44 * Z)) ** 2 < 1] = 1
    inf = np.zeros(shape, np.uint8)
    for _ in range(lesions):
        c = (rng.uniform(0.1, 0.9) * X, rng.uniform(0.2, 0.8) * Y, rng.uniform(0.1, 0.9) * Z)
        r = rng.uniform(0.008, 0.03, 3) * np.array([X, Y, Z]) + 1.0
        lo = [max(0, int(c[k] - r[k])) for k in range(3)]; hi = [min(shape[k], int(c[k] + r[k]) + 1) for k in range(3)]
        g = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        inf[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= (sum(((g[k] - c[k]) / r[k]) ** 2 for k in range(3)) < 1).astype(np.uint8)
    return np.asfortranarray(sides), np.asfortranarray(inf)


def host_table(ZO, sides, spec, inf, labels, n, d2, threads=16, slab=8):
    """zones_oracle.zone_table over z slabs on `threads` threads, summed (the zone of a voxel depends on its own coordinates: lo[., 2] moves with the slab)"""
    Z = sides.shape[2]

    def one(z0):
        z1 = min(Z, z0 + slab)
        sp = dict(spec); sp["lo"] = spec["lo"].copy(); sp["lo"][:, 2] -= z0          # (a flipped axis counts from lo + extent - 1, which moves alike)
        return ZO.zone_table(sides[:, :, z0:z1], sp, inf[:, :, z0:z1], labels[:, :, z0:z1], n, d2[:, :, z0:z1])
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(0, Z, slab)))
    out = {k: sum(p[k] for p in parts) for k in ("table", "outside", "lesion_zone", "lesion_shell")}
    out["lesion_dmin_key"] = np.minimum.reduce([p["lesion_dmin_key"] for p in parts])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_zones.json"))
    a = ap.parse_args()
    import torch
    import zones_oracle as ZO
    from covidseg_amd import volume as V, zones as Z
    shape = (128, 128, 64) if a.small else (512, 512, 301)
    N = int(np.prod(shape))
    sides, inf = phantom(shape, 40 if a.small else 300)
    lung = int(np.count_nonzero(sides))
    note(f"{shape}: {lung} lung voxels ({lung / N:.3f}), {int(np.count_nonzero(inf))} infected")
    ls = V.LungSides(sides=torch.from_numpy(sides.reshape(-1, order="F")).cuda(), shape=shape, axcodes=("L", "P", "S"), pixdim=PIX)
    inf_dev = torch.from_numpy(inf.reshape(-1, order="F")).cuda()
    labels, n = V.label_device(inf_dev, shape, 1)
    res = {"shape": list(shape), "lung_voxels": lung, "infected_voxels": int(np.count_nonzero(inf)), "lesions": int(n), "runs": a.runs}
    lz = Z.lung_zones(ls, return_device=True)
    import ctypes
    lib, ctx = V._ctx()
    P2, S = 2 * lz.zones * lz.ap_parts, lz.shells
    box, dmax = torch.empty(12, dtype=torch.int32, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
    table, outside = torch.empty(P2 * S * 2, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    les = [torch.empty(max(n, 1) * k, dtype=torch.int64, device="cuda") for k in (P2, S, 1)]
    zmap = torch.empty(N, dtype=torch.uint8, device="cuda")

    def extents():                                                    # the entries themselves, on buffers allocated once: the events see the launches and their memsets only
        ctx.check(lib.unet_vol_side_extents(ctx.handle, ls.sides.data_ptr(), lz.d2.data_ptr(), *shape, box.data_ptr(), dmax.data_ptr(), V._stream()), "vol_side_extents")

    def table_of(inf_t, lab_t, nn, zm):
        ctx.check(lib.unet_vol_zone_table(ctx.handle, ls.sides.data_ptr(), V._ptr(inf_t), V._ptr(lab_t), nn, lz.d2.data_ptr(), *shape, ctypes.byref(lz.spec), table.data_ptr(),
                                          outside.data_ptr(), les[0].data_ptr(), les[1].data_ptr(), les[2].data_ptr(), V._ptr(zm), V._stream()), "vol_zone_table")
    res["side_extents_ms"] = event_ms(extents, a.runs)
    for name, args, byts in (("zone_table_lungs_only", (None, None, 0, zmap), N * 2 + lung * 8),
                             ("zone_table_full", (inf_dev, labels, n, None), N * 2 + lung * 12)):
        ms = event_ms(lambda: table_of(*args), a.runs)
        res[name] = {"ms": ms, "bytes": int(byts), "TBps": byts / ms / 1e9, "of_8TBps": byts / (ms * 1e-3) / HBM}
        note(f"{name}: {ms:.3f} ms, {byts / ms / 1e9:.2f} TB/s")
    res["lung_zones_ms"] = wall_ms(lambda: Z.lung_zones(ls, return_device=True), max(3, a.runs // 3))
    res["lung_distribution_ms"] = wall_ms(lambda: Z.lung_distribution(inf_dev, lz, labels=labels, n=n, shape=shape), max(3, a.runs // 3))
    note(f"side_extents {res['side_extents_ms']:.3f} ms; lung_zones {res['lung_zones_ms']:.1f} ms; lung_distribution {res['lung_distribution_ms']:.1f} ms")
    if not a.no_host:
        d2 = lz.d2.cpu().numpy().reshape(shape, order="F")
        lab = labels.cpu().numpy().reshape(shape, order="F")
        spec = ZO.make_spec([int(v) for v in lz.spec.parts], [int(v) for v in lz.spec.flip], np.asarray(lz.spec.lo).reshape(2, 3), np.asarray(lz.spec.extent).reshape(2, 3),
                            tuple(tuple(float(lz.spec.r2[t][k]) for k in range(lz.shells - 1)) for t in (0, 1)))
        t0 = time.perf_counter()
        want = host_table(ZO, sides, spec, inf, lab, n, d2)
        res["numpy_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        got = Z.zone_table_device(ls.sides, lz.spec, shape, inf_dev, labels, n, lz.d2)
        res["equal"] = bool(all(np.array_equal(got[k], want[k]) for k in ("table", "lesion_zone", "lesion_shell", "lesion_dmin_key")) and got["outside"] == want["outside"])
        note(f"numpy restatement on 16 threads: {res['numpy_16_threads_ms']:.0f} ms; equal: {res['equal']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

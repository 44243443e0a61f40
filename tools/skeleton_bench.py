"""Times the centerlines (unet_vol_thin_*, unet_vol_skeleton_count / _emit, unet_vol_label_spread, skeleton.airway_tree / vessel_tree) on two 512 x 512 x 301 inputs: the
airway that lungs.lung_mask grows in the chest of tools/lungmask_bench.py (prepared as airway_tree prepares it: one closing, holes filled), and a synthetic vessel forest
(random tapering tubes drawn on a 128 x 128 x 76 grid, every voxel repeated 4 x 4 x 4).  Per input: iterations and launches, the milliseconds of every iteration (device
events around one-iteration calls), the table, the distance transform behind the radii, the growth and the label spread, the host graph, and the chain end to end; the
numpy restatement (tests/skeleton_oracle.py) on the same box, timed once; and, in fresh child processes on the same box:
  --ab-lib LIB     the thinning with the product library and with another build of it (COVIDSEG_AMD_LIB), alternating A B A B; the counts must agree
  --kernel-stats   a child runs under `rocprofv3 --kernel-trace --stats` and the candidate and re-check launches are read from its per-kernel table
A child that ends with a non-zero status ends the tool: nothing more is started on a card that may have faulted.  The kernel file has one predicate (two flood fills in
a register) and one work split (a lane per word); the LDS table form and the compaction to a lane per candidate were not built, so the record holds no A/B of them.
The figures are a record, not pass marks.  Writes profiles/volume_skeleton.json.

    python tools/skeleton_bench.py [--runs 5] [--small] [--no-host] [--ab-lib LIB] [--kernel-stats]      (--small: 128 x 128 x 76)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def forest(small):
    """-> uint8 [X, Y, Z]: 60 tubes from a fixed seed, radius 0.6 .. 1.6 coarse voxels, chained into a few trees"""
    import skeleton_oracle as SO
    rng = np.random.default_rng(11)
    shape = (128, 128, 76)
    segs, tips = [], [np.array([64.0, 64.0, 6.0])]
    for i in range(60):
        a = tips[int(rng.integers(0, len(tips)))] if i % 12 else rng.uniform((20, 20, 5), (108, 108, 70))
        b = np.clip(a + rng.normal(0.0, 1.0, 3) * (22.0, 22.0, 14.0), (3, 3, 3), (124, 124, 72))
        segs.append((tuple(a), tuple(b), float(rng.uniform(0.6, 1.6))))
        tips.append(b)
    vol = SO.tubes(shape, segs)
    if not small:
        vol = np.repeat(np.repeat(np.repeat(vol, 4, axis=0), 4, axis=1), 4, axis=2)[:, :, :301]
    return np.asfortranarray(vol)


def inputs(small):
    """-> {name: (uint8 host mask, pixdim)}; the airway comes from the device: lungs.lung_mask on the bench chest, then airway_tree's preparation"""
    import torch
    import lungmask_bench as LB
    from covidseg_amd import lungs as L, volume as V
    hu, pixdim = LB.chest(small)
    lm = L.lung_mask(hu, pixdim=pixdim, orientation="LPI", return_device=True)
    shape = hu.shape
    air = V.morph_device(V.morph_device(lm.airways.mask, shape, "dilate", 3, 1, 0)[0], shape, "erode", 3, 1, 1)[0]
    air = V.fill_holes_device(air, shape, 1)[0]
    torch.cuda.synchronize()
    return {"airway": (V._host_of(air, np.uint8, shape), pixdim), "vessels": (forest(small), pixdim)}


def thin_timed(mask_dev, shape, runs):
    """-> dict: begin / end ms, the ms of every iteration (median over runs), iterations, launches, removed"""
    import torch
    from covidseg_amd import volume as V
    lib, ctx = V._ctx()
    X, Y, Z = shape
    s = V._stream()
    ws = torch.empty(max(int(lib.unet_vol_thin_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    out = torch.empty(X * Y * Z, dtype=torch.uint8, device="cuda")
    per_run, begins, ends, removed = [], [], [], None

    def ev():
        return torch.cuda.Event(enable_timing=True)
    for r in range(runs + 1):                                        # the first run warms up
        e0, e1 = ev(), ev()
        e0.record(); ctx.check(lib.unet_vol_thin_begin(ctx.handle, mask_dev.data_ptr(), X, Y, Z, ws.data_ptr(), ws.numel(), s), "begin"); e1.record()
        its, rem, it = [], [], 0
        while True:
            cnt = torch.zeros(it + 1, dtype=torch.int64, device="cuda")
            a, b = ev(), ev()
            a.record(); ctx.check(lib.unet_vol_thin_iterations(ctx.handle, X, Y, Z, it, 1, 1, cnt.data_ptr(), ws.data_ptr(), ws.numel(), s), "iterations"); b.record()
            torch.cuda.synchronize()
            its.append(a.elapsed_time(b)); rem.append(int(cnt[it].item())); it += 1
            if rem[-1] == 0:
                break
        e2, e3 = ev(), ev()
        e2.record(); ctx.check(lib.unet_vol_thin_end(ctx.handle, X, Y, Z, out.data_ptr(), ws.data_ptr(), ws.numel(), s), "end"); e3.record()
        torch.cuda.synchronize()
        if r:
            per_run.append(its); begins.append(e0.elapsed_time(e1)); ends.append(e2.elapsed_time(e3))
        removed = rem
    med = [statistics.median(v) for v in zip(*per_run)]
    return {"iterations": len(removed), "launches": 2 + 54 * len(removed), "removed": removed, "begin_ms": statistics.median(begins), "end_ms": statistics.median(ends),
            "begin_ms_runs": begins, "end_ms_runs": ends,
            "iteration_ms": med, "iterations_total_ms": sum(med), "ms_per_launch": sum(med) / (54 * len(removed)), "voxels_left": int(out.sum(dtype=torch.int64).item())}, out


def wall_ms(fn, runs):
    import torch
    fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def case(name, host, pixdim, runs, with_host):
    import torch
    import skeleton_oracle as SO
    from covidseg_amd import lungs as L, skeleton as SK, volume as V
    shape = host.shape
    dev = torch.from_numpy(np.ascontiguousarray(host.reshape(-1, order="F"))).cuda()
    out = {"shape": list(shape), "voxels": int(host.sum(dtype=np.int64))}
    out["thin"], thin = thin_timed(dev, shape, runs)
    out["edt_sq_ms"] = wall_ms(lambda: V.edt_sq_device(dev, shape, pixdim, features_nonzero=False), runs)
    d2 = V.edt_sq_device(dev, shape, pixdim, features_nonzero=False)
    out["table_ms"] = wall_ms(lambda: SK.table_device(thin, shape, d2), runs)
    index, nbr, vals = SK.table_device(thin, shape, d2)
    del d2
    t0 = time.perf_counter()
    g = SK.graph_from_table(SK._finish_table(index, nbr, shape, np.sqrt(vals)), shape, pixdim)
    t1 = time.perf_counter()
    gp = SK.prune(g, SK.MIN_LENGTH_MM, SK.MIN_RATIO)
    t2 = time.perf_counter()
    out["graph"] = {"host_graph_ms": (t1 - t0) * 1e3, "host_prune_ms": (t2 - t1) * 1e3, "nodes": len(g.nodes), "branches": len(g.branches), "branches_after_prune": len(gp.branches),
                    "cycles": int(g.components["cycles"].sum())}
    idx, lab = SK.branch_seed_labels(gp)
    labels = torch.zeros(dev.numel(), dtype=torch.int32, device="cuda")
    labels[torch.from_numpy(idx).cuda()] = torch.from_numpy(lab).cuda()
    seeds = (labels != 0).to(torch.uint8)
    out["growth_ms"] = wall_ms(lambda: L.geodesic_device(seeds, dev, shape, 3), max(1, runs // 2))
    arrival, counts = L.geodesic_device(seeds, dev, shape, 3)
    steps = len(counts) - 1
    out["spread"] = {"steps": steps, "ms": wall_ms(lambda: SK.label_spread_device(arrival, labels.clone(), shape, steps, 3), runs)}
    out["spread"]["ms_per_step"] = out["spread"]["ms"] / max(1, steps)
    tree = SK.airway_tree if name == "airway" else SK.vessel_tree
    kw = dict(pixdim=pixdim, shape=shape, close=0, fill=False)
    if name == "airway":
        kw["orientation"] = "LPI"
    out["chain_from_device_ms"] = wall_ms(lambda: tree(dev, **kw), max(1, runs // 2))
    res = tree(dev, **kw)
    out["chain"] = {"seconds": {k: float(v) for k, v in res.seconds.items()}, "branches": len(res.graph.branches), "generations": len(res.generations), "cycles": res.cycles}
    if with_host:
        t0 = time.perf_counter()
        want, iterations, removed = SO.thin(host)
        out["numpy_restatement"] = {"thin_s": time.perf_counter() - t0, "threads": os.environ.get("OMP_NUM_THREADS"), "iterations": iterations,
                                    "equals_device": bool(np.array_equal(want, V._host_of(thin, np.uint8, shape)) and [int(v) for v in removed] == out["thin"]["removed"])}
    return out


def child(paths, runs):
    """the thinning of the saved inputs alone, with whatever library COVIDSEG_AMD_LIB names -> one JSON line"""
    import torch
    res = {}
    for name, path in paths.items():
        host = np.load(path)
        dev = torch.from_numpy(np.ascontiguousarray(host.reshape(-1, order="F"))).cuda()
        t, _ = thin_timed(dev, host.shape, runs)
        res[name] = {k: t[k] for k in ("iterations", "iterations_total_ms", "iteration_ms", "removed", "voxels_left")}
    print("CHILD " + json.dumps(res))


def run_child(paths, runs, lib=None, prefix=()):
    env = dict(os.environ)
    if lib:
        env["COVIDSEG_AMD_LIB"] = os.path.abspath(lib)
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", json.dumps(paths), "--runs", str(runs)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
    if p.returncode != 0 or not line:                                # a child that died may have faulted the card: nothing more is started on it
        raise SystemExit(f"skeleton_bench: the child {' '.join(cmd[:len(prefix) + 1])} ... ended with status {p.returncode}; stopping here\n{(p.stderr or p.stdout)[-2000:]}")
    return json.loads(line[-1][6:])


def kernel_stats(paths, runs):
    """a child under rocprofv3 --kernel-trace --stats (tracing only, no counters) -> the rows of its per-kernel table that belong to the thinning"""
    with tempfile.TemporaryDirectory() as d:
        run_child(paths, runs, prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                low = {k.lower(): v for k, v in r.items()}
                nm = low.get("name", "")
                for key in ("sk_candidates_kernel", "sk_recheck_kernel", "sk_pack_kernel", "sk_unpack_kernel"):
                    if key in nm:
                        rows[key] = {"calls": int(low.get("calls", 0)), "total_ms": float(low.get("totaldurationns", 0)) / 1e6, "average_us": float(low.get("averagens", 0)) / 1e3}
        return rows or {"error": "no kernel_stats.csv with the thinning kernels was written"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_skeleton.json"))
    a = ap.parse_args()
    if a.child:
        return child(json.loads(a.child), a.runs)
    import torch
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "cases": {}}
    data = inputs(a.small)
    for name, (host, pixdim) in data.items():
        res["cases"][name] = case(name, host, pixdim, a.runs, not a.no_host)
        print(name, json.dumps(res["cases"][name])[:600], flush=True)
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for name, (host, _) in data.items():
            paths[name] = os.path.join(d, name + ".npy")
            np.save(paths[name], host)
        if a.ab_lib:                                                 # A B A B, every leg a fresh process on this box
            legs = [("product", None), ("other", a.ab_lib)] * 2
            runs_ab = []
            for leg, lib in legs:                                    # (run_child ends the script on the first child that fails)
                runs_ab.append({"leg": leg, "result": run_child(paths, a.runs, lib)})
            res["ab"] = {"other": os.path.basename(a.ab_lib), "order": [l for l, _ in legs], "legs": runs_ab}
            for name in data:
                tot = {leg: [r["result"][name]["iterations_total_ms"] for r in runs_ab if r["leg"] == leg] for leg in ("product", "other")}
                same = len({json.dumps([r["result"][name]["removed"], r["result"][name]["voxels_left"]]) for r in runs_ab}) == 1
                res["ab"][name] = {"iterations_total_ms": tot, "same_counts": same}
        if a.kernel_stats:
            res["kernel_stats"] = kernel_stats(paths, 1)
    res["forms"] = "one predicate (two flood fills in a register over six shift masks) and one work split (a lane per word): no LDS table form and no compaction were built"
    try:
        res["clocks"] = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout.strip().splitlines()[-12:]
    except Exception as e:                                           # noted, not needed
        res["clocks"] = f"unavailable: {e}"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

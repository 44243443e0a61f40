"""Times the watershed (unet_vol_watershed_begin / _sweeps / _end, watershed.split_lesions) on the lesion mask the other volume benches use (tests/components_oracle.py's 300
random ellipsoids, tools/texture_bench.py and tools/volscore_bench.py) at 512 x 512 x 301 and at 128 x 128 x 76:
  per phase (HEIGHT, LABEL on it, SUM) on the cost and markers split_lesions derives from the mask: the sweeps, the per-sweep changed counts and the milliseconds of
  every sweep (device events around one-sweep calls), once with the brick skip and once without it -- the A/B of the runtime option skip of unet_vol_watershed_sweeps;
  the changed sequences of the two must agree;
  split_lesions end to end from a device mask (labelling, distance transform, cores, depth cost, both phases), wall time;
  the numpy restatement (tests/watershed_oracle.py fixed_point, rule "max") of the same cost and markers on the same box, at the small size only: at the full size a
  whole-volume numpy sweep over 79 M 64-bit keys takes seconds and the restatement needs one per step of the longest path.
The figures are a record, not pass marks.  Writes profiles/volume_watershed.json.

    python tools/watershed_bench.py [--runs 1] [--small] [--no-host]      (--small: 128 x 128 x 76 only)
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
PHASES = ("HEIGHT", "LABEL", "SUM")


def timed_phase(W, V, lib, ctx, cost, markers, mask, dims, phase, done, conn, skip, ws):
    """one phase, a sweep per call -> (changed list, ms list, begin ms)"""
    import torch
    X, Y, Z = dims
    ev = lambda: torch.cuda.Event(enable_timing=True)
    a, b = ev(), ev()
    a.record()
    ctx.check(lib.unet_vol_watershed_begin(ctx.handle, cost.data_ptr(), markers.data_ptr(), mask.data_ptr(), X, Y, Z, phase, done, ws.data_ptr(), ws.numel(), V._stream()), "begin")
    b.record(); torch.cuda.synchronize()
    begin_ms = a.elapsed_time(b)
    changed, ms = [], []
    counts = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    while True:
        s = len(changed)
        a, b = ev(), ev()
        a.record()
        ctx.check(lib.unet_vol_watershed_sweeps(ctx.handle, cost.data_ptr(), markers.data_ptr(), mask.data_ptr(), X, Y, Z, s, 1, phase, conn, skip, counts.data_ptr(), ws.data_ptr(),
                                                ws.numel(), V._stream()), "sweeps")
        b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        changed.append(int(counts[s].item()))
        if changed[-1] == 0:
            return changed, ms, begin_ms


def bench(shape, runs, host):
    import torch
    import components_oracle as CO
    import watershed_oracle as WO
    from covidseg_amd import volume as V, watershed as W
    lib, ctx = V._ctx()
    pixdim, depth, conn = (0.7, 0.7, 1.0), W.SEED_DEPTH_MM, 1
    lesions = np.asfortranarray((CO.ellipsoids(shape, 300, 0, 5) != 0).astype(np.uint8))
    mask, _ = V._mask_to_device(lesions)
    cost, markers, n_comp, n_cores, parent = W.split_inputs_device(mask, shape, pixdim, depth, conn)
    res = {"shape": list(shape), "mask_voxels": int(lesions.sum()), "pixdim": list(pixdim), "seed_depth_mm": depth, "connectivity": conn, "components": n_comp, "cores": n_cores,
           "parts": len(parent), "bricks": int(np.prod([-(-n // b) for n, b in zip(shape, (32, 8, 8))])), "phases": {}}
    ws = torch.empty(int(lib.unet_vol_watershed_ws_bytes(*shape)), dtype=torch.uint8, device="cuda")
    res["workspace_bytes"] = ws.numel()
    for skip in (1, 0):
        key = "skip" if skip else "no_skip"
        for _ in range(runs):
            ch_h, ms_h, bh = timed_phase(W, V, lib, ctx, cost, markers, mask, shape, W.HEIGHT, 0, conn, skip, ws)
            ch_l, ms_l, bl = timed_phase(W, V, lib, ctx, cost, markers, mask, shape, W.LABEL, len(ch_h), conn, skip, ws)
            ch_s, ms_s, bs = timed_phase(W, V, lib, ctx, cost, markers, mask, shape, W.SUM, 0, conn, skip, ws)
            for name, ch, ms, bm in (("HEIGHT", ch_h, ms_h, bh), ("LABEL", ch_l, ms_l, bl), ("SUM", ch_s, ms_s, bs)):
                p = res["phases"].setdefault(name, {})
                p.setdefault("changed", ch)
                assert p["changed"] == ch, (name, key)                 # the same sweeps with and without the skip, on every run
                p["sweeps"] = len(ch)
                r = p.setdefault(key, {"ms_runs": [], "begin_ms_runs": []})
                r["ms_runs"].append(round(sum(ms), 4)); r["begin_ms_runs"].append(round(bm, 4))
                r["sweep_ms"] = [round(v, 4) for v in ms]
        for name in PHASES:
            r = res["phases"][name][key]
            r["ms"] = round(statistics.median(r["ms_runs"]), 4)
    ts = []
    for _ in range(runs + 1):                                          # (the first call pays for allocations)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        parts = W.split_lesions_device(mask, shape, pixdim, depth, conn)
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    res["split_lesions"] = {"wall_ms": round(statistics.median(ts[1:]), 3), "wall_ms_runs": [round(t, 3) for t in ts], "parts": parts.n, "components": parts.n_components,
                            "sweeps": list(parts.sweeps)}
    if host:
        c = cost.cpu().numpy().view(np.uint32).reshape(shape, order="F"); m = markers.cpu().numpy().reshape(shape, order="F")
        t0 = time.perf_counter()
        want = WO.fixed_point(c, m, lesions, conn, "max")
        res["numpy"] = {"seconds": round(time.perf_counter() - t0, 3), "sweeps": list(want["sweeps"]), "threads": os.environ.get("OMP_NUM_THREADS", "unset"),
                        "equal": bool(np.array_equal(want["labels"], parts.labels.cpu().numpy().reshape(shape, order="F")))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    out = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "note": "one run unless runs says otherwise; a record, not pass marks", "cases": {}}
    out["cases"]["128x128x76"] = bench((128, 128, 76), a.runs, not a.no_host)
    if not a.small:
        out["cases"]["512x512x301"] = bench((512, 512, 301), a.runs, False)
    path = os.path.join(ROOT, "profiles", "volume_watershed.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name, c in out["cases"].items():
        print(name, {p: (v["sweeps"], v["skip"]["ms"], v["no_skip"]["ms"]) for p, v in c["phases"].items()}, "split_lesions", c["split_lesions"]["wall_ms"], "ms", c.get("numpy"))


if __name__ == "__main__":
    main()

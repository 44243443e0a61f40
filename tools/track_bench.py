"""Times the per-lesion follow-up (unet_vol_label_pairs / unet_vol_track_map, tracking.label_pairs and tracking.track_lesions as a whole) on a 512 x 512 x 301 pair at
spacing (0.7, 0.7, 1.25) -- tools/volscore_bench.py's pair: 300 random ellipsoids against their roll by (3, -2, 1) plus 20 more -- and the numpy restatement
(tests/track_oracle.py: np.unique over packed keys, the match, the maps; scipy.ndimage.label in front for the end-to-end figure) on the same box.
tools/components_bench.py's method: warm-up, median of `--runs`, device events around the entries.  Writes profiles/volume_track.json.

    python tools/track_bench.py [--runs 10] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
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


def entry(ms, byts):
    return {"ms": ms, "bytes": int(byts), "TBps": byts / ms / 1e9, "of_8TBps": byts / (ms * 1e-3) / HBM}


def pair(shape):
    import components_oracle as CO
    a = CO.ellipsoids(shape, 300, 0, 5)
    return a, np.roll(a, (3, -2, 1), axis=(0, 1, 2)) | CO.ellipsoids(shape, 20, 0, 9)


def bench(shape, runs, host):
    import torch
    from covidseg_amd import tracking as T, volume as V
    lib, ctx = V._ctx()
    X, Y, Z = shape
    N = X * Y * Z
    ma, mb = pair(shape)
    grid = V.Grid(shape, np.diag(PIXDIM + (1.0,)))
    da, _ = V._mask_to_device(ma); db, _ = V._mask_to_device(mb)
    la, n_a = V.label_device(da, shape, 1); lb, n_b = V.label_device(db, shape, 1)
    s = V._stream()
    out = {"shape": list(shape), "pixdim": list(PIXDIM), "lesions": [n_a, n_b]}
    cap = T.first_capacity(n_a, n_b)
    keys = torch.empty(cap, dtype=torch.int64, device="cuda"); counts = torch.empty(cap, dtype=torch.int64, device="cuda"); info = torch.empty(3, dtype=torch.int64, device="cuda")
    pairs_call = lambda: ctx.check(lib.unet_vol_label_pairs(ctx.handle, la.data_ptr(), n_a, lb.data_ptr(), n_b, X, Y, Z, keys.data_ptr(), counts.data_ptr(), cap, info.data_ptr(), s))
    out["vol_label_pairs"] = dict(entry(event_ms(pairs_call, runs), 8 * N), capacity=cap, info=info.cpu().tolist())
    pairs = T.label_pairs(la, n_a, lb, n_b, shape)
    match = T.match_lesions(pairs, n_a, n_b)
    out["pairs"], out["tracks"] = len(pairs), {e: match.events.count(e) for e in T.EVENTS}
    cls_a, cls_b = T.class_tables(match)
    tabs = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (match.lut_a, match.lut_b, cls_a, cls_b)]
    cls = torch.empty(N, dtype=torch.uint8, device="cuda"); ta = torch.empty(N, dtype=torch.int32, device="cuda"); tb = torch.empty(N, dtype=torch.int32, device="cuda")
    ps = torch.empty((Z, 6), dtype=torch.int64, device="cuda")
    map_call = lambda: ctx.check(lib.unet_vol_track_map(ctx.handle, la.data_ptr(), n_a, lb.data_ptr(), n_b, X, Y, Z, *(t.data_ptr() for t in tabs), cls.data_ptr(), ta.data_ptr(),
                                                        tb.data_ptr(), ps.data_ptr(), s))
    out["vol_track_map"] = entry(event_ms(map_call, runs), 8 * N + 9 * N)          # (its check of the class tables copies n + 1 bytes to the host and waits: inside the figure)
    del cls, ta, tb
    out["label_pairs_ms"] = wall_ms(lambda: T.label_pairs(la, n_a, lb, n_b, shape), runs)
    out["track_lesions_ms"] = wall_ms(lambda: T.track_lesions(da, grid, db, grid, interval_days=90, return_device=True), runs)
    res = T.track_lesions(da, grid, db, grid, interval_days=90, return_device=True)
    out["totals_ml"] = {"persistent": res.persistent_ml, "new": res.new_ml, "resolved": res.resolved_ml}
    if not host:
        return out
    import track_oracle as TO
    try:
        from scipy import ndimage as ndi
    except ImportError:
        out["host_path"] = "scipy does not import here: the host path was not timed"
        return out
    t0 = time.perf_counter()
    ha, hn_a = ndi.label(ma != 0); hb, hn_b = ndi.label(mb != 0); t1 = time.perf_counter()
    hp = TO.pairs(ha, hn_a, hb, hn_b); t2 = time.perf_counter()
    hm = TO.match(hp, hn_a, hn_b); t3 = time.perf_counter()
    hmap = TO.track_map(ha, hn_a, hb, hn_b, hm["lut_a"], hm["lut_b"], *TO.class_tables(hm)); t4 = time.perf_counter()
    out["host_path"] = {"label_s": t1 - t0, "pairs_s": t2 - t1, "match_s": t3 - t2, "maps_s": t4 - t3, "total_s": t4 - t0,
                        "note": "the per-track centroids are not part of the host figure"}
    assert (hn_a, hn_b) == (n_a, n_b) and hp.tolist() == pairs.tolist() and hm["events"] == match.events, "the host path and the device disagree"
    assert np.array_equal(hmap[3], res.per_slice) and np.array_equal(hmap[0].reshape(-1, order="F"), res.class_map.cpu().numpy()), "the host path and the device disagree on the maps"
    out["host_pairs_over_device"] = out["host_path"]["pairs_s"] * 1e3 / out["label_pairs_ms"]
    out["host_over_device"] = out["host_path"]["total_s"] * 1e3 / out["track_lesions_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_track.json"))
    a = ap.parse_args()
    import torch
    shape = (128, 128, 64) if a.small else (512, 512, 301)
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "case": bench(shape, a.runs, not a.no_host)}
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

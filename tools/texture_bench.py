"""Times the texture kernels (unet_vol_texture_quantize / _glcm / _runs) and texture.texture_stats as a whole on a synthetic 512 x 512 x 301 int16 CT, twice: under one
lung-sized group (a mask of two ellipsoids, about a sixth of the volume) and under a few hundred lesion groups (tools/volscore_bench.py's 300 random ellipsoids, labelled
on the device), and sets them against the numpy restatement (tests/texture_oracle.py) on the same box -- the restatement, never the code under test.
tools/components_bench.py's method: warm-up, median of `--runs`, device events around the entries.  The bandwidth figure of a counting kernel is the bytes of reading
`levels` (1 per voxel) and `labels` (4 per voxel, when there are labels) once, over its time, as a share of 8 TB/s.  Writes profiles/volume_texture.json.

    python tools/texture_bench.py [--runs 10] [--small] [--no-host]      (--small: 128 x 128 x 64, a functional check of the tool)
    python tools/texture_bench.py --ab build/exp/libunet_texture_loads.so [--ab-rounds 3]
        also the A/B of the GLCM kernel's staged brick against plain neighbour loads through the cache (make -C <package>/csrc texture_loads): the
        two libraries alternate, each in a fresh child process (COVIDSEG_AMD_LIB), before this process opens the device
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
HBM = 8.0e12
ALL = 0x1FFF
LO, SPAN = -1000.0, 900.0                                            # the bins cover -1000 .. -100 HU whatever their number: width = 900 / Ng


def note(msg):
    print(f"[texture_bench] {msg}", file=sys.stderr, flush=True)


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


def synthetic_ct(shape, seed=1):
    """int16 Hounsfield-like values: a slow wave (ground glass to consolidation) plus noise, so that neighbouring voxels share levels often but not always"""
    rng = np.random.default_rng(seed)
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    wave = (-650.0 + 250.0 * np.sin(x / 9.0) * np.cos(y / 11.0) + 120.0 * np.sin(z / 5.0)).astype(np.float32)
    return np.asfortranarray((wave + 60.0 * rng.standard_normal(shape, dtype=np.float32)).astype(np.int16))


def lung_mask(shape):
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    X, Y, Z = shape
    m = np.zeros(shape, bool)
    for cx in (0.29, 0.71):
        m |= ((x - cx * X) / (0.17 * X)) ** 2 + ((y - 0.5 * Y) / (0.3 * Y)) ** 2 + ((z - 0.5 * Z) / (0.42 * Z)) ** 2 <= 1.0
    return m.astype(np.uint8)


def cases(shape):
    """-> [(name, mask host or None, labels device or None, n)]"""
    import components_oracle as CO
    from covidseg_amd import volume as V
    lesions = CO.ellipsoids(shape, 300, 0, 5)
    dm, _ = V._mask_to_device(lesions)
    ld, n = V.label_device(dm, shape, 1)
    return [("one lung-sized group", lung_mask(shape), None, 1), ("lesion groups", None, ld, int(n))]


def glcm_configs(n):
    """(name, Ng, distance, bits, merge, path): both table paths, merged and unmerged"""
    from covidseg_amd import _lib
    out = []
    for Ng in (4, 16, 64):
        for merge in (True, False):
            for distance in (1, 2):
                K = 1 if merge else 13
                path = "lds" if n * K * Ng * Ng <= _lib.TEXTURE_LDS_COUNTERS else "global"
                out.append((f"Ng={Ng} {'merged' if merge else 'unmerged'} d={distance}", Ng, distance, ALL, merge, path))
    return out


def quantize_case(vol, dev, mask, labels_dev, n, Ng):
    from covidseg_amd import texture as T
    import torch
    md = torch.from_numpy(np.asfortranarray(mask).reshape(-1, order="F")).cuda() if mask is not None else None
    return md, *T.quantize_device(vol, dev, labels_dev, md, n, None, LO, SPAN / Ng, Ng, 0)


def bench_glcm(shape, runs):
    """the GLCM launches of both cases -> {case: {config: entry}} (what the A/B children run)"""
    import torch
    from covidseg_amd import volume as V
    lib, ctx = V._ctx()
    s = V._stream()
    vol = V._source(synthetic_ct(shape))
    dev = V.upload(vol)
    N = int(np.prod(shape))
    out = {}
    for name, mask, ld, n in cases(shape):
        res = {}
        for cname, Ng, distance, bits, merge, path in glcm_configs(n):
            _, lev, lc = quantize_case(vol, dev, mask, ld, n, Ng)
            K = 1 if merge else 13
            counts = torch.empty(n * K * Ng * Ng, dtype=torch.int64, device="cuda")
            call = lambda: ctx.check(lib.unet_vol_texture_glcm(ctx.handle, lev.data_ptr(), V._ptr(ld), n, *shape, Ng, distance, bits, 1 if merge else 0, counts.data_ptr(), s))
            res[cname] = entry(event_ms(call, runs), N * (5 if ld is not None else 1), path=path, pairs=int(counts.sum().item()))
            del counts, lev
        out[name] = {"groups": n, "glcm": res}
        note(f"glcm: {name} ({n} groups) done")
    return out


def bench(shape, runs, host):
    import torch
    from covidseg_amd import texture as T, volume as V
    lib, ctx = V._ctx()
    s = V._stream()
    ct = synthetic_ct(shape)
    vol = V._source(ct)
    dev = V.upload(vol)
    N = int(np.prod(shape))
    out = bench_glcm(shape, runs)
    for name, mask, ld, n in cases(shape):
        res = out[name]
        Ng = 16
        md, lev, lc = quantize_case(vol, dev, mask, ld, n, Ng)
        res["taking_part_voxels"] = int(lc.sum())
        lvb = torch.empty(N, dtype=torch.uint8, device="cuda"); lcb = torch.empty(max(n, 1) * Ng, dtype=torch.int64, device="cuda")
        qcall = lambda: ctx.check(lib.unet_vol_texture_quantize(ctx.handle, dev.data_ptr(), *V._vox_args(vol), V._ptr(ld), V._ptr(md), n, None, LO, SPAN / Ng, Ng, 0, lvb.data_ptr(),
                                                                lcb.data_ptr(), s))
        res["quantize"] = entry(event_ms(qcall, runs), N * ((4 if ld is not None else 1) + 1), note="bytes: the groups read and the levels written once; the CT is read under the groups only")
        max_run = 64
        rc = torch.empty(n * 13 * Ng * max_run, dtype=torch.int64, device="cuda"); cl = torch.empty(n * 13, dtype=torch.int64, device="cuda")
        rcall = lambda: ctx.check(lib.unet_vol_texture_runs(ctx.handle, lev.data_ptr(), V._ptr(ld), n, *shape, Ng, ALL, max_run, rc.data_ptr(), cl.data_ptr(), s))
        res["runs"] = entry(event_ms(rcall, runs), N * (5 if ld is not None else 1), Ng=Ng, max_run=max_run, clamped=int(cl.sum().item()))
        del rc, lvb
        kw = dict(mask=mask) if mask is not None else dict(labels=ld, n=n, shape=shape)
        res["texture_stats_ms"] = wall_ms(lambda: T.texture_stats(vol, lo=LO, width=SPAN / Ng, levels=Ng, **kw), max(runs // 3, 2))
        note(f"kernels and texture_stats: {name} done")
        if not host:
            continue
        import texture_oracle as TO
        fdata = ct.astype(np.float64)
        g = TO.group_of(shape, mask=mask, n=1) if mask is not None else TO.group_of(shape, labels=ld.cpu().numpy().reshape(shape, order="F"), n=n)
        t0 = time.perf_counter()
        hlev, hlc = TO.quantize(fdata, g, n, LO, SPAN / Ng, Ng, False); t1 = time.perf_counter()
        note(f"restatement: quantize {t1 - t0:.1f} s")
        hC = TO.glcm(hlev, g, n, Ng, 1, ALL); t2 = time.perf_counter()
        note(f"restatement: glcm {t2 - t1:.1f} s")
        hR, hcl = TO.runs(hlev, g, n, Ng, ALL, max_run); t3 = time.perf_counter()
        ts = T.texture_stats(vol, lo=LO, width=SPAN / Ng, levels=Ng, max_run=max_run, **kw)
        assert np.array_equal(hlc, ts.level_counts) and np.array_equal(hC, ts.glcm), "the restatement and the device disagree"
        if ts.runs.shape[-1] == max_run:
            assert np.array_equal(hR, ts.runs), "the restatement and the device disagree on the runs"
        res["host_path"] = {"quantize_s": t1 - t0, "glcm_s": t2 - t1, "runs_s": t3 - t2, "total_s": t3 - t0, "threads": os.environ.get("OMP_NUM_THREADS"),
                            "note": "tests/texture_oracle.py, Ng = 16, 13 directions unmerged, distance 1; the features are not part of the figure"}
        dev_ms = res["quantize"]["ms"] + res["glcm"]["Ng=16 unmerged d=1"]["ms"] + res["runs"]["ms"]
        res["host_over_device_kernels"] = (t3 - t0) * 1e3 / dev_ms
        res["host_over_texture_stats"] = (t3 - t0) * 1e3 / res["texture_stats_ms"]
        del fdata, g, hlev
    return out


def ab(lib_path, shape_flag, runs, rounds):
    """the product library and the measurement build alternate, each in a fresh child process; -> {"staged": [...], "loads": [...]} of the children's results"""
    got = {"staged": [], "loads": []}
    for _ in range(rounds):
        for key, path in (("staged", None), ("loads", lib_path)):
            env = dict(os.environ)
            env.pop("COVIDSEG_AMD_LIB", None)
            if path:
                env["COVIDSEG_AMD_LIB"] = os.path.abspath(path)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--glcm-child", "--runs", str(runs)] + shape_flag, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"the {key} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            got[key].append(json.loads(r.stdout.strip().splitlines()[-1]))
            note(f"A/B child {key} done")
    summary = {}
    for case in got["staged"][0]:
        summary[case] = {}
        for cfg in got["staged"][0][case]["glcm"]:
            a = [r[case]["glcm"][cfg]["ms"] for r in got["staged"]]
            b = [r[case]["glcm"][cfg]["ms"] for r in got["loads"]]
            assert len({r[case]["glcm"][cfg]["pairs"] for r in got["staged"] + got["loads"]}) == 1, "the two builds count different pairs"
            summary[case][cfg] = {"staged_ms": a, "loads_ms": b, "staged_median": statistics.median(a), "loads_median": statistics.median(b),
                                  "loads_over_staged": statistics.median(b) / statistics.median(a), "path": got["staged"][0][case]["glcm"][cfg]["path"]}
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--ab", default=None, help="the measurement build of make texture_loads")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--glcm-child", action="store_true", help="internal: the GLCM launches only, one JSON line on stdout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_texture.json"))
    a = ap.parse_args()
    shape = (128, 128, 64) if a.small else (512, 512, 301)
    if a.glcm_child:
        print(json.dumps(bench_glcm(shape, a.runs)))
        return
    res = {"shape": list(shape), "runs": a.runs, "binning": {"lo": LO, "width": "900 / Ng"}}
    if a.ab:
        res["glcm_staged_vs_loads"] = ab(a.ab, ["--small"] if a.small else [], a.runs, a.ab_rounds)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    res["library"] = os.environ.get("COVIDSEG_AMD_LIB") or "product"
    res["cases"] = bench(shape, a.runs, not a.no_host)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

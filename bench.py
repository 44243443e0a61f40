#!/usr/bin/env python
"""bench.py -- CT images/sec of one full U-Net training step (fwd + loss + bwd + Keras-Adam,
gradient all-reduce when >1 GPU) at 512x512x1, batch 16 per GPU, fp32, synthetic data resident
in HBM (BASELINE.json configs[1]).  One process per GPU: under torch.distributed.run the ranks read RANK / LOCAL_RANK /
WORLD_SIZE; a bare `python bench.py --gpus N` (N > 1) re-launches itself under torch.distributed.run on 127.0.0.1.
`--config 2` = BASELINE.json configs[2] (task-3 lung U-Net, same graph, batch 8 per GPU = global 64 on 8 GPUs).

Prints ONE JSON line (rank 0).  A plain run does only what the headline needs: it sets up, settles the clocks, warms up, times --steps steps,
writes what the last timed step computed if --dump-outputs DIR is given, and prints metric / value / unit / ms_per_step / dtype / config.
With --full the line also carries
  roofline     : the dominant kernel family (conv3x3 forward + data-gradient launches: fp32 tensors, products on the fp16 matrix
                 pipe as a block-scaled two-term split): matrix FLOPs its launches EXECUTE in a step / their summed
                 hipEvent durations vs that pipe's dense peak; algorithmic bytes / FLOPs beside it
  fp32_strict_img_s : the same step with every product on v_mfma_f32_32x32x2_f32 (--algo 2: exact fp32 multiply-add, the
                 out-of-domain fallback family) -- what the fp16 split buys, and what the IEEE-fp32 path costs
  fit_img_s / fit_epoch_img_s : the REAL model.fit path (T1:1059-1061): UNetModel.fit on a host-resident float64 set, whole call incl. the one-time upload / a steady epoch
  predict_batch1_ms : median latency of model.predict at batch 1 (T1:1137), synchronised per call
  cpu_baseline : the CPU oracle (torch-CPU restatement, kind "port") timed on the host cores on a
                 bounded sample of the same workload (rank 0, N=1 only)
  sclk_mhz / power_w : the operating point of the timed region (amdsmi side thread)
  comm         : N > 1 (data-parallel engines): where the gradient exchange's time goes, from extra steps behind the timed region
Before the W warm-up steps the chip is run for SETTLE_S seconds of untimed steps: its clocks need >= 1 s of load to settle at the
power-capped operating point (a 20-step run started cold reads ~5 % low or high depending on where in the ramp it lands).  After it the
model is reset to its initial weights, a fresh optimizer and the start of its dropout stream, so the same arguments give the timed steps
the same inputs and starting state from run to run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, no TF32 on gfx950
HBM_PEAK_GBS = 8000.0              # MI355X_MICROARCH.md: HBM3E ~8 TB/s
BF16_MFMA_PEAK_TFLOPS = 2500.0    # dense v_mfma_f32_32x32x16_bf16
HBM_PEAK_GBS = 8000.0


class _SmiSampler:
    """Shader clock and socket power of THIS rank's GPU sampled from a side thread (amdsmi, ~0.4 ms per read) while a region runs: the pool's boxes differ by ~7 % in what
    the same library measures, and the chip runs against its power cap -- the bench line says which kind of box / operating point it was.  Best effort: any
    failure leaves the fields null."""
    def __init__(self, index=0, period_s=0.01):
        self.clk, self.pw, self._stop, self._thr, self.ok = [], [], False, None, False
        self.period = period_s
        try:
            import amdsmi
            self._smi = amdsmi
            amdsmi.amdsmi_init()
            hs = amdsmi.amdsmi_get_processor_handles()
            self._h = hs[index if index < len(hs) else 0]
            self.ok = True
        except Exception:
            self.ok = False

    def _run(self):
        while not self._stop:
            try:
                m = self._smi.amdsmi_get_gpu_metrics_info(self._h)
                cl = [c for c in m.get("current_gfxclks", []) if isinstance(c, (int, float)) and 0 < c < 10000]
                if cl:
                    self.clk.append(sum(cl) / len(cl))
                pw = m.get("current_socket_power")
                if isinstance(pw, (int, float)) and pw > 0:
                    self.pw.append(float(pw))
            except Exception:
                pass
            time.sleep(self.period)

    def start(self):
        if self.ok:
            import threading
            self._stop = False
            self._thr = threading.Thread(target=self._run, daemon=True); self._thr.start()
        return self

    def stop(self):
        if self._thr is not None:
            self._stop = True; self._thr.join(); self._thr = None
        import statistics as st
        return {"sclk_mhz": round(st.median(self.clk), 1) if self.clk else None, "power_w": round(st.median(self.pw), 1) if self.pw else None, "samples": len(self.clk)}


def _physical_cores():
    """Physical cores this process may run on: distinct (package, core) pairs of the cpus in the affinity mask (hyper-thread siblings counted once)."""
    cpus = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    seen = set()
    for c in cpus:
        try:
            base = f"/sys/devices/system/cpu/cpu{c}/topology/"
            seen.add((open(base + "physical_package_id").read().strip(), open(base + "core_id").read().strip()))
        except OSError:
            seen.add(("?", str(c)))
    return max(1, len(seen))


def _cpu_quota():
    """cpus the container's cgroup allows (cpu.max / cfs quota), or None"""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except (OSError, ValueError):
        return None


def cpu_baseline(size, seconds_budget=28.0, arch="unet"):
    """Time the oracle's identical training step (fwd + loss + bwd + Keras-Adam, oneDNN convolutions on channels_last memory: the oracle's NHWC tensors viewed as
    NCHW ARE torch's channels_last format) on the host cores: a bounded sample of the same workload -- batch 8 of the 16 where it fits the budget, one thread per
    PHYSICAL core (the default thread count of a 256-cpu host put two threads on every core of one socket's worth and ran at a third of this), the better of the
    full core count and half of it (one socket / less memory contention)."""
    import torch
    from covidseg_amd.data import synthetic_ct
    from oracle import unet_oracle as O
    phys = _physical_cores()
    default_threads = torch.get_num_threads()
    # algorithmic FLOPs per image of one training step (2 x MAC, convs + ConvTs; SURVEY 8d: 288.65 GFLOP at 512 x 512 for the U-Net), scaled by the pixel count
    gflop_img = {"unet": 288.652, "unetpp": None, "classifier": None}[arch]
    gflop_img = gflop_img * (size / 512.0) ** 2 if gflop_img else None

    def make(bs):
        if arch == "classifier":
            from covidseg_amd.data import synthetic_classification
            x, y = synthetic_classification(bs, size, seed=0)
            return x, y, O.ClsOracleTrainer(O.cls_init_weights(0, 1, (size, size)), torch.float32)
        x, y = synthetic_ct(bs, size, seed=0)
        return x, y, O.OracleTrainer(O.init_weights(seed=0) if arch == "unet" else O.pp_init_weights(seed=0), torch.float32, arch)

    t_all = time.perf_counter()
    best = None
    quota = _cpu_quota()
    cap = max(1, min(phys, int(quota) if quota else phys))
    tried = []
    try:
        bs = 16 if arch == "classifier" else 2
        # thread counts, the likeliest first: a box whose cores outnumber what the memory system feeds (or what the container's cpu quota allows) runs this step FASTER on a
        # fraction of them (measured on the GPU box's 128-core host: 128 threads 96 GFLOP/s, below what 8 cores of the build container give) -- so sweep, one warm-up + one
        # timed small-batch step per setting, while the budget lasts; then one larger batch at the winner
        sweep = [t for t in dict.fromkeys([min(cap, 32), min(cap, 16), min(cap, 64), cap]) if t >= 1]
        x, y, tr = make(bs)
        for threads in sweep:
            left = seconds_budget - (time.perf_counter() - t_all)
            if best is not None and left < 3.0 * bs / best[0] + 6.0:          # (keep room for the larger batch)
                break
            torch.set_num_threads(threads)
            tr.train_step(x, y)                                  # warm-up at this thread count (oneDNN primitive creation, weight reorders, thread pool)
            t0 = time.perf_counter(); tr.train_step(x, y); dt = time.perf_counter() - t0
            tried.append(f"{threads}: {bs / dt:.2f}")
            if best is None or bs / dt > best[0]:
                best = (bs / dt, threads, bs, 1)
        if arch == "unet":
            left = seconds_budget - (time.perf_counter() - t_all)
            b = min(8, int(left * best[0] / 2.2) // 2 * 2)      # a warm-up step + a timed one of this batch must fit what is left of the budget
            if b > bs:
                torch.set_num_threads(best[1])
                x, y, tr = make(b)
                tr.train_step(x, y)
                t0 = time.perf_counter(); tr.train_step(x, y); dt = time.perf_counter() - t0
                tried.append(f"{best[1]} @ batch {b}: {b / dt:.2f}")
                if b / dt > best[0]:
                    best = (b / dt, best[1], b, 1)
    finally:
        torch.set_num_threads(default_threads)
    v, threads, bs, reps = best
    rate = f", {v * gflop_img:.0f} GFLOP/s algorithmic" if gflop_img else ""
    return {"value": round(v, 4), "unit": "images/sec", "cores": int(threads), "kind": "port",
            "sample": f"{reps} training step of batch {bs} at {size}x{size}x1 fp32 after a warm-up step (torch-CPU oracle: oneDNN convolutions, channels_last memory, "
                      f"{threads} threads -- the best of a sweep [threads: img/s] {'; '.join(tried)}; {phys} physical cores / {os.cpu_count()} cpus visible, "
                      f"cpu quota {quota if quota else 'none'}, torch's default was {default_threads} threads){rate}"}


def live_traffic(timeout_s=90):
    """HBM bytes of THIS build's step from the PMC counters, measured now: two counter-only rocprofv3 passes (FETCH_SIZE, WRITE_SIZE -- separate runs, no tracing, as
    MI355X_MICROARCH.md prescribes) over two training steps of tools/profile_ops.py in a child process; FETCH_SIZE (KB) x 2 (gfx950 tallies 128-B requests at 64 B) +
    WRITE_SIZE (KB), per launch of the conv3x3 forward / data-gradient family and summed over every kernel of a step.  None if rocprofv3 is not there or anything fails
    (the line then quotes the offline figure of profiles/)."""
    import collections, csv, glob, shutil, subprocess, tempfile
    if shutil.which("rocprofv3") is None:
        return None
    tmp = tempfile.mkdtemp(prefix="unet_pmc_", dir="/tmp")
    try:
        tot = {}
        for c in ("FETCH_SIZE", "WRITE_SIZE"):
            subprocess.run(["rocprofv3", "--pmc", c, "--output-format", "csv", "-d", os.path.join(tmp, c), "--", sys.executable, os.path.join(ROOT, "tools", "profile_ops.py"),
                            "--reps", "1", "--warm", "1"], cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=timeout_s, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            agg = collections.defaultdict(lambda: [0.0, 0])
            for f in glob.glob(os.path.join(tmp, c, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r["Counter_Name"] == c:
                        a = agg[r["Kernel_Name"]]; a[0] += float(r["Counter_Value"]); a[1] += 1
            tot[c] = agg
        steps = sum(n for k, (v, n) in tot["FETCH_SIZE"].items() if "adam_kernel" in k)
        dom = [k for k in tot["FETCH_SIZE"] if "conv_h2_kernel<0" in k or "conv_pp_kernel<" in k]          # (conv3x3 forward / data gradient: both schedules)
        launches = sum(tot["FETCH_SIZE"][k][1] for k in dom)
        if steps < 1 or launches < 1:
            return None
        rd = sum(tot["FETCH_SIZE"][k][0] for k in dom) * 2048.0; wr = sum(tot["WRITE_SIZE"][k][0] for k in dom if k in tot["WRITE_SIZE"]) * 1024.0
        all_b = sum(v for v, n in tot["FETCH_SIZE"].values()) * 2048.0 + sum(v for v, n in tot["WRITE_SIZE"].values()) * 1024.0
        return {"per_launch": (rd + wr) / launches, "launches_per_step": launches / steps, "per_step_all_kernels": all_b / steps, "steps": steps}
    except Exception:
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _tap_dims(eng, n, name):
    import ctypes as C
    from covidseg_amd import _lib
    plan = eng._plan(n)
    ptr, ld, nn, hh, ww, cc = _lib.vp(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    eng.ctx.check(eng.lib.unet_model_tap(plan["m"], name.encode(), 0, C.byref(ptr), C.byref(ld), C.byref(nn), C.byref(hh), C.byref(ww), C.byref(cc)), "tap")
    return ptr.value, ld.value, nn.value, hh.value, ww.value, cc.value


DUMP_BUDGET_BYTES = 60_000_000           # (under the 64 MB the dump may hold, .npy headers included)


def dump_outputs(out_dir, arrays, budget=DUMP_BUDGET_BYTES):
    """Write every array as out_dir/<name>.npy in float32 ('/' in a name becomes '.').  Where the whole would exceed `budget` bytes, every array
    is cut to the same fraction of its elements: a fixed, seeded (np.random.default_rng(0)), sorted sample of its flattened values."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.asarray(v, np.float32) for k, v in arrays.items()}
    frac = min(1.0, budget / max(1, sum(a.nbytes for a in arrays.values())))
    rng = np.random.default_rng(0)
    for name, a in arrays.items():
        if frac < 1.0:
            flat = a.reshape(-1)
            a = flat[np.sort(rng.choice(flat.size, max(1, int(flat.size * frac)), replace=False))]
        np.save(os.path.join(out_dir, name.replace("/", ".") + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--comm-selftest", action="store_true", help="N > 1 first contact: build the data-parallel engine (process group, IPC mapping of the device-side small all-reduce and its "
                    "self-test), run 1000 small all-reduces through either path and ten of the whole gradient buffer, print ONE JSON line with the per-call times of every rank, exit")
    ap.add_argument("--steps", type=int, default=40)     # the chip needs ~1 s of load to settle its clocks
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--full", action="store_true", help="besides the headline: the CPU baseline, the per-op roofline leg (+ live PMC traffic), the strict-fp32 leg, "
                    "predict latency, the model.fit leg, the timed region's clock / power and, for data-parallel engines, the `comm` leg (the --no-* switches "
                    "below turn single legs off).  Off by default: a plain run only sets up, warms up and times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32): "
                    "loss_dice ([loss, dice_coeff] as train_batch returns it) and every weight / BatchNorm moving statistic after its optimizer update")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (weak scaling); default 16 (configs[1]) or 8 (--config 2)")
    ap.add_argument("--config", type=int, default=1, choices=[1, 2], help="BASELINE.json configs index: 1 = infection U-Net 512x512x1 bs16 per GPU (headline); "
                    "2 = lung U-Net (task 3, same graph T3:850-913) 512x512x1 at batch 8 per GPU = global 64 on 8 GPUs")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--algo", type=int, default=0, help="0 auto (fp16-split h2 kernels where the shape allows), 1 direct VALU kernels, 2 strict fp32 MFMA kernels")
    ap.add_argument("--no-strict-leg", action="store_true", help="skip the untimed fp32_strict_img_s measurement (--algo 2 engine, 8 steps)")
    ap.add_argument("--fold16", action="store_true", help="UNET_OPT_BN_FOLD = 3: the classifier's 16-channel first block folded too (+15 %% there; more ReLU flips at full size, include/unet_hip.h)")
    ap.add_argument("--deterministic", action="store_true", help="UNET_OPT_DETERMINISTIC: fixed-order reductions, no floating-point atomics (bit-identical reruns)")
    ap.add_argument("--options", default="", help='context options as JSON, e.g. {"head_fused": 0} (same-box A/B of graph forms; _lib.OPTIONS)')
    ap.add_argument("--settle", type=float, default=2.0, help="seconds of untimed steps ahead of the warm-up (clock settle)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-traffic-leg", action="store_true", help="skip the live PMC measurement of roofline.traffic / step_traffic (two counter-only rocprofv3 passes in a child process, ~20 s; "
                                                                  "the line then quotes the offline figure of profiles/)")
    ap.add_argument("--no-fit-leg", action="store_true", help="skip the untimed fit_img_s measurement (UNetModel.fit on a host-resident set)")
    ap.add_argument("--fit-steps", type=int, default=20, help="steps per epoch of the fit leg")
    ap.add_argument("--no-sync-bn", action="store_true")
    ap.add_argument("--no-buckets", action="store_true", help="N > 1 A/B: ONE all-reduce of the whole gradient buffer behind backward (fully exposed) instead of the 5 overlapped buckets")
    ap.add_argument("--small-allreduce", default="device", choices=["device", "rccl"], help="N > 1: BatchNorm / loss sums through the device-side all-reduce (csrc/comm.hip) or through RCCL")
    ap.add_argument("--arch", default="unet", choices=["unet", "unetpp", "classifier"], help="unetpp = the U-Net++ graph (BASELINE "
                    "configs[3], at fp32; --size 256 --batch 32); classifier = the task-2 CNN (configs[4] at the reference's 1-channel fp32; "
                    "--size 224 --batch 256).  Neither is the headline metric")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"], help="bf16 = activations / activation gradients stored as bf16 (U-Net graph only); "
                    "NOT the headline metric, which BASELINE.json fixes at fp32")
    args = ap.parse_args()
    if args.steps < 1 and not args.comm_selftest:
        ap.error("--steps must be >= 1")
    if args.batch is None:
        args.batch = 8 if args.config == 2 else 16

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # bare `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run, rendezvous on 127.0.0.1
        # (--standalone: torchrun picks and owns the rendezvous port itself -- no bind-close-reuse race)
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)

    import numpy as np
    import torch
    import torch.distributed as dist
    from covidseg_amd.data import synthetic_ct
    from covidseg_amd.engine import HipUNet
    from covidseg_amd import weights as W

    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    # test hooks (single-GPU dry run of the multi-process path): UNET_BENCH_BACKEND=gloo UNET_BENCH_ONE_DEVICE=1
    backend = os.environ.get("UNET_BENCH_BACKEND", "nccl")
    if os.environ.get("UNET_BENCH_ONE_DEVICE"):
        local = 0
    torch.cuda.set_device(local)
    pg = None
    if world > 1 or os.environ.get("UNET_BENCH_FORCE_PG"):          # UNET_BENCH_FORCE_PG=1: run the process-group code at world 1 (RCCL path smoke on a 1-GPU box)
        kw = {}
        if "MASTER_PORT" not in os.environ:                       # world 1 without a launcher (UNET_BENCH_FORCE_PG): a private file store, no port at all
            import tempfile
            kw["init_method"] = "file://" + os.path.join(tempfile.mkdtemp(prefix="unet_bench_pg_"), "store")
        else:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local), **kw)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world, **kw)
        pg = dist.group.WORLD

    B, S = args.batch, args.size
    # synthetic batch: generate a few distinct slices on the host, tile to the batch, keep resident in HBM
    if args.arch == "classifier":
        from covidseg_amd.data import synthetic_classification
        xs, ys = synthetic_classification(min(B, 8), S, seed=rank)
        ys = ys.astype(np.float32)
    else:
        xs, ys = synthetic_ct(min(B, 4), S, seed=rank)
    reps = (B + len(xs) - 1) // len(xs)
    x = torch.from_numpy(np.concatenate([xs] * reps)[:B]).cuda(); y = torch.from_numpy(np.concatenate([ys] * reps)[:B]).cuda()
    eng = HipUNet(S, S, 1, device=local, conv_algo=args.algo, process_group=pg, sync_bn=not args.no_sync_bn, dropout_rate=0.25, seed=rank,
                  arch=args.arch, dtype=args.dtype, force_dp=bool(os.environ.get("UNET_BENCH_FORCE_PG")), small_allreduce=args.small_allreduce, grad_buckets=not args.no_buckets, options=({"deterministic": 1} if args.deterministic else {}) | ({"bn_fold": 3} if args.fold16 else {}) | (json.loads(args.options) if args.options else {}) or None)
    w0 = W.init_weights(0, 1, args.arch, (S, S))
    eng.set_weights(w0)                                              # identical replicas
    if args.comm_selftest:
        # a diagnosis that needs no training step: if the first minute on an 8-GPU node fails, this line still says which exchange path works and how fast it is
        mine = eng.comm_selftest()
        every = [mine]
        if world > 1:
            every = [None] * world
            dist.all_gather_object(every, mine)
        if rank == 0:
            keys = [k for k in ("device_us_per_call", "torch_distributed_us_per_call", "gradient_allreduce_ms") if k in mine]
            print(json.dumps({"comm_selftest": {"world": world, "backend": backend, "rank0": mine, "max_over_ranks": {k: max(e[k] for e in every) for k in keys},
                                                "all_exact": all(e.get("device_exact", True) and e.get("torch_distributed_exact", True) for e in every),
                                                "statuses": [e.get("device_status", 0) for e in every]}}), flush=True)
        if pg is not None:
            dist.barrier(); dist.destroy_process_group()
        return

    def settle(seconds):
        ts = time.perf_counter()
        while time.perf_counter() - ts < seconds:
            for _ in range(5):
                eng.train_batch(x, y)
            torch.cuda.synchronize()

    # ---- untimed setup 1 (--full; rank 0, N=1): the CPU baseline first, so the GPU work of this command is one contiguous block at its end
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(S, arch=args.arch)

    # ---- untimed setup 2 (--full), the roofline leg: per-op hipEvent timing (profiling mode serialises the ops and brackets each with events on the
    # launch stream) of PROF_STEPS steps; every rank runs them (they contain the collectives), rank 0 reports.  Running it BEFORE the
    # warm-up also means the chip has seen ~0.5 s of load when the W warm-up steps start (its clocks need ~1 s to settle)
    PROF_STEPS = 8
    roof = ops = smi_prof = None
    for _ in range(2):
        eng.train_batch(x, y)                # first-touch: plans, workspace, weight images
    if args.full:
        settle(args.settle)                  # (a cold chip runs these launches ~40 % slower than the timed region does: the per-op times would not be the step's)
        smi_prof = _SmiSampler(0).start() if rank == 0 else None          # (the per-op leg serialises the ops: its own operating point)
        eng.set_profiling(True, B)
        for _ in range(PROF_STEPS):
            eng.train_batch(x, y)
        torch.cuda.synchronize()
        eng.set_profiling(False)
        smi_prof = smi_prof.stop() if smi_prof is not None else None
        ops = eng.op_profile(B, 0) + eng.op_profile(B, 1)
        eng.set_weights(w0); eng.reset_optimizer()

    # ---- untimed setup 3 (--full; rank 0, N=1, the headline configuration only): the same step on the strict-fp32 kernel family (exact fp32 MFMA products)
    strict = None
    if args.full and rank == 0 and world == 1 and not args.no_strict_leg and args.dtype == "fp32" and args.algo == 0:
        e2 = HipUNet(S, S, 1, device=local, conv_algo=2, dropout_rate=0.25, seed=rank, arch=args.arch, dtype=args.dtype)
        e2.set_weights(W.init_weights(0, 1, args.arch, (S, S)))
        for _ in range(4):
            e2.train_batch(x, y)
        torch.cuda.synchronize(); ts = time.perf_counter()
        for _ in range(8):
            e2.train_batch(x, y)
        torch.cuda.synchronize()
        strict = round(8 * B / (time.perf_counter() - ts), 1)
        del e2
        torch.cuda.empty_cache()

    # ---- untimed setup 4 (--full; rank 0, N=1): latency of model.predict(x.reshape(1,H,W,1)) (T1:1137) -- inference forward at batch 1, synchronised per call
    predict_ms = predict_cold_ms = None
    if args.full and rank == 0 and world == 1 and args.arch == "unet":
        x1 = x[:1].contiguous()
        for _ in range(3):
            eng.predict_batch(x1)
        torch.cuda.synchronize(); lat = []
        for _ in range(20):
            ts = time.perf_counter(); eng.predict_batch(x1); torch.cuda.synchronize(); lat.append((time.perf_counter() - ts) * 1e3)
        predict_ms = round(sorted(lat)[len(lat) // 2], 3)
        lat = []                                   # ... and with the per-weight preparation (weight images, inference BatchNorm tables) redone every call: the first predict after a weight change
        for _ in range(10):
            eng._infer_ready = None
            ts = time.perf_counter(); eng.predict_batch(x1); torch.cuda.synchronize(); lat.append((time.perf_counter() - ts) * 1e3)
        predict_cold_ms = round(sorted(lat)[len(lat) // 2], 3)

    # ---- untimed setup 5 (--full; rank 0, N=1, U-Net): the REAL model.fit path (T1:1059-1061) -- a host-resident float64 set, as the reference's runner holds it,
    # through keras_like.UNetModel.fit: upload once (pinned staging), per step a device-side gather of the shuffled batch, per epoch one host sync
    fit_stats = None
    if args.full and rank == 0 and world == 1 and args.arch == "unet" and not args.no_fit_leg:
        from covidseg_amd.keras_like import UNetModel
        nfit = args.fit_steps * B
        xh = np.concatenate([xs] * ((nfit + len(xs) - 1) // len(xs)))[:nfit].astype(np.float64)
        yh = np.concatenate([ys] * ((nfit + len(ys) - 1) // len(ys)))[:nfit].astype(np.float64)
        model = UNetModel(S, 1, backend=eng); model.verbose = 0
        model.compile(lr=5e-4)
        torch.cuda.synchronize(); ts = time.perf_counter()
        hist = model.fit(xh, yh, batch_size=B, epochs=3, shuffle=True)
        torch.cuda.synchronize(); wall = time.perf_counter() - ts
        ep = sorted(hist.epoch_seconds[1:])[len(hist.epoch_seconds[1:]) // 2]
        fit_stats = {"fit_img_s": round(3 * nfit / wall, 1), "fit_epoch_img_s": round(nfit / ep, 1),
                     "fit_note": f"UNetModel.fit(x, y, batch_size={B}, epochs=3) on {nfit} host float64 slices ({args.fit_steps} steps per epoch, shuffled): fit_img_s = the whole call "
                                 f"incl. the one-time upload; fit_epoch_img_s = a steady epoch (median of epochs 2-3) -- to be read against `value`"}
        del xh, yh, model

    # ---- untimed: clock settle.  The chip needs >= 1 s of this load before its clocks sit at the power-capped operating point
    settle(args.settle)
    # ... then the state the warm-up and timed steps start from is fixed whatever ran before (the settle loop runs for a time, not a number of steps):
    # initial weights and BatchNorm statistics, a fresh optimizer, the dropout stream from its first key
    torch.cuda.synchronize()
    eng.set_weights(w0); eng.reset_optimizer(); eng._drop_calls = 0

    # ---- the measurement the contract defines: W untimed warm-up steps, then EXACTLY K timed steps between barrier + synchronize
    for _ in range(args.warmup):
        eng.train_batch(x, y)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    smi = _SmiSampler(int(os.environ.get("LOCAL_RANK", "0")) if not os.environ.get("UNET_BENCH_ONE_DEVICE") else 0).start() if args.full and rank == 0 else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = eng.train_batch(x, y)
    torch.cuda.synchronize()
    dt_local = time.perf_counter() - t0
    smi_timed = smi.stop() if smi is not None else None          # this rank's own K steps (before it waits for the others)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rank_ms = [dt_local / args.steps * 1e3]
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX); dt = float(t.item())
        rank_ms = [None] * world
        dist.all_gather_object(rank_ms, dt_local / args.steps * 1e3)
    loss_dice = last.cpu().numpy().tolist()
    comm_status = eng.comm_status()
    if comm_status != 0:                       # a device-side all-reduce that timed out: the step's numbers are not a step's
        raise RuntimeError(f"rank {rank}: device-side all-reduce missed rank {comm_status - 1}")
    # what the last timed step handed its caller: [loss, dice] and the model after its optimizer update (replicas are identical: rank 0 writes)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss_dice": last.cpu().numpy(), **eng.get_weights()})

    # ---- untimed, behind the measurement (--full; every rank; data-parallel engines only): where the gradient exchange's time goes -- BASELINE.md config 3 asks for
    # "all-reduce time exposed vs hidden".  COMM_STEPS more steps with event pairs around every gradient all-reduce (on its side stream) and around the compute stream's
    # wait in front of Adam; per-rank figures are gathered, rank 0 reports its own and the max over ranks.
    comm = None
    if args.full and eng._dp:
        COMM_STEPS = 8
        eng.set_comm_profiling(True)
        for _ in range(COMM_STEPS):
            eng.train_batch(x, y)
        mine = eng.comm_profile()
        eng.set_comm_profiling(False)
        mine["comm_status"] = eng.comm_status()
        every = [mine]
        if world > 1:
            every = [None] * world
            dist.all_gather_object(every, mine)
        comm = {"world": world, "backend": backend + (" (RCCL)" if backend == "nccl" else ""), "sync_bn": not args.no_sync_bn, "grad_buckets": not args.no_buckets,
                "small_allreduce_requested": args.small_allreduce,
                "small_allreduce_in_use": ("device (comm.hip)" if eng._comm is not None else "torch.distributed") if not args.no_sync_bn else None,
                "small_allreduce_fallback": eng._comm_fallback,          # None, or why the device-side path was asked for and is NOT in use (every rank falls back together)
                "comm_status": max(e["comm_status"] for e in every),
                "profiled_steps": mine["steps"], "small_reductions_per_step": mine["small_reductions_per_step"],
                "buckets_rank0": mine["buckets"],          # launch order = the order backward finishes them; mb = MB of gradients, ms = all-reduce duration on the side stream
                "buckets_ms_max_over_ranks": [round(max(e["buckets"][i]["ms"] for e in every), 4) for i in range(len(mine["buckets"]))],
                "allreduce_ms_per_step": {"rank0": mine["allreduce_ms"], "max": max(e["allreduce_ms"] for e in every)},
                "exposed_ms_per_step": {"rank0": mine["exposed_ms"], "max": max(e["exposed_ms"] for e in every)},          # the compute stream standing in front of Adam (engine._run finish_buckets)
                "hidden_ms_per_step": {"rank0": mine["hidden_ms"], "min": min(e["hidden_ms"] for e in every)},
                "rank_ms_per_step": {"min": round(min(rank_ms), 3), "max": round(max(rank_ms), 3), "all": [round(v, 3) for v in rank_ms]},
                "note": "allreduce = summed duration of a step's gradient all-reduces on their stream; exposed = what the compute stream waited for them in front of the "
                        "optimizer; hidden = allreduce - exposed (overlapped with backward).  A/B switches: --no-buckets (one exposed all-reduce), --no-sync-bn (no small "
                        "reductions), --small-allreduce rccl"}

    if args.full and rank == 0:
        # (conv3x3_dgrad_bn_bwd: the data gradient of a decoder block's first conv with the folded BatchNorm's backward in its epilogue -- the same
        #  kernel, same FLOPs; the op's time includes its 5 us coefficient launch)
        # (conv3x3_fwd_head: the last conv3x3 with the 1x1 sigmoid head and the loss sums in its epilogue -- the same kernel body and conv FLOPs)
        # (conv3x3_dgrad_pool_sums: a data gradient with the encoder tail's pooled sums in its epilogue -- likewise)
        dom = [o for o in ops if o[0].startswith(("conv3x3_fwd:", "conv3x3_fwd_head:", "conv3x3_dgrad:", "conv3x3_dgrad_bn_bwd:", "conv3x3_dgrad_pool_sums:"))]
        dom = [o for o in dom if not o[0].endswith(":c1a")]                  # c1a (Cin=1) runs the direct HBM-bound kernel
        fl = sum(o[1] for o in dom); ms = sum(o[3] / max(o[4], 1) for o in dom); launches = len(dom)
        shapes = W.weight_shapes(1, args.arch, (S, S))

        def exec_ratio(opname):
            """fp32-MFMA-time equivalent of a conv3x3 op's matrix work: 3 * 157.3 / 2500 on the fp16-split h2 kernels, 1 on the strict fp32 family (unet_conv3x3_exec_ratio)"""
            kind, _, lname = opname.partition(":")
            if not kind.startswith("conv3x3") or args.dtype == "bf16" or lname + "/kernel" not in shapes:
                return 1.0
            _, _, ci, co = shapes[lname + "/kernel"]
            if kind.startswith("conv3x3_dgrad"):
                ci, co = co, ci
            _, _, _, hh, ww, _ = _tap_dims(eng, B, lname)
            if kind.startswith("conv3x3_wgrad"):
                return float(eng.lib.unet_conv3x3_wgrad_exec_ratio(args.algo, hh, ww, ci, co))
            return float(eng.lib.unet_conv3x3_exec_ratio(args.algo, hh, ww, ci, co))

        groups = {}
        for name, flops, by, tms, calls in ops:
            k = name.split(":")[0]
            g = groups.setdefault(k, [0.0, 0.0, 0.0]); g[0] += tms / max(calls, 1); g[1] += flops; g[2] += by
        effective = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0               # algorithmic (direct-convolution) FLOPs / time
        # whole-step floor on the EXECUTED work: every op at max(its algorithmic bytes / HBM peak, its executed matrix FLOPs at the pipe it runs on)
        peak_fl = (BF16_MFMA_PEAK_TFLOPS if args.dtype == "bf16" else FP32_MFMA_PEAK_TFLOPS) * 1e12
        floor_ms = sum(max(o[2] / (HBM_PEAK_GBS * 1e9), o[1] * exec_ratio(o[0]) / peak_fl) for o in ops) * 1e3
        # HBM bytes per launch of the same kernel from rocprofv3 PMC passes (FETCH_SIZE x2, WRITE_SIZE): collected OFFLINE at this exact workload
        # (tools/collect_r03_profiles.sh, calibration inside the file), not in this run -- only quoted for the configuration it was measured on
        traffic, tname = None, None
        for tname in (("r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json") if args.dtype == "fp32" else ("r03_pmc_traffic_bf16.json", "r01_pmc_traffic_bf16.json")):
            tfile = os.path.join(ROOT, "profiles", tname)
            if os.path.exists(tfile) and B == 16 and S == 512 and args.algo == 0 and args.arch == "unet":
                traffic = round(json.load(open(tfile))["hbm_bytes_per_launch"])
                break
        step_traffic = None
        tf4 = os.path.join(ROOT, "profiles", "r05_pmc_traffic.json")
        if os.path.exists(tf4) and B == 16 and S == 512 and args.algo == 0 and args.arch == "unet" and args.dtype == "fp32":
            t4 = json.load(open(tf4))
            if "hbm_bytes_per_step_all_kernels" in t4:
                sb = float(t4["hbm_bytes_per_step_all_kernels"])
                step_traffic = {"hbm_bytes_per_step_all_kernels": round(sb), "vs_survey_54.3GB": round(sb / 54.300299148e9, 3),
                                "vs_op_model": round(sb / max(sum(o[2] for o in ops), 1.0), 3),
                                "source": "profiles/r05_pmc_traffic.json (FETCH_SIZE x 2 + WRITE_SIZE summed over every kernel of one step, counter-only rocprofv3 passes; offline, this workload)"}
        traffic_unit = f"HBM bytes per launch, rocprofv3 PMC collected offline on this workload (profiles/{tname}); not measured in this run"
        # ... and measured NOW where the default workload runs on one GPU (the timed region is over: nothing here touches `value`)
        live = None
        if world == 1 and not args.no_traffic_leg and B == 16 and S == 512 and args.algo == 0 and args.arch == "unet" and args.dtype == "fp32" and not args.options and not args.deterministic:
            t_leg = time.perf_counter()
            live = live_traffic()
            t_leg = time.perf_counter() - t_leg
        if live is not None:
            traffic = round(live["per_launch"])
            traffic_unit = (f"HBM bytes per launch of this kernel family, MEASURED IN THIS RUN: two counter-only rocprofv3 passes (FETCH_SIZE x 2 [gfx950 tallies 128-B requests at 64 B] + WRITE_SIZE) "
                            f"over {live['steps']} training steps in a child process, {live['launches_per_step']:.1f} launches per step")
            sb = live["per_step_all_kernels"]
            step_traffic = {"hbm_bytes_per_step_all_kernels": round(sb), "vs_survey_54.3GB": round(sb / 54.300299148e9, 3), "vs_op_model": round(sb / max(sum(o[2] for o in ops), 1.0), 3),
                            "source": "measured in this run (the same two counter passes, summed over every kernel of a step)", "leg_seconds": round(t_leg, 1)}
        alg_bytes = sum(o[2] for o in dom) / max(launches, 1)
        H2R = 3.0 * FP32_MFMA_PEAK_TFLOPS / BF16_MFMA_PEAK_TFLOPS
        n_h2 = sum(int(abs(exec_ratio(o[0]) - H2R) < 1e-9) for o in dom)
        gbs = sum(o[2] for o in dom) / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        if n_h2 == launches and launches:
            # every launch of the dominant family runs on the fp16 matrix pipe (three products per fp32 multiply): price the products it EXECUTES against that pipe's dense peak
            prod = 3.0 * fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            roof = {"bound": "mfma", "kernel": f"conv3x3 fwd + data-gradient launches: conv_h2_kernel / conv_pp_kernel (fp32 in / out, block-scaled two-term fp16 split, 3 v_mfma_f32_32x32x16_f16 products "
                                               f"per multiply, {n_h2} launches)",
                    "achieved": round(prod, 1), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(prod / BF16_MFMA_PEAK_TFLOPS, 4),
                    "effective_tflops": round(effective, 2),
                    "note": "achieved / frac = fp16 MFMA FLOPs the matrix cores EXECUTE (3 products per fp32 multiply) / time vs the 2.5 PFLOP/s dense fp16 peak; "
                            "effective_tflops = ALGORITHMIC fp32 FLOPs (SURVEY 8d) of the same launches / the same time (the fp32 MFMA peak is 157.3)",
                    "hbm_gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4),
                    # measured on this chip, not in this run (profiles/r02_mfma_power_probe.txt): back-to-back fp16 MFMAs from registers with random, half-zero
                    # operands sustain 1.74 PFLOP/s at the package power cap (sclk ~1700 MHz); `peak` / `frac` stay the guide's nominal 2.5 PFLOP/s
                    "power_capped_peak": 1740.0, "frac_of_power_capped_peak": round(prod / 1740.0, 4)}
        else:
            roof = {"bound": "mfma", "kernel": f"conv3x3 fwd + data-gradient launches: conv_mfma_kernel<0,...> (strict fp32, v_mfma_f32_32x32x2_f32, {launches - n_h2} launches)"
                                               + (f" / conv_h2_kernel ({n_h2} launches)" if n_h2 else ""),
                    "achieved": round(effective, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(effective / FP32_MFMA_PEAK_TFLOPS, 4),
                    "effective_tflops": round(effective, 2),
                    "note": "achieved = ALGORITHMIC (direct-convolution, SURVEY 8d) FLOPs of these launches / their time, against the fp32 MFMA peak",
                    "hbm_gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}
        roof.update({"traffic": traffic,
                     "traffic_unit": traffic_unit,
                     "algorithmic_bytes_per_launch": round(alg_bytes),
                     "launches_per_step": launches, "avg_launch_ms": round(ms / max(launches, 1), 4),
                     "avg_launch_gflop": round(fl / max(launches, 1) / 1e9, 3),
                     "step_floor_ms": round(floor_ms, 3), "step_frac": round(floor_ms / (dt / args.steps * 1e3), 4),
                     "step_note": "step_floor_ms = sum over the step's ops of max(algorithmic bytes / 8 TB/s, executed matrix FLOPs / that pipe's peak); step_frac = floor / measured ms_per_step",
                     "step_hbm_gbs": round(sum(o[2] for o in ops) / (dt / args.steps) / 1e9, 1), "step_hbm_frac": round(sum(o[2] for o in ops) / (dt / args.steps) / 1e9 / HBM_PEAK_GBS, 4),
                     "step_traffic": step_traffic,
                     "profiled_steps": PROF_STEPS,
                     "op_ms_per_step": {k: round(v[0], 3) for k, v in sorted(groups.items(), key=lambda kv: -kv[1][0])}})
        if args.dtype == "bf16":
            # bf16 storage: the same launches priced against HBM (they move half the bytes and the bf16 MFMA rate is 16x the fp32 one)
            gbs = sum(o[2] for o in dom) / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
            step_bytes = sum(o[2] for o in ops)
            roof.update({"bound": "hbm", "kernel": "conv3x3 fwd + data-gradient launches: conv_bf16_kernel<0,...> (v_mfma_f32_32x32x16_bf16, direct)",
                         "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                         "mfma_tflops": round(effective, 1), "mfma_frac_of_bf16_peak": round(effective / BF16_MFMA_PEAK_TFLOPS, 4),
                         "note": "achieved = algorithmic bytes (activations at 2 B/element, weights 4 B) of these launches / their time; mfma_* = their algorithmic FLOP rate",
                         "step_algorithmic_bytes": round(step_bytes), "step_hbm_frac": round(step_bytes / (dt / args.steps) / 1e9 / HBM_PEAK_GBS, 4)})
            roof.pop("effective_tflops", None)

    if rank == 0:
        total_imgs = B * world * args.steps
        out = {
            "metric": (f"CT images/sec (fwd+bwd) U-Net {S}x{S}x1 bs{B}" if args.arch == "unet" else
                       f"CT images/sec (fwd+bwd) {'U-Net++' if args.arch == 'unetpp' else 'slice classifier'} {S}x{S}x1 bs{B}"), "value": round(total_imgs / dt, 3), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32" if args.algo != 0 else "f32 storage / accumulate / parameters; conv products as a two-term fp16 split (3 fp16 MFMAs per multiply, ~2^-22 per product; --algo 2 = strict fp32)")
                     if args.dtype == "fp32" else "bf16 storage, f32 accumulate/params", "data": "synthetic",
            "config": {"workload": (f"U-Net lung seg (task3 graph T3:850-913), {S}x{S}x1, batch {B}/GPU, fp32, fwd+loss+bwd+Keras-Adam" if args.arch == "unet" and args.config == 2 else
                                    f"U-Net infection seg (task1 graph T1:853-916), {S}x{S}x1, batch {B}/GPU, fp32, fwd+loss+bwd+Keras-Adam"
                                    if args.arch == "unet" else
                                    f"U-Net++ infection seg (task1_unet_plus_plus.py:858-950), {S}x{S}x1, batch {B}/GPU, fp32, fwd+loss+bwd+Keras-Adam"
                                    if args.arch == "unetpp" else
                                    f"slice classifier (task2_covid19_classifcation.py:747-776), {S}x{S}x1, batch {B}/GPU, fp32, fwd+BCE+bwd+Keras-Adam")
                                   + f"{', RCCL grad all-reduce + sync-BN/global-Dice' if world > 1 else ''}; BASELINE.json "
                                   + {"unet": "configs[2]" if args.config == 2 else "configs[1]", "unetpp": "configs[3] graph at the reference's fp32",
                                      "classifier": "configs[4] graph at the reference's 1-channel fp32"}[args.arch],
                       "storage": args.dtype, "global_batch": B * world, "parallelism": f"dp{world}", "small_allreduce": (("device (comm.hip: IPC-mapped areas, one kernel per reduction)" if eng._comm is not None else "torch.distributed") if eng._dp else None), "conv_algo": "mfma_f32_32x32x16_bf16 direct" if args.dtype == "bf16" else {0: "auto: every conv3x3 / ConvT forward, data gradient and weight gradient as three v_mfma_f32_32x32x16_f16 products of a block-scaled two-term fp16 split (h2; fp32-class accuracy, DESIGN.md 4g); Cin=1 first layer and 1x1 head on fp32 VALU", 1: "direct fp32 VALU kernels", 2: "strict fp32: v_mfma_f32_32x32x2_f32 direct kernels"}[args.algo],
                       "deterministic": bool(args.deterministic), "bn_fold": 3 if args.fold16 else 2, "dropout": {"unet": 0.25, "unetpp": "0.2/0.4 (fused in the conv epilogue)", "classifier": 0.4}[args.arch], "last_loss_dice": [round(v, 5) for v in loss_dice]},
        }
        if args.full:
            out["roofline"] = roof
        # the operating point of the timed region (median of ~100 Hz amdsmi samples on rank 0's GPU: mean shader clock over the 8 XCDs, socket power) -- the pool's boxes
        # differ by ~7 % on the same library; a slow BENCH line with a low clock is a slow box, not a regression
        if smi_timed is not None:
            out["sclk_mhz"] = smi_timed["sclk_mhz"]; out["power_w"] = smi_timed["power_w"]; out["smi_samples"] = smi_timed["samples"]
        if smi_prof is not None and smi_prof["sclk_mhz"] and isinstance(roof, dict) and roof.get("bound") == "mfma":
            # the dominant family's fraction against the matrix peak AT THE CLOCK THE PER-OP LEG RAN AT (peak scales with the shader clock: 2400 MHz nominal)
            roof["sclk_mhz_per_op_leg"] = smi_prof["sclk_mhz"]; roof["power_w_per_op_leg"] = smi_prof["power_w"]
            roof["frac_at_observed_clock"] = round(roof["achieved"] / (roof["peak"] * smi_prof["sclk_mhz"] / 2400.0), 4)
        if strict is not None:
            out["fp32_strict_img_s"] = strict
        if fit_stats is not None:
            out.update(fit_stats)
        if predict_ms is not None:
            out["predict_batch1_ms"] = predict_ms          # median of 20 synchronised model.predict calls at batch 1 (T1:1137): latency, not throughput
            out["predict_batch1_cold_ms"] = predict_cold_ms          # the same with the weight preparation redone per call (first predict after set_weights / a training step)
        if cpu is not None:
            out["cpu_baseline"] = cpu
        if comm is not None:
            out["comm"] = comm
    # The JSON line is the LAST thing on stdout: RCCL prints a version banner through C stdio, which sits in libc's buffer until exit and would
    # land behind an earlier Python print -- flush C stdio on every rank, meet, and only then print (rank 0) and tear the group down
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    sys.stdout.flush()
    if pg is not None:
        dist.barrier()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if pg is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

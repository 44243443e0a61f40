"""Times the registration of DESIGN.md section 4x on a synthetic 512 x 512 x 301 int16 pair (tests/register_oracle.py's analytic chest, 4.5 x its size, spacing (0.7,
0.7, 1.25); the follow-up on a grid of its own, the patient moved by (5.3, -3.7, 4.1) mm and (4.3, -2.6, 6.7) degrees, other noise):
  (a) one 16-candidate unet_vol_joint_hist launch under device events at each default level (8, 4, 2 mm: the fixed volume resampled, the moving one native) and once with
      the fixed volume at its native grid; two warm runs, then the median of `--runs`;
  (b) a whole volume.register_volumes (wall clock, a device synchronisation on both sides), beside the same search (volume.rigid_search) over a host evaluator --
      scipy.ndimage.affine_transform(order=1) of the decoded moving volume + numpy.histogram2d -- timed once on the box's threads.
Writes profiles/volume_register.json.

    python tools/register_bench.py [--runs 5] [--small] [--no-host]      (--small: 96 x 96 x 60 at 4.5 x the spacing, a functional check of the tool)
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
PIXDIM = (0.7, 0.7, 1.25)
MOTION_MM_DEG = (5.3, -3.7, 4.1, 4.3, -2.6, 6.7)
SCALE = 4.5                                                         # the phantom's 68 mm chest -> 306 mm
BINS, WINDOW = 32, (-1000.0, 400.0)


def event_ms(fn, runs, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return statistics.median(ts), ts


def centred(shape, pix, centre=(0.0, 0.0, 0.0)):
    A = np.diag([pix[0], pix[1], pix[2], 1.0])
    A[:3, 3] = np.asarray(centre) - A[:3, :3] @ ((np.asarray(shape) - 1) / 2.0)
    return A


def scan(shape, affine, to_anatomy, seed, coarse):
    """the phantom in the frame to_anatomy @ world, as int16 on (shape, affine): computed on a grid `coarse` times coarser and brought to the full grid by
    volume.resample_volume (float64 numpy at 79 M voxels would take minutes), noise added at the full resolution"""
    import register_oracle as RO
    from covidseg_amd import volume as V
    small = tuple(max(2, n // coarse) for n in shape)
    g, _ = V.resample_target(V.Grid(shape, affine), shape=small)
    v = RO.phantom(small, np.diag([1 / SCALE] * 3 + [1.0]) @ to_anatomy @ g.affine, seed, sigma=0.0)
    full = v.astype(np.float32) if coarse == 1 else V.resample_volume(v.astype(np.float32), shape=shape, affine=g.affine).data
    full = full + np.random.default_rng(seed).normal(0.0, 15.0, shape).astype(np.float32)
    return np.asfortranarray(np.clip(np.rint(full), -32768, 32767).astype(np.int16))


def host_levels(V, fixed_fd, fg, moving_fd, levels_mm):
    import scipy.ndimage as ndi
    edges = np.linspace(WINDOW[0], WINDOW[1], BINS + 1)
    levels = []
    for L, g, M in V.registration_level_grids(fg, levels_mm):
        fd = fixed_fd if M is None else ndi.affine_transform(fixed_fd, M[:, :3], M[:, 3], g.shape, order=1, mode="nearest")
        fclip = np.clip(fd, WINDOW[0], np.nextafter(WINDOW[1], -np.inf)).ravel()

        def evaluate(Ms, g=g, fclip=fclip):
            out = np.zeros((len(Ms), BINS, BINS), np.uint32)
            print(".", end="", flush=True, file=sys.stderr)          # (a sign of life: the 2 mm level takes minutes on the host)
            for c, Mc in enumerate(Ms):
                s = ndi.affine_transform(moving_fd, Mc[:, :3], Mc[:, 3], g.shape, order=1, mode="constant", cval=np.nan).ravel()
                ok = ~np.isnan(s)
                h, _, _ = np.histogram2d(fclip[ok], np.clip(s[ok], WINDOW[0], np.nextafter(WINDOW[1], -np.inf)), bins=(edges, edges))
                out[c] = h.astype(np.uint32)
            return out

        levels.append(V.RegistrationLevel(L, g, int(np.prod(g.shape)), evaluate))
    return levels


def corner_error(T_found, T_true, shape, affine):
    import register_oracle as RO
    return RO.corner_error(T_found, T_true, shape, affine)


def bench(small, runs, host):
    import torch
    from covidseg_amd import volume as V
    if small:
        fshape, mshape, pix_f, pix_m, coarse = (96, 96, 60), (100, 92, 56), tuple(4.5 * p for p in PIXDIM), (3.4, 3.4, 6.0), 1
    else:
        fshape, mshape, pix_f, pix_m, coarse = (512, 512, 301), (512, 512, 280), PIXDIM, (0.74, 0.74, 1.4), 4
    levels_mm = tuple(SCALE * v for v in V.REGISTER_LEVELS_MM) if small else V.REGISTER_LEVELS_MM
    Af, Am = centred(fshape, pix_f), centred(mshape, pix_m, (3.0, -2.0, 2.5))
    truth = V.RigidTransform(MOTION_MM_DEG[:3] + tuple(np.deg2rad(MOTION_MM_DEG[3:])), (0.0, 0.0, 0.0))
    fixed = scan(fshape, Af, np.eye(4), 1, coarse)
    moving = scan(mshape, Am, np.linalg.inv(truth.matrix), 2, coarse)
    fg, mg = V.Grid(fshape, Af), V.Grid(mshape, Am)
    out = {"fixed_shape": list(fshape), "fixed_pixdim": list(pix_f), "moving_shape": list(mshape), "moving_pixdim": list(pix_m), "levels_mm": list(levels_mm),
           "bins": BINS, "window": list(WINDOW), "true_motion_mm_deg": list(MOTION_MM_DEG)}
    # (a) the kernel alone: 16 candidates around the geometric start, per level and at the native grid
    fd, md = torch.from_numpy(fixed.reshape(-1, order="F").copy()).cuda(), torch.from_numpy(moving.reshape(-1, order="F").copy()).cuda()
    fv, mv = (4,) + fshape + (0, 1.0, 0.0), (4,) + mshape + (0, 1.0, 0.0)
    start = V.initial_transform(fg, mg)
    cands = [V.RigidTransform(start.params + 0.5 * c * np.array([1.0, -1.0, 0.5, 0.004, -0.003, 0.005]), start.centre) for c in range(V.JOINT_HIST_MAX_K)]
    out["joint_hist_16_candidates"] = []
    for L, g, M in V.registration_level_grids(fg, levels_mm) + [(None, fg, None)]:
        ldev, lv = (fd, fv) if M is None else (V.resample_linear_device(fd, fv, M, 0, 0.0, g.shape, 16), (16,) + g.shape + (0, 1.0, 0.0))
        Ms = np.stack([V.voxel_matrix(g, mg, T) for T in cands])
        counts = V.joint_hist_device(ldev, lv, None, md, mv, Ms, BINS, WINDOW, WINDOW)
        torch_counts = torch.empty((len(Ms), BINS, BINS), dtype=torch.int32, device="cuda")
        lib, ctx = V._ctx()
        flat = np.ascontiguousarray(Ms)

        def launch(ldev=ldev, lv=lv, flat=flat):
            ctx.check(lib.unet_vol_joint_hist(ctx.handle, ldev.data_ptr(), *lv, None, md.data_ptr(), *mv, flat.ctypes.data, len(flat), BINS, WINDOW[0], WINDOW[1], WINDOW[0],
                                              WINDOW[1], torch_counts.data_ptr(), V._stream()), "vol_joint_hist")

        ms, ts = event_ms(launch, runs)
        voxels = int(np.prod(g.shape))
        out["joint_hist_16_candidates"].append({"level_mm": L, "fixed_shape": list(g.shape), "ms": ms, "all_ms": ts, "counted_share": float(counts.sum()) / (len(Ms) * voxels),
                                                "voxel_candidates_per_us": len(Ms) * voxels / ms / 1e3})
    # (b) the whole registration
    for _ in range(2):
        reg = V.register_volumes(fixed, moving, levels_mm=levels_mm, fixed_affine=Af, moving_affine=Am)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    reg = V.register_volumes(fixed, moving, levels_mm=levels_mm, fixed_affine=Af, moving_affine=Am)
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    out["register_volumes"] = {"seconds": wall, "batches": reg.batches, "evaluations": reg.evaluations, "metric": reg.metric, "metric_init": reg.metric_init,
                               "overlap": reg.overlap, "converged": reg.converged, "params_mm_deg": list(reg.transform.params[:3]) + list(np.rad2deg(reg.transform.params[3:])),
                               "corner_error_mm_before": corner_error(start.matrix, truth.matrix, fshape, Af),
                               "corner_error_mm_after": corner_error(reg.transform.matrix, truth.matrix, fshape, Af),
                               "levels": [{"spacing": h["spacing"], "shape": list(h["shape"]), "batches": h["batches"], "metric": h["metric"]} for h in reg.history]}
    if not host:
        return out
    t0 = time.perf_counter()
    href = V.rigid_search(host_levels(V, fixed.astype(np.float64), fg, moving.astype(np.float64), levels_mm), fg, mg)
    hs = time.perf_counter() - t0
    out["host_path"] = {"seconds": hs, "batches": href.batches, "evaluations": href.evaluations, "metric": href.metric,
                        "corner_error_mm_after": corner_error(href.transform.matrix, truth.matrix, fshape, Af),
                        "same_params_as_device": bool(np.array_equal(href.transform.params, reg.transform.params))}
    out["host_over_device"] = hs / wall
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_register.json"))
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs, "threads": os.environ.get("OMP_NUM_THREADS"), "case": bench(a.small, a.runs, not a.no_host)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of on-device augmentation (HipUNet.take_augmented, csrc/kernels_augment.hip) at BASELINE.json configs[1] (U-Net 512 x 512 x 1, batch 16, fp32):
alternating blocks of `take` + train_batch and `take_augmented` + train_batch on ONE engine and one resident set, so clock drift hits both sides alike.
Every step draws a fresh shuffled batch (a device-side gather, as fit() does); the augmented side passes a view of one uploaded table per block (an epoch's).
Also times the two input kernels alone (events around back-to-back launches) against their byte floor.
Prints one JSON line: median ms / step of each side, their relative difference, and the kernels' us / call and achieved GB/s.

    python tools/augment_step_ab.py [--n 16] [--hw 512] [--set 64] [--steps 20] [--rounds 6]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd"))


def main():
    import numpy as np
    import torch
    import covidseg_amd  # noqa: F401
    from covidseg_amd.augment import AffineAugment
    from covidseg_amd.data import synthetic_ct
    from covidseg_amd.engine import HipUNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--set", type=int, default=64, help="samples in the resident training set")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per block")
    ap.add_argument("--rounds", type=int, default=6, help="(plain, augmented) block pairs")
    ap.add_argument("--kernel-calls", type=int, default=200)
    a = ap.parse_args()
    eng = HipUNet(a.hw, a.hw, 1)
    x, y = synthetic_ct(a.set, a.hw, seed=0)
    xd, yd = eng.resident(x, max_fraction=1.0), eng.resident(y, max_fraction=1.0)
    pol = AffineAugment()
    rng = np.random.RandomState(0)
    blk = [0]

    def block(aug):
        order = [rng.permutation(a.set)[:a.n] for _ in range(a.steps)]
        table = eng.augment_table(pol.matrices(a.n * a.steps, 0, blk[0], a.hw, a.hw)) if aug else None
        blk[0] += 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(a.steps):
            if aug:
                xb, yb = eng.take_augmented(xd, yd, order[s], table[s * a.n:(s + 1) * a.n])
            else:
                xb, yb = eng.take(xd, order[s]), eng.take(yd, order[s])
            eng.train_batch(xb, yb)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    t_end = time.perf_counter() + 3.0                                    # clocks settle under load (bench.py SETTLE_S)
    while time.perf_counter() < t_end:
        block(False)
    base, cur = [], []
    for r in range(a.rounds):
        for aug in ((False, True) if r % 2 == 0 else (True, False)):
            (cur if aug else base).append(block(aug))
    mb, mc = float(np.median(base)), float(np.median(cur))

    # the input kernels alone: unet_gather_samples x 2 (image + mask) vs one unet_augment_samples (both)
    idx = rng.permutation(a.set)[:a.n]
    table = eng.augment_table(pol.matrices(a.n, 1, 0, a.hw, a.hw))

    def timed(fn):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_calls):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.kernel_calls
    # (straight through the C ABI with the indices already on the device and the outputs allocated: the host side of take / take_augmented is not timed)
    di = torch.from_numpy(idx.astype(np.int64)).to(eng.dev)
    ox, oy = torch.empty((a.n, a.hw, a.hw, 1), device=eng.dev), torch.empty((a.n, a.hw, a.hw, 1), device=eng.dev)
    lib, h, st, sf = eng.lib, eng.ctx.handle, eng._stream(), a.hw * a.hw
    us_gather = timed(lambda: (lib.unet_gather_samples(h, xd.data_ptr(), di.data_ptr(), ox.data_ptr(), a.n, sf, st),
                               lib.unet_gather_samples(h, yd.data_ptr(), di.data_ptr(), oy.data_ptr(), a.n, sf, st)))
    us_aug = timed(lambda: lib.unet_augment_samples(h, xd.data_ptr(), yd.data_ptr(), di.data_ptr(), table.data_ptr(), ox.data_ptr(), oy.data_ptr(),
                                                    a.n, a.hw, a.hw, 1, st))
    xa, ya = eng.take_augmented(xd, yd, idx, table)
    torch.cuda.synchronize()
    assert torch.equal(xa, ox) and torch.equal(ya, oy)
    nbytes = 2 * 2 * a.n * a.hw * a.hw * 4                                # read + write of image and mask
    out = {"config": f"unet {a.hw}x{a.hw} bs{a.n} fp32, resident set {a.set}", "steps_per_block": a.steps, "rounds": a.rounds,
           "ms_plain": round(mb, 4), "ms_augmented": round(mc, 4), "rel": round(mc / mb - 1.0, 5),
           "ms_plain_blocks": [round(v, 4) for v in base], "ms_augmented_blocks": [round(v, 4) for v in cur],
           "input_bytes_floor_mb": round(nbytes / 1e6, 2), "floor_us_at_8tbs": round(nbytes / 8e12 * 1e6, 2),
           "us_take_image_and_mask": round(us_gather, 2), "us_take_augmented": round(us_aug, 2),
           "gbs_take": round(nbytes / (us_gather * 1e-6) / 1e9, 1), "gbs_take_augmented": round(nbytes / (us_aug * 1e-6) / 1e9, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

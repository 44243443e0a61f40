#!/usr/bin/env python
"""Cost of the selectable losses (HipUNet.set_loss): times train_batch at BASELINE.json configs[1] (U-Net 512 x 512 x 1, batch 16, fp32) for each loss,
in alternating blocks against the default bce_dice_loss on the SAME engine (set_loss switches the live plan), so clock drift hits both sides alike.
Prints one JSON line: per loss the median ms / step of its blocks, of the default blocks next to them, and the relative difference.

    python tools/loss_step_ab.py [--n 16] [--hw 512] [--steps 20] [--rounds 5] [--losses dice_loss,tversky_loss,binary_crossentropy]
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
    from covidseg_amd.data import synthetic_ct
    from covidseg_amd.engine import HipUNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per block")
    ap.add_argument("--rounds", type=int, default=5, help="(default, loss) block pairs per loss")
    ap.add_argument("--losses", default="dice_loss,tversky_loss,binary_crossentropy")
    a = ap.parse_args()
    eng = HipUNet(a.hw, a.hw, 1)
    x, y = synthetic_ct(a.n, a.hw, seed=0)
    xd, yd = eng.resident(x, max_fraction=1.0), eng.resident(y, max_fraction=1.0)
    idx = np.arange(a.n)
    xb, yb = eng.take(xd, idx), eng.take(yd, idx)

    def block(name):
        eng.set_loss(name)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.train_batch(xb, yb)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    t_end = time.perf_counter() + 3.0                                    # clocks settle under load (bench.py SETTLE_S)
    while time.perf_counter() < t_end:
        block("bce_dice_loss")
    out = {"config": f"unet {a.hw}x{a.hw} bs{a.n} fp32", "steps_per_block": a.steps, "rounds": a.rounds, "losses": {}}
    for name in [s for s in a.losses.split(",") if s]:
        base, cur = [], []
        for r in range(a.rounds):
            order = ("bce_dice_loss", name) if r % 2 == 0 else (name, "bce_dice_loss")
            for nm in order:
                (base if nm == "bce_dice_loss" else cur).append(block(nm))
        mb, mc = float(np.median(base)), float(np.median(cur))
        out["losses"][name] = {"ms_default": round(mb, 4), "ms": round(mc, 4), "rel": round(mc / mb - 1.0, 5),
                               "ms_default_blocks": [round(v, 4) for v in base], "ms_blocks": [round(v, 4) for v in cur]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

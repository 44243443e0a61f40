"""Generate tests/golden/loss_family_goldens.npz by EXECUTING the reference's own loss closures that compile(loss=...) can select.

Runs only where the reference scripts are present.  dice_loss (T1:792-794, with dice_coeff T1:784-790), tversky_loss (T1:801-816) and weighted_bce_dice_loss (T1:835-847, with weighted_bce_loss
T1:861-867) are AST-extracted
from the reference's task1_preprocessing_plus_unet_with_comments.py and exec'd against a float64 NumPy stand-in for ``keras.backend`` (``K``), as
make_loss_goldens.py does; its pool2d restates TF's SAME average pool (TF is not a dependency) by brute force.  Only the resulting input / output VECTORS are committed -- no reference source text is stored.

    python tests/golden/make_loss_family_goldens.py path/to/Scripts/task1_preprocessing_plus_unet_with_comments.py
"""
import ast
import os
import sys

import numpy as np

WANT = ["dice_coeff", "dice_loss", "tversky_loss", "weighted_bce_loss", "weighted_bce_dice_loss"]


class K:  # float64 NumPy shim of the keras.backend calls those closures make
    flatten = staticmethod(lambda a: np.asarray(a).reshape(-1))
    sum = staticmethod(lambda a, axis=None: np.sum(a, axis=tuple(axis) if isinstance(axis, (tuple, list)) else axis))
    ones = staticmethod(lambda shape: np.ones(tuple(int(s) for s in shape)))
    shape = staticmethod(lambda a: np.asarray(a).shape)
    cast = staticmethod(lambda a, dtype: np.asarray(a, np.float64))
    ones_like = staticmethod(lambda a: np.ones_like(np.asarray(a, np.float64)))
    clip = staticmethod(np.clip)
    log = staticmethod(np.log)
    exp = staticmethod(np.exp)
    abs = staticmethod(np.abs)
    maximum = staticmethod(np.maximum)

    @staticmethod
    def pool2d(y, pool_size, strides=(1, 1), padding="valid", pool_mode="max"):
        """TF avg_pool, stride 1, SAME padding, restated from TF's published semantics: window rows r - (k-1)//2 ... r + k//2 (columns alike) clipped to the
        image, divided by the in-image cell count -- brute force"""
        assert tuple(strides) == (1, 1) and padding == "same" and pool_mode == "avg"
        y = np.asarray(y, np.float64)
        kh, kw = pool_size
        n, h, w, c = y.shape
        out = np.empty_like(y)
        for r in range(h):
            r0, r1 = max(r - (kh - 1) // 2, 0), min(r + kh // 2, h - 1) + 1
            for q in range(w):
                c0, c1 = max(q - (kw - 1) // 2, 0), min(q + kw // 2, w - 1) + 1
                out[:, r, q, :] = y[:, r0:r1, c0:c1, :].mean(axis=(1, 2))
        return out


def extract(path, names):
    tree = ast.parse(open(path).read())
    ns = {"K": K, "np": np}
    found = {node.name: node for node in ast.walk(tree) if isinstance(node, ast.FunctionDef) and node.name in names}
    for n in names:
        exec(compile(ast.Module(body=[found[n]], type_ignores=[]), f"<ref:{n}>", "exec"), ns)
    return ns


def cases(rng):
    out = []
    for shape in [(2, 8, 8, 1), (2, 64, 64, 1), (1, 128, 96, 1)]:
        t = np.round(rng.random(shape) ** 3 * 255) / 255.0             # soft labels k/255
        t[rng.random(shape) < 0.5] = 0.0
        out.append((t, rng.random(shape)))
        tb = (rng.random(shape) > 0.9).astype(np.float64)             # a small binary mask (the infection masks' imbalance)
        out.append((tb, rng.random(shape) * 0.3))
    t = np.zeros((2, 8, 8, 1)); out.append((t, np.full_like(t, 0.25)))   # empty mask
    t = np.ones((2, 8, 8, 1)); out.append((t, np.full_like(t, 0.9)))      # full mask
    t = (rng.random((2, 8, 8, 1)) > 0.5).astype(float)
    p = rng.random((2, 8, 8, 1)); p.flat[:4] = [0.0, 1.0, 1e-9, 1 - 1e-9]  # clip edges
    out.append((t, p))
    return out


def main():
    if len(sys.argv) < 2 and "REFERENCE_ROOT" not in os.environ:
        sys.exit("usage: make_loss_family_goldens.py <task1_preprocessing_plus_unet_with_comments.py>  (or REFERENCE_ROOT=<reference checkout>)")
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.environ["REFERENCE_ROOT"], "Scripts", "task1_preprocessing_plus_unet_with_comments.py")
    ns = extract(ref, WANT)
    rng = np.random.default_rng(20261016)
    arrs = {}
    for i, (t, p) in enumerate(cases(rng)):
        arrs[f"t{i}"], arrs[f"p{i}"] = t, p
        arrs[f"dice_loss{i}"] = np.float64(ns["dice_loss"](t, p))
        arrs[f"tversky_loss{i}"] = np.float64(np.asarray(ns["tversky_loss"](t, p)).reshape(()))
        arrs[f"weighted_bce_dice_loss{i}"] = np.float64(ns["weighted_bce_dice_loss"](t, p))
        arrs[f"avg_pool{i}"] = K.pool2d(t, (50, 50), strides=(1, 1), padding="same", pool_mode="avg")
    arrs["n_cases"] = np.int64(i + 1)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loss_family_goldens.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes;", i + 1, "cases")


if __name__ == "__main__":
    main()

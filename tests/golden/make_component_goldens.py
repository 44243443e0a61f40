"""Writes tests/golden/component_goldens.npz with the REAL skimage.measure.label and skimage.morphology.remove_small_objects (scikit-image 0.18.3:
/opt/conda/bin/python3.9 of the build image).  Run by hand:

    /opt/conda/bin/python3.9 tests/golden/make_component_goldens.py

Per case `name`: `name/shape`, `name/bits` (np.packbits of mask != 0 in C order), `name/values` (the non-zero values of a multi-valued mask, in C order; absent
for 0 / 1 masks), `name/c` connectivity, `name/labels` int32 = label(mask != 0, connectivity=c), `name/n`, `name/min_size`, `name/removed_bits` =
packbits(remove_small_objects(mask != 0, min_size, connectivity=c)).
"""
import os
import sys

import numpy as np
from skimage import measure, morphology

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import components_oracle as CO  # noqa: E402  (the mask generators only)


def cases():
    shape = (20, 24, 12)
    for dens, tag in ((0.05, "d05"), (0.31, "d31"), (0.6, "d60")):
        for c in (1, 2, 3):
            yield f"random_{tag}_c{c}", CO.random_mask(shape, dens, 100 + c), c, 4
    yield "serpentine_c1", CO.serpentine((21, 19, 9)), 1, 10
    for c in (1, 2, 3):
        yield f"checkerboard_c{c}", CO.checkerboard((9, 10, 7)), c, 2
    yield "ones_c1", np.ones((7, 5, 6), np.uint8), 1, 3
    yield "zeros_c3", np.zeros((7, 5, 6), np.uint8), 3, 3
    multi = CO.random_mask(shape, 0.31, 7) * np.random.default_rng(8).choice(np.array([1, 2, 255], np.uint8), shape)
    yield "multivalued_c1", multi.astype(np.uint8), 1, 5
    yield "multivalued_c3", multi.astype(np.uint8), 3, 5


def main():
    out = {}
    for name, mask, c, min_size in cases():
        fg = mask != 0
        labels, n = measure.label(fg, connectivity=c, return_num=True)
        removed = morphology.remove_small_objects(fg, min_size=min_size, connectivity=c)
        out[name + "/shape"] = np.asarray(mask.shape, np.int32)
        out[name + "/bits"] = np.packbits(fg.reshape(-1))
        if mask.max(initial=0) > 1:
            out[name + "/values"] = mask[fg]
        out[name + "/c"] = np.int32(c)
        out[name + "/labels"] = labels.astype(np.int32)
        out[name + "/n"] = np.int32(n)
        out[name + "/min_size"] = np.int32(min_size)
        out[name + "/removed_bits"] = np.packbits(removed.reshape(-1))
        print(f"{name}: {mask.shape} c={c} n={n} kept {int(removed.sum())} of {int(fg.sum())}")
    path = os.path.join(HERE, "component_goldens.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Random flip + affine augmentation of the reference's training sets, drawn on the host and applied on the device.

The reference builds one imgaug pipeline in every segmentation script (T1:547-583, CV3:547-583, CV4:582-618, UPP:582-618, T3:536-572) and in the
classification script (T2:557-584):

    seq = iaa.Sequential([iaa.Fliplr(0.5), iaa.Flipud(0.2),
                          sometimes(iaa.Affine(scale={"x": (0.8, 1.2), "y": (0.8, 1.2)},
                                               translate_percent={"x": (-0.2, 0.2), "y": (-0.2, 0.2)},
                                               rotate=(-40, 40), shear=(-16, 16)))], random_order=True)

AffineAugment restates it as one 2x3 matrix per sample.  Semantics (imgaug 0.4, written down here once; the tests hold the kernel to it):

* Coordinates are pixel indices (x = column, y = row) with pixel centres at integers; c = (W/2 - 0.5, H/2 - 0.5) is the image centre.
* Fliplr, with probability `fliplr`: x -> W - 1 - x.  Flipud, with probability `flipud`: y -> H - 1 - y.
* Affine, with probability `p_affine`: F = T(c) . A . T(-c) with skimage's AffineTransform matrix
  A = [[sx cos r, -sy sin(r + s), tx], [sx sin r, sy cos(r + s), ty]], sx, sy ~ U(scale) independently, tx = U(translate) * W, ty = U(translate) * H,
  r = deg2rad(U(rotate)), s = deg2rad(U(shear)).  Only x-shear, as imgaug does for a scalar shear.
* random_order: every sample draws a permutation (o1, o2, o3) of the three steps; the composed forward map is F_o3 . F_o2 . F_o1 (a step that is not
  drawn is the identity).  Composition and inversion run in float64; the stored row is the INVERSE map (output pixel -> source pixel), rounded to float32:
  row = [m00, m01, m02, m10, m11, m12] with (xs, ys) = (m00 x + m01 y + m02, m10 x + m11 y + m12).
* Images are sampled bilinearly, masks by nearest neighbour (floor(s + 0.5)); both read 0 outside the source (imgaug order=1 / segmentation order=0,
  mode="constant", cval=0).  A bilinear tap outside the source reads 0: cv2's BORDER_CONSTANT, scipy's mode="grid-constant".

Deliberate departures from imgaug:

* imgaug draws ONE step order per call (per batch); here every sample draws its own, so a sample's augmentation does not depend on how batches are cut.
* The random stream is numpy's PCG64 seeded by SeedSequence([seed, epoch]), 12 uniforms per sample whether it uses them or not: the table of an epoch depends
  on (seed, epoch, n) only -- never on the rank, the world size or the batch size -- and row k is the same for every n > k.
* cv2 rounds sub-pixel positions to 1/32 px; the kernel does not.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

STEPS = ("fliplr", "flipud", "affine")
DRAWS_PER_ROW = 12          # 3 coins, 3 keys of the step order, 6 affine parameters


def _range(name, v, lo_bound=None, hi_abs=None):
    lo, hi = (float(v[0]), float(v[1])) if np.ndim(v) else (-abs(float(v)), abs(float(v)))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError(f"AffineAugment: {name} must be a finite range (lo, hi) with lo <= hi, got {v!r}")
    if lo_bound is not None and lo <= lo_bound:
        raise ValueError(f"AffineAugment: {name} must be > {lo_bound}, got {v!r}")
    if hi_abs is not None and max(abs(lo), abs(hi)) >= hi_abs:
        raise ValueError(f"AffineAugment: |{name}| must be < {hi_abs}, got {v!r}")
    return lo, hi


@dataclass
class Draws:
    """The parameters drawn for n samples (policy.sample): what the matrices are built from."""
    fliplr: np.ndarray          # [n] bool
    flipud: np.ndarray          # [n] bool
    affine: np.ndarray          # [n] bool
    order: np.ndarray           # [n, 3] int: a permutation of (0 fliplr, 1 flipud, 2 affine), applied left to right
    scale_x: np.ndarray         # [n] float64 (drawn for every sample; used where affine is True)
    scale_y: np.ndarray
    translate_x: np.ndarray     # fraction of W
    translate_y: np.ndarray     # fraction of H
    rotate: np.ndarray          # degrees
    shear: np.ndarray           # degrees


class AffineAugment:
    """The reference's `seq` (defaults) or any policy of the same shape.  sample() draws, matrices() builds the float32 [n, 6] inverse-map table."""

    def __init__(self, fliplr=0.5, flipud=0.2, p_affine=0.5, scale=(0.8, 1.2), translate=(-0.2, 0.2), rotate=(-40, 40), shear=(-16, 16)):
        for name, p in (("fliplr", fliplr), ("flipud", flipud), ("p_affine", p_affine)):
            if not (0.0 <= float(p) <= 1.0):
                raise ValueError(f"AffineAugment: {name} is a probability in [0, 1], got {p!r}")
        self.fliplr, self.flipud, self.p_affine = float(fliplr), float(flipud), float(p_affine)
        self.scale = _range("scale", scale, lo_bound=0.0)
        self.translate = _range("translate", translate)
        self.rotate = _range("rotate", rotate)
        self.shear = _range("shear", shear, hi_abs=90.0)

    def config(self) -> dict:
        """The constructor's arguments (AffineAugment(**p.config()) is the same policy): how a policy travels to the ranks of a data-parallel runner."""
        return {"fliplr": self.fliplr, "flipud": self.flipud, "p_affine": self.p_affine, "scale": list(self.scale), "translate": list(self.translate),
                "rotate": list(self.rotate), "shear": list(self.shear)}

    def __repr__(self):
        return (f"AffineAugment(fliplr={self.fliplr}, flipud={self.flipud}, p_affine={self.p_affine}, scale={self.scale}, translate={self.translate}, "
                f"rotate={self.rotate}, shear={self.shear})")

    def sample(self, n: int, seed: int, epoch: int) -> Draws:
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed), int(epoch)])))
        u = rng.random((int(n), DRAWS_PER_ROW))                   # row-major: row k is the same draw for every n > k
        lin = lambda col, r: r[0] + (r[1] - r[0]) * u[:, col]
        return Draws(fliplr=u[:, 0] < self.fliplr, flipud=u[:, 1] < self.flipud, affine=u[:, 2] < self.p_affine,
                     order=np.argsort(u[:, 3:6], axis=1, kind="stable"),
                     scale_x=lin(6, self.scale), scale_y=lin(7, self.scale), translate_x=lin(8, self.translate), translate_y=lin(9, self.translate),
                     rotate=lin(10, self.rotate), shear=lin(11, self.shear))

    def matrices(self, n: int, seed: int, epoch: int, h: int, w: int) -> np.ndarray:
        """float32 [n, 6]: row k = the inverse map of the k-th position of epoch `epoch`'s order (output pixel -> source pixel) for h x w images."""
        return matrices_from_draws(self.sample(n, seed, epoch), h, w)


def forward_steps(d: Draws, h: int, w: int) -> np.ndarray:
    """float64 [n, 3, 3, 3]: the forward 3x3 map of each step (fliplr, flipud, affine) per sample; the identity where the step was not drawn."""
    n = len(d.fliplr)
    out = np.broadcast_to(np.eye(3), (n, 3, 3, 3)).copy()
    out[d.fliplr, 0, 0, 0], out[d.fliplr, 0, 0, 2] = -1.0, w - 1.0
    out[d.flipud, 1, 1, 1], out[d.flipud, 1, 1, 2] = -1.0, h - 1.0
    r, s = np.deg2rad(d.rotate), np.deg2rad(d.shear)
    a = np.zeros((n, 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2] = d.scale_x * np.cos(r), -d.scale_y * np.sin(r + s), d.translate_x * w
    a[:, 1, 0], a[:, 1, 1], a[:, 1, 2] = d.scale_x * np.sin(r), d.scale_y * np.cos(r + s), d.translate_y * h
    a[:, 2, 2] = 1.0
    cx, cy = w / 2.0 - 0.5, h / 2.0 - 0.5
    tc, tmc = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]]), np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
    f = tc @ a @ tmc
    out[d.affine, 2] = f[d.affine]
    return out


def matrices_from_draws(d: Draws, h: int, w: int) -> np.ndarray:
    steps = forward_steps(d, h, w)
    n = len(d.fliplr)
    fwd = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    for j in range(3):                                         # F = F_o3 . F_o2 . F_o1
        fwd = steps[np.arange(n), d.order[:, j]] @ fwd
    inv = np.linalg.inv(fwd)
    return np.ascontiguousarray(inv[:, :2, :].reshape(n, 6), np.float32)


def resolve(augment):
    """fit(augment=...) -> None (no augmentation) or an AffineAugment: True is the reference's policy, a dict the arguments of one (AffineAugment.config)."""
    if augment is None or augment is False:
        return None
    if augment is True:
        return AffineAugment()
    if isinstance(augment, AffineAugment):
        return augment
    if isinstance(augment, dict):
        return AffineAugment(**augment)
    raise ValueError(f"augment must be None, True, an AffineAugment or its config() dict, got {augment!r}")

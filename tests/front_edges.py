"""What tests/test_gpu_front_edges.py and tests/test_front_edges_host.py share (TEST INFRASTRUCTURE ONLY): the case lists of the first kernels a CT meets
(csrc/kernels_volume.hip: unet_vol_slices_f64, unet_vol_unslice; csrc/kernels_pre.hip: the unet_pre_* entry points), the volumes and images they are run on, the
launch caps the "second trip" shapes are chosen against, and a guarded device buffer whose data may start off its alignment.  Everything here but `Guarded` is numpy
on the host: the host module evaluates the conditions the cases rest on without a GPU."""
import numpy as np

import volume_oracle as VO

CODES = {"u1": 2, "i1": 256, "i2": 4, "u2": 512, "i4": 8, "u4": 768, "f4": 16, "f8": 64}
INT_KINDS = ("u1", "i1", "i2", "u2", "i4", "u4")
OK, E_ARG, E_SHAPE = 0, -1, -3                                      # include/unet_hip.h: UNET_OK, UNET_E_ARG, UNET_E_SHAPE
SCALE = (float(np.float32(0.37)), float(np.float32(-1024.5)))       # scl_slope, scl_inter as a float32 header stores them

# ---- the launch caps: items one trip of a grid-stride loop covers, from the launch lines of the two files (TPB = 256 in both) ------------------------------
TPB = 256
VOL_RESIZE_TRIP = 1024 * TPB            # vol_resize_kernel, dim3(vol_blocks(P, 1024), n): destination pixels, and the voxels of the slice in the uniform scan
VOL_OUTPUTS1_TRIP = 1024 * TPB          # vol_outputs_kernel<1>, dim3(vol_blocks(P, 1024), n): pixels
VOL_OUTPUTS4_TRIP = 256 * TPB * 4       # vol_outputs_kernel<4>, dim3(vol_blocks(P / 4, 256), n): pixels, four per thread
VOL_UNSLICE1_TRIP = 1024 * TPB          # vol_unslice_kernel<1>, dim3(vol_blocks((long long)X * Y, 1024), n): voxels of a slice
VOL_UNSLICE4_TRIP = 256 * TPB * 4       # vol_unslice_kernel<4>, dim3(vol_blocks((long long)(X / 4) * Y, 256), n): voxels of a slice, four per thread
PRE_MINMAX_TRIP = 256 * TPB             # minmax_kernel / norm_to_u8_kernel, bx = blocks_for(pixels, 256): pixels of an image
PRE_MINMAX_INIT_TPB = 64                # minmax_init_kernel, dim3((n + 63) / 64), dim3(64): images per workgroup
PRE_UNIT_TRIP = 2048 * TPB              # unit_to_u8_kernel / u8_to_unit_kernel, dim3(blocks_for(count, 2048)): elements

# ---- A. slices ----------------------------------------------------------------------------------------------------------------------------------------------
# (name, source shape (X, Y, Z), S, what strides): every grid-stride loop of unet_vol_slices_f64 makes a second trip in one of them
STRIDE_CASES = [("outputs<4> and resize", (20, 50, 2), 516), ("outputs<1> and resize", (20, 50, 2), 515), ("uniform scan, area tables", (520, 510, 2), 16)]
NAN_SHAPE, NAN_SIZES = (37, 23, 4), (31, 16, 48)
UNIFORM_SHAPE = (48, 48, 6)


def smooth_volume(shape, kind, seed):
    """a volume with structure in every axis plus noise (test_gpu_volume.py's)"""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    a = 90 * np.sin(x / 7.0 + z) * np.cos(y / 5.0) + rng.normal(0, 20, shape)
    if kind.startswith("u"):
        a = np.clip(a + 128, 0, 255)
    return np.asfortranarray(a.astype(kind))


def nan_inf_volume(kind):
    """slice 0: all NaN; slice 1: one NaN; slice 2: one +inf; slice 3: one -inf (the lone values away from the borders, so that a bilinear blend meets them with a
    zero weight from more than one side)"""
    raw = smooth_volume(NAN_SHAPE, kind, 5)
    raw[:, :, 0] = np.nan
    raw[17, 9, 1] = np.nan
    raw[5, 20, 2] = np.inf
    raw[30, 3, 3] = -np.inf
    return raw


def uniform_volumes():
    """-> (int16 volume, float32 volume, expected uniform flags of the float32 one's slices 1..4).  Slice 1 constant; slice 2 constant but for the last voxel in memory;
    slice 3 constant but for voxel (1, 0); slice 4 (float32 only) holds -0.0 and +0.0, one value to np.unique"""
    X, Y, _ = UNIFORM_SHAPE
    i2 = smooth_volume(UNIFORM_SHAPE, "i2", 3)
    i2[:, :, 1] = -1000
    i2[:, :, 2] = 417; i2[X - 1, Y - 1, 2] = 418
    i2[:, :, 3] = 417; i2[1, 0, 3] = 416
    f4 = np.asfortranarray(i2.astype(np.float32))
    f4[:, :, 4] = np.where(np.random.default_rng(4).random((X, Y)) < 0.5, np.float32(-0.0), np.float32(0.0))
    return i2, f4, [1, 0, 0, 1]


# ---- B. every datatype over its whole range -----------------------------------------------------------------------------------------------------------------
RANGE_SHAPE, RANGE_S = (37, 23, 4), 31


def full_range_volume(kind, seed=0):
    """integers drawn uniformly over np.iinfo(kind), the minimum and the maximum both present (twice each: once on the first slice, once on the last)"""
    info = np.iinfo(kind)
    rng = np.random.default_rng(seed + CODES[kind])
    a = rng.integers(info.min, info.max, RANGE_SHAPE, dtype=np.int64, endpoint=True).astype(kind)
    a[3, 2, 0], a[20, 11, 0] = info.min, info.max
    a[36, 22, 3], a[0, 0, 3] = info.min, info.max
    return np.asfortranarray(a)


def range_layouts(shape, seed=7):
    """(name, labels, mask, n, region): two of test_gpu_intensity.py's layouts"""
    rng = np.random.default_rng(seed)
    region = (rng.random(shape) < 0.6).astype(np.uint8) * 3
    sparse = rng.integers(-2, 10, shape)
    sparse[sparse == 3] = 0                                         # label 3 has no voxel; -2, -1, 0 and 7..9 lie outside 1..6
    return [("one group over everything", None, np.full(shape, 2, np.uint8), 1, None), ("missing and outside labels, region", sparse, None, 6, region)]


# ---- C. unslice -----------------------------------------------------------------------------------------------------------------------------------------------
UNSLICE_S = 96
# (name, (X, Y, Z), z0, z1, threshold, byte offset of the mask pointer)
UNSLICE_CASES = [
    ("X % 4 == 0, unslice<4> strides, the whole range", (516, 510, 3), 0, 3, 0.547, 0),
    ("the scalar loop strides, a single slice", (517, 509, 2), 1, 2, 0.547, 0),
    ("X % 4 == 0 behind a mask pointer off by one byte", (120, 100, 4), 1, 3, 0.547, 1),
    ("one row of four voxels", (4, 1, 1), 0, 1, 0.547, 0),
    ("one voxel", (1, 1, 1), 0, 1, 0.547, 0),
    ("a threshold above every canvas value", (120, 100, 4), 1, 3, 2.0, 0),
    ("a negative threshold", (120, 100, 4), 1, 3, -0.25, 0),
    ("a negative threshold, the scalar kernel", (121, 99, 3), 0, 3, -0.25, 0),
]
NEAR, NEAR_SHARE_CAP = 1e-6, 0.001                                  # test_gpu_volume.py's rule: voxels may differ only within NEAR of the threshold, at most this share lies there


def canvas(n, seed, S=UNSLICE_S):
    """smooth float32 maps in [0.02, 0.98] that cross a threshold along curves (test_gpu_volume.py's synthetic_prob)"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:S, 0:S].astype(np.float64) / S
    out = np.empty((n, S, S), np.float32)
    for i in range(n):
        a, b, c = rng.uniform(2, 9, 3)
        out[i] = 0.5 + 0.48 * np.sin(a * u + c) * np.cos(b * v - c)
    return out


def unslice_case(case):
    """-> (canvas float32 [n, S, S], float32 oracle mask [X, Y, Z], near [n, Y, X]: where the float64 oracle's probability lies within NEAR of the threshold)"""
    name, shape, z0, z1, t, _ = case
    c = canvas(z1 - z0, shape[0] + 7 * shape[1])
    wmask, _, _ = VO.unslice(c, t, shape, z0, z1)
    _, _, p64 = VO.unslice(c, t, shape, z0, z1, np.float64)
    return c, wmask, np.abs(p64 - t) <= NEAR


# ---- D. the uint8 front ---------------------------------------------------------------------------------------------------------------------------------------
def minmax_expected(a):
    """np.uint8((a - a.min()) / (a.max() - a.min()) * 255) of one float32 image with the cast written out (volume_oracle._u8_trunc): no platform warning decides a byte"""
    a = np.asarray(a, np.float64)
    mn, mx = a.min(), a.max()                                       # numpy's min / max propagate a NaN
    with np.errstate(invalid="ignore", divide="ignore"):
        return VO._u8_trunc((a - mn) / (mx - mn) * 255)


def minmax_batch():
    """five 37 x 91 float32 slices: plain, one NaN, one +inf, one -inf, constant"""
    x = np.random.default_rng(5).normal(-600, 400, (5, 37, 91)).astype(np.float32)
    x[1, 20, 45] = np.nan
    x[2, 3, 90] = np.inf
    x[3, 36, 0] = -np.inf
    x[4] = np.float32(-731.5)
    return x


def unit_edges():
    """float32 k / 255 for the 256 byte values and the float32 just below each: where the truncation of x * 255 decides"""
    k = (np.arange(256, dtype=np.float64) / 255).astype(np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(-1.0))[1:]])          # (nothing below 0: np.uint8 of a negative product is not defined by the expression)


UNIT_COUNTS = (1, 255, PRE_UNIT_TRIP + 3)

# ((h, w), (tiles_x, tiles_y), clip limits): tiles of 1 x 1 and 2 x 2 pixels, one axis padded by a whole tile, grids that are not square
CLAHE_CASES = [((8, 8), (8, 8), (3.0,)), ((9, 9), (8, 8), (3.0, 0.0, 40.0)), ((16, 9), (8, 8), (3.0,)), ((17, 16), (8, 8), (3.0, 0.0, 40.0)), ((15, 17), (8, 8), (3.0,)),
               ((5, 5), (4, 4), (3.0,)), ((64, 65), (8, 8), (3.0,)), ((2, 3), (3, 2), (3.0,)), ((1, 1), (1, 1), (3.0,))]
CLAHE_REFUSED = [((8, 9), (8, 8)), ((3, 5), (2, 3))]                # the reflect-101 padding reaches the image size


def clahe_padding(shape, tiles):
    """(rows, columns) OpenCV adds in front of the tile grid: `tiles - size % tiles` on BOTH axes as soon as one does not divide"""
    (h, w), (tx, ty) = shape, tiles
    return (0, 0) if (w % tx == 0 and h % ty == 0) else (ty - h % ty, tx - w % tx)


def clahe_batch(shape):
    """three images: random, constant, a ramp"""
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    return np.stack([(rng.random(shape) * 255).astype(np.uint8), np.full(shape, 37, np.uint8), (np.arange(shape[0] * shape[1]).reshape(shape) * 7 % 251).astype(np.uint8)])


RESIZE_SRC = (40, 52)                                               # sh, sw
# x, y, w, h: touching the right edge, the bottom edge, both with 1 x 1, a column 1 x h, a row w x 1 on the last row
RESIZE_RECTS = np.array([[35, 5, 17, 20], [3, 29, 20, 11], [51, 39, 1, 1], [7, 0, 1, 40], [0, 39, 52, 1]], np.int32)
RESIZE_DST = dict(dh=12, dw=9, dst_x0=5, dst_ld=20)


def resize_sources():
    rng = np.random.default_rng(52)
    yy, xx = np.mgrid[0:RESIZE_SRC[0], 0:RESIZE_SRC[1]]
    return np.stack([np.clip(120 + 90 * np.sin(yy / (5.0 + i)) * np.cos(xx / (9.0 - i)) + rng.normal(0, 6, RESIZE_SRC), 0, 255).astype(np.uint8) for i in range(len(RESIZE_RECTS))])


# ---- a device buffer between guard bands whose data may start off its alignment -------------------------------------------------------------------------------
GUARD, SENT = 256, 0xA5                                             # bytes per band (a multiple of every alignment asked for), the sentinel byte


class Guarded:
    """n elements of `dtype` (a numpy dtype name) between two guard bands of SENT bytes, the data filled with SENT too.  skew: bytes by which the data start past a
    256-byte boundary.  test_gpu_texture.py's pattern, on bytes so that the start can be off its alignment"""

    def __init__(self, n, dtype, skew=0):
        import torch
        self.dtype, self.nbytes, self.skew = np.dtype(dtype), int(n) * np.dtype(dtype).itemsize, int(skew)
        self.full = torch.full((GUARD + self.skew + self.nbytes + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        assert self.full.data_ptr() % 256 == 0
        self.ptr = self.full.data_ptr() + GUARD + self.skew

    def get(self, what=""):
        """the data as numpy, after checking both bands"""
        import torch
        torch.cuda.synchronize()
        a = self.full.cpu().numpy()
        lo = GUARD + self.skew
        assert (a[:lo] == SENT).all() and (a[lo + self.nbytes:] == SENT).all(), f"guard band written: {what}"
        return a[lo:lo + self.nbytes].copy().view(self.dtype)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.full == SENT).all().item())

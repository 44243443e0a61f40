"""What tests/test_gpu_later_trips.py and tests/test_later_trips_host.py share (TEST INFRASTRUCTURE ONLY): the launch caps of the volume kernels' bounded grids, restated
from csrc/ (the host module reads every constant's text out of its .hip file, so a changed cap fails there instead of disarming a case), and the cases whose shapes make
every workgroup of such a launch go through its loop at least twice, and some a third, ragged time.  Everything here is numpy on the host.

Three rules hold for every case, and the host module asserts them without a GPU:
  shape    every workgroup makes at least two trips and at least one makes a further one that is short of a workgroup (and of a wave where x runs along the lanes);
  content  at least half of the items a later trip reaches (index >= one launch's worth) carry information: sampled inside the source, inside the mask, not NaN, the
           first voxel of a run;
  equality the device test compares every output with the family's own oracle for equality, between sentinel bands."""
import numpy as np

import deform_oracle as DO
import resample_oracle as RS

TPB = 256
WAVE = 64

# ---- the launch caps, as the sources state them ---------------------------------------------------------------------------------------------------------------------
GRID_CAP = 256 * 32                     # workgroups of a launch in kernels_resample / deform / intensity / lungside / render / texture .hip
TRIP = GRID_CAP * TPB                   # items one trip of such a launch covers: 2,097,152
RS_TILE, RS_TILED_MIN = 64, 16          # kernels_resample.hip: TILE, TILED_MIN
JH_GRID_CAP = 1024                      # kernels_register.hip: workgroups per candidate
JH_TRIP = JH_GRID_CAP * TPB
SM_SEG, SM_ROWS = 64, TPB // 64         # kernels_deform.hip, sm_x_kernel: a tile is ROWS rows x SEG outputs along x
IB_GRID, IB_CHUNK, IB_TABLE, IB_GROUPS = 256 * 4, TPB * 16, 4096, 1024          # kernels_intensity.hip, ib_bands_kernel
MOM_CHUNK = 256                         # kernels_intensity.hip, mom_chunk_kernel: elements per partial-sum slot
TQ_TABLE = 4096                         # kernels_texture.hip: (group, level) counters of tq_quantize_kernel<true>
GLCM_WG_PER_CU, BRICK = 3, (32, 8, 8)   # kernels_texture.hip: persistent workgroups per CU, BX x BY x BZ
GLCM_LDS_COUNTERS = 8192                # include/unet_hip.h: UNET_VOL_TEXTURE_LDS_COUNTERS

# (file under csrc/, the constant, the regular expression whose group is its value, the value restated above)
CAP_SOURCES = [
    ("kernels_resample.hip", "GRID_CAP", r"constexpr long long GRID_CAP = ([^;]+);", GRID_CAP),
    ("kernels_resample.hip", "TILE", r"constexpr int TILE = ([^;]+);", RS_TILE),
    ("kernels_resample.hip", "TILED_MIN", r"constexpr int TILED_MIN = ([^;]+);", RS_TILED_MIN),
    ("kernels_register.hip", "GRID_CAP", r"constexpr long long GRID_CAP = ([^;]+);", JH_GRID_CAP),
    ("kernels_deform.hip", "GRID_CAP", r"constexpr long long GRID_CAP = ([^;]+);", GRID_CAP),
    ("kernels_deform.hip", "SEG", r"constexpr int SEG = ([^,;]+),", SM_SEG),
    ("kernels_deform.hip", "ROWS", r"constexpr int SEG = [^,;]+, ROWS = ([^;]+);", SM_ROWS),
    ("kernels_intensity.hip", "GRID_CAP", r"constexpr long long GRID_CAP = ([^;]+);", GRID_CAP),
    ("kernels_intensity.hip", "IB_GRID", r"constexpr int IB_GRID = ([^;]+);", IB_GRID),
    ("kernels_intensity.hip", "IB_CHUNK", r"constexpr int IB_CHUNK = ([^;]+);", IB_CHUNK),
    ("kernels_intensity.hip", "IB_TABLE", r"constexpr int IB_TABLE = ([^;]+);", IB_TABLE),
    ("kernels_intensity.hip", "IB_GROUPS", r"constexpr int IB_GROUPS = ([^;]+);", IB_GROUPS),
    ("kernels_intensity.hip", "MOM_CHUNK", r"constexpr int MOM_CHUNK = ([^;]+);", MOM_CHUNK),
    ("kernels_lungside.hip", "GRID_CAP", r"constexpr long long GRID_CAP = ([^;]+);", GRID_CAP),
    ("kernels_render.hip", "GRID_CAP", r"constexpr long long GRID_CAP = ([^;]+);", GRID_CAP),
    ("kernels_texture.hip", "GRID_CAP", r"constexpr long long GRID_CAP = ([^;]+);", GRID_CAP),
    ("kernels_texture.hip", "TQ_TABLE", r"constexpr int TQ_TABLE = ([^;]+);", TQ_TABLE),
    ("kernels_texture.hip", "GLCM_WG_PER_CU", r"constexpr int GLCM_WG_PER_CU = ([^;]+);", GLCM_WG_PER_CU),
] + [(f, "TPB", r"constexpr int TPB = ([^;]+);", TPB) for f in ("kernels_resample.hip", "kernels_register.hip", "kernels_deform.hip", "kernels_intensity.hip", "kernels_lungside.hip",
                                                              "kernels_render.hip", "kernels_texture.hip")]


def constant_value(text):
    """the value of a constant written as a product of integers and TPB, e.g. "256 * 32" or "TPB * 16" """
    v = 1
    for tok in text.split("*"):
        tok = tok.strip()
        if "/" in tok:
            a, b = (t.strip() for t in tok.split("/"))
            v *= (TPB if a == "TPB" else int(a)) // int(b)
        else:
            v *= TPB if tok == "TPB" else int(tok)
    return v


def later_trips(items, per_trip):
    """items walked by a launch that covers per_trip of them at a time -> (whole trips every workgroup makes, items left for the last, partial one)"""
    return int(items) // int(per_trip), int(items) % int(per_trip)


def shape_rule(items, per_trip, lanes_along_x=True):
    """every workgroup makes two trips, and a further trip exists that ends short of a workgroup (and of a wave)"""
    full, rest = later_trips(items, per_trip)
    return full >= 2 and rest > 0 and rest % TPB != 0 and (not lanes_along_x or rest % WAVE != 0)


def flat(a):
    """a volume [X, Y, Z] as the device holds it: x fastest"""
    return np.asarray(a).reshape(-1, order="F")


def tail_share(cond, start=TRIP):
    """the share of the items from `start` on, in device order, where `cond` holds"""
    f = flat(cond)[start:]
    assert f.size > 0
    return float(np.count_nonzero(f)) / f.size


# ---- volumes ------------------------------------------------------------------------------------------------------------------------------------------------------
def volume(shape, kind, seed, nan_share=0.02):
    """-> (raw [X, Y, Z] Fortran order, NIfTI code, scaling or None): the two storage kinds of the per-family tests; the float kind with few enough NaNs that most blends
    of eight neighbours are numbers"""
    rng = np.random.default_rng(seed)
    if kind == "i2":
        return np.asfortranarray(rng.integers(-1200, 600, shape, dtype=np.int16)), 4, (0.5, -100.0)
    assert kind == "f4nan"
    raw = (rng.standard_normal(shape, dtype=np.float32) * np.float32(500))
    raw[rng.random(shape, dtype=np.float32) < nan_share] = np.nan
    raw[:, 0, 0] = np.nan
    raw[-1, -1, -1] = np.inf
    return np.asfortranarray(raw), 16, None


def mask_of(shape, seed, share=0.75):
    """a uint8 mask with `share` of the voxels set (values 1..255), and the first two waves of the flat volume emptied"""
    rng = np.random.default_rng(seed)
    m = (rng.random(shape, dtype=np.float32) < share).astype(np.uint8) * rng.integers(1, 255, shape, dtype=np.uint8)
    f = flat(m).copy()
    f[:128] = 0
    return np.asfortranarray(f.reshape(shape, order="F"))


def inside(M, out_shape, src_shape):
    """where the source coordinate of an output voxel lies inside the source on every axis (what a sampler answers there is no cval)"""
    ok = np.ones(tuple(out_shape), bool)
    for s, n in zip(RS.coords(M, out_shape), src_shape):
        ok &= (s >= 0.0) & (s <= float(n - 1))
    return ok


# ---- 1. resample, the direct mapping ------------------------------------------------------------------------------------------------------------------------------
RS_OUT, RS_SRC = (257, 129, 127), (158, 133, 52)                     # 4,210,431 outputs; a source that RS_OUT's oblique and anisotropic images nearly fill
RS_MATRICES = {"oblique": RS.oblique_matrix, "anisotropic": RS.anisotropic_matrix}
# (storage, matrix, mode, dst): both matrices in both modes, float64 and uint8, both storage kinds
RS_DIRECT_LINEAR = [("i2", "oblique", 1, 64), ("i2", "anisotropic", 0, 2), ("f4nan", "oblique", 0, 2), ("f4nan", "anisotropic", 1, 64)]
RS_DIRECT_NEAREST = [("oblique", 1), ("anisotropic", 0)]            # two-byte elements
RS_CVAL = -1000.25


def rs_lane_axis(M, Y2, Z2):
    """kernels_resample.hip's choice: the output axis source x depends on most (ties to the lower), 0 when that axis is shorter than TILED_MIN"""
    M = np.asarray(M, np.float64).reshape(3, 4)
    a = 0
    for c in (1, 2):
        if abs(M[0, c]) > abs(M[0, a]):
            a = c
    if (a == 1 and Y2 < RS_TILED_MIN) or (a == 2 and Z2 < RS_TILED_MIN):
        a = 0
    return a


# ---- 2. resample, the tiled mapping -----------------------------------------------------------------------------------------------------------------------------------
# (matrix, output): tiles with x0 > 0 and a0 > 0 at once, ragged on both axes
RS_TILED_SMALL = [("perm_x_from_y", (70, 70, 3)), ("perm_x_from_z", (70, 3, 70))]
# (matrix, output, the lane axis, order, element bytes or dst, mode): 16,500 tiles
RS_TILED_LONG = [("perm_x_from_y", (3, 17, 16500), 1, "nearest", 2, 1), ("perm_x_from_z", (3, 16500, 17), 2, "linear", 16, 0)]


def perm_case(name, out):
    """-> (the source shape whose permutation fills `out`, M): test_gpu_resample.py's two permutations that feed source x from another output axis"""
    if name == "perm_x_from_y":
        src = (out[1], out[0], out[2])
        return src, np.array([[0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, src[1] - 1.0], [0.0, 0.0, 1.0, 0.0]])
    assert name == "perm_x_from_z"
    src = (out[2], out[1], out[0])
    return src, np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, src[2] - 1.0]])


def rs_tiles(out, a):
    """(tiles along x, tiles along the lane axis, tiles in all) of rs_tiled_kernel"""
    tx, ta = -(-out[0] // RS_TILE), -(-out[a] // RS_TILE)
    return tx, ta, tx * ta * out[3 - a]


# ---- 3. the joint histogram ---------------------------------------------------------------------------------------------------------------------------------------------
JH_FIXED, JH_MOVING = (131, 67, 61), (67, 33, 31)                    # 535,397 fixed voxels: two trips of 262,144 and 43 workgroups + 101 lanes
JH_WINDOWS = ((-500.0, 200.0), (-300.5, 150.25))                    # test_gpu_register.py's: narrower than the data
JH_RUNS = [(16, 64, False), (16, 2, True), (1, 64, True), (1, 2, False)]          # (K, bins, with the mask)


def jh_matrices():
    """sixteen candidates as a search step would try them: the zoom that lays the fixed grid over the moving one, turned about z by up to 3 degrees around the
    centre and shifted by fractions of a voxel -> [16, 3, 4]"""
    zoom = np.diag([(m - 1.0) / (f - 1.0) for f, m in zip(JH_FIXED, JH_MOVING)])
    cf, cm = (np.array(JH_FIXED) - 1.0) / 2.0, (np.array(JH_MOVING) - 1.0) / 2.0
    out = []
    for k in range(16):
        t = np.deg2rad((k - 7.5) * 0.4)
        R = np.array([[np.cos(t), -np.sin(t), 0.0], [np.sin(t), np.cos(t), 0.0], [0.0, 0.0, 1.0]])
        A = R @ zoom
        M = np.zeros((3, 4))
        M[:, :3] = A
        M[:, 3] = cm - A @ cf + np.array([(k % 4 - 1.5) * 0.3, (k // 4 - 1.5) * 0.2, (k % 3 - 1.0) * 0.25])
        out.append(M)
    return np.stack(out)


def jh_volumes():
    """-> (fixed raw, code, scaling), (moving raw, code, scaling), mask"""
    return volume(JH_FIXED, "i2", 131), volume(JH_MOVING, "f4nan", 67), mask_of(JH_FIXED, 5)


def jh_constant_pair():
    """a constant fixed and a constant moving volume of the fixed shape: under the identity every counted voxel of every wave falls into one cell"""
    return np.asfortranarray(np.full(JH_FIXED, -300, np.int16)), np.asfortranarray(np.full(JH_FIXED, 40, np.int16))


# ---- 4. the Gaussian pass -------------------------------------------------------------------------------------------------------------------------------------------------
SM_C, SM_SHAPE = 3, (130, 111, 99)                                   # 24,726 tiles along x, the last row group one row short; 4,285,710 elements along y and z
SM_RADII = (1, 32)
SM_SPECIALS = {(2, 129, 110, 98): np.nan, (2, 64, 50, 40): np.inf, (1, 3, 100, 95): -np.inf}          # all in the part only a later trip reaches, on every axis


def sm_tiles(C, shape):
    rows = C * shape[1] * shape[2]
    segs = -(-shape[0] // SM_SEG)
    return -(-rows // SM_ROWS) * segs, segs


def sm_field():
    x = np.random.default_rng(130).standard_normal((SM_C,) + SM_SHAPE, dtype=np.float32) * np.float32(300)
    for at, v in SM_SPECIALS.items():
        x[at] = v
    return x


def sm_weights(R):
    return np.random.default_rng(R).random(2 * R + 1) / (R + 0.5)  # the existing test's random weights


def field_index(c, i, j, k, shape):
    """where element (c, i, j, k) of a component-major field lies on the device"""
    return i + shape[0] * (j + shape[1] * (k + shape[2] * c))


# ---- 5. demons step, warp, Jacobian -------------------------------------------------------------------------------------------------------------------------------------------
DF_GRID, DF_MOVING = RS_OUT, RS_SRC
DF_COARSE = (86, 43, 43)
DF_F = np.array([[0.35, 0.02, 0.0, 0.1], [-0.03, 0.34, 0.01, -0.2], [0.0, 0.05, 0.3, 0.05]])          # test_gpu_deform.py's: output voxel -> field voxel, partly outside the field
# (name, the field's grid: "on_grid" or "coarse", order, dst dtype code (order 0: the stored int16), mode)
DF_WARPS = [("on the grid, linear to float32", "on_grid", 1, 16, 1), ("on the grid, nearest int16", "on_grid", 0, 4, 0), ("coarse field through F, linear to float64", "coarse", 1, 64, 0)]
DF_DELTA = 2.0


def oblique3(seed):
    """test_gpu_deform.py's oblique, anisotropic 3 x 3 (a rotated, sheared spacing) and its inverse"""
    A = RS.oblique_affine((2.0, 1.5, 3.0), 20.0 + seed)[:3, :3] @ np.array([[1.0, 0.1, 0.0], [0.0, 1.0, -0.05], [0.0, 0.0, 1.0]])
    return A, np.linalg.inv(A)


def random_field(shape, seed, scale):
    return np.random.default_rng(seed).standard_normal((3,) + tuple(shape), dtype=np.float32) * np.float32(scale)


def folded_field(shape):
    """test_gpu_deform.py's linear field whose determinant is negative everywhere under FOLDED_AINV"""
    return np.moveaxis(DO.world_points(shape, np.diag([2.0, 4.0, 0.5, 1.0])) @ np.diag([-1.5, 0.25, 0.0]), -1, 0).astype(np.float32)


FOLDED_AINV = np.diag([0.5, 0.25, 2.0])


# ---- 6. intensity: gather, bands, moments -------------------------------------------------------------------------------------------------------------------------------------
IV_SLOPE, IV_INTER = 0.5, -1024.0
IG_SHAPE, IG_N = RS_OUT, 3
IB_EDGES = np.array([-1080.0, -1050.0, -1024.0, -1000.0, -960.0])
# (shape, n): per = 3 chunks per workgroup; one chunk a slice, and two chunks a slice; the LDS-table arm and the global-atomic arm (n (B + 1) > IB_TABLE)
IB_CASES = [((5, 1, 2100), 4), ((5, 1, 2100), 3000), ((70, 70, 1030), 4), ((70, 70, 1030), 3000)]
MOM_N = 4180000


def ib_walk(shape):
    """-> (cps, chunks, per, grid) of the counting launch"""
    XY = shape[0] * shape[1]
    cps = -(-XY // IB_CHUNK)
    chunks = cps * shape[2]
    per = -(-chunks // IB_GRID)
    return cps, chunks, per, -(-chunks // per)


def ig_case():
    """-> (raw float32 with NaNs, labels int32 (0..3 and a few outside 1..n), region uint8)"""
    rng = np.random.default_rng(257)
    raw = (rng.standard_normal(IG_SHAPE, dtype=np.float32) * np.float32(40)).round() * np.float32(0.5)
    raw[rng.random(IG_SHAPE, dtype=np.float32) < 0.02] = np.nan
    labels = rng.integers(0, IG_N + 1, IG_SHAPE, dtype=np.int32)
    labels[rng.random(IG_SHAPE, dtype=np.float32) < 0.01] = IG_N + 2
    labels[0, 0, 0], labels[1, 0, 0] = -1, 2 ** 31 - 1
    region = (rng.random(IG_SHAPE, dtype=np.float32) < 0.9).astype(np.uint8) * 3
    return np.asfortranarray(raw), np.asfortranarray(labels), np.asfortranarray(region)


def ib_case(shape, n):
    """-> (raw int16 (decoded with IV_SLOPE, IV_INTER), labels int32 in 0..n with a tenth outside, region uint8)"""
    rng = np.random.default_rng(shape[2] + n)
    raw = rng.integers(-150, 150, shape, dtype=np.int16)
    labels = rng.integers(1, n + 1, shape, dtype=np.int32)
    labels[rng.random(shape, dtype=np.float32) < 0.1] = 0
    region = (rng.random(shape, dtype=np.float32) < 0.9).astype(np.uint8)
    return np.asfortranarray(raw), np.asfortranarray(labels), np.asfortranarray(region)


def mom_case(n=MOM_N):
    """n runs of one or two values -> (values float64, offsets int64 [n + 1])"""
    rng = np.random.default_rng(n)
    sizes = rng.integers(1, 3, n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return rng.normal(-420.0, 310.0, int(off[-1])), off


def mom_closed_form(values, off):
    """intensity_oracle.moments for runs of one or two values, vectorised: sum = a (+ b); ssd = fl(d0 d0) (+ fl(d1 d1)) with d = fl(v - fl(sum / m))"""
    off = np.asarray(off, np.int64)
    m = np.diff(off)
    assert m.min() >= 1 and m.max() <= 2
    a = values[off[:-1]]
    two = m == 2
    b = values[np.where(two, off[:-1] + 1, off[:-1])]
    s = np.where(two, a + b, a)
    mean = s / m.astype(np.float64)
    d0, d1 = a - mean, b - mean
    return np.stack([s, np.where(two, d0 * d0 + d1 * d1, d0 * d0)], axis=1)


def mom_slots(off):
    n = len(off) - 1
    return int(off[-1]) // MOM_CHUNK + n


# ---- 7. the side of every lung voxel --------------------------------------------------------------------------------------------------------------------------------------
SA_SCALAR_N = 257 * 129 * 127                                        # behind a mask pointer off its alignment by one byte: one voxel per lane
SA_VECTOR_N = 2 * TRIP * 4 + 3                                       # four voxels per lane: two whole trips and one short item


def sa_inputs(N, seed):
    """test_gpu_lungside.py's inputs for N voxels in a row: a mask with whole background waves, distances with few distinct values (ties), +inf on either or both sides"""
    rng = np.random.default_rng(seed)
    mask = (rng.random(N, dtype=np.float32) < 0.6).astype(np.uint8) * rng.integers(1, 255, N, dtype=np.uint8)
    mask[256:512] = 0
    mask[TRIP + 256:TRIP + 512] = 0
    a = rng.integers(0, 40, N).astype(np.float64) * 0.5625
    b = rng.integers(0, 40, N).astype(np.float64) * 0.5625
    b[::7] = a[::7]
    a[3::11] = np.inf
    b[5::13] = np.inf
    b[3::33] = np.inf
    return mask, a, b


# ---- 8. projections ----------------------------------------------------------------------------------------------------------------------------------------------------------
# (name, shape, axis, a, b, storage): pj_walk_kernel over 4,210,695 outputs; pj_wave_kernel over 66,049 columns, one wave each, 32,768 a trip
PJ_CASES = [("walk along y", (2049, 2, 2055), 1, 0, 2, "i2"), ("walk along z", (2049, 2055, 2), 2, 0, 2, "i2"), ("a wave per column along x", (70, 257, 257), 0, 3, 69, "f4nan")]
PJ_WAVE_TRIP = GRID_CAP * (TPB // WAVE)


def pj_labels(shape, seed):
    """test_gpu_render.py's layers: a uint8 mask that touches the border and int32 labels with negative and large ones"""
    rng = np.random.default_rng(100 + seed)
    mask = (rng.random(shape, dtype=np.float32) < 0.45).astype(np.uint8) * rng.integers(1, 250, shape, dtype=np.uint8)
    mask[0] = 7; mask[:, -1] = 1
    lab = rng.integers(-3, 14, shape, dtype=np.int32)
    lab[rng.random(shape, dtype=np.float32) < 0.3] = 0
    lab[-1, 0, 0] = 2 ** 31 - 1
    return np.asfortranarray(mask), np.asfortranarray(lab)


# ---- 9. texture: quantize, runs, GLCM ------------------------------------------------------------------------------------------------------------------------------------
TX_SHAPE = RS_OUT
TQ_CASES = [(3, 32, 0), (3, 32, 1), (700, 8, 0), (700, 8, 1)]        # (n, Ng, outside): n Ng = 96 in the LDS table, 5600 beyond it; clip and drop
TQ_LO = -1090.0


def tq_width(Ng):
    """the bins span 128 of the 150 decoded units: values clip or drop at both ends"""
    return 128.0 / Ng


TR_BITS, TR_MAX_RUN, TR_NG, TR_N = (1 << 0) | (1 << 2) | (1 << 12), 64, 8, 3
TR_LINE = (5, 7, 30, 101)                                            # x, y, z from .. to: 71 voxels of one level along z, from the first trip into the second


def tq_case(n):
    """-> (raw int16 (decoded with IV_SLOPE, IV_INTER), labels int32: three quarters in 1..n)"""
    rng = np.random.default_rng(n)
    raw = rng.integers(-150, 150, TX_SHAPE, dtype=np.int16)
    N = int(np.prod(TX_SHAPE))
    labels = (np.arange(N, dtype=np.int64) % (n + 5) + 1).astype(np.int32) if n > 64 else rng.integers(1, n + 1, N, dtype=np.int32)
    labels[rng.random(N, dtype=np.float32) < 0.25] = 0
    return np.asfortranarray(raw), np.asfortranarray(labels.reshape(TX_SHAPE, order="F"))


def tr_case():
    """-> (levels uint8, labels int32): test_gpu_texture.py's structured levels (runs along every direction, a tenth at level 0), groups in blocks, and TR_LINE"""
    rng = np.random.default_rng(12)
    x, y, z = np.indices(TX_SHAPE, dtype=np.int16)
    lev = ((x // 3 + y // 2 + z) % TR_NG + 1).astype(np.uint8)
    noise = rng.random(TX_SHAPE, dtype=np.float32)
    lev = np.where(noise < 0.3, rng.integers(1, TR_NG + 1, TX_SHAPE, dtype=np.uint8), lev)
    lev = np.where(noise > 0.9, 0, lev).astype(np.uint8)
    labels = rng.integers(0, TR_N + 1, (22, 9, 13), dtype=np.int32).repeat(12, axis=0).repeat(15, axis=1).repeat(10, axis=2)[:TX_SHAPE[0], :TX_SHAPE[1], :TX_SHAPE[2]].copy()
    lx, ly, z0, z1 = TR_LINE
    lev[lx, ly, z0:z1], labels[lx, ly, z0:z1] = 2, 1
    lev[lx, ly, z0 - 1], lev[lx, ly, z1] = 1, 1
    return np.asfortranarray(lev), np.asfortranarray(labels)


def run_starts(lev, labels, n, Ng, direction):
    """where a run along `direction` begins: the voxel takes part and its predecessor lies outside the volume or differs in level or group"""
    lv = np.asarray(lev).astype(np.int32)
    g = np.where((labels >= 1) & (labels <= n), labels, 0)
    key = np.where((lv > 0) & (lv <= Ng) & (g > 0), g * 256 + lv, 0)
    prev = np.zeros_like(key)
    src, dst = [], []
    for d, dim in zip(direction, key.shape):
        src.append(slice(0, dim - d) if d >= 0 else slice(-d, dim))
        dst.append(slice(d, dim) if d >= 0 else slice(0, dim + d))
    prev[tuple(dst)] = key[tuple(src)]
    return (key > 0) & (prev != key)


GLCM_NG, GLCM_N = 4, 3
GLCM_XY = (3, 400)                                                   # 1 x 50 thin bricks a slab


def glcm_grid(cus):
    return cus * GLCM_WG_PER_CU


def glcm_shape(cus):
    """at least 4.2 bricks per persistent workgroup: every workgroup meets four, some a fifth"""
    per_slab = -(-GLCM_XY[0] // BRICK[0]) * -(-GLCM_XY[1] // BRICK[1])
    return GLCM_XY + (BRICK[2] * -(-(42 * glcm_grid(cus)) // (10 * per_slab)),)


def glcm_bricks(shape):
    """the brick number of every voxel, as tg_glcm_kernel counts them: x fastest"""
    nbx, nby = -(-shape[0] // BRICK[0]), -(-shape[1] // BRICK[1])
    x, y, z = np.indices(shape, dtype=np.int32)
    return (x // BRICK[0]) + nbx * ((y // BRICK[1]) + nby * (z // BRICK[2]))


def glcm_case(cus, n=GLCM_N):
    """-> (levels uint8, labels int32).  Workgroup w walks the bricks w, w + G, w + 2 G, ..: its first brick is empty, its second is not, its third is empty when w is
    odd, and the rest are not"""
    shape = glcm_shape(cus)
    G = glcm_grid(cus)
    rng = np.random.default_rng(cus)
    x, y, z = np.indices(shape, dtype=np.int32)
    lev = ((x + y // 2 + z) % GLCM_NG + 1).astype(np.uint8)
    lev = np.where(rng.random(shape) < 0.3, rng.integers(1, GLCM_NG + 1, shape), lev)
    lev = np.where(rng.random(shape) < 0.1, 0, lev).astype(np.uint8)
    b = glcm_bricks(shape)
    trip, w = b // G, b % G
    lev[(trip == 0) | ((trip == 2) & (w % 2 == 1))] = 0
    labels = rng.integers(0, 4, (1, 40, shape[2] // 4 + 1)).repeat(3, axis=0).repeat(10, axis=1).repeat(4, axis=2)[:, :, :shape[2]].astype(np.int32)
    if n > 3:                                                       # many groups: beyond the LDS table
        labels = np.where(labels > 0, labels + 3 * ((z // 4) % (n // 3)), 0).astype(np.int32)
    lev = np.where(labels > 0, lev, 0).astype(np.uint8)
    return np.asfortranarray(lev), np.asfortranarray(labels)


def glcm_walks(lev, Ng, cus):
    """what every persistent workgroup meets, in order: a string of "e" (the brick's own voxels hold no level 1..Ng: left after the core check) and "s" (staged)"""
    G = glcm_grid(cus)
    b = glcm_bricks(lev.shape)
    nbricks = int(b.max()) + 1
    part = (np.asarray(lev) > 0) & (np.asarray(lev) <= Ng)
    staged = np.bincount(b.reshape(-1), weights=part.reshape(-1), minlength=nbricks) > 0
    return ["".join("s" if staged[k] else "e" for k in range(w, nbricks, G)) for w in range(min(G, nbricks))]

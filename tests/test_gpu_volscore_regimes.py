"""-m gpu: the code paths of csrc/kernels_volscore.hip and of unet_vol_paste_back that score_volume / segment_volume never enter, against the float64 / integer
oracles (tests/volscore_oracle.py, components_oracle.py, volume_oracle.py), through the C ABI and the thin device wrappers of covidseg_amd.volume.

A. the distance transform on axes of 600 .. 4096 voxels: the x pass's four 1024-voxel chunks with their forward and backward carries, the line pass with 4, 2 and 1
   lines per workgroup (L = 600 -> 4, 1025 / 1500 -> 2, 2049 / 4096 -> 1: the whole LDS tile for a single line), ragged tiles.  Bit-exact: np.array_equal.
B. lesion coverage where the atomics fall back: a voxel whose label differs from the first of its group of four, a wave that holds three or more labels, labels
   outside 1..n.  Exact.  How often each fallback runs is a condition on the data that test_overlap_cases_reach_both_fallbacks evaluates without a GPU.
C. unet_vol_surface_distances with a buffer shorter than the surface, no buffer at all, and a surface that does not start on a 16-byte boundary.  Count, maximum and
   the gathered values are exact; the sum lies within (sum_chain(N) + 1) 2^-53 relative of math.fsum(sqrt(d2)): the chain of additions include/unet_hip.h documents,
   plus one rounding for the square root -- derived, not measured.
D. unet_vol_paste_back over 130 slices: three launches of at most 64 slices, the later ones offset into prob, canvas and the rectangle list."""
import functools
import math

import numpy as np
import pytest

import components_oracle as CO
import volscore_oracle as SO
import volume_oracle as VO
from test_gpu_volscore import SPACINGS, ULP
from test_gpu_volume import synthetic_prob

gpu = pytest.mark.gpu

E_SHAPE = -3
SENT = -7.0                                                          # no d2 and no square root is negative
SENT_I = -0x0123456789ABCDEF                                         # no count is negative
GUARD = 16                                                           # sentinel words around an output; 16 doubles keep the 16-byte alignment of what lies between
INF = float("inf")


def _bytes_dev(a):
    import torch
    return torch.from_numpy(np.asfortranarray(np.asarray(a).astype(np.uint8)).reshape(-1, order="F").copy()).cuda()


def _labels_dev(a):
    import torch
    return torch.from_numpy(np.asfortranarray(np.asarray(a).astype(np.int32)).reshape(-1, order="F").copy()).cuda()


# ---- A. the distance transform on long axes ----------------------------------------------------------------------------------------------------------
EDT_SHAPES = [(0, (1025, 3, 2)), (0, (2049, 2, 3)), (0, (4095, 1, 3)), (0, (4096, 2, 2)),
              (1, (5, 600, 2)), (1, (5, 1025, 2)), (1, (3, 2049, 2)), (1, (3, 4096, 1)),
              (2, (5, 2, 600)), (2, (3, 2, 1500)), (2, (2, 3, 4096))]


def _edt(vol, nonzero, pixdim, ops):
    """unet_vol_edt_sq through ctypes -> float64 [X, Y, Z]; the output lies between two rows of sentinels, which must survive"""
    import torch
    X, Y, Z = vol.shape
    buf = torch.full((vol.size + 2 * GUARD,), SENT, dtype=torch.float64, device="cuda")
    w = np.ascontiguousarray(np.asarray(pixdim, np.float64) ** 2)
    dev = _bytes_dev(vol)
    ops.ck(ops.lib.unet_vol_edt_sq(ops.h, dev.data_ptr(), X, Y, Z, 1 if nonzero else 0, w.ctypes.data, buf.data_ptr() + 8 * GUARD, None, 0, ops.s), "vol_edt_sq")
    out = buf.cpu().numpy()
    assert (out[:GUARD] == SENT).all() and (out[GUARD + vol.size:] == SENT).all(), f"{vol.shape}: unet_vol_edt_sq wrote outside its output"
    return out[GUARD:GUARD + vol.size].reshape(vol.shape, order="F")


def _check_edt(vol, nonzero, pixdim, ops, what):
    got = _edt(vol, nonzero, pixdim, ops)
    want = SO.edt_sq_lines(vol, nonzero, pixdim)
    bad = got != want
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {bad.size} voxels differ; first at {np.argwhere(bad)[0]}: {got[bad][0]!r} against {want[bad][0]!r}"
    assert np.array_equal(got, want), what
    return got


def _lines(shape, axis):
    """the (other-axes) coordinates of every line along `axis`, as index tuples with a slice at `axis`"""
    others = [range(n) if a != axis else [slice(None)] for a, n in enumerate(shape)]
    return [(i, j, k) for i in others[0] for j in others[1] for k in others[2]]


def _edt_patterns(shape, axis):
    """(name, volume) -- features are the non-zero voxels"""
    L = shape[axis]
    lines = _lines(shape, axis)
    far = [n - 1 for n in shape]                                      # the single features sit in the last line: the ragged end of a tile
    out = []
    for name, pos in (("a single feature at index 0", 0), ("a single feature at the last index", L - 1)):
        m = np.zeros(shape, np.uint8); at = list(far); at[axis] = pos; m[tuple(at)] = 1
        out.append((name, m))
    if L > 1024:
        m = np.zeros(shape, np.uint8)
        sl = [slice(None)] * 3; sl[axis] = slice(1024, min(2048, L))
        m[tuple(sl)] = CO.random_mask(shape, 0.02, 5)[tuple(sl)]
        at = [0, 0, 0]; at[axis] = 1024; m[tuple(at)] = 1             # (at least one, also where the chunk is a single voxel)
        out.append(("features only inside the second 1024-voxel chunk", m))
        m = np.zeros(shape, np.uint8)
        for j, line in enumerate(lines):
            for k, seam in enumerate(range(1024, L, 1024)):
                at = list(line); at[axis] = seam - 1 if (j + k) % 2 == 0 else seam
                m[tuple(at)] = 1
        out.append(("a feature beside every chunk seam, alternating sides", m))
    m = np.zeros(shape, np.uint8)
    row = CO.random_mask((L,), 0.01, 7); row[L // 3] = 1
    m[lines[0]] = row
    out.append(("one line with features, the others without", m))
    return out


@gpu
@pytest.mark.parametrize("axis,shape", EDT_SHAPES)
def test_edt_long_axis_against_the_oracle(axis, shape):
    from gpu_util import Ops
    ops = Ops()
    L = shape[axis]
    pixdim = SPACINGS[1 + (axis + L) % 3]                             # anisotropic, and every one of the three is met
    for name, m in _edt_patterns(shape, axis):
        got = _check_edt(m, True, pixdim, ops, f"{shape} spacing {pixdim}: {name}")
        if len(_lines(shape, axis)) > 1:
            assert np.isfinite(got).all(), f"{shape}: {name}: the later passes reach every line"
    for i, (density, nonzero) in enumerate((d, nz) for d in (0.001, 0.3) for nz in (True, False)):
        m = CO.random_mask(shape, density if nonzero else 1.0 - density, 40 + i)
        _check_edt(m, nonzero, pixdim, ops, f"{shape} spacing {pixdim}: random, density {density}, nonzero {nonzero}")


@gpu
@pytest.mark.parametrize("shape", [s for a, s in EDT_SHAPES if a == 0])
def test_edt_x_pass_alone_leaves_a_featureless_line_infinite(shape):
    """a volume of one x line runs the x pass and nothing else: the line with features against the oracle, the one without +inf in every voxel"""
    from gpu_util import Ops
    ops = Ops()
    name, m = _edt_patterns(shape, 0)[-1]
    with_f, without = m[:, :1, :1], m[:, 1:2, :1] if shape[1] > 1 else m[:, :1, 1:2]
    assert with_f.any() and not without.any()
    _check_edt(with_f, True, SPACINGS[3], ops, f"{shape}: the line with features on its own")
    alone = _edt(without, True, SPACINGS[3], ops)
    assert np.isinf(alone).all() and (alone > 0).all(), f"{shape}: a line without features after the x pass"


@gpu
@pytest.mark.parametrize("axis,L", sorted({(a, s[a]) for a, s in EDT_SHAPES}))
def test_edt_single_feature_on_a_line_is_the_closed_form(axis, L):
    """a volume that is one line: d2 = fl(w d^2), d the integer distance to the feature -- one multiplication, no oracle behind it"""
    from gpu_util import Ops
    ops = Ops()
    shape = [1, 1, 1]; shape[axis] = L
    pixdim = SPACINGS[3]
    w = float(np.float64(pixdim[axis]) ** 2)
    for pos in (0, L - 1):
        m = np.zeros(shape, np.uint8); at = [0, 0, 0]; at[axis] = pos; m[tuple(at)] = 1
        got = _check_edt(m, True, pixdim, ops, f"{tuple(shape)}: a single feature at {pos}").reshape(-1)
        want = np.array([w * float(abs(i - pos)) ** 2 for i in range(L)])
        assert np.array_equal(got, want), f"{tuple(shape)}: a single feature at {pos}: {np.count_nonzero(got != want)} voxels differ from w d^2"


# ---- B. lesion coverage where the atomics fall back ---------------------------------------------------------------------------------------------------
# A case is a list of volume pairs; the condition below is on the case as a whole.  The two small shapes have 141 / 3780 groups of four and 3 / 60 runs of 256 voxels,
# fewer than 100 three-label runs could ever be found in one volume of either, so their cases hold as many seeds as the condition needs; the volumes themselves are
# the ones CO.random_mask(shape, d, seed) gives at d = 0.31 and 0.6.
OVERLAP_SEEDS = {(17, 1, 33): 96, (63, 40, 6): 40, (130, 70, 37): 2}
CHECKER = (48, 33, 21)
MIN_FALLBACKS = 100


@functools.lru_cache(maxsize=None)
def _overlap_cases():
    """[(name, roles, [(lt, nt, lp, np_), ..])]: roles says for which of the two tables (0: truth's, 1: the prediction's) the condition is asked"""
    cases = []
    for shape, seeds in OVERLAP_SEEDS.items():
        for d in (0.31, 0.6):
            pairs = [CO.label(CO.random_mask(shape, d, 2 * s), 1) + CO.label(CO.random_mask(shape, d, 2 * s + 1), 1) for s in range(seeds)]
            cases.append((f"random {shape} density {d}, {seeds} seeds", (0, 1), pairs))
    board = CO.label(CO.checkerboard(CHECKER), 1)
    ones = CO.label(np.ones(CHECKER, np.uint8), 1)
    rnd = CO.label(CO.random_mask(CHECKER, 0.31, 3), 1)
    assert board[1] == int(CO.checkerboard(CHECKER).sum()) and ones[1] == 1          # every voxel of the board is a lesion of its own
    cases.append(("checkerboard against all ones", (0,), [board + ones]))            # (the single label of the all-ones volume never mixes)
    cases.append(("all ones against the checkerboard", (1,), [ones + board]))
    cases.append(("checkerboard against random", (0, 1), [board + rnd]))
    cases.append(("random against the checkerboard", (0, 1), [rnd + board]))
    return cases


def _fallbacks(pairs, role):
    tot = np.zeros(3, np.int64)
    for lt, nt, lp, np_ in pairs:
        tot += SO.fallback_counts(lt, lp, nt) if role == 0 else SO.fallback_counts(lp, lt, np_)
    return tot


def _assert_fallbacks(name, roles, pairs):
    for role in roles:
        quads, runs, waves = _fallbacks(pairs, role)
        print(f"{name}, table {'tp'[role]}: {quads} mixed groups of four, {runs} runs of 256 with three labels or more, {waves} of them by the first label of each group")
        assert quads >= MIN_FALLBACKS and runs >= MIN_FALLBACKS and waves >= MIN_FALLBACKS, (name, role, quads, runs, waves)


def test_overlap_cases_reach_both_fallbacks():
    """no GPU: every case of test_lesion_overlap_where_the_atomics_fall_back sends at least 100 voxels out of cover_quad on their own and leaves at least 100 waves
    with a third label for wave_count's per-lane path, for each table the case is about"""
    for name, roles, pairs in _overlap_cases():
        _assert_fallbacks(name, roles, pairs)
    lt, nt, lp, np_ = _stray_labels()
    assert nt >= 100 and np_ >= 100
    for vol, n in ((lt, nt), (lp, np_)):
        stray = (vol < 0) | (vol > n)
        assert stray.sum() >= 200 and {int(v) for v in np.unique(vol[stray])} == {n + 5, 2 ** 31 - 1, -1, -12345}


def _overlap_raw(ops, lt_ptr, nt, lp_ptr, np_, shape):
    """unet_vol_lesion_overlap with the two tables as slices of one tensor -> (cover_t, cover_p); the words around them must survive"""
    import torch
    big = torch.full((3 * GUARD + nt + np_,), SENT_I, dtype=torch.int64, device="cuda")
    t0, p0 = GUARD, 2 * GUARD + nt
    ops.ck(ops.lib.unet_vol_lesion_overlap(ops.h, lt_ptr, nt, lp_ptr, np_, *shape, big.data_ptr() + 8 * t0, big.data_ptr() + 8 * p0, ops.s), "vol_lesion_overlap")
    out = big.cpu().numpy()
    guard = np.ones(out.size, bool); guard[t0:t0 + nt] = False; guard[p0:p0 + np_] = False
    assert (out[guard] == SENT_I).all(), f"unet_vol_lesion_overlap wrote outside its tables: words {np.nonzero(guard & (out != SENT_I))[0][:8]}"
    return out[t0:t0 + nt], out[p0:p0 + np_]


def _check_overlap(ops, lt, nt, lp, np_, what, shifted=False):
    import torch
    from covidseg_amd import volume as V
    want_t, want_p = SO.cover_tables(lt, nt, lp, np_)
    a, b = _labels_dev(lt), _labels_dev(lp)
    for how, (got_t, got_p) in (("wrapper", V.lesion_overlap_device(a, nt, b, np_, lt.shape)), ("raw", _overlap_raw(ops, a.data_ptr(), nt, b.data_ptr(), np_, lt.shape))):
        assert got_t.dtype == np.int64 and np.array_equal(got_t, want_t), f"{what} ({how}): cover_t differs in {np.count_nonzero(got_t != want_t)} of {nt} rows"
        assert got_p.dtype == np.int64 and np.array_equal(got_p, want_p), f"{what} ({how}): cover_p differs in {np.count_nonzero(got_p != want_p)} of {np_} rows"
    if shifted:                                                       # label volumes that start 4 bytes past a 16-byte boundary: the element-wise reads
        a4, b4 = torch.zeros(a.numel() + 8, dtype=torch.int32, device="cuda"), torch.zeros(b.numel() + 8, dtype=torch.int32, device="cuda")
        a4[1:1 + a.numel()] = a; b4[1:1 + b.numel()] = b
        got_t, got_p = _overlap_raw(ops, a4.data_ptr() + 4, nt, b4.data_ptr() + 4, np_, lt.shape)
        assert np.array_equal(got_t, want_t) and np.array_equal(got_p, want_p), f"{what}: label volumes off the 16-byte boundary"
    return want_t, want_p


@gpu
@pytest.mark.parametrize("case", range(10))
def test_lesion_overlap_where_the_atomics_fall_back(case):
    from gpu_util import Ops
    ops = Ops()
    name, roles, pairs = _overlap_cases()[case]
    _assert_fallbacks(name, roles, pairs)
    for i, (lt, nt, lp, np_) in enumerate(pairs):
        want_t, want_p = _check_overlap(ops, lt, nt, lp, np_, f"{name} [{i}]", shifted=i == 0)
        if name == "checkerboard against all ones":
            assert (want_t == 1).all() and want_p.tolist() == [nt]
    assert len(_overlap_cases()) == 10


@functools.lru_cache(maxsize=None)
def _stray_labels():
    shape = (63, 40, 6)
    lt, nt = CO.label(CO.random_mask(shape, 0.31, 0), 1)
    lp, np_ = CO.label(CO.random_mask(shape, 0.31, 1), 1)
    rng = np.random.default_rng(11)
    out = []
    for vol, n in ((lt, nt), (lp, np_)):
        flat = vol.reshape(-1).copy()
        where = rng.choice(flat.size, 400, replace=False)
        flat[where] = np.resize(np.array([n + 5, 2 ** 31 - 1, -1, -12345], np.int64), 400).astype(np.int32)
        out += [flat.reshape(shape), n]
    return tuple(out)


@gpu
def test_lesion_overlap_ignores_labels_outside_the_tables():
    """a label outside 1..n counts for nothing and addresses nothing (the tables lie between sentinels), and still marks the voxel for the partner's table"""
    from gpu_util import Ops
    lt, nt, lp, np_ = _stray_labels()
    want_t, want_p = _check_overlap(Ops(), lt, nt, lp, np_, "labels outside 1..n", shifted=True)
    clean_t, clean_p = SO.cover_tables(np.where((lt < 1) | (lt > nt), 0, lt), nt, np.where((lp < 1) | (lp > np_), 0, lp), np_)
    assert want_t.sum() > clean_t.sum() and want_p.sum() > clean_p.sum(), "the stray labels of one volume mark voxels of the other's lesions in this case"


# ---- C. surface distances into a short buffer ----------------------------------------------------------------------------------------------------------
SD_SHAPES = [(63, 40, 6), (17, 1, 33), (130, 70, 37)]


@functools.lru_cache(maxsize=None)
def _sd_case(shape):
    """(surface uint8 [X, Y, Z], d2 float64 [X, Y, Z]: the squared distance to ANOTHER mask's surface, by the line oracle)"""
    if min(shape) > 1:
        a, b = CO.ellipsoids(shape, 5, 0.0, 2), CO.ellipsoids(shape, 5, 0.0, 3)
    else:
        a, b = CO.random_mask(shape, 0.5, 2), CO.random_mask(shape, 0.2, 3)
    surf = SO.surface(a, 1)
    d2 = SO.edt_sq_lines(SO.surface(b, 1), True, SPACINGS[1])
    assert surf.sum() >= 64 and np.isfinite(d2).all() and (d2[surf != 0] > 0).any()
    return surf, d2


def _sd(ops, surf_ptr, d2_dev, shape, capacity, with_buffer=True):
    """unet_vol_surface_distances through ctypes -> (count, max d2, sum, the bits of the sum, what was gathered); the words behind gathered[capacity] must survive"""
    import torch
    res = torch.full((3,), SENT_I, dtype=torch.int64, device="cuda")
    ws = torch.empty(32768, dtype=torch.uint8, device="cuda")
    buf = torch.full((capacity + GUARD,), SENT, dtype=torch.float64, device="cuda")
    ops.ck(ops.lib.unet_vol_surface_distances(ops.h, surf_ptr, d2_dev.data_ptr(), *shape, res.data_ptr(), buf.data_ptr() if with_buffer else None, capacity, ws.data_ptr(),
                                              ws.numel(), ops.s), "vol_surface_distances")
    r, out = res.cpu().numpy(), buf.cpu().numpy()
    assert (out[capacity:] == SENT).all(), f"unet_vol_surface_distances wrote behind gathered[{capacity}]"
    written = out[:capacity][out[:capacity] != SENT]
    if not with_buffer:
        assert (out == SENT).all()
    return int(r[0]), float(r[1:2].view(np.float64)[0]), float(r[2:3].view(np.float64)[0]), int(r[2]), written


def _sub_multiset(part, whole):
    vp, cp = np.unique(part, return_counts=True)
    vw, cw = np.unique(whole, return_counts=True)
    at = np.searchsorted(vw, vp)
    return bool((at < len(vw)).all() and (vw[np.minimum(at, len(vw) - 1)] == vp).all() and (cp <= cw[np.minimum(at, len(vw) - 1)]).all())


@gpu
@pytest.mark.parametrize("shape", SD_SHAPES)
def test_surface_distances_short_buffer_no_buffer_and_unaligned_surface(shape):
    import torch
    from gpu_util import Ops
    from covidseg_amd import volume as V
    ops = Ops()
    surf, d2 = _sd_case(shape)
    N = surf.size
    vals = d2[surf != 0]
    count, d2max, ref_sum = int(vals.size), float(vals.max()), math.fsum(np.sqrt(vals))
    sd, dd = _bytes_dev(surf), torch.from_numpy(d2.reshape(-1, order="F").copy()).cuda()
    assert sd.data_ptr() % 16 == 0

    full = _sd(ops, sd.data_ptr(), dd, shape, count)
    assert full[0] == count and full[1] == d2max and np.array_equal(np.sort(full[4]), np.sort(vals)), f"{shape}: capacity = count"
    chain = SO.sum_chain(N)
    print(f"{shape}: {count} surface voxels, sum {full[2]!r} against {ref_sum!r}: {abs(full[2] - ref_sum) / (ULP * ref_sum):.2f} units of 2^-53, allowed {chain + 1}")
    assert abs(full[2] - ref_sum) <= (chain + 1) * ULP * ref_sum
    assert _sd(ops, sd.data_ptr(), dd, shape, count)[:4] == full[:4], f"{shape}: two runs give the same bits"

    for cap in (count // 2, 1):
        got = _sd(ops, sd.data_ptr(), dd, shape, cap)
        assert got[:4] == full[:4], f"{shape}: capacity {cap} of {count} changes the reductions: {got[:4]} against {full[:4]}"
        assert got[4].size == cap and _sub_multiset(got[4], vals), f"{shape}: capacity {cap}: {got[4].size} values written, or not from the surface"
    none = _sd(ops, sd.data_ptr(), dd, shape, 0, with_buffer=False)
    assert none[:4] == full[:4] and none[4].size == 0, f"{shape}: capacity 0 without a buffer"

    for cap in (count, count // 2, 1, 0):                             # the wrapper: min(count, capacity) values come back
        c, mx, sm, g = V.surface_distances_device(sd, dd, shape, cap)
        g = g.cpu().numpy()
        assert (c, mx) == (count, d2max) and np.float64(sm).view(np.int64) == full[3] and g.size == cap and _sub_multiset(g, vals), f"{shape}: wrapper, capacity {cap}"

    off = torch.zeros(N + 32, dtype=torch.uint8, device="cuda")       # the same surface one byte past a 16-byte boundary: element-wise reads
    off[1:1 + N] = sd
    assert (off.data_ptr() + 1) % 16 == 1
    shifted = _sd(ops, off.data_ptr() + 1, dd, shape, count)
    assert shifted[:4] == full[:4] and np.array_equal(np.sort(shifted[4]), np.sort(vals)), f"{shape}: unaligned surface: {shifted[:4]} against {full[:4]}"
    half = _sd(ops, off.data_ptr() + 1, dd, shape, count // 2)
    assert half[:4] == full[:4] and half[4].size == count // 2 and _sub_multiset(half[4], vals)

    far = _sd(ops, sd.data_ptr(), torch.full((N,), INF, dtype=torch.float64, device="cuda"), shape, count)
    assert far[0] == count and far[1] == INF and far[2] == INF and (far[4] == INF).all() and far[4].size == count, f"{shape}: d2 = +inf everywhere"


# ---- D. paste-back beyond one launch ------------------------------------------------------------------------------------------------------------------
PASTE_N, PASTE_D, PASTE_S, PASTE_CHUNK = 130, 16, 32, 64
SEAM_SLICES = (63, 64, 127, 128, 129)


def _paste_rects():
    """int32 [n, 2, 4]: per slice both lungs apart (kind 0), overlapping (1) or one of them absent (2); every eighth slice has none (3)"""
    rng = np.random.default_rng(21)
    S = PASTE_S
    rects, kinds = np.zeros((PASTE_N, 2, 4), np.int32), np.zeros(PASTE_N, np.int64)
    for i in range(PASTE_N):
        kinds[i] = 3 if i % 8 == 7 else i % 3
        if kinds[i] == 3:
            continue
        ys = rng.integers(0, 11, 2); hs = [rng.integers(12, S - y + 1) for y in ys]          # (any two of them share rows)
        if kinds[i] == 1:
            x1 = rng.integers(0, 9); w1 = rng.integers(12, 19); x2 = x1 + rng.integers(2, 9); w2 = rng.integers(8, S - x2 + 1)
        else:
            x1 = rng.integers(0, 7); w1 = rng.integers(4, 10); x2 = rng.integers(16, 23); w2 = rng.integers(4, S - x2 + 1)
        rects[i] = [[x1, ys[0], w1, hs[0]], [x2, ys[1], w2, hs[1]]]
        if kinds[i] == 2:
            rects[i, (i // 3) % 2, 2] = 0
    return rects, kinds


def test_paste_rects_hold_every_kind_in_every_chunk():
    """no GPU: the rectangles stay on the canvas, overlap or not as their kind says, and each full chunk of 64 slices has all four kinds"""
    rects, kinds = _paste_rects()
    x, y, w, h = (rects[..., k].astype(np.int64) for k in range(4))
    assert (x >= 0).all() and (y >= 0).all() and (h[kinds != 3] > 0).all() and (x + w <= PASTE_S).all() and (y + h <= PASTE_S).all()
    apart = x[:, 0] + w[:, 0] <= x[:, 1]
    meet = (x[:, 1] < x[:, 0] + w[:, 0]) & (np.maximum(y[:, 0], y[:, 1]) < np.minimum(y[:, 0] + h[:, 0], y[:, 1] + h[:, 1]))
    assert apart[kinds == 0].all() and (w[kinds == 0] > 0).all() and meet[kinds == 1].all() and ((w[kinds == 2] > 0).sum(axis=1) == 1).all() and not w[kinds == 3].any()
    for c0 in range(0, PASTE_N - PASTE_CHUNK + 1, PASTE_CHUNK):
        assert set(kinds[c0:c0 + PASTE_CHUNK]) == {0, 1, 2, 3}, c0
        assert {int(np.argmin(w[i])) for i in range(c0, c0 + PASTE_CHUNK) if kinds[i] == 2} == {0, 1}, "either lung is the absent one"
    assert PASTE_N > 2 * PASTE_CHUNK and (kinds[2 * PASTE_CHUNK:] != 3).all()


@gpu
def test_paste_back_over_three_launches():
    import torch
    from gpu_util import Ops
    from covidseg_amd import volume as V
    rects, _ = _paste_rects()
    prob = synthetic_prob(PASTE_N, PASTE_D, 4)
    dev = torch.from_numpy(prob).cuda()
    want = VO.paste_back(prob, rects, PASTE_S)
    got = V.paste_back(dev, rects[:, 0], rects[:, 1], PASTE_S).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert len({want[i].tobytes() for i in range(PASTE_N)}) == PASTE_N, "no two slices of the reference are equal: a slice pasted from another one's inputs shows"
    seams = {i: int(np.count_nonzero(got[i] != want[i])) for i in SEAM_SLICES}
    wrong = [i for i in range(PASTE_N) if not np.array_equal(got[i], want[i])]
    assert not any(seams.values()) and not wrong, f"pixels that differ in the slices beside the launch seams: {seams}; slices that differ at all: {wrong}"
    assert np.array_equal(got, want)

    ops = Ops()                                                       # a rectangle that leaves the canvas, in the second launch's slices: refused before any launch
    bad = rects.copy(); bad[100, 1] = (PASTE_S - 4, 0, 5, 8)
    canvas = torch.full((PASTE_N, PASTE_S, PASTE_S), SENT, dtype=torch.float32, device="cuda")
    r = np.ascontiguousarray(bad.reshape(PASTE_N, 8))
    assert ops.lib.unet_vol_paste_back(ops.h, dev.data_ptr(), PASTE_N, PASTE_D, r.ctypes.data, canvas.data_ptr(), PASTE_S, ops.s) == E_SHAPE
    assert "slice 100" in ops.ctx.last_error()
    torch.cuda.synchronize()
    assert bool((canvas == SENT).all()), "a refused paste-back wrote to the canvas"
    with pytest.raises(Exception, match="slice 100"):
        V.paste_back(dev, bad[:, 0], bad[:, 1], PASTE_S)

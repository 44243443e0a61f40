"""-m gpu: the paths of the persistent two-half conv3x3 schedule (csrc/kernels_conv_pp.hip) that test_gpu_conv_pp.py does not enter, through the C ABI and against
torch-CPU / numpy float64: a strided output (the skip half of a concat buffer; conv_h2_kernel too), the border-class bias table of a folded BatchNorm, the epilogue
statistics in the default and the deterministic mode under a bound derived from the tile walk, uneven trip counts of the two halves of a workgroup, an output span of
2 GiB, the one-shot K-slice arm across a launch this schedule takes, and the schedule inside the training programs at a small size (CONV_PP = 2).

Common criterion of a value comparison: rel-L2 < 2e-5 against float64, and -- wherever no ReLU follows -- the per-element bound of the h2 arithmetic (gpu_util.elem_ratio <= 1)."""
import numpy as np
import pytest
import torch

from gpu_util import cu_count
from oracle import unet_oracle as O
from test_gpu_conv_pp import PPOps, T64

pytestmark = pytest.mark.gpu
TOL = 2e-5
U = 2.0 ** -24                                 # the fp32 unit round-off
C = 32                                         # the schedule's channel counts: K = M = 32


class ModeOps(PPOps):
    """PPOps on a context with any set of options (private = a context of its own: the deterministic cases)"""
    def __init__(self, options, private=False):
        from gpu_util import Ops
        from covidseg_amd import _lib
        self.base = Ops()
        self.lib = self.base.lib
        self.ctx = _lib.Context.get(torch.cuda.current_device(), dict(options), private=private)
        self.h = self.ctx.handle
        self.d, self.z, self.wws = self.base.d, self.base.z, self.base.wws


@pytest.fixture(scope="module")
def pp():
    return PPOps(2)


@pytest.fixture(scope="module")
def h2():
    return PPOps(0)


def pp_tile_walk(cu, n, h, w):
    """The tiles every half-workgroup of conv_pp_kernel takes, transcribed from the kernel: grid = cu & ~7 workgroups, XCD b % 8 owns the tpx = ceil(total / 8) tiles from
    xcd * tpx on, its 2 * (grid / 8) half-workgroups (slot 2 * (b / 8) + half) take them round robin; a half finds its next tile with `advance` (the slot count decomposed
    into a column, row and image step once).  Returns the number of tiles per half-workgroup; asserts that the positions `advance` produces are the tiles of the round robin
    and that every tile is taken exactly once."""
    tiles_x, tiles_y = (w + 31) // 32, (h + 7) // 8
    total = tiles_x * tiles_y * n
    grid = cu & ~7
    per = grid >> 3; slots = 2 * per
    tpx = (total + 7) >> 3; iters = (tpx + slots - 1) // slots
    d_x = (slots % tiles_x) * 32; d_y = ((slots // tiles_x) % tiles_y) * 8; d_n = slots // (tiles_x * tiles_y)
    seen = np.zeros(total, np.int64); counts = []
    for b in range(grid):
        xcd, j = b & 7, b >> 3
        t_beg = xcd * tpx; t_end = min(t_beg + tpx, total)
        for half in (0, 1):
            t0 = t_beg + 2 * j + half
            t2 = t0 // tiles_x
            pn, py, px = t2 // tiles_y, (t2 % tiles_y) * 8, (t0 % tiles_x) * 32
            cnt = 0
            for it in range(iters):
                t = t0 + it * slots
                if t < t_end:
                    assert (pn * tiles_y + py // 8) * tiles_x + px // 32 == t, (b, half, it)
                    seen[t] += 1; cnt += 1
                px += d_x
                if px >= tiles_x * 32:
                    px -= tiles_x * 32; py += 8
                py += d_y
                if py >= tiles_y * 8:
                    py -= tiles_y * 8; pn += 1
                pn += d_n
            counts.append(cnt)
    assert (seen == 1).all()
    return counts


def stats_chain(cu, n, h, w):
    """L of the statistics bound: the largest number of values one lane adds into one component of its st1 over the launch.  A wave owns 2 rows of an 8 x 32 tile; per row
    it issues 4 line stores (8 pixels x 32 channels each), and a lane adds the ONE float4 it stores -- one value per component -- behind each of them (columns past the
    image add an exact 0): 8 additions per tile, over every tile of its half-workgroup.  L = 8 * (most tiles of a half-workgroup)."""
    return 8 * max(pp_tile_walk(cu, n, h, w))


def check_pp_stats(sn, yv, L, what):
    """|dev1 - S1| <= (L + 12) u sum |y_c|,  |dev2 - S2| <= (L + 13) u sum y_c^2  per channel, S from the DOWNLOADED y (the conv's own error is not in it).
    The fp32 chain of one value: L additions in a lane, 3 shuffle folds, the 8-wave fold (8 additions from 0), then exact (double atomics / window sums): L + 11 roundings,
    one to spare; a square enters through an fma (no rounding of its own), one more to spare."""
    y2 = np.asarray(yv, np.float64).reshape(-1, C)
    S1, S2, A1 = y2.sum(0), (y2 * y2).sum(0), np.abs(y2).sum(0)
    e1, e2 = np.abs(sn[:C] - S1), np.abs(sn[C:] - S2)
    b1, b2 = (L + 12) * U * A1, (L + 13) * U * S2
    r1 = float(np.max(np.where(e1 == 0, 0.0, e1 / (b1 + 1e-300)))); r2 = float(np.max(np.where(e2 == 0, 0.0, e2 / (b2 + 1e-300))))
    print(f"pp-stats {what} L={L} worst |dev-S|/bound: sums {r1:.3g} squares {r2:.3g}; worst |dev-S| {e1.max():.3g} (bound there {b1[np.argmax(e1)]:.3g}) / {e2.max():.3g} ({b2[np.argmax(e2)]:.3g})")
    assert (e1 <= b1).all() and (e2 <= b2).all(), (what, r1, r2)
    return r1, r2


def sign_words(pos):
    """bool [n,h,w,32] -> the u64 words [n][h][w / 8][1][4] of the documented sign-bit layout (include/unet_hip.h: unet_request_relu_bits)"""
    n, h, w, _ = pos.shape
    p = pos.reshape(n, h, w // 8, 8, 1, 8, 4)
    words = np.zeros((n, h, w // 8, 1, 4), np.uint64)
    for a in range(8):
        for q in range(8):
            words |= p[:, :, :, a, :, q, :].astype(np.uint64) << np.uint64(a * 8 + q)
    return words


def abs_fwd(x, k):
    """A1 of the forward: sum |x| |w| per output element (float64, zero padding)"""
    import torch.nn.functional as F
    xa = torch.as_tensor(np.abs(np.asarray(x, np.float64))).permute(0, 3, 1, 2); ka = torch.as_tensor(np.abs(np.asarray(k, np.float64))).permute(3, 2, 0, 1)
    return F.conv2d(xa, ka, padding=1).permute(0, 2, 3, 1).numpy()


def abs_dgrad(dy, k):
    import torch.nn.functional as F
    da = torch.as_tensor(np.abs(np.asarray(dy, np.float64))).permute(0, 3, 1, 2); ka = torch.as_tensor(np.abs(np.asarray(k, np.float64))).permute(3, 2, 0, 1)
    return F.conv2d(da, ka.flip(2, 3).transpose(0, 1), padding=1).permute(0, 2, 3, 1).numpy()


def conv64(x, k, b):
    """float64 conv3x3 + bias, no activation"""
    return O.conv3x3_bias_relu(T64(x), T64(k), T64(b), relu=False).numpy()


def fwd_ld(ops, x, k, b, yptr, ldy, n, h, w, act, algo=0):
    return ops.lib.unet_conv3x3_fwd_ld(ops.h, x.data_ptr(), k.data_ptr(), b.data_ptr(), yptr, ldy, n, h, w, C, C, act, algo, ops.wws(C, C), ops.s)


# ---- item 2: a strided output -------------------------------------------------------------------------------------------------------------------------------
SLACK = 4096
PAT0 = 0x3F000000                               # counter + this, viewed as float: distinct finite values from 0.5 up, no NaN pattern


@pytest.mark.parametrize("conv_pp", [2, 0])
@pytest.mark.parametrize("ldy", [64, 36])
@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 33, 70), (2, 7, 100), (1, 9, 264)])
def test_strided_output_writes_its_channel_slice_and_nothing_else(pp, h2, shape, ldy, conv_pp):
    """32 -> 32 into the LAST 32 channels of an [n,h,w,ldy] buffer (ldy = 64: c1b into the skip half of its concat; 36: the smallest legal stride above M), on the persistent
    schedule and on conv_h2_kernel.  The buffer (and 4096 floats behind its last pixel) is pre-filled with a distinct bit pattern per element: the slice meets the common
    criterion, every other element keeps its bits.  Then statistics and (w % 8 == 0) sign bits armed on a strided launch: unet_bn_stats(ldx = ldy) returns the sums of the
    slice, the bits are [y > 0] in the documented layout."""
    from gpu_util import relerr, conv_abs_sums, elem_ratio
    ops = pp if conv_pp else h2
    assert ops.lib.unet_ctx_get_option(ops.h, 13) == conv_pp
    n, h, w = shape
    c0 = ldy - C
    rng = np.random.default_rng(n * 1000 + h * 10 + w + ldy)
    x = rng.standard_normal((n, h, w, C)).astype(np.float32); k = (rng.standard_normal((3, 3, C, C)) * 0.2).astype(np.float32); b = rng.standard_normal(C).astype(np.float32)
    xd, kd, bd = ops.d(x), ops.d(k), ops.d(b)
    pre = conv64(x, k, b)
    a1 = conv_abs_sums(x, k, np.zeros((n, h, w, C), np.float32), with_floor=False)["y_a1"] + np.abs(b)[None, None, None, :]
    npix = n * h * w
    pat = np.arange(npix * ldy + SLACK, dtype=np.int32) + PAT0
    inside = np.zeros(npix * ldy + SLACK, bool)
    inside[:npix * ldy].reshape(npix, ldy)[:, c0:] = True

    def run(act, arm):
        buf = torch.from_numpy(pat.copy()).cuda()
        bits = None
        if arm:
            if w % 8 == 0:
                bits = torch.full((npix * C // 64,), -1, dtype=torch.int64, device="cuda")
                ops.ck(ops.lib.unet_request_relu_bits(ops.h, bits.data_ptr()), "arm bits")
            ops.ck(ops.lib.unet_request_bn_stats(ops.h, C), "arm stats")
        ops.ck(fwd_ld(ops, xd, kd, bd, buf.data_ptr() + 4 * c0, ldy, n, h, w, act), "conv fwd, strided")
        sums = None
        if arm:
            sums = ops.z(2 * C, dtype=torch.float64)
            ops.ck(ops.lib.unet_bn_stats(ops.h, buf.data_ptr() + 4 * c0, ldy, sums.data_ptr(), npix, C, ops.s), "bn stats, ldx = ldy")
            sums = sums.cpu().numpy()
        got = buf.cpu().numpy()
        assert np.array_equal(got[~inside], pat[~inside]), f"{np.count_nonzero(got[~inside] != pat[~inside])} elements outside the slice changed"
        y = got[:npix * ldy].reshape(n, h, w, ldy)[..., c0:].copy().view(np.float32)
        return y, sums, bits

    y, _, _ = run(1, False)
    assert relerr(y, np.maximum(pre, 0)) < TOL
    y, _, _ = run(0, False)
    r = elem_ratio(y, pre, a1)
    print(f"strided conv_pp={conv_pp} {shape} ldy={ldy}: elem_ratio {r:.3g}")
    assert relerr(y, pre) < TOL and r <= 1.0
    y, sums, bits = run(1, True)
    assert relerr(y, np.maximum(pre, 0)) < TOL
    yv = y.astype(np.float64)
    assert np.allclose(sums[:C], yv.sum((0, 1, 2)), rtol=1e-5, atol=1e-3) and np.allclose(sums[C:], (yv * yv).sum((0, 1, 2)), rtol=1e-5, atol=1e-3)
    if conv_pp:
        check_pp_stats(sums, yv, stats_chain(cu_count(), n, h, w), f"strided {shape} ldy={ldy}")
    if bits is not None:
        assert (bits.cpu().numpy().view(np.uint64).reshape(n, h, w // 8, 1, 4) == sign_words(yv > 0)).all()


def test_strided_entry_refuses_what_it_cannot_launch(pp):
    """unet_conv3x3_fwd_ld: ldy < cout or ldy % 4 != 0 -> UNET_E_ARG (-1); a launch outside the h2 family (the strict algorithms, cin = 1) -> UNET_E_STATE (-4); nothing written"""
    n, h, w = 1, 8, 8
    x = pp.z(n, h, w, C); k = pp.z(3, 3, C, C); b = pp.z(C)
    buf = torch.full((n * h * w * 64,), 7.0, device="cuda")
    for ldy in (28, 34, 0):
        assert fwd_ld(pp, x, k, b, buf.data_ptr(), ldy, n, h, w, 1) == -1, ldy
    assert fwd_ld(pp, x, k, b, buf.data_ptr(), 64, n, h, w, 1, algo=1) == -4
    assert pp.lib.unet_conv3x3_fwd_ld(pp.h, x.data_ptr(), k.data_ptr(), b.data_ptr(), buf.data_ptr(), 64, n, h, w, 1, C, 1, 0, pp.wws(C, C), pp.s) == -4
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


# ---- item 3: the border-class bias table ----------------------------------------------------------------------------------------------------------------------
def fold_ws(ops, n):
    return ops.z(int(ops.lib.unet_conv3x3_bnfold_ws_floats(n, C, C)))


@pytest.mark.parametrize("shape", [(3, 2, 33), (2, 16, 32), (1, 9, 264), (2, 7, 100), (2, 1, 40), (2, 5, 1)])
def test_border_class_bias_table_on_the_persistent_schedule(pp, h2, shape):
    """unet_conv3x3_bnfold_fwd 32 -> 32 with CONV_PP = 2 (MASK_BIAS_TAB in conv_pp_kernel) against float64 bn_apply -> zero-pad -> conv; the shift is large against the
    data, so a pixel that takes the bias row of a wrong border class is off by a multiple of its own magnitude.  Two-row, one-row and one-column images: first and last
    row / column coincide.

    Per-element bound: y = sum x (s w) + tab[class].  The product term carries the h2 bound EPS_SPLIT * A1 with A1 = sum |x| |s w|, plus u A1 for the fp32 product s w
    the image is split from.  The table entry b + sum_{taps inside} sum_c shift_c w is formed in fp32 (kernels_bnfold.hip): 8 fma per channel sub-slice, 2 pairwise
    additions, up to 9 taps, the bias: 20 roundings, and the epilogue's fma adds one: 22 u (|b| + T1) with one to spare, T1 = sum over the taps inside the image of
    |shift_c| |w|.  elem_ratio takes both as one A1-like array (EPS_SPLIT = 16 u)."""
    from gpu_util import relerr, conv_abs_sums, elem_ratio
    n, h, w = shape
    rng = np.random.default_rng(7 * h + w)
    x = (rng.standard_normal((n, h, w, C)) * rng.uniform(0.5, 2.0, C) + rng.uniform(-1.5, 1.5, C)).astype(np.float32)
    k = (rng.standard_normal((3, 3, C, C)) * np.sqrt(2.0 / (9 * C))).astype(np.float32); b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    scale = rng.uniform(0.4, 1.6, C).astype(np.float32); shift = (rng.uniform(4.0, 8.0, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    bnp = np.concatenate([scale, shift, np.zeros(2 * C, np.float32)])
    z64 = x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    pre = conv64(z64, k, b)
    zero = np.zeros((n, h, w, C), np.float32)
    a1 = conv_abs_sums(x, k.astype(np.float64) * scale.astype(np.float64)[None, None, :, None], zero, with_floor=False)["y_a1"]
    t1 = conv_abs_sums(np.broadcast_to(np.abs(shift), (1, h, w, C)), k, zero[:1], with_floor=False)["y_a1"]
    bound_a1 = a1 * (1.0 + 1.0 / 16.0) + (22.0 / 16.0) * (np.abs(b)[None, None, None, :] + t1)
    rowc = (np.arange(h) == 0).astype(int) | ((np.arange(h) == h - 1).astype(int) << 1)
    colc = (np.arange(w) == 0).astype(int) | ((np.arange(w) == w - 1).astype(int) << 1)
    cls = (rowc[:, None] << 2) | colc[None, :]                                             # the kernel's class index of pixel (py, px)
    assert cls.max() > 0 and (h > 1 or (rowc == 3).all()) and (w > 1 or (colc == 3).all())

    def run(ops, act, arm=False):
        y = ops.z(n, h, w, C)
        if arm:
            ops.ck(ops.lib.unet_request_bn_stats(ops.h, C), "arm stats")
        ops.ck(ops.lib.unet_conv3x3_bnfold_fwd(ops.h, ops.d(x).data_ptr(), ops.d(bnp).data_ptr(), ops.d(k).data_ptr(), ops.d(b).data_ptr(), y.data_ptr(), n, h, w, C, C, act, 0,
                                               fold_ws(ops, n).data_ptr(), ops.s), "fold fwd")
        sums = None
        if arm:
            sums = ops.z(2 * C, dtype=torch.float64)
            ops.ck(ops.lib.unet_bn_stats(ops.h, y.data_ptr(), C, sums.data_ptr(), n * h * w, C, ops.s), "bn stats")
            sums = sums.cpu().numpy()
        return y.cpu().numpy(), sums

    assert pp.lib.unet_ctx_get_option(pp.h, 13) == 2 and h2.lib.unet_ctx_get_option(h2.h, 13) == 0
    for act in (1, 0):
        want = np.maximum(pre, 0) if act else pre
        y, _ = run(pp, act)
        assert relerr(y, want) < TOL, act
        y0, _ = run(h2, act)
        assert relerr(y, y0) < 2e-6, act
        if act == 0:
            r = elem_ratio(y, want, bound_a1)
            worst = {}
            for c_ in np.unique(cls):
                sel = cls == c_
                worst[int(c_)] = elem_ratio(y[:, sel], want[:, sel], bound_a1[:, sel])
            print(f"bias table {shape}: elem_ratio {r:.3g}; per border class {({c_: round(v, 3) for c_, v in worst.items()})}")
            assert r <= 1.0 and max(worst.values()) <= 1.0, worst
    y, sums = run(pp, 1, arm=True)
    assert relerr(y, np.maximum(pre, 0)) < TOL
    check_pp_stats(sums, y, stats_chain(cu_count(), n, h, w), f"bias table {shape}")


# ---- items 4 and 5: shapes whose half-workgroups get different numbers of tiles -----------------------------------------------------------------------------------
def uneven_shape(kind):
    """(a) some half-workgroups get 1 tile and others 2; (b) some 4 and others 5, with tiles that overhang in x and in y -- the smallest batch at which the tile walk on
    THIS device's CU count says so (256 CUs: (7, 128, 160) and (12, 125, 340))."""
    cu = cu_count()
    h, w, want = ((128, 160, {1, 2}) if kind == "a" else (125, 340, {4, 5}))
    for n in range(1, 65):
        if set(pp_tile_walk(cu, n, h, w)) == want:
            return n, h, w
    pytest.fail(f"no batch size up to 64 gives half-workgroups {want} tiles at {h} x {w} on {cu} CUs")


_cases = {}


def uneven_case(kind):
    """inputs of one uneven shape (shared by the tests below, never modified): x, k, b (bias around 1 against a conv output of spread ~0.35: sum |y| is close to |sum y|)"""
    if kind not in _cases:
        n, h, w = uneven_shape(kind)
        counts = pp_tile_walk(cu_count(), n, h, w)
        assert set(counts) == ({1, 2} if kind == "a" else {4, 5})                          # the condition the case exists for, from the kernel's own walk
        if kind == "b":
            assert w % 32 and h % 8
        rng = np.random.default_rng(n + h + w)
        x = rng.standard_normal((n, h, w, C)).astype(np.float32); k = (rng.standard_normal((3, 3, C, C)) * 0.02).astype(np.float32)
        b = (1.0 + 0.1 * rng.standard_normal(C)).astype(np.float32)
        dy = (rng.standard_normal((n, h, w, C)) * 1e-6).astype(np.float32)
        _cases[kind] = dict(shape=(n, h, w), x=x, k=k, b=b, dy=dy, L=8 * max(counts), counts=counts)
    return _cases[kind]


@pytest.mark.parametrize("mode", ["default", "deterministic"])
@pytest.mark.parametrize("kind", ["a", "b"])
def test_epilogue_statistics_stay_within_the_bound_of_their_fp32_chain(kind, mode):
    """The (sum y, sum y^2) of an armed 32 -> 32 launch on the persistent schedule, default and deterministic mode, against float64 sums of the DOWNLOADED y under
    (L + 12) u sum |y| and (L + 13) u sum y^2 (check_pp_stats; L = 8 * tiles of the busiest half-workgroup: stats_chain).  Deterministic mode: two fresh contexts give
    the same bits in y and in the sums, and the fold does not read the tensor (it is poisoned between the conv and unet_bn_stats)."""
    cs = uneven_case(kind)
    n, h, w = cs["shape"]
    opts = {"conv_pp": 2} if mode == "default" else {"conv_pp": 2, "deterministic": 1}
    runs = []
    for rep in range(1 if mode == "default" else 2):
        ops = ModeOps(opts, private=mode != "default")
        try:
            assert ops.lib.unet_ctx_get_option(ops.h, 13) == 2 and ops.lib.unet_ctx_get_option(ops.h, 6) == (0 if mode == "default" else 1)
            y = ops.z(n, h, w, C); sums = ops.z(2 * C, dtype=torch.float64)
            ops.ck(ops.lib.unet_request_bn_stats(ops.h, C), "arm stats")
            ops.ck(ops.lib.unet_conv3x3_fwd(ops.h, ops.d(cs["x"]).data_ptr(), ops.d(cs["k"]).data_ptr(), ops.d(cs["b"]).data_ptr(), y.data_ptr(), n, h, w, C, C, 1, 0.0, 0, 0, ops.wws(C, C), ops.s), "conv")
            yv = y.cpu().numpy()
            if rep == 1:
                y.fill_(float("nan"))
            ops.ck(ops.lib.unet_bn_stats(ops.h, y.data_ptr(), C, sums.data_ptr(), n * h * w, C, ops.s), "fold")
            runs.append((yv, sums.cpu().numpy()))
        finally:
            if mode != "default":
                ops.ctx.close()
    yv, sn = runs[0]
    assert np.abs(yv.astype(np.float64).sum()) > 0.9 * np.abs(yv).astype(np.float64).sum()
    check_pp_stats(sn, yv, cs["L"], f"{mode} {cs['shape']} on {cu_count()} CUs")
    if mode != "default":
        assert np.array_equal(runs[0][0].view(np.int32), runs[1][0].view(np.int32))
        assert np.array_equal(runs[0][1].view(np.int64), runs[1][1].view(np.int64))          # (the second run's tensor was NaN when its sums were folded)


@pytest.mark.parametrize("kind", ["a", "b"])
def test_uneven_trip_counts_forward(pp, kind):
    """forward with bias, with and without ReLU, then statistics and (w % 8 == 0) sign bits, where the two halves of a workgroup and the workgroups of an XCD run different
    numbers of tiles (the pipeline's have_prev / have_cur / have_next states end at different iterations), (b) with overhanging tiles in x and y"""
    from gpu_util import relerr, elem_ratio
    cs = uneven_case(kind)
    n, h, w = cs["shape"]
    x, k, b = cs["x"], cs["k"], cs["b"]
    xd, kd, bd = pp.d(x), pp.d(k), pp.d(b)
    pre = conv64(x, k, b)
    a1 = abs_fwd(x, k) + np.abs(b)[None, None, None, :]
    for relu in (1, 0):
        y = pp.z(n, h, w, C)
        pp.ck(pp.lib.unet_conv3x3_fwd(pp.h, xd.data_ptr(), kd.data_ptr(), bd.data_ptr(), y.data_ptr(), n, h, w, C, C, relu, 0.0, 0, 0, pp.wws(C, C), pp.s), "conv fwd")
        assert relerr(y.cpu().numpy(), np.maximum(pre, 0) if relu else pre) < TOL
        if relu == 0:
            r = elem_ratio(y.cpu().numpy(), pre, a1)
            print(f"uneven forward {cs['shape']} tiles per half {sorted(set(cs['counts']))}: elem_ratio {r:.3g}")
            assert r <= 1.0
    y = pp.z(n, h, w, C); sums = pp.z(2 * C, dtype=torch.float64)
    bits = None
    if w % 8 == 0:
        bits = torch.full((n * h * w * C // 64,), -1, dtype=torch.int64, device="cuda")
        pp.ck(pp.lib.unet_request_relu_bits(pp.h, bits.data_ptr()), "arm bits")
    pp.ck(pp.lib.unet_request_bn_stats(pp.h, C), "arm stats")
    pp.ck(pp.lib.unet_conv3x3_fwd(pp.h, xd.data_ptr(), kd.data_ptr(), bd.data_ptr(), y.data_ptr(), n, h, w, C, C, 1, 0.0, 0, 0, pp.wws(C, C), pp.s), "conv fwd + stats")
    pp.ck(pp.lib.unet_bn_stats(pp.h, y.data_ptr(), C, sums.data_ptr(), n * h * w, C, pp.s), "bn stats")
    yv = y.cpu().numpy()
    assert relerr(yv, np.maximum(pre, 0)) < TOL
    check_pp_stats(sums.cpu().numpy(), yv, cs["L"], f"uneven forward {cs['shape']}")
    if bits is not None:
        assert (bits.cpu().numpy().view(np.uint64).reshape(n, h, w // 8, 1, 4) == sign_words(yv > 0)).all()


@pytest.mark.parametrize("kind", ["a", "b"])
def test_uneven_trip_counts_data_gradient(pp, h2, kind):
    """the plain and (w % 8 == 0) the bit-masked data gradient at the same shapes: against float64, the masked one equal in every bit to masking the plain one, and
    against conv_h2_kernel"""
    from gpu_util import relerr, elem_ratio
    cs = uneven_case(kind)
    n, h, w = cs["shape"]
    x, k, dy = cs["x"], cs["k"], cs["dy"]
    xt = T64(x).requires_grad_(True)
    O.conv3x3_bias_relu(xt, T64(k), torch.zeros(C, dtype=torch.float64), relu=False).backward(T64(dy))
    want = xt.grad.numpy()
    dyd, kd = pp.d(dy), pp.d(k)
    dx = pp.z(n, h, w, C)
    pp.ck(pp.lib.unet_conv3x3_bwd_data(pp.h, dyd.data_ptr(), kd.data_ptr(), None, 0, 0.0, 0, dx.data_ptr(), pp.wws(C, C), n, h, w, C, C, 0, pp.s), "dgrad")
    dxn = dx.cpu().numpy()
    r = elem_ratio(dxn, want, abs_dgrad(dy, k))
    print(f"uneven data gradient {cs['shape']}: elem_ratio {r:.3g}")
    assert relerr(dxn, want) < TOL and r <= 1.0
    if w % 8 == 0:
        bits = torch.from_numpy(sign_words(x > 0).view(np.int64).reshape(-1)).cuda()
        dxm = pp.z(n, h, w, C)
        pp.ck(pp.lib.unet_conv3x3_bwd_data(pp.h, dyd.data_ptr(), kd.data_ptr(), bits.data_ptr(), 9, 0.0, 0, dxm.data_ptr(), pp.wws(C, C), n, h, w, C, C, 0, pp.s), "dgrad bits")
        assert np.array_equal(dxm.cpu().numpy(), np.where(x > 0, dxn, np.float32(0)))
    dx0 = h2.z(n, h, w, C)
    h2.ck(h2.lib.unet_conv3x3_bwd_data(h2.h, dyd.data_ptr(), kd.data_ptr(), None, 0, 0.0, 0, dx0.data_ptr(), h2.wws(C, C), n, h, w, C, C, 0, h2.s), "dgrad h2")
    assert relerr(dxn, dx0.cpu().numpy()) < 2e-6


# ---- item 6: an output span of 2 GiB ------------------------------------------------------------------------------------------------------------------------------
def test_output_span_beyond_2_gib_with_a_strided_output():
    """n = 33, 512 x 512, 32 -> 32 into the upper half of a 64-channel buffer, CONV_PP = 1: the input (1.1 GiB) passes every 32-bit limit, the byte offset of an output row
    reaches 2^31 in image 32.  Images 0, 31, 32 against float64; the whole slice against CONV_PP = 0 per image; the lower half keeps its bit pattern."""
    from gpu_util import relerr, elem_ratio
    if torch.cuda.mem_get_info()[0] < (8 << 30):
        pytest.skip("needs 8 GiB of free device memory")
    n, h, w, ldy = 33, 512, 512, 64
    img = h * w * ldy
    assert (n - 1) * img * 4 >= 2 ** 31 > (n - 2) * img * 4 and n * h * w * C * 4 < 2 ** 31
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    x = torch.randn((n, h, w, C), device="cuda", generator=g)
    rng = np.random.default_rng(6)
    k = (rng.standard_normal((3, 3, C, C)) * 0.1).astype(np.float32); b = rng.standard_normal(C).astype(np.float32)
    outs = []
    for value in (1, 0):
        ops = PPOps(value)
        buf = torch.arange(n * img + SLACK, dtype=torch.int32, device="cuda")
        buf += PAT0
        ops.ck(fwd_ld(ops, x, ops.d(k), ops.d(b), buf.data_ptr() + 4 * C, ldy, n, h, w, 0), f"conv fwd, strided, conv_pp {value}")
        outs.append(buf)
    y1 = outs[0][:n * img].view(n, h, w, ldy); y0 = outs[1][:n * img].view(n, h, w, ldy)
    for i in (0, 31, 32):
        xi = x[i:i + 1].cpu().numpy()
        want = conv64(xi, k, b)
        got = y1[i:i + 1, :, :, C:].contiguous().view(torch.float32).cpu().numpy()
        r = elem_ratio(got, want, abs_fwd(xi, k) + np.abs(b)[None, None, None, :])
        print(f"2 GiB span, image {i}: rel-L2 {relerr(got, want):.3g} elem_ratio {r:.3g}")
        assert relerr(got, want) < TOL and r <= 1.0, i
    worst = 0.0
    for i in range(n):
        a = y1[i, :, :, C:].contiguous().view(torch.float32).double(); c = y0[i, :, :, C:].contiguous().view(torch.float32).double()
        worst = max(worst, float((a - c).norm() / c.norm()))
        pat = torch.arange(i * img, (i + 1) * img, dtype=torch.int32, device="cuda").add_(PAT0).view(h, w, ldy)[:, :, :C]
        assert torch.equal(y1[i, :, :, :C], pat) and torch.equal(y0[i, :, :, :C], pat), i
    print(f"2 GiB span: worst per-image rel-L2 between CONV_PP 1 and 0: {worst:.3g}")
    assert worst < 2e-6
    tail = torch.arange(n * img, n * img + SLACK, dtype=torch.int32, device="cuda").add_(PAT0)
    assert torch.equal(outs[0][n * img:], tail) and torch.equal(outs[1][n * img:], tail)
    del outs, y1, y0, x, buf
    torch.cuda.empty_cache()


# ---- item 7: the one-shot K-slice arm ---------------------------------------------------------------------------------------------------------------------------
def test_k_slice_arm_does_not_survive_a_launch_the_persistent_schedule_takes():
    """unet_allow_k_slices arms the NEXT launch.  When that launch is taken by the persistent schedule (a 32 -> 32 unet_conv3x3_bnfold_fwd, or the data gradient behind the
    head's stream), a later small 256 -> 256 launch on the same context must not slice its contraction: its output equals, in every bit, the same call on a fresh context
    that was never armed.  (That an armed 256 -> 256 launch itself DOES add in another order is asserted first: the comparison can see a surviving arm.)"""
    rng = np.random.default_rng(12)
    n, h, w = 2, 16, 32
    x = rng.standard_normal((n, h, w, C)).astype(np.float32); k = (rng.standard_normal((3, 3, C, C)) * 0.1).astype(np.float32); b = rng.standard_normal(C).astype(np.float32)
    bnp = np.concatenate([rng.uniform(0.5, 1.5, C), rng.standard_normal(C), np.zeros(2 * C)]).astype(np.float32)
    kh = rng.standard_normal(C).astype(np.float32)
    dzm = np.stack([(rng.standard_normal((n, h, w)) * 1e-7).astype(np.float32).view(np.uint32), rng.integers(0, 2 ** 32, (n, h, w), dtype=np.uint64).astype(np.uint32)], -1).reshape(-1).view(np.int32)
    D = 256
    xb = rng.standard_normal((1, 32, 32, D)).astype(np.float32); kb = (rng.standard_normal((3, 3, D, D)) * 0.02).astype(np.float32); bb = rng.standard_normal(D).astype(np.float32)
    bnpb = np.concatenate([rng.uniform(0.5, 1.5, D), rng.standard_normal(D), np.zeros(2 * D)]).astype(np.float32)

    def big(ops):
        y = ops.z(1, 32, 32, D)
        ws = ops.z(int(ops.lib.unet_conv3x3_bnfold_ws_floats(1, D, D)))
        ops.ck(ops.lib.unet_conv3x3_bnfold_fwd(ops.h, ops.d(xb).data_ptr(), ops.d(bnpb).data_ptr(), ops.d(kb).data_ptr(), ops.d(bb).data_ptr(), y.data_ptr(), 1, 32, 32, D, D, 1, 0,
                                               ws.data_ptr(), ops.s), "fold fwd 256 -> 256")
        return y.cpu().numpy().view(np.int32)

    def pp_fold(ops):
        y = ops.z(n, h, w, C)
        ops.ck(ops.lib.unet_conv3x3_bnfold_fwd(ops.h, ops.d(x).data_ptr(), ops.d(bnp).data_ptr(), ops.d(k).data_ptr(), ops.d(b).data_ptr(), y.data_ptr(), n, h, w, C, C, 1, 0,
                                               fold_ws(ops, n).data_ptr(), ops.s), "fold fwd 32 -> 32")

    def pp_dzm(ops):
        dx = ops.z(n, h, w, C)
        ops.ck(ops.lib.unet_conv3x3_bwd_data_dzm(ops.h, torch.from_numpy(dzm).cuda().data_ptr(), ops.d(k).data_ptr(), ops.d(kh).data_ptr(), None, dx.data_ptr(), ops.wws(C, C), n, h, w, C, ops.s),
               "dgrad of the head's stream")

    fresh = ModeOps({"conv_pp": 2}, private=True)
    armed = ModeOps({"conv_pp": 2}, private=True)
    try:
        want = big(fresh)
        armed.ck(armed.lib.unet_allow_k_slices(armed.h), "arm")
        assert not np.array_equal(big(armed), want)                    # armed: four K slices added in a second pass -- other bits
        assert np.array_equal(big(armed), want)                        # consumed
        for taken_by_pp in (pp_fold, pp_dzm):
            armed.ck(armed.lib.unet_allow_k_slices(armed.h), "arm")
            taken_by_pp(armed)
            assert np.array_equal(big(armed), want), taken_by_pp.__name__
    finally:
        fresh.ctx.close(); armed.ctx.close()


# ---- item 8: the schedule inside the programs at a small size ---------------------------------------------------------------------------------------------------
MODEL_SEED = 49          # (see test_programs_with_the_persistent_schedule_at_a_small_size)


def model_case():
    if "model" not in _cases:
        h, w_, n = 48, 80, 3
        rng = np.random.default_rng(MODEL_SEED)
        wts = O.init_weights(seed=MODEL_SEED)
        for k in wts:                                                   # non-trivial biases / BN params (test_gpu_model.py: test_live_oracle_all_grads_and_taps)
            if k.endswith("/bias") or k.endswith("/beta"):
                wts[k] = (rng.standard_normal(wts[k].shape) * 0.1).astype(np.float32)
            if k.endswith("/gamma"):
                wts[k] = rng.uniform(0.5, 1.5, wts[k].shape).astype(np.float32)
        x = rng.random((n, h, w_, 1)).astype(np.float32)
        y = (np.round(rng.random((n, h, w_, 1)) ** 4 * 255) / 255).astype(np.float32)
        r = O.loss_and_grads(wts, x, y, dtype=torch.float64, want_acts=True)
        _cases["model"] = (wts, x, y, r)
    return _cases["model"]


@pytest.mark.parametrize("extra", [{}, {"head_fused": 0}], ids=["default", "head_fused=0"])
def test_programs_with_the_persistent_schedule_at_a_small_size(extra):
    """HipUNet(48, 80), batch 3, CONV_PP = 2: c1b forward, its data gradient and the data gradient behind the head's stream are conv_pp_kernel launches inside the
    programs (head_fused = 0: c9b's forward too).  Loss, taps and all gradients against the float64 oracle with the tolerances of test_live_oracle_all_grads_and_taps, and
    against the same engine with CONV_PP = 0 (loss 1e-6, gradients rel-L2 1e-5).

    The second comparison means something only where the two engines take the same ReLU decisions: a pre-activation that the two schedules round to different sides of 0
    is a discontinuity of the gradient, not an arithmetic error (test_gpu_model.py).  Measured over the data seeds 48 .. 53 (both option sets alike): seeds 49, 50, 51, 53 --
    no decision differs among the 1.66 M, gradient distances 3e-8 .. 1.4e-6; seed 48 -- ONE element of c9a differs, every gradient moves by 2e-3 .. 4.2e-3 (c1a/kernel
    2.84e-3), and the float64 oracle evaluated on the two sign patterns differs by the same 2.84e-3; seed 52 -- two elements (c3a, c8a), 6e-3.  So the data seed is 49, and
    the test asserts that the decisions agree before it holds the gradients to 1e-5."""
    from test_gpu_model import make, relerr
    from covidseg_amd import _lib
    wts, x, y, r = model_case()
    n = x.shape[0]
    eng = make(48, 80, dropout_rate=0.0, options={"conv_pp": 2, **extra})
    assert eng.lib.unet_ctx_get_option(eng.ctx.handle, _lib.OPTIONS["conv_pp"]) == 2
    eng.set_weights(wts)
    ld = eng.forward_backward(x, y).cpu().numpy()
    assert abs(ld[0] - r["loss"]) < 1e-5 and abs(ld[1] - r["dice"]) < 1e-5
    for name in ("c1a", "c1b", "bn1", "p1", "c3b", "bn4", "p4", "c5b", "u6", "bn6", "c6a", "u9", "bn9", "c9b"):
        assert relerr(eng.tap(n, name), r["acts"][name]) < 2e-5, name
    # the gradient reference on the ENGINE's sign pattern and max-pool choices wherever an fp32 pre-activation rounds to the other side of 0 (test_gpu_model.py)
    convs = [f"c{k}{ab}" for k in range(1, 10) for ab in "ab"]
    emasks = {name: (eng.tap(n, name) > 0) for name in convs}
    flips = sum(int((emasks[name] != (r["acts"][name] > 0)).sum()) for name in convs)
    assert flips <= 1e-5 * sum(m.size for m in emasks.values()) + 8, flips
    if flips:
        r = O.loss_and_grads(wts, x, y, dtype=torch.float64, want_acts=True, relu_masks={k: m.astype(np.float64) for k, m in emasks.items()},
                             pool_sel={f"p{k}": O.pool_selection(eng.tap(n, f"bn{k}")) for k in (1, 2, 3, 4)})
        assert abs(ld[0] - r["loss"]) < 1e-5
    tol_a, tol_g = 2e-4, 3e-4
    for name, masked in (("c9a", True), ("u9", False), ("c5b", True), ("p4", False), ("c4b", True), ("c1a", True)):
        want = r["act_grads"][name] * ((eng.tap(n, name) > 0) if masked else 1.0)
        assert relerr(eng.tap(n, name, grad=True), want) < tol_a, (name, flips)
    g = eng.get_grads()
    for k in g:
        assert relerr(g[k], r["grads"][k]) < tol_g, (k, flips)
    ref = make(48, 80, dropout_rate=0.0, options={"conv_pp": 0, **extra})
    assert ref.lib.unet_ctx_get_option(ref.ctx.handle, _lib.OPTIONS["conv_pp"]) == 0
    ref.set_weights(wts)
    ld0 = ref.forward_backward(x, y).cpu().numpy()
    assert abs(ld[0] - ld0[0]) < 1e-6
    differ = {name: int((emasks[name] != (ref.tap(n, name) > 0)).sum()) for name in convs}
    assert not any(differ.values()), f"ReLU decisions that differ between CONV_PP 2 and 0: {differ}"
    g0 = ref.get_grads()
    for k in g:
        assert relerr(g[k], g0[k]) < 1e-5, k


def test_programs_with_the_persistent_schedule_are_deterministic():
    """CONV_PP = 2 with DETERMINISTIC: two engines, three Adam steps each, every weight and every loss identical in every bit"""
    from test_gpu_model import make
    wts, x, y, _ = model_case()
    outs = []
    for rep in range(2):
        eng = make(48, 80, dropout_rate=0.0, options={"conv_pp": 2, "deterministic": 1}, private_context=True)
        eng.set_weights(wts)
        traj = np.array([eng.train_batch(x, y).cpu().numpy() for _ in range(3)])
        outs.append((traj, eng.get_weights()))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert np.array_equal(outs[0][1][k].view(np.int32) if outs[0][1][k].dtype == np.float32 else outs[0][1][k], outs[1][1][k].view(np.int32) if outs[1][1][k].dtype == np.float32 else outs[1][1][k]), k

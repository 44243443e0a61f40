"""CPU: the per-element checks of test_gpu_tail_elem.py (tests/tail_checks.py) are satisfiable and can fail.  "got" is an fp32 emulation in numpy of the kernel's
OWN summation order (tail_checks.emu_*: chunked fma chains, the alternating reduce, the xor butterfly of a wave, the block adds), never the float64 reference
rounded once.  It must pass every check with a ratio of at most 0.5 wherever the allowance is that of a chain, dense at K = 50176 and the sweep at L > 1 included.
Two places cannot promise the half, because an element's allowance there is one or a handful of single roundings and a correctly rounded operation may use all
of its u: Adam (0.99 of the allowance of p where the step is far below p) and the weight gradient over a batch of one (0.75).  They hold the derived bound itself
and say so where they assert; the bound is not widened to make room.  Then the emulation carries ONE defect of the kind these kernels could have, and the check
of that op must raise."""
import numpy as np
import pytest

import tail_checks as T

f32 = np.float32
HALF = 0.5
ADAM = dict(b1=0.9, b2=0.999, eps=1e-7)


def rejected(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


# ---- dense ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 4, 4), (9, 260, 32), (3, 768, 8), (65, 512, 4), (32, 50176, 32)])
def test_dense_forward_emulation_is_within_half_the_bound(shape):
    x, w, bias, _ = T.dense_case(shape)
    for act, b, rate in ((0, bias, 0.0), (1, bias, 0.0), (2, bias, 0.0), (0, None, 0.0), (1, bias, 0.4)):
        got = T.emu_dense_fwd(x, w, b, act, rate, 99)
        assert T.check_dense_fwd(got, x, w, b, act, rate, 99, f"host dense fwd {shape} act={act}") <= HALF
    xs, ws, bs, _ = T.dense_case(shape, sparse=True)
    assert T.check_dense_fwd(T.emu_dense_fwd(xs, ws, None, 0), xs, ws, None, 0, 0.0, 0, f"host dense fwd sparse {shape}") <= HALF


@pytest.mark.parametrize("shape,defect", [((9, 260, 32), "partial_chunk"), ((9, 260, 32), "rows"), ((65, 512, 4), "rows"), ((3, 768, 8), "odd_chunk"),
                                          ((9, 260, 32), "bias"), ((32, 50176, 32), "bias")])
def test_dense_forward_defects_are_rejected(shape, defect):
    x, w, bias, _ = T.dense_case(shape)
    rejected(T.check_dense_fwd, T.emu_dense_fwd(x, w, bias, 0, defect=defect), x, w, bias, 0, 0.0, 0, f"host dense fwd {defect}")
    if defect in ("partial_chunk", "rows"):          # the one row that matters carries everything: the last x row, the last W row
        xs, ws, _, _ = T.dense_case(shape, sparse=True)
        rejected(T.check_dense_fwd, T.emu_dense_fwd(xs, ws, None, 0, defect=defect), xs, ws, None, 0, 0.0, 0, f"host dense fwd sparse {defect}")


def test_dense_dropout_pattern_must_be_equal_not_plausible():
    x, w, bias, _ = T.dense_case((9, 260, 32))
    got = T.emu_dense_fwd(x, w, bias, 0, 0.4, 99)
    other = T.emu_dense_fwd(x, w, bias, 0, 0.4, 98)          # a valid dropout of the same rate under another seed
    assert 0.3 < (got == 0).mean() < 0.5 and 0.3 < (other == 0).mean() < 0.5
    rejected(T.check_dense_fwd, other, x, w, bias, 0, 0.4, 99, "host dense fwd seed")


@pytest.mark.parametrize("shape", [(1, 4, 4), (129, 516, 16), (257, 300, 32)])
def test_dense_backward_emulation_and_defects(shape):
    x, w, _, dy = T.dense_case(shape)
    dx, dw = T.emu_dense_bwd(x, w, dy)
    # (B = 1: dw is one product, a chain of ONE rounding, which may use the whole of its allowance B u |x dy|; the half applies from two links on)
    assert max(T.check_dense_bwd(dx, dw, x, w, dy, f"host dense bwd {shape}")) <= (HALF if shape[0] > 1 else 1.0)
    if shape[0] > T.DB:
        rejected(T.check_dense_bwd, None, T.emu_dense_bwd(x, w, dy, "tile2")[1], x, w, dy, "host dense bwd tile2")
    if shape[1] > 4:
        rejected(T.check_dense_bwd, T.emu_dense_bwd(x, w, dy, "w_row")[0], dw, x, w, dy, "host dense bwd w_row")


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, 40003])
@pytest.mark.parametrize("gs", [1.0, 0.125, 0.3])
def test_adam_emulation_is_within_half_the_bound_over_three_steps(n, gs):
    p, g, m, v = T.adam_case(n)
    for step in (1, 2, 3):
        lr_t = T.adam_lr_t(step)
        got = T.emu_adam(p, g, m, v, lr_t, gs=gs, **ADAM)
        # an element-wise op: m is 3 roundings, v 4, and where the step is far below p the allowance of p is the ONE rounding of the subtract, which a correctly
        # rounded result may use in full (0.99 of it among 40003 elements).  The half is a statement about long chains; here the bound has to hold, no more.
        assert max(T.check_adam(got, p, g, m, v, lr_t, gs=gs, what=f"host adam n={n} gs={gs} step {step}", **ADAM)) <= 1.0
        p, m, v = got


@pytest.mark.parametrize("defect,n,gs", [("tail", 1, 1.0), ("tail", 3, 1.0), ("tail", 1027, 1.0), ("gs_sq", 1027, 0.125), ("eps_in", 1027, 1.0)])
def test_adam_defects_are_rejected(defect, n, gs):
    p, g, m, v = T.adam_case(n)
    if n < 4:
        g[:] = 0.3; m[:] = 0.1; v[:] = 0.01          # (element 0 of adam_case is the one that must not move)
    lr_t = T.adam_lr_t(1)
    rejected(T.check_adam, T.emu_adam(p, g, m, v, lr_t, gs=gs, defect=defect, **ADAM), p, g, m, v, lr_t, gs=gs, what=f"host adam {defect}", **ADAM)


def test_adam_leaves_p_bit_identical_where_nothing_moves():
    p, g, m, v = T.adam_case(1027)
    got = list(T.emu_adam(p, g, m, v, T.adam_lr_t(1), gs=1.0, **ADAM))
    got[0] = got[0].copy(); got[0][7] = np.nextafter(got[0][7], f32(np.inf))          # one ulp: inside u |p|, but element 7 has g = m = v = 0
    rejected(T.check_adam, got, p, g, m, v, T.adam_lr_t(1), gs=1.0, what="host adam still", **ADAM)


# ---- metric sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nthr", [(1, 1), (255, 8), (4551, 9), (4551, 17), (1024 * 2048 + 3 * 256 + 5, 3)])
def test_sweep_emulation_is_within_half_the_bound(n, nthr):
    p, gt, thr = T.sweep_case(n, nthr)
    gx, L = T.sweep_grid(n)
    assert (gx, L) == {1: (1, 1), 255: (1, 1), 4551: (3, 6)}.get(n, (1024, 9))
    assert T.check_sweep(T.emu_sweep(p, gt, thr), p, gt, thr, f"host sweep n={n} T={nthr}") <= HALF
    pre = np.arange(3.0 * nthr).reshape(nthr, 3) + np.array([0.25, 0.0, 0.5])
    assert T.check_sweep(T.emu_sweep(p, gt, thr) + pre, p, gt, thr, f"host sweep n={n} T={nthr} on top", pre=pre) <= HALF
    rejected(T.check_sweep, T.emu_sweep(p, gt, thr), p, gt, thr, "host sweep overwritten", pre=pre)


@pytest.mark.parametrize("n,nthr,defect", [(1, 1, "ge"), (4551, 9, "ge"), (4551, 9, "block"), (1024 * 2048 + 3 * 256 + 5, 2, "block")])
def test_sweep_defects_are_rejected(n, nthr, defect):
    p, gt, thr = T.sweep_case(n, nthr)
    assert (p[:, None] == thr[None, :]).any() if n < 10000 else True
    rejected(T.check_sweep, T.emu_sweep(p, gt, thr, defect), p, gt, thr, f"host sweep {defect}")


# ---- classifier head ------------------------------------------------------------------------------------------------------------------------
CW = (0.7, 1.9)


@pytest.mark.parametrize("n", [4, 8, 16, 32])
@pytest.mark.parametrize("b", [1, 7, 256, 257, 300])
def test_head_emulation_is_within_half_the_bound(b, n):
    h, w, bias, t = T.head_case(b, n)
    p, sums = T.emu_head_fwd(h, w, bias, t, *CW)
    assert max(T.check_head_fwd(p, sums, h, w, bias, t, *CW, f"host head fwd B={b} N={n}")) <= HALF
    assert not (p[:min(b, 1)] != 1.0).any() and (b < 2 or p[1] == 0.5)          # the special rows: saturated, exactly one half
    got = T.emu_head_bwd(h, w, p, t, *CW, float(b), 0.4)
    assert max(T.check_head_bwd(got, h, w, p, t, *CW, float(b), 0.4, f"host head bwd B={b} N={n}").values()) <= HALF
    ref, _ = T.head_bwd_ref(h, w, p, t, *CW, float(b), 0.4)
    outside = (p < T.LO32) | (p > T.HI32)
    assert outside[:min(b, 8)].sum() >= min(b, 8) - 1 and not ref["dh"][outside].any() and not got["dh"][outside].any()


def test_head_bias_and_two_calls_add():
    h, w, _, t = T.head_case(300, 16)
    bias = np.array([0.1], f32)
    p, sums = T.emu_head_fwd(h, w, bias, t, *CW)
    pre = np.array([3.25, 5.0, 2.0, 1.0])
    assert max(T.check_head_fwd(p, sums + pre, h, w, bias, t, *CW, "host head fwd on top", pre=pre)) <= HALF
    rejected(T.check_head_fwd, p, sums, h, w, bias, t, *CW, "host head fwd overwritten", pre=pre)


@pytest.mark.parametrize("defect", ["cw_swap", "half_away"])
def test_head_forward_defects_are_rejected(defect):
    h, w, bias, t = T.head_case(300, 16)
    assert ((t * T.emu_head_fwd(h, w, bias, t, *CW)[0]) == 0.5).any()
    rejected(T.check_head_fwd, *T.emu_head_fwd(h, w, bias, t, *CW, defect=defect), h, w, bias, t, *CW, f"host head fwd {defect}")


@pytest.mark.parametrize("defect", ["no_clip", "cw_swap"])
def test_head_backward_defects_are_rejected(defect):
    h, w, bias, t = T.head_case(300, 16)
    p, _ = T.emu_head_fwd(h, w, bias, t, *CW)
    rejected(T.check_head_bwd, T.emu_head_bwd(h, w, p, t, *CW, 300.0, 0.4, defect), h, w, p, t, *CW, 300.0, 0.4, f"host head bwd {defect}")


def test_finalize_reference_gives_zero_f1_without_positives():
    ref, tol = T.finalize_ref([12.5, 0.0, 0.0, 0.0], 50.0)
    assert ref[0] == 0.25 and ref[1] == 0.0 and tol[1] == 0.0
    ref, _ = T.finalize_ref([1.0, 3.0, 4.0, 6.0], 8.0)          # precision 1/2, recall 3/4: f1 = 0.6
    assert abs(ref[1] - 0.6) < 1e-7


# ---- cast, zero -----------------------------------------------------------------------------------------------------------------------------
def test_cast_table_reaches_every_class_and_truncation_is_rejected():
    f = T.CAST_TABLE.view(f32)
    want = T.bf16_bits_torch(f)
    T.check_cast_to_bf16(T.emu_cast(f), f, "host cast")
    by = dict(zip(T.CAST_TABLE.tolist(), want.tolist()))
    assert by[0x3F808000] == 0x3F80 and by[0x3F818000] == 0x3F82 and by[0x3F808001] == 0x3F81 and by[0xBF818000] == 0xBF82          # ties to even, both directions
    assert by[0x7F7FFFFF] == 0x7F80 and by[0xFF7FFFFF] == 0xFF80 and by[0x7F7F8000] == 0x7F80 and by[0x7F7F7FFF] == 0x7F7F          # up to Inf / stays finite
    assert by[0x80000000] == 0x8000 and (by[0x7FC00000] & 0x7FFF) > 0x7F80 and by[0x00008000] == 0x0000 and by[0x00018000] == 0x0002 and by[0x007FFFFF] == 0x0080
    rejected(T.check_cast_to_bf16, T.emu_cast(f, "trunc"), f, "host cast trunc")
    rnd = np.random.default_rng(5).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(f32)
    T.check_cast_to_bf16(T.emu_cast(rnd), rnd, "host cast random bits")
    back = T.f32_bits_torch(want)
    T.bits_equal(back.view(np.uint32), want.astype(np.uint32) << 16, "host bf16 -> f32 is the shift")


@pytest.mark.parametrize("nbytes", [0, 4, 6, 8, 12, 16, 20, 28, 4096 + 12])
def test_zero_check_and_a_left_tail_word(nbytes):
    T.check_zero(T.emu_zero(8192, 256, nbytes), 256, nbytes, f"host zero {nbytes}")
    if nbytes & 15 and nbytes % 4 == 0:
        rejected(T.check_zero, T.emu_zero(8192, 256, nbytes, "tail"), 256, nbytes, f"host zero {nbytes} tail")
    if nbytes:
        rejected(T.check_zero, T.emu_zero(8192, 256, nbytes + 1), 256, nbytes, f"host zero {nbytes} one byte too many")

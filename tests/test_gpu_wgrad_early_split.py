"""-m gpu: the h2 conv3x3 weight gradient with the next step's rows scaled and split under the current step's MFMAs (UNET_OPT_WGRAD_EARLY_SPLIT).

A step of wgrad_h2_kernel splits the rows of the next step at the block exponents it holds and confirms them behind the barrier; when a block's maximum moves an
exponent it fetches the rows again and splits them as option 0 does.  Both paths must give option 0's bits, so every case runs with
  smooth     standard normal data: the exponents settle in a workgroup's first step and the speculation always holds
  x_jump     X x 64 from image row 4 on      dy_jump   dY x 64 from image row 4 on      both_jump   both
  image_jump both x 64 from the first row of the second image on (a workgroup that walks several units keeps its exponents from one unit to the next)
and asserts (a) option 1 == option 0 in every bit of dW and db, (b) both within the per-element bound of gpu_util.py against float64 (floor 0: the operands of a
tile stay within 2^14 of each other).  A block's maximum is re-centred at [2^11, 2^12) and its exponent moves when the scaled maximum reaches 2^15, so a step whose rows
are 16 x larger than everything before them must move it: `jumps_move_the_exponent` checks that on the inputs (x 64 on normal data leaves a wide margin).
Shapes: n = 2, h in {4, 10}, w in {32, 34} (one and two 32-column strips, ragged) -- h = 10 walks five two-row steps (three four-row ones), the jump at row 4 meets a
speculative step; (cin, cout) reach the four wave layouts of k_conv3x3_h2_wgrad (64/64 and 128/128: 2,2,1; 64/32: 2,1,2; 32/64: 1,2,2; 32/32: 1,1,4 with four rows per
step).  The entry behind the head stream (32 channels, four rows per step) takes w in {32, 40}: the stream needs a multiple of 8.  One more shape, 16 x 4 x 32 x 512 -> 512,
is the smallest whose plan gives a workgroup two units (images), so that image_jump crosses from one unit to the next inside a workgroup."""
import numpy as np
import pytest
import torch

from covidseg_amd import _lib

pytestmark = pytest.mark.gpu
KINDS = ("smooth", "x_jump", "dy_jump", "both_jump", "image_jump")
OPT = _lib.OPTIONS["wgrad_early_split"]


@pytest.fixture(scope="module")
def ops():
    from gpu_util import Ops
    o = Ops()
    was = o.lib.unet_ctx_get_option(o.h, OPT)
    yield o
    o.lib.unet_ctx_set_option(o.h, OPT, was)          # (the context is shared with every other test module)


def inputs(kind, shape, seed):
    n, h, w, ci, co = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, ci)).astype(np.float32); dy = rng.standard_normal((n, h, w, co)).astype(np.float32)
    if kind in ("x_jump", "both_jump"): x[:, 4:] *= np.float32(64)
    if kind in ("dy_jump", "both_jump"): dy[:, 4:] *= np.float32(64)
    if kind == "image_jump": x[1:] *= np.float32(64); dy[1:] *= np.float32(64)
    return x, dy


def jumps_move_the_exponent(kind, x, dy):
    """the two rows behind a jump are >= 16 x everything in front of it, per operand that jumps, image and 32-column strip"""
    for name, a in (("x", x), ("dy", dy)):
        for c0 in range(0, a.shape[2], 32):
            s = np.abs(a[:, :, c0:c0 + 32])
            if kind in (name + "_jump", "both_jump") and a.shape[1] > 4:
                assert s[:, 4:6].reshape(a.shape[0], -1).max(1).min() >= 16 * s[:, :4].max(), (kind, name, c0)
            if kind == "image_jump":
                assert s[1, :2].max() >= 16 * s[0].max(), (kind, name, c0)


def wgrad64(x, dy):
    """dw[a][b][ci][co], db[co] in float64 and their sums of absolute products"""
    n, h, w, ci = x.shape
    co = dy.shape[3]
    x64 = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0))); d64 = dy.astype(np.float64).reshape(-1, co)
    dw = np.zeros((3, 3, ci, co)); a1 = np.zeros((3, 3, ci, co))
    for a in range(3):
        for b in range(3):
            win = x64[:, a:a + h, b:b + w].reshape(-1, ci)
            dw[a, b] = win.T @ d64; a1[a, b] = np.abs(win).T @ np.abs(d64)
    return dw, d64.sum(0), a1, np.abs(d64).sum(0)


def run(ops, value, launch, ci, co):
    ops.ck(ops.lib.unet_ctx_set_option(ops.h, OPT, value), "set_option")
    assert ops.lib.unet_ctx_get_option(ops.h, OPT) == value
    dw = ops.z(3, 3, ci, co); db = ops.z(co)
    dw.fill_(123.0); db.fill_(-7.0)                                  # overwritten, not accumulated
    launch(dw, db)
    return dw.cpu().numpy(), db.cpu().numpy()


def check(ops, launch, ref, ci, co, what):
    from gpu_util import elem_ratio
    dw64, db64, a1, b1 = ref
    got = {v: run(ops, v, launch, ci, co) for v in (0, 1)}
    for v in (0, 1):
        rw, rb = elem_ratio(got[v][0], dw64, a1), elem_ratio(got[v][1], db64, b1)
        print(f"bound-ratio wgrad early split {what} option {v}: dw {rw:.3g} db {rb:.3g}")
        assert rw <= 1.0 and rb <= 1.0, (what, v, rw, rb)
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)), f"{what}: dW differs between option 0 and 1 in {np.count_nonzero(got[0][0] != got[1][0])} elements"
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32)), f"{what}: db differs between option 0 and 1"
    assert 0 <= ops.lib.unet_ctx_max_kernel_scratch_bytes(ops.h) <= 128


def conv_case(ops, shape):
    n, h, w, ci, co = shape
    nb = int(ops.lib.unet_conv3x3_bwd_weights_ws_bytes(n, h, w, ci, co)); ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    for i, kind in enumerate(KINDS):
        x, dy = inputs(kind, shape, 100 * i + h + w + ci + 2 * co)
        jumps_move_the_exponent(kind, x, dy)
        xd, dyd = ops.d(x), ops.d(dy)
        check(ops, lambda dw, db: ops.ck(ops.lib.unet_conv3x3_bwd_weights(ops.h, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, n, h, w, ci, co, 0, ops.s), "wgrad"),
              wgrad64(x, dy), ci, co, f"{shape} {kind}")


@pytest.mark.parametrize("chans", [(32, 32), (64, 64), (32, 64), (64, 32), (128, 128)])
@pytest.mark.parametrize("hw", [(4, 32), (4, 34), (10, 32), (10, 34)])
def test_early_split_gives_the_bits_of_the_split_between_the_barriers(ops, hw, chans):
    conv_case(ops, (2, hw[0], hw[1], chans[0], chans[1]))


def test_early_split_keeps_the_exponents_from_one_unit_to_the_next(ops):
    conv_case(ops, (16, 4, 32, 512, 512))


@pytest.mark.parametrize("hw", [(4, 32), (4, 40), (10, 32), (10, 40)])
def test_early_split_behind_the_head_stream(ops, hw):
    """unet_conv3x3_bwd_weights_dzm: the dY operand is the stream {dz, 32 mask bits} per pixel, dy[p][c] = dz_p w_c [bit c]; the jumps of dY are jumps of dz"""
    n, (h, w), c = 2, hw, 32
    assert ops.lib.unet_head_bwd_stream_supported(ops.h, 0, w, c) == 1
    nb = int(ops.lib.unet_conv3x3_bwd_weights_ws_bytes(n, h, w, c, c)); ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    for i, kind in enumerate(KINDS):
        rng = np.random.default_rng(900 + 10 * i + h + w)
        x, dz = inputs(kind, (n, h, w, c, 1), 300 + 10 * i + h + w)
        jumps_move_the_exponent(kind, x, dz)
        mask = rng.integers(1, 2 ** 32, size=(n, h, w), dtype=np.uint64).astype(np.uint32)          # (never 0: a pixel without a live channel does not count for the block maximum)
        w_head = (rng.standard_normal(c) * 0.8).astype(np.float32); w_head[7] = 0.0
        stream = np.stack([dz[..., 0].view(np.uint32), mask], axis=-1)
        bit = ((mask[..., None] >> np.arange(c, dtype=np.uint32)) & 1).astype(np.float64)
        dy = dz.astype(np.float64) * bit * w_head.astype(np.float64)
        xd, sd, wd = ops.d(x), torch.from_numpy(stream.view(np.int64).reshape(n, h, w)).cuda(), ops.d(w_head)
        check(ops, lambda dw, db: ops.ck(ops.lib.unet_conv3x3_bwd_weights_dzm(ops.h, xd.data_ptr(), sd.data_ptr(), wd.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, n, h, w, c, ops.s),
                                         "wgrad of the stream"), wgrad64(x, dy), c, c, f"stream {(n, h, w)} {kind}")

"""-m gpu: the first kernels a CT meets, called through the C ABI at the shapes, pointers and values the wrappers cannot reach -- csrc/kernels_volume.hip
(unet_vol_slices_f64, unet_vol_unslice) against tests/volume_oracle.py and csrc/kernels_pre.hip (the unet_pre_* entry points) against oracle/preprocess_oracle.py.

Every device output of a direct call lies between two guard bands of a sentinel that must be intact afterwards (front_edges.Guarded), a refused call must leave the
outputs' own bytes as they were too, and every comparison is np.array_equal (equal_nan for the float stages).  The one exception is the rule test_gpu_volume.py applies
to unet_vol_unslice: a mask voxel may differ from the float32 oracle only where the float64 oracle's probability lies within 1e-6 of the threshold;
tests/test_front_edges_host.py verifies that at most 0.001 of the voxels of each case lie there, and the other conditions the cases rest on.

A. unet_vol_slices_f64: the scalar output kernel (S * S % 4 != 0, an output pointer off its alignment, absent outputs), second trips of every grid-stride loop, NaN and
   infinities in float volumes, the uniform flag on slices that are uniform but for one voxel, the z-ranges, a uint8 volume at an odd address, every refusal.
B. the typed decode over every integer type's whole range: unet_vol_slices_f64, unet_vol_intensity_bands, unet_vol_texture_quantize.
C. unet_vol_unslice: second trips of both loops, a mask pointer off by one byte, tiny volumes, thresholds outside the canvas' values, every refusal.
D. kernels_pre.hip: min-max with NaN / infinities / constant slices, the truncations of unit_to_u8, CLAHE on tiles of 1 x 1 and 2 x 2 pixels and on padded grids,
   resize rectangles on the source's edges into a strided destination, every refusal."""
import numpy as np
import pytest

import front_edges as FE
import intensity_oracle as IO
import texture_oracle as TO
import volume_oracle as VO
from front_edges import E_ARG, E_SHAPE, Guarded
from oracle import preprocess_oracle as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from gpu_util import Ops
    return Ops()


# ---- A. unet_vol_slices_f64 -----------------------------------------------------------------------------------------------------------------------------------
SKEW_OF = {"f32": 4, "u8": 1, "lung": 1}                            # one element past an aligned allocation
DTYPE_OF = {"f32": "float32", "u8": "uint8", "lung": "uint8"}


class SlicesCall:
    """the buffers of one unet_vol_slices_f64 call, every output guarded; `skewed` = the outputs that start one element off their alignment"""

    def __init__(self, ops, raw, slope, inter, z0, z1, S, want=("f32", "u8", "lung"), skewed=(), vox_skew=0):
        import torch
        from covidseg_amd import nifti_min
        self.ops, self.n, self.S, self.want = ops, z1 - z0, S, want
        n, Pn = max(self.n, 1), S * S
        flat = np.asfortranarray(raw).reshape(-1, order="F").view(np.uint8)
        self.vox = torch.zeros(flat.size + 16, dtype=torch.uint8, device="cuda")
        self.vox[vox_skew:vox_skew + flat.size] = torch.from_numpy(flat).cuda()
        sc = nifti_min.scaling(slope, inter)
        self.out = {k: Guarded(n * Pn, DTYPE_OF[k], SKEW_OF[k] if k in skewed else 0) for k in want}
        self.uniform, self.minmax = Guarded(n, "int32"), Guarded(2 * n, "float64")
        self.ws_bytes = int(ops.lib.unet_vol_slices_ws_bytes(n, S))
        self.ws = Guarded(self.ws_bytes, "uint8")
        X, Y, Z = raw.shape
        self.args = dict(vox=self.vox.data_ptr() + vox_skew, dtype=FE.CODES[raw.dtype.str[1:]], X=X, Y=Y, Z=Z, scaled=1 if sc else 0, slope=sc[0] if sc else 1.0,
                         inter=sc[1] if sc else 0.0, z0=z0, z1=z1, S=S, f32=self._ptr("f32"), u8=self._ptr("u8"), lung=self._ptr("lung"), uniform=self.uniform.ptr,
                         minmax=self.minmax.ptr, ws=self.ws.ptr, ws_bytes=self.ws_bytes)

    def _ptr(self, k):
        return self.out[k].ptr if k in self.out else None

    def call(self, **kw):
        a = {**self.args, **kw}
        return self.ops.lib.unet_vol_slices_f64(self.ops.h, a["vox"], a["dtype"], a["X"], a["Y"], a["Z"], a["scaled"], a["slope"], a["inter"], a["z0"], a["z1"], a["S"], a["f32"],
                                                a["u8"], a["lung"], a["uniform"], a["minmax"], a["ws"], a["ws_bytes"], self.ops.s)

    def results(self, what):
        n, S = self.n, self.S
        got = {k: g.get(f"{what}: {k}").reshape(n, S, S) for k, g in self.out.items()}
        got["uniform"], got["minmax"] = self.uniform.get(f"{what}: uniform"), self.minmax.get(f"{what}: minmax").reshape(n, 2)
        got["img64"] = self.ws.get(f"{what}: workspace")[:n * S * S * 8].view(np.float64).reshape(n, S, S)          # the workspace starts with the resized float64 images
        return got

    def untouched(self):
        return all(g.untouched() for g in (*self.out.values(), self.uniform, self.minmax, self.ws))


def _check_slices(ops, raw, slope, inter, z0, z1, S, what, **kw):
    c = SlicesCall(ops, raw, slope, inter, z0, z1, S, **kw)
    ops.ck(c.call(), str(what))
    got = c.results(what)
    with np.errstate(invalid="ignore"):
        want = VO.slices_f64(raw, slope, inter, z0, z1, S)
    assert np.array_equal(got["img64"], want["img64"], equal_nan=True), (what, "resized float64 stage")
    assert np.array_equal(got["minmax"], want["minmax"], equal_nan=True), (what, "minmax")
    assert np.array_equal(got["uniform"], want["uniform"]), (what, "uniform", got["uniform"], want["uniform"])
    for k in c.want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=k == "f32"), (what, k)
    return got, want


def test_slices_scalar_outputs_for_an_odd_pixel_count(ops):
    raw = FE.smooth_volume((63, 40, 4), "i2", 1)
    _check_slices(ops, raw, *FE.SCALE, 0, 4, 31, "S = 31")            # P = 961: no pixel quadruples; z0 = 0 with z1 = Z


@pytest.mark.parametrize("skewed", ["f32", "u8", "lung"])
def test_slices_scalar_outputs_for_one_pointer_off_its_alignment(ops, skewed):
    raw = FE.smooth_volume((63, 40, 4), "i2", 1)
    _check_slices(ops, raw, 0.0, 0.0, 1, 3, 32, f"S = 32, {skewed} off by one element", skewed=(skewed,))


@pytest.mark.parametrize("want", [("u8",), ("f32", "lung")])
@pytest.mark.parametrize("S", [32, 31])
def test_slices_absent_outputs_are_null_pointers(ops, want, S):
    raw = FE.smooth_volume((63, 40, 4), "i2", 1)
    _check_slices(ops, raw, *FE.SCALE, 1, 4, S, ("only", want, S), want=want)


@pytest.mark.parametrize("name,shape,S", FE.STRIDE_CASES, ids=[c[0] for c in FE.STRIDE_CASES])
def test_slices_second_trips_of_the_grid_stride_loops(ops, name, shape, S):
    raw = FE.smooth_volume(shape, "i2", 2)
    _check_slices(ops, raw, *FE.SCALE, 0, shape[2], S, name)


@pytest.mark.parametrize("S", FE.NAN_SIZES)
@pytest.mark.parametrize("kind", ["f4", "f8"])
def test_slices_nan_and_infinities_give_what_numpy_gives(ops, kind, S):
    raw = FE.nan_inf_volume(kind)
    got, _ = _check_slices(ops, raw, 0.0, 0.0, 0, raw.shape[2], S, (kind, S))
    assert got["uniform"].tolist() == [1, 0, 0, 0] and np.isnan(got["minmax"][:2]).all() and not got["u8"].any()          # (test_front_edges_host.py: the oracle's values)
    assert np.isnan(got["minmax"][2:]).all() if S == 48 else (got["minmax"][2, 1] == np.inf and got["minmax"][3, 0] == -np.inf)


def test_slices_uniform_flag_sees_a_single_differing_voxel(ops):
    i2, f4, flags = FE.uniform_volumes()
    got, _ = _check_slices(ops, i2, 0.0, 0.0, 0, 6, 32, "int16")
    assert got["uniform"].tolist() == [0, 1, 0, 0, 0, 0]
    got, _ = _check_slices(ops, i2, *FE.SCALE, 1, 4, 48, "int16, scaled, equal size")
    assert got["uniform"].tolist() == flags[:3]
    got, _ = _check_slices(ops, f4, 0.0, 0.0, 1, 5, 32, "float32 with a slice of both zeros")
    assert got["uniform"].tolist() == flags


def test_slices_ranges_and_a_single_slice_volume(ops):
    raw = FE.smooth_volume((33, 21, 5), "i2", 4)
    _check_slices(ops, raw, 0.0, 0.0, 0, 5, 16, "z0 = 0, z1 = Z")
    _check_slices(ops, raw, 0.0, 0.0, 4, 5, 16, "the last slice alone")
    _check_slices(ops, np.asfortranarray(raw[:, :, 2:3]), *FE.SCALE, 0, 1, 16, "Z = 1")


def test_slices_take_a_uint8_volume_at_an_odd_address(ops):
    raw = FE.smooth_volume((63, 40, 3), "u1", 6)
    _check_slices(ops, raw, 0.0, 0.0, 0, 3, 32, "u1 at an odd address", vox_skew=1)
    _check_slices(ops, raw, *FE.SCALE, 0, 3, 31, "u1 at an odd address, scaled", vox_skew=1)


def test_slices_refused_arguments_launch_nothing(ops):
    raw = np.zeros((8, 6, 3), np.float64, order="F")                  # (float64: room for every item size behind the odd address)
    c = SlicesCall(ops, raw, 0.0, 0.0, 0, 2, 4)
    refused = [(dict(vox=None), E_ARG), (dict(ws=None), E_ARG), (dict(X=0), E_ARG), (dict(Y=0), E_ARG), (dict(Z=0), E_ARG), (dict(S=0), E_ARG), (dict(X=-1), E_ARG),
               (dict(S=-4), E_ARG), (dict(dtype=3), E_ARG), (dict(dtype=1024), E_ARG), (dict(z0=1, z1=1), E_SHAPE), (dict(z0=2, z1=1), E_SHAPE), (dict(z1=4), E_SHAPE),
               (dict(z0=-1), E_SHAPE), (dict(S=32768), E_SHAPE), (dict(X=32768, Y=32768), E_SHAPE), (dict(ws_bytes=c.ws_bytes - 1), E_ARG), (dict(ws=c.ws.ptr + 8), E_ARG)]
    refused += [(dict(dtype=FE.CODES[k], vox=c.args["vox"] + 1), E_ARG) for k in ("i2", "u2", "i4", "f4", "f8")]
    for kw, code in refused:
        assert c.call(**kw) == code, kw
        assert ops.ctx.last_error().startswith("vol_slices_f64"), (kw, ops.ctx.last_error())
    assert "datatype code 3" in (c.call(dtype=3), ops.ctx.last_error())[1] and "item size" in (c.call(dtype=64, vox=c.args["vox"] + 4), ops.ctx.last_error())[1]
    assert c.untouched()
    for k in ("u1", "i1"):                                           # one-byte items have no alignment to miss: the same call is taken
        ops.ck(c.call(dtype=FE.CODES[k], vox=c.args["vox"] + 1), k)
    assert c.results("after the refusals")["uniform"].tolist() == [1, 1]


# ---- B. every integer datatype over its whole range -------------------------------------------------------------------------------------------------------------
def _nifti(raw, slope, inter):
    from covidseg_amd import nifti_min
    return nifti_min.NiftiVolume(np.asfortranarray(raw), slope, inter, (1.0, 1.0, 1.0), nifti_min.default_header(raw.shape, (1.0, 1.0, 1.0)), "<")


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kind", FE.INT_KINDS)
def test_slices_decode_every_integer_type_over_its_whole_range(ops, kind, scaled):
    raw = FE.full_range_volume(kind)
    slope, inter = FE.SCALE if scaled else (0.0, 0.0)
    got, _ = _check_slices(ops, raw, slope, inter, 0, FE.RANGE_SHAPE[2], FE.RANGE_S, (kind, scaled))
    assert np.isfinite(got["img64"]).all()


@pytest.mark.parametrize("kind", FE.INT_KINDS)
def test_intensity_and_texture_decode_every_integer_type_over_its_whole_range(kind):
    from test_gpu_intensity import _check_bands, _dev, _edges
    from test_gpu_texture import dev_quantize
    raw = FE.full_range_volume(kind)
    info = np.iinfo(kind)
    for scaled in (False, True):
        slope, inter = FE.SCALE if scaled else (0.0, 0.0)
        vol = _nifti(raw, slope, inter)
        fdata = IO.decode(raw, scaled, slope, inter)
        assert np.array_equal(vol.get_fdata(), fdata) and fdata.min() == (info.min * slope + inter if scaled else info.min)
        assert fdata.max() == (info.max * slope + inter if scaled else info.max)
        edges = _edges(fdata)
        lo, width = float(fdata.min()), float((fdata.max() - fdata.min()) / 7)
        for name, labels, mask, n, region in FE.range_layouts(raw.shape):
            what = (kind, scaled, name)
            _check_bands(vol, fdata, labels, mask, n, region, edges, what)
            g = TO.group_of(raw.shape, labels=labels, mask=mask, n=n, region=region)
            ld, md = (_dev(labels, np.int32) if labels is not None else None), (_dev(mask, np.uint8) if mask is not None else None)
            rd = _dev(region, np.uint8) if region is not None else None
            for outside in (0, 1):
                want_lv, want_lc = TO.quantize(fdata, g, n, lo, width, 8, outside)
                got_lv, got_lc, _ = dev_quantize(vol, ld, md, n, rd, lo, width, 8, outside, str(what))
                assert np.array_equal(got_lv, want_lv) and np.array_equal(got_lc, want_lc), (what, outside)
            assert want_lc.sum() > 0 and (want_lc.sum(axis=0) > 0).sum() >= 7          # the levels spread over the whole range: a wrapped decode lands in other bins


# ---- C. unet_vol_unslice ------------------------------------------------------------------------------------------------------------------------------------------
class UnsliceCall:
    def __init__(self, ops, canvas, t, shape, z0, z1, skew=0):
        X, Y, Z = shape
        self.ops, self.shape, self.n = ops, shape, z1 - z0
        self.canvas = ops.d(canvas)
        self.mask, self.counts = Guarded(X * Y * Z, "uint8", skew), Guarded(max(self.n, 1), "int64")
        self.args = dict(canvas=self.canvas.data_ptr(), S=canvas.shape[1], t=float(t), X=X, Y=Y, Z=Z, z0=z0, z1=z1, mask=self.mask.ptr, counts=self.counts.ptr)

    def call(self, **kw):
        a = {**self.args, **kw}
        return self.ops.lib.unet_vol_unslice(self.ops.h, a["canvas"], a["S"], a["t"], a["X"], a["Y"], a["Z"], a["z0"], a["z1"], a["mask"], a["counts"], self.ops.s)


@pytest.mark.parametrize("case", FE.UNSLICE_CASES, ids=[c[0] for c in FE.UNSLICE_CASES])
def test_unslice_against_the_oracle(ops, case):
    name, shape, z0, z1, t, skew = case
    canvas, wmask, near = FE.unslice_case(case)
    c = UnsliceCall(ops, canvas, t, shape, z0, z1, skew)
    assert (c.mask.ptr % 4 == 0) == (skew == 0)
    ops.ck(c.call(), name)
    mask, counts = c.mask.get(f"{name}: mask").reshape(shape, order="F"), c.counts.get(f"{name}: counts")
    differ = np.stack([np.rot90(mask[:, :, z0 + k] != wmask[:, :, z0 + k]) for k in range(z1 - z0)])          # [n, Y, X] image orientation, as `near`
    print(f"{name}: {int(differ.sum())} voxels differ from the float32 oracle, {int(near.sum())} of {near.size} lie within {FE.NEAR} of the threshold")
    assert set(np.unique(mask)) <= {0, 1}
    assert not (differ & ~near).any()
    assert np.array_equal(counts, [int(mask[:, :, z].sum()) for z in range(z0, z1)])
    assert not mask[:, :, :z0].any() and not mask[:, :, z1:].any()
    if t > canvas.max():
        assert not mask.any() and not counts.any()
    if t < 0:
        assert mask[:, :, z0:z1].all() and (counts == shape[0] * shape[1]).all()


def test_unslice_refused_arguments_launch_nothing(ops):
    shape = (12, 10, 4)
    c = UnsliceCall(ops, FE.canvas(2, 3, 16), 0.5, shape, 1, 3)
    refused = [(dict(canvas=None), E_ARG), (dict(mask=None), E_ARG), (dict(counts=None), E_ARG), (dict(S=0), E_ARG), (dict(X=0), E_ARG), (dict(Y=0), E_ARG), (dict(Z=0), E_ARG),
               (dict(X=-12), E_ARG), (dict(z0=2, z1=2), E_SHAPE), (dict(z0=3, z1=1), E_SHAPE), (dict(z1=5), E_SHAPE), (dict(z0=-1), E_SHAPE),
               (dict(X=32768, Y=32768), E_SHAPE), (dict(S=32768), E_SHAPE)]
    for kw, code in refused:
        assert c.call(**kw) == code, kw
        assert ops.ctx.last_error().startswith("vol_unslice"), (kw, ops.ctx.last_error())
    assert c.mask.untouched() and c.counts.untouched()
    ops.ck(c.call(), "the call the refusals were varied from")
    assert c.mask.get().any() and c.counts.get().sum() > 0


# ---- D. kernels_pre.hip ---------------------------------------------------------------------------------------------------------------------------------------------
def _minmax(ops, x, what):
    n, pixels = x.shape[0], int(x[0].size)
    out = Guarded(x.size, "uint8")
    ws_bytes = int(ops.lib.unet_pre_minmax_ws_bytes(n))
    assert ws_bytes == 8 * n
    ws = Guarded(ws_bytes, "uint8")
    ops.ck(ops.lib.unet_pre_minmax_to_u8(ops.h, ops.d(x).data_ptr(), out.ptr, n, pixels, ws.ptr, ws_bytes, ops.s), what)
    ws.get(f"{what}: workspace")
    return out.get(f"{what}: out").reshape(x.shape)


def test_minmax_nan_infinities_and_a_constant_slice(ops):
    """np.uint8((a - a.min()) / (a.max() - a.min()) * 255) propagates a NaN (and x / inf = 0, inf / inf = NaN): all four special slices come out 0"""
    x = FE.minmax_batch()
    got = _minmax(ops, x, "five slices in one call")
    names = ("plain", "one NaN", "one +inf", "one -inf", "constant")
    for i, name in enumerate(names):
        want = FE.minmax_expected(x[i])
        print(f"min-max, {name}: {int((got[i] != want).sum())} of {want.size} bytes differ from numpy's; device max {int(got[i].max())}, numpy max {int(want.max())}")
    for i, name in enumerate(names):
        assert np.array_equal(got[i], FE.minmax_expected(x[i])), name
    assert np.array_equal(got[0], P.minmax_to_u8(x[0])) and got[0].max() == 255 and not got[1:].any()
    for nan in (np.float32(np.nan), -np.float32(np.nan), np.array([0xFFC00001], np.uint32).view(np.float32)[0]):          # either sign, with a payload; first and last pixel
        y = x[:2].copy()
        y[1, 20, 45] = 3.0
        y[0, 0, 0] = y[1, -1, -1] = nan
        assert not _minmax(ops, y, "NaN forms").any()
    assert not _minmax(ops, np.full((2, 5, 7), np.nan, np.float32), "all NaN").any()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 3), (65, 8, 8), (1, 1, 256 * 256 + 1), (3, 1, 256 * 256 + 1)])
def test_minmax_small_images_many_images_and_a_second_trip(ops, shape):
    x = np.random.default_rng(shape[0] + shape[2]).normal(-600, 400, shape).astype(np.float32)
    if shape[2] > FE.PRE_MINMAX_TRIP:
        x[-1, 0, :-1] = np.clip(x[-1, 0, :-1], -1000, 1000)
        x[-1, 0, -1] = 5000.0                                        # the maximum is the one pixel of the second trip
    if shape[0] == 3:
        x[1, 0, -1] = np.nan                                         # ... or the NaN is
    got = _minmax(ops, x, str(shape))
    for g, im in zip(got, x):
        assert np.array_equal(g, FE.minmax_expected(im)), shape
    if shape[2] > FE.PRE_MINMAX_TRIP:
        assert got[-1, 0, -1] == 255 and got[-1].min() == 0


@pytest.mark.parametrize("count", FE.UNIT_COUNTS)
def test_unit_to_u8_truncates_and_u8_to_unit_divides(ops, count):
    e = FE.unit_edges()
    x = np.resize(e, count) if count > 1 else e[300:301]
    out = Guarded(count, "uint8")
    ops.ck(ops.lib.unet_pre_unit_to_u8(ops.h, ops.d(x).data_ptr(), out.ptr, count, ops.s), "unit_to_u8")
    assert np.array_equal(out.get("unit_to_u8"), P.to_u8(x))
    b = np.resize(np.arange(256, dtype=np.uint8), count) if count > 1 else np.array([254], np.uint8)
    outf = Guarded(count, "float32")
    ops.ck(ops.lib.unet_pre_u8_to_unit(ops.h, ops.d(b, np.uint8).data_ptr(), outf.ptr, count, ops.s), "u8_to_unit")
    assert np.array_equal(outf.get("u8_to_unit"), P.u8_to_unit(b))


def _clahe_call(ops, src_ptr, dst, n, h, w, clip, tx, ty, ws, ws_bytes):
    return ops.lib.unet_pre_clahe_u8(ops.h, src_ptr, dst.ptr if dst is not None else None, n, h, w, clip, tx, ty, ws.ptr if ws is not None else None, ws_bytes, ops.s)


@pytest.mark.parametrize("shape,tiles,clips", FE.CLAHE_CASES, ids=[f"{s[0]}x{s[1]}-grid{t[0]}x{t[1]}" for s, t, _ in FE.CLAHE_CASES])
def test_clahe_small_tiles_padded_axes_and_other_grids(ops, shape, tiles, clips):
    imgs = FE.clahe_batch(shape)
    n, (h, w), (tx, ty) = len(imgs), shape, tiles
    src = ops.d(imgs, np.uint8)
    for clip in clips:
        dst = Guarded(imgs.size, "uint8")
        ws_bytes = int(ops.lib.unet_pre_clahe_ws_bytes(n, tx, ty))
        assert ws_bytes == n * tx * ty * 256
        ws = Guarded(ws_bytes, "uint8")
        ops.ck(_clahe_call(ops, src.data_ptr(), dst, n, h, w, clip, tx, ty, ws, ws_bytes), str((shape, tiles, clip)))
        ws.get("the LUT workspace")
        got = dst.get("dst").reshape(imgs.shape)
        for i, im in enumerate(imgs):
            assert np.array_equal(got[i], P.clahe_u8(im, clip, tiles)), (shape, tiles, clip, i)


def test_resize_rectangles_on_the_edges_into_a_strided_destination(ops):
    imgs, rects, d = FE.resize_sources(), np.ascontiguousarray(FE.RESIZE_RECTS), FE.RESIZE_DST
    n, (sh, sw) = len(imgs), FE.RESIZE_SRC
    dh, dw, x0, ld = d["dh"], d["dw"], d["dst_x0"], d["dst_ld"]
    src = ops.d(imgs, np.uint8)
    for interp in (P.INTER_LINEAR, P.INTER_AREA):
        dst = Guarded(n * dh * ld, "uint8")
        ops.ck(ops.lib.unet_pre_resize_u8(ops.h, src.data_ptr(), n, sh, sw, rects.ctypes.data, dst.ptr, dh, dw, ld, x0, interp, ops.s), f"resize {interp}")
        got = dst.get("dst").reshape(n, dh, ld)
        want = np.full((n, dh, ld), FE.SENT, np.uint8)               # the columns outside [dst_x0, dst_x0 + dw) keep the sentinel
        for i, (x, y, w, h) in enumerate(rects):
            want[i, :, x0:x0 + dw] = P.resize_u8(imgs[i, y:y + h, x:x + w], (dw, dh), interp)
        assert np.array_equal(got, want), interp


def test_pre_refused_arguments_launch_nothing(ops):
    lib, h, s = ops.lib, ops.h, ops.s
    f = ops.d(np.linspace(0, 1, 128)); b = ops.d(np.arange(128), np.uint8)
    out8, outf, ws = Guarded(128, "uint8"), Guarded(128, "float32"), Guarded(4 * 64 * 256, "uint8")

    def refused(rc, code, prefix, what):
        assert rc == code, (what, rc)
        assert ops.ctx.last_error().startswith(prefix), (what, ops.ctx.last_error())

    mm = lambda img=f.data_ptr(), out=out8.ptr, n=2, pixels=64, w=ws.ptr, wb=16: lib.unet_pre_minmax_to_u8(h, img, out, n, pixels, w, wb, s)
    for kw in (dict(img=None), dict(out=None), dict(w=None), dict(n=0), dict(n=-1), dict(pixels=0), dict(wb=15)):
        refused(mm(**kw), E_ARG, "pre_minmax_to_u8", kw)
    for count in (0, -5):
        refused(lib.unet_pre_unit_to_u8(h, f.data_ptr(), out8.ptr, count, s), E_ARG, "pre_unit_to_u8", count)
        refused(lib.unet_pre_u8_to_unit(h, b.data_ptr(), outf.ptr, count, s), E_ARG, "pre_u8_to_unit", count)
    refused(lib.unet_pre_unit_to_u8(h, None, out8.ptr, 8, s), E_ARG, "pre_unit_to_u8", "img")
    refused(lib.unet_pre_unit_to_u8(h, f.data_ptr(), None, 8, s), E_ARG, "pre_unit_to_u8", "out")
    refused(lib.unet_pre_u8_to_unit(h, None, outf.ptr, 8, s), E_ARG, "pre_u8_to_unit", "src")
    refused(lib.unet_pre_u8_to_unit(h, b.data_ptr(), None, 8, s), E_ARG, "pre_u8_to_unit", "dst")

    cl = lambda src=b.data_ptr(), dst=out8, n=1, hh=8, w=16, clip=3.0, tx=4, ty=2, w_=ws, wb=8 * 256: _clahe_call(ops, src, dst, n, hh, w, clip, tx, ty, w_, wb)
    for kw in (dict(src=None), dict(dst=None), dict(w_=None), dict(n=0), dict(hh=0), dict(w=0), dict(tx=0), dict(ty=0), dict(ty=-2), dict(clip=-0.5), dict(wb=8 * 256 - 1)):
        refused(cl(**kw), E_ARG, "pre_clahe_u8", kw)
    for (hh, w), (tx, ty) in FE.CLAHE_REFUSED:
        refused(cl(hh=hh, w=w, tx=tx, ty=ty, wb=64 * 256), E_SHAPE, "pre_clahe_u8", (hh, w, tx, ty))
        assert f"image {hh} x {w} " in ops.ctx.last_error() and f"a {ty} x {tx} grid" in ops.ctx.last_error()

    rect = np.array([[0, 0, 8, 8]], np.int32)
    rs = lambda src=b.data_ptr(), n=1, sh=8, sw=16, dst=out8.ptr, dh=4, dw=6, ld=8, x0=2, interp=1: lib.unet_pre_resize_u8(h, src, n, sh, sw, rect.ctypes.data, dst, dh, dw, ld, x0,
                                                                                                                             interp, s)
    for kw in (dict(src=None), dict(dst=None), dict(n=0), dict(sh=0), dict(sw=0), dict(dh=0), dict(dw=0), dict(ld=7), dict(x0=3), dict(x0=-1), dict(x0=-1, ld=5), dict(interp=2),
               dict(interp=0)):
        refused(rs(**kw), E_ARG, "pre_resize_u8", kw)
    refused(rs(dh=65536, dw=32768, ld=32768, x0=0), E_SHAPE, "pre_resize_u8", "dh * dw = 2^31")
    assert out8.untouched() and outf.untouched() and ws.untouched()
    ops.ck(rs(), "the resize the refusals were varied from")
    assert (out8.get().reshape(-1, 8)[:4, 2:] != FE.SENT).any()

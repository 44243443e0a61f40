"""-m gpu: csrc/kernels_resample.hip and volume.resample_volume / resample_mask / resample_labels / reorient_volume / change_between against tests/resample_oracle.py.
Both kernels are defined operation by operation, so every comparison is array_equal (floats: equal_nan); every output lies inside a sentinel-filled buffer that must
survive, and a refused call must leave its output untouched."""
import numpy as np
import pytest

import lungside_oracle as LO
import resample_oracle as RS
import volscore_oracle as SO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

E_ARG = -1                                                          # UNET_E_ARG
SOURCES = [(1, 1, 1), (5, 3, 2), (64, 2, 2), (67, 5, 3), (130, 3, 2)]          # x: one voxel, short of a wave, on it, past it, past two waves
OUTPUTS = [(1, 1, 1), (5, 4, 3), (64, 2, 4), (67, 3, 2), (130, 4, 2)]
STORAGE = ["i2", "i2neg", "u1", "f4nan", "f8"]
SENTINEL = 0x5A
GUARD = 64                                                          # sentinel bytes on either side of an output
CVAL_BITS = 0x8877665544332211                                      # differs in every byte
NP_OF_DST = {64: np.float64, 16: np.float32, 2: np.uint8}


def _volume(shape, kind, seed):
    """-> (raw [X, Y, Z] Fortran order, NIfTI code, scaling or None, element offset of the upload)"""
    rng = np.random.default_rng(seed)
    if kind in ("i2", "i2neg"):
        raw = rng.integers(-1200, 600, shape).astype(np.int16)
        return np.asfortranarray(raw), 4, ((0.5, -100.0) if kind == "i2" else (-1.5, 20.25)), 0
    if kind == "u1":
        return np.asfortranarray(rng.integers(0, 256, shape).astype(np.uint8)), 2, None, 1          # the byte type: off its alignment by one element
    if kind == "f4nan":
        raw = (rng.normal(size=shape) * 500).astype(np.float32)
        raw[rng.random(shape) < 0.15] = np.nan
        raw[:, 0, 0] = np.nan                                        # a whole NaN row
        if np.prod(shape) > 1:
            raw[-1, -1, -1] = np.inf
        return np.asfortranarray(raw), 16, None, 0
    return np.asfortranarray(rng.normal(size=shape) * 400 - 300), 64, None, 0


def _up(a, offset=0):
    """the bytes of volume `a` in Fortran order on the device, `offset` elements into a larger buffer -> (tensor kept alive, pointer)"""
    import torch
    a = np.asarray(a)
    flat = np.asfortranarray(a).reshape(-1, order="F").view(np.uint8)
    buf = torch.zeros(flat.size + 64 + offset * a.itemsize, dtype=torch.uint8, device="cuda")
    buf[offset * a.itemsize:offset * a.itemsize + flat.size] = torch.from_numpy(flat.copy()).cuda()
    return buf, buf.data_ptr() + offset * a.itemsize


def _matrices(src, out):
    """name -> M [3, 4]"""
    eye = np.eye(4)[:3]
    ms = {"identity": eye.copy(), "anisotropic": RS.anisotropic_matrix(), "oblique": RS.oblique_matrix()}
    m = eye.copy(); m[0, 3] = -70.0                                  # outputs x < 70 look left of the volume: whole waves outside
    ms["shift_waves_out"] = m
    m = eye.copy(); m[:, 3] = 4000.0                                 # every output outside
    ms["shift_all_out"] = m
    m = eye.copy(); m[:, 3] = 0.5                                    # t = 0.5 on every axis, and the tie of floor(s + 0.5)
    ms["half_voxel"] = m
    m = eye.copy(); m[:, 3] = -0.5
    ms["minus_half_voxel"] = m
    n = src
    ms["perm_x_from_y"] = np.array([[0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, n[1] - 1.0], [0.0, 0.0, 1.0, 0.0]])
    ms["perm_x_from_z"] = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, n[2] - 1.0]])
    ms["perm_cycle_flip"] = np.array([[0.0, -1.0, 0.0, n[0] - 1.0], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    ms["huge"] = np.array([[1e300, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, -1e300], [0.0, -1e300, 1e300, 1.0]])
    ms["huge_cancel"] = np.array([[1e300, -1e300, 0.0, 0.25], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])          # finite on the diagonal i = j of the output
    ms["overflow_inf"] = np.array([[1.7e308, 1.7e308, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])          # i = j = 1: the coordinate is +inf
    ms["overflow_nan"] = np.array([[1.7e308, -1.7e308, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -1.7e308, 0.0]])     # i, j >= 2: inf - inf; k >= 2: -inf
    return ms


def _permuted_outputs(src):
    """for the three permutations: the output shape that holds the whole permuted source (the axis that feeds source x is long: several tiles of the transposing kernel)"""
    return {"perm_x_from_y": (src[1], src[0], src[2]), "perm_x_from_z": (src[2], src[1], src[0]), "perm_cycle_flip": (src[2], src[0], src[1])}


def _cases(src):
    for out in OUTPUTS:
        for name, M in _matrices(src, out).items():
            yield out, name, M
    for name, out in _permuted_outputs(src).items():
        yield out, name + "/whole", _matrices(src, out)[name]
    for n in (15, 16):                                               # either side of the extent at which the transposing kernel takes over
        for name, out in (("perm_x_from_y", (3, n, 2)), ("perm_x_from_z", (3, 2, n)), ("oblique", (3, n, 2))):
            yield out, f"{name}/{n}", _matrices(src, out)[name]


def _out_buffer(nbytes):
    import torch
    return torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")


def _take(buf, nbytes, np_dtype, shape):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + nbytes:] == SENTINEL).all(), "a sentinel around the output was overwritten"
    return h[GUARD:GUARD + nbytes].copy().view(np_dtype).reshape(shape, order="F")


def _untouched(buf):
    return bool((buf.cpu().numpy() == SENTINEL).all())


def _mat(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).reshape(3, 4))


def _nearest(o, ptr, eb, src_shape, M, mode, bits, out_shape, np_dtype):
    import torch
    n = int(np.prod(out_shape)) * eb
    buf = _out_buffer(n)
    m = _mat(M)
    rc = o.lib.unet_vol_resample_nearest(o.h, ptr, eb, *src_shape, m.ctypes.data, mode, bits, buf.data_ptr() + GUARD, *out_shape, o.s)
    torch.cuda.synchronize()
    return rc, buf, (_take(buf, n, np_dtype, out_shape) if rc == 0 else None)


def _linear(o, ptr, vargs, M, mode, cval, out_shape, dst):
    import torch
    n = int(np.prod(out_shape)) * np.dtype(NP_OF_DST[dst]).itemsize
    buf = _out_buffer(n)
    m = _mat(M)
    rc = o.lib.unet_vol_resample_linear(o.h, ptr, *vargs, m.ctypes.data, mode, float(cval), buf.data_ptr() + GUARD, dst, *out_shape, o.s)
    torch.cuda.synchronize()
    return rc, buf, (_take(buf, n, NP_OF_DST[dst], out_shape) if rc == 0 else None)


def _vargs(raw, code, scaling):
    return (code,) + tuple(int(v) for v in raw.shape) + ((1, float(scaling[0]), float(scaling[1])) if scaling else (0, 1.0, 0.0))


# ---- unet_vol_resample_nearest ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eb", [1, 2, 4, 8])
@pytest.mark.parametrize("src", SOURCES)
def test_nearest_equals_the_oracle(src, eb):
    o = Ops()
    udt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[eb]
    raw = np.asfortranarray(np.random.default_rng(sum(src) + eb).integers(0, 2 ** (8 * eb), src, dtype=np.uint64).astype(udt))          # every bit pattern, NaNs among the doubles
    cval = np.array(CVAL_BITS & (2 ** (8 * eb) - 1), np.uint64).astype(udt)
    keep, ptr = _up(raw, 1 if eb == 1 else 0)
    for out, name, M in _cases(src):
        for mode in (0, 1):
            rc, _, got = _nearest(o, ptr, eb, src, M, mode, CVAL_BITS, out, udt)
            assert rc == 0, o.ctx.last_error()
            want = RS.nearest(raw, M, out, mode, cval)
            assert np.array_equal(got, want), f"{name} {src} -> {out} mode {mode}: {np.count_nonzero(got != want)} of {want.size} elements differ"
    del keep


def test_nearest_cases_reach_what_they_are_for():
    """the case list itself: whole waves outside, ties, both lane mappings, constant and clamped reads all occur"""
    src, out = (130, 3, 2), (130, 4, 2)
    ms = _matrices(src, out)
    s = RS.coords(ms["shift_waves_out"], out)[0]
    assert (s[:64] < -1).all() and (s[70:] >= 0).all()               # the first wave of every row loads nothing in mode 1
    s = RS.coords(ms["half_voxel"], out)[0]
    assert ((s + 0.5) == np.rint(s + 0.5)).all() and ((s - np.floor(s)) == 0.5).all()
    for name in ("perm_x_from_y", "perm_x_from_z", "perm_cycle_flip"):
        M = ms[name]
        assert int(np.argmax(np.abs(M[0, :3]))) != 0 and (np.abs(M[:, :3]).sum(axis=0) == 1).all() and (M[:, :3] < 0).any()
    got = RS.nearest(np.arange(780, dtype=np.int32).reshape(src, order="F"), ms["huge"], out, 1, -1)
    assert (got == -1).sum() > 0
    with np.errstate(over="ignore", invalid="ignore"):
        s = RS.coords(ms["overflow_inf"], (5, 4, 3))[0]
        assert np.isposinf(s[1, 1, 0]) and s[0, 0, 0] == 0.0
        s, sz = RS.coords(ms["overflow_nan"], (5, 4, 3))[0], RS.coords(ms["overflow_nan"], (5, 4, 3))[2]
        assert np.isnan(s[2, 2, 0]) and np.isneginf(sz[0, 0, 2])
    fd = np.arange(780, dtype=np.float64).reshape(src, order="F")
    for name in ("overflow_inf", "overflow_nan"):                    # an inf or NaN coordinate is outside: cval, not NaN, in both forms; the edge in mode 0
        lin, near = RS.linear(fd, ms[name], (5, 4, 3), 1, -7.5), RS.nearest(fd, ms[name], (5, 4, 3), 1, -7.5)
        assert not np.isnan(lin).any() and (lin[2:, 2:, :] == -7.5).all() and (near[2:, 2:, :] == -7.5).all() and lin[0, 0, 0] == fd[0, 0, 0]
        assert not np.isnan(RS.linear(fd, ms[name], (5, 4, 3), 0, -7.5)).any()
    assert RS.linear(fd, ms["overflow_inf"], (5, 4, 3), 0, 0.0)[1, 1, 0] == fd[129, 1, 0] and RS.linear(fd, ms["overflow_nan"], (5, 4, 3), 0, 0.0)[2, 2, 0] == fd[0, 2, 0]


# ---- unet_vol_resample_linear -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", STORAGE)
@pytest.mark.parametrize("src", SOURCES)
def test_linear_equals_the_oracle(src, kind):
    o = Ops()
    raw, code, scaling, off = _volume(src, kind, sum(src))
    fd = RS.decode(raw, scaling)
    keep, ptr = _up(raw, off)
    vargs = _vargs(raw, code, scaling)
    cval = -1000.25
    for out, name, M in _cases(src):
        for mode in (0, 1):
            ref = RS.linear(fd, M, out, mode, cval, 64)
            for dst in (64, 16, 2):
                rc, _, got = _linear(o, ptr, vargs, M, mode, cval, out, dst)
                assert rc == 0, o.ctx.last_error()
                want = ref if dst == 64 else (ref.astype(np.float32) if dst == 16 else (ref >= 0.5).astype(np.uint8))
                assert np.array_equal(got, want, equal_nan=dst != 2), \
                    f"{name} {kind} {src} -> {out} mode {mode} dst {dst}: {np.count_nonzero(~((got == want) | ((got != got) & (want != want))))} of {want.size} differ"
    del keep


@pytest.mark.parametrize("mode", [0, 1])
def test_linear_mask_cut_at_exactly_one_half(mode):
    """dst_dtype 2 on a 0 / 1 mask: a half-voxel shift along x puts the interpolant of every 0 | 1 pair at exactly 0.5, which counts as foreground"""
    o = Ops()
    src = (67, 5, 3)
    mask = np.asfortranarray((np.random.default_rng(11).random(src) < 0.5).astype(np.uint8))
    keep, ptr = _up(mask, 1)
    M = np.eye(4)[:3].copy(); M[0, 3] = 0.5
    ref = RS.linear(mask.astype(np.float64), M, src, mode, 0.0, 64)
    assert (ref == 0.5).sum() > 100
    rc, _, got = _linear(o, ptr, (2,) + src + (0, 1.0, 0.0), M, mode, 0.0, src, 2)
    assert rc == 0, o.ctx.last_error()
    assert np.array_equal(got, (ref >= 0.5).astype(np.uint8)) and (got[ref == 0.5] == 1).all()
    del keep


def test_a_nan_neighbour_wins_even_at_weight_zero():
    o = Ops()
    raw = np.asfortranarray(np.arange(24, dtype=np.float32).reshape((4, 3, 2), order="F"))
    raw[2, 1, 0] = np.nan
    keep, ptr = _up(raw)
    rc, _, got = _linear(o, ptr, (16, 4, 3, 2, 0, 1.0, 0.0), np.eye(4)[:3], 0, 0.0, (4, 3, 2), 64)
    assert rc == 0
    want = RS.linear(raw.astype(np.float64), np.eye(4)[:3], (4, 3, 2), 0, 0.0)
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[1, 1, 0]) and np.isnan(got[2, 0, 0]) and not np.isnan(got[3, 1, 0])
    del keep


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_output_untouched():
    import torch
    o = Ops()
    src, out = (5, 3, 2), (5, 4, 3)
    raw = np.asfortranarray(np.arange(30, dtype=np.int16).reshape(src, order="F"))
    keep, ptr = _up(raw)
    eye = np.eye(4)[:3]
    bad_ms = []
    for v in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (1, 3), (2, 2)):
            m = eye.copy(); m[at] = v
            bad_ms.append(m)
    n = int(np.prod(out))

    def near(src_shape=src, M=eye, mode=1, eb=2, out_shape=out, null_m=False):
        buf = _out_buffer(n * 8)
        m = _mat(M)
        rc = o.lib.unet_vol_resample_nearest(o.h, ptr, eb, *src_shape, None if null_m else m.ctypes.data, mode, CVAL_BITS, buf.data_ptr() + GUARD, *out_shape, o.s)
        torch.cuda.synchronize()
        return rc, buf

    def lin(src_shape=src, M=eye, mode=1, dtype=4, dst=64, out_shape=out, null_m=False):
        buf = _out_buffer(n * 8)
        m = _mat(M)
        rc = o.lib.unet_vol_resample_linear(o.h, ptr, dtype, *src_shape, 1, 0.5, -100.0, None if null_m else m.ctypes.data, mode, -7.0, buf.data_ptr() + GUARD, dst, *out_shape, o.s)
        torch.cuda.synchronize()
        return rc, buf

    for f in (near, lin):
        cases = [dict(M=m) for m in bad_ms] + [dict(null_m=True)]
        cases += [dict(out_shape=s) for s in ((0, 4, 3), (5, 0, 3), (5, 4, 0), (-1, 4, 3), (5, 4, -2), (2048, 2048, 512), (65536, 65536, 1))]
        cases += [dict(src_shape=s) for s in ((2048, 2048, 512), (-5, 3, 2), (5, 3, -2), (65536, 65536, 1), (65536, 65536, -1))]
        cases += [dict(mode=-1), dict(mode=2)]
        cases += [dict(src_shape=s, mode=0) for s in ((0, 3, 2), (5, 0, 2), (5, 3, 0))]          # no voxels and no edge to repeat
        cases += [dict(eb=e) for e in (0, 3, 16, -1)] if f is near else [dict(dtype=d) for d in (0, 7, 32, 1024)] + [dict(dst=d) for d in (0, 4, 8, 256)]
        for kw in cases:
            rc, buf = f(**kw)
            assert rc == E_ARG, f"{f.__name__} {kw}: rc {rc}"
            assert o.ctx.last_error()
            assert _untouched(buf), f"{f.__name__} {kw}: refused but wrote"
    # misaligned buffers
    buf = _out_buffer(n * 8)
    m = _mat(eye)
    assert o.lib.unet_vol_resample_nearest(o.h, ptr + 1, 2, *src, m.ctypes.data, 1, 0, buf.data_ptr() + GUARD, *out, o.s) == E_ARG
    assert o.lib.unet_vol_resample_nearest(o.h, ptr, 2, *src, m.ctypes.data, 1, 0, buf.data_ptr() + GUARD + 1, *out, o.s) == E_ARG
    assert o.lib.unet_vol_resample_linear(o.h, ptr, 4, *src, 0, 1.0, 0.0, m.ctypes.data, 1, 0.0, buf.data_ptr() + GUARD + 4, 64, *out, o.s) == E_ARG
    assert o.lib.unet_vol_resample_linear(o.h, ptr, 4, *src, 0, 1.0, 0.0, m.ctypes.data, 1, 0.0, None, 64, *out, o.s) == E_ARG
    torch.cuda.synchronize()
    assert _untouched(buf)
    del keep


@pytest.mark.parametrize("src", [(0, 3, 2), (5, 0, 2), (5, 3, 0), (0, 0, 0), (65536, 65536, 0), (0, 2147483647, 2147483647)])
def test_a_source_without_voxels_fills_with_cval_in_constant_mode(src):
    o = Ops()
    out = (67, 3, 2)
    for M in (np.eye(4)[:3], RS.oblique_matrix()):
        rc, _, got = _nearest(o, None, 4, src, M, 1, CVAL_BITS, out, np.uint32)
        assert rc == 0, o.ctx.last_error()
        assert (got == (CVAL_BITS & 0xFFFFFFFF)).all()
        for dst in (64, 16, 2):
            rc, _, got = _linear(o, None, (4,) + src + (1, 0.5, -100.0), M, 1, 3.5, out, dst)
            assert rc == 0, o.ctx.last_error()
            assert np.array_equal(got, RS.linear(np.zeros(tuple(min(n, 3) for n in src)), M, out, 1, 3.5, dst)) and (got == (3.5 if dst != 2 else 1)).all()          # (numpy refuses the huge empty shapes)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
E2E_SHAPE, E2E_PIX = (67, 9, 7), (0.7, 0.7, 2.5)
# a second grid over the same region: other voxels, turned by 10 degrees about z, stored "LPS" like the scan
OTHER_SHAPE, OTHER_AFFINE = (40, 6, 12), RS.oblique_affine((1.1, 0.9, 1.3), offset=(119.0, 95.0, -300.5)) @ np.diag([-1.0, -1.0, 1.0, 1.0])


def _ct():
    rng = np.random.default_rng(21)
    raw = np.asfortranarray(rng.integers(-1024, 3000, E2E_SHAPE).astype(np.int16))
    A = LO.affine_of(("L", "P", "S"), E2E_PIX); A[:3, 3] = (120.0, 95.5, -300.0)
    return raw, A


def test_resample_volume_spacing_shape_and_like(tmp_path):
    import torch
    from covidseg_amd import nifti_min
    from covidseg_amd import volume as V
    raw, A = _ct()
    scaling = (0.5, -100.0)
    fd = RS.decode(raw, scaling)
    vol = nifti_min.NiftiVolume(raw, scaling[0], scaling[1], E2E_PIX, nifti_min.header_with_affine(E2E_SHAPE, A), "<")
    # (a) a NiftiVolume to 1 mm: the stated shape, grid and matrix; float32 and float64; both modes (cval: the decoded minimum)
    res = V.resample_volume(vol, spacing=(1, 1, 1))
    assert res.grid.shape == (47, 6, 18) and res.grid.oriented and res.grid.axcodes == ("L", "P", "S") and res.data.dtype == np.float32 and res.data.flags.f_contiguous
    z = np.array([67 / 47, 9 / 6, 7 / 18])
    assert np.array_equal(res.matrix[:, :3], np.diag(z)) and np.array_equal(res.matrix[:, 3], 0.5 * z - 0.5)
    assert np.array_equal(res.data, RS.linear(fd, res.matrix, (47, 6, 18), 0, 0.0, 16))
    res64 = V.resample_volume(vol, spacing=(1, 1, 1), dtype="float64", mode="constant")
    assert np.array_equal(res64.data, RS.linear(fd, res.matrix, (47, 6, 18), 1, fd.min(), 64))
    # (b) a file (float32 voxels, the sform written by header_with_affine) to a shape, and out_path read back
    src_path, out_path = tmp_path / "ct.nii.gz", tmp_path / "ct_33.nii"
    nifti_min.write(src_path, fd.astype(np.float32), header=nifti_min.header_with_affine(E2E_SHAPE, A))
    f32 = fd.astype(np.float32).astype(np.float64)
    res = V.resample_volume(str(src_path), shape=(33, 9, 14), out_path=str(out_path))
    assert res.grid.shape == (33, 9, 14) and np.array_equal(res.data, RS.linear(f32, res.matrix, (33, 9, 14), 0, 0.0, 16))
    back = nifti_min.read(out_path)
    assert np.array_equal(back.raw, res.data) and back.affine_source == "sform"
    assert np.array_equal(back.affine[:3], res.grid.affine[:3].astype(np.float32).astype(np.float64))
    # (c) an array with affine= onto a second grid with a 10 degree oblique sform; the same from a device buffer, kept on the device
    other = V.Grid(OTHER_SHAPE, OTHER_AFFINE)
    res = V.resample_volume(raw, like=other, affine=A, mode="constant", cval=-1024.0, dtype="float64")
    M = (np.linalg.inv(A) @ other.affine)[:3]
    assert np.array_equal(res.matrix, M) and res.grid is other
    want = RS.linear(raw.astype(np.float64), M, other.shape, 1, -1024.0, 64)
    assert np.array_equal(res.data, want) and (want != -1024.0).mean() > 0.2
    dev = torch.from_numpy(raw.reshape(-1, order="F").copy()).cuda()
    rdev = V.resample_volume(dev, grid=other, affine=A, src_shape=E2E_SHAPE, mode="constant", cval=-1024.0, dtype="float64", return_device=True)
    assert rdev.data.is_cuda and rdev.data.dtype == torch.float64 and np.array_equal(rdev.data.cpu().numpy().reshape(other.shape, order="F"), want)
    # (d) nearest: the stored elements with their scaling, or decoded on the host
    rraw = V.resample_volume(vol, spacing=(1, 1, 1), order="nearest", dtype="raw", mode="constant")
    want_raw = RS.nearest(raw, rraw.matrix, (47, 6, 18), 1, raw.min())
    assert rraw.data.dtype == np.int16 and np.array_equal(rraw.data, want_raw) and (rraw.slope, rraw.inter) == scaling
    rdec = V.resample_volume(vol, spacing=(1, 1, 1), order="nearest", mode="constant")
    assert rdec.data.dtype == np.float32 and np.array_equal(rdec.data, RS.decode(want_raw, scaling).astype(np.float32))
    # an explicit cval is a DECODED value unless dtype is "raw": -1000.5 is no stored element of this volume (0.5 v - 100), and -1000 would decode to -600
    other = V.Grid(OTHER_SHAPE, OTHER_AFFINE)
    for cval in (-1000.5, -1000.0):
        for dtype in ("float64", "float32"):
            r = V.resample_volume(vol, like=other, order="nearest", mode="constant", cval=cval, dtype=dtype)
            want = RS.nearest(fd, r.matrix, other.shape, 1, cval)
            assert (want == cval).mean() > 0.2 and (want != cval).mean() > 0.2
            assert r.data.dtype == np.dtype(dtype) and np.array_equal(r.data, want.astype(dtype))
    rraw = V.resample_volume(vol, like=other, order="nearest", mode="constant", cval=-1000, dtype="raw")          # ... and a stored one with "raw"
    assert np.array_equal(rraw.data, RS.nearest(raw, rraw.matrix, other.shape, 1, -1000))


def test_reorient_volume_in_all_48_orientations():
    import torch
    from covidseg_amd import volume as V
    ras = np.random.default_rng(5).integers(-1000, 1000, (12, 10, 6)).astype(np.int16)
    pix_ras = np.array([0.7, 0.8, 2.5])
    for n, codes in enumerate(LO.all_axcodes()):
        stored = LO.reorient(ras, codes)
        res = V.reorient_volume(stored, "RAS", orientation=codes)
        assert res.data.dtype == np.int16 and np.array_equal(res.data, ras) and np.array_equal(res.data, LO.to_canonical(stored, codes))
        assert res.grid.axcodes == ("R", "A", "S")
        A = LO.affine_of(codes, LO.reorient_pixdim(pix_ras, codes)); A[:3, 3] = (3.0, -4.0, 5.0)
        if n % 3 == 0:                                               # from canonical to the codes, through an affine, from a device buffer
            dev = torch.from_numpy(ras.reshape(-1, order="F").copy()).cuda()
            res = V.reorient_volume(dev, codes, orientation=LO.affine_of(("R", "A", "S"), pix_ras), src_shape=ras.shape, return_device=True)
            assert np.array_equal(res.data.cpu().numpy().reshape(stored.shape, order="F"), stored) and res.grid.axcodes == tuple(codes)
            assert np.allclose(res.grid.pixdim, LO.reorient_pixdim(pix_ras, codes))
        else:
            res = V.reorient_volume(stored, "RAS", orientation=A)
            assert np.array_equal(res.data, ras) and np.allclose(res.grid.pixdim, pix_ras)
            # the world position of every voxel is kept: new affine @ new index == old affine @ old index
            old = np.linalg.inv(A) @ res.grid.affine @ np.array([1.0, 2.0, 3.0, 1.0])
            assert stored[tuple(np.rint(old[:3]).astype(int))] == ras[1, 2, 3]


def test_resample_mask_labels_and_change_between():
    import torch
    from covidseg_amd import volume as V
    rng = np.random.default_rng(31)
    _, A = _ct()
    g = np.meshgrid(*(np.arange(n) * p for n, p in zip(E2E_SHAPE, E2E_PIX)), indexing="ij")
    mask = (((g[0] - 20) / 12) ** 2 + ((g[1] - 3) / 2.5) ** 2 + ((g[2] - 8) / 6) ** 2 <= 1.0).astype(np.uint8) * 3          # non-zero = foreground
    mask[60:, :, :] = 1                                              # touches the border
    labels = (rng.integers(0, 5, E2E_SHAPE) * (rng.random(E2E_SHAPE) < 0.6)).astype(np.int32)
    labels[0, 0, 0] = 2 ** 31 - 1; labels[1, 0, 0] = -5
    m01 = (mask != 0).astype(np.uint8)
    for order in ("nearest", "linear"):
        res = V.resample_mask(mask, spacing=(1, 1, 1), order=order, pixdim=E2E_PIX)
        want = RS.nearest(m01, res.matrix, res.grid.shape, 0, 0) if order == "nearest" else RS.linear(m01.astype(np.float64), res.matrix, res.grid.shape, 0, 0.0, 2)
        assert res.data.dtype == np.uint8 and set(np.unique(res.data)) <= {0, 1} and np.array_equal(res.data, want) and not res.grid.oriented
    other = V.Grid(OTHER_SHAPE, OTHER_AFFINE)
    for order in ("nearest", "linear"):                              # another grid: background outside by default
        res = V.resample_mask(mask, like=other, order=order, affine=A)
        want = RS.nearest(m01, res.matrix, other.shape, 1, 0) if order == "nearest" else RS.linear(m01.astype(np.float64), res.matrix, other.shape, 1, 0.0, 2)
        assert np.array_equal(res.data, want) and want.any()
    res = V.resample_labels(labels, shape=(33, 9, 14), pixdim=E2E_PIX)
    assert res.data.dtype == np.int32 and np.array_equal(res.data, RS.nearest(labels, res.matrix, (33, 9, 14), 0, 0))
    res = V.resample_labels(torch.from_numpy(labels.reshape(-1, order="F").copy()).cuda(), grid=other, affine=A, src_shape=E2E_SHAPE, return_device=True)
    assert np.array_equal(res.data.cpu().numpy().reshape(other.shape, order="F"), RS.nearest(labels, res.matrix, other.shape, 1, 0))
    # change: b drawn on the oblique grid, a on the scan's
    gb = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in other.shape), indexing="ij")
    mask_b = (((gb[0] - 18) / 9) ** 2 + ((gb[1] - 3) / 2.5) ** 2 + ((gb[2] - 6) / 4) ** 2 <= 1.0).astype(np.uint8)
    ga = V.Grid(E2E_SHAPE, A)
    ch = V.change_between(m01, ga, mask_b, other)
    M = (np.linalg.inv(other.affine) @ A)[:3]
    b_on_a = RS.nearest(mask_b, M, E2E_SHAPE, 1, 0)
    counts = SO.confusion(b_on_a, m01)
    tp, fp, fn = (int(v) for v in counts.sum(axis=0))
    assert tp > 0 and fp > 0 and fn > 0
    assert np.array_equal(ch.matrix, M) and np.array_equal(ch.b_on_a, b_on_a) and np.array_equal(ch.per_slice, counts)
    assert (ch.persistent, ch.new, ch.resolved) == (tp, fp, fn) and ch.dice == 2 * tp / (2 * tp + fp + fn)
    ml = abs(np.linalg.det(A[:3, :3])) / 1000.0
    assert (ch.persistent_ml, ch.new_ml, ch.resolved_ml) == (tp * ml, fp * ml, fn * ml) and abs(ml - 0.7 * 0.7 * 2.5 / 1000.0) < 1e-15

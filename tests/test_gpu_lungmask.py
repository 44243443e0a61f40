"""GPU: unet_vol_threshold, unet_vol_geodesic_begin / _steps (csrc/kernels_lungmask.hip) and lungs.* against tests/lungmask_oracle.py, every comparison for equality,
every output of a direct call between sentinel bands.

Which cases reach which path.  The threshold takes its eight-voxel form when the source is aligned to 16 bytes (8 for the one-byte types) and mask and region to 8, and
the one-voxel form otherwise (a source one element into its buffer, a mask one byte into its own); a flat volume's last item is short when X Y Z is no multiple of 8.
The slice counts leave as one atomic per workgroup and trip while the workgroup's voxels lie in one slice (Z = 1; the large shapes) and voxel by voxel where it
straddles slices (Z = 2100 with 15 voxels per slice).  The growth packs sixteen voxels per lane with 16-byte accesses when X is a multiple of 16 (64, 128) and voxel by
voxel otherwise; X = 63 .. 65, 127 .. 129 and 200 put a row's end just short of, on and beyond a word."""
import numpy as np
import pytest
import torch

import later_trips as LT
import lungmask_oracle as LO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

CODES = {"u1": 2, "i1": 256, "i2": 4, "u2": 512, "i4": 8, "u4": 768, "f4": 16, "f8": 64}
BAND = 96                                                            # sentinel bytes / elements either side of an output (a multiple of 16: the alignment stays)
SENTINEL = 0xA5
COUNT_SENTINEL = 0x5A5A5A5A5A5A5A5A
XS = (1, 5, 63, 64, 65, 67, 129, 200)
GROW_XS = (63, 64, 65, 127, 128, 129, 200)
STRUCTURES = ((1, False), (2, False), (3, False), (1, True), (2, True))


def _flat(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1, order="F"))


def _volume(shape, dt, seed):
    rng = np.random.default_rng(seed)
    if dt[0] == "f":
        a = (rng.standard_normal(shape) * 300).astype(dt)
        f = a.reshape(-1)
        if f.size >= 8:
            f[rng.choice(f.size, max(3, f.size // 10), replace=False)] = rng.choice(np.array([np.nan, np.inf, -np.inf], dt), max(3, f.size // 10))
        return np.asfortranarray(a)
    info = np.iinfo(np.dtype(dt))
    lo, hi = (max(info.min, -1200), min(int(info.max), 600)) if info.min < 0 else (0, min(int(info.max), 1800))
    return np.asfortranarray(rng.integers(lo, hi + 1, shape).astype(dt))


def _threshold(ops, raw, scaling, lo, hi, region=None, counts=True, src_offset=0, out_offset=0):
    """-> (rc, mask, slice counts or None, whether every sentinel band survived); the source may start src_offset elements, the mask out_offset bytes into its buffer"""
    dt = raw.dtype
    eb, N, Z = dt.itemsize, raw.size, raw.shape[2]
    src = torch.zeros((N + src_offset) * eb + 16, dtype=torch.uint8, device="cuda")
    src[src_offset * eb:(src_offset + N) * eb] = torch.from_numpy(_flat(raw).view(np.uint8)).cuda()
    dst = torch.full((N + 2 * BAND + out_offset,), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((Z + 2 * BAND,), COUNT_SENTINEL, dtype=torch.int64, device="cuda")
    reg = None if region is None else ops.d(_flat(region), np.uint8)
    scaled, slope, inter = (1, scaling[0], scaling[1]) if scaling is not None else (0, 0.0, 0.0)
    rc = ops.lib.unet_vol_threshold(ops.h, src.data_ptr() + src_offset * eb, CODES[dt.str[1:]], *raw.shape, scaled, slope, inter, lo, hi, None if reg is None else reg.data_ptr(),
                                    dst.data_ptr() + BAND + out_offset, cnt.data_ptr() + 8 * BAND if counts else None, ops.s)
    torch.cuda.synchronize()
    host, ch = dst.cpu().numpy(), cnt.cpu().numpy()
    bands = bool((host[:BAND + out_offset] == SENTINEL).all() and (host[BAND + out_offset + N:] == SENTINEL).all() and (ch[:BAND] == COUNT_SENTINEL).all()
                 and (ch[BAND + Z:] == COUNT_SENTINEL).all() and (counts or (ch == COUNT_SENTINEL).all()))
    return rc, host[BAND + out_offset:BAND + out_offset + N].reshape(raw.shape, order="F"), (ch[BAND:BAND + Z] if counts else None), bands


def _check_threshold(ops, raw, scaling, lo, hi, region=None, **kw):
    rc, got, counts, bands = _threshold(ops, raw, scaling, lo, hi, region, **kw)
    want, wc = LO.threshold(LO.decode(raw, *(scaling if scaling is not None else (None, None))), lo, hi, region)
    assert rc == 0 and bands, (raw.shape, raw.dtype, scaling, lo, hi)
    assert np.array_equal(got, want), (raw.shape, raw.dtype, scaling, lo, hi, int(np.count_nonzero(got != want)))
    assert counts is None or np.array_equal(counts, wc), (raw.shape, raw.dtype)
    return want


# ---- the threshold --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(CODES))
def test_threshold_every_code_scaling_and_row_length(dt):
    """all eight codes; unscaled, scaled and a negative slope; X short of, on and beyond the vector width and the wave; edges exactly on a voxel's value: lo is in, hi out;
    NaN and +-inf in the float volumes; region null and given; the aligned and the one-voxel form"""
    ops = Ops()
    for xi, X in enumerate(XS):
        raw = _volume((X, 3, 2), dt, 10 * xi + len(dt))
        region = np.asfortranarray(np.random.default_rng(xi).random(raw.shape) < 0.6)
        for scaling in (None, (0.5, -1024.0), (-2.0, 100.5)):
            dec = LO.decode(raw, *(scaling if scaling is not None else (None, None)))
            fin = np.sort(dec[np.isfinite(dec)].reshape(-1))
            lo, hi = float(fin[fin.size // 4]), float(fin[(3 * fin.size) // 4])
            pairs = [(-np.inf, np.inf), (-np.inf, lo), (hi, np.inf)] + ([(lo, hi)] if lo < hi else [])
            for a, b in pairs:
                want = _check_threshold(ops, raw, scaling, a, b, None)
                _check_threshold(ops, raw, scaling, a, b, region)
                if np.isfinite(a):
                    assert want[dec == a].all()                       # the value on lo is in
                if np.isfinite(b):
                    assert not want[dec == b].any()                   # the value on hi is out
                assert not want[np.isnan(dec)].any()
            a, b = pairs[-1]
            _check_threshold(ops, raw, scaling, a, b, region, src_offset=1)          # a misaligned source
            _check_threshold(ops, raw, scaling, a, b, None, out_offset=1)            # a misaligned mask
            _check_threshold(ops, raw, scaling, a, b, region, counts=False)


def test_threshold_slice_counts_of_one_and_of_many_slices():
    ops = Ops()
    for shape, dt in (((65, 7, 1), "i2"), ((5, 3, 2100), "i2"), ((8, 4, 2100), "u1"), ((300, 40, 3), "f4")):
        raw = _volume(shape, dt, sum(shape))
        region = np.asfortranarray(np.random.default_rng(1).random(shape) < 0.5)
        for reg in (None, region):
            _check_threshold(ops, raw, None, -300.0 if dt != "u1" else 200.0, 250.0 if dt != "u1" else 1200.0, reg)
            _check_threshold(ops, raw, None, -np.inf, np.inf, reg, src_offset=1)


def test_threshold_refusals_launch_nothing():
    ops = Ops()
    raw = _volume((9, 5, 3), "i2", 3)
    for lo, hi in ((np.nan, 0.0), (0.0, np.nan), (1.0, 1.0), (2.0, 1.0), (np.inf, np.inf)):
        rc, got, counts, bands = _threshold(ops, raw, None, lo, hi)
        assert rc != 0 and bands and (got == SENTINEL).all() and (counts == COUNT_SENTINEL).all()
    rc, got, _, bands = _threshold(ops, np.zeros((0, 4, 4), np.int16, order="F"), None, 0.0, 1.0)          # a zero dimension touches nothing
    assert rc == 0 and bands


@pytest.mark.parametrize("case", ["vector", "one_voxel"])
def test_threshold_later_trips(case):
    """every workgroup of the bounded grid makes two trips and a ragged third (tests/test_lungmask_host.py asserts the shapes)"""
    ops = Ops()
    if case == "vector":
        shape, dt, off = LO.LATER_THRESHOLD_VEC, "u1", 0
        assert LT.shape_rule(-(-int(np.prod(shape)) // LO.TH_VEC), LO.TRIP)
    else:
        shape, dt, off = LO.LATER_THRESHOLD_ONE, "i2", 1
        assert LT.shape_rule(int(np.prod(shape)), LO.TRIP)
    rng = np.random.default_rng(9)
    raw = np.asfortranarray(rng.integers(0, 200, shape).astype(dt))
    region = np.asfortranarray(rng.random(shape) < 0.75)
    want = _check_threshold(ops, raw, (2.0, -100.0), 0.0, 250.0, region, src_offset=off)
    late = _flat(want)[(LO.TH_VEC if case == "vector" else 1) * LO.TRIP:]
    assert 0.25 * late.size < int(late.sum()) < 0.75 * late.size      # the later trips carry information


# ---- the growth -----------------------------------------------------------------------------------------------------------------------------------------------------
def _geodesic(ops, seeds, constraint, conn=1, planar=False, max_steps=None, chunk=32, offset=0):
    """the two entries as lungs.geodesic_device drives them, every output between sentinels -> (arrival, counts, bands, calls of _steps); offset: bytes the input masks
    and (twice) the arrival volume start into their buffers"""
    shape = seeds.shape
    X, Y, Z = shape
    N = seeds.size
    limit = LO.MAX_STEP if max_steps is None else max_steps
    sd = torch.zeros(N + offset + 16, dtype=torch.uint8, device="cuda"); cd = torch.zeros(N + offset + 16, dtype=torch.uint8, device="cuda")
    sd[offset:offset + N] = torch.from_numpy(_flat(seeds).astype(np.uint8) * 3).cuda()          # any non-zero byte is set
    cd[offset:offset + N] = torch.from_numpy(_flat(constraint).astype(np.uint8) * 255).cuda()
    arr = torch.full((2 * (N + 2 * BAND + offset),), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((limit + 1 + 2 * BAND,), COUNT_SENTINEL, dtype=torch.int64, device="cuda")
    wsb = int(ops.lib.unet_vol_geodesic_ws_bytes(X, Y, Z))
    ws = torch.full((wsb + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    ap, cp, wp = arr.data_ptr() + 2 * (BAND + offset), cnt.data_ptr() + 8 * BAND, ws.data_ptr() + BAND
    ops.ck(ops.lib.unet_vol_geodesic_begin(ops.h, sd.data_ptr() + offset, cd.data_ptr() + offset, X, Y, Z, ap, cp, wp, wsb, ops.s), "begin")
    calls, first, last = 0, 1, limit
    if int(cnt[BAND].item()) == 0:
        last = 0
    else:
        while first <= limit:
            n = min(chunk, limit - first + 1)
            ops.ck(ops.lib.unet_vol_geodesic_steps(ops.h, X, Y, Z, first, n, conn, 1 if planar else 0, ap, cp, wp, wsb, ops.s), "steps")
            calls += 1
            empty = np.flatnonzero(cnt[BAND + first:BAND + first + n].cpu().numpy() == 0)
            if empty.size:
                last = first + int(empty[0]) - 1
                break
            first += n
    ah, ch, wh = arr.cpu().numpy().view(np.uint16), cnt.cpu().numpy(), ws.cpu().numpy()
    written = min(limit, first + chunk - 1 if calls else 0)
    bands = bool((ah[:BAND + offset] == 0xA5A5).all() and (ah[BAND + offset + N:] == 0xA5A5).all() and (ch[:BAND] == COUNT_SENTINEL).all()
                 and (ch[BAND + written + 1:] == COUNT_SENTINEL).all() and (wh[:BAND] == SENTINEL).all() and (wh[BAND + wsb:] == SENTINEL).all())
    return ah[BAND + offset:BAND + offset + N].reshape(shape, order="F"), ch[BAND:BAND + last + 1], bands, calls


def _check_growth(ops, seeds, constraint, conn=1, planar=False, max_steps=None, chunk=32, offset=0):
    got, counts, bands, calls = _geodesic(ops, seeds, constraint, conn, planar, max_steps, chunk, offset)
    want, wc = LO.geodesic(seeds, constraint, conn, planar, max_steps)
    assert bands, (seeds.shape, conn, planar)
    assert np.array_equal(counts, wc), (seeds.shape, conn, planar, counts.tolist(), wc.tolist())
    assert np.array_equal(got, want), (seeds.shape, conn, planar, int(np.count_nonzero(got != want)))
    assert int(counts.sum()) == int((got < 0xFFFF).sum())
    return got, counts, calls


@pytest.mark.parametrize("X", GROW_XS)
def test_growth_every_structure_and_row_length(X):
    ops = Ops()
    rng = np.random.default_rng(X)
    shape = (X, 6, 5)
    constraint = np.asfortranarray(rng.random(shape) < 0.55)
    seeds = np.asfortranarray(rng.random(shape) < 0.01)
    seeds[0, 0, 0] = seeds[X - 1, 5, 4] = True
    seeds[X // 2, 3, 2] = constraint[X // 2, 3, 2] = True
    constraint[0, 0, 0] = False
    outside = seeds & ~constraint                                     # seeds outside the constraint are ignored
    assert outside.any()
    for conn, planar in STRUCTURES:
        got, _, _ = _check_growth(ops, seeds, constraint, conn, planar)
        assert (got[outside] == 0xFFFF).all()
        _check_growth(ops, seeds, constraint, conn, planar, offset=1)          # misaligned buffers: the voxel-by-voxel pack
    if X > 64:                                                        # contacts that exist only across a word boundary: along x, and along a diagonal
        x0, x1 = 60, min(X, 68) - 1
        line = np.zeros(shape, bool, order="F")
        line[x0:x1 + 1, 2, 2] = True
        s = np.zeros(shape, bool, order="F")
        s[x0, 2, 2] = True
        got, counts, _ = _check_growth(ops, s, line)
        assert got[x1, 2, 2] == x1 - x0 and np.array_equal(counts, [1] * (x1 - x0 + 1))
        s[x0, 2, 2], s[x1, 2, 2] = False, True                        # and back
        assert _check_growth(ops, s, line)[0][x0, 2, 2] == x1 - x0
        diag = np.zeros(shape, bool, order="F")
        diag[63, 1, 1] = diag[64, 2, 1] = diag[63, 3, 2] = True
        s = np.zeros(shape, bool, order="F")
        s[63, 1, 1] = True
        assert np.array_equal(_check_growth(ops, s, diag, 1)[1], [1])
        assert _check_growth(ops, s, diag, 2)[0][64, 2, 1] == 1 and _check_growth(ops, s, diag, 2)[0][63, 3, 2] == 0xFFFF
        assert _check_growth(ops, s, diag, 3)[0][63, 3, 2] == 2 and _check_growth(ops, s, diag, 2, True)[0][64, 2, 1] == 1


def test_growth_without_a_seed_makes_one_call():
    ops = Ops()
    constraint = np.asfortranarray(np.random.default_rng(2).random((65, 4, 3)) < 0.5)
    got, counts, calls = _check_growth(ops, np.zeros(constraint.shape, bool, order="F"), constraint)
    assert np.array_equal(counts, [0]) and calls == 0 and (got == 0xFFFF).all()
    seeds = np.asfortranarray(~constraint)                            # every seed outside the constraint
    got, counts, calls = _check_growth(ops, seeds, constraint)
    assert np.array_equal(counts, [0]) and calls == 0 and (got == 0xFFFF).all()


def test_growth_continues_over_chunks_and_stops_at_max_steps():
    """a serpentine corridor longer than two chunks: first_step continues; max_steps reached with voxels left; a second run bit for bit"""
    from covidseg_amd import lungs as L
    ops = Ops()
    c, s, length = LO.serpentine(67, 5)
    assert length - 1 > 2 * 32
    got, counts, calls = _check_growth(ops, s, c, chunk=32)
    assert calls == -(-length // 32) and np.array_equal(counts, np.ones(length)) and int(got.max()) == 0xFFFF and int(got[c != 0].max()) == length - 1
    for chunk in (1, 7, 300):
        again, ca, _ = _check_growth(ops, s, c, chunk=chunk)
        assert np.array_equal(again, got) and np.array_equal(ca, counts)
    part, cp, calls = _check_growth(ops, s, c, max_steps=70, chunk=32)
    assert calls == 3 and cp.size == 71 and int((part < 0xFFFF).sum()) == 71 and int((c != 0).sum()) > 71
    a1, c1 = L.geodesic_distance(s, c, chunk=16)                      # the public entry: the same volume and counts, twice
    a2, c2 = L.geodesic_distance(s, c, chunk=16)
    assert a1.dtype == np.uint16 and np.array_equal(a1, got) and np.array_equal(c1, counts) and np.array_equal(a1, a2) and np.array_equal(c1, c2)
    dev, cd = L.geodesic_distance(torch.from_numpy(_flat(s)).cuda(), torch.from_numpy(_flat(c)).cuda(), shape=s.shape, max_steps=70, return_device=True)
    assert dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy().view(np.uint16).reshape(s.shape, order="F"), part) and np.array_equal(cd, cp)


def test_growth_later_trips():
    ops = Ops()
    shape = LO.LATER_GROWTH
    assert LT.shape_rule(shape[1] * shape[2], LO.TRIP)
    rng = np.random.default_rng(4)
    constraint = np.asfortranarray(rng.random(shape) < 0.8)
    seeds = np.asfortranarray(rng.random(shape) < 0.02)
    got, counts, _ = _check_growth(ops, seeds, constraint, 1, False, max_steps=3)
    late = got[:, :, -(shape[2] // 3):]                               # rows the later trips reach
    assert counts.size == 4 and (late == 0).any() and (late == 3).any() and (late == 0xFFFF).any()


def test_growth_refusals_launch_nothing():
    ops = Ops()
    X, Y, Z = 9, 4, 3
    wsb = int(ops.lib.unet_vol_geodesic_ws_bytes(X, Y, Z))
    assert wsb == 4 * 16 * ((1 * Y * Z * 8 + 15) // 16) and ops.lib.unet_vol_geodesic_ws_bytes(0, 4, 4) == 0 and ops.lib.unet_vol_geodesic_ws_bytes(-1, 4, 4) == 0
    m = torch.ones(X * Y * Z, dtype=torch.uint8, device="cuda")
    arr = torch.full((2 * X * Y * Z,), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((16,), COUNT_SENTINEL, dtype=torch.int64, device="cuda")
    ws = torch.full((wsb,), SENTINEL, dtype=torch.uint8, device="cuda")
    lib, h = ops.lib, ops.h
    assert lib.unet_vol_geodesic_begin(h, m.data_ptr(), m.data_ptr(), X, Y, Z, arr.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb - 1, ops.s) != 0
    assert lib.unet_vol_geodesic_begin(h, m.data_ptr(), m.data_ptr(), X, Y, Z, arr.data_ptr(), cnt.data_ptr() + 4, ws.data_ptr(), wsb, ops.s) != 0
    assert lib.unet_vol_geodesic_begin(h, m.data_ptr(), m.data_ptr(), X, Y, Z, arr.data_ptr() + 1, cnt.data_ptr(), ws.data_ptr(), wsb, ops.s) != 0
    for first, n, conn, planar in ((0, 1, 1, 0), (1, 0, 1, 0), (65534, 2, 1, 0), (1, 1, 0, 0), (1, 1, 4, 0), (1, 1, 3, 1), (1, 1, 1, 2)):
        assert lib.unet_vol_geodesic_steps(h, X, Y, Z, first, n, conn, planar, arr.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb, ops.s) != 0
    assert lib.unet_vol_geodesic_steps(h, X, Y, Z, 1, 1, 1, 0, arr.data_ptr(), cnt.data_ptr(), ws.data_ptr(), wsb - 1, ops.s) != 0
    assert lib.unet_vol_geodesic_begin(h, None, None, 0, Y, Z, None, None, None, 0, ops.s) == 0          # a zero dimension touches nothing
    assert lib.unet_vol_geodesic_steps(h, X, 0, Z, 1, 1, 1, 0, None, None, None, 0, ops.s) == 0
    torch.cuda.synchronize()
    assert (arr.cpu().numpy() == SENTINEL).all() and (cnt.cpu().numpy() == COUNT_SENTINEL).all() and (ws.cpu().numpy() == SENTINEL).all()


# ---- the passes of lungs.py -----------------------------------------------------------------------------------------------------------------------------------------
def test_threshold_volume_reconstruct_and_body_mask():
    from covidseg_amd import lungs as L
    from covidseg_amd import nifti_min
    rng = np.random.default_rng(12)
    raw = _volume((67, 9, 5), "i2", 5)
    region = np.asfortranarray(rng.random(raw.shape) < 0.5)
    assert np.array_equal(L.threshold_volume(raw, hi=-100.0), LO.threshold(LO.decode(raw), None, -100.0)[0])
    assert np.array_equal(L.threshold_volume(raw, lo=-100.0, hi=200.0, region=region.astype(np.uint8)), LO.threshold(LO.decode(raw), -100.0, 200.0, region)[0])
    vol = nifti_min.NiftiVolume(raw, 0.5, -10.0, (1.0, 1.0, 1.0), nifti_min.default_header(raw.shape), "<")
    assert np.array_equal(L.threshold_volume(vol, lo=-100.0), LO.threshold(LO.decode(raw, 0.5, -10.0), -100.0)[0])
    dev = L.threshold_volume(torch.from_numpy(_flat(raw)).cuda(), hi=0.0, src_shape=raw.shape, return_device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().reshape(raw.shape, order="F"), LO.threshold(LO.decode(raw), None, 0.0)[0])
    mask = np.asfortranarray(rng.random((33, 12, 7)) < 0.3)
    marker = np.asfortranarray(rng.random(mask.shape) < 0.02)
    for conn in (1, 2, 3):
        assert np.array_equal(L.reconstruct(mask, marker, conn), LO.reconstruct(mask, marker, conn))
    assert not L.reconstruct(mask, np.zeros(mask.shape, np.uint8)).any() and not L.reconstruct(np.zeros(mask.shape, np.uint8), marker).any()
    ph = _phantom(False, "z-")[0]
    assert np.array_equal(L.body_mask(ph["hu"]), LO.body_mask(LO.decode(ph["hu"])))


# ---- the procedure --------------------------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}
CODES_OF = {"z-": "LPI", "z+": "LPS"}


def _phantom(leak, superior):
    """the phantom and the oracle's result on it, computed once"""
    key = (leak, superior)
    if key not in _CACHE:
        ph = LO.phantom(leak=leak, superior=superior)
        v = LO.decode(ph["hu"])
        _CACHE[key] = (ph, LO.lung_mask(v, ph["pixdim"], superior), LO.lung_mask(v, ph["pixdim"], None))
    return _CACHE[key]


def _same_result(got, want, ph):
    assert got.mask.dtype == np.uint8 and np.array_equal(got.mask, want["mask"])
    assert got.shape == ph["hu"].shape and got.pixdim == ph["pixdim"] and got.method == "threshold"
    assert [int(v) for v in got.components["label"]] == want["kept"] and [int(v) for v in got.components["voxels"]] == want["voxels"]
    assert got.lung_ml == int(want["mask"].sum()) * float(np.prod(ph["pixdim"])) / 1000.0
    if want["airways"] is None:
        assert got.airways is None
    else:
        a, w = got.airways, want["airways"]
        assert np.array_equal(a.mask, w["mask"]) and np.array_equal(a.counts, w["counts"]) and a.leak_step == w["leak_step"] and a.stop_step == w["stop_step"]


@pytest.mark.parametrize("superior", ["z-", "z+"])
@pytest.mark.parametrize("leak", [False, True])
def test_lung_mask_on_the_phantoms(leak, superior):
    from covidseg_amd import lungs as L
    ph, want, plain = _phantom(leak, superior)
    hu = np.asfortranarray(ph["hu"])
    for airways in ("auto", True):
        got = L.lung_mask(hu, pixdim=ph["pixdim"], orientation=CODES_OF[superior], airways=airways)
        _same_result(got, want, ph)
        assert got.airway_error is None and (got.airways.leak_step is not None) == leak and len(got.components) == 2
    off = L.lung_mask(hu, pixdim=ph["pixdim"], orientation=CODES_OF[superior], airways=False)
    _same_result(off, plain, ph)
    assert off.airway_error is None and off.airways is None


def test_lung_mask_from_a_file_a_device_buffer_and_without_orientation(tmp_path):
    from covidseg_amd import lungs as L
    from covidseg_amd import nifti_min
    ph, want, plain = _phantom(True, "z-")
    hu = np.asfortranarray(ph["hu"])
    path = tmp_path / "ct.nii.gz"                                     # float32 HU with an sform: the pixdim and the axis codes come from the file
    nifti_min.write(path, hu.astype(np.float32), nifti_min.header_with_affine(hu.shape, nifti_min.affine_from_axcodes("LPI", ph["pixdim"])))
    out = tmp_path / "lungs.nii.gz"
    got = L.lung_mask(path, out_path=out)
    _same_result(got, want, ph)
    assert np.array_equal(nifti_min.read(out).raw, want["mask"]) and nifti_min.read(out).axcodes == ("L", "P", "I")
    dev = L.lung_mask(torch.from_numpy(_flat(hu)).cuda(), src_shape=hu.shape, pixdim=ph["pixdim"], orientation="LPI", return_device=True)
    assert dev.mask.is_cuda and np.array_equal(dev.mask.cpu().numpy().reshape(hu.shape, order="F"), want["mask"])
    assert np.array_equal(dev.airways.mask.cpu().numpy().reshape(hu.shape, order="F"), want["airways"]["mask"]) and dev.airways.stop_step == want["airways"]["stop_step"]
    none = L.lung_mask(hu, pixdim=ph["pixdim"])                       # no orientation: the step is skipped and says why
    _same_result(none, plain, ph)
    assert "orientation" in none.airway_error and len(none.components) == 1
    side = L.lung_mask(hu, pixdim=ph["pixdim"], orientation="LSP")    # axis 2 is no S / I axis
    assert "axis 2" in side.airway_error and np.array_equal(side.mask, plain["mask"])
    small = L.lung_mask(hu, pixdim=ph["pixdim"], orientation="LPI", area_mm2=(1.0, 20.0))          # no trachea of that area
    assert "no trachea" in small.airway_error and small.airways is None and np.array_equal(small.mask, plain["mask"])
    with pytest.raises(L.LungMaskError, match="trachea"):
        L.lung_mask(hu, pixdim=ph["pixdim"], orientation="LPI", area_mm2=(1.0, 20.0), airways=True)
    with pytest.raises(L.LungMaskError, match="min_lung_ml"):
        L.lung_mask(hu, pixdim=ph["pixdim"], orientation="LPI", min_lung_ml=1e6)
    closed = L.lung_mask(hu, pixdim=ph["pixdim"], orientation="LPI", close_mm=4.0, airway_dilate_mm=2.5, fill=False)
    v = LO.decode(ph["hu"])
    assert np.array_equal(closed.mask, LO.lung_mask(v, ph["pixdim"], "z-", close_mm=4.0, airway_dilate_mm=2.5, fill=False)["mask"])


def _model():
    from covidseg_amd.keras_like import UNetModel
    model = UNetModel(64, 1, seed=1)
    model.verbose = 0
    return model


def _ct_volume(ph):
    from covidseg_amd import nifti_min
    hu = np.asfortranarray(ph["hu"])
    return nifti_min.NiftiVolume(hu, 0.0, 0.0, ph["pixdim"], nifti_min.header_with_affine(hu.shape, nifti_min.affine_from_axcodes("LPI", ph["pixdim"])), "<")


def test_lung_mask_from_a_lung_unet():
    """a small randomly initialised U-Net: the procedure on ITS candidates equals the oracle applied to the same probabilities (thresholded at their median)"""
    from covidseg_amd import lungs as L
    from covidseg_amd import volume as V
    ph = _phantom(False, "z-")[0]
    vol, model = _ct_volume(ph), _model()
    t = float(np.median(model.predict(V.load_volume(vol, "cts", img_size=128, trim=(0, 1), new_dim=64), batch_size=8)))
    cand = L._model_candidates(vol, model, t, 8, 128, {}).cpu().numpy().reshape(ph["hu"].shape, order="F")
    assert 0 < int(cand.sum()) < cand.size
    want = LO.lung_mask(LO.decode(ph["hu"]), ph["pixdim"], "z-", candidates=cand)
    print(f"model candidates: {int(cand.sum())} voxels at threshold {t!r}; the oracle on them: error {want['error']!r}, airway_error {want['airway_error']!r}, kept {want['voxels']}")
    if want["error"] is not None:
        with pytest.raises(L.LungMaskError):
            L.lung_mask(vol, model=model, threshold=t, batch_size=8, img_size=128)
        return
    got = L.lung_mask(vol, model=model, threshold=t, batch_size=8, img_size=128)
    assert got.method == "model" and np.array_equal(got.mask, want["mask"]) and [int(v) for v in got.components["voxels"]] == want["voxels"]
    assert (got.airways is None) == (want["airways"] is None) and (got.airways is None or np.array_equal(got.airways.mask, want["airways"]["mask"]))


# ---- segment_volume(lungs=) -----------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, path="res"):
    """two results field by field; the times are not compared"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, path
        if a.dtype.names:
            for k in a.dtype.names:
                _same(a[k], b[k], f"{path}[{k}]")
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), path
    elif isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            if k != "seconds":
                _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, float):
        assert isinstance(b, float) and (a == b or (a != a and b != b)), path
    elif hasattr(a, "__dict__") and not callable(a):
        assert type(a) is type(b), path
        _same(vars(a), vars(b), path)
    else:
        assert a == b, path


def test_segment_volume_computes_the_lung_mask_first():
    from covidseg_amd import lungs as L
    from covidseg_amd import volume as V
    ph = _phantom(False, "z-")[0]
    vol, model = _ct_volume(ph), _model()
    t = float(np.median(model.predict(V.load_volume(vol, "cts", img_size=128, new_dim=64), batch_size=8)))
    kw = dict(threshold=t, batch_size=8, img_size=128, lesions=True, per_lung=True, distribution=True, density=True)
    lm = L.lung_mask(vol)
    assert np.array_equal(lm.mask, _phantom(False, "z-")[1]["mask"])
    given = V.segment_volume(vol, model, lung_mask=lm.mask, **kw)
    found = V.segment_volume(vol, model, lungs=True, **kw)
    assert given.per_lung is not None and given.distribution is not None and given.lung_ml is not None
    assert isinstance(found.lungs, L.LungMask) and np.array_equal(found.lungs.mask, lm.mask) and found.seconds["lungs"] > 0 and not hasattr(given, "lungs")
    rest = {k: v for k, v in vars(found).items() if k != "lungs"}
    _same(rest, vars(given))
    tuned = V.segment_volume(vol, model, lungs=dict(airways=False, min_ratio=0.5), **kw)
    _same({k: v for k, v in vars(tuned).items() if k != "lungs"}, vars(V.segment_volume(vol, model, lung_mask=L.lung_mask(vol, airways=False, min_ratio=0.5).mask, **kw)))
    assert tuned.lungs.airways is None and len(tuned.lungs.components) == 1
    _same(vars(V.segment_volume(vol, model, lungs=None, threshold=t, batch_size=8, img_size=128)), vars(V.segment_volume(vol, model, threshold=t, batch_size=8, img_size=128)))
    eg = V.segment_volume_ensemble(vol, [model], tta=("id", "hflip"), lung_mask=lm.mask, **kw)
    ef = V.segment_volume_ensemble(vol, [model], tta=("id", "hflip"), lungs=True, **kw)
    assert np.array_equal(ef.lungs.mask, lm.mask) and ef.seconds["lungs"] > 0
    _same({k: v for k, v in vars(ef).items() if k != "lungs"}, vars(eg))

"""GPU: unet_vol_hessian_eig, unet_vol_vesselness (csrc/kernels_vessel.hip) and vessels.* against tests/vessel_oracle.py, every comparison for equality -- float32 bits for
the eigenvalues and the response with the NaN positions equal, the scale element for element --, every output of a direct call between sentinel bands.

Which cases reach which path.  A workgroup walks bricks of 32 x 8 x 8 voxels staged with a halo of 1: (1, 1, 1) and (2, 1, 3) read nothing but the repeated edge voxel,
(33, 9, 9) is one voxel past a brick on every axis, (64, 16, 16) holds eight bricks of which the region covers some wholly, some partly and some not at all (those are
left before staging), and (2, 2, 8 (2 GRID_CAP + 3)) makes every workgroup of the bounded grid walk its loop at least twice.  The direct calls are fed noise volumes --
the entries' definition does not ask that L be smooth --, the end-to-end calls the phantom of the oracle through filters.gaussian_filter."""
import os
import re

import numpy as np
import pytest
import torch

import later_trips as LT
import lungmask_oracle as LO
import vessel_oracle as VO
from gpu_util import Ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 96                                                            # sentinel elements either side of an output
SENTINEL = 0xA5
E_ARG = -1
VS_GRID_CAP = 256 * 8                                                 # kernels_vessel.hip: GRID_CAP, restated; test_later_trips holds the file's text to it
ISO, ANISO = (1.0, 1.0, 1.0), (0.8, 0.8, 2.0)
DENS = VO.denominators()


def _flat(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1, order="F"))


def _same_bits(got, want, what):
    """float32 arrays: NaNs at the same positions, the same bits everywhere else"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), (what, int(ng.sum()), int(nw.sum()))
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nw
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def _eig(ops, L32, k, region=None):
    """-> (rc, eigenvalues float32 [3, X, Y, Z], whether both sentinel bands survived)"""
    shape, N = L32.shape, L32.size
    src = ops.d(_flat(L32), np.float32)
    reg = None if region is None else ops.d(_flat(region), np.uint8)
    buf = torch.full((4 * (3 * N + 2 * BAND),), SENTINEL, dtype=torch.uint8, device="cuda")
    kk = np.ascontiguousarray(k, np.float64)
    rc = ops.lib.unet_vol_hessian_eig(ops.h, src.data_ptr(), *shape, kk.ctypes.data, None if reg is None else reg.data_ptr(), buf.data_ptr() + 4 * BAND, ops.s)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    bands = bool((host[:4 * BAND] == SENTINEL).all() and (host[4 * (BAND + 3 * N):] == SENTINEL).all())
    e = host[4 * BAND:4 * (BAND + 3 * N)].view(np.float32).reshape(3, N)
    return rc, np.stack([v.reshape(shape, order="F") for v in e]), bands


def _vesselness(ops, volumes, ks, dens=DENS, bright=True, region=None, first_index=0):
    """the scales one after the other into one pair of buffers -> (rcs, best float32, scale uint8, bands)"""
    shape, N = volumes[0].shape, volumes[0].size
    reg = None if region is None else ops.d(_flat(region), np.uint8)
    best = torch.full((4 * (N + 2 * BAND),), SENTINEL, dtype=torch.uint8, device="cuda")
    scale = torch.full((N + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    rcs = []
    for i, (L32, k) in enumerate(zip(volumes, ks)):
        src = ops.d(_flat(L32), np.float32)
        kk = np.ascontiguousarray(k, np.float64)
        rcs.append(ops.lib.unet_vol_vesselness(ops.h, src.data_ptr(), *shape, kk.ctypes.data, None if reg is None else reg.data_ptr(), dens[0], dens[1], dens[2],
                                               1 if bright else 0, first_index + i, best.data_ptr() + 4 * BAND, scale.data_ptr() + BAND, ops.s))
        torch.cuda.synchronize()
    bh, sh = best.cpu().numpy(), scale.cpu().numpy()
    bands = bool((bh[:4 * BAND] == SENTINEL).all() and (bh[4 * (BAND + N):] == SENTINEL).all() and (sh[:BAND] == SENTINEL).all() and (sh[BAND + N:] == SENTINEL).all())
    return rcs, bh[4 * BAND:4 * (BAND + N)].view(np.float32).reshape(shape, order="F"), sh[BAND:BAND + N].reshape(shape, order="F"), bands


def _check_both(ops, L32, k, region=None, bright=True, what=""):
    """both entries on one volume against the oracle -> (eigenvalues, response)"""
    rc, e, bands = _eig(ops, L32, k, region)
    assert rc == 0 and bands, what
    _same_bits(e, VO.eigenvalues(L32, k, region), ("eig", what))
    rcs, best, scale, bands = _vesselness(ops, [L32], [k], bright=bright, region=region)
    want = VO.response(L32, k, DENS, bright, region)
    assert rcs == [0] and bands, what
    _same_bits(best, want, ("response", what))
    assert np.array_equal(scale, (want > 0).astype(np.uint8)), what
    return e, best


def _region_of_bricks(seed):
    """(64, 16, 16) = 2 x 2 x 2 bricks: two covered wholly, three partly (one by a single voxel in its far corner), three not at all"""
    rng = np.random.default_rng(seed)
    r = np.zeros((64, 16, 16), np.uint8)
    r[:32, :8, :8] = 1
    r[32:, 8:, 8:] = 7                                                # (non-zero = takes part)
    r[32:, :8, :8] = rng.random((32, 8, 8)) < 0.4
    r[:32, 8:, :8] = rng.random((32, 8, 8)) < 0.05
    r[31, 7, 15] = 1
    return r


@pytest.mark.parametrize("pixdim", [ISO, ANISO], ids=["iso", "aniso"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 3), (33, 9, 9), (31, 8, 17)])
def test_entries_equal_the_oracle(shape, pixdim):
    ops = Ops()
    k = VO.hessian_factors(1.5, pixdim)
    a = VO.noise_volume(shape, 11 + shape[0])
    e, best = _check_both(ops, a, k, what=(shape, pixdim))
    if a.size > 100:
        assert (best > 0).any() and (best == 0).any()
    _check_both(ops, a, k, bright=False, what=(shape, pixdim, "dark"))


def test_region_covers_bricks_wholly_partly_and_not_at_all():
    ops = Ops()
    a = VO.noise_volume((64, 16, 16), 21)
    region = _region_of_bricks(22)
    k = VO.hessian_factors(2.0, ANISO)
    e, best = _check_both(ops, a, k, region, what="region")
    out = region == 0
    assert (e.view(np.uint32)[:, out] == 0).all() and (best.view(np.uint32)[out] == 0).all() and (best[~out] > 0).any()          # +0.0 outside, bit for bit
    # a later scale leaves the outside as the first one initialised it, empty bricks included
    b = VO.noise_volume((64, 16, 16), 23)
    rcs, best, scale, bands = _vesselness(ops, [a, b], [k, VO.hessian_factors(3.0, ANISO)], region=region)
    wb, ws = VO.multi_scale([VO.response(a, k, DENS, True, region), VO.response(b, VO.hessian_factors(3.0, ANISO), DENS, True, region)])
    assert rcs == [0, 0] and bands
    _same_bits(best, wb, "two scales under a region")
    assert np.array_equal(scale, ws) and (scale[out] == 0).all() and (best[out] == 0).all() and (scale == 2).any()


def test_later_trips():
    """every workgroup of the bounded grid walks its brick loop at least twice; the cap is read out of the source so that a changed cap fails here instead of disarming
    the case"""
    src = open(os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc", "kernels_vessel.hip")).read()
    cap = LT.constant_value(re.search(r"constexpr long long GRID_CAP = ([^;]+);", src).group(1))
    assert cap == VS_GRID_CAP
    assert LT.constant_value(re.search(r"constexpr int TPB = ([^;]+);", src).group(1)) == LT.TPB
    assert re.search(r"constexpr int BX = 32, BY = 8, BZ = 8,", src)
    shape = (2, 2, 8 * (2 * VS_GRID_CAP + 3))
    bricks = shape[2] // 8
    assert LT.later_trips(bricks, VS_GRID_CAP) == (2, 3)
    ops = Ops()
    a = VO.noise_volume(shape, 31)
    region = (np.random.default_rng(32).random(shape) < 0.7).astype(np.uint8)
    region[:, :, 8 * 5:8 * 9] = 0                                     # a few empty bricks on the way
    k = VO.hessian_factors(1.0, ANISO)
    _check_both(ops, a, k, what="later trips")
    _check_both(ops, a, k, region, what="later trips, region")


def _grid(shape):
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")


def test_polynomials_are_exact():
    ops = Ops()
    shape = (35, 10, 9)
    x, y, z = _grid(shape)
    k = VO.hessian_factors(1.0, ISO)
    inner = (slice(1, -1),) * 3
    for name, f, want in (("x2", x * x, (0.0, 0.0, 2.0)), ("xy", x * y, (0.0, -1.0, 1.0)), ("r2", (x * x + y * y) + z * z, (2.0, 2.0, 2.0)),
                          ("ramp", (x + 2.0 * y) + 3.0 * z, (0.0, 0.0, 0.0)), ("const", np.full(shape, 7.0), (0.0, 0.0, 0.0))):
        e, best = _check_both(ops, f.astype(np.float32), k, what=name)
        for i in range(3):
            assert (e[i][inner] == np.float32(want[i])).all(), (name, i)
        assert (best[inner] == 0).all(), name
    e, _ = _check_both(ops, ((x + 2.0 * y) + 3.0 * z).astype(np.float32), k, what="ramp faces")
    assert tuple(e[:, 0, 2, 2]) == (0.0, 0.0, 1.0) and tuple(e[:, 34, 2, 2]) == (0.0, 0.0, -1.0) and tuple(e[:, 0, 0, 0]) == (1.0, 2.0, 3.0)


def test_nan_and_inf_voxels():
    ops = Ops()
    a = VO.noise_volume((34, 9, 10), 41)
    a[31, 7, 8] = np.nan                                              # next to a brick's corner: its neighbourhood lies in eight bricks
    a[3, 2, 4] = np.inf
    k = VO.hessian_factors(1.5, ANISO)
    e, best = _check_both(ops, a, k, what="nan / inf")
    want = np.zeros(a.shape, bool)
    for cx, cy, cz in ((31, 7, 8), (3, 2, 4)):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    if abs(dx) + abs(dy) + abs(dz) <= 2:
                        want[cx + dx, cy + dy, cz + dz] = True
    assert np.array_equal(np.isnan(e[0]), want) and np.array_equal(np.isnan(e[1]), want) and np.array_equal(np.isnan(e[2]), want)
    assert (e.view(np.uint32)[:, want] == VO.QNAN_BITS).all()
    assert (best[want] == 0).all() and np.isfinite(best).all()
    # such a voxel never becomes a best scale, whichever scale it is not finite at
    b = VO.noise_volume(a.shape, 42)
    for vols in ([a, b], [b, a]):
        ks = [k, VO.hessian_factors(2.5, ANISO)]
        rcs, best, scale, bands = _vesselness(ops, vols, ks)
        wb, ws = VO.multi_scale([VO.response(v, kk, DENS) for v, kk in zip(vols, ks)])
        assert rcs == [0, 0] and bands
        _same_bits(best, wb, "nan / inf, two scales")
        assert np.array_equal(scale, ws)
        bad_at = 1 if vols[0] is a else 2
        assert (scale[want] != bad_at).all()


def test_dark_tubes_are_bright_tubes_of_the_negated_volume():
    ops = Ops()
    a = VO.noise_volume((40, 11, 9), 51)
    k = VO.hessian_factors(1.0, ANISO)
    _, bright, s1, _ = _vesselness(ops, [a], [k], bright=True)
    _, dark, s2, _ = _vesselness(ops, [-a], [k], bright=False)
    assert (bright > 0).any() and np.array_equal(bright.view(np.uint32), dark.view(np.uint32)) and np.array_equal(s1, s2)


def test_three_scales_ties_and_strict_wins():
    ops = Ops()
    shape = (36, 12, 10)
    a, b = VO.noise_volume(shape, 61), VO.noise_volume(shape, 62)
    a[:12] = 250.0                                                    # a constant part: response 0 at every scale, scale 0
    b[:12] = -40.0
    ks = [VO.hessian_factors(s, ANISO) for s in (1.0, 2.0, 3.0)]
    # the second scale repeats the first (every voxel ties: scale stays 1), the third wins strictly somewhere
    vols, kk = [a, a, b], [ks[0], ks[0], ks[2]]
    rcs, best, scale, bands = _vesselness(ops, vols, kk)
    wb, ws = VO.multi_scale([VO.response(v, k, DENS) for v, k in zip(vols, kk)])
    assert rcs == [0, 0, 0] and bands
    _same_bits(best, wb, "three scales")
    assert np.array_equal(scale, ws)
    assert (scale[:11] == 0).all() and (best[:11] == 0).all() and not (scale == 2).any() and (scale == 1).any() and (scale == 3).any()
    # three different scales
    vols = [a, b, VO.noise_volume(shape, 63)]
    rcs, best, scale, bands = _vesselness(ops, vols, ks)
    wb, ws = VO.multi_scale([VO.response(v, k, DENS) for v, k in zip(vols, ks)])
    assert rcs == [0, 0, 0] and bands
    _same_bits(best, wb, "three scales")
    assert np.array_equal(scale, ws) and set(np.unique(scale)) == {0, 1, 2, 3}
    # the largest index the entry takes writes 254
    rcs, best, scale, bands = _vesselness(ops, [a], [ks[0]], first_index=253)          # (over the sentinel, a tiny negative float32: every response replaces it)
    assert rcs == [0] and bands and (scale == 254).all()
    _same_bits(best, VO.response(a, ks[0], DENS), "index 253")


def test_two_runs_give_the_same_bits():
    ops = Ops()
    a = VO.noise_volume((70, 19, 17), 71)
    region = (np.random.default_rng(72).random(a.shape) < 0.5).astype(np.uint8)
    k = VO.hessian_factors(2.0, ANISO)
    r1, r2 = _eig(ops, a, k, region), _eig(ops, a, k, region)
    assert r1[0] == r2[0] == 0 and np.array_equal(r1[1].view(np.uint32), r2[1].view(np.uint32))
    v1, v2 = _vesselness(ops, [a, -a], [k, k], region=region), _vesselness(ops, [a, -a], [k, k], region=region)
    assert np.array_equal(v1[1].view(np.uint32), v2[1].view(np.uint32)) and np.array_equal(v1[2], v2[2])


def test_every_refusal():
    """UNET_E_ARG before any launch: the outputs keep their sentinels"""
    ops = Ops()
    shape = (5, 4, 3)
    N = 60
    a = ops.d(_flat(VO.noise_volume(shape, 81)), np.float32)
    reg = ops.d(np.ones(N), np.uint8)
    k = np.ascontiguousarray(VO.hessian_factors(1.0, ANISO), np.float64)
    eig = torch.full((4 * 3 * N,), SENTINEL, dtype=torch.uint8, device="cuda")
    best = torch.full((4 * N,), SENTINEL, dtype=torch.uint8, device="cuda")
    scale = torch.full((N,), SENTINEL, dtype=torch.uint8, device="cuda")
    lib, h, s = ops.lib, ops.h, ops.s

    def e(L=a.data_ptr(), shp=shape, kk=k, region=None, out=eig.data_ptr()):
        return lib.unet_vol_hessian_eig(h, L, *shp, None if kk is None else kk.ctypes.data, region, out, s)

    def v(L=a.data_ptr(), shp=shape, kk=k, region=None, dens=DENS, bright=1, index=0, b=best.data_ptr(), sc=scale.data_ptr()):
        return lib.unet_vol_vesselness(h, L, *shp, None if kk is None else kk.ctypes.data, region, dens[0], dens[1], dens[2], bright, index, b, sc, s)

    def factors(i, value):
        kk = k.copy(); kk[i] = value
        return kk

    assert e() == 0 and v() == 0                                      # (the arguments the refusals vary are good ones)
    torch.cuda.synchronize()
    eig.fill_(SENTINEL); best.fill_(SENTINEL); scale.fill_(SENTINEL)
    both = [dict(L=None), dict(kk=None), dict(L=a.data_ptr() + 2), dict(shp=(0, 4, 3)), dict(shp=(5, -1, 3)), dict(shp=(5, 4, 0)), dict(shp=(2048, 2048, 512)),
            dict(shp=(65536, 65536, 1))]
    both += [dict(kk=factors(i, bad)) for i in range(6) for bad in (0.0, -1.0, np.inf, np.nan)]
    for kw in both:
        assert e(**kw) == E_ARG, kw
        assert v(**kw) == E_ARG, kw
    assert lib.unet_vol_hessian_eig(None, a.data_ptr(), *shape, k.ctypes.data, None, eig.data_ptr(), s) == E_ARG
    assert lib.unet_vol_vesselness(None, a.data_ptr(), *shape, k.ctypes.data, None, *DENS, 1, 0, best.data_ptr(), scale.data_ptr(), s) == E_ARG
    for kw in (dict(out=None), dict(out=a.data_ptr()), dict(out=eig.data_ptr() + 1), dict(region=reg.data_ptr(), out=reg.data_ptr())):
        assert e(**kw) == E_ARG, kw
    for kw in ([dict(dens=tuple(bad if j == i else d for j, d in enumerate(DENS))) for i in range(3) for bad in (0.0, -2.0, np.inf, np.nan)] +
               [dict(bright=2), dict(bright=-1), dict(index=-1), dict(index=254), dict(b=None), dict(sc=None), dict(b=a.data_ptr()), dict(sc=a.data_ptr()),
                dict(sc=a.data_ptr() + 4 * N - 1), dict(b=best.data_ptr() + 2), dict(b=best.data_ptr(), sc=best.data_ptr()), dict(region=reg.data_ptr(), sc=reg.data_ptr())]):
        assert v(**kw) == E_ARG, kw
    torch.cuda.synchronize()
    assert (eig.cpu().numpy() == SENTINEL).all() and (best.cpu().numpy() == SENTINEL).all() and (scale.cpu().numpy() == SENTINEL).all()
    assert "vol_vesselness" in ops.ctx.last_error()


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------------------------------------
_PHANTOM = {}


def _phantom():
    """the oracle's phantom with its oracle results, computed once and left unchanged"""
    if not _PHANTOM:
        ph = VO.phantom()
        ct32 = LO.decode(ph["hu"]).astype(np.float32)
        _PHANTOM.update(ph=ph, ct32=ct32, vm=VO.vessel_mask(LO.decode(ph["hu"]), ph["lungs"], ph["pixdim"]), full=VO.vesselness(ct32, ph["pixdim"]),
                        eig=VO.hessian_eigenvalues(ct32, ph["pixdim"], 2.0))
    return _PHANTOM


def test_hessian_eigenvalues_end_to_end():
    from covidseg_amd import nifti_min
    from covidseg_amd import vessels as VS
    P = _phantom()
    ph = P["ph"]
    got = VS.hessian_eigenvalues(ph["hu"], 2.0, pixdim=ph["pixdim"])
    assert got.dtype == np.float32 and got.shape == (3,) + ph["hu"].shape
    _same_bits(got, P["eig"], "hessian_eigenvalues")
    assert (np.abs(got[0]) <= np.abs(got[1])).all() and (np.abs(got[1]) <= np.abs(got[2])).all()
    # a NiftiVolume carries its voxel size; a flat float32 device tensor takes src_shape= and pixdim=; a region
    vol = nifti_min.NiftiVolume(ph["hu"], 0.0, 0.0, ph["pixdim"], nifti_min.header_with_affine(ph["hu"].shape, nifti_min.affine_from_axcodes("LPI", ph["pixdim"])), "<")
    _same_bits(VS.hessian_eigenvalues(vol, 2.0), P["eig"], "hessian_eigenvalues of a NiftiVolume")
    dev = torch.from_numpy(_flat(P["ct32"])).cuda()
    region = ph["lungs"]
    out = VS.hessian_eigenvalues(dev, 2.0, pixdim=ph["pixdim"], src_shape=ph["hu"].shape, region=region, return_device=True)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.numel() == 3 * ph["hu"].size
    want = VO.hessian_eigenvalues(P["ct32"], ph["pixdim"], 2.0, region)
    _same_bits(np.stack([v.reshape(ph["hu"].shape, order="F") for v in out.cpu().numpy().reshape(3, -1)]), want, "hessian_eigenvalues of a device tensor under a region")


def test_vesselness_end_to_end():
    from covidseg_amd import vessels as VS
    P = _phantom()
    ph = P["ph"]
    got = VS.vesselness(ph["hu"], pixdim=ph["pixdim"])
    assert isinstance(got, VS.Vesselness) and got.sigmas_mm == (1.0, 2.0, 3.0) and got.shape == ph["hu"].shape and got.pixdim == ph["pixdim"]
    assert got.response.dtype == np.float32 and got.scale.dtype == np.uint8
    _same_bits(got.response, P["full"][0], "vesselness")
    assert np.array_equal(got.scale, P["full"][1]) and set(np.unique(got.scale)) == {0, 1, 2, 3}
    # other parameters, darker tubes, a region, the device results
    region = ph["lungs"]
    kw = dict(sigmas_mm=(1.5, 2.5), alpha=0.4, beta=0.6, c=250.0, bright=False)
    dev = VS.vesselness(ph["hu"], pixdim=ph["pixdim"], region=torch.from_numpy(_flat(region)).cuda(), return_device=True, **kw)
    wb, ws = VO.vesselness(P["ct32"], ph["pixdim"], region=region, **kw)
    assert isinstance(dev.response, torch.Tensor) and dev.scale.dtype == torch.uint8
    _same_bits(dev.response.cpu().numpy().reshape(ph["hu"].shape, order="F"), wb, "vesselness, dark")
    assert np.array_equal(dev.scale.cpu().numpy().reshape(ph["hu"].shape, order="F"), ws) and (wb > 0).any()


def test_vessel_mask_end_to_end():
    from covidseg_amd import vessels as VS
    P = _phantom()
    ph, want = P["ph"], P["vm"]
    got = VS.vessel_mask(ph["hu"], ph["lungs"], pixdim=ph["pixdim"])
    assert isinstance(got, VS.VesselMask) and got.mask.dtype == np.uint8
    assert np.array_equal(got.mask, want["mask"])
    _same_bits(got.vesselness.response, want["response"], "vessel_mask's response")
    assert np.array_equal(got.vesselness.scale, want["scale"])
    assert got.ml == int(want["mask"].sum()) * float(np.prod(np.asarray(ph["pixdim"], np.float64))) / 1000.0 and got.n_components >= 1
    share = float((got.mask[ph["tube"]] != 0).mean())
    assert share >= 0.9 and not (got.mask[ph["ball"]] != 0).mean() > 0.1
    # other parameters; the lungs as a device mask; the mask on the device
    kw = dict(threshold=0.5, dense_hu=-600.0, max_radius_mm=2.5, min_ml=0.05, connectivity=1, erode_mm=3.0, sigmas_mm=(1.0, 2.0))
    dev = VS.vessel_mask(ph["hu"], torch.from_numpy(_flat(ph["lungs"])).cuda(), pixdim=ph["pixdim"], return_device=True, **kw)
    w2 = VO.vessel_mask(LO.decode(ph["hu"]), ph["lungs"], ph["pixdim"], **kw)
    assert isinstance(dev.mask, torch.Tensor) and np.array_equal(dev.mask.cpu().numpy().reshape(ph["hu"].shape, order="F"), w2["mask"])


# ---- segment_volume(vessels=) -----------------------------------------------------------------------------------------------------------------------------------------
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


def test_segment_volume_reports_the_infection_against_the_vessels():
    """the stub model of the lung-mask test (a small randomly initialised U-Net, thresholded at its median) on the chest phantom sampled at 3 x 3 x 6 mm"""
    from covidseg_amd import nifti_min
    from covidseg_amd import vessels as VS
    from covidseg_amd import volume as V
    from covidseg_amd.keras_like import UNetModel
    pixdim = (3.0, 3.0, 6.0)
    ph = LO.phantom(False, "z-", shape=(56, 48, 28), pixdim=pixdim)
    hu = np.asfortranarray(ph["hu"])
    vol = nifti_min.NiftiVolume(hu, 0.0, 0.0, pixdim, nifti_min.header_with_affine(hu.shape, nifti_min.affine_from_axcodes("LPI", pixdim)), "<")
    model = UNetModel(64, 1, seed=1)
    model.verbose = 0
    t = float(np.median(model.predict(V.load_volume(vol, "cts", img_size=64, new_dim=64), batch_size=8)))
    kw = dict(lung_mask=ph["lungs"], threshold=t, batch_size=8, img_size=64, density=True)
    vkw = dict(sigmas_mm=(2.0, 3.0), erode_mm=3.0, max_radius_mm=6.0, min_ml=0.05)
    plain = V.segment_volume(vol, model, **kw)
    res = V.segment_volume(vol, model, vessels=vkw, **kw)
    want = VO.vessel_mask(LO.decode(hu), ph["lungs"], pixdim, **vkw)
    assert isinstance(res.vessels, VS.VesselMask) and isinstance(res.vessels.mask, np.ndarray) and np.array_equal(res.vessels.mask, want["mask"])
    _same_bits(res.vessels.vesselness.response, want["response"], "segment_volume's vesselness")
    on = int(np.count_nonzero((res.mask != 0) & (want["mask"] != 0)))
    print(f"segment_volume(vessels=): {int(want['mask'].sum())} vessel voxels, {int((res.mask != 0).sum())} infected, {on} both")
    assert int(want["mask"].sum()) > 0 and res.infected_ml_on_vessels == float(on) * float(np.prod(np.asarray(pixdim, np.float64))) / 1000.0
    assert res.seconds["vessels"] > 0
    free = V.intensity_stats(vol, mask=res.mask, region=(ph["lungs"] != 0) & (want["mask"] == 0))
    _same(vars(res.vessel_free_density), vars(free))
    # the infection mask and every earlier field are as without vessels=; vessels=None adds no field
    added = ("vessels", "infected_ml_on_vessels", "vessel_free_density")
    _same({k: v for k, v in vars(res).items() if k not in added}, vars(plain))
    assert not any(hasattr(plain, k) for k in added)
    _same(vars(V.segment_volume(vol, model, vessels=None, **kw)), vars(plain))
    # vessels=True: the defaults; without density= no vessel_free_density
    d = V.segment_volume(vol, model, lung_mask=ph["lungs"], threshold=t, batch_size=8, img_size=64, vessels=True)
    assert np.array_equal(d.vessels.mask, VO.vessel_mask(LO.decode(hu), ph["lungs"], pixdim)["mask"]) and not hasattr(d, "vessel_free_density")

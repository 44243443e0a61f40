"""-m gpu: the later trips of the volume kernels' bounded-grid loops.  Every kernel of csrc/kernels_resample / register / deform / intensity / lungside / render /
texture .hip launches at most a fixed number of workgroups and lets each stride over the rest; the per-family tests run shapes of at most one launch's worth of items, so
there every workgroup goes through its loop once.  The cases of tests/later_trips.py make every workgroup go through it at least twice and some a third, ragged time
(tests/test_later_trips_host.py asserts that, and that the later trips' items carry information, without a GPU).  The calls, the uploads, the guard bands and the
comparison are the per-family tests' own: every output lies between sentinel bands that must survive and equals its oracle bit for bit (a NaN matches a NaN)."""
import numpy as np
import pytest

import deform_oracle as DO
import intensity_oracle as IO
import later_trips as LT
import lungside_oracle as LO
import register_oracle as RO
import render_oracle as RD
import resample_oracle as RS
import test_gpu_deform as TDF
import test_gpu_register as TRG
import test_gpu_render as TRD
import test_gpu_resample as TRS
import test_gpu_texture as TTX
import texture_oracle as TO
from front_edges import Guarded
from gpu_util import Ops, cu_count

pytestmark = pytest.mark.gpu


def _check(got, want, what, per_trip=LT.TRIP):
    """equality of the stored bits in device order (deform_oracle.same_bits' rule); the message says how many elements differ and in which trip the first one lies"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} for {want.dtype} {want.shape}"
    g, w = LT.flat(got), LT.flat(want)
    if g.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
        bad = ~((g.view(u) == w.view(u)) | (np.isnan(g) & np.isnan(w)))
    else:
        bad = g != w
    if bad.any():
        first = int(np.argmax(bad))
        where = f": trip {first // per_trip + 1} of its launch" if per_trip else ""          # (None: the items of a trip are not consecutive outputs)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ from the oracle's, the first at index {first}{where}")
    assert DO.same_bits(got, want)


def _dev(a, dtype=None):
    import torch
    a = np.asarray(a) if dtype is None else np.asarray(a).astype(dtype)
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, order="F"))).cuda()


def _field_flat(a):
    """[C, X, Y, Z] -> device order"""
    return np.concatenate([LT.flat(c) for c in a])


# ---- 1. rs_direct_kernel ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mname,mode,dst", LT.RS_DIRECT_LINEAR)
def test_resample_linear_direct_mapping(kind, mname, mode, dst):
    o = Ops()
    raw, code, sc = LT.volume(LT.RS_SRC, kind, 7)
    keep, ptr = TRS._up(raw)
    M = LT.RS_MATRICES[mname]()
    rc, _, got = TRS._linear(o, ptr, TRS._vargs(raw, code, sc), M, mode, LT.RS_CVAL, LT.RS_OUT, dst)
    assert rc == 0, o.ctx.last_error()
    _check(got, RS.linear(RS.decode(raw, sc), M, LT.RS_OUT, mode, LT.RS_CVAL, dst), f"linear {kind} {mname} mode {mode} dst {dst} -> {LT.RS_OUT}")
    del keep


@pytest.mark.parametrize("mname,mode", LT.RS_DIRECT_NEAREST)
def test_resample_nearest_direct_mapping(mname, mode):
    o = Ops()
    raw = LT.volume(LT.RS_SRC, "i2", 7)[0]
    keep, ptr = TRS._up(raw)
    M = LT.RS_MATRICES[mname]()
    cval = np.int16(-31999)
    rc, _, got = TRS._nearest(o, ptr, 2, LT.RS_SRC, M, mode, int(cval.view(np.uint16)), LT.RS_OUT, np.int16)
    assert rc == 0, o.ctx.last_error()
    _check(got, RS.nearest(raw, M, LT.RS_OUT, mode, cval), f"nearest {mname} mode {mode} -> {LT.RS_OUT}")
    del keep


# ---- 2. rs_tiled_kernel -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,out", LT.RS_TILED_SMALL)
def test_resample_tiles_off_both_origins(name, out):
    """tiles with x0 > 0 and a0 > 0 at once, ragged on both axes: every element size and every dst type"""
    o = Ops()
    src, M = LT.perm_case(name, out)
    for eb in (1, 2, 4, 8):
        udt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[eb]
        raw = np.asfortranarray(np.random.default_rng(eb).integers(0, 2 ** (8 * eb), src, dtype=np.uint64).astype(udt))
        cval = np.array(TRS.CVAL_BITS & (2 ** (8 * eb) - 1), np.uint64).astype(udt)
        keep, ptr = TRS._up(raw, 1 if eb == 1 else 0)
        for mode in (0, 1):
            rc, _, got = TRS._nearest(o, ptr, eb, src, M, mode, TRS.CVAL_BITS, out, udt)
            assert rc == 0, o.ctx.last_error()
            _check(got, RS.nearest(raw, M, out, mode, cval), f"nearest {name} {eb} bytes mode {mode} -> {out}")
        del keep
    for kind in ("i2", "f4nan"):
        raw, code, sc = LT.volume(src, kind, 70)
        keep, ptr = TRS._up(raw)
        for mode in (0, 1):
            for dst in (64, 16, 2):
                rc, _, got = TRS._linear(o, ptr, TRS._vargs(raw, code, sc), M, mode, LT.RS_CVAL, out, dst)
                assert rc == 0, o.ctx.last_error()
                _check(got, RS.linear(RS.decode(raw, sc), M, out, mode, LT.RS_CVAL, dst), f"linear {name} {kind} mode {mode} dst {dst} -> {out}")
        del keep


@pytest.mark.parametrize("name,out,a,order,size,mode", LT.RS_TILED_LONG)
def test_resample_tiles_of_a_later_trip(name, out, a, order, size, mode):
    o = Ops()
    src, M = LT.perm_case(name, out)
    raw, code, sc = LT.volume(src, "i2", 16500)
    keep, ptr = TRS._up(raw)
    if order == "nearest":
        rc, _, got = TRS._nearest(o, ptr, size, src, M, mode, 0x7B7B, out, np.int16)
        want = RS.nearest(raw, M, out, mode, np.int16(0x7B7B))
    else:
        rc, _, got = TRS._linear(o, ptr, TRS._vargs(raw, code, sc), M, mode, LT.RS_CVAL, out, size)
        want = RS.linear(RS.decode(raw, sc), M, out, mode, LT.RS_CVAL, size)
    assert rc == 0, o.ctx.last_error()
    _check(got, want, f"{order} {name} -> {out}: 16,500 tiles", per_trip=None)
    del keep


# ---- 3. jh_kernel ---------------------------------------------------------------------------------------------------------------------------------------------------------
_JH = {}


def _jh_inputs():
    """the volumes on the device and decoded on the host, once"""
    if not _JH:
        (fraw, fcode, fsc), (mraw, mcode, msc), mask = LT.jh_volumes()
        _JH.update(f=TRG._up(fraw), m=TRG._up(mraw), k=TRG._up(mask, 1), fv=TRG._vargs(fraw, fcode, fsc), mv=TRG._vargs(mraw, mcode, msc),
                   ffd=RS.decode(fraw, fsc), mfd=RS.decode(mraw, msc), mask=mask, Ms=LT.jh_matrices())
    return _JH


@pytest.mark.parametrize("K,bins,masked", LT.JH_RUNS)
def test_joint_hist_counts_in_every_trip(K, bins, masked):
    o = Ops()
    c = _jh_inputs()
    Ms = c["Ms"][:K] if K > 1 else c["Ms"][9:10]
    got = TRG._hist(o, c["f"][1], c["fv"], c["k"][1] if masked else None, c["m"][1], c["mv"], Ms, bins, *LT.JH_WINDOWS)
    want = RO.joint_hist(c["ffd"], c["mfd"], Ms, bins, *LT.JH_WINDOWS, c["mask"] if masked else None)
    for q in range(K):
        assert np.array_equal(got[q], want[q]), f"candidate {q} of {K}, {bins} bins, mask {masked}: {np.count_nonzero(got[q] != want[q])} cells differ, {got[q].sum()} counted for {want[q].sum()}"


def test_joint_hist_one_cell_for_every_wave_of_every_trip():
    """the identity on a constant pair: the leader's ballot covers every counted lane"""
    o = Ops()
    fc, mc = LT.jh_constant_pair()
    kf, fptr = TRG._up(fc)
    km, mptr = TRG._up(mc)
    v = (4,) + LT.JH_FIXED + (0, 1.0, 0.0)
    eye = np.eye(4)[:3][None]
    got = TRG._hist(o, fptr, v, None, mptr, v, eye, 2, *LT.JH_WINDOWS)
    want = RO.joint_hist(fc.astype(np.float64), mc.astype(np.float64), eye, 2, *LT.JH_WINDOWS)
    assert np.array_equal(got, want) and got.sum() == int(np.prod(LT.JH_FIXED)), f"{got.reshape(-1).tolist()} for {want.reshape(-1).tolist()}"
    del kf, km


# ---- 4. sm_x_kernel, sm_yz_kernel -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", LT.SM_RADII)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_smooth_axis_later_tiles_and_elements(axis, R):
    o = Ops()
    x = LT.sm_field()
    keep, ptr = TDF._up_field(x)
    w = LT.sm_weights(R)
    rc, buf = TDF._smooth(o, ptr, LT.SM_C, LT.SM_SHAPE, axis, w)
    assert rc == 0, o.ctx.last_error()
    per_trip = LT.TRIP if axis else None
    _check(_field_flat(TDF._take(buf, np.float32, LT.SM_SHAPE, LT.SM_C)), _field_flat(DO.smooth_axis(x, axis, w)), f"smooth axis {axis} R {R}", per_trip)
    del keep


# ---- 5. dm_kernel, wf_kernel, jc_kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_demons_step_later_trips(masked):
    o = Ops()
    fraw, fcode, fsc = LT.volume(LT.DF_GRID, "i2", 257)
    mraw, mcode, msc = LT.volume(LT.DF_MOVING, "f4nan", 158)
    mask = LT.mask_of(LT.DF_GRID, 9)
    field = LT.random_field(LT.DF_GRID, 3, 1.5)
    kf, fptr = TDF._up(fraw)
    km, mptr = TDF._up(mraw)
    kk, kptr = TDF._up(mask, 1)
    ku, uptr = TDF._up_field(field)
    _, Ainv = LT.oblique3(0)
    W, L, G = RS.oblique_matrix(), Ainv * 0.8, Ainv.T
    n = int(np.prod(LT.DF_GRID))
    rc, buf = TDF._step(o, fptr, TDF._vargs(fraw, fcode, fsc), kptr if masked else None, mptr, TDF._vargs(mraw, mcode, msc), W, L, G, LT.DF_DELTA, uptr, n)
    assert rc == 0, o.ctx.last_error()
    want = DO.demons_step(RS.decode(fraw, fsc), RS.decode(mraw, msc), W, L, G, LT.DF_DELTA, field, mask if masked else None)
    got = TDF._take(buf, np.float32, LT.DF_GRID, 3)
    for c in range(3):
        _check(got[c], want[c], f"demons step, mask {masked}, component {c}")
    del kf, km, kk, ku


@pytest.mark.parametrize("name,grid,order,dst,mode", LT.DF_WARPS, ids=[w[0] for w in LT.DF_WARPS])
def test_warp_field_later_trips(name, grid, order, dst, mode):
    o = Ops()
    seed = [w[0] for w in LT.DF_WARPS].index(name)
    raw, code, sc = LT.volume(LT.DF_MOVING, "i2", 158)
    fshape, F = (LT.DF_GRID, None) if grid == "on_grid" else (LT.DF_COARSE, LT.DF_F)
    field = LT.random_field(fshape, 20 + seed, 2.0)
    ks, sptr = TDF._up(raw)
    ku, uptr = TDF._up_field(field)
    _, Ainv = LT.oblique3(1)
    W, L = RS.oblique_matrix(), Ainv * 0.7
    sv = TDF._vargs(raw, code, sc)
    if order == 1:
        rc, buf = TDF._warp(o, sptr, sv, W, L, uptr, fshape, F, 1, mode, -777.25, 0, dst, LT.DF_GRID, np.dtype(TDF._DST[dst]).itemsize)
        assert rc == 0, o.ctx.last_error()
        got, want = TDF._take(buf, TDF._DST[dst], LT.DF_GRID), DO.warp(raw, sc, W, L, field, F, LT.DF_GRID, 1, mode, -777.25, dst)
    else:
        cval = np.int16(-31999)
        rc, buf = TDF._warp(o, sptr, sv, W, L, uptr, fshape, F, 0, mode, 0.0, int(cval.view(np.uint16)), code, LT.DF_GRID, 2)
        assert rc == 0, o.ctx.last_error()
        got, want = TDF._take(buf, np.int16, LT.DF_GRID), DO.warp(raw, None, W, L, field, F, LT.DF_GRID, 0, mode, cval)
    _check(got, want, f"warp, {name}")
    del ks, ku


@pytest.mark.parametrize("which", ["random", "folded everywhere"])
def test_jacobian_later_trips_and_the_fold_count_across_them(which):
    o = Ops()
    field, Ai = (LT.random_field(LT.DF_GRID, 4, 2.0), LT.oblique3(0)[1]) if which == "random" else (LT.folded_field(LT.DF_GRID), LT.FOLDED_AINV)
    keep, uptr = TDF._up_field(field)
    rc, det, folded = TDF._jacobian(o, uptr, LT.DF_GRID, Ai)
    assert rc == 0, o.ctx.last_error()
    want, want_folded = DO.jacobian(field, Ai)
    _check(TDF._take(det, np.float32, LT.DF_GRID), want, f"jacobian, {which}")
    got_folded = int(TDF._take(folded, np.uint32, (1, 1, 1))[0, 0, 0])
    assert got_folded == want_folded, f"jacobian, {which}: {got_folded} folded voxels for {want_folded}"
    del keep


# ---- 6. ig_gather_kernel, ib_bands_kernel, mom_chunk_kernel -------------------------------------------------------------------------------------------------------------
def test_intensity_gather_later_trips():
    o = Ops()
    raw, labels, region = LT.ig_case()
    g = IO.group_of(LT.IG_SHAPE, labels=labels, n=LT.IG_N, region=region)
    wv, wg, off = IO.ordered(raw.astype(np.float64), g, LT.IG_N)
    count = len(wv)
    vd, ld, rd = _dev(raw), _dev(labels), _dev(region)
    for cap in (count, count // 2):                                  # the exact capacity; a short buffer: the count is still the true one, nothing is written past the capacity
        vals, grps, cnt = Guarded(cap, "f8"), Guarded(cap, "i4"), Guarded(1, "i8")
        rc = o.lib.unet_vol_intensity_gather(o.h, vd.data_ptr(), 16, *LT.IG_SHAPE, 0, 1.0, 0.0, ld.data_ptr(), None, LT.IG_N, rd.data_ptr(), vals.ptr, grps.ptr, cap, cnt.ptr, o.s)
        assert rc == 0, o.ctx.last_error()
        assert int(cnt.get("count")[0]) == count, f"capacity {cap}: {int(cnt.get()[0])} gathered for {count}"
        v, k = vals.get("values"), grps.get("groups")
        if cap == count:
            order = np.lexsort((v, k))                               # slot order is not defined: sorted per group
            assert np.array_equal(k[order], wg) and np.array_equal(v[order], wv), f"capacity {cap}: the gathered (group, value) pairs are not the oracle's"
        else:
            assert ((k >= 1) & (k <= LT.IG_N)).all()
            have = np.stack([np.bincount(k, minlength=LT.IG_N + 1)[1:], np.diff(off)])
            assert (have[0] <= have[1]).all()
            for grp in range(1, LT.IG_N + 1):                      # every written pair is one of the oracle's, as often at most
                mine, theirs = np.sort(v[k == grp]), wv[off[grp - 1]:off[grp]]
                at = np.searchsorted(theirs, mine)
                assert (at < theirs.size).all() and np.array_equal(theirs[np.minimum(at, theirs.size - 1)], mine), f"capacity {cap}: group {grp} holds a value the oracle does not"
                um, cm = np.unique(mine, return_counts=True)
                assert (cm <= np.searchsorted(theirs, um, side="right") - np.searchsorted(theirs, um, side="left")).all()


@pytest.mark.parametrize("shape,n", LT.IB_CASES)
def test_intensity_bands_across_slice_changes(shape, n):
    """per = 3 chunks a workgroup: its slice counters leave LDS and are reset in the middle of its loop; the LDS-table arm (n = 4) and the global-atomic arm"""
    o = Ops()
    raw, labels, region = LT.ib_case(shape, n)
    g = IO.group_of(shape, labels=labels, n=n, region=region)
    want = IO.bands(IO.decode(raw, True, LT.IV_SLOPE, LT.IV_INTER), g, n, LT.IB_EDGES)
    vd, ld, rd = _dev(raw), _dev(labels), _dev(region)
    W, Z = LT.IB_EDGES.size + 2, shape[2]
    bc, sc, mm = Guarded(n * W, "i8"), Guarded(Z * W, "i8"), Guarded(2 * n, "f8")
    e = np.ascontiguousarray(LT.IB_EDGES)
    rc = o.lib.unet_vol_intensity_bands(o.h, vd.data_ptr(), 4, *shape, 1, LT.IV_SLOPE, LT.IV_INTER, ld.data_ptr(), None, n, rd.data_ptr(), e.ctypes.data, e.size, bc.ptr, sc.ptr, mm.ptr, o.s)
    assert rc == 0, o.ctx.last_error()
    got = (bc.get("band_counts").reshape(n, W), sc.get("slice_counts").reshape(Z, W), mm.get("minmax").reshape(n, 2))
    for name, a, b in zip(("band_counts", "slice_counts", "minmax"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{shape} n {n}: {np.count_nonzero(a != b)} of {b.size} {name} differ; sums {a.sum()} for {b.sum()}"


def test_group_moments_more_slots_than_two_launches():
    o = Ops()
    values, off = LT.mom_case()
    n = len(off) - 1
    want = LT.mom_closed_form(values, off)
    vd, od = _dev(values), _dev(off)
    ws_bytes = int(o.lib.unet_vol_group_moments_ws_bytes(int(off[-1]), n))
    assert ws_bytes // 8 - n >= LT.mom_slots(off)
    out, ws = Guarded(2 * n, "f8"), Guarded(ws_bytes // 8, "f8")
    rc = o.lib.unet_vol_group_moments(o.h, vd.data_ptr(), od.data_ptr(), n, out.ptr, ws.ptr, ws_bytes, o.s)
    assert rc == 0, o.ctx.last_error()
    ws.get("workspace")
    _check(out.get("moments").reshape(n, 2), want, "group moments of 4,180,000 runs of one or two values", per_trip=None)


# ---- 7. side_assign_kernel<1>, <4> ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm,N", [("one voxel a lane", LT.SA_SCALAR_N), ("four voxels a lane", LT.SA_VECTOR_N)])
def test_side_assign_later_trips(arm, N):
    o = Ops()
    mask, a, b = LT.sa_inputs(N, 1)
    skew = 1 if arm == "one voxel a lane" else 0                    # the mask off its alignment by one byte: the scalar kernel
    km, mptr = TRS._up(mask.reshape(N, 1, 1), skew)
    assert mptr % 4 == skew
    at, bt = _dev(a), _dev(b)
    for side_a, side_b in ((1, 2), (2, 1)):
        sides, counts = Guarded(N, "u1"), Guarded(3, "i8")
        rc = o.lib.unet_vol_side_assign(o.h, mptr, at.data_ptr(), bt.data_ptr(), N, 1, 1, side_a, side_b, sides.ptr, counts.ptr, o.s)
        assert rc == 0, o.ctx.last_error()
        want, wc = LO.side_assign(mask, a, b, side_a, side_b)
        _check(sides.get("sides"), want, f"side_assign, {arm}, sides {side_a} {side_b}", per_trip=LT.TRIP * (1 if skew else 4))
        gc = counts.get("counts")
        assert np.array_equal(gc, wc), f"side_assign, {arm}: counts {gc.tolist()} for {wc.tolist()}"
    del km


# ---- 8. pj_walk_kernel, pj_wave_kernel ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LT.PJ_CASES, ids=[c[0] for c in LT.PJ_CASES])
def test_project_later_trips(case):
    name, shape, axis, a, b, kind = case
    o = Ops()
    raw, code, sc = LT.volume(shape, kind, sum(shape))
    fd = RD.fdata(raw, sc)
    mask, lab = LT.pj_labels(shape, sum(shape))
    keep, ptr = TRD._up(raw)
    km, mp = TRD._up(mask, 1)
    kl, lp = TRD._up(lab)
    per_trip = LT.PJ_WAVE_TRIP if axis == 0 else LT.TRIP
    for mode in (0, 1):
        rc, plane, (pm, pl) = TRD._project(o, ptr, TRD._vargs(raw, code, sc), axis, a, b, mode, [(mp, np.uint8), (lp, np.int32)])
        assert rc == 0, o.ctx.last_error()
        _check(plane, RD.project(fd, axis, a, b, mode), f"{name}, mode {mode}: the plane", per_trip)
        _check(pm, RD.project_labels(mask, axis, a, b), f"{name}, mode {mode}: the uint8 layer", per_trip)
        _check(pl, RD.project_labels(lab, axis, a, b), f"{name}, mode {mode}: the int32 layer", per_trip)
    del keep, km, kl


# ---- 9. tq_quantize_kernel, tr_runs_kernel, tg_glcm_kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Ng,outside", LT.TQ_CASES)
def test_texture_quantize_later_trips(n, Ng, outside):
    raw, labels = LT.tq_case(n)
    g = TO.group_of(LT.TX_SHAPE, labels=labels, n=n)
    want_lv, want_lc = TO.quantize(TO.decode(raw, True, LT.IV_SLOPE, LT.IV_INTER), g, n, LT.TQ_LO, LT.tq_width(Ng), Ng, outside)
    assert (TTX.SLOPE, TTX.INTER) == (LT.IV_SLOPE, LT.IV_INTER)
    got_lv, got_lc, _ = TTX.dev_quantize(TTX._vol(raw, True), _dev(labels), None, n, None, LT.TQ_LO, LT.tq_width(Ng), Ng, outside, f"quantize n {n} Ng {Ng} outside {outside}")
    _check(got_lv, want_lv, f"quantize n {n} Ng {Ng} outside {outside}: levels")
    assert np.array_equal(got_lc, want_lc), f"quantize n {n} Ng {Ng} outside {outside}: {np.count_nonzero(got_lc != want_lc)} level counts differ, {got_lc.sum()} counted for {want_lc.sum()}"


def test_texture_runs_later_trips_and_a_line_across_them():
    lev, labels = LT.tr_case()
    g = TO.group_of(LT.TX_SHAPE, labels=labels, n=LT.TR_N)
    want, wcl = TO.runs(lev, g, LT.TR_N, LT.TR_NG, LT.TR_BITS, LT.TR_MAX_RUN)
    assert wcl[0, 1] >= 1                                            # TR_LINE: group 1, along z, longer than max_run
    got, cl = TTX.dev_runs(_dev(lev), _dev(labels), LT.TR_N, LT.TX_SHAPE, LT.TR_NG, LT.TR_BITS, LT.TR_MAX_RUN, "runs")
    assert np.array_equal(got, want), f"runs: {np.count_nonzero(got != want)} of {want.size} counts differ, {got.sum()} runs for {want.sum()}"
    assert np.array_equal(cl, wcl), f"runs: clamped {cl.tolist()} for {wcl.tolist()}"


@pytest.mark.parametrize("distance", [1, 4])
@pytest.mark.parametrize("n", [LT.GLCM_N, 99], ids=["LDS table", "global atomics"])
def test_texture_glcm_empty_bricks_before_and_between_staged_ones(n, distance):
    """every persistent workgroup meets an empty brick first, every other one another between two staged ones (the walks: tests/test_later_trips_host.py)"""
    cus = cu_count()
    lev, labels = LT.glcm_case(cus, n)
    walks = LT.glcm_walks(lev, LT.GLCM_NG, cus)
    G = LT.glcm_grid(cus)
    assert len(walks) == G and all(w[0] == "e" for w in walks) and sum(w.startswith("eses") for w in walks) >= G // 3          # (the host test's figure, on this device's CU count)
    g = TO.group_of(lev.shape, labels=labels, n=n)
    want = TO.glcm(lev, g, n, LT.GLCM_NG, distance, TTX.ALL, False)
    got = TTX.dev_glcm(_dev(lev), _dev(labels), n, lev.shape, LT.GLCM_NG, distance, TTX.ALL, False, f"glcm n {n} distance {distance}")
    assert got.shape == want.shape and np.array_equal(got, want), f"glcm n {n} distance {distance} on {cus} CUs: {np.count_nonzero(got != want)} of {want.size} counts differ, {got.sum()} pairs for {want.sum()}"

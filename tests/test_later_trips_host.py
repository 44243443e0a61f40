"""No GPU: the conditions the cases of tests/test_gpu_later_trips.py rest on, from the case lists of tests/later_trips.py and the oracles alone.  For every case: the
trips every workgroup makes, computed from the launch caps restated in later_trips.py (the shape rule), and the share of the items a later trip reaches that carry
information (the content rule).  Every restated cap is read out of its .hip file, so a cap that changes fails here instead of silently disarming a case."""
import os
import re

import numpy as np
import pytest

import deform_oracle as DO
import intensity_oracle as IO
import later_trips as LT
import lungside_oracle as LO
import register_oracle as RO
import render_oracle as RD
import resample_oracle as RS
import texture_oracle as TO

HALF = 0.5


# ---- the caps ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file,name,pattern,value", LT.CAP_SOURCES, ids=[f"{f}:{n}" for f, n, _, _ in LT.CAP_SOURCES])
def test_a_restated_cap_is_the_sources(file, name, pattern, value):
    from covidseg_amd import _lib
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", file)).read()
    found = re.findall(pattern, src)
    assert len(found) == 1, f"{file}: {name} is written {len(found)} times as /{pattern}/"
    assert LT.constant_value(found[0]) == value, f"{file}: {name} = {found[0]}, the cases were chosen for {value}"


def test_the_lds_counters_of_the_glcm_table_are_the_headers():
    from covidseg_amd import _lib
    assert _lib.TEXTURE_LDS_COUNTERS == LT.GLCM_LDS_COUNTERS
    assert LT.TRIP == 2097152 and LT.JH_TRIP == 262144 and LT.PJ_WAVE_TRIP == 32768


# ---- 1, 2. resample -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_resample_direct_cases():
    N = int(np.prod(LT.RS_OUT))
    assert LT.shape_rule(N, LT.TRIP) and LT.RS_OUT[0] % 64 != 0
    full, rest = LT.later_trips(N, LT.TRIP)
    assert (full, rest // LT.TPB, rest % LT.TPB) == (2, 62, 255)
    for name, make in LT.RS_MATRICES.items():
        M = make()
        assert LT.rs_lane_axis(M, LT.RS_OUT[1], LT.RS_OUT[2]) == 0, name          # the direct mapping
        share = LT.tail_share(LT.inside(M, LT.RS_OUT, LT.RS_SRC))
        print(f"{name}: {share:.3f} of the later trips' outputs sample inside the source")
        assert share >= HALF
    assert {(m, mode) for _, m, mode, _ in LT.RS_DIRECT_LINEAR} == {(m, mode) for m in LT.RS_MATRICES for mode in (0, 1)}
    assert {d for _, _, _, d in LT.RS_DIRECT_LINEAR} == {64, 2} and {k for k, _, _, _ in LT.RS_DIRECT_LINEAR} == {"i2", "f4nan"}


@pytest.mark.parametrize("case", [c for c in LT.RS_DIRECT_LINEAR if c[0] == "f4nan"], ids=lambda c: f"{c[1]}-mode{c[2]}")
def test_resample_direct_blends_of_the_nan_source_are_mostly_numbers(case):
    kind, mname, mode, dst = case
    raw, _, sc = LT.volume(LT.RS_SRC, kind, 7)
    ref = RS.linear(RS.decode(raw, sc), LT.RS_MATRICES[mname](), LT.RS_OUT, mode, LT.RS_CVAL, 64)
    share = LT.tail_share(~np.isnan(ref) & ((ref != LT.RS_CVAL) if mode else True))
    nans = LT.tail_share(np.isnan(ref))
    print(f"{mname} mode {mode}: {share:.3f} numbers from the source, {nans:.3f} NaN in the later trips")
    assert share >= HALF and nans > 0.01
    if dst == 2:
        ones = LT.tail_share(ref >= 0.5)
        assert 0.2 < ones < 0.8                                       # the uint8 cut separates


def test_resample_tiled_cases():
    for name, out in LT.RS_TILED_SMALL:
        src, M = LT.perm_case(name, out)
        a = LT.rs_lane_axis(M, out[1], out[2])
        assert a == (1 if name == "perm_x_from_y" else 2)
        tx, ta, tiles = LT.rs_tiles(out, a)
        assert tx == 2 and ta == 2 and tiles == 12 and out[0] % 64 == 6 and out[a] % 64 == 6          # the tile at x0 = 64, a0 = 64 is 6 x 6
        assert LT.inside(M, out, src).all() and int(np.prod(src)) == int(np.prod(out))
    for name, out, a, order, _, _ in LT.RS_TILED_LONG:
        src, M = LT.perm_case(name, out)
        assert LT.rs_lane_axis(M, out[1], out[2]) == a
        assert LT.rs_tiles(out, a) == (1, 1, 16500)
        full, rest = LT.later_trips(16500, LT.GRID_CAP)
        assert (full, rest) == (2, 116)                              # every workgroup walks two tiles, 116 a third; every tile is ragged: 3 x 17
        assert LT.inside(M, out, src).all()
    assert LT.rs_lane_axis(LT.perm_case("perm_x_from_y", (3, 15, 2))[1], 15, 2) == 0          # (below TILED_MIN the direct kernel runs)


# ---- 3. joint histogram -------------------------------------------------------------------------------------------------------------------------------------------------
def test_joint_hist_later_trips_count_for_every_candidate():
    N = int(np.prod(LT.JH_FIXED))
    assert LT.shape_rule(N, LT.JH_TRIP) and LT.JH_FIXED[0] % 64 != 0
    full, rest = LT.later_trips(N, LT.JH_TRIP)
    assert (full, rest // LT.TPB, rest % LT.TPB) == (2, 43, 101)
    (fraw, _, fsc), (mraw, _, msc), mask = LT.jh_volumes()
    ffd, mfd = RS.decode(fraw, fsc), RS.decode(mraw, msc)
    Ms = LT.jh_matrices()
    assert Ms.shape == (16, 3, 4) and len({M.tobytes() for M in Ms}) == 16
    m_later = LT.flat(mask)[LT.JH_TRIP:]
    assert 0.7 < (m_later != 0).mean() < 0.8 and (LT.flat(mask)[:LT.JH_TRIP] != 0).any()          # the mask's voxels lie in every trip
    for c, M in enumerate(Ms):                                       # what the second trip alone, and the third, add to this candidate's histogram
        ok = LT.flat(RO.counted(ffd, mfd, M)[0])
        okm = ok & (LT.flat(mask) != 0)                              # (the mask only removes voxels)
        second, third = ok[LT.JH_TRIP:2 * LT.JH_TRIP], ok[2 * LT.JH_TRIP:]
        assert second.sum() > LT.JH_TRIP // 2 and third.sum() > 0 and okm[LT.JH_TRIP:2 * LT.JH_TRIP].sum() > LT.JH_TRIP // 4 and okm[2 * LT.JH_TRIP:].sum() > 0, c
        assert ok[LT.JH_TRIP:].mean() >= HALF and okm[LT.JH_TRIP:].mean() >= HALF, (c, ok[LT.JH_TRIP:].mean(), okm[LT.JH_TRIP:].mean())          # without and under the mask
    fc, mc = LT.jh_constant_pair()
    h = RO.joint_hist(fc.astype(np.float64), mc.astype(np.float64), np.eye(4)[:3][None], 2, *LT.JH_WINDOWS)
    assert np.count_nonzero(h) == 1 and h.sum() == N                 # one cell: one ballot covers every counted lane of a wave, in every trip


# ---- 4. the Gaussian pass ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_smooth_cases():
    tiles, segs = LT.sm_tiles(LT.SM_C, LT.SM_SHAPE)
    full, rest = LT.later_trips(tiles, LT.GRID_CAP)
    rows = LT.SM_C * LT.SM_SHAPE[1] * LT.SM_SHAPE[2]
    assert tiles == 24726 and segs == 3 and full >= 2 and rest > 0 and LT.SM_SHAPE[0] % 64 == 2          # a last segment of two outputs
    assert rows % LT.SM_ROWS == 3 and tiles - 1 >= 2 * LT.GRID_CAP   # the last row group is short of a workgroup by a wave, in a later trip: `row < rows` fails there
    total = LT.SM_C * int(np.prod(LT.SM_SHAPE))
    assert LT.shape_rule(total, LT.TRIP)
    x = LT.sm_field()
    for (c, i, j, k), v in LT.SM_SPECIALS.items():
        at = LT.field_index(c, i, j, k, LT.SM_SHAPE)
        assert at >= LT.TRIP and (at // LT.SM_SHAPE[0]) // LT.SM_ROWS * segs >= LT.GRID_CAP          # later trips of sm_yz_kernel and of sm_x_kernel
        assert np.array_equal(x[c, i, j, k], np.float32(v), equal_nan=True)
    assert np.isfinite(x).sum() == x.size - 3
    for R in LT.SM_RADII:
        w = LT.sm_weights(R)
        assert w.size == 2 * R + 1 and np.isfinite(w).all()


# ---- 5. demons, warp, Jacobian ------------------------------------------------------------------------------------------------------------------------------------------
def test_demons_cases():
    N = int(np.prod(LT.DF_GRID))
    assert LT.shape_rule(N, LT.TRIP)
    fraw, _, fsc = LT.volume(LT.DF_GRID, "i2", 257)
    mraw, _, msc = LT.volume(LT.DF_MOVING, "f4nan", 158)
    _, Ainv = LT.oblique3(0)
    field = LT.random_field(LT.DF_GRID, 3, 1.5)
    mask = LT.mask_of(LT.DF_GRID, 9)
    ok = DO.demons_force(RS.decode(fraw, fsc), RS.decode(mraw, msc), RS.oblique_matrix(), Ainv * 0.8, Ainv.T, LT.DF_DELTA, field)[1]
    share, masked = LT.tail_share(ok), LT.tail_share(ok & (mask != 0))
    print(f"demons: a force at {share:.3f} of the later trips' voxels, {masked:.3f} under the mask")
    assert share >= HALF and masked >= HALF


def test_warp_cases():
    assert LT.shape_rule(int(np.prod(LT.DF_GRID)), LT.TRIP)
    _, Ainv = LT.oblique3(1)
    W, L = RS.oblique_matrix(), Ainv * 0.7
    for seed, (name, grid, order, dst, mode) in enumerate(LT.DF_WARPS):
        fshape = LT.DF_GRID if grid == "on_grid" else LT.DF_COARSE
        field = LT.random_field(fshape, 20 + seed, 2.0)
        s = DO.coords(W, L, DO.field_at(field, None if grid == "on_grid" else LT.DF_F, LT.DF_GRID), LT.DF_GRID)
        ok = np.ones(LT.DF_GRID, bool)
        for sr, n in zip(s, LT.DF_MOVING):
            ok &= (sr >= 0.0) & (sr <= float(n - 1))
        share = LT.tail_share(ok)
        print(f"warp, {name}: {share:.3f} of the later trips' outputs sample inside the source")
        assert share >= HALF
    q = RS.coords(LT.DF_F, LT.DF_GRID)
    assert (q[1] < 0).any() and (q[0] > LT.DF_COARSE[0] - 1).any()  # the coarse field is looked up beyond both of its edges (clamped)
    assert {o for _, _, o, _, _ in LT.DF_WARPS} == {0, 1}


def test_jacobian_cases():
    N = int(np.prod(LT.DF_GRID))
    _, Ainv = LT.oblique3(0)
    det, folded = DO.jacobian(LT.random_field(LT.DF_GRID, 4, 2.0), Ainv)
    later = LT.flat(det)[LT.TRIP:]
    assert 0 < (later <= 0).sum() < later.size and 0 < folded < N   # folds in the later trips, and voxels that do not fold
    det, folded = DO.jacobian(LT.folded_field(LT.DF_GRID), LT.FOLDED_AINV)
    assert folded == N == 4210431                                    # the count crosses every trip


# ---- 6. intensity ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_gather_case():
    N = int(np.prod(LT.IG_SHAPE))
    assert LT.shape_rule(N, LT.TRIP)
    raw, labels, region = LT.ig_case()
    g = IO.group_of(LT.IG_SHAPE, labels=labels, n=LT.IG_N, region=region)
    take = (g > 0) & ~np.isnan(raw)
    share = LT.tail_share(take)
    print(f"gather: {share:.3f} of the later trips' voxels are gathered")
    assert share >= HALF and np.isnan(raw[g > 0]).any() and set(np.unique(g)) == {0, 1, 2, 3}


@pytest.mark.parametrize("shape,n", LT.IB_CASES)
def test_bands_cases(shape, n):
    cps, chunks, per, grid = LT.ib_walk(shape)
    assert per == 3 and chunks > 2 * LT.IB_GRID and grid <= LT.IB_GRID
    assert cps == (1 if shape[0] * shape[1] <= LT.IB_CHUNK else 2)
    # workgroups whose chunk range holds a slice boundary in its middle: the flush and reset inside the loop
    crossing = sum(1 for b in range(grid) if (b * per) // cps != (min(chunks, (b + 1) * per) - 1) // cps)
    assert crossing >= grid // 2
    last = chunks - (grid - 1) * per
    assert 1 <= last <= per
    W = LT.IB_EDGES.size + 2
    assert (n * W <= LT.IB_TABLE and n <= LT.IB_GROUPS) == (n == 4)  # the two arms
    raw, labels, region = LT.ib_case(shape, n)
    g = IO.group_of(shape, labels=labels, n=n, region=region)
    assert (g > 0).mean() >= HALF
    bc, sc, mm = IO.bands(IO.decode(raw, True, LT.IV_SLOPE, LT.IV_INTER), g, n, LT.IB_EDGES)
    assert (sc.sum(axis=1) > 0).mean() > 0.99 and (bc.sum(axis=0)[:-1] > 0).all()          # the slices count (five voxels may all lie outside), every band occurs


def test_moments_case_and_its_closed_form():
    values, off = LT.mom_case()
    slots = LT.mom_slots(off)
    assert LT.shape_rule(slots, LT.TRIP, lanes_along_x=False), LT.later_trips(slots, LT.TRIP)
    m = np.diff(off)
    assert set(np.unique(m)) == {1, 2}
    k = 10000
    want = IO.moments(values[:off[k]], off[:k + 1])
    got = LT.mom_closed_form(values, off)
    assert np.array_equal(got[:k].view(np.uint64), want.view(np.uint64))
    assert (got[m == 1, 1] == 0.0).all() and (got[m == 2, 1] > 0.0).all()


# ---- 7. sides ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_side_assign_cases():
    assert LT.shape_rule(LT.SA_SCALAR_N, LT.TRIP)
    items = -(-LT.SA_VECTOR_N // 4)
    assert LT.later_trips(items, LT.TRIP) == (2, 1) and LT.SA_VECTOR_N % 4 == 3          # two whole trips, then one item of three voxels
    mask, a, b = LT.sa_inputs(LT.SA_SCALAR_N, 1)
    later = slice(LT.TRIP, None)
    assert (mask[later] != 0).mean() >= HALF
    ties = (mask != 0) & (a == b)
    assert ties[later].sum() > 1000 and np.isinf(a[later]).any() and (np.isinf(a) & np.isinf(b))[later].any()
    sides, counts = LO.side_assign(mask, a, b, 1, 2)
    other, _ = LO.side_assign(mask, a, b, 2, 1)
    assert (sides[ties] == 1).all() and (other[ties] == 1).all() and (sides != other)[mask != 0][~ties[mask != 0]].all()          # a tie goes to side 1 in either order
    assert counts.sum() == LT.SA_SCALAR_N and (counts > 0).all()
    mask, a, b = LT.sa_inputs(LT.SA_VECTOR_N, 1)                    # the vector arm: a later trip begins at voxel 4 TRIP
    later = slice(4 * LT.TRIP, None)
    ties = (mask != 0) & (a == b)
    assert (mask[later] != 0).mean() >= HALF and ties[later].sum() > 1000 and np.isinf(a[later]).any() and (np.isinf(a) & np.isinf(b))[later].any()
    assert mask[-3:].any() and not mask[LT.TRIP + 256:LT.TRIP + 512].any()          # the short last item takes part; whole waves off the mask


# ---- 8. projections ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LT.PJ_CASES, ids=[c[0] for c in LT.PJ_CASES])
def test_project_cases(case):
    name, shape, axis, a, b, kind = case
    if axis == 0:
        cols = shape[1] * shape[2]
        full, rest = LT.later_trips(cols, LT.PJ_WAVE_TRIP)
        assert full >= 2 and rest > 0 and rest % (LT.TPB // LT.WAVE) != 0          # a last workgroup with fewer columns than waves
        assert shape[0] % 64 != 0 and (b - a) % 64 != 0 and (b - a) > 64          # the slab: a wave and a ragged rest
        start = LT.PJ_WAVE_TRIP
    else:
        outs = shape[0] * shape[3 - axis]
        assert LT.shape_rule(outs, LT.TRIP) and shape[0] % 64 != 0
        start = LT.TRIP
    raw, _, sc = LT.volume(shape, kind, sum(shape))
    plane = RD.project(RD.fdata(raw, sc), axis, a, b, 0)
    assert LT.tail_share(~np.isnan(plane), start) >= HALF
    mask, lab = LT.pj_labels(shape, sum(shape))
    assert LT.tail_share(RD.project_labels(mask, axis, a, b) != 0, start) >= HALF and LT.tail_share(RD.project_labels(lab, axis, a, b) > 0, start) >= HALF


# ---- 9. texture ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Ng,outside", LT.TQ_CASES)
def test_quantize_cases(n, Ng, outside):
    assert LT.shape_rule(int(np.prod(LT.TX_SHAPE)), LT.TRIP)
    assert (n * Ng <= LT.TQ_TABLE) == (n == 3)
    raw, labels = LT.tq_case(n)
    g = TO.group_of(LT.TX_SHAPE, labels=labels, n=n)
    lev, lc = TO.quantize(TO.decode(raw, True, LT.IV_SLOPE, LT.IV_INTER), g, n, LT.TQ_LO, LT.tq_width(Ng), Ng, outside)
    share = LT.tail_share(lev > 0)
    print(f"quantize n {n} Ng {Ng} outside {outside}: {share:.3f} of the later trips' voxels get a level")
    assert share >= HALF and (lc.sum(axis=0) > 0).all()
    assert (LT.tail_share(lev > 0) < LT.tail_share(g > 0)) == bool(outside)          # dropping drops something


def test_runs_case():
    lev, labels = LT.tr_case()
    idx = TO.indices_of(LT.TR_BITS)
    assert idx == [0, 2, 12]
    starts = np.zeros(LT.TX_SHAPE, bool)
    for k in idx:
        starts |= LT.run_starts(lev, labels, LT.TR_N, LT.TR_NG, TO.DIRECTIONS[k])
    share = LT.tail_share(starts)
    print(f"runs: {share:.3f} of the later trips' voxels begin a run")
    assert share >= HALF
    x, y, z0, z1 = LT.TR_LINE
    X, Y, _ = LT.TX_SHAPE
    assert z1 - z0 > LT.TR_MAX_RUN and x + X * (y + Y * z0) < LT.TRIP <= x + X * (y + Y * (z1 - 1))
    along_z = LT.run_starts(lev, labels, LT.TR_N, LT.TR_NG, (0, 0, 1))
    assert along_z[x, y, z0] and not along_z[x, y, z0 + 1:z1].any() and along_z[x, y, z1] == (labels[x, y, z1] in (1, 2, 3))


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_glcm_walks_meet_empty_bricks_before_and_between_staged_ones(cus):
    shape = LT.glcm_shape(cus)
    G = LT.glcm_grid(cus)
    nb = int(np.prod([-(-s // b) for s, b in zip(shape, LT.BRICK)]))
    assert nb >= 4 * G and nb % G != 0 and shape[:2] == LT.GLCM_XY and shape[0] < LT.BRICK[0]          # thin bricks; every workgroup walks four, some five
    for n in (LT.GLCM_N, 99):
        lev, labels = LT.glcm_case(cus, n)
        walks = LT.glcm_walks(lev, LT.GLCM_NG, cus)
        assert len(walks) == G and all(w[0] == "e" for w in walks)  # the first brick of every workgroup is empty
        assert sum(w.startswith("eses") for w in walks) >= G // 3 and sum(w.startswith("esss") for w in walks) >= G // 3
        K = 13
        assert (n * K * LT.GLCM_NG ** 2 <= LT.GLCM_LDS_COUNTERS) == (n == LT.GLCM_N)
        assert labels.max() == n and (lev[labels == 0] == 0).all()

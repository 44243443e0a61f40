"""GPU: unet_vol_thin_*, unet_vol_skeleton_count / _emit, unet_vol_label_spread (csrc/kernels_skeleton.hip) and skeleton.* against tests/skeleton_oracle.py, every
comparison for equality, every output of a direct call between sentinel bands.

Which cases reach which path.  A row of X <= 64 is one word, X = 65 and 130 two and three: X = 63, 64, 65 put a row's end just short of, on and beyond a word, and a
tube crosses the x = 63 | 64 word edge diagonally, so candidates sit at bit 63 and bit 0 and read the edge bit of the adjacent word.  Voxels lie on every face of the
volume (a neighbour outside is background).  Extents of 1 and 2 (Y, Z from 1, 2, 9, 12; X = 1) are the degenerate volumes: a 2-D image, a single row, a single voxel.
Every grid of the file is sized to its work (its header says so): there is no bounded grid and no later trip to enter.  The table kernels give a workgroup 256 words:
(130, 12, 9) has 324 words, so two workgroups, the second ragged."""
import numpy as np
import pytest
import torch

import lungmask_oracle as LO
import skeleton_oracle as SO
import volscore_oracle as VS
from gpu_util import Ops

pytestmark = pytest.mark.gpu

BAND = 96                                                            # sentinel bytes / elements either side of an output (a multiple of 16: the alignment stays)
SENTINEL = 0xA5
COUNT_SENTINEL = 0x5A5A5A5A5A5A5A5A
XS = (1, 63, 64, 65, 130)
MAIN_YZ = ((12, 9), (9, 12))                                         # the cases whose content is asserted on the oracle
DEGENERATE_YZ = ((1, 1), (2, 1), (1, 12), (12, 1), (2, 2), (2, 9))   # compared for equality; too thin for two iterations


def _flat(a):
    return np.ascontiguousarray(np.asarray(a).reshape(-1, order="F"))


def _content(shape, seed):
    """smoothed-noise blobs at about a third, a tube across the x = 63 | 64 word edge where the row has one, voxels on every face"""
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    vol = SO.blobs(shape, seed, 0.33 if X > 1 else 0.55).astype(bool) if min(Y, Z) >= 9 else rng.random(shape) < 0.6
    if X >= 65:
        vol |= SO.tubes(shape, (((55.0, 1.5, 1.5), (73.0, Y - 2.5, Z - 2.5), 1.8),)).astype(bool)
    for ax in range(3):
        for side in (0, -1):
            face = [slice(None)] * 3
            face[ax] = side
            vol[tuple(face)] |= rng.random(vol[tuple(face)].shape) < 0.3
    return np.asfortranarray(vol.astype(np.uint8))


def _asserted_content(shape):
    """the first seed whose content, on the ORACLE, is cleared by at least two iterations and leaves voxels of degree 1, 2 and >= 3: a case cannot pass by being empty"""
    for seed in range(40):
        vol = _content(shape, seed)
        skel, _, removed = SO.thin(vol, True)
        deg = SO.degrees(skel)
        if int((removed > 0).sum()) >= 2 and (deg == 1).any() and (deg == 2).any() and (deg >= 3).any() and int((SO.thin(vol, False)[2] > 0).sum()) >= 2:
            return vol
    raise AssertionError(f"no seed gives {shape} the asserted content")


def _thin(ops, vol, endpoints=True, max_iterations=None, chunk=8, in_off=0, out_off=0):
    """the three entries as skeleton.thin_device drives them, every output between sentinels -> (mask, removed, bands, calls of _iterations); in_off / out_off: bytes the
    input and the output start into their buffers"""
    X, Y, Z = vol.shape
    N = vol.size
    src = torch.zeros(N + in_off + 16, dtype=torch.uint8, device="cuda")
    src[in_off:in_off + N] = torch.from_numpy(_flat(vol != 0).astype(np.uint8) * np.tile(np.array([1, 255, 3], np.uint8), N // 3 + 1)[:N]).cuda()          # any non-zero byte is set
    dst = torch.full((N + 2 * BAND + out_off,), SENTINEL, dtype=torch.uint8, device="cuda")
    wsb = int(ops.lib.unet_vol_thin_ws_bytes(X, Y, Z))
    ws = torch.full((wsb + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    wp = ws.data_ptr() + BAND
    ops.ck(ops.lib.unet_vol_thin_begin(ops.h, src.data_ptr() + in_off, X, Y, Z, wp, wsb, ops.s), "begin")
    removed, first, calls, bands = [], 0, 0, True
    while max_iterations is None or first < max_iterations:
        n = chunk if max_iterations is None else min(chunk, max_iterations - first)
        cnt = torch.full((first + n + 2 * BAND,), COUNT_SENTINEL, dtype=torch.int64, device="cuda")
        ops.ck(ops.lib.unet_vol_thin_iterations(ops.h, X, Y, Z, first, n, 1 if endpoints else 0, cnt.data_ptr() + 8 * BAND, wp, wsb, ops.s), "iterations")
        calls += 1
        ch = cnt.cpu().numpy()
        bands = bands and bool((ch[:BAND + first] == COUNT_SENTINEL).all() and (ch[BAND + first + n:] == COUNT_SENTINEL).all())          # only removed[first .. first + n - 1]
        got = ch[BAND + first:BAND + first + n]
        empty = np.flatnonzero(got == 0)
        if empty.size:
            removed.extend(int(v) for v in got[:int(empty[0]) + 1])
            break
        removed.extend(int(v) for v in got)
        first += n
    ops.ck(ops.lib.unet_vol_thin_end(ops.h, X, Y, Z, dst.data_ptr() + BAND + out_off, wp, wsb, ops.s), "end")
    dh, wh = dst.cpu().numpy(), ws.cpu().numpy()
    bands = bands and bool((dh[:BAND + out_off] == SENTINEL).all() and (dh[BAND + out_off + N:] == SENTINEL).all() and (wh[:BAND] == SENTINEL).all()
                           and (wh[BAND + wsb:] == SENTINEL).all())
    return dh[BAND + out_off:BAND + out_off + N].reshape(vol.shape, order="F"), np.asarray(removed, np.int64), bands, calls


def _check_thin(ops, vol, endpoints=True, max_iterations=None, **kw):
    got, removed, bands, calls = _thin(ops, vol, endpoints, max_iterations, **kw)
    want, iterations, wr = SO.thin(vol, endpoints, max_iterations)
    assert bands, (vol.shape, endpoints)
    assert np.array_equal(removed, wr), (vol.shape, endpoints, removed.tolist(), wr.tolist())
    assert np.array_equal(got, want), (vol.shape, endpoints, int(np.count_nonzero(got != want)))
    assert len(removed) == iterations and int(removed.sum()) == int((vol != 0).sum()) - int(got.sum())
    return got, removed, calls


# ---- the thinning -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("X", XS)
def test_thinning_over_row_lengths_and_degenerate_extents(X):
    ops = Ops()
    for Y, Z in MAIN_YZ:
        vol = _asserted_content((X, Y, Z))
        assert all(vol[tuple(f)].any() for f in ((0,), (-1,), (slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)))
        for endpoints in (True, False):
            got, removed, _ = _check_thin(ops, vol, endpoints)
            assert int((removed > 0).sum()) >= 2 and got.any()
    for si, (Y, Z) in enumerate(DEGENERATE_YZ):
        vol = _content((X, Y, Z), 50 + si)
        if not vol.any():
            vol[0, 0, 0] = 1
        for endpoints in (True, False):
            _check_thin(ops, vol, endpoints)


def test_thinning_of_the_phantoms():
    ops = Ops()
    got, removed, _ = _check_thin(ops, SO.three_armed_tube())
    assert int(got.sum()) == 51 and removed.tolist() == [1240, 337, 0]
    got, _, _ = _check_thin(ops, SO.torus())
    assert int(got.sum()) == 56 and (SO.degrees(got) == 2).all()
    assert int(_check_thin(ops, SO.ball(), True)[0].sum()) == 2 and int(_check_thin(ops, SO.ball(), False)[0].sum()) == 1


def test_thinning_chunks_limits_reruns_and_alignment():
    ops = Ops()
    vol = _asserted_content((130, 12, 9))
    full = SO.thin(vol)[1]
    assert full >= 3
    a, ra, calls_a = _check_thin(ops, vol, chunk=1)
    b, rb, calls_b = _check_thin(ops, vol, chunk=8)
    assert calls_a == full and calls_b == 1 and np.array_equal(a, b) and np.array_equal(ra, rb)
    for limit in (0, 1, 2, full, full + 3):
        got, removed, calls = _check_thin(ops, vol, max_iterations=limit, chunk=2)          # stops where the oracle's truncated loop stops
        assert len(removed) == min(limit, full)
    assert np.array_equal(_check_thin(ops, vol, max_iterations=0)[0], vol)
    c, rc, _ = _check_thin(ops, vol)                                 # a second run: the same bits
    assert np.array_equal(a, c) and np.array_equal(ra, rc)
    for in_off, out_off in ((1, 0), (0, 3), (5, 7)):                   # byte offsets that break the 8-byte alignment of input and output
        for endpoints in (True, False):
            _check_thin(ops, vol, endpoints, in_off=in_off, out_off=out_off)
    empty = np.zeros((65, 9, 12), np.uint8, order="F")
    got, removed, _ = _check_thin(ops, empty)
    assert removed.tolist() == [0] and not got.any()


def test_thinning_refusals_launch_nothing():
    ops = Ops()
    lib = ops.lib
    X, Y, Z = 65, 9, 12
    N = X * Y * Z
    wsb = int(lib.unet_vol_thin_ws_bytes(X, Y, Z))
    assert wsb == 2 * (2 * Y * Z * 8) and lib.unet_vol_thin_ws_bytes(-1, 2, 2) == 0 and lib.unet_vol_thin_ws_bytes(0, 2, 2) == 0 and lib.unet_vol_thin_ws_bytes(2048, 2048, 512) == 0
    src = torch.ones(N, dtype=torch.uint8, device="cuda")
    ws = torch.full((wsb + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full((N,), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((16,), COUNT_SENTINEL, dtype=torch.int64, device="cuda")
    sp, wp, dp, cp = src.data_ptr(), ws.data_ptr() + BAND, dst.data_ptr(), cnt.data_ptr()
    begin = lambda *a: lib.unet_vol_thin_begin(ops.h, *a, ops.s)
    its = lambda *a: lib.unet_vol_thin_iterations(ops.h, *a, ops.s)
    end = lambda *a: lib.unet_vol_thin_end(ops.h, *a, ops.s)
    refused = [begin(None, X, Y, Z, wp, wsb), begin(sp, X, Y, Z, None, wsb), begin(sp, X, Y, Z, wp, wsb - 1), begin(sp, X, Y, Z, wp + 8, wsb), begin(sp, -1, Y, Z, wp, wsb),
               begin(sp, 2048, 2048, 512, wp, wsb), begin(wp + 16, X, Y, Z, wp, wsb),
               its(X, Y, Z, -1, 1, 1, cp, wp, wsb), its(X, Y, Z, 0, -1, 1, cp, wp, wsb), its(X, Y, Z, 0, 1, 2, cp, wp, wsb), its(X, Y, Z, 0, 1, 1, None, wp, wsb),
               its(X, Y, Z, 0, 1, 1, cp + 4, wp, wsb), its(X, Y, Z, 0, 1, 1, cp, None, wsb), its(X, Y, Z, 0, 1, 1, cp, wp, wsb - 1), its(X, Y, -2, 0, 1, 1, cp, wp, wsb),
               its(X, Y, Z, 0, 1, 1, wp + 64, wp, wsb),
               end(X, Y, Z, None, wp, wsb), end(X, Y, Z, dp, None, wsb), end(X, Y, Z, dp, wp, wsb - 1), end(X, Y, Z, wp + 32, wp, wsb), end(X, -1, Z, dp, wp, wsb)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert (ws.cpu().numpy() == SENTINEL).all() and (dst.cpu().numpy() == SENTINEL).all() and (cnt.cpu().numpy() == COUNT_SENTINEL).all()
    ok = [its(X, Y, Z, 3, 0, 1, cp, wp, wsb), begin(sp, 0, Y, Z, wp, wsb), its(0, Y, Z, 0, 2, 1, cp, wp, wsb), end(X, 0, Z, dp, wp, wsb)]          # nothing to do: no launch
    torch.cuda.synchronize()
    assert ok == [0, 0, 0, 0]
    assert (ws.cpu().numpy() == SENTINEL).all() and (dst.cpu().numpy() == SENTINEL).all() and (cnt.cpu().numpy() == COUNT_SENTINEL).all()


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------------------
def _table(ops, vol, d2=None, capacity=None, offset=0):
    """count, the total, emit -> (rc of emit, total, index, nbr, vals, bands); capacity: None = the total"""
    X, Y, Z = vol.shape
    N = vol.size
    src = torch.zeros(N + offset + 16, dtype=torch.uint8, device="cuda")
    src[offset:offset + N] = torch.from_numpy(_flat(vol != 0).astype(np.uint8) * 7).cuda()
    wsb = int(ops.lib.unet_vol_skeleton_ws_bytes(X, Y, Z))
    ws = torch.full((wsb + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    tot = torch.full((1 + 2 * BAND,), COUNT_SENTINEL, dtype=torch.int64, device="cuda")
    wp = ws.data_ptr() + BAND
    ops.ck(ops.lib.unet_vol_skeleton_count(ops.h, src.data_ptr() + offset, X, Y, Z, tot.data_ptr() + 8 * BAND, wp, wsb, ops.s), "count")
    th = tot.cpu().numpy()
    total = int(th[BAND])
    cap = total if capacity is None else capacity
    idx = torch.full((cap + 2 * BAND,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    nbr = torch.full((cap + 2 * BAND,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    val = torch.full((cap + 2 * BAND,), -7.0, dtype=torch.float64, device="cuda")
    dd = None if d2 is None else ops.d(_flat(d2), np.float64)
    rc = ops.lib.unet_vol_skeleton_emit(ops.h, src.data_ptr() + offset, X, Y, Z, None if dd is None else dd.data_ptr(), total, cap, idx.data_ptr() + 4 * BAND,
                                        nbr.data_ptr() + 4 * BAND, None if dd is None else val.data_ptr() + 8 * BAND, wp, wsb, ops.s)
    torch.cuda.synchronize()
    ih, nh, vh, wh = idx.cpu().numpy(), nbr.cpu().numpy(), val.cpu().numpy(), ws.cpu().numpy()
    bands = bool((th[:BAND] == COUNT_SENTINEL).all() and (th[BAND + 1:] == COUNT_SENTINEL).all() and (wh[:BAND] == SENTINEL).all() and (wh[BAND + wsb:] == SENTINEL).all()
                 and all((a[:BAND] == s).all() and (a[BAND + cap:] == s).all() for a, s in ((ih, 0x5A5A5A5A), (nh, 0x5A5A5A5A), (vh, -7.0))) and (dd is not None or (vh == -7.0).all()))
    return rc, total, ih[BAND:BAND + cap], nh[BAND:BAND + cap].view(np.uint32), vh[BAND:BAND + cap], bands


@pytest.mark.parametrize("shape", [(130, 12, 9), (65, 9, 12), (64, 12, 9), (63, 2, 9), (1, 12, 12), (1, 1, 1), (300, 70, 3)])
def test_skeleton_table(shape):
    ops = Ops()
    rng = np.random.default_rng(sum(shape))
    dense = _content(shape, 3)
    thin = SO.thin(dense)[0]
    d2 = np.asfortranarray(rng.random(shape) * 50.0)
    for vol in (thin, dense):
        if not vol.any():
            vol = vol.copy(); vol[0, 0, 0] = 1
        wi, wn, wv = SO.table(vol, d2)
        for dd, off in ((d2, 0), (None, 0), (d2, 3)):
            rc, total, idx, nbr, vals, bands = _table(ops, vol, dd, offset=off)                      # a capacity equal to the total
            assert rc == 0 and bands and total == len(wi)
            assert np.array_equal(idx, wi) and (np.diff(idx) > 0).all() and np.array_equal(nbr, wn)
            assert dd is None or np.array_equal(vals, wv)
        if len(wi):
            rc, total, idx, nbr, vals, bands = _table(ops, vol, d2, capacity=len(wi) - 1)            # one below: refused, nothing written
            assert rc != 0 and bands and (idx == 0x5A5A5A5A).all() and (vals == -7.0).all()
            rc, total, idx, nbr, vals, bands = _table(ops, vol, d2, capacity=len(wi) + 5)            # above: the rows past the total stay
            assert rc == 0 and bands and np.array_equal(idx[:len(wi)], wi) and (idx[len(wi):] == 0x5A5A5A5A).all() and (vals[len(wi):] == -7.0).all()
    rc, total, idx, nbr, vals, bands = _table(ops, np.zeros(shape, np.uint8), d2)                   # an empty mask
    assert rc == 0 and bands and total == 0 and idx.size == 0


def test_skeleton_table_refusals_and_the_public_table():
    from covidseg_amd import skeleton as SK
    ops = Ops()
    lib = ops.lib
    vol = _content((65, 9, 12), 1)
    N = vol.size
    src = ops.d(_flat(vol), np.uint8)
    wsb = int(lib.unet_vol_skeleton_ws_bytes(65, 9, 12))
    ws = torch.full((wsb + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"); out2 = torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    tot = torch.full((2,), COUNT_SENTINEL, dtype=torch.int64, device="cuda")
    wp, n = ws.data_ptr() + BAND, int(vol.sum())
    count = lambda *a: lib.unet_vol_skeleton_count(ops.h, *a, ops.s)
    emit = lambda *a: lib.unet_vol_skeleton_emit(ops.h, *a, ops.s)
    d2 = ops.d(np.zeros(N), np.float64)
    refused = [count(None, 65, 9, 12, tot.data_ptr(), wp, wsb), count(src.data_ptr(), 65, 9, 12, None, wp, wsb), count(src.data_ptr(), 65, 9, 12, tot.data_ptr() + 4, wp, wsb),
               count(src.data_ptr(), 65, 9, 12, tot.data_ptr(), wp, wsb - 1), count(src.data_ptr(), 65, -9, 12, tot.data_ptr(), wp, wsb),
               emit(src.data_ptr(), 65, 9, 12, None, n, n, None, out2.data_ptr(), None, wp, wsb), emit(src.data_ptr(), 65, 9, 12, None, n, n, out.data_ptr() + 2, out2.data_ptr(), None, wp, wsb),
               emit(src.data_ptr(), 65, 9, 12, d2.data_ptr(), n, n, out.data_ptr(), out2.data_ptr(), None, wp, wsb),          # d2 without vals
               emit(src.data_ptr(), 65, 9, 12, None, n, n, out.data_ptr(), out.data_ptr(), None, wp, wsb),                     # two outputs overlap
               emit(src.data_ptr(), 65, 9, 12, None, -1, n, out.data_ptr(), out2.data_ptr(), None, wp, wsb), emit(src.data_ptr(), 65, 9, 12, None, n, n, out.data_ptr(), out2.data_ptr(), None, wp, 0)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert (ws.cpu().numpy() == SENTINEL).all() and (out.cpu().numpy() == 0x5A5A5A5A).all() and (out2.cpu().numpy() == 0x5A5A5A5A).all() and (tot.cpu().numpy() == COUNT_SENTINEL).all()
    from scipy import ndimage
    wide = np.asfortranarray(ndimage.binary_dilation(vol, np.ones((3, 3, 3)), iterations=2).astype(np.uint8))
    p = (0.8, 0.8, 2.5)
    t = SK.skeleton_table(vol, radius_of=wide, pixdim=p)
    wi, wn, wv = SO.table(vol, VS.edt_sq_lines(wide, False, p))
    assert np.array_equal(t["index"], wi) and np.array_equal(t["neighbours"], wn) and np.array_equal(t["degree"], SO.popcount(wn)) and np.array_equal(t["radius_mm"], np.sqrt(wv))
    x, y, z = np.unravel_index(wi, vol.shape, order="F")
    assert np.array_equal(t["x"], x) and np.array_equal(t["y"], y) and np.array_equal(t["z"], z)
    assert "radius_mm" not in SK.skeleton_table(torch.from_numpy(_flat(vol)).cuda(), shape=vol.shape).dtype.names


# ---- the label spread -----------------------------------------------------------------------------------------------------------------------------------------------
def _spread(ops, arrival, labels, conn, first=1, n=None, chunk=64):
    X, Y, Z = arrival.shape
    N = arrival.size
    reached = arrival[arrival != 0xFFFF]
    steps = int(reached.max()) if reached.size else 0
    last = steps if n is None else min(steps, first + n - 1)
    arr = torch.from_numpy(_flat(arrival).view(np.int16)).cuda()
    lab = torch.full((N + 2 * BAND,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lab[BAND:BAND + N] = torch.from_numpy(_flat(labels).astype(np.int32)).cuda()
    s = first
    while s <= last:
        k = min(chunk, last - s + 1)
        ops.ck(ops.lib.unet_vol_label_spread(ops.h, arr.data_ptr(), lab.data_ptr() + 4 * BAND, X, Y, Z, s, k, conn, ops.s), "spread")
        s += k
    lh = lab.cpu().numpy()
    return lh[BAND:BAND + N].reshape(arrival.shape, order="F"), bool((lh[:BAND] == 0x5A5A5A5A).all() and (lh[BAND + N:] == 0x5A5A5A5A).all())


@pytest.mark.parametrize("conn", [1, 2, 3])
def test_label_spread_every_connectivity(conn):
    ops = Ops()
    rng = np.random.default_rng(conn)
    for shape in ((65, 12, 9), (130, 9, 12), (63, 12, 1), (1, 9, 12)):
        mask = _content(shape, 5)
        seeds = np.zeros(shape, bool)
        inside = np.argwhere(mask != 0)
        seeds[tuple(inside[rng.choice(len(inside), max(3, len(inside) // 30), replace=False)].T)] = True
        arrival = LO.geodesic(seeds, mask, conn)[0]
        labels = np.zeros(shape, np.int32)
        labels[seeds] = rng.permutation(int(seeds.sum())) + 1
        want = SO.label_spread(arrival, labels, conn)
        assert int((arrival[arrival != 0xFFFF]).max()) >= 2 and len(np.unique(want)) > 2
        for chunk in (64, 1):
            got, bands = _spread(ops, arrival, labels, conn, chunk=chunk)
            assert bands and np.array_equal(got, want), (shape, conn, chunk)
        got, bands = _spread(ops, arrival, labels, conn, n=1)       # one step only
        assert bands and np.array_equal(got, SO.label_spread(arrival, labels, conn, 1, 1))


def test_label_spread_ties_and_refusals():
    ops = Ops()
    a = np.full((5, 3, 1), 0xFFFF, np.uint16, order="F"); a[:, 1, 0] = (0, 1, 2, 1, 0)              # the middle voxel is equidistant from two seeds
    l = np.zeros((5, 3, 1), np.int32, order="F"); l[0, 1, 0], l[4, 1, 0] = 7, 3
    for conn in (1, 2, 3):
        got, bands = _spread(ops, a, l, conn)
        assert bands and got[:, 1, 0].tolist() == [7, 7, 3, 3, 3] and np.array_equal(got, SO.label_spread(a, l, conn))
    b = np.full((3, 3, 1), 0xFFFF, np.uint16, order="F"); b[0, 0, 0] = b[2, 0, 0] = b[0, 2, 0] = 0; b[1, 1, 0] = 1          # three seeds diagonal to one voxel
    m = np.zeros((3, 3, 1), np.int32, order="F"); m[0, 0, 0], m[2, 0, 0], m[0, 2, 0] = 9, 4, 6
    assert _spread(ops, b, m, 2)[0][1, 1, 0] == 4 and _spread(ops, b, m, 1)[0][1, 1, 0] == 0          # no face neighbour arrived before it: it keeps its label
    arr = torch.from_numpy(_flat(a).view(np.int16)).cuda()
    lab = torch.full((15,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    f = lambda *x: ops.lib.unet_vol_label_spread(ops.h, *x, ops.s)
    refused = [f(None, lab.data_ptr(), 5, 3, 1, 1, 1, 1), f(arr.data_ptr(), None, 5, 3, 1, 1, 1, 1), f(arr.data_ptr(), lab.data_ptr(), 5, 3, 1, 0, 1, 1),
               f(arr.data_ptr(), lab.data_ptr(), 5, 3, 1, 1, -1, 1), f(arr.data_ptr(), lab.data_ptr(), 5, 3, 1, 1, 1, 4), f(arr.data_ptr(), lab.data_ptr(), 5, 3, 1, 1, 1, 0),
               f(arr.data_ptr(), lab.data_ptr(), 5, 3, 1, 65534, 2, 1), f(arr.data_ptr(), lab.data_ptr() + 2, 5, 3, 1, 1, 1, 1), f(arr.data_ptr() + 1, lab.data_ptr(), 5, 3, 1, 1, 1, 1),
               f(arr.data_ptr(), arr.data_ptr(), 5, 3, 1, 1, 1, 1), f(arr.data_ptr(), lab.data_ptr(), 5, -3, 1, 1, 1, 1)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert f(arr.data_ptr(), lab.data_ptr(), 5, 3, 1, 1, 0, 1) == 0 and f(arr.data_ptr(), lab.data_ptr(), 0, 3, 1, 1, 1, 1) == 0
    torch.cuda.synchronize()
    assert (lab.cpu().numpy() == 0x5A5A5A5A).all()


# ---- the public functions and the chain -------------------------------------------------------------------------------------------------------------------------------
def _host_chain(mask, pixdim, root, orientation=None, min_length_mm=3.0, min_ratio=1.5, conn=3, affine=None, close=1, fill=True):
    """prepare -> thin -> table -> graph -> prune -> root -> territories over the oracles: what airway_tree / vessel_tree compute, without a device"""
    import morph_oracle as MO
    from covidseg_amd import skeleton as SK
    if close:
        mask = MO.erosion(MO.dilation(mask, 3, close, 0), 3, close, 1)
    if fill:
        mask = MO.fill_holes(mask, 1)
    mask = np.asfortranarray(np.asarray(mask).astype(np.uint8))
    skel = SO.thin(mask)[0]
    idx, codes, d2 = SO.table(skel, VS.edt_sq_lines(mask, False, pixdim))
    g = SK.prune(SK.graph_from_table(SK._finish_table(idx, codes, mask.shape, np.sqrt(d2)), mask.shape, pixdim, affine), min_length_mm, min_ratio)
    t = SK.root_tree(g, root, orientation)
    si, sl = SK.branch_seed_labels(g)
    lab = np.zeros(mask.size, np.int32)
    lab[si] = sl
    lab = np.asfortranarray(lab.reshape(mask.shape, order="F") * (mask != 0))
    labels = SO.label_spread(LO.geodesic(lab != 0, mask, conn)[0], lab, conn)
    return mask, skel, g, t, labels


def _same_tree(got, mask, skel, g, t, labels, pixdim):
    assert got.mask.dtype == np.uint8 and np.array_equal(got.mask, mask)
    assert np.array_equal(got.skeleton.mask, skel) and got.skeleton.voxels == int(skel.sum())
    assert len(got.graph.branches) == len(g.branches) and len(got.graph.nodes) == len(g.nodes)
    for rec_a, rec_b in ((got.graph.nodes, g.nodes), (got.graph.components, g.components), (got.graph.table, g.table)):
        assert rec_a.dtype == rec_b.dtype and all(np.array_equal(rec_a[k], rec_b[k], equal_nan=rec_a[k].dtype.kind == "f") for k in rec_a.dtype.names)
    for a, b in zip(got.graph.branches, g.branches):
        assert (a.a, a.b, a.length_mm, a.chord_mm, a.radius_min, a.radius_mean, a.radius_max) == (b.a, b.b, b.length_mm, b.chord_mm, b.radius_min, b.radius_mean, b.radius_max)
        assert np.array_equal(a.path, b.path)
    assert np.array_equal(got.tree.generation, t.generation) and np.array_equal(got.tree.parent, t.parent) and np.array_equal(got.tree.closes_cycle, t.closes_cycle)
    assert np.array_equal(got.tree.roots, t.roots)
    assert got.territories.labels.dtype == np.int32 and np.array_equal(got.territories.labels, labels)
    vox = np.bincount(labels.reshape(-1), minlength=len(g.branches) + 1)[1:]
    assert np.array_equal(got.territories.voxels, vox) and np.array_equal(got.territories.ml, vox * float(np.prod(pixdim)) / 1000.0)
    gens = got.generations
    assert gens["generation"].tolist() == sorted(set(t.generation[t.generation >= 0].tolist())) and int(gens["branches"].sum()) == int((t.generation >= 0).sum())
    assert int(gens["voxels"].sum()) == int(vox[t.generation >= 0].sum()) and got.cycles == int(g.components["cycles"].sum())


def test_thin_volume_sources_and_the_graph(tmp_path):
    from covidseg_amd import nifti_min
    from covidseg_amd import skeleton as SK
    vol = SO.three_armed_tube()
    want, iterations, removed = SO.thin(vol)
    sk = SK.thin_volume(vol)
    assert sk.mask.dtype == np.uint8 and np.array_equal(sk.mask, want) and sk.iterations == iterations == 3 and np.array_equal(sk.removed, removed) and sk.voxels == 51
    assert sk.removed.dtype == np.int64 and sk.shape == vol.shape
    path = tmp_path / "tube.nii.gz"
    nifti_min.write(path, vol, nifti_min.default_header(vol.shape))
    assert np.array_equal(SK.thin_volume(path).mask, want) and np.array_equal(SK.thin_volume(nifti_min.read(path), chunk=1).mask, want)
    dev = SK.thin_volume(torch.from_numpy(_flat(vol)).cuda(), shape=vol.shape, return_device=True)
    assert dev.mask.is_cuda and np.array_equal(dev.mask.cpu().numpy().reshape(vol.shape, order="F"), want)
    assert np.array_equal(SK.thin_volume(vol, endpoints=False, max_iterations=1).mask, SO.thin(vol, False, 1)[0])
    g = SK.skeleton_graph(sk, (1.0, 1.0, 1.0), radius_of=vol)
    assert sorted(g.nodes["kind"].tolist()) == ["end", "end", "end", "junction"] and len(g.branches) == 3
    assert sorted(SK.root_tree(g, "thickest").generation.tolist()) == [0, 1, 1]
    gd = SK.skeleton_graph(dev, (1.0, 1.0, 1.0), radius_of=vol)
    assert np.array_equal(gd.table, g.table)
    terr = SK.branch_territories(vol, sk, g)
    assert (terr.labels[vol != 0] > 0).all() and (terr.labels[vol == 0] == 0).all() and int(terr.voxels.sum()) == int(vol.sum()) == 1628
    none = SK.thin_volume(np.zeros((5, 4, 3), np.uint8))
    assert none.iterations == 1 and none.removed.tolist() == [0] and none.voxels == 0 and len(SK.skeleton_graph(none, (1.0, 1.0, 1.0)).nodes) == 0


def test_airway_tree_on_the_lung_phantom():
    from covidseg_amd import lungs as L
    from covidseg_amd import skeleton as SK
    from test_gpu_lungmask import _phantom
    ph, want, _ = _phantom(False, "z-")
    air = np.asfortranarray(want["airways"]["mask"])
    chain = _host_chain(air, ph["pixdim"], "superior", "LPI")
    got = SK.airway_tree(air, pixdim=ph["pixdim"], orientation="LPI")
    _same_tree(got, *chain, ph["pixdim"])
    assert len(got.graph.branches) == 3 and sorted(got.tree.generation.tolist()) == [0, 1, 1] and got.cycles == 0 and got.skeleton.iterations >= 3          # trachea, two bronchi
    raw = SK.airway_tree(air, pixdim=ph["pixdim"], orientation="LPI", close=0, fill=False)          # as grown: the noise leaves cavities, and thinning keeps them
    _same_tree(raw, *_host_chain(air, ph["pixdim"], "superior", "LPI", close=0, fill=False), ph["pixdim"])
    assert raw.cycles >= 1 and np.array_equal(raw.mask, air)
    root = int(got.tree.roots[0])
    assert got.graph.nodes["z"][root] == got.graph.nodes["z"][got.graph.nodes["kind"] == "end"].min()          # "z-": the superior end is the lowest z
    lm = L.lung_mask(np.asfortranarray(ph["hu"]), pixdim=ph["pixdim"], orientation="LPI")
    _same_tree(SK.airway_tree(lm, orientation="LPI"), *chain, ph["pixdim"])
    with pytest.raises(ValueError, match="not guessed"):
        SK.airway_tree(lm)
    with pytest.raises(ValueError, match="did not run"):
        SK.airway_tree(L.lung_mask(np.asfortranarray(ph["hu"]), pixdim=ph["pixdim"], airways=False), orientation="LPI")


def test_vessel_tree_on_two_tubes():
    from covidseg_amd import skeleton as SK
    p = (0.9, 0.9, 1.2)
    vol = SO.tubes((70, 40, 36), (((6, 8, 5), (30, 20, 18), 3.2), ((30, 20, 18), (62, 10, 30), 2.0), ((30, 20, 18), (58, 34, 28), 2.0), ((8, 33, 6), (40, 33, 8), 2.4)))
    chain = _host_chain(vol, p, "thickest", conn=3, close=0)         # vessel_tree's default: holes filled, no closing
    got = SK.vessel_tree(vol, pixdim=p)
    assert np.array_equal(got.mask, vol)
    _same_tree(got, *chain, p)
    assert len(got.graph.components) == 2 and len(got.tree.roots) == 2 and sorted(got.tree.generation.tolist()).count(0) == 2 and got.cycles == 0
    chain1 = _host_chain(vol, p, "thickest", min_length_mm=0.0, min_ratio=None, conn=1, close=1)
    _same_tree(SK.vessel_tree(vol, pixdim=p, min_length_mm=0.0, min_ratio=None, connectivity=1, close=1), *chain1, p)


def test_segment_volume_adds_the_airway_tree():
    from covidseg_amd import skeleton as SK
    from covidseg_amd import volume as V
    from test_gpu_lungmask import _ct_volume, _model, _phantom, _same
    ph, want, _ = _phantom(False, "z-")
    vol, model = _ct_volume(ph), _model()
    t = float(np.median(model.predict(V.load_volume(vol, "cts", img_size=128, new_dim=64), batch_size=8)))
    kw = dict(threshold=t, batch_size=8, img_size=128, lesions=True)
    base = V.segment_volume(vol, model, lungs=True, **kw)
    found = V.segment_volume(vol, model, lungs=True, airway_tree=True, **kw)
    assert not hasattr(base, "airway_tree") and "airway_tree" not in base.seconds
    assert isinstance(found.airway_tree, SK.CenterlineTree) and found.airway_tree_error is None and found.seconds["airway_tree"] > 0
    _same_tree(found.airway_tree, *_host_chain(np.asfortranarray(want["airways"]["mask"]), ph["pixdim"], "superior", "LPI"), ph["pixdim"])
    _same({k: v for k, v in vars(found).items() if k not in ("airway_tree", "airway_tree_error")}, vars(base))
    tuned = V.segment_volume(vol, model, lungs=True, airway_tree=dict(min_length_mm=0.0, min_ratio=None, territories=False), **kw)
    assert tuned.airway_tree.territories is None and len(tuned.airway_tree.graph.branches) >= len(found.airway_tree.graph.branches)
    skipped = V.segment_volume(vol, model, lungs=dict(area_mm2=(1.0, 20.0)), airway_tree=True, **kw)          # no trachea of that area: the airway step says why
    assert skipped.airway_tree is None and "no trachea" in skipped.airway_tree_error

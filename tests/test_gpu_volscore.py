"""-m gpu: a mask volume against its ground truth (csrc/kernels_volscore.hip, covidseg_amd.volume.surface / distance_transform / score_volume /
segment_volume(truth=...)) against tests/volscore_oracle.py.

Bounds.  Counts, surfaces, the squared distance transform, the Hausdorff distances and the lesion tables are exact: np.array_equal / ==.  hd95: the two order
statistics are exact and two interpolation formulas differ by rounding only: 4 * 2^-53 relative.  asd / assd: every term of the sum is positive, so a summation
whose longest chain of additions is c errs by at most c * 2^-53 relative; c comes from the reduction shape include/unet_hip.h documents (volscore_oracle.sum_chain);
+ 1 for a square root, + 1 for the division, + 1 for the oracle's own division: (c + 3) * 2^-53.  Against scipy (another order of the three products: 2 more): c + 5."""
import math

import numpy as np
import pytest

import components_oracle as CO
import volscore_oracle as SO

pytestmark = pytest.mark.gpu

E_ARG = -1
ULP = 2.0 ** -53
SPACINGS = [(1.0, 1.0, 1.0), (0.7, 0.7, 1.25), (0.68359375, 0.68359375, 5.0), (0.3, 0.7, 1.1)]
SHAPES = [(1, 1, 1), (17, 1, 33), (63, 40, 6), (130, 70, 37), (257, 129, 65)]
INT_FIELDS = ("tp", "fp", "fn", "n_surface_pred", "n_surface_truth", "n_truth_lesions", "n_pred_lesions", "missed_lesions", "false_positive_lesions")


def _dev(a):
    import torch
    return torch.from_numpy(np.asfortranarray(np.asarray(a).astype(np.uint8)).reshape(-1, order="F").copy()).cuda()


def _edt(vol, nonzero, pixdim, ops=None):
    """unet_vol_edt_sq through ctypes -> float64 [X, Y, Z]"""
    import torch
    from gpu_util import Ops
    ops = ops or Ops()
    X, Y, Z = vol.shape
    d2 = torch.full((max(vol.size, 1),), -7.0, dtype=torch.float64, device="cuda")
    w = np.ascontiguousarray(np.asarray(pixdim, np.float64) ** 2)
    ops.ck(ops.lib.unet_vol_edt_sq(ops.h, _dev(vol).data_ptr(), X, Y, Z, 1 if nonzero else 0, w.ctypes.data, d2.data_ptr(), None, 0, ops.s), "vol_edt_sq")
    return d2[:vol.size].cpu().numpy().reshape(vol.shape, order="F")


def _check_edt(vol, nonzero, pixdim, what):
    got = _edt(vol, nonzero, pixdim)
    want = SO.edt_sq_lines(vol, nonzero, pixdim)
    bad = ~((got == want) | (np.isinf(got) & np.isinf(want) & (got > 0)))
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {bad.size} voxels differ; first at {np.argwhere(bad)[0]}: {got[bad][0]!r} against {want[bad][0]!r}"
    assert np.array_equal(got, want), what


@pytest.mark.parametrize("shape", SHAPES)
def test_edt_against_the_oracle(shape):
    """small shapes: every density x polarity x spacing; the two large ones walk through the combinations so that each value of each factor is met"""
    combos = [(d, nz, p) for d in (0.001, 0.05, 0.6) for nz in (True, False) for p in SPACINGS]
    if np.prod(shape) > 100000:
        step = 5 if np.prod(shape) < 1000000 else 7
        combos = combos[(len(shape) + shape[0]) % step::step]
        assert {c[0] for c in combos} == {0.001, 0.05, 0.6} and {c[1] for c in combos} == {True, False} and len({c[2] for c in combos}) >= 3
    for i, (density, nonzero, pixdim) in enumerate(combos):
        m = CO.random_mask(shape, density if nonzero else 1.0 - density, 17 + i)
        _check_edt(m, nonzero, pixdim, f"{shape} density {density} nonzero {nonzero} spacing {pixdim}")


def test_edt_corners_last_planes_and_no_feature():
    for shape in ((63, 40, 6), (130, 70, 37)):
        X, Y, Z = shape
        for pixdim in SPACINGS[1:]:
            for cx in (0, X - 1):
                for cy in (0, Y - 1):
                    for cz in (0, Z - 1):
                        m = np.zeros(shape, np.uint8); m[cx, cy, cz] = 1
                        _check_edt(m, True, pixdim, f"{shape} corner {(cx, cy, cz)}")
                        if pixdim == SPACINGS[1]:
                            _check_edt(1 - m, False, pixdim, f"{shape} corner {(cx, cy, cz)} as the only zero")
            for axis in range(3):
                m = np.zeros(shape, np.uint8)
                sl = [slice(None)] * 3; sl[axis] = shape[axis] - 1
                m[tuple(sl)] = CO.random_mask(shape, 0.3, axis)[tuple(sl)]
                _check_edt(m, True, pixdim, f"{shape} features in the last plane of axis {axis}")
        none = _edt(np.zeros(shape, np.uint8), True, SPACINGS[1])
        assert np.isinf(none).all() and (none > 0).all()
        assert np.isinf(_edt(np.ones(shape, np.uint8), False, SPACINGS[3])).all()
        assert not _edt(np.ones(shape, np.uint8), True, SPACINGS[3]).any()


def test_edt_zero_sized_volume_touches_nothing():
    import torch
    from gpu_util import Ops
    ops = Ops()
    d2 = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")
    w = np.ones(3)
    for shape in ((0, 5, 7), (4, 0, 3), (6, 2, 0)):
        assert ops.lib.unet_vol_edt_sq(ops.h, d2.data_ptr(), *shape, 1, w.ctypes.data, d2.data_ptr(), None, 0, ops.s) == 0
    torch.cuda.synchronize()
    assert bool((d2 == -7.0).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_surface_and_confusion_against_the_oracle(shape):
    import torch
    from covidseg_amd import volume as V
    for i, density in enumerate((0.05, 0.6, 0.93)):
        a, b = CO.random_mask(shape, density, 3 + i), CO.random_mask(shape, 0.5, 30 + i)
        if min(shape) > 4:
            a[2:-1, 1:-2, :] = 1                                      # a solid block that reaches two faces: interior voxels exist at every connectivity
        for c in (1, 2, 3):
            surf, n = V.surface_device(_dev(a), shape, c)
            want = SO.surface(a, c)
            got = surf.cpu().numpy().reshape(shape, order="F")
            assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, density, c)
            assert n == int(want.sum())
            assert np.array_equal(V.surface(a * 3, c), want)          # the public form; any non-zero value is foreground
        counts = V.confusion_device(_dev(a), _dev(b * 255), shape)
        assert counts.dtype == np.int64 and np.array_equal(counts, SO.confusion(a, b)), (shape, density)
    full = V.surface(np.ones(shape, bool), 3)
    inner = full[1:-1, 1:-1, 1:-1]
    assert full.sum() == full.size - inner.size and not inner.any()


def test_distance_transform_public_form():
    from covidseg_amd import volume as V
    m = CO.ellipsoids((96, 80, 40), 10, 0.0, 4)
    for pixdim in (SPACINGS[0], SPACINGS[1]):
        want = SO.edt_sq_lines(m, False, pixdim)
        assert np.array_equal(V.distance_transform(m, pixdim, squared=True), want)
        got = V.distance_transform(m.astype(bool), pixdim)
        ref = np.sqrt(want)
        rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
        print(f"device sqrt, spacing {pixdim}: {np.count_nonzero(got != ref)} of {got.size} values differ from numpy's correctly rounded sqrt; worst {rel.max():.3g}")
        assert rel.max() <= 2 * ULP                                   # one unit in the last place
        assert got.dtype == np.float64 and got.shape == m.shape and not got[m == 0].any()
    dev = V.distance_transform(_dev(m), SPACINGS[1], squared=True, return_device=True, shape=m.shape)
    assert np.array_equal(dev.cpu().numpy().reshape(m.shape, order="F"), SO.edt_sq_lines(m, False, SPACINGS[1]))


def _pair(shape, seed, count):
    """ellipsoids (truth) against a shifted copy without every third of them (misses) plus extra blobs (false positives)"""
    truth = CO.ellipsoids(shape, count, 0.0, seed)
    lab, _ = CO.label(truth, 1)
    kept = truth.copy(); kept[(lab % 3) == 1] = 0
    pred = np.roll(kept, (2, -1, 1), axis=(0, 1, 2)) | CO.ellipsoids(shape, 3, 0.0, seed + 50)
    return pred, truth


def _close(got, want, k, what):
    assert (got == want) or abs(got - want) <= k * ULP * abs(want), f"{what}: {got!r} against {want!r}: {abs(got - want) / (ULP * abs(want)):.2f} units of 2^-53, allowed {k}"


def _same_or_nan(a, b):
    return (a == b) or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _check_score(s, o, n_voxels, what):
    for k in INT_FIELDS[:5]:
        assert getattr(s, k) == o[k] and isinstance(getattr(s, k), int), (what, k)
    assert s.n_truth_lesions == o["n_t"] and s.n_pred_lesions == o["n_p"] and s.missed_lesions == o["missed_lesions"] and s.false_positive_lesions == o["false_positive_lesions"]
    for k in ("dice", "iou", "precision", "recall", "pred_ml", "truth_ml", "volume_error_ml", "lesion_recall", "lesion_precision"):
        assert _same_or_nan(getattr(s, k), o[k]), (what, k, getattr(s, k), o[k])
    for k in ("tp_per_slice", "fp_per_slice", "fn_per_slice"):
        assert np.array_equal(getattr(s, k), o[k]), (what, k)
    assert np.array_equal(s.per_slice_dice, o["per_slice_dice"], equal_nan=True)
    for k in ("hd", "hd_pred_to_truth", "hd_truth_to_pred"):
        assert getattr(s, k) == o[k], (what, k, getattr(s, k), o[k])
    c = SO.sum_chain(n_voxels)
    print(f"{what}: hd {s.hd!r} hd95 {s.hd95!r} / {o['hd95']!r} assd {s.assd!r} / {o['assd']!r} chain {c}")
    if math.isinf(o["hd"]) or o["hd"] == 0.0:
        for k in ("hd95", "asd_pred_to_truth", "asd_truth_to_pred", "assd"):
            assert getattr(s, k) == o[k], (what, k)
    else:
        _close(s.hd95, o["hd95"], 4, what + " hd95")
        for k in ("asd_pred_to_truth", "asd_truth_to_pred", "assd"):
            _close(getattr(s, k), o[k], c + 3, what + " " + k)
    return c


def _check_lesions(s, o, pred, truth, pixdim, lc):
    vox = float(np.prod(np.asarray(pixdim, np.float64)))
    for tab, labels, n, cover, flag, key in ((s.truth_lesions, o["labels_t"], o["n_t"], o["cover_t"], "detected", "detected"),
                                             (s.pred_lesions, o["labels_p"], o["n_p"], o["cover_p"], "matched", "matched")):
        st = CO.stats(labels, n)
        assert len(tab) == n and np.array_equal(tab["label"], np.arange(1, n + 1))
        for k in ("voxels", "x0", "x1", "y0", "y1", "z0", "z1"):
            assert np.array_equal(tab[k], st[k]), k
        for k in "xyz":
            assert np.array_equal(tab["c" + k], st["s" + k] / st["voxels"])
        assert np.array_equal(tab["ml"], st["voxels"] * vox / 1000.0)
        assert np.array_equal(tab["covered_voxels"], cover) and np.array_equal(tab["covered_share"], cover / st["voxels"]) and np.array_equal(tab[flag], o[key])


@pytest.mark.parametrize("pixdim", SPACINGS)
def test_score_volume_on_ellipsoid_pairs(pixdim):
    from covidseg_amd import volume as V
    for seed, (shape, c, lc, mov, count) in enumerate([((144, 112, 40), 1, 1, 1, 9), ((121, 99, 33), 2, 3, 5, 8), ((128, 96, 24), 3, 2, 1, 8)]):
        pred, truth = _pair(shape, seed, count)
        o = SO.score(pred, truth, pixdim, c, lc, 95.0, mov)
        assert o["fp"] > 0 and o["fn"] > 0 and o["missed_lesions"] > 0 and o["false_positive_lesions"] > 0 and 0 < o["hd"] < np.inf, "the case has misses and false positives"
        s = V.score_volume(pred, truth, pixdim, connectivity=c, lesion_connectivity=lc, min_overlap_voxels=mov)
        _check_score(s, o, pred.size, f"{shape} spacing {pixdim} c={c}")
        _check_lesions(s, o, pred, truth, pixdim, lc)
        assert V.score_volume(_dev(pred), truth.astype(bool), pixdim, connectivity=c, lesion_connectivity=lc, min_overlap_voxels=mov, shape=shape) == s
        if seed == 1 and pixdim == SPACINGS[1]:
            for q in (0.0, 50.0, 99.9, 100.0):
                o2 = SO.score(pred, truth, pixdim, c, lc, q, mov)
                s2 = V.score_volume(pred, truth, pixdim, connectivity=c, lesion_connectivity=lc, percentile=q, min_overlap_voxels=mov, lesions=False)
                _close(s2.hd95, o2["hd95"], 4, f"percentile {q}")
                assert s2.truth_lesions is None and s2.lesion_recall is None and s2.hd == s.hd
            assert s2.hd95 == s.hd                                    # the 100th percentile of the pooled distances is the Hausdorff distance


def test_empty_one_empty_and_identical_masks():
    from covidseg_amd import volume as V
    shape = (40, 33, 17)
    z = np.zeros(shape, np.uint8); m = CO.ellipsoids(shape, 4, 0.0, 1)
    for pred, truth in ((z, z), (z, m), (m, z), (m, m)):
        o = SO.score(pred, truth, SPACINGS[1])
        s = V.score_volume(pred, truth, SPACINGS[1])
        _check_score(s, o, m.size, "empty / identical")
        _check_lesions(s, o, pred, truth, SPACINGS[1], 1)
    s = V.score_volume(z, z)
    assert s.dice == 1.0 and s.iou == 1.0 and s.hd == s.hd95 == s.assd == 0.0 and math.isnan(s.precision) and math.isnan(s.lesion_recall)
    s = V.score_volume(m, z)
    assert s.dice == 0.0 and s.hd == s.hd95 == s.assd == s.asd_pred_to_truth == float("inf") and s.n_surface_truth == 0 and s.false_positive_lesions == s.n_pred_lesions > 0
    s = V.score_volume(m, m, SPACINGS[3])
    assert s.dice == 1.0 and s.hd == s.hd95 == s.assd == 0.0 and s.lesion_recall == 1.0 and s.lesion_precision == 1.0 and (s.truth_lesions["covered_share"] == 1.0).all()
    e = V.score_volume(np.zeros((0, 4, 4), np.uint8), np.zeros((0, 4, 4), np.uint8))
    assert e.dice == 1.0 and e.hd == 0.0 and e.tp == 0 and len(e.per_slice_dice) == 4


def test_full_size_volume():
    """512 x 512 x 301, spacing (0.7, 0.7, 1.25): 300 ellipsoids against their roll by (3, -2, 1) plus 20 more"""
    import torch
    from covidseg_amd import volume as V
    shape, pixdim = (512, 512, 301), (0.7, 0.7, 1.25)
    pred = CO.ellipsoids(shape, 300, 0, 5)
    truth = np.roll(pred, (3, -2, 1), axis=(0, 1, 2)) | CO.ellipsoids(shape, 20, 0, 9)
    pd, td = _dev(pred), _dev(truth)
    s = V.score_volume(pd, td, pixdim, shape=shape)
    assert V.score_volume(pd, td, pixdim, shape=shape) == s, "two runs give the same VolumeScore"
    counts = SO.confusion(pred, truth)
    assert np.array_equal(np.stack([s.tp_per_slice, s.fp_per_slice, s.fn_per_slice], 1), counts) and (s.tp, s.fp, s.fn) == tuple(int(v) for v in counts.sum(0))
    sa_dev, na = V.surface_device(pd, shape, 1)
    sb_dev, nb = V.surface_device(td, shape, 1)
    sa, sb = SO.surface(pred, 1), SO.surface(truth, 1)
    assert np.array_equal(sa_dev.cpu().numpy().reshape(shape, order="F"), sa) and np.array_equal(sb_dev.cpu().numpy().reshape(shape, order="F"), sb)
    assert (na, nb) == (int(sa.sum()), int(sb.sum())) == (s.n_surface_pred, s.n_surface_truth)
    print(f"full size: {na} and {nb} surface voxels, dice {s.dice:.4f}, hd {s.hd!r}, hd95 {s.hd95!r}, assd {s.assd!r}")
    d2_dev = V.edt_sq_device(sb_dev, shape, pixdim, True)
    assert torch.equal(d2_dev, V.edt_sq_device(sb_dev, shape, pixdim, True)), "two runs give bit-identical d2"
    d2_b = d2_dev.cpu().numpy().reshape(shape, order="F")
    d2_a = V.edt_sq_device(sa_dev, shape, pixdim, True).cpu().numpy().reshape(shape, order="F")
    del d2_dev
    rng = np.random.default_rng(2)
    for d2, feat, other, name in ((d2_b, sb, sa, "to the truth's surface"), (d2_a, sa, sb, "to the prediction's surface")):
        on = np.argwhere(other)                                       # half of the voxels from the other mask's surface, half from anywhere
        pts = np.concatenate([on[rng.choice(len(on), 1024, replace=False)], np.stack([rng.integers(0, n, 1024) for n in shape], 1)])
        want = SO.edt_sq_at(pts, np.argwhere(feat), pixdim)
        got = d2[pts[:, 0], pts[:, 1], pts[:, 2]]
        assert len(pts) == 2048 and np.array_equal(got, want), f"d2 {name}: {np.count_nonzero(got != want)} of {len(pts)} sampled voxels differ"
    assert s.hd_pred_to_truth == float(np.sqrt(d2_b[sa != 0].max())) and s.hd_truth_to_pred == float(np.sqrt(d2_a[sb != 0].max())) and s.hd == max(s.hd_pred_to_truth, s.hd_truth_to_pred)
    c = SO.sum_chain(pred.size)
    o = SO.surface_metrics(sa, sb, d2_b, d2_a)                        # the metric formulas on the device's own d2: the reductions alone
    _close(s.hd95, o["hd95"], 4, "hd95")
    for k in ("asd_pred_to_truth", "asd_truth_to_pred", "assd"):
        _close(getattr(s, k), o[k], c + 3, k)
    try:
        import scipy.ndimage as ndi
    except ImportError:
        print("full size: scipy does not import here; the scipy comparison did not run")
        return
    ea, eb = ndi.distance_transform_edt(sb == 0, sampling=pixdim), ndi.distance_transform_edt(sa == 0, sampling=pixdim)
    da, db = ea[sa != 0], eb[sb != 0]
    _close(s.hd, float(max(da.max(), db.max())), 4, "hd against scipy")
    _close(s.hd95, float(np.percentile(np.concatenate([da, db]), 95.0)), 4, "hd95 against scipy")
    _close(s.assd, (math.fsum(da) / len(da) + math.fsum(db) / len(db)) / 2.0, c + 5, "assd against scipy")


def test_segment_volume_with_truth(tmp_path):
    from test_gpu_volume import NEW_DIM, SIZE, _patient
    from covidseg_amd import volume as V
    from covidseg_amd.keras_like import UNetModel
    paths, (ct, lung, inf) = _patient(tmp_path)
    model = UNetModel(NEW_DIM, 1, seed=1)
    model.verbose = 0
    t = float(np.median(model.predict(V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM))))
    kw = dict(lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    plain = V.segment_volume(paths[0], model, **kw)
    assert plain.score is None and "score" not in plain.seconds
    res = V.segment_volume(paths[0], model, truth=paths[2], **kw)
    assert np.array_equal(res.mask, plain.mask) and res.total_ml == plain.total_ml and "score" in res.seconds
    assert isinstance(res.score, V.VolumeScore) and res.score == V.score_volume(res.mask, inf, res.pixdim)
    assert res.score == V.segment_volume(paths[0], model, truth=inf, **kw).score
    assert res.score.tp + res.score.fp == int(res.mask.sum()) and res.score.tp + res.score.fn == int(np.count_nonzero(inf))
    o = SO.score(res.mask, inf, res.pixdim)
    _check_score(res.score, o, res.mask.size, "segment_volume")
    c = 2
    sizes = np.sort(CO.stats(*CO.label(plain.mask, c))["voxels"])
    vox = float(np.prod(np.asarray(plain.pixdim, np.float64)))
    min_ml = (int(sizes[len(sizes) // 2]) + 0.5) * vox / 1000.0
    f = V.segment_volume(paths[0], model, truth=paths[2], min_lesion_ml=min_ml, connectivity=c, **kw)
    assert f.mask.sum() < plain.mask.sum(), "the filter removes something in this case"
    assert f.score == V.score_volume(f.mask, inf, f.pixdim, lesion_connectivity=c) and f.score != res.score
    assert f.score.n_pred_lesions == f.n_lesions and np.array_equal(f.score.pred_lesions["voxels"], f.lesions["voxels"])
    with pytest.raises(ValueError):
        V.segment_volume(paths[0], model, truth=inf[:, :, :-1], **kw)


def test_refused_arguments_launch_nothing():
    import torch
    from gpu_util import Ops
    from covidseg_amd import volume as V
    ops = Ops()
    X, Y, Z = 32, 16, 8
    N = X * Y * Z
    mask = torch.ones(N, dtype=torch.uint8, device="cuda")
    d2 = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    surf = torch.full((N,), 9, dtype=torch.uint8, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    gath = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(32768, dtype=torch.uint8, device="cuda")
    w = np.ones(3)
    edt = lambda x, y, z, wv: ops.lib.unet_vol_edt_sq(ops.h, mask.data_ptr(), x, y, z, 1, wv.ctypes.data, d2.data_ptr(), None, 0, ops.s)
    cap = V.EDT_MAX_DIM
    assert edt(cap + 1, 1, 1, w) == E_ARG and edt(1, cap + 1, 1, w) == E_ARG and edt(1, 1, cap + 1, w) == E_ARG and "above" in ops.ctx.last_error()
    assert edt(2048, 1024, 1024, w) == E_ARG and edt(-1, 4, 4, w) == E_ARG
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("inf")), (float("nan"), 1.0, 1.0)):
        assert edt(X, Y, Z, np.array(bad)) == E_ARG
    sf = lambda c, x=X: ops.lib.unet_vol_surface(ops.h, mask.data_ptr(), x, Y, Z, c, surf.data_ptr(), cnt.data_ptr(), ops.s)
    assert sf(0) == E_ARG and sf(4) == E_ARG and sf(1, -3) == E_ARG
    assert ops.lib.unet_vol_surface(ops.h, mask.data_ptr(), X, Y, Z, 1, mask.data_ptr(), cnt.data_ptr(), ops.s) == E_ARG
    assert ops.lib.unet_vol_confusion(ops.h, mask.data_ptr(), mask.data_ptr(), 65536, 32768, 1, cnt.data_ptr(), ops.s) == E_ARG
    assert ops.lib.unet_vol_surface_distances(ops.h, mask.data_ptr(), d2.data_ptr(), X, Y, Z, cnt.data_ptr(), gath.data_ptr(), N, ws.data_ptr(), 32767, ops.s) == E_ARG
    assert ops.lib.unet_vol_surface_distances(ops.h, mask.data_ptr(), d2.data_ptr(), X, Y, Z, cnt.data_ptr(), gath.data_ptr(), -1, ws.data_ptr(), 32768, ops.s) == E_ARG
    assert ops.lib.unet_vol_lesion_overlap(ops.h, None, -1, None, 0, X, Y, Z, cnt.data_ptr(), cnt.data_ptr(), ops.s) == E_ARG
    torch.cuda.synchronize()
    assert bool((d2 == -7.0).all()) and bool((surf == 9).all()) and bool((cnt == -7).all()) and bool((gath == -7.0).all()), "a refused call wrote to its outputs"
    big = np.zeros((cap + 1, 1, 1), np.uint8)
    for call in (lambda: V.distance_transform(big), lambda: V.score_volume(big, big), lambda: V.score_volume(np.ones((4, 4, 4)), np.ones((4, 4, 4))),
                 lambda: V.score_volume(np.ones((4, 4, 4), np.uint8), np.ones((4, 4, 5), np.uint8)), lambda: V.score_volume(big[:4], big[:4], pixdim=(1, 1, 0)),
                 lambda: V.score_volume(big[:4], big[:4], connectivity=4), lambda: V.score_volume(big[:4], big[:4], percentile=101)):
        with pytest.raises(ValueError):
            call()
    assert edt(X, Y, Z, w) == 0 and sf(1) == 0                       # the same buffers through the accepted calls
    torch.cuda.synchronize()
    assert bool((d2 == 0).all()) and int(cnt[0].item()) == N - (X - 2) * (Y - 2) * (Z - 2)

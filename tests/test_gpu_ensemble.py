"""-m gpu: csrc/kernels_ensemble.hip and volume.segment_volume_ensemble / vote_volume / dihedral against tests/ensemble_oracle.py.  Copies, integer sums and float32
operations that numpy performs one at a time: every comparison is array_equal."""
import numpy as np
import pytest

import ensemble_oracle as EO
import volume_oracle as VO

pytestmark = pytest.mark.gpu

F = np.float32
PASTE_RECTS = np.array([[[10, 12, 40, 100], [60, 8, 50, 110]], [[5, 5, 70, 90], [50, 20, 70, 100]], [[0, 0, 0, 0], [0, 0, 0, 0]]], np.int32)   # apart, overlapping, none


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the symmetries --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 7, 64, 65])          # an odd centre line, a full wave row, one past it
def test_dihedral_is_a_bit_exact_copy(d):
    import torch
    from covidseg_amd import volume as V
    rng = np.random.default_rng(d)
    a = rng.normal(size=(3, d, d)).astype(F)
    flat = a.reshape(-1).view(np.uint32)
    flat[0] = 0x7FC12345                                            # a NaN with a payload
    flat[1] = 0x80000000                                            # -0.0
    flat[2] = 0xFF800001                                            # a signalling NaN
    dev = torch.from_numpy(a).cuda()
    for code, name in enumerate(EO.TTA):
        want = EO.dihedral(a, name)
        got = V.dihedral(a, name)
        assert got.shape == a.shape and got.dtype == F and np.array_equal(_bits(got), _bits(want)), name
        back = V.dihedral(got, name, inverse=True)
        assert np.array_equal(_bits(back), _bits(a)), name
        assert np.array_equal(_bits(V.dihedral(got, EO.INVERSE[name])), _bits(a)), name
        t = V.dihedral(dev[..., None], code, return_device=True)    # [n, d, d, 1] device in, device out
        assert t.is_cuda and tuple(t.shape) == (3, d, d, 1) and np.array_equal(_bits(t.cpu().numpy()[..., 0]), _bits(want)), name


def test_entry_points_refuse_bad_arguments_and_take_empty_inputs():
    import torch
    from covidseg_amd import _lib, volume as V
    lib, ctx = V._ctx()
    s = V._stream()
    a = torch.zeros(64, dtype=torch.float32, device="cuda"); b = torch.zeros(64, dtype=torch.float32, device="cuda")
    m = torch.zeros(64, dtype=torch.uint8, device="cuda"); w = torch.zeros(64, dtype=torch.int32, device="cuda"); o = torch.zeros(64, dtype=torch.int64, device="cuda")
    E = -1                                                          # UNET_E_ARG
    assert lib.unet_vol_dihedral(ctx.handle, a.data_ptr(), 1, 8, 8, b.data_ptr(), s) == E and lib.unet_vol_dihedral(ctx.handle, a.data_ptr(), 1, 8, -1, b.data_ptr(), s) == E
    assert lib.unet_vol_dihedral(ctx.handle, a.data_ptr(), 1, 8, 1, a.data_ptr(), s) == E                   # dst = src
    assert lib.unet_vol_dihedral(ctx.handle, a.data_ptr(), -1, 8, 1, b.data_ptr(), s) == E and lib.unet_vol_dihedral(ctx.handle, None, 1, 8, 1, b.data_ptr(), s) == E
    assert lib.unet_vol_dihedral(ctx.handle, None, 0, 8, 1, None, s) == 0 and lib.unet_vol_dihedral(ctx.handle, None, 4, 0, 1, None, s) == 0
    assert lib.unet_vol_canvas_axpy(ctx.handle, a.data_ptr(), 1.0, a.data_ptr(), 64, 1, s) == E and lib.unet_vol_canvas_axpy(ctx.handle, a.data_ptr(), 1.0, b.data_ptr(), -1, 1, s) == E
    assert lib.unet_vol_canvas_axpy(ctx.handle, None, 1.0, None, 0, 1, s) == 0 and lib.unet_vol_canvas_div(ctx.handle, None, 1.0, 0, s) == 0
    assert lib.unet_vol_canvas_div(ctx.handle, None, 1.0, 4, s) == E
    assert lib.unet_vol_unslice_prob(ctx.handle, a.data_ptr(), 8, 4, 4, 4, 2, 2, b.data_ptr(), s) == E      # empty slice range
    assert lib.unet_vol_unslice_prob(ctx.handle, a.data_ptr(), 8, 4, 4, 4, 0, 5, b.data_ptr(), s) == E and lib.unet_vol_unslice_prob(ctx.handle, None, 8, 0, 4, 4, 0, 1, None, s) == 0
    assert lib.unet_vol_unslice_prob(ctx.handle, a.data_ptr(), 8, 2048, 2048, 512, 0, 1, b.data_ptr(), s) == E          # 2^31 voxels
    assert lib.unet_vol_vote_pack(ctx.handle, m.data_ptr(), 32, 1, w.data_ptr(), 64, s) == E and lib.unet_vol_vote_pack(ctx.handle, m.data_ptr(), -1, 1, w.data_ptr(), 64, s) == E
    assert lib.unet_vol_vote_pack(ctx.handle, None, 0, 1, None, 0, s) == 0 and lib.unet_vol_vote_pack(ctx.handle, None, 0, 1, w.data_ptr(), 64, s) == E
    red = lambda M, k, X=4, Y=4, Z=4, words=w: lib.unet_vol_vote_reduce(ctx.handle, words.data_ptr() if words is not None else None, M, X, Y, Z, k, m.data_ptr(), None, o.data_ptr(),
                                                                       o.data_ptr() + 64, o.data_ptr() + 128, o.data_ptr() + 256, s)
    assert red(0, 1) == E and red(33, 1) == E and red(2, 0) == E and red(2, 3) == E and red(2, 1, words=None) == E and red(2, 1, X=2048, Y=2048, Z=512) == E
    assert red(2, 1, Z=0) == 0 and red(2, 1) == 0
    torch.cuda.synchronize()
    assert "min_votes" in ctx.last_error() or "vote_reduce" in ctx.last_error()
    assert isinstance(_lib.UNetHipError("x"), RuntimeError)


# ---- the weighted mean -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 4097])
def test_canvas_axpy_and_div_round_every_operation_on_its_own(count):
    import torch
    from covidseg_amd import volume as V
    rng = np.random.default_rng(count)
    cs = [rng.random(count).astype(F) for _ in range(3)]
    ws = (0.3, 0.3, 0.4)                                            # not dyadic: a fused multiply-add or another order of the sum shows in the last bit
    acc = torch.full((count,), float("nan"), dtype=torch.float32, device="cuda")
    want = None
    for k, (c, w) in enumerate(zip(cs, ws)):
        V.canvas_axpy_device(torch.from_numpy(c).cuda(), w, acc, k == 0)
        want = EO.axpy(want, c, w, k == 0)
        assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want)), k
    mean, wsum = EO.weighted_mean(cs, ws)
    V.canvas_div_device(acc, wsum)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(mean))
    fused = (F(0.3) * cs[0].astype(np.float64) + F(0.3) * cs[1].astype(np.float64)).astype(F)          # what a contracted second step would give
    print(f"count {count}: {int((fused != EO.axpy(EO.axpy(None, cs[0], 0.3, True), cs[1], 0.3, False)).sum())} elements tell a fused sum from a rounded one")
    one = torch.full((count,), float("nan"), dtype=torch.float32, device="cuda")
    V.canvas_axpy_device(torch.from_numpy(cs[0]).cuda(), 1.0, one, True)
    V.canvas_div_device(one, 1.0)
    assert np.array_equal(_bits(one.cpu().numpy()), _bits(cs[0]))    # 1 p and p / 1 are exact


# ---- votes -----------------------------------------------------------------------------------------------------------------------------------------
def _members(shape, M, seed):
    """random masks of mixed density; from M = 2 on one all-one member, from 3 one all-zero, from 5 two identical ones; foreground values other than 1 too"""
    rng = np.random.default_rng(seed)
    ms = [((rng.random(shape) < rng.uniform(0.02, 0.8)) * rng.integers(1, 255)).astype(np.uint8) for _ in range(M)]
    if M >= 2:
        ms[1] = np.ones(shape, np.uint8)
    if M >= 3:
        ms[2] = np.zeros(shape, np.uint8)
    if M >= 5:
        ms[4] = ms[3].copy()
    return ms


def _check_vote(ms, rule):
    import torch
    from covidseg_amd import volume as V
    M, shape = len(ms), ms[0].shape
    k = EO.min_votes(rule, M)
    want = EO.reduce(EO.pack(ms), M, k)
    got = V.vote_volume(ms, rule)
    assert got.min_votes == k and got.mask.dtype == np.uint8 and got.votes.dtype == np.uint8 and got.mask.shape == shape
    for name in ("mask", "votes", "counts", "member_voxels", "pair", "hist"):
        g = getattr(got, name)
        assert g.shape == want[name].shape and np.array_equal(g, want[name]), (name, rule)
    assert got.counts.dtype == got.pair.dtype == got.hist.dtype == got.member_voxels.dtype == np.int64
    assert np.array_equal(got.pairwise_dice, EO.pairwise_dice(want["pair"]), equal_nan=True)
    assert got.unanimous_voxels == want["hist"][M] and got.uncertain_voxels == want["hist"][1:M].sum()
    dev = [torch.from_numpy(np.asfortranarray(m).reshape(-1, order="F")).cuda() for m in ms]               # device masks in, device out; the second run: identical
    again = V.vote_volume(dev, rule, return_device=True, shape=shape)
    assert again.mask.is_cuda and np.array_equal(again.mask.cpu().numpy().reshape(shape, order="F"), got.mask)
    assert np.array_equal(again.votes.cpu().numpy().reshape(shape, order="F"), got.votes)
    for name in ("counts", "member_voxels", "pair", "hist"):
        assert np.array_equal(getattr(again, name), getattr(got, name)), name


@pytest.mark.parametrize("M", [1, 2, 3, 32])
@pytest.mark.parametrize("shape", [(5, 7, 3), (64, 3, 2), (33, 31, 9)])
def test_vote_pack_and_reduce_against_the_oracle(shape, M):
    ms = _members(shape, M, 100 * M + shape[0])
    for rule in ("majority", "any", "all") + ((2,) if M >= 2 else ()):
        _check_vote(ms, rule)


@pytest.mark.parametrize("shape", [(64, 3, 2), (33, 31, 9), (256, 5, 2)])
def test_vote_reduce_skips_all_zero_waves(shape):
    """a wave of all-zero words followed by non-zero ones (and, on the larger shapes, workgroups with both kinds): the skipped waves still write their zeros and count
    into hist[0]"""
    rng = np.random.default_rng(7)
    X, Y, Z = shape
    ms = [(rng.random(shape) < 0.4).astype(np.uint8) for _ in range(3)]
    for m in ms:
        m[:, 0, :] = 0                                              # the first row(s) of every slice: (64, 3, 2) -> exactly the first wave of each slice
        m[:, :, 0][: X // 2] = 0
    for rule in ("majority", "any", 3):
        _check_vote(ms, rule)


# ---- the probability volume ------------------------------------------------------------------------------------------------------------------------
def synthetic_prob(n, d, seed):
    """smooth probability maps in [0.02, 0.98] that cross the thresholds along curves"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:d, 0:d].astype(np.float64) / d
    out = np.empty((n, d, d), F)
    for i in range(n):
        a, b, c = rng.uniform(2, 9, 3)
        out[i] = 0.5 + 0.48 * np.sin(a * u + c) * np.cos(b * v - c)
    return out


@pytest.mark.parametrize("shape", [(96, 80, 5), (121, 99, 5)])          # X a multiple of 4: the 16-byte stores; not one: the scalar kernel
def test_unslice_prob_is_what_unslice_thresholds(shape):
    import torch
    from covidseg_amd import volume as V
    S, d, z0, z1 = 128, 64, 1, 4
    prob = synthetic_prob(3, d, 1)
    canvas = V.paste_back(torch.from_numpy(prob).cuda(), PASTE_RECTS[:, 0], PASTE_RECTS[:, 1], S)
    got = V.unslice_prob(canvas, shape, z0, z1).cpu().numpy().reshape(shape, order="F")
    want = EO.unslice_prob(VO.paste_back(prob, PASTE_RECTS, S), shape, z0, z1)
    assert got.dtype == F and np.array_equal(_bits(got), _bits(want))
    assert not got[:, :, :z0].any() and not got[:, :, z1:].any() and got[:, :, z0:z1].any()
    for t in (0.3, 0.547, 0.8):
        mask_dev, counts_dev = V.unslice(canvas, t, shape, z0, z1)
        mask = mask_dev.cpu().numpy().reshape(shape, order="F")
        assert np.array_equal(got > F(t), mask != 0), t
        assert np.array_equal(counts_dev.cpu().numpy(), (got > F(t)).sum(axis=(0, 1))[z0:z1])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
SIZE, Z, NEW_DIM = 128, 20, 64


def _patient(tmp_path):
    """CT: int16 with slope / inter (Hounsfield-like); lung mask: two blobs per slice, empty on a few slices (one inside the kept range); infection mask"""
    from covidseg_amd import nifti_min
    from covidseg_amd.data import synthetic_ct
    x, y = synthetic_ct(Z, SIZE, seed=11)
    ct = np.empty((SIZE, SIZE, Z), np.int16, order="F"); lung = np.zeros((SIZE, SIZE, Z), np.uint8, order="F"); inf = np.zeros((SIZE, SIZE, Z), np.uint8, order="F")
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    z0, z1 = VO.trim_range(Z)
    for z in range(Z):
        ct[:, :, z] = np.round(x[z, :, :, 0] * 2800).astype(np.int16)
        if z not in (0, 1, z0 + 2, Z - 1):
            r = 1.0 + 0.02 * (z - Z / 2)
            lung[:, :, z] = (((xx - 38) / (22 * r)) ** 2 + ((yy - 64) / (40 * r)) ** 2 < 1) | (((xx - 90) / (24 * r)) ** 2 + ((yy - 66) / (38 * r)) ** 2 < 1)
        if z not in (z0 + 1, z0 + 4):
            inf[:, :, z] = (y[z, :, :, 0] > 0.5) * (1 + z % 2)
    hdr = nifti_min.default_header(ct.shape, (0.8, 0.8, 5.0))
    paths = [tmp_path / "ct.nii.gz", tmp_path / "lung.nii.gz", tmp_path / "inf.nii.gz"]
    nifti_min.write(paths[1], lung, hdr); nifti_min.write(paths[2], inf, hdr)
    import gzip, struct
    h = bytearray(hdr)                                              # the writer stores uint8 / float32 only: the int16 CT with slope 0.5 / inter -1000 is assembled here
    struct.pack_into("<2h", h, 70, 4, 16); struct.pack_into("<3f", h, 108, 352.0, 0.5, -1000.0)
    paths[0].write_bytes(gzip.compress(bytes(h) + b"\0\0\0\0" + ct.tobytes(order="F"), 1))
    return paths, (ct, lung, inf)


class _Stub:
    """clip(a x + b ramp, 0, 1) with a ramp that no symmetry of the square maps onto itself: a wrong or missing inverse transform changes the result"""

    def __init__(self, a, b, d=NEW_DIM):
        self.h, self.a, self.b = d, F(a), F(b)
        i, j = np.mgrid[0:d, 0:d].astype(F)
        self.ramp = ((F(1.7) * i + F(0.6) * j + i * j / F(d)) / F(3.3 * d)).astype(F)[None, :, :, None]
        self.calls = 0

    def __call__(self, x):
        return np.clip((self.a * np.asarray(x, F) + (self.b * self.ramp).astype(F)).astype(F), F(0), F(1)).astype(F)

    def predict(self, x, batch_size=32):
        self.calls += 1
        return self(x.cpu().numpy() if hasattr(x, "cpu") else x)


def _prepared(paths):
    """the batch and the rectangles segment_volume works with, from the public pieces"""
    from covidseg_amd import volume as V
    z0, z1 = VO.trim_range(Z)
    r1, r2, kept = V.load_volume(paths[1], "lungs", img_size=SIZE)
    x = V.load_volume(paths[0], "cts", img_size=SIZE, rects=(r1, r2, kept), box_indexing="slice", new_dim=NEW_DIM).cpu().numpy()
    plan = V.box_plan(z1 - z0, kept, "slice")
    rects = np.zeros((z1 - z0, 2, 4), np.int32)
    for i in np.nonzero(plan >= 0)[0]:
        rects[i, 0], rects[i, 1] = r1[plan[i]], r2[plan[i]]
    return x, rects, z0, z1


def test_ensemble_of_stub_members_equals_the_oracle(tmp_path):
    from covidseg_amd import nifti_min, volume as V
    paths, (ct, lung, inf) = _patient(tmp_path)
    stubs = [_Stub(0.9, 0.35), _Stub(0.6, 0.8)]
    tta, weights = ("id", "hflip", "rot90"), (0.3, 0.7)
    x, rects, z0, z1 = _prepared(paths)
    t = float(np.median(stubs[0](x)))
    for combine in ("mean", "majority"):
        pp, vp = tmp_path / f"prob_{combine}.nii.gz", tmp_path / f"votes_{combine}.nii"
        res = V.segment_volume_ensemble(paths[0], stubs, tta=tta, combine=combine, weights=weights, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE,
                                        return_prob=True, prob_path=pp, votes_path=vp)
        want = EO.ensemble(x, stubs, tta, weights, rects, SIZE, ct.shape, z0, z1, t, combine)
        assert res.members == [(0, "id"), (0, "hflip"), (0, "rot90"), (1, "id"), (1, "hflip"), (1, "rot90")] and res.combine == combine
        assert np.array_equal(res.mask, want["mask"]) and np.array_equal(res.counts, want["counts"]) and res.mask.any() and not res.mask.all()
        assert np.array_equal(res.votes, want["votes"]) and res.votes.dtype == np.uint8
        assert res.prob.dtype == F and np.array_equal(_bits(res.prob), _bits(want["prob"]))
        assert np.array_equal(res.vote_pair, want["pair"]) and np.array_equal(res.vote_hist, want["hist"])
        assert np.array_equal(res.pairwise_dice, EO.pairwise_dice(want["pair"]), equal_nan=True)
        assert np.array_equal(res.member_ml, want["member_voxels"] * res.voxel_ml)
        assert len(res.seconds["members"]) == 6 and res.fell_through == [2]
        assert np.array_equal(nifti_min.read(pp).raw, res.prob) and np.array_equal(nifti_min.read(vp).raw, res.votes)
        assert 0 < res.vote_hist[1:6].sum()                          # the members do disagree somewhere: the ramp moves with the symmetry
    assert len({int(v) for v in want["member_voxels"]}) > 2          # and a member's volume depends on its symmetry
    no_prob = V.segment_volume_ensemble(paths[0], stubs[:1], lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    assert no_prob.prob is None and np.array_equal(no_prob.votes, no_prob.mask)


@pytest.fixture(scope="module")
def real_models():
    from covidseg_amd.keras_like import UNetModel
    models = [UNetModel(NEW_DIM, 1, seed=s) for s in (1, 2)]
    for m in models:
        m.verbose = 0
    return models


def test_one_identity_member_is_segment_volume(tmp_path, real_models):
    import torch
    from covidseg_amd import volume as V
    paths, _ = _patient(tmp_path)
    model = real_models[0]
    x = V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM)
    p = model.predict(x, batch_size=8)
    assert torch.equal(model.predict_device(x, batch_size=8).cpu(), torch.from_numpy(p))          # the device loop returns predict's bits
    t = float(np.median(p))
    one = V.segment_volume(paths[0], model, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    ens = V.segment_volume_ensemble(paths[0], [model], lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    assert np.array_equal(ens.mask, one.mask) and np.array_equal(ens.counts, one.counts) and one.mask.any()
    assert ens.total_ml == one.total_ml and ens.infected_share == one.infected_share and ens.fell_through == one.fell_through
    assert np.array_equal(ens.votes, one.mask) and ens.vote_hist[1] == one.counts.sum()


def test_two_models_two_flips_keep_their_books(tmp_path, real_models):
    from covidseg_amd import volume as V
    paths, (ct, lung, inf) = _patient(tmp_path)
    x = V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM)
    t = float(np.median(real_models[0].predict(x, batch_size=8)))
    res = V.segment_volume_ensemble(paths[0], real_models, tta=("id", "vflip"), lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE, truth=paths[2],
                                    min_lesion_ml=0.05, combine="majority")
    X, Y, Zn = ct.shape
    N = X * Y * Zn
    assert res.members == [(0, "id"), (0, "vflip"), (1, "id"), (1, "vflip")] and res.votes.max() <= 4
    assert np.array_equal(res.counts, res.mask.sum(axis=(0, 1))) and res.counts.dtype == np.int64
    assert res.vote_hist.shape == (5,) and res.vote_hist.sum() == N
    hist = res.vote_hist
    assert res.unanimous_ml == float(hist[4]) * res.voxel_ml and res.uncertain_ml == float(hist[1:4].sum()) * res.voxel_ml
    # three products of an integer below 2^24 with voxel_ml, each within half an ulp of the true product, summed twice: the books close to within 4 ulp of the total
    total = N * res.voxel_ml
    assert abs(res.uncertain_ml + res.unanimous_ml + float(hist[0]) * res.voxel_ml - total) <= 4 * np.spacing(total)
    assert res.score is not None and 0.0 <= res.score.dice <= 1.0 and res.score.tp + res.score.fp == res.counts.sum()
    assert res.lesions is not None and res.n_lesions == len(res.lesions) and res.removed_ml >= 0.0
    assert (res.lesions["ml"] >= 0.05).all()
    assert np.array_equal(np.diag(res.vote_pair) * res.voxel_ml, res.member_ml) and np.array_equal(res.vote_pair, res.vote_pair.T)
    mean = V.segment_volume_ensemble(paths[0], real_models, tta=("id", "vflip"), lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE, return_prob=True)
    assert np.array_equal(mean.mask, (mean.prob > F(t)).astype(np.uint8)) and np.array_equal(mean.votes, res.votes) and np.array_equal(mean.vote_hist, res.vote_hist)

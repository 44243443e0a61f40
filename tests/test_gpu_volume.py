"""-m gpu: the volume path (csrc/kernels_volume.hip, covidseg_amd.volume) against tests/volume_oracle.py -- the forward kernel bit for bit, the paste-back
and the way back into the patient's volume, and file in -> dataset / mask volume out end to end."""
import numpy as np
import pytest

import volume_oracle as VO
from oracle import preprocess_oracle as P

pytestmark = pytest.mark.gpu

CODES = {"u1": 2, "i1": 256, "i2": 4, "u2": 512, "i4": 8, "u4": 768, "f4": 16, "f8": 64}
PASTE_RECTS = np.array([[[10, 12, 40, 100], [60, 8, 50, 110]], [[5, 5, 70, 90], [50, 20, 70, 100]], [[0, 0, 0, 0], [0, 0, 0, 0]]], np.int32)   # apart, overlapping, none


def synthetic_prob(n, d, seed):
    """smooth probability maps in [0.02, 0.98] that cross the threshold along curves (few pixels land within 1e-6 of it)"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:d, 0:d].astype(np.float64) / d
    out = np.empty((n, d, d), np.float32)
    for i in range(n):
        a, b, c = rng.uniform(2, 9, 3)
        out[i] = 0.5 + 0.48 * np.sin(a * u + c) * np.cos(b * v - c)
    return out


def _volume(shape, kind, seed):
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    a = 90 * np.sin(x / 7.0 + z) * np.cos(y / 5.0) + rng.normal(0, 20, shape)
    if kind.startswith("u"):
        a = a + 128
    if kind in ("i1", "u1"):
        a = np.clip(a / 2 + (64 if kind == "u1" else 0), -128 if kind == "i1" else 0, 127 if kind == "i1" else 255)
    if kind in ("i4", "u4"):
        a = a * 1000
    return np.asfortranarray(a.astype(kind))


def _run_slices(raw, slope, inter, z0, z1, S):
    from covidseg_amd import nifti_min, volume as V
    vol = nifti_min.NiftiVolume(np.asfortranarray(raw), slope, inter, (1.0, 1.0, 1.0), nifti_min.default_header(raw.shape), "<")
    st = V.slices_f64(vol, V.upload(vol), z0, z1, S, ("f32", "u8", "lung"))
    n = z1 - z0
    import torch
    img64 = st["_ws"][:n * S * S * 8].view(torch.float64).reshape(n, S, S)          # the workspace starts with the resized float64 images
    out = {k: v.cpu().numpy() for k, v in st.items() if k != "_ws"}
    out["img64"] = img64.cpu().numpy()
    return out


def _check_slices(raw, slope, inter, z0, z1, S):
    got = _run_slices(raw, slope, inter, z0, z1, S)
    want = VO.slices_f64(raw, slope, inter, z0, z1, S)
    assert np.array_equal(got["img64"], want["img64"], equal_nan=True), "resized float64 stage"
    assert np.array_equal(got["minmax"], want["minmax"], equal_nan=True)
    assert np.array_equal(got["f32"], want["f32"], equal_nan=True)
    assert np.array_equal(got["u8"], want["u8"]) and np.array_equal(got["lung"], want["lung"])
    assert np.array_equal(got["uniform"], want["uniform"])
    return got, want


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kind", sorted(CODES))
def test_slices_bit_exact_every_datatype(kind, scaled):
    raw = _volume((63, 40, 6), kind, 1)                               # image [Y = 40, X = 63] -> 32 x 32: the table path
    slope, inter = (float(np.float32(0.37)), float(np.float32(-1024.5))) if scaled else (0.0, 3.0)
    _check_slices(raw, slope, inter, 1, 5, 32)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("yx", [(32, 32), (64, 96), (40, 63), (20, 50), (63, 20), (50, 20)])
def test_slices_bit_exact_every_resize_case(yx, scaled):
    """S = 32: equal size, integer scales, the table path, both axes up-scaled, and the two mixed shapes"""
    Y, X = yx
    raw = _volume((X, Y, 5), "i2", 2)
    slope, inter = (float(np.float32(1.5)), float(np.float32(-1000.0))) if scaled else (float("nan"), 0.0)
    _check_slices(raw, slope, inter, 1, 4, 32)


def test_constant_slice_gives_what_numpy_gives_and_is_reported():
    from covidseg_amd import volume as V
    raw = _volume((48, 48, 10), "i2", 3)
    raw[:, :, 4] = -1000                                              # kept range of Z = 10 is 2..8: slice 2 of it
    got, want = _check_slices(raw, 0.0, 0.0, 2, 8, 32)
    assert list(got["uniform"]) == [0, 0, 1, 0, 0, 0]
    assert np.isnan(got["f32"][2]).all() and not got["u8"][2].any() and not got["lung"][2].any()
    with pytest.warns(RuntimeWarning, match=r"slices \[2\]"):
        x, info = V.load_volume(raw, "demo", img_size=32, return_info=True)
    assert info["flat"] == [2] and x.is_cuda and np.array_equal(x.cpu().numpy(), want["f32"], equal_nan=True)


def test_full_size_stage_by_stage():
    """int16 512 x 512 x 40 -> S = 512 (the equal-size path: the oracle vectorises) and one 630 x 630 slice -> 512 (the tables at the reference's other frame size)"""
    from covidseg_amd.data import synthetic_ct
    x = synthetic_ct(4, 512, seed=7)[0][..., 0]
    raw = np.empty((512, 512, 40), np.int16, order="F")
    for z in range(40):
        raw[:, :, z] = np.round(np.roll(x[z % 4], 13 * z, axis=1) * 2000).astype(np.int16) + z
    z0, z1 = VO.trim_range(40)
    _check_slices(raw, 0.5, -1000.0, z0, z1, 512)
    raw2 = _volume((630, 630, 3), "i2", 9)
    _check_slices(raw2, 0.0, 0.0, 1, 2, 512)


def _near_threshold(p64, t):
    return np.abs(p64 - t) <= 1e-6


def test_paste_back_and_unslice_against_the_oracle():
    import torch
    from covidseg_amd import volume as V
    S, d, t = 128, 64, 0.547
    shape, z0, z1 = (120, 100, 5), 1, 4
    prob = synthetic_prob(3, d, 1)
    dev = torch.from_numpy(prob).cuda()
    canvas = V.paste_back(dev, PASTE_RECTS[:, 0], PASTE_RECTS[:, 1], S)
    want = VO.paste_back(prob, PASTE_RECTS, S)
    got = canvas.cpu().numpy()
    assert np.array_equal(got, want)                                 # the same written-out operation order: the float32 canvases are equal
    inside = np.zeros((3, S, S), bool)
    for i in range(2):
        for x, y, w, h in PASTE_RECTS[i]:
            inside[i, y:y + h, x:x + w] = True
    assert not got[:2][~inside[:2]].any() and got[2].min() > 0        # 0 outside both rectangles; the slice without rectangles is sampled everywhere
    mask_dev, counts_dev = V.unslice(canvas, t, shape, z0, z1)
    mask = mask_dev.cpu().numpy().reshape(shape, order="F"); counts = counts_dev.cpu().numpy()
    wmask, wcounts, _ = VO.unslice(want, t, shape, z0, z1)
    c64 = VO.paste_back(prob, PASTE_RECTS, S, np.float64)
    _, _, p64 = VO.unslice(c64, t, shape, z0, z1, np.float64)
    near = _near_threshold(p64, t)                                   # [n, Y, X] image orientation
    differ = np.stack([np.rot90(mask[:, :, z0 + k] != wmask[:, :, z0 + k]) for k in range(z1 - z0)])
    print(f"paste/unslice: {int(differ.sum())} voxels differ from the oracle, {int(near.sum())} of {near.size} lie within 1e-6 of the threshold")
    assert not (differ & ~near).any()
    assert near.mean() <= 0.001
    assert np.array_equal(counts, [mask[:, :, z].sum() for z in range(z0, z1)]) and counts.dtype == np.int64
    assert not mask[:, :, :z0].any() and not mask[:, :, z1:].any()
    mask2, counts2 = V.unslice(V.paste_back(dev, PASTE_RECTS[:, 0], PASTE_RECTS[:, 1], S), t, shape, z0, z1)
    assert torch.equal(mask2, mask_dev) and torch.equal(counts2, counts_dev)          # two runs: bit-identical
    odd = V.unslice(canvas, t, (121, 99, 5), z0, z1)                  # X not a multiple of 4: the scalar kernel
    womask, wocounts, _ = VO.unslice(want, t, (121, 99, 5), z0, z1)
    assert np.array_equal(odd[1].cpu().numpy(), wocounts) and np.array_equal(odd[0].cpu().numpy().reshape((121, 99, 5), order="F"), womask)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
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
    # the writer stores uint8 / float32 only: the int16 CT with slope 0.5 / inter -1000 is assembled here at the specification's offsets
    import gzip, struct
    h = bytearray(hdr)
    struct.pack_into("<2h", h, 70, 4, 16); struct.pack_into("<3f", h, 108, 352.0, 0.5, -1000.0)
    paths[0].write_bytes(gzip.compress(bytes(h) + b"\0\0\0\0" + ct.tobytes(order="F"), 1))
    return paths, (ct, lung, inf)


def _oracle_dataset(ct, lung, inf, box_indexing):
    from covidseg_amd import volume as V
    z0, z1 = VO.trim_range(Z)
    n = z1 - z0
    L = VO.slices_f64(lung, 0.0, 0.0, z0, z1, SIZE)
    kept = [i for i in range(n) if not L["uniform"][i]]
    rects = [P.lung_rects(L["lung"][i]) for i in kept]
    plan = V.box_plan(n, kept, box_indexing)
    C = VO.slices_f64(ct, 0.5, -1000.0, z0, z1, SIZE); I = VO.slices_f64(inf, 0.0, 0.0, z0, z1, SIZE)
    cts, infs = [], []
    for i in range(n):
        if plan[i] >= 0:
            r1, r2 = rects[plan[i]]
            nrm, _, _ = VO.normalise(C["img64"][i])
            c = P.crop_resize_fuse(P.clahe_enhancer(nrm), r1, r2)
            m = P.crop_resize_fuse(I["u8"][i], r1, r2)
        else:
            c, m = C["u8"][i], I["u8"][i]                             # fell through: the whole frame, no CLAHE
        if np.unique(m).size == 1:                                    # T1:423
            continue
        cts.append(P.u8_to_unit(P.resize_u8(c, (NEW_DIM, NEW_DIM), P.INTER_LINEAR)))
        infs.append(P.u8_to_unit(P.resize_u8(m, (NEW_DIM, NEW_DIM), P.INTER_LINEAR)))
    return np.stack(cts)[..., None], np.stack(infs)[..., None], kept, rects, plan


@pytest.mark.parametrize("box_indexing", ["reference", "slice"])
def test_build_dataset_equals_the_oracle_chain(tmp_path, box_indexing):
    from covidseg_amd import volume as V
    paths, (ct, lung, inf) = _patient(tmp_path)
    x, y, report = V.build_dataset([tuple(paths)], img_size=SIZE, new_dim=NEW_DIM, box_indexing=box_indexing, return_info=True)
    wx, wy, kept, rects, plan = _oracle_dataset(ct, lung, inf, box_indexing)
    assert x.dtype == y.dtype == np.float32 and x.shape == y.shape == wx.shape
    assert np.array_equal(x, wx) and np.array_equal(y, wy)
    assert report[0]["fell_through"] == [int(i) for i in np.nonzero(plan < 0)[0]] and len(report[0]["dropped"]) >= 2
    r1, r2, k = V.load_volume(paths[1], "lungs", img_size=SIZE)
    assert k == kept and [tuple(r) for r in r1] == [tuple(r[0]) for r in rects] and [tuple(r) for r in r2] == [tuple(r[1]) for r in rects]
    cts = V.load_volume(paths[0], "cts", img_size=SIZE, rects=(r1, r2, k), box_indexing=box_indexing, new_dim=NEW_DIM)
    assert cts.is_cuda and cts.dtype.is_floating_point and tuple(cts.shape) == (len(plan), NEW_DIM, NEW_DIM, 1)          # the batch stays on the device


def test_build_dataset_feeds_the_holdout_runner(tmp_path):
    from covidseg_amd import runners, volume as V
    paths, _ = _patient(tmp_path)
    data = V.build_dataset([tuple(paths)], img_size=SIZE, new_dim=NEW_DIM)
    assert data[0].shape == data[1].shape and data[0].shape[1:] == (NEW_DIM, NEW_DIM, 1)
    runners.holdout_runner_unet_infection_segmentation(data=data, epochs=1, batch_size=4, verbose=0, workdir=str(tmp_path))


def test_segment_volume_end_to_end(tmp_path):
    from covidseg_amd import nifti_min, volume as V
    from covidseg_amd.keras_like import UNetModel
    from covidseg_amd.routed import ClusterRoutedModel
    paths, (ct, lung, inf) = _patient(tmp_path)
    model = UNetModel(NEW_DIM, 1, seed=1)
    model.verbose = 0
    out = tmp_path / "mask.nii.gz"
    t = float(np.median(model.predict(V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM))))          # an untrained model: a threshold inside its output range
    res = V.segment_volume(paths[0], model, lung_mask=paths[1], threshold=t, batch_size=8, out_path=out, img_size=SIZE)
    z0, z1 = VO.trim_range(Z)
    assert res.mask.shape == ct.shape and res.mask.dtype == np.uint8 and set(np.unique(res.mask)) <= {0, 1}
    assert not res.mask[:, :, :z0].any() and not res.mask[:, :, z1:].any() and res.mask.any()
    assert np.array_equal(res.counts, res.mask.sum(axis=(0, 1)))
    vox = np.prod(np.asarray([np.float32(0.8), np.float32(0.8), np.float32(5.0)], np.float64))
    assert res.total_ml == float(res.counts.sum()) * float(vox) / 1000.0 and np.array_equal(res.ml_per_slice, res.counts * float(vox) / 1000.0)
    assert res.fell_through == [2] and res.lung_ml > 0 and res.infected_share == res.total_ml / res.lung_ml
    back = nifti_min.read(out)
    assert np.array_equal(back.raw, res.mask) and back.pixdim == res.pixdim and back.header[252:328] == nifti_min.read(paths[0]).header[252:328]
    whole = V.segment_volume(paths[0], model, threshold=t, batch_size=8, img_size=SIZE)          # no lung mask: whole-frame boxes
    assert whole.fell_through == [] and whole.lung_ml is None and whole.mask.shape == ct.shape
    x = V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM)
    rm = ClusterRoutedModel(model, n_components=6).fit_router(x)
    routed = V.segment_volume(paths[0], rm, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    assert routed.mask.shape == ct.shape and not routed.mask[:, :, :z0].any() and not routed.mask[:, :, z1:].any()
    assert np.array_equal(routed.counts, routed.mask.sum(axis=(0, 1)))

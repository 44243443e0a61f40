"""-m gpu: connected components of a mask volume (csrc/kernels_components.hip, covidseg_amd.volume.label_volume / component_table / remove_small /
keep_largest / segment_volume(min_lesion_ml=...)) against tests/components_oracle.py and the scikit-image goldens.  Everything is an integer: every comparison
is np.array_equal, there is no tolerance anywhere."""
import os

import numpy as np
import pytest

import components_oracle as CO

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "component_goldens.npz")
E_ARG = -1


def _goldens():
    g = np.load(GOLD)
    for name in sorted({k.split("/")[0] for k in g.files}):
        shape = tuple(int(v) for v in g[name + "/shape"])
        size = int(np.prod(shape))
        mask = np.unpackbits(g[name + "/bits"])[:size].reshape(shape).astype(np.uint8)
        if name + "/values" in g.files:
            mask[mask != 0] = g[name + "/values"]
        removed = np.unpackbits(g[name + "/removed_bits"])[:size].reshape(shape).astype(np.uint8)
        yield name, mask, int(g[name + "/c"]), g[name + "/labels"], int(g[name + "/n"]), int(g[name + "/min_size"]), removed


def _label(mask, c, ops=None):
    """unet_vol_label through ctypes -> (labels [X, Y, Z] int32, n, the device labels)"""
    import torch
    from gpu_util import Ops
    ops = ops or Ops()
    X, Y, Z = mask.shape
    dev = torch.from_numpy(np.asfortranarray(mask.astype(np.uint8)).reshape(-1, order="F").copy()).cuda()
    labels = torch.full((max(mask.size, 1),), -7, dtype=torch.int32, device="cuda")
    n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(ops.lib.unet_vol_label_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ops.ck(ops.lib.unet_vol_label(ops.h, dev.data_ptr(), X, Y, Z, c, labels.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), ops.s), "vol_label")
    return labels[:mask.size].cpu().numpy().reshape(mask.shape, order="F"), int(n.item()), labels


def _stats(labels_dev, shape, n):
    from covidseg_amd import volume as V
    return V.component_stats_device(labels_dev, shape, n)


def _check_stats(got, labels, n):
    want = CO.stats(labels, n)
    assert len(got) == n
    for k in CO.STAT_FIELDS:
        assert np.array_equal(got[k].astype(np.int64), want[k]), k
    return want


def _check(mask, c, what=""):
    labels, n, dev = _label(mask, c)
    want, wn = CO.label(mask, c)
    assert n == wn, f"{what}: {n} components, the oracle finds {wn}"
    assert np.array_equal(labels, want), what
    return labels, n, dev


def test_every_golden_through_the_entry():
    count = 0
    for name, mask, c, want, wn, _, _ in _goldens():
        labels, n, _ = _label(mask, c)
        assert n == wn and labels.dtype == np.int32 and np.array_equal(labels, want), name
        count += 1
    assert count >= 12


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 1, 33), (63, 40, 6), (130, 70, 37), (257, 129, 65)])
def test_ragged_shapes_against_the_oracle(shape, c):
    for density in (0.05, 0.31, 0.6):
        labels, n, dev = _check(CO.random_mask(shape, density, 11 + c), c, f"{shape} c={c} density {density}")
        _check_stats(_stats(dev, shape, n), labels, n)
    if shape == (1, 1, 1):
        for v in (0, 1):
            labels, n, _ = _check(np.full(shape, v, np.uint8), c)
            assert n == v and labels[0, 0, 0] == v


def test_zero_sized_volume():
    for shape in ((0, 5, 7), (4, 0, 3), (6, 2, 0)):
        labels, n, _ = _label(np.zeros(shape, np.uint8), 1)
        assert n == 0 and labels.shape == shape


@pytest.mark.parametrize("c", [1, 2, 3])
def test_serpentine_and_spiral(c):
    for name, m in (("serpentine", CO.serpentine((128, 128, 64))), ("spiral", CO.spiral((128, 128, 64)))):
        labels, n, dev = _check(m, c, name)
        assert n == 1
        st = _stats(dev, m.shape, n)
        _check_stats(st, labels, n)
        assert int(st["voxels"][0]) == int(np.count_nonzero(m))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_components_that_touch_only_across_a_brick_boundary(axis):
    """at every multiple of 8 up to 64 along each axis (whatever the brick is, one of them is its boundary): two blobs that touch only across that plane --
    face to face (all c), edge to edge (c >= 2), corner to corner (c = 3); every pair sits in its own corner of the volume and touches nothing else"""
    shape = [24, 24, 24]
    shape[axis] = 80
    others = [a for a in range(3) if a != axis]
    for c in (1, 2, 3):
        for kind in ("face", "edge", "corner"):
            m = np.zeros(shape, np.uint8)
            for b in range(8, 65, 8):
                lo = [0, 0, 0]; hi = [0, 0, 0]
                lo[axis], hi[axis] = b - 1, b
                off = {"face": (0, 0), "edge": (1, 0), "corner": (1, 1)}[kind]
                base = 7 + 8 * ((b // 8) % 2)                         # the sideways step of an edge / corner contact crosses a multiple of 8 too
                lo[others[0]], lo[others[1]] = base, base
                hi[others[0]], hi[others[1]] = base + off[0], base + off[1]
                m[tuple(lo)] = 1; m[tuple(hi)] = 1
                lo2 = list(lo); lo2[axis] -= 1; m[tuple(lo2)] = 1     # blobs of two voxels along the axis, so the pair is not two singletons
                hi2 = list(hi); hi2[axis] += 1; m[tuple(hi2)] = 1
            labels, n, _ = _check(m, c, f"axis {axis} {kind} c={c}")
            joined = {"face": True, "edge": c >= 2, "corner": c >= 3}[kind]
            for b in range(8, 65, 8):
                lo = [0, 0, 0]; lo[axis] = b - 1
                base = 7 + 8 * ((b // 8) % 2)
                lo[others[0]], lo[others[1]] = base, base
                hi = list(lo); hi[axis] = b
                off = {"face": (0, 0), "edge": (1, 0), "corner": (1, 1)}[kind]
                hi[others[0]] += off[0]; hi[others[1]] += off[1]
                assert (labels[tuple(lo)] == labels[tuple(hi)]) == joined, f"axis {axis} plane {b} {kind} c={c}"


def test_foreground_is_every_non_zero_value():
    rng = np.random.default_rng(3)
    m = CO.random_mask((66, 30, 19), 0.31, 5) * rng.choice(np.array([1, 2, 255], np.uint8), (66, 30, 19))
    assert set(np.unique(m)) == {0, 1, 2, 255}
    for c in (1, 2, 3):
        _check(m.astype(np.uint8), c)


def test_statistics_giant_component_and_singletons():
    ones = np.ones((128, 64, 40), np.uint8)
    labels, n, dev = _check(ones, 1)
    st = _stats(dev, ones.shape, n)
    _check_stats(st, labels, n)
    assert n == 1 and int(st["voxels"][0]) == ones.size and (st["x1"][0], st["y1"][0], st["z1"][0]) == (127, 63, 39)
    cb = CO.checkerboard((48, 33, 21))
    labels, n, dev = _check(cb, 1)
    st = _stats(dev, cb.shape, n)
    _check_stats(st, labels, n)
    assert n == int(cb.sum()) and (st["voxels"] == 1).all() and int(st["voxels"].sum()) == int(np.count_nonzero(cb))
    from covidseg_amd import volume as V
    m = CO.ellipsoids((96, 80, 40), 12, 0.01, 2)
    labels, n = V.label_volume(m, 2)
    t = V.component_table(labels, n, (0.5, 0.5, 2.0))
    want = CO.stats(labels, n)
    assert np.array_equal(t["label"], np.arange(1, n + 1)) and np.array_equal(t["voxels"], want["voxels"]) and int(t["voxels"].sum()) == int(np.count_nonzero(m))
    assert np.array_equal(t["ml"], want["voxels"] * 0.5 / 1000.0)
    for k in "xyz":
        assert np.array_equal(t["c" + k], want["s" + k].astype(np.float64) / want["voxels"].astype(np.float64))
        assert np.array_equal(t[k + "0"], want[k + "0"]) and np.array_equal(t[k + "1"], want[k + "1"])


def test_remove_small_and_keep_largest():
    import torch
    from covidseg_amd import volume as V
    for name, mask, c, _, _, min_size, removed in _goldens():
        got = V.remove_small(mask, min_voxels=min_size, connectivity=c)
        assert got.dtype == np.uint8 and np.array_equal(got, removed), name
        assert np.array_equal(got, CO.remove_small(mask, min_size, c)), name
        for k in (0, 1, 2, 5):
            assert np.array_equal(V.keep_largest(mask, k, c), CO.keep_largest(mask, k, c)), (name, k)
    m = CO.ellipsoids((100, 64, 33), 10, 0.01, 4)                     # X * Y is a multiple of 16: the vector kernel; (99, 63, 33): the scalar one
    for mask in (m, m[:99, :63]):
        assert np.array_equal(V.remove_small(mask, min_ml=0.02, pixdim=(1.0, 1.0, 2.5)), CO.remove_small(mask, 8, 1))
        assert np.array_equal(V.remove_small(mask.astype(bool), min_voxels=8), CO.remove_small(mask, 8, 1))
        assert np.array_equal(V.keep_largest(np.ascontiguousarray(mask).astype(np.int16), 3, 2), CO.keep_largest(mask, 3, 2))
        labels, n = V.label_volume(mask, 1, return_device=True)
        keep = np.zeros(n + 1, bool); keep[1::2] = True
        shape = mask.shape
        out, counts = V.filter_components(labels, keep, n, shape, 5, 20)
        out = out.cpu().numpy().reshape(shape, order="F")
        host = labels.cpu().numpy().reshape(shape, order="F")
        assert np.array_equal(out, keep[host].astype(np.uint8))
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), [out[:, :, z].sum() for z in range(5, 20)])


def test_full_size_volume():
    """512 x 512 x 301: 300 random ellipsoids + 0.2 % salt noise; labels, n and the table equal the oracle's; two device runs are bit-identical"""
    import torch
    from covidseg_amd import volume as V
    shape = (512, 512, 301)
    m = CO.ellipsoids(shape, 300, 0.002, 5)
    dev, _ = V._mask_to_device(m)
    labels_dev, n = V.label_device(dev, shape, 1)
    st = V.component_stats_device(labels_dev, shape, n)
    labels2, n2 = V.label_device(dev, shape, 1)
    st2 = V.component_stats_device(labels2, shape, n2)
    assert n2 == n and torch.equal(labels_dev, labels2) and st.tobytes() == st2.tobytes()
    del labels2
    labels = labels_dev.cpu().numpy().reshape(shape, order="F")
    want, wn = CO.label(m, 1)
    print(f"full size: {n} components, {int(np.count_nonzero(m))} foreground voxels")
    assert n == wn and n > 100000
    assert np.array_equal(labels, want)
    _check_stats(st, want, wn)
    t = V.component_table(labels_dev, n, (0.7, 0.7, 1.25), shape=shape)
    ws = CO.stats(want, wn)
    assert np.array_equal(t["voxels"], ws["voxels"]) and np.array_equal(t["cx"], ws["sx"] / ws["voxels"]) and np.array_equal(t["z1"], ws["z1"])


def test_segment_volume_with_lesion_filter(tmp_path):
    from test_gpu_volume import NEW_DIM, SIZE, Z, _patient
    import volume_oracle as VO
    from covidseg_amd import nifti_min, volume as V
    from covidseg_amd.keras_like import UNetModel
    paths, (ct, lung, inf) = _patient(tmp_path)
    model = UNetModel(NEW_DIM, 1, seed=1)
    model.verbose = 0
    t = float(np.median(model.predict(V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM))))
    plain = V.segment_volume(paths[0], model, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    assert plain.lesions is None and plain.n_lesions is None and plain.removed_ml is None and "components" not in plain.seconds
    z0, z1 = VO.trim_range(Z)
    assert np.array_equal(plain.counts, plain.mask.sum(axis=(0, 1))) and not plain.mask[:, :, :z0].any() and not plain.mask[:, :, z1:].any()
    listed = V.segment_volume(paths[0], model, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE, lesions=True)
    assert np.array_equal(listed.mask, plain.mask) and np.array_equal(listed.counts, plain.counts) and listed.total_ml == plain.total_ml and listed.removed_ml is None
    wl, wn = CO.label(plain.mask, 1)
    assert listed.n_lesions == wn == len(listed.lesions) and "components" in listed.seconds
    c = 2
    sizes = np.sort(CO.stats(*CO.label(plain.mask, c))["voxels"])
    vox = float(np.prod(np.asarray(plain.pixdim, np.float64)))
    min_ml = (int(sizes[len(sizes) // 2]) + 0.5) * vox / 1000.0      # between two voxel counts: the median-sized component and everything smaller goes
    min_vox = CO.min_voxels_from_ml(min_ml, plain.pixdim)
    assert min_vox == V.min_voxels_from_ml(min_ml, plain.pixdim) == int(sizes[len(sizes) // 2]) + 1
    out = tmp_path / "filtered.nii.gz"
    res = V.segment_volume(paths[0], model, lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE, out_path=out, min_lesion_ml=min_ml, connectivity=c)
    want = CO.remove_small(plain.mask, min_vox, c)
    print(f"segment_volume filter: {int(plain.mask.sum())} -> {int(want.sum())} voxels, min {min_vox} voxels")
    assert want.sum() < plain.mask.sum(), "the filter removes something in this case"
    assert res.mask.dtype == np.uint8 and np.array_equal(res.mask, want)
    assert np.array_equal(nifti_min.read(out).raw, want)
    assert np.array_equal(res.counts, want.sum(axis=(0, 1)))
    assert res.total_ml == float(want.sum()) * vox / 1000.0 and np.array_equal(res.ml_per_slice, res.counts * vox / 1000.0)
    assert res.total_ml + res.removed_ml == plain.total_ml
    assert res.infected_share == res.total_ml / res.lung_ml
    fl, fn = CO.label(want, c)
    fs = CO.stats(fl, fn)
    assert res.n_lesions == fn and np.array_equal(res.lesions["label"], np.arange(1, fn + 1))
    for k in ("voxels", "x0", "x1", "y0", "y1", "z0", "z1"):
        assert np.array_equal(res.lesions[k], fs[k]), k
    for k in "xyz":
        assert np.array_equal(res.lesions["c" + k], fs["s" + k] / fs["voxels"])
    assert np.array_equal(res.lesions["ml"], fs["voxels"] * vox / 1000.0)


def test_bad_arguments_launch_nothing():
    import torch
    from gpu_util import Ops
    ops = Ops()
    X, Y, Z = 32, 16, 8
    mask = torch.ones(X * Y * Z, dtype=torch.uint8, device="cuda")
    labels = torch.full((X * Y * Z,), -7, dtype=torch.int32, device="cuda")
    n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    need = int(ops.lib.unet_vol_label_ws_bytes(X, Y, Z))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    call = lambda x, y, z, c, nbytes: ops.lib.unet_vol_label(ops.h, mask.data_ptr(), x, y, z, c, labels.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes, ops.s)
    assert call(X, Y, Z, 0, need) == E_ARG and call(X, Y, Z, 4, need) == E_ARG
    assert call(X, Y, Z, 1, need - 1) == E_ARG
    assert call(2048, 1024, 1024, 1, need) == E_ARG and call(65536, 32768, 1, 1, need) == E_ARG and call(-1, 4, 4, 1, need) == E_ARG          # by dimensions only
    assert ops.lib.unet_vol_label_ws_bytes(2048, 1024, 1024) == 0
    torch.cuda.synchronize()
    assert int(n.item()) == -7 and bool((labels == -7).all()), "a refused call wrote to its outputs"
    assert "connectivity" in ops.ctx.last_error() or "2^31" in ops.ctx.last_error() or "workspace" in ops.ctx.last_error()
    from covidseg_amd import volume as V
    with pytest.raises(ValueError):
        V.label_volume(np.ones((4, 4, 4), np.uint8), connectivity=4)
    assert call(X, Y, Z, 1, need) == 0
    torch.cuda.synchronize()
    assert int(n.item()) == 1 and bool((labels == 1).all())

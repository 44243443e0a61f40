"""-m gpu: binary morphology of a mask volume (csrc/kernels_morph.hip, unet_vol_label_planar; covidseg_amd.volume.binary_dilation ... binary_closing, dilate_mm ...
close_mm, fill_holes, label_volume(per_slice=True), postprocess, segment_volume(postprocess=...)) against tests/morph_oracle.py.

Every result is integer or boolean and is compared with np.array_equal / == only; two runs give the same bits."""
import numpy as np
import pytest

import components_oracle as CO
import morph_oracle as MO
from test_gpu_volscore import SHAPES, SPACINGS

pytestmark = pytest.mark.gpu

E_ARG = -1
OPS = {"dilate": 0, "erode": 1, "open": 2, "close": 3}
X_SHAPES = [(63, 9, 5), (64, 9, 5), (65, 9, 5), (127, 6, 4), (128, 6, 4), (129, 6, 4), (200, 7, 3)]


def _dev(a):
    import torch
    return torch.from_numpy(np.asfortranarray(np.asarray(a).astype(np.uint8)).reshape(-1, order="F").copy()).cuda()


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _morph(m, op, c=1, planar=False, it=1, b=0, ops=None):
    """unet_vol_morph through ctypes -> (uint8 [X, Y, Z], counts int64 [Z])"""
    import torch
    from gpu_util import Ops
    ops = ops or Ops()
    X, Y, Z = m.shape
    out = torch.full((max(m.size, 1),), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((max(Z, 1),), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(ops.lib.unet_vol_morph_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ops.ck(ops.lib.unet_vol_morph(ops.h, _dev(m * 5).data_ptr(), X, Y, Z, OPS[op], c, 1 if planar else 0, it, b, out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), ops.s),
           "vol_morph")
    return _host(out[:m.size], m.shape), counts[:Z].cpu().numpy()


def _fill(m, c=1, planar=False, ops=None):
    """unet_vol_fill_holes through ctypes"""
    import torch
    from gpu_util import Ops
    ops = ops or Ops()
    X, Y, Z = m.shape
    out = torch.full((max(m.size, 1),), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((max(Z, 1),), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(ops.lib.unet_vol_fill_holes_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ops.ck(ops.lib.unet_vol_fill_holes(ops.h, _dev(m * 255).data_ptr(), X, Y, Z, c, 1 if planar else 0, out.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), ops.s),
           "vol_fill_holes")
    return _host(out[:m.size], m.shape), counts[:Z].cpu().numpy()


def _label_planar(m, c, ops=None):
    import torch
    from gpu_util import Ops
    ops = ops or Ops()
    X, Y, Z = m.shape
    labels = torch.full((max(m.size, 4),), -7, dtype=torch.int32, device="cuda")
    n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(ops.lib.unet_vol_label_ws_bytes(X, Y, Z)), 16), dtype=torch.uint8, device="cuda")
    ops.ck(ops.lib.unet_vol_label_planar(ops.h, _dev(m).data_ptr(), X, Y, Z, c, labels.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), ops.s), "vol_label_planar")
    return _host(labels[:m.size], m.shape), int(n.item())


def _check_morph(m, op, c, planar, it, b, what=""):
    got, counts = _morph(m, op, c, planar, it, b)
    want = MO.OPS[op](m, c, it, b, planar)
    assert got.dtype == np.uint8 and np.array_equal(got, want), f"{what} {m.shape} {op} c={c} planar={planar} it={it} border={b}: {np.count_nonzero(got != want)} voxels differ"
    assert np.array_equal(counts, want.sum(axis=(0, 1), dtype=np.int64)), f"{what} {m.shape} {op}: counts"


def _combos():
    return [(op, c, planar, it, b) for op in OPS for c in (1, 2, 3) for planar in (False, True) for it in (1, 2, 3, 5) for b in (0, 1) if not (planar and c == 3)]


@pytest.mark.parametrize("shape", SHAPES + X_SHAPES)
def test_operators_against_the_oracle(shape):
    """small shapes: every op x connectivity x planar x iterations x border value; the large ones walk through the combinations with a stride that meets every value of
    every factor"""
    combos = _combos()
    if np.prod(shape) > 100000:
        combos = combos[(shape[0] % 7)::7] if np.prod(shape) < 1000000 else combos[::13]
        assert {c[0] for c in combos} == set(OPS) and {c[1] for c in combos} == {1, 2, 3} and {c[2] for c in combos} == {False, True} and {c[4] for c in combos} == {0, 1}
        assert {c[3] for c in combos} == {1, 2, 3, 5}
    for i, (op, c, planar, it, b) in enumerate(combos):
        m = CO.random_mask(shape, (0.02, 0.3, 0.85)[i % 3], 40 + i % 5)
        _check_morph(m, op, c, planar, it, b)


def test_contacts_across_a_word_boundary():
    """two voxels that meet only across x = 63 | 64 (and 127 | 128): straight and diagonal neighbours; a dilation must join them, an erosion of the complement too"""
    for X in (65, 129, 200):
        shape = (X, 5, 4)
        for xb in (64, 128):
            if xb >= X:
                continue
            for dy, dz in ((0, 0), (1, 0), (0, 1), (1, 1)):
                m = np.zeros(shape, np.uint8)
                m[xb - 1, 2, 1] = 1; m[xb, 2 + dy, 1 + dz] = 1
                for c in (1, 2, 3):
                    for planar in ((False, True) if c < 3 else (False,)):
                        for b in (0, 1):
                            _check_morph(m, "dilate", c, planar, 1, b, "word boundary")
                            _check_morph(1 - m, "erode", c, planar, 1, b, "word boundary")
                            _check_morph(m, "close", c, planar, 2, b, "word boundary")
    row = np.zeros((200, 1, 1), np.uint8); row[63] = 1                # the carry into the next word, and back
    got, _ = _morph(row, "dilate", 1, False, 3, 0)
    assert np.array_equal(np.nonzero(got[:, 0, 0])[0], np.arange(60, 67))


def test_corner_voxels_with_both_border_values():
    for shape in ((63, 40, 6), (130, 70, 37), (64, 8, 8)):
        X, Y, Z = shape
        for cx in (0, X - 1):
            for cy in (0, Y - 1):
                for cz in (0, Z - 1):
                    m = np.zeros(shape, np.uint8); m[cx, cy, cz] = 1
                    for b in (0, 1):
                        for c in (1, 3):
                            _check_morph(m, "dilate", c, False, 2, b, "corner")
                            _check_morph(1 - m, "erode", c, False, 2, b, "corner")
                        _check_morph(m, "close", 2, True, 1, b, "corner")
                        _check_morph(1 - m, "open", 1, True, 2, b, "corner")


def test_empty_and_full_volumes():
    for shape in ((65, 9, 5), (128, 16, 9)):
        for m in (np.zeros(shape, np.uint8), np.ones(shape, np.uint8)):
            for op in OPS:
                for b in (0, 1):
                    _check_morph(m, op, 1, False, 2, b, "empty / full")
                    _check_morph(m, op, 2, True, 3, b, "empty / full")
            for planar in (False, True):
                got, counts = _fill(m, 1, planar)
                assert np.array_equal(got, m) and np.array_equal(counts, m.sum(axis=(0, 1), dtype=np.int64))
    assert _morph(np.ones((65, 9, 5), np.uint8), "erode", 3, False, 4, 1)[0].all()
    assert not _morph(np.ones((9, 9, 9), np.uint8), "erode", 1, False, 5, 0)[0].any()


@pytest.mark.parametrize("shape", SHAPES[:4] + X_SHAPES[2::2])
def test_planar_labels_against_the_oracle(shape):
    from covidseg_amd import volume as V
    for c in (1, 2):
        for i, density in enumerate((0.05, 0.45, 0.8)):
            m = CO.random_mask(shape, density, 60 + i)
            got, n = _label_planar(m, c)
            want, wn = MO.label_planar(m, c)
            assert n == wn and np.array_equal(got, want), (shape, c, density)
            lab, n2 = V.label_volume(m * 7, c, per_slice=True)
            assert n2 == wn and lab.dtype == np.int32 and np.array_equal(lab, want)
    full = np.ones(shape, np.uint8)
    lab, n = V.label_volume(full, 1, per_slice=True)
    assert n == shape[2] and np.array_equal(lab, np.broadcast_to(np.arange(1, shape[2] + 1, dtype=np.int32), shape))          # one component per slice, numbered by z


def test_planar_labels_across_brick_faces():
    """bricks are 64 x 8 x 8: contacts that exist only across x = 63 | 64 and y = 7 | 8 join inside a slice (diagonal ones only at connectivity 2); nothing joins across
    z = 7 | 8, nor across any other pair of slices"""
    shape = (130, 20, 18)
    m = np.zeros(shape, np.uint8)
    m[60:64, 3, 2] = 1; m[64:70, 3, 2] = 1                            # straight across x
    m[63, 10, 4] = 1; m[64, 11, 4] = 1                               # diagonal across x (and y stays inside a brick)
    m[20, 4:8, 6] = 1; m[20, 8:12, 6] = 1                            # straight across y
    m[30, 7, 9] = 1; m[31, 8, 9] = 1                                 # diagonal across y
    m[100, 15, 6:10] = 1                                             # a column along z through z = 7 | 8: four components
    m[90:128, 17, :] = 1                                             # a wall through every slice and across x = 127 | 128... one component per slice
    for c in (1, 2):
        got, n = _label_planar(m, c)
        want, wn = MO.label_planar(m, c)
        assert n == wn and np.array_equal(got, want), c
        assert got[60, 3, 2] == got[69, 3, 2] and got[20, 4, 6] == got[20, 11, 6]
        assert (got[63, 10, 4] == got[64, 11, 4]) == (c == 2) and (got[30, 7, 9] == got[31, 8, 9]) == (c == 2)
        assert len({int(v) for v in got[100, 15, 6:10]}) == 4 and len({int(v) for v in got[95, 17, :]}) == shape[2]
    m3, n3 = CO.label(m, 1)
    assert n3 < MO.label_planar(m, 1)[1]                              # the 3-D labelling joins what the planar one keeps apart


@pytest.mark.parametrize("shape", SHAPES[1:] + X_SHAPES[::3])
def test_fill_holes_against_the_oracle(shape):
    from covidseg_amd import volume as V
    big = np.prod(shape) > 1000000
    for i, density in enumerate((0.6,) if big else (0.3, 0.6, 0.8)):
        m = CO.random_mask(shape, density, 70 + i)
        if min(shape) > 12:
            m |= MO.hollow_shell(shape, (2, 3, 1), (shape[0] - 3, shape[1] - 2, shape[2] - 2))          # a large cavity full of noise
        for c, planar in ((1, False), (2, False), (3, False), (1, True), (2, True)):
            if big and (c, planar) not in ((1, False), (2, True)):
                continue
            got, counts = _fill(m, c, planar)
            want = MO.fill_holes(m, c, planar)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, density, c, planar, int(np.count_nonzero(got != want)))
            assert np.array_equal(counts, want.sum(axis=(0, 1), dtype=np.int64))
            if i == 1 or big:
                assert np.array_equal(V.fill_holes(m.astype(bool), c, per_slice=planar), want)


def test_shell_and_tube():
    """(the reasoning is in tests/test_morph_host.py::test_shell_and_tube: per-slice filling never fills less than 3-D filling)  A closed shell is filled both ways; a
    shell with an opening in one slice is filled nowhere in 3-D and per slice everywhere but in the slice that is cut open; a tube open at one z end is filled per slice,
    not in 3-D."""
    from covidseg_amd import volume as V
    shape = (70, 20, 12)
    shell = MO.hollow_shell(shape, (3, 4, 2), (66, 14, 8))
    full = shell.copy(); full[3:67, 4:15, 2:9] = 1
    cut = shell.copy(); cut[66, 9, 5] = 0
    tube = MO.open_tube(shape, (3, 4, 0), (66, 14, 8))
    tube_filled = tube.copy(); tube_filled[3:67, 4:15, 0:9] = 1
    cut_per = full.copy(); cut_per[:, :, 5] = cut[:, :, 5]
    for m, want3, want2 in ((shell, full, full), (cut, cut, cut_per), (tube, tube, tube_filled)):
        assert np.array_equal(MO.fill_holes(m), want3) and np.array_equal(MO.fill_holes(m, planar=True), want2)
        assert np.array_equal(_fill(m, 1, False)[0], want3) and np.array_equal(_fill(m, 1, True)[0], want2)
        assert np.array_equal(V.fill_holes(m), want3) and np.array_equal(V.fill_holes(m, per_slice=True), want2)
    assert cut_per.sum() > cut.sum() and tube_filled.sum() > tube.sum() and full.sum() > shell.sum()


def test_ball_operators():
    import torch
    from gpu_util import Ops
    from covidseg_amd import volume as V
    ops = Ops()
    for shape, count in (((130, 70, 37), 12), ((63, 40, 6), 3), ((17, 1, 33), 2)):
        m = CO.ellipsoids(shape, count, 0.002, 3)
        for pixdim, r in ((SPACINGS[0], 2.0), (SPACINGS[1], 1.5), (SPACINGS[3], 1.1), (SPACINGS[2], 0.68359375)):
            for name, fn in (("dilate_mm", MO.dilate_mm), ("erode_mm", MO.erode_mm), ("open_mm", MO.open_mm), ("close_mm", MO.close_mm)):
                got = getattr(V, name)(m, r, pixdim)
                assert got.dtype == np.uint8 and np.array_equal(got, fn(m, r, pixdim)), (shape, pixdim, r, name)
        X, Y, Z = shape
        for keep_le, want in ((1, MO.dilate_mm(m, 2.0, SPACINGS[1])), (0, MO.erode_mm(m, 2.0, SPACINGS[1]))):          # the entry itself, with counts
            d2 = V.edt_sq_device(_dev(m), shape, SPACINGS[1], features_nonzero=bool(keep_le))
            out = torch.full((m.size,), 9, dtype=torch.uint8, device="cuda"); counts = torch.full((Z,), -7, dtype=torch.int64, device="cuda")
            ops.ck(ops.lib.unet_vol_ball(ops.h, d2.data_ptr(), X, Y, Z, 4.0, keep_le, out.data_ptr(), counts.data_ptr(), ops.s), "vol_ball")
            assert np.array_equal(_host(out, shape), want) and np.array_equal(counts.cpu().numpy(), want.sum(axis=(0, 1), dtype=np.int64))
    assert V.erode_mm(np.ones((9, 8, 7), np.uint8), 3.0).all() and not V.dilate_mm(np.zeros((9, 8, 7), np.uint8), 3.0).any()          # the outside: foreground / background
    try:
        import scipy.ndimage as ndi
    except ImportError:
        print("ball: scipy does not import here; the footprint comparison did not run")
        return
    m = CO.ellipsoids((130, 70, 37), 12, 0.001, 3)
    assert np.array_equal(V.dilate_mm(m, 2.0), ndi.binary_dilation(m, structure=MO.ball_footprint(2.0)))


def test_public_forms_and_postprocess():
    from covidseg_amd import volume as V
    shape = (129, 40, 17)
    m = CO.ellipsoids(shape, 14, 0.01, 8)
    dev = _dev(m)
    for name, op in (("binary_dilation", "dilate"), ("binary_erosion", "erode"), ("binary_opening", "open"), ("binary_closing", "close")):
        fn = getattr(V, name)
        assert np.array_equal(fn(m * 3, 2, 2, 1), MO.OPS[op](m, 2, 2, 1))
        assert np.array_equal(fn(m.astype(bool), connectivity=1, iterations=3, per_slice=True), MO.OPS[op](m, 1, 3, 0, True))
        out = fn(dev, 3, 1, 0, return_device=True, shape=shape)
        assert out.dtype.is_floating_point is False and np.array_equal(_host(out, shape), MO.OPS[op](m, 3, 1, 0))
    pixdim = SPACINGS[1]
    steps = [("close", {"iterations": 2}), ("fill_holes", {}), ("open_mm", {"radius_mm": 1.0}), ("remove_small", {"min_voxels": 30, "connectivity": 2}), ("keep_largest", {"k": 5})]
    want = MO.closing(m, 1, 2)
    want = MO.fill_holes(want)
    want = MO.open_mm(want, 1.0, pixdim)
    want = CO.remove_small(want, 30, 2)
    want = CO.keep_largest(want, 5, 1)
    got = V.postprocess(m, steps, pixdim=pixdim)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and 0 < want.sum() != m.sum()
    got_dev, counts = V.postprocess_device(dev, shape, steps, pixdim)
    assert np.array_equal(_host(got_dev, shape), want) and np.array_equal(counts.cpu().numpy(), want.sum(axis=(0, 1), dtype=np.int64))
    assert np.array_equal(V.postprocess(m, [], pixdim=pixdim), m) and np.array_equal(V.postprocess(m, ["fill_holes"]), MO.fill_holes(m))


def test_full_size_volume_against_scipy():
    """512 x 512 x 301 (the volume of test_gpu_components: 300 random ellipsoids + 0.2 % salt noise), closed twice and hole-filled: equal to scipy's result, the per-slice
    counts equal the sums, and a second run gives the same bits; then the hollowed ellipsoids, whose cavities the filling must find"""
    import torch
    ndi = pytest.importorskip("scipy.ndimage")
    from covidseg_amd import volume as V
    shape = (512, 512, 301)
    m = CO.ellipsoids(shape, 300, 0.002, 5)
    dev, _ = V._mask_to_device(m)
    closed, c1 = V.morph_device(dev, shape, "close", 1, 2, 0)
    filled, c2 = V.fill_holes_device(closed, shape, 1)
    closed_b, c1b = V.morph_device(dev, shape, "close", 1, 2, 0)
    filled_b, c2b = V.fill_holes_device(closed_b, shape, 1)
    assert torch.equal(closed, closed_b) and torch.equal(filled, filled_b) and torch.equal(c1, c1b) and torch.equal(c2, c2b), "two runs give the same bits"
    del closed_b, filled_b
    want_closed = ndi.binary_closing(m, iterations=2)
    got = _host(closed, shape)
    assert np.array_equal(got, want_closed), f"closing: {np.count_nonzero(got != want_closed)} voxels differ"
    assert np.array_equal(c1.cpu().numpy(), want_closed.sum(axis=(0, 1), dtype=np.int64))
    want = ndi.binary_fill_holes(want_closed)
    got = _host(filled, shape)
    print(f"full size: {int(m.sum())} voxels, closed {int(want_closed.sum())}, filled {int(want.sum())}")
    assert np.array_equal(got, want), f"fill_holes: {np.count_nonzero(got != want)} voxels differ"
    assert np.array_equal(c2.cpu().numpy(), want.sum(axis=(0, 1), dtype=np.int64))
    assert np.array_equal(V.postprocess(dev, [("close", {"iterations": 2}), ("fill_holes", {})], return_device=True, shape=shape).cpu().numpy(), filled.cpu().numpy())
    # With border_value 0 the closing's erosions eat into whatever lies within two voxels of a face, so the closed mask may hold FEWER voxels than the input, and solid
    # ellipsoids have no cavity to fill.  A second full-size case with cavities: the same ellipsoids hollowed out (the mask without its erosion by three steps).
    del closed, filled, got, want, want_closed
    solid = CO.ellipsoids(shape, 300, 0, 5)
    hollow = solid & ~ndi.binary_erosion(solid, iterations=3)
    hdev, _ = V._mask_to_device(hollow)
    eroded, _ = V.morph_device(_dev(solid), shape, "erode", 1, 3, 0)
    assert np.array_equal(_host(eroded, shape) == 0, ~ndi.binary_erosion(solid, iterations=3))
    refilled, c3 = V.fill_holes_device(hdev, shape, 1)
    want = ndi.binary_fill_holes(hollow)
    got = _host(refilled, shape)
    print(f"full size, hollowed: {int(hollow.sum())} voxels, filled {int(want.sum())}")
    assert want.sum() > hollow.sum(), "the hollowed ellipsoids have cavities"
    assert np.array_equal(got, want), f"fill_holes of the hollowed volume: {np.count_nonzero(got != want)} voxels differ"
    assert np.array_equal(c3.cpu().numpy(), want.sum(axis=(0, 1), dtype=np.int64))


def test_segment_volume_with_postprocess(tmp_path):
    from test_gpu_volume import NEW_DIM, SIZE, _patient
    from covidseg_amd import volume as V
    from covidseg_amd.keras_like import UNetModel
    paths, (ct, lung, inf) = _patient(tmp_path)
    model = UNetModel(NEW_DIM, 1, seed=1)
    model.verbose = 0
    t = float(np.median(model.predict(V.load_volume(paths[0], "cts", img_size=SIZE, new_dim=NEW_DIM))))
    kw = dict(lung_mask=paths[1], threshold=t, batch_size=8, img_size=SIZE)
    plain = V.segment_volume(paths[0], model, **kw)
    assert plain.postprocess_ml is None and "postprocess" not in plain.seconds
    steps = [("close", {"iterations": 2, "connectivity": 2}), ("fill_holes", {"connectivity": 1})]
    cleaned = MO.fill_holes(MO.closing(plain.mask, 2, 2), 1)
    assert not np.array_equal(cleaned, plain.mask), "the steps change something in this case"
    vox = float(np.prod(np.asarray(plain.pixdim, np.float64)))
    res = V.segment_volume(paths[0], model, postprocess=steps, lesions=True, **kw)
    assert res.mask.dtype == np.uint8 and np.array_equal(res.mask, cleaned) and "postprocess" in res.seconds
    assert np.array_equal(res.counts, cleaned.sum(axis=(0, 1), dtype=np.int64)) and res.total_ml == float(cleaned.sum()) * vox / 1000.0
    assert np.array_equal(res.ml_per_slice, res.counts * vox / 1000.0) and res.infected_share == res.total_ml / res.lung_ml
    assert res.postprocess_ml == float(int(cleaned.sum()) - int(plain.mask.sum())) * vox / 1000.0
    lab, n = V.label_volume(cleaned, 1)
    tab = V.component_table(lab, n, res.pixdim)
    assert res.n_lesions == n and all(np.array_equal(res.lesions[k], tab[k]) for k in tab.dtype.names)
    c = 2
    sizes = np.sort(CO.stats(*CO.label(cleaned, c))["voxels"])
    min_ml = (int(sizes[len(sizes) // 2]) + 0.5) * vox / 1000.0
    f = V.segment_volume(paths[0], model, postprocess=steps, min_lesion_ml=min_ml, connectivity=c, truth=paths[2], **kw)
    want = CO.remove_small(cleaned, CO.min_voxels_from_ml(min_ml, plain.pixdim), c)
    assert want.sum() < cleaned.sum(), "the filter removes something in this case"
    assert np.array_equal(f.mask, want) and np.array_equal(f.counts, want.sum(axis=(0, 1), dtype=np.int64))
    assert f.postprocess_ml == res.postprocess_ml and f.removed_ml == float(cleaned.sum()) * vox / 1000.0 - float(want.sum()) * vox / 1000.0
    lab, n = V.label_volume(want, c)
    tab = V.component_table(lab, n, f.pixdim)
    assert f.n_lesions == n and all(np.array_equal(f.lesions[k], tab[k]) for k in tab.dtype.names)
    assert f.score == V.score_volume(want, inf, f.pixdim, lesion_connectivity=c)
    with pytest.raises(ValueError):
        V.segment_volume(paths[0], model, postprocess=[("close", {"iterations": 0})], **kw)


def test_refused_arguments_launch_nothing():
    import torch
    from gpu_util import Ops
    ops = Ops()
    X, Y, Z = 32, 16, 8
    N = X * Y * Z
    mask = torch.ones(N, dtype=torch.uint8, device="cuda")
    out = torch.full((N,), 9, dtype=torch.uint8, device="cuda")
    counts = torch.full((Z,), -7, dtype=torch.int64, device="cuda")
    labels = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    n = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.zeros(N, dtype=torch.float64, device="cuda")
    need_m, need_f, need_l = (int(f(X, Y, Z)) for f in (ops.lib.unet_vol_morph_ws_bytes, ops.lib.unet_vol_fill_holes_ws_bytes, ops.lib.unet_vol_label_ws_bytes))
    assert need_m >= 2 * N // 8 and need_f >= 6 * N
    ws = torch.empty(max(need_m, need_f, need_l), dtype=torch.uint8, device="cuda")

    def morph(x=X, y=Y, z=Z, op=0, c=1, planar=0, it=1, b=0, o=out, nbytes=need_m):
        return ops.lib.unet_vol_morph(ops.h, mask.data_ptr(), x, y, z, op, c, planar, it, b, o.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, ops.s)

    def fill(x=X, y=Y, z=Z, c=1, planar=0, o=out, nbytes=need_f):
        return ops.lib.unet_vol_fill_holes(ops.h, mask.data_ptr(), x, y, z, c, planar, o.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, ops.s)

    def planar_label(x=X, y=Y, z=Z, c=1, nbytes=need_l):
        return ops.lib.unet_vol_label_planar(ops.h, mask.data_ptr(), x, y, z, c, labels.data_ptr(), n.data_ptr(), ws.data_ptr(), nbytes, ops.s)

    def ball(x=X, y=Y, z=Z, r2=1.0, o=out):
        return ops.lib.unet_vol_ball(ops.h, d2.data_ptr(), x, y, z, r2, 1, o.data_ptr(), counts.data_ptr(), ops.s)

    assert morph(op=-1) == E_ARG and morph(op=4) == E_ARG and "op" in ops.ctx.last_error()
    assert morph(c=0) == E_ARG and morph(c=4) == E_ARG and morph(c=3, planar=1) == E_ARG
    assert morph(it=0) == E_ARG and morph(it=-3) == E_ARG and morph(it=65) == E_ARG and "iterations" in ops.ctx.last_error()
    assert morph(b=2) == E_ARG and morph(b=-1) == E_ARG
    assert morph(2048, 1024, 1024) == E_ARG and morph(65536, 32768, 1) == E_ARG and morph(x=-1) == E_ARG and "2^31" in ops.ctx.last_error()
    assert morph(o=mask) == E_ARG and morph(nbytes=need_m - 1) == E_ARG
    assert fill(c=0) == E_ARG and fill(c=4) == E_ARG and fill(c=3, planar=1) == E_ARG
    assert fill(2048, 1024, 1024) == E_ARG and fill(y=-2) == E_ARG and fill(o=mask) == E_ARG and fill(nbytes=need_f - 1) == E_ARG
    assert planar_label(c=0) == E_ARG and planar_label(c=3) == E_ARG and planar_label(2048, 1024, 1024) == E_ARG and planar_label(nbytes=need_l - 1) == E_ARG
    assert ball(2048, 1024, 1024) == E_ARG and ball(r2=-1.0) == E_ARG and ball(r2=float("nan")) == E_ARG and ball(r2=float("inf")) == E_ARG and ball(z=-1) == E_ARG
    assert ops.lib.unet_vol_morph_ws_bytes(2048, 1024, 1024) == 0 and ops.lib.unet_vol_fill_holes_ws_bytes(2048, 1024, 1024) == 0
    for shape in ((0, 5, 7), (4, 0, 3), (6, 2, 0)):                   # a zero dimension: accepted, touches nothing
        assert morph(*shape) == 0 and fill(*shape) == 0 and ball(*shape) == 0
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((counts == -7).all()) and bool((labels == -7).all()) and int(n.item()) == -7 and bool((mask == 1).all()), "a refused call wrote"
    assert morph(op=1, c=3, it=2, b=0) == 0                          # the same buffers through the accepted calls
    torch.cuda.synchronize()
    want = MO.erosion(np.ones((X, Y, Z), np.uint8), 3, 2, 0)
    assert np.array_equal(_host(out, (X, Y, Z)), want) and np.array_equal(counts.cpu().numpy(), want.sum(axis=(0, 1), dtype=np.int64))
    assert fill() == 0 and planar_label(c=2) == 0 and ball(r2=0.0) == 0
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and int(n.item()) == Z and bool((counts == X * Y).all())

"""CPU: tests/skeleton_oracle.py pinned to the slow per-voxel form (scipy.ndimage.label on every 3 x 3 x 3), the phantom figures of DESIGN.md section 4ag, topology on
random blobs, csrc/kernels_skeleton.hip's own predicate and per-word functions run on the CPU (tools/skeleton_host_check.hip), and the host half of skeleton.py -- graph,
pruning, rooting -- on hand-drawn skeletons with known answers."""
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import skeleton_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graph(vol, pixdim=(1.0, 1.0, 1.0), radius_of=None, affine=None):
    """graph_from_table over the oracle's table; radius_of: the mask whose Euclidean distance transform gives the radii"""
    from covidseg_amd import skeleton as SK
    idx, codes, _ = SO.table(vol)
    radius = None
    if radius_of is not None:
        radius = ndimage.distance_transform_edt(radius_of != 0, sampling=pixdim).reshape(-1, order="F")[idx]
    return SK.graph_from_table(SK._finish_table(idx, codes, vol.shape, radius), vol.shape, pixdim, affine)


@pytest.fixture(scope="module")
def thinned():
    out = {}
    for name, make in (("tube", SO.three_armed_tube), ("torus", SO.torus), ("ball", SO.ball)):
        vol = make()
        out[name] = (vol, SO.thin(vol, True))
    out["ball0"] = (out["ball"][0], SO.thin(out["ball"][0], False))
    return out


# ---- pinning the oracle ---------------------------------------------------------------------------------------------------------------------------------
def test_the_predicate_equals_the_slow_form():
    rng = np.random.default_rng(26)
    codes = [rng.integers(0, 1 << 26, 7000, dtype=np.int64)]                                          # half full
    codes.append(codes[0][:6000] & rng.integers(0, 1 << 26, 6000, dtype=np.int64))                      # a quarter
    codes.append(codes[0][:6000] | rng.integers(0, 1 << 26, 6000, dtype=np.int64))                      # three quarters
    codes.append(codes[1][:2000] & rng.integers(0, 1 << 26, 2000, dtype=np.int64))                      # an eighth
    few = [0] + [1 << a for a in range(26)] + [(1 << a) | (1 << b) for a in range(26) for b in range(a)]
    few += [(1 << a) | (1 << b) | (1 << c) for a in range(26) for b in range(a) for c in range(b)]      # every neighbourhood with at most 3 set voxels
    codes = np.concatenate(codes + [np.asarray(few, np.int64)]).astype(np.uint32)
    assert codes.size >= 20000 + 2952
    got = SO.simple(codes)
    want = np.array([SO.simple_slow(SO.cube_of(c)) for c in codes])
    assert np.array_equal(got, want)
    assert 0.05 < got.mean() < 0.95
    assert not SO.simple(np.uint32(0)) and not SO.simple(np.uint32((1 << 26) - 1))                      # isolated; interior


def test_the_thinning_equals_the_slow_form():
    for shape, seed, endpoints, limit in (((18, 14, 12), 3, True, None), ((9, 16, 12), 4, False, None), ((13, 12, 1), 5, True, None), ((12, 10, 10), 6, True, 1)):
        vol = SO.blobs(shape, seed, 0.4)
        assert shape[2] == 1 or int(vol.sum()) >= 400
        a, b = SO.thin(vol, endpoints, limit), SO.thin_slow(vol, endpoints, limit)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]), (shape, seed)
        assert a[2][0] > 0


# ---- the phantoms ---------------------------------------------------------------------------------------------------------------------------------------
def test_three_armed_tube(thinned):
    vol, (skel, iterations, removed) = thinned["tube"]
    assert int(vol.sum()) == 1628 and iterations == 3 and int(skel.sum()) == 51 and int(removed.sum()) == 1628 - 51 and removed[-1] == 0
    assert ndimage.label(skel, np.ones((3, 3, 3)))[1] == 1
    deg = SO.degrees(skel)
    assert (int((deg == 1).sum()), int((deg == 2).sum()), int((deg >= 3).sum())) == (3, 47, 1)


def test_torus(thinned):
    _, (skel, _, _) = thinned["torus"]
    deg = SO.degrees(skel)
    assert int(skel.sum()) == 56 and (deg == 2).all() and ndimage.label(skel, np.ones((3, 3, 3)))[1] == 1


def test_ball(thinned):
    assert int(thinned["ball0"][1][0].sum()) == 1
    assert int(thinned["ball"][1][0].sum()) == 2


def test_topology_on_random_blobs():
    s26, s6 = np.ones((3, 3, 3)), ndimage.generate_binary_structure(3, 1)
    for seed, shape in enumerate(((24, 20, 16), (31, 9, 14), (18, 18, 18), (40, 12, 1))):
        vol = SO.blobs(shape, 100 + seed, 0.35)
        for endpoints in (True, False):
            skel = SO.thin(vol, endpoints)[0]
            assert not (skel & ~vol).any() and int(skel.sum()) < int(vol.sum())
            lab, n = ndimage.label(vol, s26)
            assert ndimage.label(skel, s26)[1] == n
            assert sorted(set(lab[skel != 0].tolist())) == list(range(1, n + 1))                       # every component of the input survives
            pad = lambda a: np.pad(a, 1)                                                                # outside the volume is background: one component with the rim
            assert ndimage.label(pad(skel) == 0, s6)[1] == ndimage.label(pad(vol) == 0, s6)[1]


# ---- the kernel file's own functions on the CPU ----------------------------------------------------------------------------------------------------------
def test_the_kernels_predicate_and_words_on_the_cpu_equal_the_oracle(tmp_path, thinned):
    csrc = os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc")
    exe = str(tmp_path / "skeleton_host_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", csrc,
                    os.path.join(ROOT, "tools", "skeleton_host_check.hip"), "-o", exe], check=True, cwd=str(tmp_path))
    assert int(subprocess.run([exe, "count"], check=True, capture_output=True, text=True).stdout) == SO.SIMPLE_COUNT == 25985144
    cases = [(thinned[k][0], e, -1, thinned[k][1]) for k, e in (("tube", True), ("torus", True), ("ball", True), ("ball0", False))]
    rnd = SO.blobs((130, 11, 9), 7, 0.35)
    rnd[:, 0, :] |= rnd[:, 1, :]                                     # voxels on faces of the volume
    rnd[0, :, :] = rnd[1, :, :]; rnd[129, :, :] = rnd[128, :, :]
    cases += [(rnd, True, -1, SO.thin(rnd, True)), (rnd, False, -1, SO.thin(rnd, False)), (rnd, True, 1, SO.thin(rnd, True, 1))]
    for vol, endpoints, limit, (want, iterations, removed) in cases:
        vol.reshape(-1, order="F").tofile(tmp_path / "in.bin")
        out = subprocess.run([exe, "thin", *(str(n) for n in vol.shape), str(tmp_path / "in.bin"), "1" if endpoints else "0", str(limit), str(tmp_path / "out.bin")],
                             check=True, capture_output=True, text=True).stdout.split("\n")
        got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(vol.shape, order="F")
        assert np.array_equal(got, want), (vol.shape, endpoints, limit)
        assert out[0] == f"iterations {iterations}" and out[1].split()[1:] == [str(int(v)) for v in removed]


# ---- graph, pruning, rooting --------------------------------------------------------------------------------------------------------------------------------
def test_a_diagonal_line_has_its_length():
    from covidseg_amd import skeleton as SK
    vol = np.zeros((12, 12, 12), np.uint8)
    for i in range(2, 10):
        vol[i, i, i] = 1
    g = _graph(vol, (1.0, 2.0, 3.0))
    assert len(g.nodes) == 2 and list(g.nodes["kind"]) == ["end", "end"] and len(g.branches) == 1
    br = g.branches[0]
    assert len(br.path) == 8 and br.length_mm == pytest.approx(7 * np.sqrt(14.0), rel=1e-14) and br.chord_mm == pytest.approx(br.length_mm, rel=1e-14)
    assert br.tortuosity == pytest.approx(1.0, rel=1e-14) and np.isnan(br.radius_mean)
    assert g.components["cycles"].tolist() == [0] and np.isnan(g.nodes["wx"]).all()
    with pytest.raises(ValueError, match="not guessed"):
        SK.root_tree(g, "superior")                                  # no orientation: refused
    assert SK.root_tree(g, "superior", orientation="LPS").roots.tolist() == [1]
    assert SK.root_tree(g, "superior", orientation="LPI").roots.tolist() == [0]
    with pytest.raises(ValueError, match="radii"):
        SK.root_tree(g, "thickest")
    A = np.diag([1.0, 2.0, 3.0, 1.0]); A[:3, 3] = (10.0, 20.0, 30.0)
    gw = _graph(vol, (1.0, 2.0, 3.0), affine=A)
    assert (gw.nodes["wx"][0], gw.nodes["wy"][0], gw.nodes["wz"][0]) == (12.0, 24.0, 36.0)
    assert SK.root_tree(gw, (9, 9, 9)).roots.tolist() == [1] and SK.root_tree(gw, (12.5, 24.0, 36.0)).roots.tolist() == [0]


def test_three_armed_tube_graph(thinned):
    from covidseg_amd import skeleton as SK
    vol, (skel, _, _) = thinned["tube"]
    g = _graph(skel, radius_of=vol)
    assert sorted(g.nodes["kind"].tolist()) == ["end", "end", "end", "junction"] and len(g.branches) == 3 and g.components["cycles"].tolist() == [0]
    assert sum(len(b.path) for b in g.branches) == 51 + 2            # the junction voxel ends all three
    t = SK.root_tree(g, "thickest")
    trunk = int(np.flatnonzero(t.generation == 0)[0])
    assert sorted(t.generation.tolist()) == [0, 1, 1] and not t.closes_cycle.any() and sorted(t.children[trunk]) == sorted(set(range(3)) - {trunk})
    assert g.branches[trunk].radius_mean > 3.0 > max(g.branches[b].radius_mean for b in t.children[trunk])
    assert abs(g.branches[trunk].length_mm - 18.0) <= 2.0            # (20, 18, 4) .. (20, 18, 22), less what the end keeps off the cap
    p = SK.prune(g, 3.0, 1.5)
    assert len(p.branches) == 3 and len(p.nodes) == 4               # nothing to prune


def test_torus_graph(thinned):
    from covidseg_amd import skeleton as SK
    _, (skel, _, _) = thinned["torus"]
    g = _graph(skel)
    assert len(g.nodes) == 1 and g.nodes["kind"][0] == "loop" and len(g.branches) == 1 and g.components["cycles"].tolist() == [1]
    br = g.branches[0]
    assert br.a == br.b == 0 and len(br.path) == 57 and br.path[0] == br.path[-1] == int(SO.table(skel)[0][0]) and br.tortuosity == float("inf")
    t = SK.root_tree(g, (0, 0, 0))
    assert t.closes_cycle.tolist() == [True] and t.generation.tolist() == [-1]


def test_adjacent_junction_voxels_are_one_cluster():
    vol = np.zeros((16, 9, 3), np.uint8)
    vol[2:7, 4, 1] = 1; vol[7, 4, 1] = vol[8, 4, 1] = 1; vol[9:14, 4, 1] = 1          # a line along x ...
    vol[7, 5:8, 1] = 1; vol[8, 1:4, 1] = 1                                             # ... with a branch up from x = 7 and one down from x = 8
    deg = SO.degrees(vol)
    assert int((deg >= 3).sum()) >= 2
    g = _graph(vol)
    assert (g.nodes["kind"] == "junction").sum() == 1 and (g.nodes["kind"] == "end").sum() == 4 and len(g.branches) == 4
    j = int(np.flatnonzero(g.nodes["kind"] == "junction")[0])
    assert g.nodes["voxels"][j] == int((deg >= 3).sum()) and g.nodes["branches"][j] == 4 and g.components["cycles"].tolist() == [0]
    assert (g.nodes["x"][j], g.nodes["y"][j], g.nodes["z"][j]) == (float(np.mean([np.unravel_index(i, vol.shape, order="F")[0] for i in g.node_voxels[j]])),
                                                                 float(np.mean([np.unravel_index(i, vol.shape, order="F")[1] for i in g.node_voxels[j]])), 1.0)


def test_prune_removes_a_spur_and_keeps_a_long_branch():
    from covidseg_amd import skeleton as SK
    vol = np.zeros((30, 20, 3), np.uint8)
    vol[2:28, 5, 1] = 1                                              # a trunk of 26 voxels along x
    vol[10, 6:8, 1] = 1                                              # a spur of 2 voxels
    vol[20, 6:16, 1] = 1                                             # a branch of 10 voxels
    g = _graph(vol)
    assert (g.nodes["kind"] == "junction").sum() == 2 and (g.nodes["kind"] == "end").sum() == 4
    p = SK.prune(g, 3.0)
    assert (p.nodes["kind"] == "junction").sum() == 1 and (p.nodes["kind"] == "end").sum() == 3 and len(p.branches) == 3 and len(p.nodes) == 4
    # each T is a cluster of four voxels of degree >= 3 -- (9..11, 5) and (10, 6) -- so before pruning the pieces measure 7 | spur 1 | 8 | side 9 | 6 between the voxels they
    # touch; without the spur its junction joins 7 + 2 (through the cluster) + 8 into one branch
    assert sorted(b.length_mm for b in g.branches) == [1.0, 6.0, 7.0, 8.0, 9.0]
    assert sorted(b.length_mm for b in p.branches) == [6.0, 9.0, 17.0]
    on = set(np.concatenate([b.path for b in p.branches]).tolist())
    assert np.ravel_multi_index((10, 7, 1), vol.shape, order="F") not in on and np.ravel_multi_index((20, 15, 1), vol.shape, order="F") in on
    assert len(g.branches) == 5 and len(g.nodes) == 6               # prune leaves its argument alone
    assert len(SK.prune(g, 0.5).branches) == 5                       # nothing is that short
    one = SK.prune(g, 11.0)                                          # the spur goes, then the trunk's 6 (its 7 has become 17): one line from end to end is left
    assert len(one.branches) == 1 and sorted(one.nodes["kind"].tolist()) == ["end", "end"] and one.components["cycles"].tolist() == [0]
    assert one.branches[0].length_mm == pytest.approx(17.0 + np.sqrt(2.0) + 9.0, rel=1e-14)
    with pytest.raises(ValueError, match="radius_of"):
        SK.prune(g, None, 1.5)
    wide = ndimage.binary_dilation(vol, np.ones((3, 3, 3)), iterations=2).astype(np.uint8)
    gr = _graph(vol, radius_of=wide)
    assert gr.branches[[b.length_mm for b in gr.branches].index(1.0)].radius_a == np.sqrt(13.0)          # the nearest background voxel of the widened T lies at (3, 2) from (10, 6)
    assert len(SK.prune(gr, None, 1.0).branches) == 3 and len(SK.prune(gr, None, 0.25).branches) == 5          # the spur is 1 long where the tube's radius is 3.6


def test_rooting_flags_the_branch_that_closes_a_cycle():
    from covidseg_amd import skeleton as SK
    vol = np.zeros((20, 20, 3), np.uint8)
    vol[2:9, 10, 1] = 1                                              # a stem along x ...
    for i in range(1, 6):
        vol[8 + i, 10 + i, 1] = vol[8 + i, 10 - i, 1] = 1            # ... that splits ...
    for i in range(1, 5):
        vol[13 + i, 15 - i, 1] = vol[13 + i, 5 + i, 1] = 1           # ... and joins again
    vol[18, 10, 1] = 1
    g = _graph(vol)
    assert g.components["cycles"].tolist() == [1]
    t = SK.root_tree(g, (2, 10, 1))
    assert int(t.closes_cycle.sum()) == 1 and (t.generation[t.closes_cycle] == -1).all() and sorted(t.generation[~t.closes_cycle].tolist())[0] == 0


# ---- the label spread -----------------------------------------------------------------------------------------------------------------------------------
def test_the_label_spread_against_a_direct_statement():
    import lungmask_oracle as LO
    rng = np.random.default_rng(12)
    for conn in (1, 2, 3):
        mask = SO.blobs((17, 13, 9), 40 + conn, 0.5)
        seeds = (mask != 0) & (rng.random(mask.shape) < 0.02)
        arrival = LO.geodesic(seeds, mask, conn)[0]
        labels = np.zeros(mask.shape, np.int32)
        labels[seeds] = rng.permutation(int(seeds.sum())) + 1
        got = SO.label_spread(arrival, labels, conn)
        want = labels.copy()
        for s in range(1, int(arrival[arrival != 0xFFFF].max()) + 1):                                  # voxel by voxel
            prev = want.copy()
            for x, y, z in np.argwhere(arrival == s):
                best = 0
                for dx, dy, dz in SO.OFFSETS:
                    q = (x + dx, y + dy, z + dz)
                    if (dx != 0) + (dy != 0) + (dz != 0) > conn or min(q) < 0 or any(q[i] >= mask.shape[i] for i in range(3)):
                        continue
                    if arrival[q] == s - 1 and prev[q] != 0 and (best == 0 or prev[q] < best):
                        best = int(prev[q])
                if best:
                    want[x, y, z] = best
        assert np.array_equal(got, want)
        reached = arrival != 0xFFFF
        assert (got[reached] != 0).all() and (got[~reached] == 0).all()
    a = np.full((5, 1, 1), 0xFFFF, np.uint16); a[:, 0, 0] = (0, 1, 2, 1, 0)                            # equidistant from two seeds: the smaller label
    l = np.zeros((5, 1, 1), np.int32); l[0, 0, 0], l[4, 0, 0] = 7, 3
    assert SO.label_spread(a, l, 1)[:, 0, 0].tolist() == [7, 7, 3, 3, 3]


def test_argument_errors_need_no_device():
    from covidseg_amd import skeleton as SK
    m = np.zeros((4, 4, 4), np.uint8)
    for kw in (dict(endpoints=1), dict(max_iterations=-1), dict(max_iterations=1.5), dict(chunk=0), dict(return_device="yes")):
        with pytest.raises(ValueError):
            SK.thin_volume(m, **kw)
    for bad in (np.zeros((4, 4)), np.zeros((4, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            SK.thin_volume(bad)
    with pytest.raises(ValueError):
        SK.skeleton_table(m, pixdim=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        SK.airway_tree(m, leaves=True)
    with pytest.raises(ValueError, match="not guessed"):
        SK.airway_tree(m)                                            # no orientation
    with pytest.raises(ValueError):
        SK.vessel_tree(m, connectivity=4)
    with pytest.raises(ValueError):
        SK.branch_territories(m, None, "graph")
    from covidseg_amd import volume as V
    with pytest.raises(ValueError, match="lungs="):
        V.segment_volume(np.zeros((8, 8, 8), np.int16), None, airway_tree=True)
    with pytest.raises(ValueError, match="lungs="):
        V.segment_volume(np.zeros((8, 8, 8), np.int16), None, lungs=dict(airways=False), airway_tree=True)
    with pytest.raises(ValueError):
        V.segment_volume(np.zeros((8, 8, 8), np.int16), None, lungs=True, airway_tree=dict(leaves=1))


def test_the_package_exports_the_surface():
    import covidseg_amd
    from covidseg_amd import _lib, skeleton as SK
    for name in ("thin_volume", "skeleton_table", "skeleton_graph", "prune", "root_tree", "branch_territories", "airway_tree", "vessel_tree", "Skeleton", "SkeletonGraph",
                 "RootedTree", "BranchTerritories", "CenterlineTree"):
        assert getattr(covidseg_amd, name) is getattr(SK, name) and name in covidseg_amd.__all__
    for name in ("unet_vol_thin_ws_bytes", "unet_vol_thin_begin", "unet_vol_thin_iterations", "unet_vol_thin_end", "unet_vol_skeleton_ws_bytes", "unet_vol_skeleton_count",
                 "unet_vol_skeleton_emit", "unet_vol_label_spread"):
        assert name in _lib._PROTOS
    assert tuple(SO.OFFSETS) == tuple(SK.OFFSETS)

"""CPU: the two statements of the watershed definition in tests/watershed_oracle.py (the whole-volume numpy iteration and the priority queues) held to each other on every
case the GPU tests use, the counter-example that gives the ABI its phases, csrc/kernels_watershed.hip's own relaxations, brick rule and sweep sequence run on the CPU
(tools/watershed_host_check.hip), split_lesions' marker numbering, the figures of the two-ball case of DESIGN.md section 4ah, and the surface."""
import os
import subprocess

import numpy as np
import pytest

import watershed_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd")
MAIN_SHAPES = ((33, 9, 17), (65, 17, 9), (32, 8, 8), (64, 16, 8))
FIELDS = {"max": ("labels", "height", "steps"), "sum": ("labels", "distance")}


def _agree(cost, markers, mask, conn, rule):
    a, b = WO.fixed_point(cost, markers, mask, conn, rule), WO.by_heap(cost, markers, mask, conn, rule)
    for f in FIELDS[rule]:
        assert np.array_equal(a[f], b[f]), (cost.shape, conn, rule, f)
    assert tuple(a["counts"]) == tuple(b["counts"])
    return a


def _small(seed, shape=(20, 17, 1), n_markers=3):
    """a 20 x 17 image of costs 0 .. 5 with three markers: the size the definition was first tried at"""
    rng = np.random.default_rng(seed)
    cost = rng.integers(0, 6, shape).astype(np.uint32)
    markers = np.zeros(shape, np.int32)
    markers.reshape(-1)[rng.choice(cost.size, n_markers, replace=False)] = rng.permutation(n_markers) + 1
    return cost, markers


# ---- the two oracles ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MAIN_SHAPES)
def test_the_two_oracles_agree_on_the_main_cases(shape):
    for conn in (1, 2, 3):
        for rule in ("max", "sum"):
            cost, markers, mask, want = WO.asserted_content(shape, conn, rule)
            got = _agree(cost, markers, mask, conn, rule)
            assert np.array_equal(got["labels"], want["labels"])
            assert len(np.unique(want["labels"])) >= 3 and want["counts"][1] >= 1 and min(want["sweeps"]) >= 2 and WO.tie_decided(cost, markers, mask, conn, rule, want) >= 1
            assert abs(float((mask != 0).mean()) - 0.85) < 0.06 and 0.015 < float((markers > 0).mean()) < 0.06 and (cost % 8 == 0).all()


def test_the_two_oracles_agree_on_the_other_cases():
    cost, markers, mask = WO.serpentine((33, 17, 9))
    for rule in ("max", "sum"):
        res = _agree(cost, markers, mask, 1, rule)
        assert res["counts"][:2] == (int(mask.sum()), 0) and min(res["sweeps"]) > 500          # one voxel per whole-volume sweep: a corridor of some 1300 voxels, two ends
    big = np.full((300, 1, 1), 2 ** 32 - 2, np.uint32)
    m = np.zeros((300, 1, 1), np.int32); m[0, 0, 0] = 9
    res = _agree(big, m, None, 1, "sum")
    assert res["counts"] == (257, 43, 1, 0)                            # 256 (2^32 - 2) <= 2^40 - 2 < 257 (2^32 - 2): x = 257 is the one overflowed voxel
    for seed in range(6):
        for conn in (1, 2, 3):
            _agree(*_small(seed), None, conn, "max")
            _agree(*_small(seed, (7, 5, 4), 4), None, conn, "sum")
    line = np.zeros((1, 1, 7), np.uint32); m = np.zeros((1, 1, 7), np.int32); m[0, 0, 0], m[0, 0, 6] = 3, 1
    assert _agree(line, m, None, 1, "max")["labels"][0, 0].tolist() == [3, 3, 3, 1, 1, 1, 1]          # the middle is equally near: the lower label


def test_a_plateau_is_divided_and_not_swallowed():
    cost = np.zeros((9, 1, 1), np.uint32); cost[4, 0, 0] = 5
    m = np.zeros((9, 1, 1), np.int32); m[0, 0, 0], m[8, 0, 0] = 2, 1
    res = _agree(cost, m, None, 1, "max")
    assert res["labels"][:, 0, 0].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1] and res["height"][:, 0, 0].tolist() == [0, 0, 0, 0, 5, 0, 0, 0, 0] and res["steps"][4, 0, 0] == 4
    s = _agree(cost, m, None, 1, "sum")
    assert s["labels"][:, 0, 0].tolist() == [2, 2, 2, 2, 1, 1, 1, 1, 1] and s["distance"][:, 0, 0].tolist() == [0, 0, 0, 0, 5, 0, 0, 0, 0]


def test_one_key_for_height_and_label_is_not_the_definition():
    """height << k | label in one phase: (3, label 2) < (4, label 1), but through a voxel of cost 5 they become (5, 2) > (5, 1): the operator is not monotone.  The
    prototype's limit differs from the priority queues on these cases, which is why the ABI has a HEIGHT and a LABEL phase."""
    assert (3 << 24 | 2) < (4 << 24 | 1) and (max(3, 5) << 24 | 2) > (max(4, 5) << 24 | 1)
    differing = 0
    for seed in range(9):
        cost, markers = _small(seed)
        heap = WO.by_heap(cost, markers, None, 1, "max")["labels"]
        assert np.array_equal(WO.fixed_point(cost, markers, None, 1, "max")["labels"], heap)
        differing += int(not np.array_equal(WO.packed_one_phase(cost, markers, None, 1), heap))
    assert differing >= 1


# ---- the kernel file's own functions on the CPU ------------------------------------------------------------------------------------------------------------------------------
def test_the_kernels_relaxations_and_sweeps_on_the_cpu_equal_the_oracle(tmp_path):
    exe = str(tmp_path / "watershed_host_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tools", "watershed_host_check.hip"), "-o", exe], check=True, cwd=str(tmp_path))

    def run(cost, markers, mask, conn, rule, skip):
        N = cost.size
        for name, a, dt in (("cost", cost, np.uint32), ("markers", markers, np.int32), ("mask", mask, np.uint8)):
            np.asarray(a).reshape(-1, order="F").astype(dt).tofile(tmp_path / f"{name}.bin")
        out = subprocess.run([exe, *(str(n) for n in cost.shape), str(conn), rule, str(skip), *(str(tmp_path / f"{n}.bin") for n in ("cost", "markers", "mask", "out"))],
                             check=True, capture_output=True, text=True).stdout.strip().split("\n")
        raw = (tmp_path / "out.bin").read_bytes()
        vol = lambda off, dt: np.frombuffer(raw, dt, N, off).reshape(cost.shape, order="F")
        got = dict(labels=vol(0, np.int32), counts=tuple(int(v) for v in out[-1].split()[1:]), changed=[[int(v) for v in line.split()[1:]] for line in out[:-1]])
        got.update(dict(height=vol(4 * N, np.uint32), steps=vol(8 * N, np.uint32)) if rule == "max" else dict(distance=vol(4 * N, np.uint64)))
        return got

    cases = [(*WO.asserted_content((33, 9, 17), conn, rule)[:3], conn, rule) for conn in (1, 2, 3) for rule in ("max", "sum")]
    cases += [(*WO.asserted_content((65, 17, 9), 3, "max")[:3], 3, "max"), (*WO.serpentine((33, 17, 9)), 1, "max"), (*WO.serpentine((33, 17, 9)), 1, "sum")]
    big = np.full((300, 1, 1), 2 ** 32 - 2, np.uint32); m = np.zeros((300, 1, 1), np.int32); m[0, 0, 0], m[299, 0, 0] = 9, -3
    cases.append((big, m, np.ones((300, 1, 1), np.uint8), 1, "sum"))
    for cost, markers, mask, conn, rule in cases:
        want = WO.fixed_point(cost, markers, mask, conn, rule)
        got, plain = run(cost, markers, mask, conn, rule, 1), run(cost, markers, mask, conn, rule, 0)
        for f in FIELDS[rule]:
            assert np.array_equal(got[f], want[f]) and np.array_equal(plain[f], want[f]), (cost.shape, conn, rule, f)
        assert got["counts"] == plain["counts"] == tuple(want["counts"])
        assert got["changed"] == plain["changed"] and all(c[-1] == 0 and min(c[:-1], default=1) > 0 for c in got["changed"])          # the skip changes no sweep
    assert got["counts"] == (257, 43, 1, 1)
    assert len(run(*WO.serpentine((33, 17, 9)), 1, "max", 1)["changed"][0]) >= 10


# ---- split_lesions ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_marker_numbering():
    from covidseg_amd import watershed as W
    # components 1..4; cores: 1 (in component 2, 1 voxel), 2 (component 1, 9 voxels), 3 (component 2, 6 voxels), 4 (component 4, 1 voxel, its only core); component 3 has none
    size, owner = [1, 9, 6, 1], [2, 1, 2, 4]
    core, comp, parent = W.number_markers(size, owner, 4, 1)
    assert core.tolist() == [0, 1, 2, 3, 4] and comp.tolist() == [0, 0, 0, 5, 0] and parent.tolist() == [2, 1, 2, 4, 3]          # cores first in label order, then component 3
    core, comp, parent = W.number_markers(size, owner, 4, 3)
    assert core.tolist() == [0, 0, 1, 2, 3] and comp.tolist() == [0, 0, 0, 4, 0] and parent.tolist() == [1, 2, 4, 3]          # core 1 is dropped; core 4 stays: its component's only one
    core, comp, parent = W.number_markers([1, 2], [1, 1], 2, 5)
    assert core.tolist() == [0, 0, 0] and comp.tolist() == [0, 1, 2] and parent.tolist() == [1, 2]          # every core dropped: the components themselves
    rng = np.random.default_rng(2)
    comp_vol = np.zeros((12, 6, 1), np.int64); comp_vol[:5] = 1; comp_vol[6:9] = 2; comp_vol[10:] = 3
    cores = np.zeros_like(comp_vol); cores[1, 1:3] = 1; cores[3, 4] = 2; cores[7, 2] = 3
    for min_seed in (1, 2):
        markers, n, par = WO.numbered_markers(comp_vol, 3, cores, 3, min_seed)
        sizes = np.bincount(cores.reshape(-1))[1:]
        cn, kn, par2 = W.number_markers(sizes, [1, 1, 2], 3, min_seed)
        mine = np.where(cn[cores] > 0, cn[cores], kn[comp_vol])
        assert np.array_equal(mine, markers) and n == len(par2) and par.tolist() == par2.tolist()
    assert WO.numbered_markers(comp_vol, 3, cores, 3, 2)[1] == 3 and (WO.numbered_markers(comp_vol, 3, cores, 3, 2)[0][comp_vol == 3] == 3).all()


def test_two_balls_and_a_speck():
    mask = WO.two_balls()
    for conn in (1, 3):
        res = WO.split_lesions(mask, seed_depth_mm=6.0, conn=conn)
        assert int(mask.sum()) == 6116 and res["n_components"] == 2 and res["d2max"] == 82.0 and res["cores"] == 2 and res["n"] == 3 and res["parent"].tolist() == [1, 1, 2]
        assert np.bincount(res["labels"].reshape(-1)).tolist()[1:] == [3070, 3013, 33]
        assert res["labels"][22:26, 12, 12].tolist() == [1, 1, 2, 2]          # part 2 begins at x = 24 on the axis; the tie at x = 23 goes to the lower label
        assert np.array_equal(res["labels"] > 0, mask > 0)
        heap = WO.by_heap(res["cost"], res["markers"], mask, conn, "max")
        assert np.array_equal(heap["labels"], res["labels"])
    assert WO.depth_cost([82.0, 81.9, 0.0, 90.0, 3.0], [1, 1, 1, 1, 0], 82.0, 0.25).tolist() == [0, 0, 328, 0, 0]


# ---- the surface --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    from covidseg_amd import volume as V
    from covidseg_amd import watershed as W
    c, m = np.zeros((4, 4, 4), np.uint32), np.zeros((4, 4, 4), np.int32)
    for kw in (dict(connectivity=4), dict(rule="min"), dict(max_sweeps=0), dict(max_sweeps=1.5), dict(chunk=0), dict(return_device="yes"), dict(allow_overflow=1)):
        with pytest.raises(ValueError):
            W.watershed(c, m, **kw)
    for bad_c, bad_m in ((c.astype(np.float32), m), (np.zeros((4, 4)), m), (c, m[:3]), (c.astype(np.int64) - 1, m), (c.astype(np.uint64) + 2 ** 32 - 1, m), (c, m - 1), (c, m + 2 ** 24)):
        with pytest.raises(ValueError):
            W.watershed(bad_c, bad_m)
    for kw in (dict(pixdim=(1.0, 0.0, 1.0)), dict(seed_depth_mm=0.0), dict(seed_depth_mm="deep"), dict(min_seed_voxels=0), dict(quantum_mm2=-1.0), dict(connectivity=0)):
        with pytest.raises(ValueError):
            W.split_lesions(np.zeros((4, 4, 4), np.uint8), **kw)
    for bad in ("yes", dict(depth=1.0), dict(seed_depth_mm=-2.0)):
        with pytest.raises(ValueError):
            V.segment_volume(np.zeros((8, 8, 8), np.int16), None, split_lesions=bad)


def test_the_package_exports_the_surface():
    import covidseg_amd
    from covidseg_amd import _lib, watershed as W
    assert covidseg_amd.watershed is W and "watershed" in covidseg_amd.__all__
    for name in ("watershed_device", "depth_cost_device", "split_lesions", "split_lesions_device", "WatershedResult", "SplitLesions", "WatershedError"):
        assert getattr(covidseg_amd, name) is getattr(W, name) and name in covidseg_amd.__all__
    header = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    source = open(os.path.join(PKG, "csrc", "kernels_watershed.hip")).read()
    for name in ("unet_vol_watershed_ws_bytes", "unet_vol_watershed_begin", "unet_vol_watershed_sweeps", "unet_vol_watershed_end", "unet_vol_depth_cost"):
        assert name in _lib._PROTOS and f" {name}(" in header and f" {name}(" in source
    for name, value in (("HEIGHT", W.HEIGHT), ("LABEL", W.LABEL), ("SUM", W.SUM)):
        assert f"#define UNET_VOL_WATERSHED_{name} {value}\n" in header
    assert (W.COST_MAX, W.LABEL_MAX, W.DIST_MAX) == (2 ** 32 - 2, WO.LABEL_MAX, WO.DIST_MAX)
    assert "kernels_watershed.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()

"""CPU: tests/lungmask_oracle.py against scipy.ndimage (the threshold on get_fdata's values, the growth as iterated masked dilations, the reconstruction by labels), the
leak rule on written-out count series, the trachea search, the whole procedure on a phantom chest, the declarations and bindings of the new entries, the shape rule of
their later-trip cases, and every argument error of lungs.* and of segment_volume(lungs=), which must be raised before a device is needed."""
import inspect
import os
import re

import numpy as np
import pytest

import components_oracle as CO
import later_trips as LT
import lungmask_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [(1, 1, 1), (5, 1, 2), (9, 7, 5), (65, 6, 3), (13, 11, 4)]


# ---- the oracle against scipy ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_threshold_is_a_comparison_on_get_fdata():
    from covidseg_amd import nifti_min
    rng = np.random.default_rng(1)
    for dt, slope, inter in (("i2", 0.0, 0.0), ("i2", 0.5, -1024.0), ("u1", -2.0, 100.0), ("f4", 1.0 / 3.0, 0.1), ("f8", 0.0, 0.0)):
        raw = np.asfortranarray((rng.standard_normal((9, 7, 5)) * 60 + 100).astype(dt))
        if dt[0] == "f":
            raw[0, 0, 0], raw[1, 0, 0], raw[2, 0, 0] = np.nan, np.inf, -np.inf
        vol = nifti_min.NiftiVolume(raw, slope, inter, (1.0, 1.0, 1.0), nifti_min.default_header(raw.shape), "<")
        fd = vol.get_fdata()
        dec = LO.decode(raw, *((slope, inter) if vol.scaling is not None else (None, None)))
        assert np.array_equal(dec, fd, equal_nan=True)
        region = rng.random(raw.shape) < 0.7
        edge = float(fd[3, 3, 3])                                     # a value exactly on an edge: in as lo, out as hi
        for lo, hi in ((None, edge), (edge, None), (edge, edge + 50.0), (-np.inf, np.inf), (None, None)):
            with np.errstate(invalid="ignore"):
                want = (fd >= (-np.inf if lo is None else lo)) & (fd < (np.inf if hi is None else hi))
            got, counts = LO.threshold(dec, lo, hi)
            assert got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(counts, want.sum(axis=(0, 1)))
            assert np.array_equal(LO.threshold(dec, lo, hi, region)[0], want & region)
        assert LO.threshold(dec, edge, None)[0][3, 3, 3] == 1 and LO.threshold(dec, None, edge)[0][3, 3, 3] == 0
    for bad in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan)):
        with pytest.raises(ValueError):
            LO.threshold(np.zeros((2, 2, 2)), *bad)


@pytest.mark.parametrize("shape", RAGGED)
def test_the_growth_is_an_iterated_masked_dilation(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(sum(shape))
    constraint = rng.random(shape) < 0.6
    seeds = rng.random(shape) < 0.05
    seeds[0, 0, 0] = True
    for conn, planar in ((1, False), (2, False), (3, False), (1, True), (2, True)):
        s = ndi.generate_binary_structure(3, conn)
        if planar:
            s[:, :, 0] = s[:, :, 2] = False
        arrival, counts = LO.geodesic(seeds, constraint, conn, planar)
        reached = seeds & constraint
        want = np.full(shape, 0xFFFF, np.uint16)
        want[reached] = 0
        wc = [int(reached.sum())]
        step = 0
        while wc[0]:
            grown = ndi.binary_dilation(reached, s, mask=constraint) if reached.any() else reached
            new = grown & ~reached
            if not new.any():
                break
            step += 1
            want[new] = step
            wc.append(int(new.sum()))
            reached = grown
        assert np.array_equal(arrival, want) and np.array_equal(counts, wc), (shape, conn, planar)
        assert int(counts.sum()) == int((arrival < 0xFFFF).sum())
        if len(wc) > 2:                                               # max_steps reached with voxels left
            a2, c2 = LO.geodesic(seeds, constraint, conn, planar, max_steps=1)
            assert np.array_equal(c2, wc[:2]) and np.array_equal(a2, np.where(want <= 1, want, 0xFFFF))
    a0, c0 = LO.geodesic(np.zeros(shape, bool), constraint)
    assert np.array_equal(c0, [0]) and (a0 == 0xFFFF).all()


def test_reconstruct_keeps_the_marked_components():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    mask = rng.random((13, 11, 6)) < 0.35
    marker = rng.random(mask.shape) < 0.02
    for conn in (1, 2, 3):
        lab, n = ndi.label(mask, ndi.generate_binary_structure(3, conn))
        hit = np.unique(lab[marker & mask])
        want = np.isin(lab, hit[hit > 0])
        assert np.array_equal(LO.reconstruct(mask, marker, conn), want)
    assert not LO.reconstruct(mask, np.zeros(mask.shape, bool)).any()


# ---- the leak rule --------------------------------------------------------------------------------------------------------------------------------------------------
PLATEAU = [60, 58, 61, 59, 60, 57, 40, 33, 20, 14, 9, 5, 2, 1]
LEAK = [60, 58, 61, 59, 60, 57, 40, 33, 20, 14, 16, 14, 19, 30, 43, 80, 150]
TAIL = [60, 58, 61, 59, 40, 20, 9, 2, 2, 6, 6, 3]


def test_the_leak_rule_on_written_out_series():
    from covidseg_amd import lungs as L
    for rule in (LO.leak_rule, L.leak_rule):
        assert rule(PLATEAU) == (None, len(PLATEAU) - 1)              # a plateau that tapers to zero
        assert rule(LEAK) == (14, 11)                                 # 43 > 3 x 14: the leak; the last 14 is the stop (30 <= 42 is none yet)
        assert rule(TAIL) == (None, len(TAIL) - 1)                    # 6 = 3 x 2 but under 3 x min_front
        assert rule(TAIL, min_front=1) == (None, len(TAIL) - 1) and rule(TAIL, leak_ratio=2.5, min_front=1) == (9, 8)
        assert rule([5]) == (None, 0) and rule([5, 4, 3]) == (None, 2) and rule([3, 3, 3, 3, 100]) == (4, 3)
        assert rule([10, 9, 9, 12, 11, 9, 40]) == (6, 5)


# ---- the phantom ----------------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's own figures on the two phantoms (DESIGN.md section 4ae records them)
PLAIN = dict(steps=55, leak_step=None, stop_step=55, kept=2)
LEAKY = dict(leak_step=50, stop_step=43, kept=2)
_CACHE = {}


def _run(leak, superior="z-"):
    key = (leak, superior)
    if key not in _CACHE:
        ph = LO.phantom(leak=leak, superior=superior)
        _CACHE[key] = (ph, LO.lung_mask(LO.decode(ph["hu"]), ph["pixdim"], superior))
    return _CACHE[key]


@pytest.mark.parametrize("leak", [False, True])
def test_the_procedure_finds_the_lungs_of_the_phantom(leak):
    ph, r = _run(leak)
    a = r["airways"]
    assert ph["hu"].shape == (112, 96, 56) and ph["hu"].dtype == np.int16 and ph["pixdim"] == (1.5, 1.5, 3.0)
    assert r["error"] is None and r["airway_error"] is None and a is not None
    d = LO.dice(r["mask"], ph["lungs"])
    inside = int((a["mask"] & ph["leak_region"]).sum())
    print(f"phantom leak={leak}: steps {len(a['counts']) - 1}, leak {a['leak_step']}, stop {a['stop_step']}, airway voxels {int(a['mask'].sum())}, in the leak region {inside}, "
          f"trachea left {int((r['mask'] & ph['trachea']).sum())}, kept {r['kept']} {r['voxels']}, dice {d:.4f}")
    assert d >= 0.98
    assert not (r["mask"] & ph["trachea"]).any()
    assert len(r["kept"]) == 2
    assert (a["leak_step"] is not None) == leak
    assert inside <= 0.05 * int(a["mask"].sum())
    want = LEAKY if leak else PLAIN
    assert a["leak_step"] == want["leak_step"] and a["stop_step"] == want["stop_step"] and len(r["kept"]) == want["kept"]
    if not leak:
        assert len(a["counts"]) - 1 == want["steps"]
    lab, n = CO.label(r["mask"], 1)                                   # one component per lung, each on its side
    assert n == 2


def test_the_flipped_phantom_gives_the_flipped_mask():
    ph, r = _run(True)
    fh, fr = _run(True, "z+")
    assert np.array_equal(fh["hu"], ph["hu"][:, :, ::-1])
    assert np.array_equal(fr["mask"], r["mask"][:, :, ::-1]) and np.array_equal(fr["airways"]["counts"], r["airways"]["counts"])
    assert np.array_equal(fr["airways"]["mask"], r["airways"]["mask"][:, :, ::-1])


def test_the_paths_without_airways():
    ph, r = _run(False)
    v = LO.decode(ph["hu"])
    none = LO.lung_mask(v, ph["pixdim"], None)                        # no orientation: the step is skipped, the trachea joins the lungs
    assert none["airway_error"] == "no orientation" and none["airways"] is None and len(none["kept"]) == 1 and (none["mask"] & ph["trachea"]).any()
    off = LO.lung_mask(v, ph["pixdim"], "z-", airways=False)
    assert off["airway_error"] is None and np.array_equal(off["mask"], none["mask"])
    small = LO.lung_mask(v, ph["pixdim"], "z-", trachea_kw=dict(area_mm2=(1.0, 20.0)))          # no candidate of that area
    assert small["airway_error"] == "no trachea" and small["airways"] is None and np.array_equal(small["mask"], none["mask"])
    wrong = LO.lung_mask(v, ph["pixdim"], "z+")                       # walked from the wrong end the bowel gas is taken for the trachea: why the end is never guessed
    assert wrong["airways"] is not None and (wrong["mask"] & ph["trachea"]).any() and not (wrong["airways"]["mask"] & ph["trachea"]).any()
    assert LO.lung_mask(v, ph["pixdim"], "z-", min_lung_ml=1e6)["error"] is not None


def test_the_trachea_search_of_the_product_is_the_oracles():
    from covidseg_amd import lungs as L
    import morph_oracle as MO
    ph, _ = _run(False)
    v = LO.decode(ph["hu"])
    air = LO.threshold(v, hi=-320.0, region=LO.body_mask(v))[0]
    lab, n = MO.label_planar(air, 1)
    st = CO.stats(lab, n)
    for superior in ("z-", "z+"):
        for kw in ({}, dict(seed_slices=1), dict(seed_shift_mm=0.5), dict(area_mm2=(500.0, 5000.0), max_extent_mm=80.0), dict(area_mm2=(1.0, 20.0))):
            want = LO.find_trachea(air, ph["pixdim"], superior, **kw)
            got = L.trachea_from_stats(st, air.shape[2], ph["pixdim"], superior, *L._check_trachea_args(**kw))
            assert (got is None) == (want is None) and (want is None or got + 1 == want["label"]), (superior, kw)
    seed = LO.find_trachea(air, ph["pixdim"], "z-")
    assert seed["z"] == 0 and abs(seed["cx"] * 1.5 - 84.0) < 1.5 and abs(seed["cy"] * 1.5 - 60.0) < 1.5
    assert L.superior_of(("L", "P", "S")) == "z+" and L.superior_of("RAI") == "z-" and L.superior_of(("L", "S", "P")) is None and L.superior_of(None) is None


# ---- declarations, bindings, exports ------------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_bound_and_built():
    import covidseg_amd
    from covidseg_amd import _lib, lungs as L, volume as V
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    hdr = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for name, nargs, res in (("unet_vol_threshold", 15, _lib.i32), ("unet_vol_geodesic_ws_bytes", 3, _lib.sz), ("unet_vol_geodesic_begin", 11, _lib.i32),
                             ("unet_vol_geodesic_steps", 13, _lib.i32)):
        m = re.search(r"(?:int32_t|size_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr)
        assert m and m.group(1).count(",") + 1 == nargs, name
        assert name in _lib._PROTOS and len(_lib._PROTOS[name][1]) == nargs and _lib._PROTOS[name][0] is res and name in _lib.EXPORTED_SYMBOLS
    m = re.search(r"int32_t\s+unet_vol_threshold\s*\(([^;{]*?)\)\s*;", hdr).group(1)
    assert "double lo, double hi" in m and "const uint8_t* region, uint8_t* mask, int64_t* slice_counts" in m
    assert [_lib._PROTOS["unet_vol_threshold"][1][i] for i in (7, 8, 9, 10)] == [_lib.f64] * 4
    assert _lib.ABI_VERSION == 16 and re.search(r"#define UNET_ABI_VERSION 16\b", text)
    assert re.search(r"#define UNET_VOL_GEODESIC_MAX_STEP 65534\b", text) and _lib.GEODESIC_MAX_STEP == 65534 == L.MAX_STEP == LO.MAX_STEP
    assert "DESIGN.md section 4ae" in text and "GEODESIC STEP DISTANCE" in text
    mk = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    first = [line for line in mk.splitlines() if line.startswith("SRCS =")]
    assert len(first) == 1 and re.search(r"\bkernels_lungmask\.hip\b", first[0])
    assert mk.count("kernels_lungmask") >= 5                         # SRCS, the comment, the -ffp-contract=off list in its three places
    assert re.search(r"^# kernels_lungmask\.hip: ", mk, flags=re.M)
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "kernels_lungmask.hip")).read()
    assert re.search(r"constexpr long long GRID_CAP = ([^;]+);", src)
    assert "atomicAdd(" in src and not re.search(r"atomicAdd\([^;]*\(float\)|atomicAdd\([^;]*\(double\)", src)          # integer atomics only
    names = ("lung_mask", "threshold_volume", "geodesic_distance", "reconstruct", "body_mask", "find_trachea", "grow_airways", "LungMask", "AirwayGrowth", "TracheaSeed",
             "LungMaskError")
    for name in names:
        assert getattr(covidseg_amd, name) is getattr(L, name) and name in covidseg_amd.__all__
    assert "lungs" in covidseg_amd.__all__ and issubclass(L.LungMaskError, ValueError)
    assert "not clinically validated" in L.grow_airways.__doc__ and "never guessed" in L.lung_mask.__doc__ and "not millimetres" in L.geodesic_distance.__doc__
    for fn in (V.segment_volume, V.segment_volume_ensemble):
        assert inspect.signature(fn).parameters["lungs"].default is None
    sig = inspect.signature(L.lung_mask).parameters
    assert [sig[k].default for k in ("model", "threshold", "air_hu", "body_hu", "airways", "airway_dilate_mm", "min_lung_ml", "min_ratio", "fill", "close_mm", "orientation",
                                     "out_path", "return_device", "batch_size", "img_size")] == [None, 0.5, -320.0, -500.0, "auto", None, 50.0, 0.25, True, None, None, None,
                                                                                                 False, 32, 512]
    g = inspect.signature(L.grow_airways).parameters
    assert [g[k].default for k in ("airway_hu", "leak_ratio", "min_front", "ref_steps", "max_steps", "connectivity")] == [-950.0, 3.0, 8, 4, 2000, 1]
    t = inspect.signature(L.find_trachea).parameters
    assert [t[k].default for k in ("area_mm2", "max_extent_mm", "seed_slices", "seed_shift_mm")] == [(50.0, 1200.0), 35.0, 3, 10.0]


def test_the_later_trip_cases_obey_the_shape_rule():
    """the caps read out of the .hip text: every workgroup makes at least two trips, and one makes a ragged further one"""
    from covidseg_amd import _lib
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "kernels_lungmask.hip")).read()
    tpb = LT.constant_value(re.search(r"constexpr int TPB = ([^;]+);", src).group(1))
    cap = LT.constant_value(re.search(r"constexpr long long GRID_CAP = ([^;]+);", src).group(1))
    vec = LT.constant_value(re.search(r"constexpr int TH_VEC = ([^;]+);", src).group(1))
    assert (tpb, cap, vec) == (LO.TPB, LO.GRID_CAP, LO.TH_VEC) and LO.TRIP == tpb * cap and tpb == LT.TPB
    n = int(np.prod(LO.LATER_THRESHOLD_VEC))
    assert LT.shape_rule(-(-n // vec), LO.TRIP) and n % vec != 0     # items of 8 voxels; the last one is short
    assert LT.shape_rule(int(np.prod(LO.LATER_THRESHOLD_ONE)), LO.TRIP)
    X, Y, Z = LO.LATER_GROWTH
    words = ((X + 63) // 64) * Y * Z                                  # the step kernel takes one word per lane, rows are padded to words
    assert X == 2 and LT.shape_rule(words, LO.TRIP) and X * Y * Z < 10_000_000
    assert LT.later_trips(words * 4, LO.TRIP)[0] >= 2                # the pack of _begin: four lanes per word


# ---- every argument error comes before a device is needed -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from covidseg_amd import volume as V

    def boom(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(V, "_ctx", boom)
    monkeypatch.setattr(V, "upload", boom)
    monkeypatch.setattr(V, "_mask_to_device", boom)
    return V


def test_the_passes_refuse_their_arguments_before_any_device_work(no_device):
    from covidseg_amd import lungs as L
    ct = np.zeros((4, 4, 4), np.int16)
    m = np.zeros((4, 4, 4), np.uint8)
    for bad in (dict(lo=float("nan")), dict(hi=float("nan")), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(lo=float("inf")), dict(hi=float("-inf")), dict(lo="0"),
                dict(hi=True), dict(region=np.zeros((4, 4, 5), np.uint8)), dict(region=np.zeros((4, 4, 4), np.float32)), dict(return_device=1), dict(src_shape=(4, 4, 4))):
        with pytest.raises(ValueError):
            L.threshold_volume(ct, **bad)
    with pytest.raises(ValueError):
        L.threshold_volume(np.zeros((4, 4), np.int16), hi=0.0)
    for bad in (dict(connectivity=0), dict(connectivity=4), dict(connectivity=3, per_slice=True), dict(per_slice=1), dict(chunk=0), dict(chunk=65535), dict(chunk=1.0),
                dict(chunk=True), dict(max_steps=0), dict(max_steps=65535), dict(max_steps=2.0), dict(return_device=1)):
        with pytest.raises(ValueError):
            L.geodesic_distance(m, m, **bad)
    with pytest.raises(ValueError):
        L.geodesic_distance(m, np.zeros((4, 4, 5), np.uint8))
    with pytest.raises(ValueError):
        L.geodesic_distance(m.astype(np.float32), m)
    for bad in (dict(connectivity=4), dict(return_device="no")):
        with pytest.raises(ValueError):
            L.reconstruct(m, m, **bad)
    with pytest.raises(ValueError):
        L.reconstruct(m, np.zeros((3, 4, 4), np.uint8))
    for bad in (float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            L.body_mask(ct, body_hu=bad)
    for args, kw in (((m, (1, 1, 1), "up"), {}), ((m, (1, 1), "z+"), {}), ((m, (1, 0, 1), "z+"), {}), ((m, (1, 1, 1), "z+"), dict(area_mm2=(10.0,))),
                     ((m, (1, 1, 1), "z+"), dict(area_mm2=(20.0, 10.0))), ((m, (1, 1, 1), "z-"), dict(max_extent_mm=0.0)), ((m, (1, 1, 1), "z-"), dict(seed_slices=0)),
                     ((m, (1, 1, 1), "z-"), dict(seed_slices=2.0)), ((m, (1, 1, 1), "z-"), dict(seed_shift_mm=-1.0)), ((m.astype(np.float64), (1, 1, 1), "z-"), {})):
        with pytest.raises(ValueError):
            L.find_trachea(*args, **kw)
    for bad in (dict(airway_hu=float("nan")), dict(leak_ratio=1.0), dict(leak_ratio=float("inf")), dict(leak_ratio="3"), dict(min_front=0), dict(min_front=1.5),
                dict(ref_steps=0), dict(max_steps=None), dict(max_steps=0), dict(max_steps=70000), dict(connectivity=5), dict(return_device=1)):
        with pytest.raises(ValueError):
            L.grow_airways(ct, m, m, **bad)
    with pytest.raises(ValueError):
        L.grow_airways(ct, np.zeros((4, 4, 5), np.uint8), m)
    with pytest.raises(ValueError):
        L.grow_airways(ct, m, np.zeros((4, 4, 5), np.uint8))
    # good arguments pass the checks and only then ask for the device
    for call in (lambda: L.threshold_volume(ct, hi=0.0), lambda: L.geodesic_distance(m, m), lambda: L.reconstruct(m, m), lambda: L.body_mask(ct),
                 lambda: L.find_trachea(m, (1, 1, 1), "z+"), lambda: L.grow_airways(ct, m, m)):
        with pytest.raises((AssertionError, RuntimeError, ImportError)):
            call()


def test_lung_mask_refuses_its_arguments_before_any_device_work(no_device, tmp_path):
    from covidseg_amd import lungs as L
    from covidseg_amd import nifti_min
    V = no_device
    ct = np.zeros((4, 4, 4), np.int16)
    for bad in (dict(model=object()), dict(threshold=1.5), dict(threshold="0.5"), dict(air_hu=float("nan")), dict(body_hu=None), dict(airways="yes"), dict(airways=1),
                dict(airway_dilate_mm=-1.0), dict(min_lung_ml=-1.0), dict(min_lung_ml=float("nan")), dict(min_ratio=0.0), dict(min_ratio=1.5), dict(fill=1),
                dict(close_mm=float("inf")), dict(orientation="XYZ"), dict(orientation=np.zeros((3, 3))), dict(batch_size=0), dict(img_size=0.5), dict(pixdim=(1, 1)),
                dict(return_device=1), dict(out_path=3), dict(leak_ratio=0.5), dict(min_front=0), dict(ref_steps=0), dict(max_steps=0), dict(seed_slices=0),
                dict(area_mm2=(5.0, 1.0)), dict(connectivity=4), dict(chunk=8), dict(unknown=1), dict(src_shape=(4, 4, 4))):
        with pytest.raises(ValueError):
            L.lung_mask(ct, **bad)
    with pytest.raises(ValueError, match="superior"):                 # airways=True without an orientation: before any device work
        L.lung_mask(ct, airways=True)
    with pytest.raises(ValueError, match="superior"):
        L.lung_mask(ct, airways=True, orientation="LSP")              # axis 2 is no S / I axis
    vol = nifti_min.NiftiVolume(np.asfortranarray(ct), 0.0, 0.0, (1.0, 1.0, 1.0), nifti_min.header_with_affine(ct.shape, nifti_min.affine_from_axcodes("LPS")), "<")
    for call in (lambda: L.lung_mask(ct), lambda: L.lung_mask(ct, airways=True, orientation="LPS"), lambda: L.lung_mask(vol, airways=True)):
        with pytest.raises((AssertionError, RuntimeError, ImportError)):          # the checks pass; only then the device is asked for
            call()

    class Model:
        h = 64

        def predict(self, x, batch_size=32):
            raise AssertionError("predict was called")
    for bad in (dict(lungs=True, lung_mask=np.ones((4, 4, 4), np.uint8)), dict(lungs={}, lung_mask=np.ones((4, 4, 4), np.uint8)), dict(lungs=1), dict(lungs="auto"),
                dict(lungs=dict(air=0)), dict(lungs=dict(min_ratio=2.0)), dict(lungs=dict(airways="maybe")), dict(lungs=dict(out_path="x.nii")),
                dict(lungs=dict(return_device=True))):
        with pytest.raises(ValueError):
            V.segment_volume(ct, Model(), **bad)
        with pytest.raises(ValueError):
            V.segment_volume_ensemble(ct, [Model()], **bad)
    with pytest.raises(ValueError, match="lung_mask"):                # per_lung still needs a lung mask when lungs= is off
        V.segment_volume(ct, Model(), per_lung=True)
    with pytest.raises((AssertionError, RuntimeError, ImportError)):  # with lungs= it passes the checks
        V.segment_volume(ct, Model(), lungs=True, per_lung=dict(orientation="LPS"))

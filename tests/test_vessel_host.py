"""CPU: tests/vessel_oracle.py, the numpy restatement of csrc/kernels_vessel.hip, against independent references -- its Jacobi against np.linalg.eigvalsh, its exp(-u)
against np.exp, its Hessian against polynomials whose second differences are exact, its vessel_mask against a phantom with a tube, a ball and a plate -- and every
argument check of covidseg_amd.vessels that needs no device.  tests/test_gpu_vessels.py holds the device to the oracle for equality."""
import os
import re
import subprocess

import numpy as np
import pytest

import lungmask_oracle as LO
import vessel_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrices(seed):
    """float32-valued symmetric matrices at the scales 1e-3, 1, 1e3: random ones, ones with zero off-diagonals (one, two, all three), with equal diagonals, the zero
    matrix, a multiple of the identity, a rank-one matrix -> the six entries as float64 [n]"""
    rng = np.random.default_rng(seed)
    rows = []
    for scale in (1e-3, 1.0, 1e3):
        a = (rng.standard_normal((4000, 6)) * scale).astype(np.float32).astype(np.float64)
        a[500:1000, 3] = 0.0
        a[1000:1500, 3:5] = 0.0
        a[1500:2000, 3:6] = 0.0                                       # diagonal already
        a[2000:2500, 1] = a[2000:2500, 0]                              # two equal diagonal entries
        a[2500:3000, 1] = a[2500:3000, 0]; a[2500:3000, 2] = a[2500:3000, 0]          # all three equal
        a[3000:3200, 3:6] = 0.0; a[3000:3200, 1] = a[3000:3200, 0]; a[3000:3200, 2] = a[3000:3200, 0]          # multiples of the identity
        v = (rng.standard_normal((300, 3)) * np.sqrt(scale)).astype(np.float32).astype(np.float64)          # rank one: v v^T rounded to float32
        r1 = np.stack([v[:, 0] * v[:, 0], v[:, 1] * v[:, 1], v[:, 2] * v[:, 2], v[:, 0] * v[:, 1], v[:, 0] * v[:, 2], v[:, 1] * v[:, 2]], 1).astype(np.float32).astype(np.float64)
        a[3200:3500] = r1
        a[3500] = 0.0                                                 # the zero matrix
        rows.append(a)
    return np.concatenate(rows)


def test_jacobi_agrees_with_eigvalsh():
    """|sorted(jacobi) - eigvalsh| <= 1e-12 max|lambda| on 12,000 float32-valued matrices.  The bound is not tuned: it only has to sit far under the float32 the result is
    stored in (6e-8) and far above LAPACK's own rounding.  The oracle's own figure: 1.3e-15 after five sweeps and the same after four."""
    a = _matrices(3)
    d = np.sort(np.stack(VO.jacobi(*a.T), 1), axis=1)
    M = np.zeros((a.shape[0], 3, 3))
    M[:, 0, 0], M[:, 1, 1], M[:, 2, 2] = a[:, 0], a[:, 1], a[:, 2]
    M[:, 0, 1] = M[:, 1, 0] = a[:, 3]
    M[:, 0, 2] = M[:, 2, 0] = a[:, 4]
    M[:, 1, 2] = M[:, 2, 1] = a[:, 5]
    want = np.linalg.eigvalsh(M)
    top = np.abs(want).max(axis=1)
    err = np.abs(d - want).max(axis=1)
    zero = top == 0
    assert zero.sum() == 3 and (d[zero] == 0).all()
    worst = float((err[~zero] / top[~zero]).max())
    d4 = np.sort(np.stack(VO.jacobi(*a.T, sweeps=4), 1), axis=1)
    print(f"jacobi against eigvalsh: worst error {worst:.3g} of the largest |lambda| after 5 sweeps, {float((np.abs(d4 - want).max(axis=1)[~zero] / top[~zero]).max()):.3g} after 4")
    assert worst <= 1e-12
    diag = (a[:, 3] == 0) & (a[:, 4] == 0) & (a[:, 5] == 0)          # nothing to rotate: the diagonal leaves untouched
    assert diag.sum() >= 2000 and np.array_equal(np.stack(VO.jacobi(*a[diag].T), 1), a[diag, :3])


def test_sort_is_stable_by_magnitude():
    d = np.array([[3.0, -3.0, 1.0], [-2.0, 2.0, -2.0], [0.0, -0.0, 0.0], [1.0, 2.0, 3.0], [3.0, 2.0, 1.0], [2.0, -3.0, 1.0]])
    got = np.stack(VO.sort_by_magnitude(*d.T), 1)
    want = np.array([[1.0, 3.0, -3.0], [-2.0, 2.0, -2.0], [0.0, -0.0, 0.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, -3.0]])
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


def test_exp_neg_against_numpy():
    """within 4 units of 2^-53 of np.exp(-u), relative, on [0, 700]; 1 at 0.  The oracle's own figure: 2.0 units."""
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.uniform(0.0, 700.0, 400000), rng.uniform(0.0, 2.0, 200000), np.arange(0, 701, dtype=np.float64), np.arange(1, 1000) * (np.log(2.0) / 2.0),
                        [0.0, 5e-324, 1e-300, 2.0 ** -60, 700.0]])
    got, want = VO.exp_neg(u), np.exp(-u)
    worst = float((np.abs(got - want) / want).max() / 2.0 ** -53)
    print(f"exp_neg against np.exp: worst relative error {worst:.3g} units of 2^-53")
    assert worst <= 4.0
    assert VO.exp_neg(np.array([0.0]))[0] == 1.0 and VO.exp_neg(np.array([-0.0]))[0] == 1.0
    big = VO.exp_neg(np.array([745.0, 800.0, np.inf, np.nan]))      # the clamp, which a NaN takes too
    assert (big == big[0]).all() and 0.0 <= big[0] < 1e-300


def _grid(shape):
    return np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")


def test_hessian_of_polynomials_is_exact():
    """small integers, exact in float32, sigma = h = 1 (kxx = 1, kxy = 1 / 4): the interior eigenvalues are exactly {0, 0, 2}, {-1, 0, 1}, {2, 2, 2}, 0, 0; at the faces
    what the repeated edge voxel implies"""
    shape = (7, 6, 5)
    X, Y, Z = shape
    x, y, z = _grid(shape)
    k = VO.hessian_factors(1.0, (1.0, 1.0, 1.0))
    assert k == [1.0, 1.0, 1.0, 0.25, 0.25, 0.25]
    inner = (slice(1, -1),) * 3
    cases = {"x2": (x * x, (0.0, 0.0, 2.0)), "xy": (x * y, (0.0, -1.0, 1.0)), "r2": ((x * x + y * y) + z * z, (2.0, 2.0, 2.0)), "ramp": ((x + 2.0 * y) + 3.0 * z, (0.0, 0.0, 0.0)),
             "const": (np.full(shape, 7.0), (0.0, 0.0, 0.0))}
    for name, (f, want) in cases.items():
        e = VO.eigenvalues(f.astype(np.float32), k)
        for i in range(3):
            assert (e[i][inner] == np.float32(want[i])).all(), (name, i)
    # the faces.  x^2: L[-1] = L[0] gives Hxx = (1 + 0) - 0 = 1 at x = 0 and L[X] = L[X - 1] gives (X - 2)^2 - (X - 1)^2 = -(2 X - 3) at x = X - 1; nothing else moves
    e = VO.eigenvalues((x * x).astype(np.float32), k)
    assert (e[2][0] == 1.0).all() and (e[2][X - 1] == -(2.0 * X - 3.0)).all() and (e[:2] == 0.0).all()
    # a ramp a x + b y + c z: the second difference at a face is the slope (low face) or minus the slope (high face); an edge has two of them, a corner three
    e = VO.eigenvalues(((x + 2.0 * y) + 3.0 * z).astype(np.float32), k)
    assert tuple(e[:, 0, 2, 2]) == (0.0, 0.0, 1.0) and tuple(e[:, X - 1, 2, 2]) == (0.0, 0.0, -1.0) and tuple(e[:, 3, 0, 2]) == (0.0, 0.0, 2.0)
    assert tuple(e[:, 3, 2, Z - 1]) == (0.0, 0.0, -3.0) and tuple(e[:, 0, Y - 1, 2]) == (0.0, 1.0, -2.0) and tuple(e[:, 0, 0, 0]) == (1.0, 2.0, 3.0)
    # x y on the edge x = y = 0: both second differences are (0 + 0) - 0 and the mixed one keeps one term of four, (1 - 0) - (0 - 0) = 1, times 1 / 4
    e = VO.eigenvalues((x * y).astype(np.float32), k)
    assert tuple(e[:, 0, 0, 2]) == (0.0, -0.25, 0.25)
    # a constant gives response 0 and scale 0 at every scale; x^2 + y^2 + z^2 is a dark blob: no bright tube, and RB = 1 keeps the dark response low
    dens = VO.denominators()
    assert (VO.response(np.full(shape, 7.0, np.float32), k, dens) == 0).all()
    assert (VO.response(((x * x + y * y) + z * z).astype(np.float32), k, dens)[inner] == 0).all()


def test_nonfinite_voxels_touch_their_19_neighbours():
    a = VO.noise_volume((9, 8, 7), 2)
    a[4, 4, 3] = np.nan
    a[1, 6, 5] = np.inf
    k = VO.hessian_factors(1.5, (0.8, 0.8, 2.0))
    e = VO.eigenvalues(a, k)
    want = np.zeros(a.shape, bool)
    for cx, cy, cz in ((4, 4, 3), (1, 6, 5)):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    if abs(dx) + abs(dy) + abs(dz) <= 2:
                        want[cx + dx, cy + dy, cz + dz] = True
    assert np.array_equal(np.isnan(e[0]), want) and np.array_equal(np.isnan(e[1]), want) and np.array_equal(np.isnan(e[2]), want)
    assert (e.view(np.uint32)[:, want] == VO.QNAN_BITS).all()
    r = VO.response(a, k, VO.denominators())
    assert (r[want] == 0).all() and np.isfinite(r).all()


def test_multi_scale_keeps_the_first_maximum():
    r = [np.array([0.0, 0.5, 0.5, 0.2, 0.0], np.float32), np.array([0.0, 0.5, 0.7, 0.1, 0.3], np.float32), np.array([0.0, 0.5, 0.7, 0.2, 0.3], np.float32)]
    best, scale = VO.multi_scale(r)
    assert best.tolist() == [0.0, 0.5, np.float32(0.7), np.float32(0.2), np.float32(0.3)] and scale.tolist() == [0, 1, 2, 1, 2] and scale.dtype == np.uint8


def test_bright_and_dark_are_mirror_images():
    a = VO.noise_volume((12, 9, 8), 4)
    k, dens = VO.hessian_factors(1.0, (0.8, 0.8, 2.0)), VO.denominators()
    b = VO.response(a, k, dens, True)
    assert (b > 0).any() and np.array_equal(VO.response(-a, k, dens, False).view(np.uint32), b.view(np.uint32))


def test_the_definition_does_its_job_on_the_phantom():
    """The oracle alone, at the defaults, on the phantom of vessel_oracle.phantom (48^3 voxels of 0.8 x 0.8 x 2.0 mm, noise 35 HU): conditions on the DEFINITION, not
    tolerances on a kernel.  The oracle's own figures: 0.998 of the tube's 500 voxels are in the mask (at least 0.9 asked), 0.0 of the plate's 6912 (at most 0.01), 0.0 of
    the ball's 400 (at most 0.1) and no voxel elsewhere.  Before the opening 0.88 of the ball's voxels are candidates, with a median response of 0.67 against the tube's
    0.58: a threshold alone cannot separate them.  What the opening leaves of a ball depends on where its centre falls on so coarse a grid (2 mm slices against a 3 mm
    ball): from 0.02 of its voxels, centred between voxel centres as here, to 0.16 centred on one -- the phantom takes the former."""
    ph = VO.phantom()
    assert ph["hu"].shape == (48, 48, 48) and ph["pixdim"] == (0.8, 0.8, 2.0)
    r = VO.vessel_mask(LO.decode(ph["hu"]), ph["lungs"], ph["pixdim"])
    m = r["mask"] != 0
    share = {k: float((m & ph[k]).sum()) / float(ph[k].sum()) for k in ("tube", "plate", "ball")}
    elsewhere = int((m & ~(ph["tube"] | ph["plate"] | ph["ball"])).sum())
    cand = r["response"] >= np.float32(0.3)
    print(f"phantom: in the mask {share}, elsewhere {elsewhere}; candidates in the ball {float((cand & ph['ball']).sum()) / float(ph['ball'].sum()):.3f}, median response tube "
          f"{float(np.median(r['response'][ph['tube']])):.3f} ball {float(np.median(r['response'][ph['ball']])):.3f}")
    assert share["tube"] >= 0.9
    assert share["plate"] <= 0.01
    assert share["ball"] <= 0.1
    assert elsewhere == 0
    assert float((cand & ph["ball"]).sum()) / float(ph["ball"].sum()) > 0.5          # (the reason for the opening exists in this phantom)


# ---- the Python surface without a device ------------------------------------------------------------------------------------------------------------------------------
def test_factors_and_denominators_restate_each_other():
    from covidseg_amd import vessels as VS
    for s, p in ((1.0, (1.0, 1.0, 1.0)), (2.5, (0.8, 0.8, 2.0)), (0.7, (0.683, 0.683, 1.25))):
        assert VS.hessian_factors(s, p).tolist() == VO.hessian_factors(s, p)
    assert VS.denominators(0.5, 0.5, 100.0) == VO.denominators(0.5, 0.5, 100.0) == (0.5, 0.5, 20000.0)
    assert VS.denominators(0.3, 0.7, 55.5) == VO.denominators(0.3, 0.7, 55.5)


def test_the_oracle_states_the_kernels_constants():
    src = open(os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc", "kernels_vessel.hip")).read()
    m = re.search(r"INV_LN2 = (\S+), LN2_HI = (\S+), LN2_LO = (\S+);", src)
    assert [float.fromhex(v) for v in m.groups()] == [VO.INV_LN2, VO.LN2_HI, VO.LN2_LO]
    c = re.search(r"constexpr double C\[14\] = \{([^}]+)\}", src).group(1)
    assert [float.fromhex(v.strip()) if "x" in v else float(v) for v in c.split(",")] == list(VO.EXP_C)
    assert int(re.search(r"constexpr int SWEEPS = (\d+);", src).group(1)) == VO.SWEEPS
    assert int(re.search(r"QNAN_BITS = (0x[0-9A-Fa-f]+)u;", src).group(1), 16) == VO.QNAN_BITS
    import math
    assert all(VO.EXP_C[n] == 1.0 / math.factorial(n) for n in range(14))


def test_the_kernels_arithmetic_on_the_cpu_equals_the_oracle(tmp_path):
    """tools/vessel_host_check.hip runs the kernel file's own per-voxel functions (__host__ __device__) behind a host copy of its brick walk: eigenvalues and response
    equal the oracle bit for bit, NaN positions included, without a GPU.  (The device is held to the same oracle by tests/test_gpu_vessels.py.)"""
    exe = str(tmp_path / "vessel_host_check")
    csrc = os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I", csrc,
                    os.path.join(ROOT, "tools", "vessel_host_check.hip"), "-o", exe], check=True, cwd=str(tmp_path))
    ph = VO.phantom()
    cases = [(VO.noise_volume((33, 9, 9), 1), (1.0, 1.0, 1.0), 1.5, True), (VO.noise_volume((70, 19, 17), 2), (0.8, 0.8, 2.0), 2.0, False),
             (VO.noise_volume((2, 1, 3), 4), (1.0, 1.0, 1.0), 1.0, True), (VO.noise_volume((40, 30, 20), 5, 1e-3), (0.7, 0.7, 1.25), 1.0, True),
             (VO.noise_volume((40, 30, 20), 6, 1e6), (0.7, 0.7, 1.25), 3.0, True), (VO.smoothed(ph["hu"].astype(np.float32), ph["pixdim"], 2.0), ph["pixdim"], 2.0, True)]
    dens = VO.denominators()
    for a, pixdim, sigma, bright in cases:
        if a.size > 1000:
            a = a.copy(); a[5, 4, 3] = np.nan; a[20, 6, 7] = -np.inf
        k = VO.hessian_factors(sigma, pixdim)
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.ascontiguousarray(a.reshape(-1, order="F")).tobytes()); f.write(np.array(list(k) + list(dens), np.float64).tobytes())
        subprocess.run([exe, *(str(n) for n in a.shape), str(tmp_path / "in.bin"), "1" if bright else "0", str(tmp_path / "out.bin")], check=True)
        got = np.stack([v.reshape(a.shape, order="F") for v in np.fromfile(tmp_path / "out.bin", np.float32).reshape(4, a.size)])
        want = np.concatenate([VO.eigenvalues(a, k), VO.response(a, k, dens, bright)[None]])
        assert np.array_equal(np.isnan(got), np.isnan(want)), (a.shape, sigma)
        ok = ~np.isnan(want)
        assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]), (a.shape, sigma)
        assert a.size < 100 or (got[3] > 0).any()


def test_argument_errors_need_no_device():
    from covidseg_amd import vessels as VS
    from covidseg_amd import volume as V
    ct = np.zeros((6, 5, 4), np.int16)
    p = (0.8, 0.8, 2.0)
    lungs = np.ones((6, 5, 4), np.uint8)
    bad = [
        lambda: VS.hessian_eigenvalues(ct, 0.0, pixdim=p),                                  # sigma = 0 is refused
        lambda: VS.hessian_eigenvalues(ct, -1.0, pixdim=p),
        lambda: VS.hessian_eigenvalues(ct, np.nan, pixdim=p),
        lambda: VS.hessian_eigenvalues(ct, "1", pixdim=p),
        lambda: VS.hessian_eigenvalues(ct, True, pixdim=p),
        lambda: VS.hessian_eigenvalues(ct, 1.0),                                            # an array carries no voxel size
        lambda: VS.hessian_eigenvalues(ct, 9.0, pixdim=p),                                  # ceil(3 * 9 / 0.8) = 34 taps > 32
        lambda: VS.hessian_eigenvalues(ct, 1.0, pixdim=(0.8, 0.0, 2.0)),
        lambda: VS.hessian_eigenvalues(ct, 1.0, pixdim=p, region=np.ones((6, 5, 3), np.uint8)),
        lambda: VS.hessian_eigenvalues(ct, 1.0, pixdim=p, region=np.ones((6, 5, 4), np.float32)),
        lambda: VS.hessian_eigenvalues(ct, 1.0, pixdim=p, return_device=1),
        lambda: VS.hessian_eigenvalues(ct, 1.0, pixdim=p, src_shape=(6, 5, 4)),            # src_shape describes a device tensor
        lambda: VS.hessian_eigenvalues(ct.astype(np.float64), 1.0, pixdim=p),               # float64 sources are not filtered
        lambda: VS.hessian_eigenvalues(np.zeros((0, 5, 4), np.int16), 1.0, pixdim=p),
        lambda: VS.vesselness(ct, pixdim=None),
        lambda: VS.vesselness(ct, sigmas_mm=(), pixdim=p),
        lambda: VS.vesselness(ct, sigmas_mm=1.0, pixdim=p),
        lambda: VS.vesselness(ct, sigmas_mm=(2.0, 1.0), pixdim=p),
        lambda: VS.vesselness(ct, sigmas_mm=(1.0, 1.0), pixdim=p),
        lambda: VS.vesselness(ct, sigmas_mm=(0.0, 1.0), pixdim=p),
        lambda: VS.vesselness(ct, sigmas_mm=(1.0, 9.0), pixdim=p),
        lambda: VS.vesselness(ct, sigmas_mm=tuple(0.01 * (i + 1) for i in range(255)), pixdim=p),          # at most 254 scales
        lambda: VS.vesselness(ct, alpha=0.0, pixdim=p),
        lambda: VS.vesselness(ct, beta=-0.5, pixdim=p),
        lambda: VS.vesselness(ct, c=np.inf, pixdim=p),
        lambda: VS.vesselness(ct, c=1e200, pixdim=p),                                       # 2 c^2 overflows
        lambda: VS.vesselness(ct, bright=1, pixdim=p),
        lambda: VS.vesselness(ct, region=np.ones((5, 5, 4), np.uint8), pixdim=p),
        lambda: VS.vessel_mask(ct, lungs),
        lambda: VS.vessel_mask(ct, np.ones((6, 5, 5), np.uint8), pixdim=p),
        lambda: VS.vessel_mask(ct, lungs.astype(np.float32), pixdim=p),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, threshold=0.0),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, threshold=1.5),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, dense_hu=np.nan),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, max_radius_mm=-1.0),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, erode_mm=np.inf),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, min_ml=-0.1),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, connectivity=4),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, sigmas_mm=(3.0, 2.0)),
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, gamma=1.0),                            # no such keyword
        lambda: VS.vessel_mask(ct, lungs, pixdim=p, return_device="yes"),
        lambda: V.segment_volume(ct, None, vessels=True),                                   # needs a lung mask
        lambda: V.segment_volume(ct, None, lung_mask=lungs, vessels="yes"),
        lambda: V.segment_volume(ct, None, lung_mask=lungs, vessels=dict(radius=3.0)),
        lambda: V.segment_volume(ct, None, lung_mask=lungs, vessels=dict(threshold=2.0)),
        lambda: V.segment_volume(ct, None, lungs=True, vessels=dict(sigmas_mm=(2.0, 1.0))),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} raised nothing")
    assert VS._check_sigmas((1.0, 2, np.float32(3.0)), p) == (1.0, 2.0, 3.0)
    assert V._check_vessels(None, None) is None and V._check_vessels(False, None) is None and V._check_vessels(True, lungs) == {}
    assert V._check_vessels(dict(threshold=0.4, sigmas_mm=(1.0,)), True) == dict(threshold=0.4, sigmas_mm=(1.0,))


def test_the_package_exports_the_surface():
    import covidseg_amd
    from covidseg_amd import vessels as VS
    for name in ("hessian_eigenvalues", "vesselness", "vessel_mask", "Vesselness", "VesselMask"):
        assert name in covidseg_amd.__all__ and getattr(covidseg_amd, name) is getattr(VS, name)
    assert "vessels" in covidseg_amd.__all__

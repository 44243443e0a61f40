"""numpy restatement of csrc/kernels_vessel.hip and vessels.py (TEST INFRASTRUCTURE ONLY), operation for operation in float64: the scale-normalised Hessian of a smoothed
volume from 19 samples, its eigenvalues by cyclic Jacobi, the library's own exp(-u), Frangi's tube measure, the best scale, and vessel_mask over morph_oracle /
lungmask_oracle / components_oracle with the Gaussian of filter_oracle.  tests/test_vessel_host.py holds it to np.linalg.eigvalsh, np.exp and a phantom on the CPU;
tests/test_gpu_vessels.py holds the device to it for equality.

    hessian(L32, k)                     the six entries, float64 [X, Y, Z] each; k = hessian_factors(sigma, pixdim)
    jacobi(a00, a11, a22, a01, a02, a12)   the diagonal after five sweeps of the pairs (0,1), (0,2), (1,2)
    eigenvalues(L32, k, region)         float32 [3, X, Y, Z], |l1| <= |l2| <= |l3|; NaN where an entry is not finite, +0.0 outside the region
    response(L32, k, dens, bright, region)   float32 [X, Y, Z]
    vesselness(ct32, pixdim, sigmas_mm, ...)   (best float32, scale uint8)
    vessel_mask(values, ct32, lungs, pixdim, ...)   dict(mask, response, scale, region)"""
import numpy as np

import components_oracle as CO
import filter_oracle as FO
import lungmask_oracle as LO
import morph_oracle as MO

SWEEPS = 5
INV_LN2, LN2_HI, LN2_LO = float.fromhex("0x1.71547652b82fep+0"), float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33")
# the doubles nearest 1 / n!, n = 0 .. 13
EXP_C = tuple(float.fromhex(h) for h in ("0x1.0p+0", "0x1.0p+0", "0x1.0000000000000p-1", "0x1.5555555555555p-3", "0x1.5555555555555p-5", "0x1.1111111111111p-7",
                                         "0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-13", "0x1.a01a01a01a01ap-16", "0x1.71de3a556c734p-19", "0x1.27e4fb7789f5cp-22",
                                         "0x1.ae64567f544e4p-26", "0x1.1eed8eff8d898p-29", "0x1.6124613a86d09p-33"))
QNAN_BITS = 0x7FC00000


def hessian_factors(sigma_mm, pixdim):
    """kxx, kyy, kzz = sigma^2 / h^2; kxy, kxz, kyz = sigma^2 / ((4 h_a) h_b), float64"""
    s = np.float64(sigma_mm)
    hx, hy, hz = (np.float64(v) for v in pixdim)
    s2 = s * s
    return [float(v) for v in (s2 / (hx * hx), s2 / (hy * hy), s2 / (hz * hz), s2 / ((4.0 * hx) * hy), s2 / ((4.0 * hx) * hz), s2 / ((4.0 * hy) * hz))]


def denominators(alpha=0.5, beta=0.5, c=100.0):
    """2 alpha^2, 2 beta^2, 2 c^2 as 2 (v v), float64"""
    return tuple(float(2.0 * (np.float64(v) * np.float64(v))) for v in (alpha, beta, c))


def hessian(L32, k):
    """the edge voxel repeats outside; every operation float64 and rounded on its own"""
    L = np.asarray(L32, np.float32)
    X, Y, Z = L.shape
    P = np.pad(L.astype(np.float64), 1, mode="edge")

    def at(dx, dy, dz):
        return P[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]

    with np.errstate(all="ignore"):
        two = 2.0 * at(0, 0, 0)
        a00 = ((at(1, 0, 0) + at(-1, 0, 0)) - two) * k[0]
        a11 = ((at(0, 1, 0) + at(0, -1, 0)) - two) * k[1]
        a22 = ((at(0, 0, 1) + at(0, 0, -1)) - two) * k[2]
        a01 = ((at(1, 1, 0) - at(1, -1, 0)) - (at(-1, 1, 0) - at(-1, -1, 0))) * k[3]
        a02 = ((at(1, 0, 1) - at(1, 0, -1)) - (at(-1, 0, 1) - at(-1, 0, -1))) * k[4]
        a12 = ((at(0, 1, 1) - at(0, 1, -1)) - (at(0, -1, 1) - at(0, -1, -1))) * k[5]
    return a00, a11, a22, a01, a02, a12


def _rotate(app, aqq, apq, arp, arq):
    """one rotation of the pair (p, q), r the third index, where apq != 0 -> the five entries after it"""
    m = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * np.where(m, apq, 1.0))
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        tau = s / (1.0 + c)
        h = t * apq
        npp, nqq = app - h, aqq + h
        nrp = arp - s * (arq + tau * arp)
        nrq = arq + s * (arp - tau * arq)
    return np.where(m, npp, app), np.where(m, nqq, aqq), np.where(m, 0.0, apq), np.where(m, nrp, arp), np.where(m, nrq, arq)


def jacobi(a00, a11, a22, a01, a02, a12, sweeps=SWEEPS):
    """-> the diagonal (d0, d1, d2) after `sweeps` sweeps (a rotation whose pivot is 0 is skipped, so further sweeps of a diagonal matrix change nothing)"""
    a00, a11, a22, a01, a02, a12 = (np.array(v, np.float64) for v in (a00, a11, a22, a01, a02, a12))
    for _ in range(sweeps):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12)          # (0, 1), r = 2
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12)          # (0, 2), r = 1
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02)          # (1, 2), r = 0
    return a00, a11, a22


def sort_by_magnitude(d0, d1, d2):
    """stable: the exchanges (1,2), (2,3), (1,2), each on strictly greater magnitude only"""
    def exchange(a, b):
        with np.errstate(invalid="ignore"):
            sw = np.abs(a) > np.abs(b)
        return np.where(sw, b, a), np.where(sw, a, b)
    d0, d1 = exchange(d0, d1)
    d1, d2 = exchange(d1, d2)
    d0, d1 = exchange(d0, d1)
    return d0, d1, d2


def exp_neg(u):
    """the library's exp(-u), u >= 0: clamp to 745 (a NaN counts as the clamp), k = rint(u / ln 2), two-constant reduction, degree-13 Taylor in Horner form, ldexp"""
    u = np.asarray(u, np.float64)
    with np.errstate(all="ignore"):
        u = np.where(u < 745.0, u, 745.0)
        k = np.rint(u * INV_LN2)
        r = -((u - k * LN2_HI) - k * LN2_LO)
        p = np.full(u.shape, EXP_C[13])
        for n in range(12, -1, -1):
            p = p * r + EXP_C[n]
        return np.ldexp(p, -k.astype(np.int32))


def frangi(l1, l2, l3, dens, bright=True):
    """-> float32; 0 unless l2 < 0 and l3 < 0 (dark: > 0)"""
    with np.errstate(all="ignore"):
        ok = ((l2 < 0.0) & (l3 < 0.0)) if bright else ((l2 > 0.0) & (l3 > 0.0))
        m1, m2, m3 = np.abs(l1), np.abs(l2), np.abs(l3)
        ra = m2 / m3
        rb = m1 / np.sqrt(m2 * m3)
        s2 = (l1 * l1 + l2 * l2) + l3 * l3
        v = ((1.0 - exp_neg((ra * ra) / dens[0])) * exp_neg((rb * rb) / dens[1])) * (1.0 - exp_neg(s2 / dens[2]))
        return np.where(ok, v, 0.0).astype(np.float32)


def _sorted_eigenvalues(L32, k):
    H = hessian(L32, k)
    finite = np.ones(H[0].shape, bool)
    for a in H:
        finite &= np.isfinite(a)
    H = [np.where(finite, a, 0.0) for a in H]                        # (a voxel that is not finite takes no part; its slots are filled below)
    return sort_by_magnitude(*jacobi(*H)), finite


def eigenvalues(L32, k, region=None):
    (l1, l2, l3), finite = _sorted_eigenvalues(L32, k)
    out = np.stack([l.astype(np.float32) for l in (l1, l2, l3)])
    out[:, ~finite] = np.array([QNAN_BITS], np.uint32).view(np.float32)[0]
    if region is not None:
        out[:, np.asarray(region) == 0] = np.float32(0.0)
    return out


def response(L32, k, dens, bright=True, region=None):
    (l1, l2, l3), finite = _sorted_eigenvalues(L32, k)
    v = frangi(l1, l2, l3, dens, bright)
    v[~finite] = np.float32(0.0)
    if region is not None:
        v[np.asarray(region) == 0] = np.float32(0.0)
    return v


def multi_scale(responses):
    """-> (best float32, scale uint8): the first scale initialises, a later one replaces on strictly greater only; scale 0 where best == 0"""
    best = np.array(responses[0], np.float32)
    scale = (best > 0).astype(np.uint8)
    for i, v in enumerate(responses[1:], 1):
        up = v > best
        best = np.where(up, v, best)
        scale = np.where(up, np.uint8(i + 1), scale).astype(np.uint8)
    return best, scale


def smoothed(ct32, pixdim, sigma_mm):
    """filters.gaussian_filter(sigma_mm=): the width in voxels is sigma_mm / pixdim per axis"""
    return FO.gaussian_filter(ct32, [float(np.float64(sigma_mm) / np.float64(h)) for h in pixdim])


def hessian_eigenvalues(ct32, pixdim, sigma_mm, region=None):
    return eigenvalues(smoothed(ct32, pixdim, sigma_mm), hessian_factors(sigma_mm, pixdim), region)


def vesselness(ct32, pixdim, sigmas_mm=(1.0, 2.0, 3.0), alpha=0.5, beta=0.5, c=100.0, bright=True, region=None):
    dens = denominators(alpha, beta, c)
    return multi_scale([response(smoothed(ct32, pixdim, s), hessian_factors(s, pixdim), dens, bright, region) for s in sigmas_mm])


def vessel_mask(values, lungs, pixdim, threshold=0.3, dense_hu=-500.0, max_radius_mm=3.0, min_ml=0.01, connectivity=3, erode_mm=2.0, **kw):
    """values: what get_fdata gives (float64).  region = erode_mm(lungs != 0); candidates = (response >= threshold) & dense & region, without open_mm(dense,
    max_radius_mm), without the components under min_ml"""
    values = np.asarray(values, np.float64)
    region = MO.erode_mm(np.asarray(lungs) != 0, erode_mm, pixdim)
    best, scale = vesselness(values.astype(np.float32), pixdim, region=region, **kw)
    dense = LO.threshold(values, dense_hu, None)[0]
    cand = LO.threshold(best, threshold, None, LO.threshold(values, dense_hu, None, region)[0])[0]
    thick = MO.open_mm(dense, max_radius_mm, pixdim)
    cand = LO.threshold(thick, None, 1.0, cand)[0]                    # candidates & ~thick
    mask = CO.remove_small(cand, CO.min_voxels_from_ml(min_ml, pixdim), connectivity)
    return dict(mask=mask, response=best, scale=scale, region=region, thick=thick)


# ---- test volumes ---------------------------------------------------------------------------------------------------------------------------------------------------
PHANTOM_SHAPE, PHANTOM_PIXDIM = (48, 48, 48), (0.8, 0.8, 2.0)


def phantom(seed=11, shape=PHANTOM_SHAPE, pixdim=PHANTOM_PIXDIM, noise=35.0):
    """Lung-like -850 HU with Gaussian noise of sigma = 35 HU from a fixed seed, 48^3 voxels of 0.8 x 0.8 x 2.0 mm (38.4 x 38.4 x 96 mm), as int16 HU, with three objects
    of +40 HU laid out in millimetres -> dict(hu, lungs, tube, ball, plate, pixdim): one oblique tube of radius 2 mm, one ball of radius 5 mm, and one plate 2 mm thick
    that crosses the whole volume as a fissure does (it has no rim inside the lungs).  lungs: the volume without a margin of 3 voxels."""
    X, Y, Z = shape
    px, py, pz = pixdim
    g = np.meshgrid(np.arange(X) * px, np.arange(Y) * py, np.arange(Z) * pz, indexing="ij")
    P = np.stack(g, -1)
    x, y, z = g
    tube = LO._tube(P, (8.0, 9.0, 14.0), (18.0, 15.0, 62.0), 2.0, 2.0)
    ball = (x - 12.4) ** 2 + (y - 27.6) ** 2 + (z - 79.0) ** 2 <= 25.0                           # (centred between voxel centres on every axis)
    plate = np.abs(x - 30.4) <= 1.0
    hu = np.full(tuple(shape), -850.0)
    hu[tube | ball | plate] = 40.0
    hu = np.rint(hu + np.random.default_rng(seed).normal(0.0, float(noise), tuple(shape))).astype(np.int16)
    lungs = np.zeros(tuple(shape), np.uint8)
    lungs[3:-3, 3:-3, 3:-3] = 1
    return dict(hu=np.asfortranarray(hu), lungs=lungs, tube=tube, ball=ball, plate=plate, pixdim=tuple(pixdim))


def noise_volume(shape, seed, scale=300.0):
    return np.asfortranarray((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))

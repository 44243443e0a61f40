// Vesselness of a CT: the eigenvalues of the scale-normalised Hessian of the smoothed volume and Frangi's tube measure over them, per voxel
//                                                                                                                                  unet_vol_hessian_eig, unet_vol_vesselness
// The definition is include/unet_hip.h's; tests/vessel_oracle.py restates it in numpy operation for operation and the device is held to it for equality.  All arithmetic
// is float64 and every operation is rounded on its own (-ffp-contract=off); only + - * /, the correctly rounded square root, rint and ldexp are used, so both sides give
// the same bits: the eigenvalues come from cyclic Jacobi and not from a closed form with acos / cos, and exp(-u) is the file's own (vs_exp_neg), not the device library's.
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31.  Persistent workgroups of 256 lanes walk bricks of 32 x 8 x 8 voxels, x fastest.  A brick is
// staged in LDS as float32 with a halo of 1, the edge voxel repeating outside the volume while staging: 34 x 10 x 10 x 4 B = 13.3 KiB, and the 19 samples of a voxel know
// no border.  The 32 lanes of a half-wave read 32 consecutive floats of one staged row: no bank conflict.  With a region, a brick none of whose voxels takes part is left
// before it is staged: the vote is __syncthreads_or, uniform over the workgroup, as every branch and loop bound that holds a barrier must be.  The Jacobi sweeps hold no
// barrier, so a lane ends them as soon as its three off-diagonals are exactly 0 (skipping a rotation whose pivot is 0 gives the same bits as running to the fifth sweep).
// One launch per scale, no atomics, no workgroup waits for another, every output element written by one lane: the same bits on every run.
#include "common.h"
#include "vol_common.h"

namespace {
constexpr int TPB = 256;
constexpr int BX = 32, BY = 8, BZ = 8, BRICK = BX * BY * BZ;         // the brick a workgroup takes at a time: 8 voxels per lane
constexpr int SX = BX + 2, SY = BY + 2, SZ = BZ + 2, S = SX * SY * SZ;          // staged with a halo of 1: 3400 floats
constexpr long long GRID_CAP = 256 * 8;                              // persistent workgroups of a launch: up to 8 per CU (13.3 KiB of LDS each; the registers decide how many are resident)
constexpr int SWEEPS = 5;
constexpr uint32_t QNAN_BITS = 0x7FC00000u;                          // the canonical quiet NaN (float32) of a voxel whose Hessian is not finite

struct vs_params {
  double kxx, kyy, kzz, kxy, kxz, kyz;                               // sigma^2 / h_a^2 and sigma^2 / (4 h_a h_b), computed once on the host
  double den_a, den_b, den_c;                                        // 2 alpha^2, 2 beta^2, 2 c^2
  int bright, index;
};

// the correctly rounded square root (the host side exists for tools/vessel_host_check.hip, which runs the very same arithmetic on the CPU: the per-voxel functions below
// are __host__ __device__)
__host__ __device__ __forceinline__ double vs_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return __builtin_sqrt(x);
#endif
}

// exp(-u) for u >= 0 (a NaN counts as the clamp): k = rint(u / ln 2), r = -((u - k LN2_HI) - k LN2_LO) in [-ln 2 / 2, ln 2 / 2] (k LN2_HI is exact: LN2_HI ends in 21 zero
// bits and k <= 1075), the Taylor polynomial of degree 13 in Horner form (truncation 4e-18 of the result), scaled by 2^-k.
__host__ __device__ __forceinline__ double vs_exp_neg(double u) {
  constexpr double INV_LN2 = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
  constexpr double C[14] = {1.0, 1.0, 0x1.0000000000000p-1, 0x1.5555555555555p-3, 0x1.5555555555555p-5, 0x1.1111111111111p-7, 0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-13,
                            0x1.a01a01a01a01ap-16, 0x1.71de3a556c734p-19, 0x1.27e4fb7789f5cp-22, 0x1.ae64567f544e4p-26, 0x1.1eed8eff8d898p-29, 0x1.6124613a86d09p-33};          // 1 / n!
  u = u < 745.0 ? u : 745.0;
  const double k = rint(u * INV_LN2);
  const double r = -((u - k * LN2_HI) - k * LN2_LO);
  double p = C[13];
#pragma unroll
  for (int n = 12; n >= 0; --n) p = p * r + C[n];
  return ldexp(p, -(int)k);
}

// one rotation of the pair (p, q); r is the third index.  theta^2 may overflow: then sqrt gives +inf, t = +-0, c = 1, s = +-0 and the pivot is dropped -- no special case.
__host__ __device__ __forceinline__ void vs_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + vs_sqrt(theta * theta + 1.0));
  const double c = 1.0 / vs_sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  const double rp = arp, rq = arq;
  arp = rp - s * (rq + tau * rp);
  arq = rq + s * (rp - tau * rq);
  apq = 0.0;
}

// The eigenvalues of the Hessian at the staged sample c, sorted by magnitude -> whether all six entries are finite (otherwise l1, l2, l3 are not set)
__host__ __device__ __forceinline__ bool vs_eigenvalues(const float* s_l, int c, const vs_params& P, double& l1, double& l2, double& l3) {
  constexpr int DX = 1, DY = SX, DZ = SX * SY;
  const double two = 2.0 * (double)s_l[c];
  double a00 = (((double)s_l[c + DX] + (double)s_l[c - DX]) - two) * P.kxx;
  double a11 = (((double)s_l[c + DY] + (double)s_l[c - DY]) - two) * P.kyy;
  double a22 = (((double)s_l[c + DZ] + (double)s_l[c - DZ]) - two) * P.kzz;
  double a01 = (((double)s_l[c + DX + DY] - (double)s_l[c + DX - DY]) - ((double)s_l[c - DX + DY] - (double)s_l[c - DX - DY])) * P.kxy;
  double a02 = (((double)s_l[c + DX + DZ] - (double)s_l[c + DX - DZ]) - ((double)s_l[c - DX + DZ] - (double)s_l[c - DX - DZ])) * P.kxz;
  double a12 = (((double)s_l[c + DY + DZ] - (double)s_l[c + DY - DZ]) - ((double)s_l[c - DY + DZ] - (double)s_l[c - DY - DZ])) * P.kyz;
  const double big = __builtin_inf();                                 // finite: |a| < inf, which a NaN fails too
  if (!(fabs(a00) < big && fabs(a11) < big && fabs(a22) < big && fabs(a01) < big && fabs(a02) < big && fabs(a12) < big)) return false;
#pragma unroll 1
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    vs_rotate(a00, a11, a01, a02, a12);                               // (0, 1), r = 2
    vs_rotate(a00, a22, a02, a01, a12);                               // (0, 2), r = 1
    vs_rotate(a11, a22, a12, a01, a02);                               // (1, 2), r = 0
  }
  double tmp;                                                         // stable by magnitude: adjacent exchanges on strictly greater only
  l1 = a00; l2 = a11; l3 = a22;
  if (fabs(l1) > fabs(l2)) { tmp = l1; l1 = l2; l2 = tmp; }
  if (fabs(l2) > fabs(l3)) { tmp = l2; l2 = l3; l3 = tmp; }
  if (fabs(l1) > fabs(l2)) { tmp = l1; l1 = l2; l2 = tmp; }
  return true;
}

// Frangi's measure of sorted eigenvalues, rounded once to float32
__host__ __device__ __forceinline__ float vs_measure(double l1, double l2, double l3, const vs_params& P) {
  if (!(P.bright ? (l2 < 0.0 && l3 < 0.0) : (l2 > 0.0 && l3 > 0.0))) return 0.0f;
  const double m1 = fabs(l1), m2 = fabs(l2), m3 = fabs(l3);
  const double ra = m2 / m3, rb = m1 / vs_sqrt(m2 * m3), s2 = (l1 * l1 + l2 * l2) + l3 * l3;
  return (float)(((1.0 - vs_exp_neg((ra * ra) / P.den_a)) * vs_exp_neg((rb * rb) / P.den_b)) * (1.0 - vs_exp_neg(s2 / P.den_c)));
}

// EIG: the three eigenvalues leave (eig, three volumes one after the other); otherwise best / scale are read and updated in place.
// Every branch and loop bound that holds a barrier is uniform over the workgroup: the brick loop, the region vote and the staging loop.
template <bool EIG>
__global__ __launch_bounds__(TPB) void vs_kernel(const float* __restrict__ L, const uint8_t* __restrict__ region, int X, int Y, int Z, vs_params P, float* __restrict__ eig,
                                                 float* __restrict__ best, uint8_t* __restrict__ scale, long long nbricks, int nbx, int nby) {
  __shared__ float s_l[S];
  const int tid = threadIdx.x;
  const long long N = (long long)X * Y * Z;
  for (long long b = blockIdx.x; b < nbricks; b += gridDim.x) {
    const int bz = (int)(b / ((long long)nbx * nby)), br = (int)(b - (long long)bz * nbx * nby), by = br / nbx, bx = br - by * nbx;
    const int x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;
    if (region != nullptr) {
      int any = 0;
#pragma unroll
      for (int j = 0; j < BRICK / TPB; ++j) {
        const int l = tid + j * TPB, gx = x0 + (l & (BX - 1)), gy = y0 + ((l >> 5) & (BY - 1)), gz = z0 + (l >> 8);
        if (gx < X && gy < Y && gz < Z) any |= region[gx + (long long)X * (gy + (long long)Y * gz)] != 0 ? 1 : 0;
      }
      if (__syncthreads_or(any) == 0) {                               // nobody of this brick takes part: its outputs are the outside's, and nothing is staged
        if (EIG || P.index == 0) {
#pragma unroll
          for (int j = 0; j < BRICK / TPB; ++j) {
            const int l = tid + j * TPB, gx = x0 + (l & (BX - 1)), gy = y0 + ((l >> 5) & (BY - 1)), gz = z0 + (l >> 8);
            if (gx < X && gy < Y && gz < Z) {
              const long long f = gx + (long long)X * (gy + (long long)Y * gz);
              if constexpr (EIG) { eig[f] = 0.0f; eig[N + f] = 0.0f; eig[2 * N + f] = 0.0f; }
              else { best[f] = 0.0f; scale[f] = 0; }
            }
          }
        }
        continue;
      }
    }
    for (int i = tid; i < S; i += TPB) {                              // the brick and its halo, the edge voxel repeating (0 <= p < extent on every axis)
      const int sx = i % SX, t = i / SX, sy = t % SY, sz = t / SY;
      const long long px = min(max((long long)x0 + sx - 1, 0LL), (long long)X - 1), py = min(max((long long)y0 + sy - 1, 0LL), (long long)Y - 1),
                      pz = min(max((long long)z0 + sz - 1, 0LL), (long long)Z - 1);
      s_l[i] = L[px + X * (py + Y * pz)];
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < BRICK / TPB; ++j) {
      const int l = tid + j * TPB, lx = l & (BX - 1), ly = (l >> 5) & (BY - 1), lz = l >> 8;
      const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
      if (gx >= X || gy >= Y || gz >= Z) continue;                    // (no barrier inside this loop)
      const long long f = gx + (long long)X * (gy + (long long)Y * gz);
      if (region != nullptr && region[f] == 0) {
        if constexpr (EIG) { eig[f] = 0.0f; eig[N + f] = 0.0f; eig[2 * N + f] = 0.0f; }
        else if (P.index == 0) { best[f] = 0.0f; scale[f] = 0; }
        continue;
      }
      const int c = (lx + 1) + SX * ((ly + 1) + SY * (lz + 1));       // c +- 1, +- SX, +- SX SY stay inside the staged brick
      double l1, l2, l3;
      const bool finite = vs_eigenvalues(s_l, c, P, l1, l2, l3);
      float v = 0.0f;
      if constexpr (EIG) {
        const float qnan = __uint_as_float(QNAN_BITS);
        eig[f] = finite ? (float)l1 : qnan; eig[N + f] = finite ? (float)l2 : qnan; eig[2 * N + f] = finite ? (float)l3 : qnan;
      } else if (finite) {
        v = vs_measure(l1, l2, l3, P);
      }
      if constexpr (!EIG) {
        if (P.index == 0) { best[f] = v; scale[f] = v > 0.0f ? 1 : 0; }
        else if (v > best[f]) { best[f] = v; scale[f] = (uint8_t)(P.index + 1); }          // a later scale replaces on strictly greater only
      }
    }
    __syncthreads();                                                  // the staged brick was read: the next one may be written
  }
}

bool vs_factor_ok(double v) { return v > 0.0 && v < __builtin_inf(); }          // (a NaN fails the first comparison)

// the checks both entries share -> UNET_OK and N, or the refusal
int32_t vs_check(unet_ctx* ctx, const char* what, const float* L, int X, int Y, int Z, const double* k, long long* N) {
  if (!ctx) return UNET_E_ARG;
  if (X <= 0 || Y <= 0 || Z <= 0 || !vol_dims_ok(X, Y, Z))
    UNET_FAIL(ctx, UNET_E_ARG, "%s: an extent is <= 0 or the volume has 2^31 voxels or more", what);
  if (!L || !k || reinterpret_cast<uintptr_t>(L) % 4 != 0) UNET_FAIL(ctx, UNET_E_ARG, "%s: null volume or factors, or a volume not aligned to its element", what);
  for (int i = 0; i < 6; ++i)
    if (!vs_factor_ok(k[i])) UNET_FAIL(ctx, UNET_E_ARG, "%s: factor %d is not a finite positive number", what, i);
  *N = (long long)X * Y * Z;
  return UNET_OK;
}

template <bool EIG>
void vs_launch(hipStream_t s, const float* L, const uint8_t* region, int X, int Y, int Z, const vs_params& P, float* eig, float* best, uint8_t* scale) {
  const int nbx = (X + BX - 1) / BX, nby = (Y + BY - 1) / BY, nbz = (Z + BZ - 1) / BZ;
  const long long nbricks = (long long)nbx * nby * nbz;
  const unsigned grid = (unsigned)(nbricks < GRID_CAP ? nbricks : GRID_CAP);
  hipLaunchKernelGGL((vs_kernel<EIG>), dim3(grid), dim3(TPB), 0, s, L, region, X, Y, Z, P, eig, best, scale, nbricks, nbx, nby);
}
}  // namespace

extern "C" {

int32_t unet_vol_hessian_eig(unet_ctx* ctx, const float* L, int32_t X, int32_t Y, int32_t Z, const double* k, const uint8_t* region, float* eig, void* stream) {
  long long N = 0;
  const int32_t rc = vs_check(ctx, "vol_hessian_eig", L, X, Y, Z, k, &N);
  if (rc != UNET_OK) return rc;
  if (!eig || reinterpret_cast<uintptr_t>(eig) % 4 != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_hessian_eig: null output, or one not aligned to its element");
  if (vol_overlap(eig, (size_t)N * 12, L, (size_t)N * 4) || (region && vol_overlap(eig, (size_t)N * 12, region, (size_t)N)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_hessian_eig: the output overlaps the volume or the region (a voxel's neighbours must be read as they were)");
  vs_params P{k[0], k[1], k[2], k[3], k[4], k[5], 1.0, 1.0, 1.0, 1, 0};
  vs_launch<true>(as_stream(stream), L, region, X, Y, Z, P, eig, nullptr, nullptr);
  UNET_CHECK_LAUNCH(ctx, "vol_hessian_eig"); return UNET_OK;
}

int32_t unet_vol_vesselness(unet_ctx* ctx, const float* L, int32_t X, int32_t Y, int32_t Z, const double* k, const uint8_t* region, double den_a, double den_b, double den_c,
                            int32_t bright, int32_t index, float* best, uint8_t* scale, void* stream) {
  long long N = 0;
  const int32_t rc = vs_check(ctx, "vol_vesselness", L, X, Y, Z, k, &N);
  if (rc != UNET_OK) return rc;
  if (!vs_factor_ok(den_a) || !vs_factor_ok(den_b) || !vs_factor_ok(den_c))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_vesselness: a denominator (2 alpha^2, 2 beta^2, 2 c^2) is not a finite positive number");
  if (bright != 0 && bright != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_vesselness: bright is 0 or 1, not %d", bright);
  if (index < 0 || index > UNET_VOL_VESSEL_MAX_SCALES - 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_vesselness: the scale's index lies in 0 .. %d, not %d", UNET_VOL_VESSEL_MAX_SCALES - 1, index);
  if (!best || !scale || reinterpret_cast<uintptr_t>(best) % 4 != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_vesselness: null best or scale, or best not aligned to its element");
  if (vol_overlap(best, (size_t)N * 4, L, (size_t)N * 4) || vol_overlap(scale, (size_t)N, L, (size_t)N * 4) || vol_overlap(best, (size_t)N * 4, scale, (size_t)N) ||
      (region && (vol_overlap(best, (size_t)N * 4, region, (size_t)N) || vol_overlap(scale, (size_t)N, region, (size_t)N))))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_vesselness: best or scale overlaps the volume, the region or each other");
  vs_params P{k[0], k[1], k[2], k[3], k[4], k[5], den_a, den_b, den_c, bright, index};
  vs_launch<false>(as_stream(stream), L, region, X, Y, Z, P, nullptr, best, scale);
  UNET_CHECK_LAUNCH(ctx, "vol_vesselness"); return UNET_OK;
}

}  // extern "C"

// The similarity of two volumes under candidate transforms: the joint intensity histogram of a fixed volume and a moving volume sampled through
// K matrices at once                                                                                                                       unet_vol_joint_hist
// Both volumes are [X, Y, Z] in Fortran order, described and decoded as for unet_vol_resample_linear; M_c (12 doubles, row-major 3 x 4, in the kernel arguments) maps a
// fixed voxel index to a moving voxel coordinate in section 4w's convention.  A fixed voxel is counted for candidate c iff its mask byte is non-zero (or there is no
// mask), its decoded value is not NaN, every coordinate satisfies 0 <= s_r <= n_r - 1 as a double (a NaN or inf coordinate is outside, and nothing is converted to an
// integer before that test) and the moving sample -- vol_trilinear.h's rs_blend_inside: the float64 unet_vol_resample_linear writes there -- is not NaN.  Its cell is
// (bin_f(fixed value), bin_m(sample)), bin(v) = floor(fl(fl(v - lo) scale)) clamped to [0, B - 1] as a double first (+-inf clamp).  The counts are integers: the result
// does not depend on the order of accumulation, and every test is an equality.
//   jh_kernel    fixed x along the lanes (the fixed loads coalesce, the moving loads of a wave run along one line of the moving volume); a bounded grid strides the fixed
//                voxels, blockIdx.y is the candidate.  One B x B uint32 histogram per workgroup in LDS (16 KiB at B = 64), LDS integer atomics, and one pass of global
//                integer atomics over its non-zero bins at the end.  A CT puts most voxels into a few cells (air / air, tissue / tissue), so before the LDS atomic a
//                wave takes out its most likely collision: the lanes whose cell equals the first counted lane's are counted with one ballot and added by that lane
//                alone; the other lanes add 1 each.  A constant pair -- every voxel in one cell -- is then one LDS atomic per wave and step instead of 64 on one address.
// The trip count and the barriers are uniform over the workgroup; no floating-point atomics; vector stores and vector atomics only.
#include "common.h"
#include "vol_trilinear.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int MAX_K = UNET_VOL_JOINT_HIST_MAX_K, MAX_BINS = UNET_VOL_JOINT_HIST_MAX_BINS;
constexpr long long GRID_CAP = 1024;                                  // workgroups per candidate (x 16 candidates: 64 per CU)

struct jh_mats { rs_mat M[MAX_K]; };                                  // 1536 bytes of kernel arguments
struct jh_window { double lo, scale; };

__device__ __forceinline__ int jh_bin(double v, const jh_window& w, int B) {
  const double q = __dmul_rn(__dsub_rn(v, w.lo), w.scale);
  return !(q >= 0.0) ? 0 : (q >= (double)B ? B - 1 : (int)floor(q));
}

__global__ __launch_bounds__(TPB) void jh_kernel(vol_voxels fix, const uint8_t* __restrict__ mask, int X, int Y, int Z, vol_voxels mov, int Xm, int Ym, int Zm, jh_mats mats, int B,
                                                 jh_window wf, jh_window wm, uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[MAX_BINS * MAX_BINS];
  const int cells = B * B, lane = threadIdx.x & 63;
  for (int c = threadIdx.x; c < cells; c += TPB) hist[c] = 0;
  __syncthreads();
  const rs_mat& M = mats.M[blockIdx.y];
  const long long N = (long long)X * Y * Z;
  const double top[3] = {(double)(Xm - 1), (double)(Ym - 1), (double)(Zm - 1)};
  for (long long base = (long long)blockIdx.x * TPB; base < N; base += (long long)gridDim.x * TPB) {          // (base is workgroup-uniform)
    const long long o = base + threadIdx.x;
    bool ok = o < N && (!mask || mask[o] != 0);
    int cell = 0;
    if (ok) {
      const double fv = vol_dec(fix, o);
      const long long c = o / X;
      const int i = (int)(o - c * X), k = (int)(c / Y), j = (int)(c - (long long)k * Y);
      double s[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) s[r] = rs_coord(M, r, i, j, k);
      ok = fv == fv && s[0] >= 0.0 && s[0] <= top[0] && s[1] >= 0.0 && s[1] <= top[1] && s[2] >= 0.0 && s[2] <= top[2];
      if (ok) {
        const double mv = rs_blend_inside(mov, Xm, Ym, Zm, s);
        ok = mv == mv;
        cell = jh_bin(fv, wf, B) * B + jh_bin(mv, wm, B);
      }
    }
    const unsigned long long counted = __ballot(ok);
    if (counted) {                                                    // (wave-uniform)
      const int lead = __ffsll((long long)counted) - 1;
      const int lead_cell = __shfl(cell, lead, 64);
      const unsigned long long same = __ballot(ok && cell == lead_cell);
      if (lane == lead) atomicAdd(&hist[lead_cell], (uint32_t)__popcll(same));
      else if (ok && cell != lead_cell) atomicAdd(&hist[cell], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = counts + (size_t)blockIdx.y * cells;
  for (int c = threadIdx.x; c < cells; c += TPB) {
    const uint32_t v = hist[c];
    if (v) atomicAdd(out + c, v);
  }
}

inline bool jh_vol_ok(int X, int Y, int Z) { return rs_out_ok(X, Y, Z); }          // at least one voxel, fewer than 2^31
}  // namespace

extern "C" {

int32_t unet_vol_joint_hist(unet_ctx* ctx, const void* fixed, int32_t f_dtype, int32_t X, int32_t Y, int32_t Z, int32_t f_scaled, double f_slope, double f_inter,
                            const uint8_t* mask, const void* moving, int32_t m_dtype, int32_t Xm, int32_t Ym, int32_t Zm, int32_t m_scaled, double m_slope, double m_inter,
                            const double* M, int32_t K, int32_t bins, double f_lo, double f_hi, double m_lo, double m_hi, uint32_t* counts, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (K < 1 || K > MAX_K) UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: %d candidates, not 1 to %d", K, MAX_K);
  if (bins < 2 || bins > MAX_BINS) UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: %d bins, not 2 to %d", bins, MAX_BINS);
  if (!jh_vol_ok(X, Y, Z) || !jh_vol_ok(Xm, Ym, Zm)) UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: a volume of %d x %d x %d and one of %d x %d x %d (every extent is at least 1, fewer than 2^31 voxels)", X, Y, Z, Xm, Ym, Zm);
  if (vol_itemsize(f_dtype) == 0 || vol_itemsize(m_dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: a NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64");
  if (!std::isfinite(f_lo) || !std::isfinite(f_hi) || !std::isfinite(m_lo) || !std::isfinite(m_hi) || !(f_hi > f_lo) || !(m_hi > m_lo))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: a window is two finite numbers lo < hi");
  const jh_window wf{f_lo, (double)bins / (f_hi - f_lo)}, wm{m_lo, (double)bins / (m_hi - m_lo)};
  if (!(wf.scale > 0.0) || !(wm.scale > 0.0)) UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: hi - lo of a window overflows");
  if (!M) UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: M is K x 12 finite doubles");
  jh_mats mats{};
  for (int c = 0; c < K; ++c)
    for (int i = 0; i < 12; ++i) {
      if (!std::isfinite(M[12 * c + i])) UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: entry %d of matrix %d is not finite", i, c);
      mats.M[c].m[i] = M[12 * c + i];
    }
  if (!fixed || (reinterpret_cast<uintptr_t>(fixed) % vol_itemsize(f_dtype)) != 0 || !moving || (reinterpret_cast<uintptr_t>(moving) % vol_itemsize(m_dtype)) != 0 || !counts ||
      (reinterpret_cast<uintptr_t>(counts) % sizeof(uint32_t)) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_joint_hist: a null buffer, or one not aligned to its element size");
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)K * bins * bins * sizeof(uint32_t), s));
  const long long N = (long long)X * Y * Z, blocks = (N + TPB - 1) / TPB;
  const vol_voxels fs{fixed, f_dtype, f_scaled ? 1 : 0, f_slope, f_inter}, ms{moving, m_dtype, m_scaled ? 1 : 0, m_slope, m_inter};
  hipLaunchKernelGGL(jh_kernel, dim3((unsigned)(blocks > GRID_CAP ? GRID_CAP : blocks), (unsigned)K), dim3(TPB), 0, s, fs, mask, X, Y, Z, ms, Xm, Ym, Zm, mats, bins, wf, wm, counts);
  UNET_CHECK_LAUNCH(ctx, "vol_joint_hist"); return UNET_OK;
}

}  // extern "C"

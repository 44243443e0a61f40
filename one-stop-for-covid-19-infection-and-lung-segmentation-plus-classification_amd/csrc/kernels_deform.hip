// The deformable refinement of a registered follow-up: a dense displacement field u on a field grid, float32 [3][X Y Z], component major, each
// component a volume in Fortran order, in millimetres of the fixed world frame.
//   one pass of a normalised Gaussian along one axis of C float32 volumes                                            unet_vol_smooth_axis
//   one demons iteration's u + v (Thirion's additive force of the squared difference)                                unet_vol_demons_step
//   a volume, a mask or labels through the rigid matrix and the field onto a grid                                    unet_vol_warp_field
//   det(I + D inv(A)) of a field and the number of folded voxels                                                     unet_vol_jacobian
// A target voxel x looks at the moving voxel coordinate s_r = ((rs_coord(W, x)_r + L[r][0] u_0) + L[r][1] u_1) + L[r][2] u_2: W (3 x 4) is the rigid voxel matrix, L
// (3 x 3) takes a displacement in mm to moving voxels, u is the stored element (the target grid is the field grid) or the field sampled trilinearly at F x, clamped into
// the field.  Every float64 operation is a rounded one of its own (-ffp-contract=off and the __d*_rn forms), the field is rounded to float32 once on store: numpy restates
// all four kernels bit for bit (tests/deform_oracle.py).  The samplers are vol_trilinear.h's, so a field of zeros makes unet_vol_warp_field the resampling entries.
//   sm_x_kernel    axis 0: a wave owns 64 consecutive x of one row and stages them with a halo of R on either side in LDS (64 + 2R floats, 2 KiB per workgroup of four rows)
//                  -- every source element is loaded once instead of 2R + 1 times; the taps are ds_read_b32 at consecutive addresses (no bank conflict)
//   sm_yz_kernel   axes 1 and 2: x along the lanes, every tap one coalesced load a row (a plane) further on
//   dm_kernel      fixed x along the lanes; the 7-point stencil of f and the eight moving neighbours straight from memory, the warped image is never stored
//   wf_kernel      output x along the lanes (one mapping: the field is read along x whatever the rigid part does)
//   jc_kernel      x along the lanes; the folded voxels of a wave are counted with one ballot and added by one lane (an integer atomic)
// Trip counts and barriers are uniform over the workgroup; no floating-point atomics; vector stores and vector atomics only; volumes have fewer than 2^31 voxels.
#include "common.h"
#include "vol_trilinear.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int MAX_R = UNET_VOL_SMOOTH_MAX_RADIUS;
constexpr int SEG = 64, ROWS = TPB / 64;                              // sm_x_kernel: a wave per row segment
constexpr int MAX_C = 1024;
constexpr long long GRID_CAP = 256 * 32;
constexpr double DEN_MIN = 1e-9;                                      // a demons denominator (HU^2 / mm^2) at or below this moves nothing: no gradient and no difference

inline bool df_finite(const double* p, int n) {
  if (!p) return false;
  for (int i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
  return true;
}
inline bool df_aligned(const void* p, size_t a) { return p && vol_aligned(p, a); }          // (a null pointer is refused too: every buffer of these entries is required)

// ---- the Gaussian pass: out = fl32(sum_t w[t] src[clamp(p + t - R)]), t ascending, acc = acc + fl(w v) from acc = 0 ---------------------------------------------------
struct sm_weights { double w[2 * MAX_R + 1]; };                       // 520 bytes of kernel arguments

__global__ __launch_bounds__(TPB) void sm_x_kernel(const float* __restrict__ src, float* __restrict__ dst, int X, long long rows, int segs, long long tiles, int R, sm_weights wt) {
  __shared__ float line[ROWS][SEG + 2 * MAX_R];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {         // (workgroup-uniform)
    const int x0 = (int)(t % segs) * SEG;
    const long long row = (t / segs) * ROWS + w;
    if (row < rows) {
      const float* p = src + row * X;
      for (int e = lane; e < SEG + 2 * R; e += 64) line[w][e] = p[min(max(x0 - R + e, 0), X - 1)];
    }
    __syncthreads();
    const int x = x0 + lane;
    if (row < rows && x < X) {
      double acc = 0.0;
      for (int e = 0; e <= 2 * R; ++e) acc = __dadd_rn(acc, __dmul_rn(wt.w[e], (double)line[w][lane + e]));
      dst[row * X + x] = (float)acc;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(TPB) void sm_yz_kernel(const float* __restrict__ src, float* __restrict__ dst, int X, int Y, int Z, long long total, int axis, int R, sm_weights wt) {
  const long long pitch = axis == 1 ? (long long)X : (long long)X * Y;
  const int n = axis == 1 ? Y : Z;
  for (long long o = (long long)blockIdx.x * TPB + threadIdx.x; o < total; o += (long long)gridDim.x * TPB) {
    const long long row = o / X, slab = row / Y;                      // row = j + Y (k + Z c)
    const int p = axis == 1 ? (int)(row - slab * Y) : (int)(slab % Z);
    const long long base = o - p * pitch;
    double acc = 0.0;
    for (int t = -R; t <= R; ++t) acc = __dadd_rn(acc, __dmul_rn(wt.w[t + R], (double)src[base + min(max(p + t, 0), n - 1) * pitch]));
    dst[o] = (float)acc;
  }
}

// ---- the index-space difference along one axis: central (half the difference of the two neighbours), one-sided with denominator 1 at a border, 0 on an axis of extent 1 ---
template <typename Get>
__device__ __forceinline__ double df_diff(const Get& get, long long at, long long pitch, int p, int n) {
  if (n == 1) return 0.0;
  if (p == 0) return __dsub_rn(get(at + pitch), get(at));
  if (p == n - 1) return __dsub_rn(get(at), get(at - pitch));
  return __dmul_rn(__dsub_rn(get(at + pitch), get(at - pitch)), 0.5);
}
struct df_mat3 { double m[9]; };
// s_r = ((c_r + L[r][0] u_0) + L[r][1] u_1) + L[r][2] u_2
__device__ __forceinline__ double df_displace(double c, const df_mat3& L, int r, const double u[3]) {
  return __dadd_rn(__dadd_rn(__dadd_rn(c, __dmul_rn(L.m[3 * r], u[0])), __dmul_rn(L.m[3 * r + 1], u[1])), __dmul_rn(L.m[3 * r + 2], u[2]));
}

// ---- the demons step ---------------------------------------------------------------------------------------------------------------------------------------------
struct dm_geom { rs_mat W; df_mat3 L, G; double delta2; };

__global__ __launch_bounds__(TPB) void dm_kernel(vol_voxels fix, const uint8_t* __restrict__ mask, int X, int Y, int Z, vol_voxels mov, int Xm, int Ym, int Zm, dm_geom g,
                                                 const float* __restrict__ uin, float* __restrict__ uout) {
  const long long N = (long long)X * Y * Z;
  const double top[3] = {(double)(Xm - 1), (double)(Ym - 1), (double)(Zm - 1)};
  const auto get = [&](long long f) { return vol_dec(fix, f); };
  for (long long o = (long long)blockIdx.x * TPB + threadIdx.x; o < N; o += (long long)gridDim.x * TPB) {
    const double u[3] = {(double)uin[o], (double)uin[N + o], (double)uin[2 * N + o]};
    double v[3] = {0.0, 0.0, 0.0};
    if (!mask || mask[o] != 0) {
      const double fv = vol_dec(fix, o);
      const long long c = o / X;
      const int i = (int)(o - c * X), k = (int)(c / Y), j = (int)(c - (long long)k * Y);
      double s[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) s[r] = df_displace(rs_coord(g.W, r, i, j, k), g.L, r, u);
      if (fv == fv && s[0] >= 0.0 && s[0] <= top[0] && s[1] >= 0.0 && s[1] <= top[1] && s[2] >= 0.0 && s[2] <= top[2]) {
        const double mv = rs_blend_inside(mov, Xm, Ym, Zm, s);
        if (mv == mv) {
          const double d = __dsub_rn(fv, mv);
          const double gi[3] = {df_diff(get, o, 1, i, X), df_diff(get, o, X, j, Y), df_diff(get, o, (long long)X * Y, k, Z)};
          double gw[3];
#pragma unroll
          for (int r = 0; r < 3; ++r)
            gw[r] = __dadd_rn(__dadd_rn(__dmul_rn(g.G.m[3 * r], gi[0]), __dmul_rn(g.G.m[3 * r + 1], gi[1])), __dmul_rn(g.G.m[3 * r + 2], gi[2]));
          const double gg = __dadd_rn(__dadd_rn(__dmul_rn(gw[0], gw[0]), __dmul_rn(gw[1], gw[1])), __dmul_rn(gw[2], gw[2]));
          const double den = __dadd_rn(gg, __ddiv_rn(__dmul_rn(d, d), g.delta2));
          if (den > DEN_MIN) {                                        // (a NaN denominator -- a NaN neighbour of f -- is not above it)
#pragma unroll
            for (int r = 0; r < 3; ++r) v[r] = __ddiv_rn(__dmul_rn(d, gw[r]), den);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) uout[r * N + o] = (float)__dadd_rn(u[r], v[r]);
  }
}

// ---- the warp ------------------------------------------------------------------------------------------------------------------------------------------------------
struct wf_geom { rs_mat W, F; df_mat3 L; const float* field; int Xf, Yf, Zf, has_F; int X, Y, Z, mode; };

__device__ __forceinline__ void wf_coord(const wf_geom& g, int i, int j, int k, long long o, double s[3]) {
  const long long Nf = (long long)g.Xf * g.Yf * g.Zf;
  double u[3];
  if (!g.has_F) {                                                     // the output grid is the field grid
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = (double)g.field[c * Nf + o];
  } else {
    const int n[3] = {g.Xf, g.Yf, g.Zf};
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double v = rs_coord(g.F, r, i, j, k), top = (double)(n[r] - 1);
      q[r] = !(v >= 0.0) ? 0.0 : (v > top ? top : v);                 // mode 0: clamped into the field (a NaN goes to 0)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = rs_blend_inside(vol_voxels{g.field + c * Nf, 16, 0, 1.0, 0.0}, g.Xf, g.Yf, g.Zf, q);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) s[r] = df_displace(rs_coord(g.W, r, i, j, k), g.L, r, u);
}

template <typename D>
struct wf_lin {
  wf_geom g; vol_voxels src; double cval;
  __device__ __forceinline__ D operator()(int i, int j, int k, long long o) const {
    double s[3];
    wf_coord(g, i, j, k, o, s);
    return rs_store<D>(rs_linear_at(src, g.X, g.Y, g.Z, g.mode, cval, s));
  }
};
template <typename T>
struct wf_near {
  wf_geom g; const T* src; T cval;
  __device__ __forceinline__ T operator()(int i, int j, int k, long long o) const {
    double s[3];
    wf_coord(g, i, j, k, o, s);
    return rs_nearest_at<T>(src, g.X, g.Y, g.Z, g.mode, cval, s);
  }
};

template <typename T, typename Op>
__global__ __launch_bounds__(TPB) void wf_kernel(Op op, T* __restrict__ dst, int X2, int Y2, int Z2) {
  const long long outs = (long long)X2 * Y2 * Z2;
  for (long long o = (long long)blockIdx.x * TPB + threadIdx.x; o < outs; o += (long long)gridDim.x * TPB) {
    const long long c = o / X2;
    const int i = (int)(o - c * X2), k = (int)(c / Y2), j = (int)(c - (long long)k * Y2);
    dst[o] = op(i, j, k, o);
  }
}
template <typename T, typename Op>
void wf_launch(const Op& op, void* dst, int X2, int Y2, int Z2, hipStream_t s) {
  hipLaunchKernelGGL((wf_kernel<T, Op>), dim3(vol_blocks((long long)X2 * Y2 * Z2, GRID_CAP, TPB)), dim3(TPB), 0, s, op, static_cast<T*>(dst), X2, Y2, Z2);
}

// ---- the Jacobian determinant: J = I + D inv(A), D[c][a] the index-space difference of u_c along axis a; det by the first row --------------------------------------------
__global__ __launch_bounds__(TPB) void jc_kernel(const float* __restrict__ field, int X, int Y, int Z, df_mat3 Ai, float* __restrict__ det, uint32_t* __restrict__ folded) {
  const long long N = (long long)X * Y * Z;
  const int lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * TPB; base < N; base += (long long)gridDim.x * TPB) {          // (base is workgroup-uniform)
    const long long o = base + threadIdx.x;
    bool fold = false;
    if (o < N) {
      const long long c = o / X;
      const int i = (int)(o - c * X), k = (int)(c / Y), j = (int)(c - (long long)k * Y);
      double J[3][3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float* uc = field + q * N;
        const auto get = [&](long long f) { return (double)uc[f]; };
        const double D[3] = {df_diff(get, o, 1, i, X), df_diff(get, o, X, j, Y), df_diff(get, o, (long long)X * Y, k, Z)};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double m = __dadd_rn(__dadd_rn(__dmul_rn(D[0], Ai.m[r]), __dmul_rn(D[1], Ai.m[3 + r])), __dmul_rn(D[2], Ai.m[6 + r]));
          J[q][r] = q == r ? __dadd_rn(1.0, m) : m;
        }
      }
      const double m0 = __dsub_rn(__dmul_rn(J[1][1], J[2][2]), __dmul_rn(J[1][2], J[2][1]));
      const double m1 = __dsub_rn(__dmul_rn(J[1][0], J[2][2]), __dmul_rn(J[1][2], J[2][0]));
      const double m2 = __dsub_rn(__dmul_rn(J[1][0], J[2][1]), __dmul_rn(J[1][1], J[2][0]));
      const double dj = __dadd_rn(__dsub_rn(__dmul_rn(J[0][0], m0), __dmul_rn(J[0][1], m1)), __dmul_rn(J[0][2], m2));
      det[o] = (float)dj;
      fold = dj <= 0.0;                                               // (a NaN determinant is not counted)
    }
    const unsigned long long folds = __ballot(fold);
    if (folds && lane == __ffsll((long long)folds) - 1) atomicAdd(folded, (uint32_t)__popcll(folds));
  }
}
}  // namespace

extern "C" {

int32_t unet_vol_smooth_axis(unet_ctx* ctx, const float* src, int32_t C, int32_t X, int32_t Y, int32_t Z, int32_t axis, int32_t R, const double* weights, float* dst,
                             void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (C < 1 || C > MAX_C) UNET_FAIL(ctx, UNET_E_ARG, "vol_smooth_axis: %d volumes, not 1 to %d", C, MAX_C);
  if (!rs_out_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_smooth_axis: volumes of %d x %d x %d (every extent is at least 1, fewer than 2^31 voxels)", X, Y, Z);
  if (axis < 0 || axis > 2) UNET_FAIL(ctx, UNET_E_ARG, "vol_smooth_axis: axis %d is not 0, 1 or 2", axis);
  if (R < 0 || R > MAX_R) UNET_FAIL(ctx, UNET_E_ARG, "vol_smooth_axis: a radius of %d taps, not 0 to %d", R, MAX_R);
  if (!df_finite(weights, 2 * R + 1)) UNET_FAIL(ctx, UNET_E_ARG, "vol_smooth_axis: weights is 2 R + 1 finite doubles");
  if (!df_aligned(src, sizeof(float)) || !df_aligned(dst, sizeof(float)) || src == dst)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_smooth_axis: a null buffer, one not aligned to its element size, or src = dst");
  sm_weights wt{};
  for (int i = 0; i <= 2 * R; ++i) wt.w[i] = weights[i];
  hipStream_t s = as_stream(stream);
  const long long N = (long long)X * Y * Z;
  if (axis == 0) {
    const long long rows = (long long)C * Y * Z;
    const int segs = (X + SEG - 1) / SEG;
    const long long tiles = ((rows + ROWS - 1) / ROWS) * segs;
    hipLaunchKernelGGL(sm_x_kernel, dim3((unsigned)(tiles > GRID_CAP ? GRID_CAP : tiles)), dim3(TPB), 0, s, src, dst, X, rows, segs, tiles, R, wt);
  } else {
    hipLaunchKernelGGL(sm_yz_kernel, dim3(vol_blocks(C * N, GRID_CAP, TPB)), dim3(TPB), 0, s, src, dst, X, Y, Z, C * N, axis, R, wt);
  }
  UNET_CHECK_LAUNCH(ctx, "vol_smooth_axis"); return UNET_OK;
}

int32_t unet_vol_demons_step(unet_ctx* ctx, const void* fixed, int32_t f_dtype, int32_t X, int32_t Y, int32_t Z, int32_t f_scaled, double f_slope, double f_inter,
                             const uint8_t* mask, const void* moving, int32_t m_dtype, int32_t Xm, int32_t Ym, int32_t Zm, int32_t m_scaled, double m_slope, double m_inter,
                             const double* W, const double* L, const double* Ginv, double delta, const float* field_in, float* field_out, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!rs_out_ok(X, Y, Z) || !rs_out_ok(Xm, Ym, Zm)) UNET_FAIL(ctx, UNET_E_ARG, "vol_demons_step: a volume of %d x %d x %d and one of %d x %d x %d (every extent is at least 1, fewer than 2^31 voxels)", X, Y, Z, Xm, Ym, Zm);
  if (vol_itemsize(f_dtype) == 0 || vol_itemsize(m_dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_demons_step: a NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64");
  if (!df_finite(W, 12) || !df_finite(L, 9) || !df_finite(Ginv, 9)) UNET_FAIL(ctx, UNET_E_ARG, "vol_demons_step: W is 12, L and Ginv are 9 finite doubles");
  if (!std::isfinite(delta) || !(delta > 0.0) || !std::isfinite(delta * delta) || !(delta * delta > 0.0))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_demons_step: the step bound is a finite positive number of millimetres whose square is one too");
  if (!df_aligned(fixed, vol_itemsize(f_dtype)) || !df_aligned(moving, vol_itemsize(m_dtype)) || !df_aligned(field_in, sizeof(float)) || !df_aligned(field_out, sizeof(float)) ||
      field_in == field_out)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_demons_step: a null buffer, one not aligned to its element size, or field_in = field_out");
  dm_geom g{};
  for (int i = 0; i < 12; ++i) g.W.m[i] = W[i];
  for (int i = 0; i < 9; ++i) { g.L.m[i] = L[i]; g.G.m[i] = Ginv[i]; }
  g.delta2 = delta * delta;
  const vol_voxels fs{fixed, f_dtype, f_scaled ? 1 : 0, f_slope, f_inter}, ms{moving, m_dtype, m_scaled ? 1 : 0, m_slope, m_inter};
  hipLaunchKernelGGL(dm_kernel, dim3(vol_blocks((long long)X * Y * Z, GRID_CAP, TPB)), dim3(TPB), 0, as_stream(stream), fs, mask, X, Y, Z, ms, Xm, Ym, Zm, g, field_in, field_out);
  UNET_CHECK_LAUNCH(ctx, "vol_demons_step"); return UNET_OK;
}

int32_t unet_vol_warp_field(unet_ctx* ctx, const void* src, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, const double* W,
                            const double* L, const float* field, int32_t Xf, int32_t Yf, int32_t Zf, const double* F, int32_t order, int32_t mode, double cval,
                            uint64_t cval_bits, void* dst, int32_t dst_dtype, int32_t X2, int32_t Y2, int32_t Z2, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok_or_empty(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: a source dimension is negative or the source has 2^31 voxels or more");
  if (!rs_out_ok(X2, Y2, Z2) || !rs_out_ok(Xf, Yf, Zf)) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: an output of %d x %d x %d and a field of %d x %d x %d (every extent is at least 1, fewer than 2^31 voxels)", X2, Y2, Z2, Xf, Yf, Zf);
  if (vol_itemsize(dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: the NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64");
  if (order < 0 || order > 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: order %d is not 0 (nearest) or 1 (linear)", order);
  if (order == 1 && dst_dtype != 64 && dst_dtype != 16 && dst_dtype != 2) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: dst_dtype %d is not 64 (float64), 16 (float32) or 2 (uint8 mask)", dst_dtype);
  if (order == 0 && dst_dtype != dtype) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: order 0 moves the stored elements: dst_dtype %d is not the source's %d", dst_dtype, dtype);
  if (mode < 0 || mode > 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: mode %d is not 0 (nearest edge) or 1 (constant)", mode);
  const bool empty = (long long)X * Y * Z == 0;
  if (empty && mode == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: the source has no voxels and mode 0 has no edge to repeat");
  if (!df_finite(W, 12) || !df_finite(L, 9) || (F && !df_finite(F, 12))) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: W and F are 12, L is 9 finite doubles");
  if (!F && (Xf != X2 || Yf != Y2 || Zf != Z2)) UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: without F the field lies on the output grid, and %d x %d x %d is not %d x %d x %d", Xf, Yf, Zf, X2, Y2, Z2);
  const size_t out_size = order == 0 ? vol_itemsize(dtype) : vol_itemsize(dst_dtype);
  if ((!empty && !df_aligned(src, vol_itemsize(dtype))) || !df_aligned(field, sizeof(float)) || !df_aligned(dst, out_size))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_warp_field: a null buffer, or one not aligned to its element size");
  wf_geom g{};
  for (int i = 0; i < 12; ++i) { g.W.m[i] = W[i]; g.F.m[i] = F ? F[i] : 0.0; }
  for (int i = 0; i < 9; ++i) g.L.m[i] = L[i];
  g.field = field; g.Xf = Xf; g.Yf = Yf; g.Zf = Zf; g.has_F = F ? 1 : 0;
  g.X = X; g.Y = Y; g.Z = Z; g.mode = mode;
  hipStream_t s = as_stream(stream);
  if (order == 1) {
    const vol_voxels sv{src, dtype, scaled ? 1 : 0, slope, inter};
    switch (dst_dtype) {
      case 64: wf_launch<double>(wf_lin<double>{g, sv, cval}, dst, X2, Y2, Z2, s); break;
      case 16: wf_launch<float>(wf_lin<float>{g, sv, cval}, dst, X2, Y2, Z2, s); break;
      default: wf_launch<uint8_t>(wf_lin<uint8_t>{g, sv, cval}, dst, X2, Y2, Z2, s); break;
    }
  } else {
    switch (vol_itemsize(dtype)) {
      case 1: wf_launch<uint8_t>(wf_near<uint8_t>{g, static_cast<const uint8_t*>(src), (uint8_t)cval_bits}, dst, X2, Y2, Z2, s); break;
      case 2: wf_launch<uint16_t>(wf_near<uint16_t>{g, static_cast<const uint16_t*>(src), (uint16_t)cval_bits}, dst, X2, Y2, Z2, s); break;
      case 4: wf_launch<uint32_t>(wf_near<uint32_t>{g, static_cast<const uint32_t*>(src), (uint32_t)cval_bits}, dst, X2, Y2, Z2, s); break;
      default: wf_launch<uint64_t>(wf_near<uint64_t>{g, static_cast<const uint64_t*>(src), (uint64_t)cval_bits}, dst, X2, Y2, Z2, s); break;
    }
  }
  UNET_CHECK_LAUNCH(ctx, "vol_warp_field"); return UNET_OK;
}

int32_t unet_vol_jacobian(unet_ctx* ctx, const float* field, int32_t X, int32_t Y, int32_t Z, const double* Ainv, float* det, uint32_t* folded, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!rs_out_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_jacobian: a field of %d x %d x %d (every extent is at least 1, fewer than 2^31 voxels)", X, Y, Z);
  if (!df_finite(Ainv, 9)) UNET_FAIL(ctx, UNET_E_ARG, "vol_jacobian: Ainv is 9 finite doubles");
  if (!df_aligned(field, sizeof(float)) || !df_aligned(det, sizeof(float)) || !df_aligned(folded, sizeof(uint32_t)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_jacobian: a null buffer, or one not aligned to its element size");
  df_mat3 Ai{};
  for (int i = 0; i < 9; ++i) Ai.m[i] = Ainv[i];
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(folded, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(jc_kernel, dim3(vol_blocks((long long)X * Y * Z, GRID_CAP, TPB)), dim3(TPB), 0, s, field, X, Y, Z, Ai, det, folded);
  UNET_CHECK_LAUNCH(ctx, "vol_jacobian"); return UNET_OK;
}

}  // extern "C"

// The operations that define a trilinear sample of a stored volume bit for bit, shared by kernels_resample.hip, kernels_register.hip (4x) and
// kernels_deform.hip (4y) so that the moving sample a joint histogram bins or a demons step subtracts is, by construction, the float64 unet_vol_resample_linear writes at the
// same coordinate: the source coordinate, the blend a + fl((b - a) w) of voxels decoded by vol_common.h's vol_dec, the blend of the eight neighbours of a coordinate
// that lies inside the volume, and the two per-coordinate samplers (rs_linear_at, rs_nearest_at) that the resampling entries and unet_vol_warp_field both call.
// All three files are compiled with -ffp-contract=off; the __d*_rn forms keep every operation a rounded float64 one either way.
#pragma once
#include "common.h"
#include "vol_common.h"

namespace {
// a grid to write: at least one voxel, fewer than 2^31 (X Y is tested before it is multiplied by Z)
inline bool rs_out_ok(int X, int Y, int Z) { return X > 0 && Y > 0 && Z > 0 && (long long)X * Y < 0x80000000LL && (long long)X * Y * Z < 0x80000000LL; }
struct rs_mat { double m[12]; };
__device__ __forceinline__ double rs_coord(const rs_mat& M, int r, int i, int j, int k) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M.m[4 * r], (double)i), __dmul_rn(M.m[4 * r + 1], (double)j)), __dmul_rn(M.m[4 * r + 2], (double)k)), M.m[4 * r + 3]);
}

__device__ __forceinline__ double rs_lerp(double a, double b, double w) { return __dadd_rn(a, __dmul_rn(__dsub_rn(b, a), w)); }

// the blend at a coordinate already found inside, 0 <= s_r <= n_r - 1 as doubles (so the conversions are safe): f = floor(s), t = s - f, the upper neighbour clamped,
// lerp along x, then y, then z -- what rs_lin computes in mode 0, where its clamp of s is then the identity
__device__ __forceinline__ double rs_blend_inside(const vol_voxels& src, int X, int Y, int Z, const double s[3]) {
  const int n[3] = {X, Y, Z};
  int a0[3], a1[3];
  double t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double f = floor(s[r]);
    a0[r] = (int)f; a1[r] = min(a0[r] + 1, n[r] - 1);
    t[r] = __dsub_rn(s[r], f);
  }
  double p[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)                                         // c = dx + 2 dy + 4 dz
    p[c] = vol_dec(src, ((c & 1) ? a1[0] : a0[0]) + (long long)X * (((c & 2) ? a1[1] : a0[1]) + (long long)Y * ((c & 4) ? a1[2] : a0[2])));
  const double c00 = rs_lerp(p[0], p[1], t[0]), c10 = rs_lerp(p[2], p[3], t[0]), c01 = rs_lerp(p[4], p[5], t[0]), c11 = rs_lerp(p[6], p[7], t[0]);
  return rs_lerp(rs_lerp(c00, c10, t[1]), rs_lerp(c01, c11, t[1]), t[2]);
}

// ---- the sample of unet_vol_resample_linear at a coordinate s, as a float64 ---------------------------------------------------------------------------------------
__device__ __forceinline__ double rs_linear_at(const vol_voxels& src, int X, int Y, int Z, int mode, double cval, const double sc[3]) {
  const int n[3] = {X, Y, Z};
  int a0[3], a1[3];                                                   // the two neighbours of every axis, as indices that are always inside
  bool in0[3], in1[3];
  double t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double s = sc[r];
    const double top = (double)(n[r] - 1);
    if (mode == 0) s = !(s >= 0.0) ? 0.0 : (s > top ? top : s);              // (a NaN goes to 0)
    const double f = floor(s);
    if (mode == 0) {                                                  // 0 <= f <= n - 1 here
      a0[r] = (int)f; a1[r] = min(a0[r] + 1, n[r] - 1); in0[r] = in1[r] = true;
      t[r] = __dsub_rn(s, f);
    } else {                                                          // f outside [-1, n - 1] (or a NaN): both neighbours are outside, nothing is converted
      in0[r] = f >= 0.0 && f <= top; in1[r] = f >= -1.0 && f <= top - 1.0;
      const int fi = (f >= -1.0 && f <= top) ? (int)f : 0;
      a0[r] = in0[r] ? fi : 0; a1[r] = in1[r] ? fi + 1 : 0;
      t[r] = (in0[r] || in1[r]) ? __dsub_rn(s, f) : 0.0;              // both outside: all eight read cval, and a weight of inf - inf or NaN must not turn it into a NaN
    }
  }
  double p[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {                                       // c = dx + 2 dy + 4 dz
    const bool in = ((c & 1) ? in1[0] : in0[0]) && ((c & 2) ? in1[1] : in0[1]) && ((c & 4) ? in1[2] : in0[2]);
    const long long f = ((c & 1) ? a1[0] : a0[0]) + (long long)X * (((c & 2) ? a1[1] : a0[1]) + (long long)Y * ((c & 4) ? a1[2] : a0[2]));
    p[c] = in ? vol_dec(src, f) : cval;
  }
  const double c00 = rs_lerp(p[0], p[1], t[0]), c10 = rs_lerp(p[2], p[3], t[0]), c01 = rs_lerp(p[4], p[5], t[0]), c11 = rs_lerp(p[6], p[7], t[0]);
  return rs_lerp(rs_lerp(c00, c10, t[1]), rs_lerp(c01, c11, t[1]), t[2]);
}
template <typename D> __device__ __forceinline__ D rs_store(double v);
template <> __device__ __forceinline__ double rs_store<double>(double v) { return v; }
template <> __device__ __forceinline__ float rs_store<float>(double v) { return (float)v; }                  // one rounding to nearest even
template <> __device__ __forceinline__ uint8_t rs_store<uint8_t>(double v) { return v >= 0.5 ? 1 : 0; }      // (a NaN is not >= 0.5)

// ---- the element of unet_vol_resample_nearest at a coordinate s: q = floor(s + 0.5); mode 0 clamps q into the volume (a NaN goes to 0), mode 1 reads cval outside ----
template <typename T>
__device__ __forceinline__ T rs_nearest_at(const T* __restrict__ src, int X, int Y, int Z, int mode, T cval, const double sc[3]) {
  const int n[3] = {X, Y, Z};
  int q[3];
  bool inside = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double v = floor(__dadd_rn(sc[r], 0.5)), top = (double)(n[r] - 1);
    if (mode == 0) q[r] = !(v >= 0.0) ? 0 : (v > top ? n[r] - 1 : (int)v);
    else { const bool in = v >= 0.0 && v <= top; inside = inside && in; q[r] = in ? (int)v : 0; }
  }
  if (!inside) return cval;
  return src[q[0] + (long long)X * (q[1] + (long long)Y * q[2])];
}
}  // namespace

// The operations that define a trilinear sample of a stored volume bit for bit, shared by kernels_resample.hip and kernels_register.hip (4x) so
// that the moving sample a joint histogram bins is, by construction, the float64 unet_vol_resample_linear writes at the same coordinate: the source coordinate, the decode
// of kernels_intensity.hip's iv_dec (restated), the blend a + fl((b - a) w), and the blend of the eight neighbours of a coordinate that lies inside the volume.  Both files
// are compiled with -ffp-contract=off; the __d*_rn forms keep every operation a rounded float64 one either way.
#pragma once
#include "common.h"

namespace {
// (X Y is tested before it is multiplied by Z: three extents near 2^31 overflow a 64-bit product; a source with a zero extent has no voxels whatever the others are)
inline bool rs_dims_ok(int X, int Y, int Z) {
  return X >= 0 && Y >= 0 && Z >= 0 && (X == 0 || Y == 0 || Z == 0 || ((long long)X * Y < 0x80000000LL && (long long)X * Y * Z < 0x80000000LL));
}
inline bool rs_out_ok(int X, int Y, int Z) { return X > 0 && Y > 0 && Z > 0 && (long long)X * Y < 0x80000000LL && (long long)X * Y * Z < 0x80000000LL; }
inline int rs_itemsize(int dt) {
  switch (dt) { case 2: case 256: return 1; case 4: case 512: return 2; case 8: case 768: case 16: return 4; case 64: return 8; default: return 0; }
}

struct rs_mat { double m[12]; };
__device__ __forceinline__ double rs_coord(const rs_mat& M, int r, int i, int j, int k) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M.m[4 * r], (double)i), __dmul_rn(M.m[4 * r + 1], (double)j)), __dmul_rn(M.m[4 * r + 2], (double)k)), M.m[4 * r + 3]);
}

// ---- the decode of kernels_intensity.hip (NIfTI-1 datatype codes; (float64(v) * slope) + inter, two rounded operations) ----------------------------------------------
struct rs_src { const void* p; int dt; int scaled; double slope, inter; };
__device__ __forceinline__ double rs_dec(const rs_src& s, long long i) {
  double v;
  switch (s.dt) {                                                     // (wave-uniform: one datatype per launch)
    case 2: v = (double)static_cast<const uint8_t*>(s.p)[i]; break;
    case 256: v = (double)static_cast<const int8_t*>(s.p)[i]; break;
    case 4: v = (double)static_cast<const int16_t*>(s.p)[i]; break;
    case 512: v = (double)static_cast<const uint16_t*>(s.p)[i]; break;
    case 8: v = (double)static_cast<const int32_t*>(s.p)[i]; break;
    case 768: v = (double)static_cast<const uint32_t*>(s.p)[i]; break;
    case 16: v = (double)static_cast<const float*>(s.p)[i]; break;
    default: v = static_cast<const double*>(s.p)[i]; break;           // 64
  }
  return s.scaled ? __dadd_rn(__dmul_rn(v, s.slope), s.inter) : v;
}
__device__ __forceinline__ double rs_lerp(double a, double b, double w) { return __dadd_rn(a, __dmul_rn(__dsub_rn(b, a), w)); }

// the blend at a coordinate already found inside, 0 <= s_r <= n_r - 1 as doubles (so the conversions are safe): f = floor(s), t = s - f, the upper neighbour clamped,
// lerp along x, then y, then z -- what rs_lin computes in mode 0, where its clamp of s is then the identity
__device__ __forceinline__ double rs_blend_inside(const rs_src& src, int X, int Y, int Z, const double s[3]) {
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
    p[c] = rs_dec(src, ((c & 1) ? a1[0] : a0[0]) + (long long)X * (((c & 2) ? a1[1] : a0[1]) + (long long)Y * ((c & 4) ? a1[2] : a0[2])));
  const double c00 = rs_lerp(p[0], p[1], t[0]), c10 = rs_lerp(p[2], p[3], t[0]), c01 = rs_lerp(p[4], p[5], t[0]), c11 = rs_lerp(p[6], p[7], t[0]);
  return rs_lerp(rs_lerp(c00, c10, t[1]), rs_lerp(c01, c11, t[1]), t[2]);
}
}  // namespace

// What the CT-volume kernel files ("shared by the volume kernels") all need, defined once: the extents predicates, the bounded-grid size, the NIfTI
// datatype table, the decode of a stored voxel, the order-preserving keys of the doubles, the group of a voxel, wave and workgroup sums, and the packed one-bit volume.
// Results that are defined as bit-equal across files -- the value a joint histogram bins and the value the resampler writes, the value the threshold compares and the value
// the intensity statistics count -- are equal because they all come from vol_dec below.
#pragma once
#include "common.h"

namespace {
// ---- host side --------------------------------------------------------------------------------------------------------------------------------------
// A volume is [X, Y, Z] in Fortran order (f = x + X (y + Y z)) with X Y Z < 2^31.  X Y < 2^31 is established before X Y is multiplied by Z: with it the product fits 64
// bits whatever Z is (three extents near 2^31 would overflow it otherwise).
// The strict form: a slice of 2^31 voxels or more is refused even when Z == 0; X == 0 or Y == 0 is accepted whatever the other extents are.
inline bool vol_dims_ok(int X, int Y, int Z) {
  if (X < 0 || Y < 0 || Z < 0) return false;
  const long long XY = (long long)X * Y;
  return XY < 0x80000000LL && XY * Z < 0x80000000LL;
}
// The lenient form: a volume with any zero extent has no voxels and is accepted whatever its other extents are (a resample source, an ensemble's empty volume).
inline bool vol_dims_ok_or_empty(int X, int Y, int Z) { return X >= 0 && Y >= 0 && Z >= 0 && (X == 0 || Y == 0 || Z == 0 || vol_dims_ok(X, Y, Z)); }
// workgroups of tpb lanes for `items` items, at least 1 and at most cap (the grid-stride launches' bounded grid)
inline unsigned vol_blocks(long long items, long long cap, int tpb) { long long b = (items + tpb - 1) / tpb; return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b)); }
// bytes of a voxel of a NIfTI-1 datatype code; 0: not one of the eight
inline int vol_itemsize(int dt) {
  switch (dt) { case 2: case 256: return 1; case 4: case 512: return 2; case 8: case 768: case 16: return 4; case 64: return 8; default: return 0; }
}
inline bool vol_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline bool vol_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
  return p < q + nb && q < p + na;
}
inline size_t vol_pad16(size_t b) { return (b + 15) / 16 * 16; }

// ---- the stored voxels: NIfTI-1 datatype codes, decoded as get_fdata() decodes them: (float64(v) * slope) + inter, two rounded operations ------------------------------
// (the __d*_rn forms keep them two in the files that are built without -ffp-contract=off)
struct vol_voxels { const void* p; int dt; int scaled; double slope, inter; };
__device__ __forceinline__ double vol_dec(const vol_voxels& s, long long i) {
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

// order-preserving keys of the doubles (-0.0 below +0.0); no non-NaN value maps to ~0 or to 0, the two "nothing seen" marks of an integer atomicMin / atomicMax
__device__ __forceinline__ unsigned long long vol_d2ord(double d) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double vol_ord2d(unsigned long long o) { return __longlong_as_double((long long)((o >> 63) ? (o & 0x7FFFFFFFFFFFFFFFull) : ~o)); }

// the group of voxel i: 1..n, or 0 when it takes no part.  A label outside 1..n is ignored, never an address.
struct vol_groups { const int32_t* labels; const uint8_t* mask; const uint8_t* region; int n; };
__device__ __forceinline__ int vol_group(const vol_groups& g, long long i) {
  if (g.region && g.region[i] == 0) return 0;
  const int l = g.labels ? g.labels[i] : (g.mask[i] ? 1 : 0);
  return (unsigned)(l - 1) < (unsigned)g.n ? l : 0;
}

// ---- sums: a butterfly over the 64 lanes of a wave (both partners compute a + b: the same bits in every lane), then the wave sums in LDS ------------------------------
template <typename T>
__device__ __forceinline__ T vol_wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// -> the sum in every lane, the wave sums added to T(0) left to right; s_w: TPB / 64 words; a barrier separates two uses of s_w
template <typename T, int TPB>
__device__ __forceinline__ T vol_block_sum(T v, T* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
#pragma unroll
  for (int w = 0; w < TPB / 64; ++w) t += s_w[w];
  return t;
}

// ---- a volume packed to one bit per voxel along x: word wi of row (y, z) holds the voxels x = 64 wi .. 64 wi + 63, bit b voxel 64 wi + b; rows are padded to words ------
struct vol_bits { int X, Y, Z, WX; long long N, words; };             // WX words per row, words = WX Y Z
inline vol_bits vol_bits_make(int X, int Y, int Z) { const int WX = (X + 63) / 64; return {X, Y, Z, WX, (long long)X * Y * Z, (long long)WX * Y * Z}; }
// a workspace of `planes` packed volumes, each padded to 16 bytes
struct vol_bits_layout { size_t plane, total; };
inline vol_bits_layout vol_bits_layout_of(const vol_bits& d, int planes) { const size_t p = vol_pad16((size_t)d.words * sizeof(unsigned long long)); return {p, planes * p}; }
__device__ __forceinline__ unsigned vol_bytes_to_bits(uint4 w) {      // 16 bytes -> 16 bits (byte != 0)
  const unsigned ws[4] = {w.x, w.y, w.z, w.w};
  unsigned bits = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) bits |= ((ws[i >> 2] >> (8 * (i & 3))) & 0xFFu) ? (1u << i) : 0u;
  return bits;
}
// the bits of word wi that are voxels (0 <= wi < WX: at least one)
__device__ __forceinline__ unsigned long long vol_bits_valid(const vol_bits& d, int wi) { const int left = d.X - wi * 64; return left >= 64 ? ~0ull : ((1ull << left) - 1ull); }
// a word of a packed volume that holds no bit at or beyond X; every word outside the volume reads as 0
__host__ __device__ __forceinline__ unsigned long long vol_bits_load(const unsigned long long* P, const vol_bits& d, int wi, int y, int z) {
  if (wi < 0 || wi >= d.WX || y < 0 || y >= d.Y || z < 0 || z >= d.Z) return 0ull;
  return P[wi + (long long)d.WX * (y + (long long)d.Y * z)];
}
// a word as a structuring element sees it under a border value: the bits beyond X, and every word outside the volume, hold fill (0 or ~0)
__device__ __forceinline__ unsigned long long vol_bits_load(const unsigned long long* __restrict__ P, const vol_bits& d, int wi, int y, int z, unsigned long long fill) {
  if (wi < 0 || wi >= d.WX || y < 0 || y >= d.Y || z < 0 || z >= d.Z) return fill;
  const unsigned long long v = vol_bits_valid(d, wi);
  return (P[wi + (long long)d.WX * (y + (long long)d.Y * z)] & v) | (fill & ~v);
}
}  // namespace

// Centerlines of a mask volume: topology-preserving 3-D thinning, the table of a thin mask's voxels, and the spread of labels along recorded
// arrival steps.  Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, outside the volume is background, extents of 1 are legal.
//   unet_vol_thin_begin / _iterations / _end     bytes -> bits, n iterations of 6 x (1 candidate launch + 8 re-check launches), bits -> bytes
//   unet_vol_skeleton_count / _emit              count -> scan -> emit: flat index, 26-bit neighbour mask and (optionally) a float64 value of every set voxel, in index order
//   unet_vol_label_spread                        labels[v] = the smallest non-zero label among the neighbours that arrived one step earlier, step by step
// The 26 neighbours of a voxel are numbered i = (dx + 1) + 3 (dy + 1) + 9 (dz + 1), i = 0 .. 26 without the centre 13: neighbour i is bit i for i < 13 and bit i - 1 for
// i > 13 of a uint32 (the NEIGHBOUR MASK of the table and the argument of sk_simple).
// sk_simple(n) is Bertrand and Malandain's characterisation for (26, 6): the set neighbours form exactly one 26-connected component, and the clear voxels of the
// 18-neighbourhood that are 6-adjacent to the centre are not empty and lie in one 6-connected component of the clear voxels of the 18-neighbourhood.  Both are flood fills in
// one register over the 27-bit cube (the centre as bit 13, always clear): a 26-dilation inside the cube is three shifts pairs -- x by 1, y by 3, z by 9, the x and y shifts
// masked so that no bit leaves its row or plane -- applied one after the other, a 6-dilation the union of the three; the fill repeats until it stops growing.  Those six
// masks take the place of a table of 26 adjacency constants: they are the same adjacency, and no lane reads memory for them.
// Thinning: vol_common.h's packed layout (vol_bits) -- word wi of row (y, z) holds the voxels x = 64 wi .. 64 wi + 63, bit b voxel 64 wi + b, rows padded to words, no bit at or
// beyond X.  The workspace holds the image P and the candidates Q.  One lane per word; the rows (y +- 1, z +- 1) and the edge bits of the x-adjacent words are gathered as
// gd_step_kernel gathers them.  A word with no set bit reads no neighbour; a word with no border bit in the pass's direction (no candidate of the sub-pass) does no
// predicate work.
//   sk_candidates_kernel(d)   Q = the set voxels of P whose neighbour in direction d is clear, that have at least 2 (endpoints) or 1 set neighbours, and are simple.  Reads P,
//                             writes Q: every voxel is judged on the image as it stands when the pass begins.
//   sk_recheck_kernel(k)      clears the voxels of Q in subfield k = (x & 1) | (y & 1) << 1 | (z & 1) << 2 that are still simple in P, in place.
// Why the in-place re-check does not depend on the order the lanes run in: a launch changes only bits of subfield k.  A lane writes only its own word.  Of the other words it
// reads, those of the eight other rows (dy, dz) != (0, 0) lie in rows whose y or z parity differs from k's, which no lane of this launch writes; of the two x-adjacent words
// of its own row it uses only bit 63 of the lower one for a candidate at bit 0 and bit 0 of the upper one for a candidate at bit 63, and those two voxels have the other x
// parity, so whichever lane writes that word leaves that bit as it was: the bit has one value throughout the launch.  Inside its own word the candidates of one subfield are
// two apart in x and never 26-neighbours, so every one is judged on the word as loaded and "all at once" equals any sequential order.
// removed[it] receives one 64-bit integer atomic per workgroup: integer sums, the same bits on every run.  No workgroup waits for another: a sub-pass boundary is a kernel
// boundary.  Every grid is sized to its work (one lane per word, per voxel or per block of words; at most 2^31 / 64 workgroups): there is no grid-stride loop and no later trip.
// Table: a workgroup owns SK_CHUNK words.  count: the set bytes of a word by a ballot (lane l reads voxel 64 wi + l), the chunk's sum into the workspace; scan: one
// workgroup turns the chunk sums into offsets and the total; emit: the ballot again, a lane's row = the chunk's offset + the words before + the set bits below its own.
// Label spread: a launch of step s writes only labels of voxels with arrival == s and reads only labels of voxels with arrival == s - 1; the two sets are disjoint, so the
// result does not depend on the order the lanes run in.
#include "common.h"
#include "vol_common.h"

namespace {
typedef unsigned long long u64;
constexpr int SK_TPB = 256;
constexpr int SK_CHUNK = 256;                                         // words of a workgroup of the table kernels: 64 per wave

// ---- the predicate ------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t SK_ALL = 0x7FFFFFFu;                              // the 27 voxels of the cube
constexpr uint32_t SK_X0 = 0x1249249u, SK_X2 = SK_X0 << 2;           // dx = -1 / dx = +1
constexpr uint32_t SK_Y0 = 0x7u | (0x7u << 9) | (0x7u << 18), SK_Y2 = SK_Y0 << 6;          // dy = -1 / dy = +1
constexpr uint32_t SK_CENTRE = 1u << 13;
constexpr uint32_t SK_N6 = (1u << 12) | (1u << 14) | (1u << 10) | (1u << 16) | (1u << 4) | (1u << 22);
constexpr uint32_t SK_CORNERS = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26);
constexpr uint32_t SK_N18 = SK_ALL & ~SK_CORNERS & ~SK_CENTRE;

__host__ __device__ __forceinline__ uint32_t sk_expand(uint32_t n26) { return (n26 & 0x1FFFu) | ((n26 >> 13) << 14); }          // 26 bits -> the cube, centre clear
__host__ __device__ __forceinline__ uint32_t sk_compress(uint32_t c27) { return (c27 & 0x1FFFu) | ((c27 >> 14) << 13); }
__host__ __device__ __forceinline__ uint32_t sk_dil_x(uint32_t f) { return ((f & ~SK_X2) << 1) | ((f & ~SK_X0) >> 1); }
__host__ __device__ __forceinline__ uint32_t sk_dil_y(uint32_t f) { return ((f & ~SK_Y2) << 3) | ((f & ~SK_Y0) >> 3); }
__host__ __device__ __forceinline__ uint32_t sk_dil_z(uint32_t f) { return ((f << 9) | (f >> 9)) & SK_ALL; }

__host__ __device__ inline bool sk_simple(uint32_t n26) {
  const uint32_t n = sk_expand(n26 & 0x3FFFFFFu);
  if (n == 0) return false;                                           // no component at all
  uint32_t f = n & (0u - n), g;                                       // the lowest set voxel
  do {
    g = f;
    f |= sk_dil_x(f);
    f |= sk_dil_y(f);
    f |= sk_dil_z(f);
    f &= n;
  } while (f != g);
  if (f != n) return false;                                           // more than one 26-component
  const uint32_t c = ~n & SK_N18, c6 = c & SK_N6;
  if (c6 == 0) return false;                                          // no clear 6-neighbour
  f = c6 & (0u - c6);
  do {
    g = f;
    f = (f | sk_dil_x(f) | sk_dil_y(f) | sk_dil_z(f)) & c;
  } while (f != g);
  return (c6 & ~f) == 0;
}

// ---- the packed image (vol_common.h's vol_bits; the workspace is P | Q) ----------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int sk_popc64(u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}
__host__ __device__ __forceinline__ int sk_popc32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}
__host__ __device__ __forceinline__ int sk_ctz64(u64 v) {             // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)v) - 1;
#else
  return __builtin_ctzll(v);
#endif
}

// the nine rows around a word: c = the word, l / r = the same row seen from x - 1 / x + 1 (bit b = voxel 64 wi + b -+ 1, across the word's edges)
struct sk_rows { u64 c[9], l[9], r[9]; };
__host__ __device__ __forceinline__ void sk_gather(const u64* P, const vol_bits& d, int wi, int y, int z, sk_rows& R) {
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int yy = y + (q % 3) - 1, zz = z + (q / 3) - 1;
    const u64 c = vol_bits_load(P, d, wi, yy, zz), lo = vol_bits_load(P, d, wi - 1, yy, zz), hi = vol_bits_load(P, d, wi + 1, yy, zz);
    R.c[q] = c;
    R.l[q] = (c << 1) | (lo >> 63);
    R.r[q] = (c >> 1) | (hi << 63);
  }
}
__host__ __device__ __forceinline__ uint32_t sk_code(const sk_rows& R, int b) {          // the neighbour mask of voxel b of the word
  uint32_t c27 = 0;
#pragma unroll
  for (int q = 0; q < 9; ++q)
    c27 |= ((uint32_t)((R.l[q] >> b) & 1ull) | ((uint32_t)((R.c[q] >> b) & 1ull) << 1) | ((uint32_t)((R.r[q] >> b) & 1ull) << 2)) << (3 * q);
  return sk_compress(c27);
}
// the set voxels of word w whose neighbour in direction dir is clear or outside; dir: 0 +z, 1 -z, 2 +y, 3 -y, 4 +x, 5 -x (the order of the passes)
__host__ __device__ __forceinline__ u64 sk_border(const u64* P, const vol_bits& d, u64 w, int wi, int y, int z, int dir) {
  switch (dir) {
    case 0: return w & ~vol_bits_load(P, d, wi, y, z + 1);
    case 1: return w & ~vol_bits_load(P, d, wi, y, z - 1);
    case 2: return w & ~vol_bits_load(P, d, wi, y + 1, z);
    case 3: return w & ~vol_bits_load(P, d, wi, y - 1, z);
    case 4: return w & ~((w >> 1) | (vol_bits_load(P, d, wi + 1, y, z) << 63));
    default: return w & ~((w << 1) | (vol_bits_load(P, d, wi - 1, y, z) >> 63));
  }
}
// the candidates of a direction pass in word `word` of P
__host__ __device__ inline u64 sk_candidates_word(const u64* P, const vol_bits& d, long long word, int dir, int min_n26) {
  const u64 w = P[word];
  if (!w) return 0ull;
  const long long row = word / d.WX;
  const int wi = (int)(word - row * d.WX), z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
  u64 border = sk_border(P, d, w, wi, y, z, dir);
  if (!border) return 0ull;
  sk_rows R;
  sk_gather(P, d, wi, y, z, R);
  u64 cand = 0;
  for (; border; border &= border - 1) {
    const int b = sk_ctz64(border);
    const uint32_t n = sk_code(R, b);
    if (sk_popc32(n) >= min_n26 && sk_simple(n)) cand |= 1ull << b;
  }
  return cand;
}
// the candidates `cand` (of one subfield) of word `word` that are still simple in P
__host__ __device__ inline u64 sk_recheck_word(const u64* P, const vol_bits& d, long long word, u64 cand) {
  const long long row = word / d.WX;
  const int wi = (int)(word - row * d.WX), z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
  sk_rows R;
  sk_gather(P, d, wi, y, z, R);
  u64 clear = 0;
  for (; cand; cand &= cand - 1) {
    const int b = sk_ctz64(cand);
    if (sk_simple(sk_code(R, b))) clear |= 1ull << b;
  }
  return clear;
}
// the bits of subfield k in a word of row (y, z): none when the row's parities differ, else every second bit
__host__ __device__ __forceinline__ u64 sk_subfield_bits(int k, int y, int z) {
  if ((y & 1) != ((k >> 1) & 1) || (z & 1) != ((k >> 2) & 1)) return 0ull;
  return (k & 1) ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull;
}

// ---- thinning kernels ---------------------------------------------------------------------------------------------------------------------------
// a wave per word: lane l holds voxel 64 wi + l, the ballot is the word
__global__ __launch_bounds__(SK_TPB) void sk_pack_kernel(const uint8_t* __restrict__ vol, vol_bits d, u64* __restrict__ P, u64* __restrict__ Q) {
  const long long word = ((long long)blockIdx.x * SK_TPB + threadIdx.x) >> 6;          // wave-uniform
  if (word >= d.words) return;
  const int lane = threadIdx.x & 63;
  const long long row = word / d.WX;
  const int x = (int)(word - row * d.WX) * 64 + lane;
  const bool set = x < d.X && vol[row * d.X + x] != 0;
  const u64 bits = __ballot(set);
  if (lane == 0) { P[word] = bits; Q[word] = 0ull; }
}
__global__ __launch_bounds__(SK_TPB) void sk_unpack_kernel(const u64* __restrict__ P, vol_bits d, uint8_t* __restrict__ vol) {
  const long long word = ((long long)blockIdx.x * SK_TPB + threadIdx.x) >> 6;
  if (word >= d.words) return;
  const int lane = threadIdx.x & 63;
  const long long row = word / d.WX;
  const int x = (int)(word - row * d.WX) * 64 + lane;
  if (x < d.X) vol[row * d.X + x] = (uint8_t)((P[word] >> lane) & 1ull);
}
__global__ __launch_bounds__(SK_TPB) void sk_candidates_kernel(const u64* __restrict__ P, u64* __restrict__ Q, vol_bits d, int dir, int min_n26) {
  const long long word = (long long)blockIdx.x * SK_TPB + threadIdx.x;
  if (word >= d.words) return;
  Q[word] = sk_candidates_word(P, d, word, dir, min_n26);
}
__global__ __launch_bounds__(SK_TPB) void sk_recheck_kernel(u64* __restrict__ P, const u64* __restrict__ Q, vol_bits d, int k, u64* __restrict__ removed) {
  __shared__ int s_w[SK_TPB / 64];
  const long long word = (long long)blockIdx.x * SK_TPB + threadIdx.x;
  int cnt = 0;
  if (word < d.words) {
    const long long row = word / d.WX;
    const int z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
    const u64 sub = sk_subfield_bits(k, y, z);
    const u64 cand = sub ? (Q[word] & sub) : 0ull;
    if (cand) {
      const u64 clear = sk_recheck_word(P, d, word, cand);
      if (clear) {
        P[word] &= ~clear;                                            // only this lane writes this word
        cnt = sk_popc64(clear);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < SK_TPB / 64; ++w) t += s_w[w];
    if (t) atomicAdd(removed, (u64)t);                                // integer sums: exact in any order
  }
}

// ---- the table ----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 sk_word_of_bytes(const uint8_t* __restrict__ vol, const vol_bits& d, long long word, int lane) {
  bool set = false;
  if (word < d.words) {
    const long long row = word / d.WX;
    const int x = (int)(word - row * d.WX) * 64 + lane;
    set = x < d.X && vol[row * d.X + x] != 0;
  }
  return __ballot(set);
}
__global__ __launch_bounds__(SK_TPB) void sk_count_kernel(const uint8_t* __restrict__ vol, vol_bits d, uint32_t* __restrict__ chunk_sums) {
  __shared__ int s_w[SK_TPB / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * SK_CHUNK + wv * 64;
  int cnt = 0;                                                        // the same in every lane of the wave
  for (int j = 0; j < 64; ++j) cnt += sk_popc64(sk_word_of_bytes(vol, d, base + j, lane));
  if (lane == 0) s_w[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < SK_TPB / 64; ++w) t += s_w[w];
    chunk_sums[blockIdx.x] = (uint32_t)t;
  }
}
// one workgroup: chunk sums -> exclusive offsets, in place, in index order; the total as int64
__global__ __launch_bounds__(SK_TPB) void sk_scan_kernel(uint32_t* __restrict__ chunk, long long chunks, long long* __restrict__ total) {
  __shared__ unsigned s_v[SK_TPB];
  __shared__ u64 s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (long long c0 = 0; c0 < chunks; c0 += SK_TPB) {
    const long long c = c0 + threadIdx.x;
    const unsigned v = c < chunks ? chunk[c] : 0u;
    s_v[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < SK_TPB; o <<= 1) {                            // Hillis and Steele, inclusive
      const unsigned a = threadIdx.x >= (unsigned)o ? s_v[threadIdx.x - o] : 0u;
      __syncthreads();
      s_v[threadIdx.x] += a;
      __syncthreads();
    }
    const u64 carry = s_carry;
    if (c < chunks) chunk[c] = (uint32_t)(carry + s_v[threadIdx.x] - v);          // the total is below 2^31
    __syncthreads();
    if (threadIdx.x == SK_TPB - 1) s_carry = carry + s_v[SK_TPB - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = (long long)s_carry;
}
__global__ __launch_bounds__(SK_TPB) void sk_emit_kernel(const uint8_t* __restrict__ vol, vol_bits d, const uint32_t* __restrict__ chunk_off, const double* __restrict__ d2,
                                                        long long capacity, int32_t* __restrict__ index, uint32_t* __restrict__ nbr, double* __restrict__ vals) {
  __shared__ unsigned s_cnt[SK_CHUNK], s_wt[SK_TPB / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * SK_CHUNK + wv * 64;
  for (int j = 0; j < 64; ++j) {
    const int c = sk_popc64(sk_word_of_bytes(vol, d, base + j, lane));
    if (lane == 0) s_cnt[wv * 64 + j] = (unsigned)c;
  }
  __syncthreads();
  const unsigned own = s_cnt[threadIdx.x];
  unsigned incl = own;                                                // inclusive scan over the wave's 64 words
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned a = __shfl_up(incl, o, 64);
    if (lane >= o) incl += a;
  }
  if (lane == 63) s_wt[wv] = incl;
  __syncthreads();
  unsigned before = chunk_off[blockIdx.x];
  for (int w = 0; w < wv; ++w) before += s_wt[w];
  __syncthreads();
  s_cnt[threadIdx.x] = before + incl - own;                           // the row of the word's first set voxel
  __syncthreads();
  for (int j = 0; j < 64; ++j) {
    const long long word = base + j;
    const u64 bits = sk_word_of_bytes(vol, d, word, lane);
    const long long pos = (long long)s_cnt[wv * 64 + j] + sk_popc64(bits & ((1ull << lane) - 1ull));
    if (((bits >> lane) & 1ull) && pos < capacity) {                  // never past the capacity; every lane comes back to the next word's ballot
      const long long row = word / d.WX;
      const int x = (int)(word - row * d.WX) * 64 + lane, z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
      const long long f = row * d.X + x;
      uint32_t c27 = 0;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx, yy = y + dy, zz = z + dz;
            if ((dx | dy | dz) == 0 || xx < 0 || xx >= d.X || yy < 0 || yy >= d.Y || zz < 0 || zz >= d.Z) continue;
            if (vol[xx + (long long)d.X * (yy + (long long)d.Y * zz)]) c27 |= 1u << ((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1));
          }
      index[pos] = (int32_t)f;
      nbr[pos] = sk_compress(c27);
      if (vals) vals[pos] = d2[f];
    }
  }
}

// ---- the label spread -----------------------------------------------------------------------------------------------------------------------------
// generate_binary_structure(3, conn): (dx, dy, dz) moves along at most conn axes
__global__ __launch_bounds__(SK_TPB) void sk_spread_kernel(const uint16_t* __restrict__ arrival, int32_t* __restrict__ labels, vol_bits d, int conn, unsigned step) {
  const long long f = (long long)blockIdx.x * SK_TPB + threadIdx.x;
  if (f >= d.N || arrival[f] != step) return;
  const long long row = f / d.X;
  const int x = (int)(f - row * d.X), z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
  int32_t best = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int n = (dx != 0) + (dy != 0) + (dz != 0), xx = x + dx, yy = y + dy, zz = z + dz;
        if (n == 0 || n > conn || xx < 0 || xx >= d.X || yy < 0 || yy >= d.Y || zz < 0 || zz >= d.Z) continue;
        const long long g = xx + (long long)d.X * (yy + (long long)d.Y * zz);
        if (arrival[g] != step - 1) continue;
        const int32_t l = labels[g];
        if (l != 0 && (best == 0 || l < best)) best = l;
      }
  if (best != 0) labels[f] = best;
}
}  // namespace

extern "C" {

size_t unet_vol_thin_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!vol_dims_ok(X, Y, Z) || (long long)X * Y * Z == 0) return 0;
  return vol_bits_layout_of(vol_bits_make(X, Y, Z), 2).total;
}

int32_t unet_vol_thin_begin(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_begin: a dimension is negative or the volume has 2^31 voxels or more");
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!mask || !ws) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_begin: null buffer");
  if (ws_bytes < unet_vol_thin_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_begin: workspace too small or not 16-byte aligned");
  const vol_bits_layout L = vol_bits_layout_of(d, 2);
  if (vol_overlap(mask, (size_t)d.N, ws, L.total)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_begin: the mask must not overlap the workspace");
  uint8_t* base = static_cast<uint8_t*>(ws);
  hipLaunchKernelGGL(sk_pack_kernel, dim3((unsigned)((d.words * 64 + SK_TPB - 1) / SK_TPB)), dim3(SK_TPB), 0, as_stream(stream), mask, d, reinterpret_cast<u64*>(base),
                     reinterpret_cast<u64*>(base + L.plane));
  UNET_CHECK_LAUNCH(ctx, "vol_thin_begin"); return UNET_OK;
}

int32_t unet_vol_thin_iterations(unet_ctx* ctx, int32_t X, int32_t Y, int32_t Z, int32_t first, int32_t n, int32_t endpoints, int64_t* removed, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_iterations: a dimension is negative or the volume has 2^31 voxels or more");
  if (first < 0 || n < 0 || (long long)first + n > 0x7FFFFFFFLL) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_iterations: first %d or n %d is negative (or their sum overflows)", first, n);
  if (endpoints != 0 && endpoints != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_iterations: endpoints %d is not 0 or 1", endpoints);
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0 || n == 0) return UNET_OK;
  if (!removed || !ws || !vol_aligned(removed, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_iterations: null or misaligned buffer");
  if (ws_bytes < unet_vol_thin_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_iterations: workspace too small or not 16-byte aligned");
  const vol_bits_layout L = vol_bits_layout_of(d, 2);
  if (vol_overlap(removed + first, (size_t)n * 8, ws, L.total)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_iterations: removed must not overlap the workspace");
  hipStream_t s = as_stream(stream);
  uint8_t* base = static_cast<uint8_t*>(ws);
  u64 *P = reinterpret_cast<u64*>(base), *Q = reinterpret_cast<u64*>(base + L.plane);
  UNET_HIP(ctx, hipMemsetAsync(removed + first, 0, (size_t)n * sizeof(int64_t), s));
  const unsigned blocks = (unsigned)((d.words + SK_TPB - 1) / SK_TPB);
  for (int it = first; it < first + n; ++it)
    for (int dir = 0; dir < 6; ++dir) {
      hipLaunchKernelGGL(sk_candidates_kernel, dim3(blocks), dim3(SK_TPB), 0, s, P, Q, d, dir, endpoints ? 2 : 1);
      for (int k = 0; k < 8; ++k) hipLaunchKernelGGL(sk_recheck_kernel, dim3(blocks), dim3(SK_TPB), 0, s, P, Q, d, k, reinterpret_cast<u64*>(removed) + it);
    }
  UNET_CHECK_LAUNCH(ctx, "vol_thin_iterations"); return UNET_OK;
}

int32_t unet_vol_thin_end(unet_ctx* ctx, int32_t X, int32_t Y, int32_t Z, uint8_t* out, const void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_end: a dimension is negative or the volume has 2^31 voxels or more");
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!out || !ws) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_end: null buffer");
  if (ws_bytes < unet_vol_thin_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_end: workspace too small or not 16-byte aligned");
  if (vol_overlap(out, (size_t)d.N, ws, vol_bits_layout_of(d, 2).total)) UNET_FAIL(ctx, UNET_E_ARG, "vol_thin_end: the output must not overlap the workspace");
  hipLaunchKernelGGL(sk_unpack_kernel, dim3((unsigned)((d.words * 64 + SK_TPB - 1) / SK_TPB)), dim3(SK_TPB), 0, as_stream(stream), static_cast<const u64*>(ws), d, out);
  UNET_CHECK_LAUNCH(ctx, "vol_thin_end"); return UNET_OK;
}

size_t unet_vol_skeleton_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!vol_dims_ok(X, Y, Z) || (long long)X * Y * Z == 0) return 0;
  const vol_bits d = vol_bits_make(X, Y, Z);
  return vol_pad16((size_t)((d.words + SK_CHUNK - 1) / SK_CHUNK) * sizeof(uint32_t));
}

int32_t unet_vol_skeleton_count(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int64_t* total, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_count: a dimension is negative or the volume has 2^31 voxels or more");
  if (!total || !vol_aligned(total, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_count: total is null or misaligned");
  const vol_bits d = vol_bits_make(X, Y, Z);
  hipStream_t s = as_stream(stream);
  if (d.N == 0) { UNET_HIP(ctx, hipMemsetAsync(total, 0, sizeof(int64_t), s)); return UNET_OK; }
  if (!mask || !ws) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_count: null buffer");
  if (ws_bytes < unet_vol_skeleton_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_count: workspace too small or not 16-byte aligned");
  const long long chunks = (d.words + SK_CHUNK - 1) / SK_CHUNK;
  if (vol_overlap(total, 8, ws, (size_t)chunks * 4) || vol_overlap(mask, (size_t)d.N, ws, (size_t)chunks * 4) || vol_overlap(mask, (size_t)d.N, total, 8))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_count: the mask, the total and the workspace must not overlap");
  uint32_t* cs = static_cast<uint32_t*>(ws);
  hipLaunchKernelGGL(sk_count_kernel, dim3((unsigned)chunks), dim3(SK_TPB), 0, s, mask, d, cs);
  hipLaunchKernelGGL(sk_scan_kernel, dim3(1), dim3(SK_TPB), 0, s, cs, chunks, reinterpret_cast<long long*>(total));
  UNET_CHECK_LAUNCH(ctx, "vol_skeleton_count"); return UNET_OK;
}

int32_t unet_vol_skeleton_emit(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, const double* d2, int64_t total, int64_t capacity, int32_t* index,
                               uint32_t* nbr, double* vals, const void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: a dimension is negative or the volume has 2^31 voxels or more");
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (total < 0 || total > d.N || capacity < 0 || capacity >= 0x80000000LL) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: total or capacity out of range");
  if (capacity < total) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: capacity %lld is below the total %lld", (long long)capacity, (long long)total);
  if ((d2 == nullptr) != (vals == nullptr)) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: d2 and vals are given together or not at all");
  if (d.N == 0 || total == 0) return UNET_OK;
  if (!mask || !ws || !index || !nbr || !vol_aligned(index, 4) || !vol_aligned(nbr, 4) || !vol_aligned(d2, 8) || !vol_aligned(vals, 8))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: null or misaligned buffer");
  if (ws_bytes < unet_vol_skeleton_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: workspace too small or not 16-byte aligned");
  const long long chunks = (d.words + SK_CHUNK - 1) / SK_CHUNK;
  const size_t cap = (size_t)capacity;
  const void* ins[3] = {mask, ws, d2};
  const size_t in_bytes[3] = {(size_t)d.N, (size_t)chunks * 4, d2 ? (size_t)d.N * 8 : 0};
  const void* outs[3] = {index, nbr, vals};
  const size_t out_bytes[3] = {cap * 4, cap * 4, vals ? cap * 8 : 0};
  for (int o = 0; o < 3; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 3; ++i)
      if (ins[i] && vol_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: an output overlaps an input");
    for (int p = o + 1; p < 3; ++p)
      if (outs[p] && vol_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) UNET_FAIL(ctx, UNET_E_ARG, "vol_skeleton_emit: two outputs overlap");
  }
  hipLaunchKernelGGL(sk_emit_kernel, dim3((unsigned)chunks), dim3(SK_TPB), 0, as_stream(stream), mask, d, static_cast<const uint32_t*>(ws), d2, (long long)capacity, index, nbr,
                     vals);
  UNET_CHECK_LAUNCH(ctx, "vol_skeleton_emit"); return UNET_OK;
}

int32_t unet_vol_label_spread(unet_ctx* ctx, const uint16_t* arrival, int32_t* labels, int32_t X, int32_t Y, int32_t Z, int32_t first, int32_t n, int32_t connectivity,
                              void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_spread: a dimension is negative or the volume has 2^31 voxels or more");
  if (connectivity < 1 || connectivity > 3) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_spread: connectivity %d is not 1, 2 or 3", connectivity);
  if (first < 1 || n < 0 || (long long)first + n - 1 > UNET_VOL_GEODESIC_MAX_STEP)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_label_spread: steps %d .. %lld are not inside 1 .. %d", first, (long long)first + n - 1, UNET_VOL_GEODESIC_MAX_STEP);
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0 || n == 0) return UNET_OK;
  if (!arrival || !labels || !vol_aligned(arrival, 2) || !vol_aligned(labels, 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_spread: null or misaligned buffer");
  if (vol_overlap(arrival, (size_t)d.N * 2, labels, (size_t)d.N * 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_spread: the labels must not overlap the arrival volume");
  hipStream_t s = as_stream(stream);
  const unsigned blocks = (unsigned)((d.N + SK_TPB - 1) / SK_TPB);
  for (int st = first; st < first + n; ++st) hipLaunchKernelGGL(sk_spread_kernel, dim3(blocks), dim3(SK_TPB), 0, s, arrival, labels, d, connectivity, (unsigned)st);
  UNET_CHECK_LAUNCH(ctx, "vol_label_spread"); return UNET_OK;
}

}  // extern "C"

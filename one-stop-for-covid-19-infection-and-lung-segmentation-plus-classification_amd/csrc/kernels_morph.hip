// Binary morphology of a mask volume on the device: dilate / erode / open / close, the same by a ball in millimetres, hole filling.
//   scipy.ndimage.binary_dilation / _erosion / _opening / _closing(mask, generate_binary_structure(3, c), iterations, border_value)      unet_vol_morph
//   the same with the structure's z = -1 and z = +1 planes cleared: every axial slice on its own                                          unet_vol_morph (planar)
//   d2 <= r^2 / d2 > r^2 on the exact squared distance transform of unet_vol_edt_sq: dilation / erosion by a ball of r millimetres        unet_vol_ball
//   scipy.ndimage.binary_fill_holes(mask, structure): the background components that do not reach the border                              unet_vol_fill_holes
// The volume is [X, Y, Z] in Fortran order (f = x + X (y + Y z)).  unet_vol_morph packs the bytes once to one bit per voxel along x -- word wi of row (y, z) holds
// the voxels x = 64 wi .. 64 wi + 63, bit b voxel 64 wi + b --, every step reads and writes packed words only (x neighbours: a shift with the carry of the adjacent
// word; y and z neighbours: whole words), and the result is unpacked once together with the per-slice counts.
// Launches (phase boundaries are kernel boundaries; no workgroup ever waits for another one):
//   morph_pack_kernel      bytes -> bits: 16 voxels per lane, four lanes make a word
//   morph_step_kernel      one dilation or erosion step, one word per lane, ping-pong between two packed buffers
//   morph_unpack_kernel    bits -> bytes 0 / 1 and the set voxels of every slice
//   morph_ball_kernel      out = d2 <= r2 or d2 > r2, and the slice counts
//   fh_faces_kernel        the labels met on the volume's faces (the four edges of every slice when planar) raise their byte in `touches`
//   fh_final_kernel        out = mask | !touches[label of the background component], and the slice counts
// Everything is integer / boolean: the result is the same on every run.
#include "common.h"
#include "vol_common.h"

namespace {
constexpr int TPB = 256;
constexpr long long GRID_CAP = 256 * 32;                             // grid-stride launches: 32 workgroups per CU
typedef unsigned long long u64;

__device__ __forceinline__ unsigned nibble_to_bytes(unsigned n) { return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21); }
__device__ __forceinline__ uint4 bits_to_bytes(unsigned bits) {
  return make_uint4(nibble_to_bytes(bits & 15u), nibble_to_bytes((bits >> 4) & 15u), nibble_to_bytes((bits >> 8) & 15u), nibble_to_bytes((bits >> 12) & 15u));
}

// ---- pack: one 16-voxel segment per lane (VEC: one 16-byte load; X % 16 == 0, so a segment is inside or outside as a whole); the four lanes of a word join by shuffles
template <bool VEC>
__global__ __launch_bounds__(TPB) void morph_pack_kernel(const uint8_t* __restrict__ mask, vol_bits d, u64* __restrict__ P) {
  const long long segs = d.words * 4;                                 // a multiple of 4: the four lanes of a word are all inside or all outside
  const int lane = threadIdx.x & 63;
  for (long long t0 = (long long)blockIdx.x * TPB + (threadIdx.x - lane); t0 < segs; t0 += (long long)gridDim.x * TPB) {          // wave-uniform trip count
    const long long t = t0 + lane;
    unsigned bits = 0;
    if (t < segs) {
      const long long w = t >> 2, row = w / d.WX;
      const int x0 = (int)(w - row * d.WX) * 64 + (int)(t & 3) * 16;
      const uint8_t* p = mask + row * d.X + x0;
      if (VEC) {
        if (x0 < d.X) bits = vol_bytes_to_bits(*reinterpret_cast<const uint4*>(p));
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) bits |= (x0 + i < d.X && p[i]) ? (1u << i) : 0u;
      }
    }
    u64 v = (u64)bits << (16 * (lane & 3));
    v |= __shfl_xor(v, 1, 64);
    v |= __shfl_xor(v, 2, 64);
    if (t < segs && (lane & 3) == 0) P[t >> 2] = v;
  }
}

// ---- one step.  A word is read as the structuring element sees it (vol_bits_load with a border value, fill = 0 or ~0)
// generate_binary_structure(3, conn) holds (dx, dy, dz) when it moves along at most conn axes: a row (dy, dz) with n = (dy != 0) + (dz != 0) <= conn takes part, with its
// x neighbours when n < conn.  planar: only dz = 0.
template <bool DILATE>
__global__ __launch_bounds__(TPB) void morph_step_kernel(const u64* __restrict__ src, vol_bits d, int conn, int planar, u64 fill, u64* __restrict__ dst) {
  const int zr = planar ? 0 : 1;
  for (long long w = (long long)blockIdx.x * TPB + threadIdx.x; w < d.words; w += (long long)gridDim.x * TPB) {
    const long long row = w / d.WX;
    const int wi = (int)(w - row * d.WX), z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
    u64 acc = DILATE ? 0ull : ~0ull;
    for (int dz = -zr; dz <= zr; ++dz)
      for (int dy = -1; dy <= 1; ++dy) {
        const int n = (dy != 0) + (dz != 0);
        if (n > conn) continue;
        const u64 c = vol_bits_load(src, d, wi, y + dy, z + dz, fill);
        u64 t = c;
        if (n < conn) {
          const u64 lo = vol_bits_load(src, d, wi - 1, y + dy, z + dz, fill), hi = vol_bits_load(src, d, wi + 1, y + dy, z + dz, fill);
          const u64 a = (c << 1) | (lo >> 63), b = (c >> 1) | (hi << 63);          // bit x takes voxel x - 1 / voxel x + 1
          t = DILATE ? (c | a | b) : (c & a & b);
        }
        acc = DILATE ? (acc | t) : (acc & t);
      }
    dst[w] = acc & vol_bits_valid(d, wi);
  }
}

// ---- unpack + counts: a workgroup stays inside one slice (bps workgroups per slice); one 16-voxel segment per lane and trip
template <bool VEC>
__global__ __launch_bounds__(TPB) void morph_unpack_kernel(const u64* __restrict__ P, vol_bits d, int bps, uint8_t* __restrict__ out, u64* __restrict__ counts) {
  __shared__ int s_w[TPB / 64];
  const int z = blockIdx.x / bps, part = blockIdx.x - z * bps;
  const long long sps = (long long)d.Y * d.WX * 4;                    // segments per slice
  int cnt = 0;
  for (long long i = (long long)part * TPB + threadIdx.x; i < sps; i += (long long)bps * TPB) {
    const long long w = i >> 2;
    const int y = (int)(w / d.WX), wi = (int)(w - (long long)y * d.WX), seg = (int)(i & 3);
    const int x0 = wi * 64 + seg * 16;
    if (x0 >= d.X) continue;
    const long long row = y + (long long)d.Y * z;
    unsigned bits = (unsigned)(P[wi + (long long)d.WX * row] >> (16 * seg)) & 0xFFFFu;
    if (d.X - x0 < 16) bits &= (1u << (d.X - x0)) - 1u;
    cnt += __popc(bits);
    uint8_t* o = out + row * d.X + x0;
    if (VEC) *reinterpret_cast<uint4*>(o) = bits_to_bytes(bits);
    else {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (x0 + k < d.X) o[k] = (uint8_t)((bits >> k) & 1u);
    }
  }
  const int t = vol_block_sum<int, TPB>(cnt, s_w);
  if (counts && threadIdx.x == 0 && t) atomicAdd(counts + z, (u64)t);          // integer sums: exact in any order
}

// ---- ball: V = 4: two 16-byte loads of d2 and one 4-byte store per lane and trip
template <int V>
__global__ __launch_bounds__(TPB) void morph_ball_kernel(const double* __restrict__ d2, long long XY, int bps, double r2, int keep_le, uint8_t* __restrict__ out,
                                                        u64* __restrict__ counts) {
  __shared__ int s_w[TPB / 64];
  const int z = blockIdx.x / bps, part = blockIdx.x - z * bps;
  const long long base = (long long)z * XY;
  int cnt = 0;
  for (long long i = ((long long)part * TPB + threadIdx.x) * V; i < XY; i += (long long)bps * TPB * V) {
    double v[V];
    if constexpr (V == 4) {
      const double2 a = *reinterpret_cast<const double2*>(d2 + base + i), b = *reinterpret_cast<const double2*>(d2 + base + i + 2);
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else v[0] = d2[base + i];
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const unsigned b = (keep_le ? (v[k] <= r2) : (v[k] > r2)) ? 1u : 0u;
      cnt += (int)b; word |= b << (8 * k);
    }
    if constexpr (V == 4) *reinterpret_cast<unsigned*>(out + base + i) = word;
    else out[base + i] = (uint8_t)word;
  }
  const int t = vol_block_sum<int, TPB>(cnt, s_w);
  if (counts && threadIdx.x == 0 && t) atomicAdd(counts + z, (u64)t);
}

// ---- fill holes -------------------------------------------------------------------------------------------------------------------------------
// labels: the components of the mask's zero voxels.  One lane per face voxel: faces x = 0, x = X - 1 (Y Z voxels each), y = 0, y = Y - 1 (X Z each) and, unless planar,
// z = 0, z = Z - 1 (X Y each).  Every writer stores the same value 1: the order does not matter.
__global__ __launch_bounds__(TPB) void fh_faces_kernel(const int32_t* __restrict__ labels, vol_bits d, long long FX, long long FY, long long FZ, long long tsize,
                                                      uint8_t* __restrict__ touches) {
  const long long total = 2 * (FX + FY + FZ);
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    int x, y, z;
    if (i < 2 * FX) { const long long j = i >> 1; x = (i & 1) ? d.X - 1 : 0; y = (int)(j % d.Y); z = (int)(j / d.Y); }
    else if (i < 2 * (FX + FY)) { const long long k = i - 2 * FX, j = k >> 1; y = (k & 1) ? d.Y - 1 : 0; x = (int)(j % d.X); z = (int)(j / d.X); }
    else { const long long k = i - 2 * (FX + FY), j = k >> 1; z = (k & 1) ? d.Z - 1 : 0; x = (int)(j % d.X); y = (int)(j / d.X); }
    const int l = labels[x + (long long)d.X * (y + (long long)d.Y * z)];
    if (l > 0 && l < tsize) touches[l] = 1;
  }
}
// out = 1 on the mask itself (label 0) and on the background components that no face voxel marked
template <int V>
__global__ __launch_bounds__(TPB) void fh_final_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ touches, long long tsize, long long XY, int bps,
                                                      uint8_t* __restrict__ out, u64* __restrict__ counts) {
  __shared__ int s_w[TPB / 64];
  const int z = blockIdx.x / bps, part = blockIdx.x - z * bps;
  const long long base = (long long)z * XY;
  int cnt = 0;
  for (long long i = ((long long)part * TPB + threadIdx.x) * V; i < XY; i += (long long)bps * TPB * V) {
    int l[V]; unsigned b[V];
    if constexpr (V == 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int4 w = *reinterpret_cast<const int4*>(labels + base + i + 4 * j); l[4 * j] = w.x; l[4 * j + 1] = w.y; l[4 * j + 2] = w.z; l[4 * j + 3] = w.w; }
    } else l[0] = labels[base + i];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      b[k] = (l[k] == 0 || ((unsigned)l[k] < (unsigned long long)tsize && !touches[l[k]])) ? 1u : 0u;          // a label outside the table is dropped, never an address
      cnt += (int)b[k];
    }
    if constexpr (V == 16) {
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
      *reinterpret_cast<uint4*>(out + base + i) = make_uint4(w[0], w[1], w[2], w[3]);
    } else out[base + i] = (uint8_t)b[0];
  }
  const int t = vol_block_sum<int, TPB>(cnt, s_w);
  if (counts && threadIdx.x == 0 && t) atomicAdd(counts + z, (u64)t);
}

inline int slice_blocks(long long items_per_slice, long long per_block) {
  long long bps = (items_per_slice + per_block - 1) / per_block;
  return (int)(bps < 1 ? 1 : (bps > 64 ? 64 : bps));
}
// the fill-holes workspace: labels [N] int32 | n (16 bytes) | touches [N + 1] bytes | the label workspace
struct fh_layout { size_t labels, n, touches, label_ws, total; };
inline fh_layout fh_make(int X, int Y, int Z) {
  const size_t N = (size_t)X * Y * Z;
  fh_layout L;
  L.labels = 0; L.n = vol_pad16(N * sizeof(int32_t)); L.touches = L.n + 16; L.label_ws = L.touches + vol_pad16(N + 1);
  L.total = L.label_ws + vol_pad16(unet_vol_label_ws_bytes(X, Y, Z));
  return L;
}
}  // namespace

extern "C" {

size_t unet_vol_morph_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!vol_dims_ok(X, Y, Z)) return 0;
  const vol_bits d = vol_bits_make(X, Y, Z);
  return d.N == 0 ? 0 : vol_bits_layout_of(d, 2).total;          // two packed volumes, ping and pong
}

int32_t unet_vol_morph(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t op, int32_t connectivity, int32_t planar, int32_t iterations,
                       int32_t border_value, uint8_t* out, int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: bad args");
  if (op < UNET_MORPH_DILATE || op > UNET_MORPH_CLOSE) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: op %d is not dilate (0), erode (1), open (2) or close (3)", op);
  if (connectivity < 1 || connectivity > (planar ? 2 : 3))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: connectivity %d is not 1, 2%s", connectivity, planar ? " (a planar structure has no third axis)" : " or 3");
  if (iterations < 1 || iterations > UNET_VOL_MORPH_MAX_ITERATIONS) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: %d iterations are outside 1..%d", iterations, UNET_VOL_MORPH_MAX_ITERATIONS);
  if (border_value != 0 && border_value != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: border_value %d is not 0 or 1", border_value);
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!mask || !out || !ws) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: bad args");
  if (vol_overlap(mask, (size_t)d.N, out, (size_t)d.N)) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: out must not be (or overlap) the mask's buffer");
  if (ws_bytes < unet_vol_morph_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: workspace too small or not 16-byte aligned");
  if (counts && !vol_aligned(counts, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_morph: counts is not 8-byte aligned");
  hipStream_t s = as_stream(stream);
  u64* cur = static_cast<u64*>(ws);
  u64* nxt = reinterpret_cast<u64*>(static_cast<uint8_t*>(ws) + vol_bits_layout_of(d, 2).plane);
  if (counts) UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)Z * sizeof(int64_t), s));
  const unsigned pack_blocks = vol_blocks(d.words * 4, GRID_CAP, TPB);
  if ((X % 16) == 0 && vol_aligned(mask, 16)) hipLaunchKernelGGL(morph_pack_kernel<true>, dim3(pack_blocks), dim3(TPB), 0, s, mask, d, cur);
  else hipLaunchKernelGGL(morph_pack_kernel<false>, dim3(pack_blocks), dim3(TPB), 0, s, mask, d, cur);
  const u64 fill = border_value ? ~0ull : 0ull;
  const bool first_dilates = op == UNET_MORPH_DILATE || op == UNET_MORPH_CLOSE;
  const int phases = (op == UNET_MORPH_OPEN || op == UNET_MORPH_CLOSE) ? 2 : 1;
  for (int ph = 0; ph < phases; ++ph) {
    const bool dilate = (ph == 0) == first_dilates;
    for (int it = 0; it < iterations; ++it) {
      if (dilate) hipLaunchKernelGGL(morph_step_kernel<true>, dim3(vol_blocks(d.words, GRID_CAP, TPB)), dim3(TPB), 0, s, cur, d, connectivity, planar ? 1 : 0, fill, nxt);
      else hipLaunchKernelGGL(morph_step_kernel<false>, dim3(vol_blocks(d.words, GRID_CAP, TPB)), dim3(TPB), 0, s, cur, d, connectivity, planar ? 1 : 0, fill, nxt);
      u64* t = cur; cur = nxt; nxt = t;
    }
  }
  const int bps = slice_blocks((long long)Y * d.WX * 4, TPB);
  u64* cnt = reinterpret_cast<u64*>(counts);
  if ((X % 16) == 0 && vol_aligned(out, 16)) hipLaunchKernelGGL(morph_unpack_kernel<true>, dim3((unsigned)bps * Z), dim3(TPB), 0, s, cur, d, bps, out, cnt);
  else hipLaunchKernelGGL(morph_unpack_kernel<false>, dim3((unsigned)bps * Z), dim3(TPB), 0, s, cur, d, bps, out, cnt);
  UNET_CHECK_LAUNCH(ctx, "vol_morph"); return UNET_OK;
}

int32_t unet_vol_ball(unet_ctx* ctx, const double* d2, int32_t X, int32_t Y, int32_t Z, double r2, int32_t keep_le, uint8_t* out, int64_t* counts, void* stream) {
  if (!ctx) UNET_FAIL(ctx, UNET_E_ARG, "vol_ball: bad args");
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_ball: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  if (!(r2 >= 0.0) || r2 > 1.7976931348623157e308) UNET_FAIL(ctx, UNET_E_ARG, "vol_ball: r2 must be finite and not negative");
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!d2 || !out || !vol_aligned(d2, 8) || (counts && !vol_aligned(counts, 8))) UNET_FAIL(ctx, UNET_E_ARG, "vol_ball: null or misaligned buffer (d2 and counts 8 bytes)");
  if (vol_overlap(d2, (size_t)d.N * sizeof(double), out, (size_t)d.N)) UNET_FAIL(ctx, UNET_E_ARG, "vol_ball: out must not overlap d2");
  hipStream_t s = as_stream(stream);
  if (counts) UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)Z * sizeof(int64_t), s));
  u64* cnt = reinterpret_cast<u64*>(counts);
  const long long XY = (long long)X * Y;
  const bool vec = (XY % 4) == 0 && vol_aligned(d2, 16) && vol_aligned(out, 4);
  const int bps = slice_blocks(XY, vec ? (long long)TPB * 4 : TPB);
  if (vec) hipLaunchKernelGGL(morph_ball_kernel<4>, dim3((unsigned)bps * Z), dim3(TPB), 0, s, d2, XY, bps, r2, keep_le ? 1 : 0, out, cnt);
  else hipLaunchKernelGGL(morph_ball_kernel<1>, dim3((unsigned)bps * Z), dim3(TPB), 0, s, d2, XY, bps, r2, keep_le ? 1 : 0, out, cnt);
  UNET_CHECK_LAUNCH(ctx, "vol_ball"); return UNET_OK;
}

size_t unet_vol_fill_holes_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!vol_dims_ok(X, Y, Z) || (long long)X * Y * Z == 0) return 0;
  return fh_make(X, Y, Z).total;
}

int32_t unet_vol_fill_holes(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, int32_t planar, uint8_t* out, int64_t* counts, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!ctx) UNET_FAIL(ctx, UNET_E_ARG, "vol_fill_holes: bad args");
  if (connectivity < 1 || connectivity > (planar ? 2 : 3))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_fill_holes: connectivity %d is not 1, 2%s", connectivity, planar ? " (a planar structure has no third axis)" : " or 3");
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_fill_holes: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!mask || !out || !ws) UNET_FAIL(ctx, UNET_E_ARG, "vol_fill_holes: bad args");
  if (vol_overlap(mask, (size_t)d.N, out, (size_t)d.N)) UNET_FAIL(ctx, UNET_E_ARG, "vol_fill_holes: out must not be (or overlap) the mask's buffer");
  if (ws_bytes < unet_vol_fill_holes_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_fill_holes: workspace too small or not 16-byte aligned");
  if (counts && !vol_aligned(counts, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_fill_holes: counts is not 8-byte aligned");
  hipStream_t s = as_stream(stream);
  const fh_layout L = fh_make(X, Y, Z);
  uint8_t* base = static_cast<uint8_t*>(ws);
  int32_t* labels = reinterpret_cast<int32_t*>(base + L.labels);
  int32_t* n_dev = reinterpret_cast<int32_t*>(base + L.n);
  uint8_t* touches = base + L.touches;
  const long long tsize = d.N + 1;
  const int32_t rc = k_vol_label(ctx, mask, X, Y, Z, connectivity, planar ? 1 : 0, 1, labels, n_dev, base + L.label_ws, L.total - L.label_ws, s);
  if (rc != UNET_OK) return rc;
  UNET_HIP(ctx, hipMemsetAsync(touches, 0, (size_t)tsize, s));
  if (counts) UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)Z * sizeof(int64_t), s));
  const long long XY = (long long)X * Y, FX = (long long)Y * Z, FY = (long long)X * Z, FZ = planar ? 0 : XY;
  hipLaunchKernelGGL(fh_faces_kernel, dim3(vol_blocks(2 * (FX + FY + FZ), GRID_CAP, TPB)), dim3(TPB), 0, s, labels, d, FX, FY, FZ, tsize, touches);
  u64* cnt = reinterpret_cast<u64*>(counts);
  const bool vec = (XY % 16) == 0 && vol_aligned(out, 16);
  const int bps = slice_blocks(XY, vec ? (long long)TPB * 16 : TPB);
  if (vec) hipLaunchKernelGGL(fh_final_kernel<16>, dim3((unsigned)bps * Z), dim3(TPB), 0, s, labels, touches, tsize, XY, bps, out, cnt);
  else hipLaunchKernelGGL(fh_final_kernel<1>, dim3((unsigned)bps * Z), dim3(TPB), 0, s, labels, touches, tsize, XY, bps, out, cnt);
  UNET_CHECK_LAUNCH(ctx, "vol_fill_holes"); return UNET_OK;
}

}  // extern "C"

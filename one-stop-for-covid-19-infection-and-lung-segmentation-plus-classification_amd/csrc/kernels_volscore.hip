// A mask volume against its ground truth on the device: overlap counts, surfaces, the exact squared Euclidean distance transform with
// anisotropic spacing, the surface-distance reductions and the lesion-wise coverage counts.
//   per-slice tp / fp / fn                                                                                                   unet_vol_confusion
//   m ^ scipy.ndimage.binary_erosion(m, generate_binary_structure(3, c))                                                     unet_vol_surface
//   scipy.ndimage.distance_transform_edt(.., sampling=) squared, as one stated sequence of IEEE double operations              unet_vol_edt_sq
//   count, max d2, sum sqrt(d2) and the d2 values over a surface                                                             unet_vol_surface_distances
//   voxels of every truth lesion the prediction marks, and the other way round                                               unet_vol_lesion_overlap
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, as in kernels_components.hip.
// The distance transform is three launches that run in place in the output: edt_x_kernel (a wave per x line: the integer distance to the nearest feature of the
// line from two scans, stored as fl(wx i^2)), then edt_line_kernel along y and along z: a workgroup holds XT adjacent lines in LDS and every output is the minimum
// over ALL positions l' of its line of fl(g[l'] + fl(w (l - l')^2)) -- an exhaustive scan, so the minimum is the true one and the result is the header's definition
// bit for bit.  The only candidates skipped are those whose g is +inf in every lane of the wave: fl(inf + c) = inf never lowers a minimum.  This file is compiled
// with -ffp-contract=off: a fused multiply-add would round w d^2 + g once instead of twice.
// Phase boundaries are kernel boundaries; no workgroup waits for another one inside a launch; the sums are integers or fixed-shape trees: the same bits on every run.
#include "common.h"
#include "vol_common.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr long long GRID_CAP = 256 * 32;                             // grid-stride launches: 32 workgroups per CU
constexpr int EDT_MAX = UNET_VOL_EDT_MAX_DIM;                        // longest line of the distance transform
constexpr int EDT_TILE = 4096;                                       // doubles of LDS per workgroup of a line pass (32 KiB: four workgroups per CU)
constexpr int XCH = EDT_MAX / 1024;                                  // a lane of the x pass holds 16 voxels of each 1024-voxel chunk of its line
constexpr int SD_GROUPS_CAP = UNET_VOL_SURFDIST_WS_BYTES / 8;        // workgroups (= partial sums) of the surface-distance reduction

inline bool al16(const void* p) { return vol_aligned(p, 16); }

// vol_common.h's vol_block_sum with a barrier in front, so that it can be called back to back on one s_w (kept here: the shared form has no such barrier)
__device__ __forceinline__ long long block_sum_ll(long long v, long long* s_w) {          // -> the sum in every lane; s_w: TPB / 64 words; integer: exact in any order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                                    // (s_w may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  long long t = 0;
#pragma unroll
  for (int w = 0; w < TPB / 64; ++w) t += s_w[w];
  return t;
}
__device__ __forceinline__ unsigned nz16(const uint4& w) {           // bit i: byte i of the 16 is non-zero
  const unsigned ws[4] = {w.x, w.y, w.z, w.w};
  unsigned b = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) b |= ((ws[i >> 2] >> (8 * (i & 3))) & 0xFFu) ? (1u << i) : 0u;
  return b;
}
// bit i: byte base[i] is non-zero, for the i < 16 with lo <= i < hi (hi - lo <= 16; everything else reads nothing)
__device__ __forceinline__ unsigned nz_bytes(const uint8_t* base, int lo, int hi) {
  unsigned b = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) b |= (i >= lo && i < hi && base[i]) ? (1u << i) : 0u;
  return b;
}

// ---- (a) overlap counts: a slice is X * Y contiguous voxels; V = 16: two 16-byte loads per lane ---------------------------------------------------
template <int V>
__global__ __launch_bounds__(TPB) void vs_confusion_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, long long XY, int bps,
                                                          unsigned long long* __restrict__ out) {
  __shared__ long long s_w[TPB / 64];
  const int z = blockIdx.x / bps, part = blockIdx.x - z * bps;
  const long long base = (long long)z * XY;
  int tp = 0, fp = 0, fn = 0;
  for (long long i = ((long long)part * TPB + threadIdx.x) * V; i < XY; i += (long long)bps * TPB * V) {
    unsigned p, t;
    if constexpr (V == 16) {
      p = nz16(*reinterpret_cast<const uint4*>(pred + base + i)); t = nz16(*reinterpret_cast<const uint4*>(truth + base + i));
    } else { p = pred[base + i] ? 1u : 0u; t = truth[base + i] ? 1u : 0u; }
    tp += __popc(p & t); fp += __popc(p & ~t); fn += __popc(t & ~p);
  }
  const long long a = block_sum_ll(tp, s_w), b = block_sum_ll(fp, s_w), c = block_sum_ll(fn, s_w);
  if (threadIdx.x == 0) {
    if (a) atomicAdd(out + 3 * z, (unsigned long long)a);
    if (b) atomicAdd(out + 3 * z + 1, (unsigned long long)b);
    if (c) atomicAdd(out + 3 * z + 2, (unsigned long long)c);
  }
}

// ---- (b) surface: 16 voxels along x per lane -----------------------------------------------------------------------------------------------------
// 18 bits of one x row: bit j is voxel x0 - 1 + j; everything outside the volume is background
__device__ __forceinline__ unsigned row18(const uint8_t* __restrict__ mask, int X, int Y, int Z, int x0, int y, int z, bool vec) {
  if (y < 0 || y >= Y || z < 0 || z >= Z) return 0u;
  const uint8_t* row = mask + (long long)X * (y + (long long)Y * z);
  unsigned mid;
  if (vec) mid = nz16(*reinterpret_cast<const uint4*>(row + x0));     // X % 16 == 0: the segment is inside as a whole
  else mid = nz_bytes(row + x0, 0, min(16, X - x0));
  unsigned b = mid << 1;
  if (x0 > 0 && row[x0 - 1]) b |= 1u;
  if (x0 + 16 < X && row[x0 + 16]) b |= 1u << 17;
  return b;
}
__global__ __launch_bounds__(TPB) void vs_surface_kernel(const uint8_t* __restrict__ mask, int X, int Y, int Z, int conn, int vec, uint8_t* __restrict__ surf,
                                                        unsigned long long* __restrict__ count) {
  __shared__ long long s_w[TPB / 64];
  const int segs = (X + 15) / 16;
  const long long items = (long long)segs * Y * Z;
  int cnt = 0;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < items; i += (long long)gridDim.x * TPB) {
    const int seg = (int)(i % segs); const long long r = i / segs;
    const int y = (int)(r % Y), z = (int)(r / Y), x0 = seg * 16;
    const unsigned centre = (row18(mask, X, Y, Z, x0, y, z, vec) >> 1) & 0xFFFFu;
    unsigned inner = centre;                                          // voxels whose whole neighbourhood is foreground
    if (centre) {
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
          const int moved = (dy != 0) + (dz != 0);                    // an offset belongs to connectivity c when it moves along at most c axes
          if (moved > conn) continue;
          const unsigned b = row18(mask, X, Y, Z, x0, y + dy, z + dz, vec);
          unsigned all = b >> 1;                                      // dx = 0
          if (moved + 1 <= conn) all &= b & (b >> 2);                 // dx = -1, +1
          inner &= all;
        }
    }
    const unsigned s = centre & ~inner & 0xFFFFu;
    cnt += __popc(s);
    uint8_t* out = surf + (long long)X * (y + (long long)Y * z) + x0;
    if (vec) {
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = ((s >> (4 * j)) & 1u) | (((s >> (4 * j + 1)) & 1u) << 8) | (((s >> (4 * j + 2)) & 1u) << 16) | (((s >> (4 * j + 3)) & 1u) << 24);
      *reinterpret_cast<uint4*>(out) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      const int n = min(16, X - x0);
      for (int k = 0; k < n; ++k) out[k] = (uint8_t)((s >> k) & 1u);
    }
  }
  const long long t = block_sum_ll(cnt, s_w);
  if (threadIdx.x == 0 && t) atomicAdd(count, (unsigned long long)t);
}

// ---- (c) distance transform ----------------------------------------------------------------------------------------------------------------------
// x pass: a wave per line (y, z).  Lane l holds voxels [1024 c + 16 l, + 16) of every chunk c; the last feature at or before a voxel comes from a max-scan over the
// lanes and a carry over the chunks, the first one at or after it from the mirrored min-scan.  out[v] = fl(wx i^2), i the smaller of the two distances; +inf
// on a line without features.
constexpr int NONE_L = -0x40000000, NONE_R = 0x40000000, FAR = 0x20000000;
__global__ __launch_bounds__(TPB) void edt_x_kernel(const uint8_t* __restrict__ vol, int X, long long lines, int nonzero, int vec, double wx, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long line = (long long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (line >= lines) return;                                          // wave-uniform
  const uint8_t* row = vol + line * X;
  double* orow = out + line * X;
  unsigned fb[XCH]; int prevL[XCH], nextR[XCH];
  const unsigned flip = nonzero ? 0u : 0xFFFFu;
#pragma unroll
  for (int c = 0; c < XCH; ++c) {
    const int x0 = c * 1024 + lane * 16;
    fb[c] = 0;
    if (x0 < X) {
      const int n = min(16, X - x0);
      const unsigned nz = vec ? nz16(*reinterpret_cast<const uint4*>(row + x0)) : nz_bytes(row + x0, 0, n);
      fb[c] = (nz ^ flip) & (n == 16 ? 0xFFFFu : ((1u << n) - 1u));
    }
  }
  int carry = NONE_L;
#pragma unroll
  for (int c = 0; c < XCH; ++c) {
    const int x0 = c * 1024 + lane * 16;
    int inc = fb[c] ? x0 + 31 - __clz((int)fb[c]) : NONE_L;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc = max(inc, t); }
    const int before = __shfl_up(inc, 1, 64);
    prevL[c] = max(lane ? before : NONE_L, carry);
    carry = max(carry, __shfl(inc, 63, 64));
  }
  carry = NONE_R;
#pragma unroll
  for (int c = XCH - 1; c >= 0; --c) {
    const int x0 = c * 1024 + lane * 16;
    int inc = fb[c] ? x0 + __ffs((int)fb[c]) - 1 : NONE_R;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(inc, o, 64); if (lane + o < 64) inc = min(inc, t); }
    const int after = __shfl_down(inc, 1, 64);
    nextR[c] = min(lane < 63 ? after : NONE_R, carry);
    carry = min(carry, __shfl(inc, 0, 64));
  }
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
#pragma unroll
  for (int c = 0; c < XCH; ++c) {
    const int x0 = c * 1024 + lane * 16;
    if (x0 >= X) continue;
    int dist[16];
    int last = prevL[c];
#pragma unroll
    for (int i = 0; i < 16; ++i) { if ((fb[c] >> i) & 1u) last = x0 + i; dist[i] = x0 + i - last; }
    int next = nextR[c];
#pragma unroll
    for (int i = 15; i >= 0; --i) { if ((fb[c] >> i) & 1u) next = x0 + i; dist[i] = min(dist[i], next - (x0 + i)); }
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { const double dd = (double)dist[i]; v[i] = dist[i] >= FAR ? inf : wx * (dd * dd); }          // dd * dd is an exact integer: one rounding
    if (vec) {                                                        // X % 16 == 0 and out 16-byte aligned
#pragma unroll
      for (int i = 0; i < 16; i += 2) *reinterpret_cast<double2*>(orow + x0 + i) = make_double2(v[i], v[i + 1]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) if (x0 + i < X) orow[x0 + i] = v[i];
    }
  }
}

// line pass along an axis of length L whose elements are A apart: element (a, l, b) sits at a + A (l + L b).  The y pass has A = X, b = z; the z pass A = X Y, b = 0.
// A workgroup owns the XT (a power of two, XT L <= EDT_TILE) lines a0 .. a0 + XT - 1 of one b: it reads them all into LDS before it writes any of them back.
constexpr int EDT_R = 4;                                             // outputs per lane that share one LDS read
__global__ __launch_bounds__(TPB) void edt_line_kernel(double* __restrict__ d2, long long A, int L, int xt_log, long long tiles, double w) {
  __shared__ double g[EDT_TILE];
  const int XT = 1 << xt_log;
  const long long b = blockIdx.x / tiles, a0 = (blockIdx.x - b * tiles) << xt_log;
  double* base = d2 + A * (long long)L * b + a0;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  for (int i = threadIdx.x; i < (L << xt_log); i += TPB) {
    const int l = i >> xt_log, xl = i & (XT - 1);
    g[i] = a0 + xl < A ? base[A * l + xl] : inf;
  }
  __syncthreads();
  const int xl = threadIdx.x & (XT - 1), row = threadIdx.x >> xt_log, rows = TPB >> xt_log;
  if (a0 + xl >= A) return;                                           // (no barrier below)
  for (int l0 = 0; l0 < L; l0 += EDT_R * rows) {                      // wave-uniform trip count
    double pos[EDT_R], m[EDT_R];
#pragma unroll
    for (int r = 0; r < EDT_R; ++r) { pos[r] = (double)(l0 + row + r * rows); m[r] = inf; }
    double lp = 0.0;
    for (int l2 = 0; l2 < L; ++l2, lp += 1.0) {
      const double gv = g[(l2 << xt_log) + xl];
      if (__ballot(gv < inf) == 0ull) continue;                       // inf + c = inf lowers no minimum
#pragma unroll
      for (int r = 0; r < EDT_R; ++r) {
        const double dl = pos[r] - lp;                                // exact integers
        const double cand = gv + w * (dl * dl);                       // fl(g + fl(w d^2)); dl * dl is exact
        m[r] = cand < m[r] ? cand : m[r];
      }
    }
#pragma unroll
    for (int r = 0; r < EDT_R; ++r) {
      const int l = l0 + row + r * rows;
      if (l < L) base[A * l + xl] = m[r];
    }
  }
}

__global__ __launch_bounds__(TPB) void vs_sqrt_kernel(double* __restrict__ x, long long n) {
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) x[i] = sqrt(x[i]);
}

// ---- (d) surface distances --------------------------------------------------------------------------------------------------------------------------
// Reduction shape of sum sqrt(d2) (include/unet_hip.h repeats it; tests derive their bound from it).  items = ceil(N / 16) groups of 16 voxels, G = min(ceil(items / 256),
// SD_GROUPS_CAP) workgroups of 256 lanes.  A lane adds its groups k = 0, 1, .. (group index (k G + workgroup) 256 + lane) voxel by voxel into one double: a chain
// of at most 16 ceil(items / (256 G)) additions; then a 6-level butterfly over the 64 lanes of its wave, then the four wave sums left to right (3 additions).  The second
// launch is ONE workgroup: lane t adds the partial sums t, t + 256, .. (a chain of ceil(G / 256)), the same butterfly, the same three additions.
// (kept here and not vol_common.h's vol_block_sum: the wave sums are added from s_w[0], not from 0.0, and that order is the documented one)
__device__ __forceinline__ double block_sum_f64(double v, double* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);        // both partners compute a + b: the same bits in every lane
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
__global__ __launch_bounds__(TPB) void vs_surfdist_kernel(const uint8_t* __restrict__ surf, const double* __restrict__ d2, long long N, int vec, long long cap,
                                                         unsigned long long* __restrict__ res, double* __restrict__ gathered, double* __restrict__ partial) {
  __shared__ double s_w[TPB / 64];
  __shared__ unsigned long long s_m[TPB / 64];
  const long long items = (N + 15) / 16;
  const int lane = threadIdx.x & 63;
  double sum = 0.0;
  unsigned long long mx = 0;                                          // non-negative doubles (and +inf) order like their bit patterns
  for (long long i0 = (long long)blockIdx.x * TPB + (threadIdx.x - lane); i0 < items; i0 += (long long)gridDim.x * TPB) {          // wave-uniform trip count
    const long long i = i0 + lane, f0 = 16 * i;
    unsigned s = 0;
    if (i < items) {
      const int n = (int)min(16LL, N - f0);
      s = (vec && n == 16) ? nz16(*reinterpret_cast<const uint4*>(surf + f0)) : nz_bytes(surf + f0, 0, n);
    }
    const int mine = __popc(s);
    int incl = mine;                                                  // one slot range per wave: a prefix sum over the lanes, one atomic by the last lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    const int total = __shfl(incl, 63, 64);
    if (total == 0) continue;
    unsigned long long start = 0;
    if (lane == 63) start = atomicAdd(res, (unsigned long long)total);
    start = __shfl(start, 63, 64);
    long long slot = (long long)start + incl - mine;
    for (unsigned rest = s; rest; rest &= rest - 1) {
      const double v = d2[f0 + __ffs((int)rest) - 1];
      sum += sqrt(v);
      const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
      mx = bits > mx ? bits : mx;
      if (slot < cap) gathered[slot] = v;
      ++slot;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(mx, o, 64); mx = t > mx ? t : mx; }
  if (lane == 0) s_m[threadIdx.x >> 6] = mx;
  const double t = block_sum_f64(sum, s_w);                           // (its barrier also publishes s_m)
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = t;
    unsigned long long m = s_m[0];
    for (int k = 1; k < TPB / 64; ++k) m = s_m[k] > m ? s_m[k] : m;
    if (m) atomicMax(res + 1, m);
  }
}
__global__ __launch_bounds__(TPB) void vs_surfdist_fold_kernel(const double* __restrict__ partial, int G, double* __restrict__ sum_out) {
  __shared__ double s_w[TPB / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < G; i += TPB) s += partial[i];
  const double t = block_sum_f64(s, s_w);
  if (threadIdx.x == 0) *sum_out = t;
}

// ---- (e) lesion coverage ------------------------------------------------------------------------------------------------------------------------------
// table[label - 1] += cnt for the lanes with label != 0: two rounds in which the lanes that hold the first pending lane's label are summed with shuffles and sent as
// one atomic (a wave inside one lesion, or on the border of two), the rest per lane.  Called by whole waves.
__device__ __forceinline__ void wave_count(int label, int cnt, unsigned long long* table) {
  const int lane = threadIdx.x & 63;
  for (int round = 0; round < 2; ++round) {
    const unsigned long long pending = __ballot(label != 0);
    if (!pending) return;
    const int leader = __ffsll((long long)pending) - 1;
    const int L = __shfl(label, leader, 64);
    const bool part = label == L;
    int c = part ? cnt : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == leader) atomicAdd(table + (L - 1), (unsigned long long)c);
    if (part) label = 0;
  }
  if (label != 0) atomicAdd(table + (label - 1), (unsigned long long)cnt);
}
// four voxels per lane; own = the labels being counted (1..n), other = the partner volume (any non-zero value marks)
__device__ __forceinline__ void cover_quad(const int* own, const int* other, int n, unsigned long long* table) {
  int label = 0, cnt = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (other[i] == 0 || (unsigned)(own[i] - 1) >= (unsigned)n) continue;          // a label outside 1..n is ignored, never an address
    if (label == 0) label = own[i];
    if (own[i] == label) ++cnt;
    else atomicAdd(table + (own[i] - 1), 1ull);
  }
  wave_count(label, cnt, table);
}
__global__ __launch_bounds__(TPB) void vs_overlap_kernel(const int32_t* __restrict__ lt, const int32_t* __restrict__ lp, long long N, int nt, int np, int vec,
                                                        unsigned long long* __restrict__ cover_t, unsigned long long* __restrict__ cover_p) {
  const long long quads = (N + 3) / 4;
  const int lane = threadIdx.x & 63;
  for (long long q0 = (long long)blockIdx.x * TPB + (threadIdx.x - lane); q0 < quads; q0 += (long long)gridDim.x * TPB) {          // wave-uniform trip count
    const long long q = q0 + lane, f0 = 4 * q;
    int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (q < quads) {
      if (vec && f0 + 3 < N) {
        const int4 u = *reinterpret_cast<const int4*>(lt + f0), v = *reinterpret_cast<const int4*>(lp + f0);
        a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w; b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
      } else for (int i = 0; f0 + i < N && i < 4; ++i) { a[i] = lt[f0 + i]; b[i] = lp[f0 + i]; }
    }
    cover_quad(a, b, nt, cover_t);
    cover_quad(b, a, np, cover_p);
  }
}
}  // namespace

extern "C" {

int32_t unet_vol_confusion(unet_ctx* ctx, const uint8_t* pred, const uint8_t* truth, int32_t X, int32_t Y, int32_t Z, int64_t* counts, void* stream) {
  if (!ctx || !vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_confusion: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  const long long XY = (long long)X * Y, N = XY * Z;
  if (Z == 0) return UNET_OK;
  if (!counts) UNET_FAIL(ctx, UNET_E_ARG, "vol_confusion: bad args");
  hipStream_t s = as_stream(stream);
  if (N == 0) { UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)Z * 3 * sizeof(int64_t), s)); return UNET_OK; }
  if (!pred || !truth) UNET_FAIL(ctx, UNET_E_ARG, "vol_confusion: bad args");
  UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)Z * 3 * sizeof(int64_t), s));
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  const bool vec = (XY % 16) == 0 && al16(pred) && al16(truth);
  const long long per = vec ? (long long)TPB * 16 : TPB;
  long long bps = (XY + per - 1) / per;
  bps = bps > 64 ? 64 : bps;
  if (vec) hipLaunchKernelGGL(vs_confusion_kernel<16>, dim3((unsigned)(bps * Z)), dim3(TPB), 0, s, pred, truth, XY, (int)bps, out);
  else hipLaunchKernelGGL(vs_confusion_kernel<1>, dim3((unsigned)(bps * Z)), dim3(TPB), 0, s, pred, truth, XY, (int)bps, out);
  UNET_CHECK_LAUNCH(ctx, "vol_confusion"); return UNET_OK;
}

int32_t unet_vol_surface(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, uint8_t* surface, int64_t* count, void* stream) {
  if (!ctx || !count) UNET_FAIL(ctx, UNET_E_ARG, "vol_surface: bad args");
  if (connectivity < 1 || connectivity > 3) UNET_FAIL(ctx, UNET_E_ARG, "vol_surface: connectivity %d is not 1 (6 neighbours), 2 (18) or 3 (26)", connectivity);
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_surface: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  hipStream_t s = as_stream(stream);
  const long long N = (long long)X * Y * Z;
  if (N == 0) { UNET_HIP(ctx, hipMemsetAsync(count, 0, sizeof(int64_t), s)); return UNET_OK; }
  if (!mask || !surface || mask == surface) UNET_FAIL(ctx, UNET_E_ARG, "vol_surface: null buffer, or the surface would overwrite the mask it is read from");
  UNET_HIP(ctx, hipMemsetAsync(count, 0, sizeof(int64_t), s));
  const int vec = (X % 16) == 0 && al16(mask) && al16(surface);
  const long long items = (long long)((X + 15) / 16) * Y * Z;
  hipLaunchKernelGGL(vs_surface_kernel, dim3(vol_blocks(items, GRID_CAP, TPB)), dim3(TPB), 0, s, mask, X, Y, Z, connectivity, vec, surface,
                     reinterpret_cast<unsigned long long*>(count));
  UNET_CHECK_LAUNCH(ctx, "vol_surface"); return UNET_OK;
}

size_t unet_vol_edt_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  (void)X; (void)Y; (void)Z;
  return 0;                                                           // the three passes run in place in d2
}

int32_t unet_vol_edt_sq(unet_ctx* ctx, const uint8_t* vol, int32_t X, int32_t Y, int32_t Z, int32_t features_nonzero, const double* w, double* d2, void* ws, size_t ws_bytes,
                        void* stream) {
  (void)ws;
  if (!ctx || !w) UNET_FAIL(ctx, UNET_E_ARG, "vol_edt_sq: bad args");
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_edt_sq: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  if (X > EDT_MAX || Y > EDT_MAX || Z > EDT_MAX) UNET_FAIL(ctx, UNET_E_ARG, "vol_edt_sq: %d x %d x %d has a dimension above %d", X, Y, Z, EDT_MAX);
  for (int k = 0; k < 3; ++k)
    if (!(w[k] > 0.0) || !std::isfinite(w[k])) UNET_FAIL(ctx, UNET_E_ARG, "vol_edt_sq: weight %d (a squared spacing) is not positive and finite", k);
  if (ws_bytes < unet_vol_edt_ws_bytes(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_edt_sq: workspace too small");
  const long long N = (long long)X * Y * Z;
  if (N == 0) return UNET_OK;
  if (!vol || !d2 || (reinterpret_cast<uintptr_t>(d2) % 8) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_edt_sq: null or misaligned buffer");
  hipStream_t s = as_stream(stream);
  const long long lines = (long long)Y * Z;
  const int vec = (X % 16) == 0 && al16(vol) && al16(d2);
  hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)((lines + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, s, vol, X, lines, features_nonzero ? 1 : 0, vec, w[0], d2);
  const long long As[2] = {X, (long long)X * Y}, Bs[2] = {Z, 1};
  const int Ls[2] = {Y, Z};
  for (int p = 0; p < 2; ++p) {
    if (Ls[p] == 1) continue;                                         // the minimum over a line of one element is that element: g + w 0 = g
    int xt_log = 0;
    while (xt_log < 4 && (Ls[p] << (xt_log + 1)) <= EDT_TILE) ++xt_log;
    const long long tiles = (As[p] + (1 << xt_log) - 1) >> xt_log;
    hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)(tiles * Bs[p])), dim3(TPB), 0, s, d2, As[p], Ls[p], xt_log, tiles, w[p + 1]);
  }
  UNET_CHECK_LAUNCH(ctx, "vol_edt_sq"); return UNET_OK;
}

int32_t unet_vol_sqrt_f64(unet_ctx* ctx, double* x, int64_t n, void* stream) {
  if (!ctx || n < 0 || (n > 0 && !x)) UNET_FAIL(ctx, UNET_E_ARG, "vol_sqrt_f64: bad args");
  if (n == 0) return UNET_OK;
  hipLaunchKernelGGL(vs_sqrt_kernel, dim3(vol_blocks(n, GRID_CAP, TPB)), dim3(TPB), 0, as_stream(stream), x, (long long)n);
  UNET_CHECK_LAUNCH(ctx, "vol_sqrt_f64"); return UNET_OK;
}

int32_t unet_vol_surface_distances(unet_ctx* ctx, const uint8_t* surface, const double* d2, int32_t X, int32_t Y, int32_t Z, void* result, double* gathered, int64_t capacity,
                                   void* ws, size_t ws_bytes, void* stream) {
  if (!ctx || !result || capacity < 0 || (capacity > 0 && !gathered) || (reinterpret_cast<uintptr_t>(result) % 8) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_surface_distances: bad args");
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_surface_distances: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  hipStream_t s = as_stream(stream);
  const long long N = (long long)X * Y * Z;
  if (N == 0) { UNET_HIP(ctx, hipMemsetAsync(result, 0, 24, s)); return UNET_OK; }
  if (!surface || !d2 || !ws || ws_bytes < UNET_VOL_SURFDIST_WS_BYTES || (reinterpret_cast<uintptr_t>(ws) % 8) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_surface_distances: null buffer, or a workspace below UNET_VOL_SURFDIST_WS_BYTES");
  UNET_HIP(ctx, hipMemsetAsync(result, 0, 24, s));
  const long long items = (N + 15) / 16;
  const int G = (int)vol_blocks(items, SD_GROUPS_CAP, TPB);
  unsigned long long* res = static_cast<unsigned long long*>(result);
  double* partial = static_cast<double*>(ws);
  hipLaunchKernelGGL(vs_surfdist_kernel, dim3((unsigned)G), dim3(TPB), 0, s, surface, d2, N, al16(surface) ? 1 : 0, (long long)capacity, res, gathered, partial);
  hipLaunchKernelGGL(vs_surfdist_fold_kernel, dim3(1), dim3(TPB), 0, s, partial, G, reinterpret_cast<double*>(res + 2));
  UNET_CHECK_LAUNCH(ctx, "vol_surface_distances"); return UNET_OK;
}

int32_t unet_vol_lesion_overlap(unet_ctx* ctx, const int32_t* labels_t, int32_t n_t, const int32_t* labels_p, int32_t n_p, int32_t X, int32_t Y, int32_t Z, int64_t* cover_t,
                                int64_t* cover_p, void* stream) {
  if (!ctx || n_t < 0 || n_p < 0 || !vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_lesion_overlap: bad args");
  if ((n_t > 0 && !cover_t) || (n_p > 0 && !cover_p)) UNET_FAIL(ctx, UNET_E_ARG, "vol_lesion_overlap: bad args");
  hipStream_t s = as_stream(stream);
  const long long N = (long long)X * Y * Z;
  if (N > 0 && n_t > 0 && n_p > 0 && (!labels_t || !labels_p)) UNET_FAIL(ctx, UNET_E_ARG, "vol_lesion_overlap: bad args");
  if (n_t > 0) UNET_HIP(ctx, hipMemsetAsync(cover_t, 0, (size_t)n_t * sizeof(int64_t), s));
  if (n_p > 0) UNET_HIP(ctx, hipMemsetAsync(cover_p, 0, (size_t)n_p * sizeof(int64_t), s));
  if (N == 0 || n_t == 0 || n_p == 0) return UNET_OK;                  // nothing can overlap
  const int vec = al16(labels_t) && al16(labels_p);
  hipLaunchKernelGGL(vs_overlap_kernel, dim3(vol_blocks((N + 3) / 4, GRID_CAP, TPB)), dim3(TPB), 0, s, labels_t, labels_p, N, n_t, n_p, vec,
                     reinterpret_cast<unsigned long long*>(cover_t), reinterpret_cast<unsigned long long*>(cover_p));
  UNET_CHECK_LAUNCH(ctx, "vol_lesion_overlap"); return UNET_OK;
}

}  // extern "C"

// A lung mask from the CT itself: the pass that turns the CT's own voxels into a mask, and the growth from seeds inside a mask that records when
// each voxel was reached.
//   mask[v] = lo <= value(v) < hi (and region[v] != 0), the value decoded as get_fdata() decodes it, + the set voxels of every slice             unet_vol_threshold
//   arrival[v] = the breadth-first step at which the growth from `seeds` inside `constraint` reaches v, + the voxels reached at every step      unet_vol_geodesic_begin / _steps
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, as in kernels_components.hip.
// Threshold: a lane holds eight consecutive voxels -- 16-byte loads of the source (one 8-byte load of a one-byte type), one 8-byte load of the region, one 8-byte store --
// when the buffers are aligned for it, one voxel otherwise (the form of kernels_lungside.hip's side_assign_kernel).  The comparison is on the decoded double,
// (double(raw) * slope) + inter as two rounded operations (-ffp-contract=off); a NaN satisfies neither edge and gives 0.  The slice counts: popcounts (a ballot in the
// one-voxel form), summed per wave by butterflies and per workgroup in LDS, leave as one 64-bit integer atomic per workgroup and trip while the workgroup's voxels lie
// in one slice, and voxel by voxel where a workgroup straddles slices (slices smaller than a trip).  Integer sums: the same bits on every run.
// Growth: vol_common.h's packed layout (vol_bits: one bit per voxel along x, rows padded to 64-bit words; a set holds no bit at or beyond X).  The
// workspace holds four packed volumes: the constraint C, the reached set R and two frontiers F[0], F[1]; step s reads F[(s - 1) & 1] and writes F[s & 1].
//   gd_begin_kernel   bytes -> bits of C and of S = seeds & C (16 voxels per lane, four lanes make a word), R = F[0] = S, arrival = 0 on S and 0xFFFF elsewhere, counts[0]
//   gd_step_kernel    one word per lane: new = dilate(F[(s - 1) & 1]) & C & ~R under the structure of section 4r (x neighbours: a shift with the edge bit of the
//                     adjacent word; y and z neighbours: whole words; outside the volume: 0); F[s & 1] = new, R |= new, arrival = s on the bits of new, counts[s]
// A word with no unreached constraint voxel reads no neighbour.  A lane reads and writes only its own word of R; the frontier it reads is the one the previous launch
// wrote.  No workgroup waits for another: a step boundary is a kernel boundary.  Integer work only: the same bits on every run.
#include "common.h"
#include "vol_common.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr long long GRID_CAP = 256 * 32;                             // grid-stride launches: 32 workgroups per CU
constexpr int TH_VEC = 8;                                            // voxels of a lane in the vector form of the threshold
typedef unsigned long long u64;

// ---- threshold ----------------------------------------------------------------------------------------------------------------------------------
struct th_args { int scaled; double slope, inter, lo, hi; };
template <typename T>
__device__ __forceinline__ unsigned th_bit(T raw, const th_args& a) {
  double v = (double)raw;
  if (a.scaled) v = __dadd_rn(__dmul_rn(v, a.slope), a.inter);
  return (a.lo <= v && v < a.hi) ? 1u : 0u;                           // a NaN fails both
}
template <typename T>
__device__ __forceinline__ void th_load8(const T* p, T (&e)[TH_VEC]) {          // p is aligned to min(16, 8 sizeof(T)) bytes
  if constexpr (sizeof(T) == 1) {
    const uint2 w = *reinterpret_cast<const uint2*>(p);
    __builtin_memcpy(e, &w, 8);
  } else {
    constexpr int Q = (int)sizeof(T) / 2;                             // 16-byte loads
    uint4 w[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) w[q] = reinterpret_cast<const uint4*>(p)[q];
    __builtin_memcpy(e, w, 16 * Q);
  }
}

// VEC: item g = voxels [8 g, 8 g + 8) (the last item may be short: it goes voxel by voxel); otherwise item g = voxel g.  The trip count is uniform over the workgroup.
template <typename T, bool VEC>
__global__ __launch_bounds__(TPB) void th_threshold_kernel(const T* __restrict__ vox, th_args a, const uint8_t* __restrict__ region, long long N, long long XY,
                                                          uint8_t* __restrict__ mask, u64* __restrict__ slice_counts) {
  constexpr int V = VEC ? TH_VEC : 1;
  __shared__ int s_w[TPB / 64];
  const int tid = threadIdx.x;
  const long long items = (N + V - 1) / V;
  for (long long g0 = (long long)blockIdx.x * TPB; g0 < items; g0 += (long long)gridDim.x * TPB) {
    const long long g = g0 + tid, v0 = g * V;
    unsigned bits = 0;                                                // bit k: voxel v0 + k is set
    if (g < items) {
      if constexpr (VEC) {
        if (v0 + V <= N) {
          T e[V];
          th_load8(vox + v0, e);
#pragma unroll
          for (int k = 0; k < V; ++k) bits |= th_bit(e[k], a) << k;
          if (region) {
            const uint2 r = *reinterpret_cast<const uint2*>(region + v0);
#pragma unroll
            for (int k = 0; k < V; ++k) if ((((k < 4 ? r.x : r.y) >> (8 * (k & 3))) & 0xFFu) == 0) bits &= ~(1u << k);
          }
          uint2 o;
          o.x = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);
          o.y = ((bits >> 4) & 1u) | ((bits & 32u) << 3) | ((bits & 64u) << 10) | ((bits & 128u) << 17);
          *reinterpret_cast<uint2*>(mask + v0) = o;
        } else {
          for (int k = 0; k < V; ++k)
            if (v0 + k < N) {
              const unsigned b = (!region || region[v0 + k]) ? th_bit(vox[v0 + k], a) : 0u;
              mask[v0 + k] = (uint8_t)b;
              bits |= b << k;
            }
        }
      } else {
        bits = (!region || region[g]) ? th_bit(vox[g], a) : 0u;
        mask[g] = (uint8_t)bits;
      }
    }
    if (slice_counts) {                                               // (uniform over the launch)
      const long long first = g0 * V, end = (g0 + TPB) * V < N ? (g0 + TPB) * V : N;          // the workgroup's voxels of this trip: [first, end), first < N
      const long long zb = first / XY;
      if ((end - 1) / XY == zb) {                                     // (uniform over the workgroup) one slice: one atomic
        int c;
        if constexpr (VEC) c = __popc(bits);
        else { const u64 set = __ballot(bits != 0); c = (tid & 63) == 0 ? (int)__popcll(set) : 0; }
        const int t = vol_block_sum<int, TPB>(c, s_w);
        if (tid == 0 && t) atomicAdd(slice_counts + zb, (u64)t);
        __syncthreads();                                              // s_w is written again on the next trip
      } else {
        for (unsigned b = bits; b; b &= b - 1) atomicAdd(slice_counts + (v0 + (__ffs((int)b) - 1)) / XY, 1ull);
      }
    }
  }
}

template <typename T>
void th_launch(hipStream_t s, const void* vox, const th_args& a, const uint8_t* region, long long N, long long XY, uint8_t* mask, u64* sc) {
  const T* p = static_cast<const T*>(vox);
  const bool vec = vol_aligned(vox, sizeof(T) == 1 ? 8 : 16) && vol_aligned(mask, 8) && vol_aligned(region, 8);
  if (vec) hipLaunchKernelGGL((th_threshold_kernel<T, true>), dim3(vol_blocks((N + TH_VEC - 1) / TH_VEC, GRID_CAP, TPB)), dim3(TPB), 0, s, p, a, region, N, XY, mask, sc);
  else hipLaunchKernelGGL((th_threshold_kernel<T, false>), dim3(vol_blocks(N, GRID_CAP, TPB)), dim3(TPB), 0, s, p, a, region, N, XY, mask, sc);
}

// ---- growth: the workspace is C | R | F[0] | F[1], `words` 64-bit words each ----------------------------------------------------------------------
// one 16-voxel segment per lane (VEC: X % 16 == 0, so a segment is inside or outside as a whole, and 16-byte accesses); the four lanes of a word join by shuffles
template <bool VEC>
__global__ __launch_bounds__(TPB) void gd_begin_kernel(const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ constraint, vol_bits d, u64* __restrict__ C,
                                                      u64* __restrict__ R, u64* __restrict__ F0, uint16_t* __restrict__ arrival, u64* __restrict__ count0) {
  __shared__ int s_w[TPB / 64];
  const long long segs = d.words * 4;                                 // a multiple of 4: the four lanes of a word are all inside or all outside
  const int lane = threadIdx.x & 63;
  int cnt = 0;
  for (long long t0 = (long long)blockIdx.x * TPB + (threadIdx.x - lane); t0 < segs; t0 += (long long)gridDim.x * TPB) {          // wave-uniform trip count
    const long long t = t0 + lane;
    unsigned cb = 0, sb = 0;
    if (t < segs) {
      const long long w = t >> 2, row = w / d.WX;
      const int x0 = (int)(w - row * d.WX) * 64 + (int)(t & 3) * 16;
      if (x0 < d.X) {
        const long long f = row * d.X + x0;
        if (VEC) {
          cb = vol_bytes_to_bits(*reinterpret_cast<const uint4*>(constraint + f));
          sb = vol_bytes_to_bits(*reinterpret_cast<const uint4*>(seeds + f)) & cb;
          unsigned h[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) h[i] = (((sb >> (2 * i)) & 1u) ? 0u : 0xFFFFu) | (((sb >> (2 * i + 1)) & 1u) ? 0u : 0xFFFF0000u);
          uint4* o = reinterpret_cast<uint4*>(arrival + f);
          o[0] = make_uint4(h[0], h[1], h[2], h[3]);
          o[1] = make_uint4(h[4], h[5], h[6], h[7]);
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (x0 + i < d.X) {
              const unsigned c = constraint[f + i] ? 1u : 0u, sd = (c && seeds[f + i]) ? 1u : 0u;
              cb |= c << i; sb |= sd << i;
              arrival[f + i] = sd ? (uint16_t)0 : (uint16_t)0xFFFF;
            }
        }
      }
    }
    cnt += __popc(sb);
    u64 cv = (u64)cb << (16 * (lane & 3)), sv = (u64)sb << (16 * (lane & 3));
    cv |= __shfl_xor(cv, 1, 64); cv |= __shfl_xor(cv, 2, 64);
    sv |= __shfl_xor(sv, 1, 64); sv |= __shfl_xor(sv, 2, 64);
    if (t < segs && (lane & 3) == 0) { C[t >> 2] = cv; R[t >> 2] = sv; F0[t >> 2] = sv; }
  }
  const int tot = vol_block_sum<int, TPB>(cnt, s_w);
  if (threadIdx.x == 0 && tot) atomicAdd(count0, (u64)tot);           // integer sums: exact in any order
}

// generate_binary_structure(3, conn) holds (dx, dy, dz) when it moves along at most conn axes: a row (dy, dz) with n = (dy != 0) + (dz != 0) <= conn takes part, with its
// x neighbours when n < conn.  planar: only dz = 0.
__global__ __launch_bounds__(TPB) void gd_step_kernel(const u64* __restrict__ C, u64* __restrict__ R, const u64* __restrict__ Fp, u64* __restrict__ Fn, vol_bits d, int conn,
                                                     int planar, unsigned step, uint16_t* __restrict__ arrival, u64* __restrict__ count) {
  __shared__ int s_w[TPB / 64];
  const int zr = planar ? 0 : 1;
  int cnt = 0;
  for (long long w = (long long)blockIdx.x * TPB + threadIdx.x; w < d.words; w += (long long)gridDim.x * TPB) {
    const u64 reached = R[w], avail = C[w] & ~reached;
    u64 got = 0;
    if (avail) {
      const long long row = w / d.WX;
      const int wi = (int)(w - row * d.WX), z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
      u64 acc = 0;
      for (int dz = -zr; dz <= zr; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
          const int n = (dy != 0) + (dz != 0);
          if (n > conn) continue;
          const u64 c = vol_bits_load(Fp, d, wi, y + dy, z + dz);
          u64 t = c;
          if (n < conn) {
            const u64 lo = vol_bits_load(Fp, d, wi - 1, y + dy, z + dz), hi = vol_bits_load(Fp, d, wi + 1, y + dy, z + dz);
            t |= (c << 1) | (lo >> 63) | (c >> 1) | (hi << 63);       // bit x takes voxel x - 1 / voxel x + 1
          }
          acc |= t;
        }
      got = acc & avail;
      if (got) {
        R[w] = reached | got;
        cnt += (int)__popcll(got);
        uint16_t* o = arrival + row * d.X + (long long)wi * 64;
        for (u64 b = got; b; b &= b - 1) o[__ffsll((long long)b) - 1] = (uint16_t)step;
      }
    }
    Fn[w] = got;
  }
  const int tot = vol_block_sum<int, TPB>(cnt, s_w);
  if (threadIdx.x == 0 && tot) atomicAdd(count, (u64)tot);
}
}  // namespace

extern "C" {

int32_t unet_vol_threshold(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, double lo, double hi,
                           const uint8_t* region, uint8_t* mask, int64_t* slice_counts, void* stream) {
  if (!ctx) return UNET_E_ARG;
  const int isz = vol_itemsize(dtype);
  if (!isz) UNET_FAIL(ctx, UNET_E_ARG, "vol_threshold: dtype %d is not a NIfTI element type (2, 256, 4, 512, 8, 768, 16, 64)", dtype);
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_threshold: a dimension is negative or the volume has 2^31 voxels or more");
  if (std::isnan(lo) || std::isnan(hi) || !(lo < hi)) UNET_FAIL(ctx, UNET_E_ARG, "vol_threshold: the edges must satisfy lo < hi and neither is NaN (-inf and +inf are allowed)");
  if (scaled && (std::isnan(slope) || std::isnan(inter))) UNET_FAIL(ctx, UNET_E_ARG, "vol_threshold: NaN scaling");
  const long long XY = (long long)X * Y, N = XY * Z;
  if (N == 0) return UNET_OK;
  if (!vox || !mask || !vol_aligned(vox, (uintptr_t)isz) || !vol_aligned(slice_counts, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_threshold: null or misaligned buffer");
  if (vol_overlap(vox, (size_t)N * isz, mask, (size_t)N) || (region && vol_overlap(region, (size_t)N, mask, (size_t)N)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_threshold: mask must not overlap the voxels or the region");
  hipStream_t s = as_stream(stream);
  if (slice_counts) UNET_HIP(ctx, hipMemsetAsync(slice_counts, 0, (size_t)Z * sizeof(int64_t), s));
  const th_args a{scaled ? 1 : 0, slope, inter, lo, hi};
  u64* sc = reinterpret_cast<u64*>(slice_counts);
  switch (dtype) {
    case 2: th_launch<uint8_t>(s, vox, a, region, N, XY, mask, sc); break;
    case 256: th_launch<int8_t>(s, vox, a, region, N, XY, mask, sc); break;
    case 4: th_launch<int16_t>(s, vox, a, region, N, XY, mask, sc); break;
    case 512: th_launch<uint16_t>(s, vox, a, region, N, XY, mask, sc); break;
    case 8: th_launch<int32_t>(s, vox, a, region, N, XY, mask, sc); break;
    case 768: th_launch<uint32_t>(s, vox, a, region, N, XY, mask, sc); break;
    case 16: th_launch<float>(s, vox, a, region, N, XY, mask, sc); break;
    default: th_launch<double>(s, vox, a, region, N, XY, mask, sc); break;
  }
  UNET_CHECK_LAUNCH(ctx, "vol_threshold"); return UNET_OK;
}

size_t unet_vol_geodesic_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!vol_dims_ok(X, Y, Z) || (long long)X * Y * Z == 0) return 0;
  return vol_bits_layout_of(vol_bits_make(X, Y, Z), 4).total;
}

int32_t unet_vol_geodesic_begin(unet_ctx* ctx, const uint8_t* seeds, const uint8_t* constraint, int32_t X, int32_t Y, int32_t Z, uint16_t* arrival, int64_t* counts, void* ws,
                                size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_begin: a dimension is negative or the volume has 2^31 voxels or more");
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!seeds || !constraint || !arrival || !counts || !ws || !vol_aligned(arrival, 2) || !vol_aligned(counts, 8))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_begin: null or misaligned buffer");
  if (ws_bytes < unet_vol_geodesic_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_begin: workspace too small or not 16-byte aligned");
  const vol_bits_layout L = vol_bits_layout_of(d, 4);
  if (vol_overlap(arrival, (size_t)d.N * 2, ws, L.total) || vol_overlap(arrival, (size_t)d.N * 2, seeds, (size_t)d.N) || vol_overlap(arrival, (size_t)d.N * 2, constraint, (size_t)d.N))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_begin: arrival must not overlap the workspace, the seeds or the constraint");
  hipStream_t s = as_stream(stream);
  uint8_t* base = static_cast<uint8_t*>(ws);
  u64 *C = reinterpret_cast<u64*>(base), *R = reinterpret_cast<u64*>(base + L.plane), *F0 = reinterpret_cast<u64*>(base + 2 * L.plane);
  UNET_HIP(ctx, hipMemsetAsync(counts, 0, sizeof(int64_t), s));
  const unsigned blocks = vol_blocks(d.words * 4, GRID_CAP, TPB);
  if ((X % 16) == 0 && vol_aligned(seeds, 16) && vol_aligned(constraint, 16) && vol_aligned(arrival, 16))
    hipLaunchKernelGGL(gd_begin_kernel<true>, dim3(blocks), dim3(TPB), 0, s, seeds, constraint, d, C, R, F0, arrival, reinterpret_cast<u64*>(counts));
  else
    hipLaunchKernelGGL(gd_begin_kernel<false>, dim3(blocks), dim3(TPB), 0, s, seeds, constraint, d, C, R, F0, arrival, reinterpret_cast<u64*>(counts));
  UNET_CHECK_LAUNCH(ctx, "vol_geodesic_begin"); return UNET_OK;
}

int32_t unet_vol_geodesic_steps(unet_ctx* ctx, int32_t X, int32_t Y, int32_t Z, int32_t first_step, int32_t n_steps, int32_t connectivity, int32_t planar, uint16_t* arrival,
                                int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_steps: a dimension is negative or the volume has 2^31 voxels or more");
  if (planar != 0 && planar != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_steps: planar %d is not 0 or 1", planar);
  if (connectivity < 1 || connectivity > (planar ? 2 : 3))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_steps: connectivity %d is not 1, 2%s", connectivity, planar ? " (a planar structure has no third axis)" : " or 3");
  if (first_step < 1 || n_steps < 1 || (long long)first_step + n_steps - 1 > UNET_VOL_GEODESIC_MAX_STEP)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_steps: steps %d .. %lld are not inside 1 .. %d", first_step, (long long)first_step + n_steps - 1, UNET_VOL_GEODESIC_MAX_STEP);
  const vol_bits d = vol_bits_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!arrival || !counts || !ws || !vol_aligned(arrival, 2) || !vol_aligned(counts, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_steps: null or misaligned buffer");
  if (ws_bytes < unet_vol_geodesic_ws_bytes(X, Y, Z) || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_steps: workspace too small or not 16-byte aligned");
  const vol_bits_layout L = vol_bits_layout_of(d, 4);
  if (vol_overlap(arrival, (size_t)d.N * 2, ws, L.total)) UNET_FAIL(ctx, UNET_E_ARG, "vol_geodesic_steps: arrival must not overlap the workspace");
  hipStream_t s = as_stream(stream);
  uint8_t* base = static_cast<uint8_t*>(ws);
  u64 *C = reinterpret_cast<u64*>(base), *R = reinterpret_cast<u64*>(base + L.plane);
  u64* F[2] = {reinterpret_cast<u64*>(base + 2 * L.plane), reinterpret_cast<u64*>(base + 3 * L.plane)};
  UNET_HIP(ctx, hipMemsetAsync(counts + first_step, 0, (size_t)n_steps * sizeof(int64_t), s));
  const unsigned blocks = vol_blocks(d.words, GRID_CAP, TPB);
  for (int st = first_step; st < first_step + n_steps; ++st)
    hipLaunchKernelGGL(gd_step_kernel, dim3(blocks), dim3(TPB), 0, s, C, R, F[(st - 1) & 1], F[st & 1], d, connectivity, planar, (unsigned)st, arrival,
                       reinterpret_cast<u64*>(counts) + st);
  UNET_CHECK_LAUNCH(ctx, "vol_geodesic_steps"); return UNET_OK;
}

}  // extern "C"

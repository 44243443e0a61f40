// What the CT holds where a mask is set: the raw NIfTI voxels already on the device, decoded as get_fdata() decodes them, under the groups of a
// label volume (or one mask) and an optional region.
//   voxels per group and value band (np.searchsorted(edges, v, side="right")), per slice and band, exact min / max per group      unet_vol_intensity_bands
//   the taking-part values and their groups, compacted (they are sorted afterwards)                                              unet_vol_intensity_gather
//   (sum, sum of squared deviations) per group of an ordered run, as one stated tree of IEEE double operations                    unet_vol_group_moments
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, as in kernels_components.hip.
// Counting: a lane holds one voxel.  The lanes of a wave that share a (group, band) key are counted with one ballot and their first lane adds the popcount -- to a table in
// LDS while n (B + 1) <= IB_TABLE and n <= IB_GROUPS (a workgroup then leaves one 64-bit atomic per non-zero entry), straight to the output beyond that.  A wave inside one
// lesion and one band costs one add; a wave whose 64 lanes hold 64 groups costs 64: correct either way.  Min / max travel as order-preserving 64-bit keys through integer
// atomicMin / atomicMax (min and max do not round); a lane first reads the entry and skips the atomic when it would not change it (entries only ever move one way, so a stale
// read costs an atomic, never a result).  Integer sums and min / max only: the same bits on every run.
// The moments are a fixed tree over a canonical order (see include/unet_hip.h): 256-element chunks summed left to right by one lane each, the chunk sums left to right by
// one lane per group; no floating-point atomics.  Compiled with -ffp-contract=off: d d + acc must round twice.
#include "common.h"
#include "vol_common.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int MAX_EDGES = UNET_VOL_INTENSITY_MAX_EDGES;
constexpr int IB_TABLE = 4096;                                       // (group, band) counters of a workgroup's LDS table (16 KiB)
constexpr int IB_GROUPS = 1024;                                      // groups whose min / max keys a workgroup holds in LDS (16 KiB)
constexpr int IB_CHUNK = TPB * 16;                                   // voxels of a slice a workgroup takes at a time
constexpr int IB_GRID = 256 * 4;                                     // workgroups of the counting launch: each walks a contiguous range of chunks
constexpr long long GRID_CAP = 256 * 32;
constexpr int MOM_CHUNK = 256;                                       // elements per partial sum of unet_vol_group_moments

struct iv_edges { double e[MAX_EDGES]; int n; };

// ---- (a) bands ------------------------------------------------------------------------------------------------------------------------------------
__global__ void ib_minmax_init_kernel(unsigned long long* __restrict__ keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { keys[2 * i] = ~0ull; keys[2 * i + 1] = 0ull; }
}
__global__ void ib_minmax_final_kernel(unsigned long long* __restrict__ keys, int n) {          // keys -> doubles in place; nothing seen: (+inf, -inf)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long a = keys[2 * i], b = keys[2 * i + 1];
  double* out = reinterpret_cast<double*>(keys);
  out[2 * i] = a == ~0ull ? __longlong_as_double(0x7FF0000000000000ll) : vol_ord2d(a);
  out[2 * i + 1] = b == 0ull ? __longlong_as_double((long long)0xFFF0000000000000ull) : vol_ord2d(b);
}

// LDS_TABLE: the (group, band) counters and the min / max keys of this workgroup live in LDS and leave it once, at the end; otherwise every add goes to the output.
// Chunk c of the launch = IB_CHUNK voxels of one slice (cps chunks per slice); workgroup b walks chunks [b per, (b + 1) per): the slice changes rarely, and the per-slice
// counters leave LDS when it does.  Every loop bound and every barrier below is uniform over the workgroup.
template <bool LDS_TABLE>
__global__ __launch_bounds__(TPB) void ib_bands_kernel(vol_voxels src, vol_groups grp, iv_edges ed, long long XY, int Z, int cps, long long per,
                                                      unsigned long long* __restrict__ band_counts, unsigned long long* __restrict__ slice_counts,
                                                      unsigned long long* __restrict__ minmax) {
  __shared__ int s_tab[LDS_TABLE ? IB_TABLE : 1];
  __shared__ unsigned long long s_mm[LDS_TABLE ? 2 * IB_GROUPS : 2];
  __shared__ int s_slice[MAX_EDGES + 2];
  const int W = ed.n + 2;                                             // columns: B = ed.n + 1 bands, then the NaN count
  const int n = grp.n, tid = threadIdx.x, lane = tid & 63;
  const bool want_mm = minmax != nullptr;
  if constexpr (LDS_TABLE) {
    for (int i = tid; i < n * W; i += TPB) s_tab[i] = 0;
    if (want_mm) for (int i = tid; i < n; i += TPB) { s_mm[2 * i] = ~0ull; s_mm[2 * i + 1] = 0ull; }
  }
  if (tid < W) s_slice[tid] = 0;
  __syncthreads();
  const long long chunks = (long long)cps * Z;
  const long long c0 = (long long)blockIdx.x * per, c1 = min(chunks, c0 + per);
  for (long long c = c0; c < c1; ++c) {
    const int z = (int)(c / cps);
    const long long i0 = (c - (long long)z * cps) * IB_CHUNK, base = (long long)z * XY;
    for (int k = 0; k < IB_CHUNK / TPB; ++k) {
      const long long i = i0 + (long long)k * TPB + tid;
      const int g = i < XY ? vol_group(grp, base + i) : 0;
      unsigned long long pending = __ballot(g != 0);
      if (!pending) continue;                                         // wave-uniform: most waves of a CT lie outside every lesion and never read a voxel
      long long key = -1;                                             // (g - 1) W + band: n W may pass 2^31 beyond the LDS table
      if (g) {
        const double v = vol_dec(src, base + i);
        int band = ed.n + 1;                                          // NaN
        if (v == v) {
          band = 0;
          for (int e = 0; e < ed.n; ++e) band += ed.e[e] <= v ? 1 : 0;          // the number of edges <= v
          if (want_mm) {
            const unsigned long long o = vol_d2ord(v);
            if constexpr (LDS_TABLE) {
              unsigned long long* q = s_mm + 2 * (g - 1);
              if (o < __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMin(q, o);
              if (o > __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(q + 1, o);
            } else {
              unsigned long long* q = minmax + 2 * (long long)(g - 1);
              if (o < __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(q, o);
              if (o > __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(q + 1, o);
            }
          }
        }
        key = (long long)(g - 1) * W + band;
      }
      while (pending) {                                               // one round per distinct key of the wave
        const int leader = __ffsll((long long)pending) - 1;
        const long long K = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == K);
        if (lane == leader) {
          const int cnt = __popcll(same);
          if constexpr (LDS_TABLE) atomicAdd(s_tab + K, cnt);
          else atomicAdd(band_counts + K, (unsigned long long)cnt);
          if (slice_counts) atomicAdd(s_slice + (int)(K % W), cnt);
        }
        pending &= ~same;
      }
    }
    if (slice_counts && (c + 1 == c1 || (int)((c + 1) / cps) != z)) {          // the slice ends here for this workgroup
      __syncthreads();
      if (tid < W) {
        const int v = s_slice[tid];
        if (v) atomicAdd(slice_counts + (long long)z * W + tid, (unsigned long long)v);
        s_slice[tid] = 0;
      }
      __syncthreads();
    }
  }
  if constexpr (LDS_TABLE) {
    __syncthreads();
    for (int i = tid; i < n * W; i += TPB) { const int v = s_tab[i]; if (v) atomicAdd(band_counts + i, (unsigned long long)v); }
    if (want_mm)
      for (int i = tid; i < n; i += TPB) {
        if (s_mm[2 * i] != ~0ull) atomicMin(minmax + 2 * i, s_mm[2 * i]);
        if (s_mm[2 * i + 1] != 0ull) atomicMax(minmax + 2 * i + 1, s_mm[2 * i + 1]);
      }
  }
}

// ---- (b) gather: one slot range per wave from a ballot, one atomic by its first taking-part lane -----------------------------------------------------------
__global__ __launch_bounds__(TPB) void ig_gather_kernel(vol_voxels src, vol_groups grp, long long N, long long cap, double* __restrict__ values, int32_t* __restrict__ groups,
                                                       unsigned long long* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  for (long long i0 = (long long)blockIdx.x * TPB + (threadIdx.x - lane); i0 < N; i0 += (long long)gridDim.x * TPB) {          // wave-uniform trip count
    const long long i = i0 + lane;
    const int g = i < N ? vol_group(grp, i) : 0;
    if (!__ballot(g != 0)) continue;
    double v = 0.0;
    bool take = false;
    if (g) { v = vol_dec(src, i); take = v == v; }
    const unsigned long long m = __ballot(take);
    if (!m) continue;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long start = 0;
    if (lane == leader) start = atomicAdd(count, (unsigned long long)__popcll(m));
    start = __shfl(start, leader, 64);
    if (take) {
      const long long slot = (long long)start + __popcll(m & ((1ull << lane) - 1ull));
      if (slot < cap) { values[slot] = v; if (groups) groups[slot] = g; }
    }
  }
}

// ---- (c) moments ------------------------------------------------------------------------------------------------------------------------------------
// Group g owns the partial-sum slots [off[g] / 256 + g, .. + ceil(m_g / 256)): floor((a + m) / 256) - floor(a / 256) + 1 >= ceil(m / 256), so the ranges never overlap
// and nothing has to be scanned.  slots = off[n] / 256 + n bounds them all.
__device__ __forceinline__ long long mom_slot0(const long long* off, int g) { return off[g] / MOM_CHUNK + g; }
// SQ = false: partial[s] = v[a] + v[a + 1] + ..; SQ = true: the same over fl(d d), d = fl(v - mean[g]); left to right, starting from the first term
template <bool SQ>
__global__ __launch_bounds__(TPB) void mom_chunk_kernel(const double* __restrict__ values, const long long* __restrict__ off, int n, const double* __restrict__ mean,
                                                       double* __restrict__ partial, long long slot_cap) {
  const long long slots = min(mom_slot0(off, n), slot_cap);
  for (long long s = (long long)blockIdx.x * TPB + threadIdx.x; s < slots; s += (long long)gridDim.x * TPB) {
    int lo = 0, hi = n - 1;                                           // the last group whose first slot is <= s
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (mom_slot0(off, mid) <= s) lo = mid; else hi = mid - 1; }
    const long long a0 = off[lo], m = off[lo + 1] - a0, c = s - mom_slot0(off, lo);
    if (c * MOM_CHUNK >= m) continue;                                 // a slot between two groups' ranges
    const long long a = a0 + c * MOM_CHUNK, b = min(a0 + m, a + MOM_CHUNK);
    const double mu = SQ ? mean[lo] : 0.0;
    double acc = 0.0;
    for (long long i = a; i < b; ++i) {
      double t = values[i];
      if (SQ) { const double d = __dsub_rn(t, mu); t = __dmul_rn(d, d); }
      acc = i == a ? t : __dadd_rn(acc, t);
    }
    partial[s] = acc;
  }
}
// one lane per group: the chunk sums left to right.  SQ = false: out[g][0] = sum, mean[g] = sum / m; SQ = true: out[g][1] = ssd.  An empty group: 0.
template <bool SQ>
__global__ __launch_bounds__(TPB) void mom_fold_kernel(const long long* __restrict__ off, int n, const double* __restrict__ partial, long long slot_cap,
                                                      double* __restrict__ mean, double* __restrict__ out) {
  const int g = blockIdx.x * TPB + threadIdx.x;
  if (g >= n) return;
  const long long m = off[g + 1] - off[g], s0 = mom_slot0(off, g), chunks = (m + MOM_CHUNK - 1) / MOM_CHUNK;
  double acc = 0.0;
  for (long long c = 0; c < chunks && s0 + c < slot_cap; ++c) acc = c == 0 ? partial[s0] : __dadd_rn(acc, partial[s0 + c]);
  if (!SQ) { out[2 * g] = acc; mean[g] = m > 0 ? __ddiv_rn(acc, (double)m) : 0.0; }
  else out[2 * g + 1] = acc;
}

// the checks the two volume entry points share -> 0, or the message of the refusal
const char* iv_refusal(int dtype, int X, int Y, int Z, const void* labels, const void* mask, int n) {
  if (!vol_dims_ok(X, Y, Z)) return "a dimension is negative or the volume has 2^31 voxels or more";
  if (vol_itemsize(dtype) == 0) return "the NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64";
  if ((labels != nullptr) == (mask != nullptr)) return "exactly one of labels and mask is given";
  if (n < 0) return "n is negative";
  return nullptr;
}
}  // namespace

extern "C" {

int32_t unet_vol_intensity_bands(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                                 const int32_t* labels, const uint8_t* mask, int32_t n, const uint8_t* region, const double* edges, int32_t n_edges, int64_t* band_counts,
                                 int64_t* slice_counts, double* minmax, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (const char* why = iv_refusal(dtype, X, Y, Z, labels, mask, n)) UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_bands: %s", why);
  if (!edges || n_edges < 1 || n_edges > MAX_EDGES) UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_bands: 1 to %d edges are taken, not %d", MAX_EDGES, n_edges);
  iv_edges ed;
  ed.n = n_edges;
  for (int e = 0; e < MAX_EDGES; ++e) ed.e[e] = e < n_edges ? edges[e] : 0.0;
  for (int e = 0; e < n_edges; ++e)
    if (!std::isfinite(edges[e]) || (e > 0 && !(edges[e] > edges[e - 1]))) UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_bands: the edges are not finite and strictly ascending at %d", e);
  if ((n > 0 && !band_counts) || (reinterpret_cast<uintptr_t>(band_counts) % 8) != 0 || (reinterpret_cast<uintptr_t>(slice_counts) % 8) != 0 ||
      (reinterpret_cast<uintptr_t>(minmax) % 8) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_bands: null or misaligned output");
  const long long XY = (long long)X * Y, N = XY * Z;
  if (N > 0 && (!vox || (reinterpret_cast<uintptr_t>(vox) % vol_itemsize(dtype)) != 0 || (labels && (reinterpret_cast<uintptr_t>(labels) % 4) != 0)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_bands: null voxel buffer, or a buffer not aligned to its item size");
  hipStream_t s = as_stream(stream);
  const int W = n_edges + 2;
  if (n > 0) UNET_HIP(ctx, hipMemsetAsync(band_counts, 0, (size_t)n * W * sizeof(int64_t), s));
  if (slice_counts && Z > 0) UNET_HIP(ctx, hipMemsetAsync(slice_counts, 0, (size_t)Z * W * sizeof(int64_t), s));
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(minmax);
  if (minmax && n > 0) hipLaunchKernelGGL(ib_minmax_init_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, s, keys, n);
  if (N > 0 && n > 0) {
    const vol_voxels src{vox, dtype, scaled ? 1 : 0, slope, inter};
    const vol_groups grp{labels, mask, region, n};
    const int cps = (int)((XY + IB_CHUNK - 1) / IB_CHUNK);
    const long long chunks = (long long)cps * Z;
    const long long per = (chunks + IB_GRID - 1) / IB_GRID;
    const unsigned grid = (unsigned)((chunks + per - 1) / per);
    unsigned long long* bc = reinterpret_cast<unsigned long long*>(band_counts);
    unsigned long long* sc = reinterpret_cast<unsigned long long*>(slice_counts);
    if ((long long)n * W <= IB_TABLE && n <= IB_GROUPS)
      hipLaunchKernelGGL(ib_bands_kernel<true>, dim3(grid), dim3(TPB), 0, s, src, grp, ed, XY, Z, cps, per, bc, sc, keys);
    else
      hipLaunchKernelGGL(ib_bands_kernel<false>, dim3(grid), dim3(TPB), 0, s, src, grp, ed, XY, Z, cps, per, bc, sc, keys);
  }
  if (minmax && n > 0) hipLaunchKernelGGL(ib_minmax_final_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, s, keys, n);
  UNET_CHECK_LAUNCH(ctx, "vol_intensity_bands"); return UNET_OK;
}

int32_t unet_vol_intensity_gather(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                                  const int32_t* labels, const uint8_t* mask, int32_t n, const uint8_t* region, double* values, int32_t* groups, int64_t capacity,
                                  int64_t* count, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (const char* why = iv_refusal(dtype, X, Y, Z, labels, mask, n)) UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_gather: %s", why);
  if (!count || (reinterpret_cast<uintptr_t>(count) % 8) != 0 || capacity < 0 || (capacity > 0 && !values) || (reinterpret_cast<uintptr_t>(values) % 8) != 0 ||
      (reinterpret_cast<uintptr_t>(groups) % 4) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_gather: null or misaligned output, or a negative capacity");
  const long long N = (long long)X * Y * Z;
  if (N > 0 && (!vox || (reinterpret_cast<uintptr_t>(vox) % vol_itemsize(dtype)) != 0 || (labels && (reinterpret_cast<uintptr_t>(labels) % 4) != 0)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_intensity_gather: null voxel buffer, or a buffer not aligned to its item size");
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(count, 0, sizeof(int64_t), s));
  if (N == 0 || n == 0) return UNET_OK;
  const vol_voxels src{vox, dtype, scaled ? 1 : 0, slope, inter};
  const vol_groups grp{labels, mask, region, n};
  hipLaunchKernelGGL(ig_gather_kernel, dim3(vol_blocks(N, GRID_CAP, TPB)), dim3(TPB), 0, s, src, grp, N, (long long)capacity, values, groups,
                     reinterpret_cast<unsigned long long*>(count));
  UNET_CHECK_LAUNCH(ctx, "vol_intensity_gather"); return UNET_OK;
}

size_t unet_vol_group_moments_ws_bytes(int64_t total, int32_t n) {
  if (total < 0 || n < 0) return 0;
  return ((size_t)n + (size_t)(total / MOM_CHUNK) + (size_t)n + 1) * sizeof(double);          // the means, then the partial-sum slots
}

int32_t unet_vol_group_moments(unet_ctx* ctx, const double* values, const int64_t* offsets, int32_t n, double* out, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (n < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_group_moments: n is negative");
  if (n == 0) return UNET_OK;
  if (!offsets || !out || !ws || (reinterpret_cast<uintptr_t>(ws) % 8) != 0 || (reinterpret_cast<uintptr_t>(out) % 8) != 0 || (reinterpret_cast<uintptr_t>(values) % 8) != 0 ||
      (reinterpret_cast<uintptr_t>(offsets) % 8) != 0 || ws_bytes < unet_vol_group_moments_ws_bytes(0, n))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_group_moments: null or misaligned buffer, or a workspace below unet_vol_group_moments_ws_bytes(total, n)");
  hipStream_t s = as_stream(stream);
  double* mean = static_cast<double*>(ws);
  double* partial = mean + n;
  const long long slot_cap = (long long)(ws_bytes / sizeof(double)) - n;          // nothing is written past the workspace whatever the offsets say
  const long long* off = reinterpret_cast<const long long*>(offsets);
  const unsigned gc = vol_blocks(slot_cap, GRID_CAP, TPB), gf = (unsigned)((n + TPB - 1) / TPB);
  hipLaunchKernelGGL(mom_chunk_kernel<false>, dim3(gc), dim3(TPB), 0, s, values, off, n, mean, partial, slot_cap);
  hipLaunchKernelGGL(mom_fold_kernel<false>, dim3(gf), dim3(TPB), 0, s, off, n, partial, slot_cap, mean, out);
  hipLaunchKernelGGL(mom_chunk_kernel<true>, dim3(gc), dim3(TPB), 0, s, values, off, n, mean, partial, slot_cap);
  hipLaunchKernelGGL(mom_fold_kernel<true>, dim3(gf), dim3(TPB), 0, s, off, n, partial, slot_cap, mean, out);
  UNET_CHECK_LAUNCH(ctx, "vol_group_moments"); return UNET_OK;
}

}  // extern "C"

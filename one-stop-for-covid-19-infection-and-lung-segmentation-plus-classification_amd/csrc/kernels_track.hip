// Every lesion from a baseline to its follow-up: the sparse contingency table of two label volumes on one grid, and the per-voxel maps drawn
// from the host's match of that table.
//   (a, b) -> voxels with labels_a == a and labels_b == b, every pair but (0, 0), in an open-addressing table                 unet_vol_label_pairs
//   track_a = lut_a[a], track_b = lut_b[b], the change class of every voxel and the voxels of every class per slice           unet_vol_track_map
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, as in kernels_volscore.hip.  A label outside 0..n counts as 0 and is never an address.
// Integer arithmetic only; every sum is an integer that leaves as an integer atomic: the same bits on every run (the SLOT a pair lands in depends on who claims first and
// is unspecified -- callers sort by key).  No workgroup waits for another one: a slot's key is written once, by the compare-and-swap that claims it, and never changes, so
// a plain load that sees a non-zero key may be trusted and an apparently empty slot is confirmed by the compare-and-swap's return value; every probe loop is bounded by
// the size of its table, so a full table ends in the overflow counter and never spins.
// Pairs: a lane holds four consecutive voxels (one 16-byte load per volume when both are aligned for it, voxel by voxel otherwise and in the last, short quad).  Inside a
// lesion a whole wave holds one pair: the lanes that share the leading lane's pair are summed with shuffles and sent as one add (kernels_volscore.hip's wave_count), the
// rest go per lane.  A workgroup walks a contiguous range of chunks of UNET_VOL_PAIRS_CHUNK voxels and counts in an LDS table of UNET_VOL_PAIRS_LDS_SLOTS slots first (at
// most PAIRS_LDS_PROBES probes; a pair that finds no slot there goes straight to the global table); the LDS table is flushed when the range ends.
#include "common.h"
#include "vol_common.h"

#include <vector>

namespace {
constexpr int TPB = 256;
constexpr int PAIRS_CHUNK = UNET_VOL_PAIRS_CHUNK;                    // voxels a workgroup takes at a time: TPB lanes x 4 voxels x 4 rounds
constexpr int PAIRS_SLOTS = UNET_VOL_PAIRS_LDS_SLOTS;                // 64-bit key + 32-bit count per slot: 12 KiB of LDS
constexpr int PAIRS_SLOTS_LOG = 10;
constexpr int PAIRS_LDS_PROBES = 16;
constexpr int TRACK_GRID = 256 * 4;                                  // workgroups of either launch
constexpr unsigned long long HASH_MUL = 0x9E3779B97F4A7C15ull;       // 2^64 / the golden ratio: the top bits of key * HASH_MUL spread consecutive keys
static_assert((1 << PAIRS_SLOTS_LOG) == PAIRS_SLOTS && PAIRS_SLOTS < PAIRS_CHUNK && PAIRS_CHUNK % (TPB * 4) == 0, "the LDS stage is a power of two below a chunk");

__device__ __forceinline__ int tk_clamp(int l, int n) { return (unsigned)l <= (unsigned)n ? l : 0; }          // n >= 0: a negative label is above it as unsigned
__device__ __forceinline__ unsigned long long tk_key(int a, int b) { return ((unsigned long long)(unsigned)a << 32) | (unsigned)b; }

// counts[slot of key] += cnt in the global table; info[0] counts the slots claimed, info[1] the voxels that found none
__device__ __forceinline__ void pairs_global_add(unsigned long long key, unsigned long long cnt, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts,
                                                 long long capacity, int cap_log, unsigned long long* __restrict__ info) {
  long long slot = (long long)((key * HASH_MUL) >> (64 - cap_log));
  for (long long p = 0; p < capacity; ++p) {
    unsigned long long k = __atomic_load_n(keys + slot, __ATOMIC_RELAXED);
    if (k == 0) {
      k = atomicCAS(keys + slot, 0ull, key);
      if (k == 0) { k = key; atomicAdd(info, 1ull); }
    }
    if (k == key) { atomicAdd(counts + slot, cnt); return; }
    slot = (slot + 1) & (capacity - 1);
  }
  atomicAdd(info + 1, cnt);
}
// the same in the workgroup's LDS table, with bounded probes; a pair that finds no slot there goes to the global table
__device__ __forceinline__ void pairs_add(unsigned long long key, unsigned cnt, unsigned long long* s_key, unsigned* s_cnt, unsigned long long* __restrict__ keys,
                                          unsigned long long* __restrict__ counts, long long capacity, int cap_log, unsigned long long* __restrict__ info) {
  int slot = (int)((key * HASH_MUL) >> (64 - PAIRS_SLOTS_LOG));
  for (int p = 0; p < PAIRS_LDS_PROBES; ++p) {
    unsigned long long k = __atomic_load_n(s_key + slot, __ATOMIC_RELAXED);
    if (k == 0) {
      k = atomicCAS(s_key + slot, 0ull, key);
      if (k == 0) k = key;
    }
    if (k == key) { atomicAdd(s_cnt + slot, cnt); return; }
    slot = (slot + 1) & (PAIRS_SLOTS - 1);
  }
  pairs_global_add(key, cnt, keys, counts, capacity, cap_log, info);
}

__global__ __launch_bounds__(TPB) void pairs_kernel(const int32_t* __restrict__ la, const int32_t* __restrict__ lb, long long N, int na, int nb, int vec, long long per,
                                                   unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts, long long capacity, int cap_log,
                                                   unsigned long long* __restrict__ info) {
  __shared__ unsigned long long s_key[PAIRS_SLOTS];
  __shared__ unsigned s_cnt[PAIRS_SLOTS];
  __shared__ int s_any[TPB / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < PAIRS_SLOTS; i += TPB) { s_key[i] = 0; s_cnt[i] = 0; }
  __syncthreads();
  const long long chunks = (N + PAIRS_CHUNK - 1) / PAIRS_CHUNK;
  const long long c0 = (long long)blockIdx.x * per, c1 = min(chunks, c0 + per);
  int any = 0;                                                        // voxels of this lane with either label non-zero
  for (long long c = c0; c < c1; ++c) {                               // trip counts are uniform over the workgroup
    for (int r = 0; r < PAIRS_CHUNK / (TPB * 4); ++r) {
      const long long f0 = c * PAIRS_CHUNK + ((long long)r * TPB + tid) * 4;
      unsigned long long k4[4] = {0, 0, 0, 0};
      if (f0 < N) {
        if (vec && f0 + 3 < N) {
          const int4 u = *reinterpret_cast<const int4*>(la + f0), v = *reinterpret_cast<const int4*>(lb + f0);
          k4[0] = tk_key(tk_clamp(u.x, na), tk_clamp(v.x, nb)); k4[1] = tk_key(tk_clamp(u.y, na), tk_clamp(v.y, nb));
          k4[2] = tk_key(tk_clamp(u.z, na), tk_clamp(v.z, nb)); k4[3] = tk_key(tk_clamp(u.w, na), tk_clamp(v.w, nb));
        } else {
          for (int i = 0; i < 4 && f0 + i < N; ++i) k4[i] = tk_key(tk_clamp(la[f0 + i], na), tk_clamp(lb[f0 + i], nb));
        }
      }
      unsigned long long key = 0;                                     // the lane's first pair and how many of its four voxels hold it
      unsigned cnt = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (k4[i] == 0) continue;
        ++any;
        if (key == 0) key = k4[i];
        if (k4[i] == key) ++cnt;
        else pairs_add(k4[i], 1u, s_key, s_cnt, keys, counts, capacity, cap_log, info);
      }
      for (int round = 0; round < 2; ++round) {                       // the lanes that hold the first pending lane's pair: one add
        const unsigned long long pending = __ballot(key != 0);
        if (!pending) break;                                          // (wave-uniform)
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned long long K = __shfl(key, leader, 64);
        const bool part = key == K;
        unsigned s = part ? cnt : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == leader) pairs_add(K, s, s_key, s_cnt, keys, counts, capacity, cap_log, info);
        if (part) key = 0;
      }
      if (key != 0) pairs_add(key, cnt, s_key, s_cnt, keys, counts, capacity, cap_log, info);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) any += __shfl_xor(any, o, 64);
  if (lane == 0) s_any[tid >> 6] = any;
  __syncthreads();                                                    // (also: every add to the LDS table has landed)
  if (tid == 0) {
    long long t = 0;
    for (int w = 0; w < TPB / 64; ++w) t += s_any[w];
    if (t) atomicAdd(info + 2, (unsigned long long)t);
  }
  for (int i = tid; i < PAIRS_SLOTS; i += TPB) {
    const unsigned long long k = s_key[i];
    if (k != 0) pairs_global_add(k, (unsigned long long)s_cnt[i], keys, counts, capacity, cap_log, info);
  }
}

// ---- the maps -------------------------------------------------------------------------------------------------------------------------------------------
// A lane holds the four voxels [4 g, 4 g + 4) of the flat volume; chunk c = TM_CHUNK voxels, a workgroup walks a contiguous range of chunks.  s_slice holds the class
// counts of slice `zcur`, the slice of the chunk's first voxel; they leave when the next chunk starts in another slice.  A wave whose 256 voxels lie in one slice sums its
// lanes' counts (six 10-bit fields of one 64-bit word) with shuffles and adds once per class; any other wave (a slice border, the tail) adds voxel by voxel.  What falls
// into another slice than zcur goes straight to per_slice.
constexpr int TM_CHUNK = TPB * 16;
constexpr int TM_VEC_IN = 1, TM_VEC_CLS = 2, TM_VEC_TA = 4, TM_VEC_TB = 8;

__global__ __launch_bounds__(TPB) void track_map_kernel(const int32_t* __restrict__ la, const int32_t* __restrict__ lb, long long N, unsigned XY, int na, int nb,
                                                       const int32_t* __restrict__ lut_a, const int32_t* __restrict__ lut_b, const uint8_t* __restrict__ cls_a,
                                                       const uint8_t* __restrict__ cls_b, int vec, long long per, uint8_t* __restrict__ cls, int32_t* __restrict__ track_a,
                                                       int32_t* __restrict__ track_b, unsigned long long* __restrict__ per_slice) {
  __shared__ int s_slice[6];
  const int tid = threadIdx.x, lane = tid & 63;
  const bool want_cls = cls != nullptr || per_slice != nullptr;
  if (tid < 6) s_slice[tid] = 0;
  __syncthreads();
  const long long chunks = (N + TM_CHUNK - 1) / TM_CHUNK;
  const long long c0 = (long long)blockIdx.x * per, c1 = min(chunks, c0 + per);
  for (long long c = c0; c < c1; ++c) {                               // trip counts and barriers are uniform over the workgroup
    const unsigned zcur = (unsigned)(c * TM_CHUNK) / XY;
    for (int r = 0; r < TM_CHUNK / (TPB * 4); ++r) {
      const long long f0 = c * TM_CHUNK + ((long long)r * TPB + tid) * 4;
      const int nv = f0 < N ? (int)min(4LL, N - f0) : 0;              // voxels of this lane
      int a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
      if (nv == 4 && (vec & TM_VEC_IN)) {
        const int4 u = *reinterpret_cast<const int4*>(la + f0), v = *reinterpret_cast<const int4*>(lb + f0);
        a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w; b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
      } else for (int i = 0; i < nv; ++i) { a[i] = la[f0 + i]; b[i] = lb[f0 + i]; }
      int ta[4], tb[4], k[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = tk_clamp(a[i], na); b[i] = tk_clamp(b[i], nb);
        ta[i] = (track_a && a[i]) ? lut_a[a[i]] : 0;                  // entry 0 reads as 0, whatever it holds
        tb[i] = (track_b && b[i]) ? lut_b[b[i]] : 0;
        k[i] = 0;
        if (want_cls) k[i] = (a[i] && b[i]) ? 3 : (a[i] ? (int)cls_a[a[i]] : (b[i] ? (int)cls_b[b[i]] : 0));
      }
      if (nv == 4) {
        if (cls) {
          if (vec & TM_VEC_CLS) *reinterpret_cast<unsigned*>(cls + f0) = (unsigned)k[0] | ((unsigned)k[1] << 8) | ((unsigned)k[2] << 16) | ((unsigned)k[3] << 24);
          else for (int i = 0; i < 4; ++i) cls[f0 + i] = (uint8_t)k[i];
        }
        if (track_a) {
          if (vec & TM_VEC_TA) *reinterpret_cast<int4*>(track_a + f0) = make_int4(ta[0], ta[1], ta[2], ta[3]);
          else for (int i = 0; i < 4; ++i) track_a[f0 + i] = ta[i];
        }
        if (track_b) {
          if (vec & TM_VEC_TB) *reinterpret_cast<int4*>(track_b + f0) = make_int4(tb[0], tb[1], tb[2], tb[3]);
          else for (int i = 0; i < 4; ++i) track_b[f0 + i] = tb[i];
        }
      } else {
        for (int i = 0; i < nv; ++i) {
          if (cls) cls[f0 + i] = (uint8_t)k[i];
          if (track_a) track_a[f0 + i] = ta[i];
          if (track_b) track_b[f0 + i] = tb[i];
        }
      }
      if (per_slice) {
        unsigned z0 = 0, rem = 0;
        if (nv) { z0 = (unsigned)f0 / XY; rem = (unsigned)f0 - z0 * XY; }
        const bool one = nv == 4 && rem + 3 < XY && z0 == (unsigned)__shfl((int)z0, 0, 64);
        if (__ballot(one) == ~0ull) {                                 // the wave's 256 voxels lie in slice z0
          unsigned long long packed = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) packed += 1ull << (10 * k[i]);
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) packed += __shfl_xor(packed, o, 64);
          if (lane < 6) {
            const int v = (int)((packed >> (10 * lane)) & 1023ull);
            if (v) { if (z0 == zcur) atomicAdd(s_slice + lane, v); else atomicAdd(per_slice + (long long)z0 * 6 + lane, (unsigned long long)v); }
          }
        } else {
          for (int i = 0; i < nv; ++i) {
            unsigned z = z0, q = rem + i;
            while (q >= XY) { q -= XY; ++z; }
            if (z == zcur) atomicAdd(s_slice + k[i], 1); else atomicAdd(per_slice + (long long)z * 6 + k[i], 1ull);
          }
        }
      }
    }
    if (per_slice && (c + 1 == c1 || (unsigned)((c + 1) * TM_CHUNK) / XY != zcur)) {          // the next chunk starts in another slice
      __syncthreads();
      if (tid < 6) {
        const int v = s_slice[tid];
        if (v) atomicAdd(per_slice + (long long)zcur * 6 + tid, (unsigned long long)v);
        s_slice[tid] = 0;
      }
      __syncthreads();
    }
  }
}
}  // namespace

extern "C" {

int32_t unet_vol_label_pairs(unet_ctx* ctx, const int32_t* labels_a, int32_t n_a, const int32_t* labels_b, int32_t n_b, int32_t X, int32_t Y, int32_t Z, uint64_t* keys,
                             int64_t* counts, int64_t capacity, int64_t* info, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (n_a < 0 || n_b < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_pairs: n_a, n_b are not negative");
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_pairs: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  if (capacity < 16 || capacity > (1LL << 30) || (capacity & (capacity - 1)) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_label_pairs: capacity %lld is not a power of two in 16 .. 2^30", (long long)capacity);
  if (!keys || !counts || !info || !vol_aligned(keys, 8) || !vol_aligned(counts, 8) || !vol_aligned(info, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_pairs: null or misaligned table");
  const long long N = (long long)X * Y * Z;
  if (N > 0 && (!labels_a || !labels_b || !vol_aligned(labels_a, 4) || !vol_aligned(labels_b, 4))) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_pairs: null or misaligned label volume");
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(keys, 0, (size_t)capacity * sizeof(uint64_t), s));
  UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)capacity * sizeof(int64_t), s));
  UNET_HIP(ctx, hipMemsetAsync(info, 0, 3 * sizeof(int64_t), s));
  if (N == 0) return UNET_OK;
  int cap_log = 0;
  while ((1LL << cap_log) < capacity) ++cap_log;
  const long long chunks = (N + PAIRS_CHUNK - 1) / PAIRS_CHUNK;
  const long long per = (chunks + TRACK_GRID - 1) / TRACK_GRID;
  const unsigned grid = (unsigned)((chunks + per - 1) / per);
  const int vec = vol_aligned(labels_a, 16) && vol_aligned(labels_b, 16);
  hipLaunchKernelGGL(pairs_kernel, dim3(grid), dim3(TPB), 0, s, labels_a, labels_b, N, n_a, n_b, vec, per, reinterpret_cast<unsigned long long*>(keys),
                     reinterpret_cast<unsigned long long*>(counts), (long long)capacity, cap_log, reinterpret_cast<unsigned long long*>(info));
  UNET_CHECK_LAUNCH(ctx, "vol_label_pairs"); return UNET_OK;
}

int32_t unet_vol_track_map(unet_ctx* ctx, const int32_t* labels_a, int32_t n_a, const int32_t* labels_b, int32_t n_b, int32_t X, int32_t Y, int32_t Z, const int32_t* lut_a,
                           const int32_t* lut_b, const uint8_t* cls_a, const uint8_t* cls_b, uint8_t* cls, int32_t* track_a, int32_t* track_b, int64_t* per_slice, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (n_a < 0 || n_b < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: n_a, n_b are not negative");
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  if (!cls && !track_a && !track_b && !per_slice) UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: no output");
  if (!vol_aligned(track_a, 4) || !vol_aligned(track_b, 4) || !vol_aligned(per_slice, 8) || !vol_aligned(lut_a, 4) || !vol_aligned(lut_b, 4))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: misaligned buffer");
  const bool want_cls = cls || per_slice;
  if ((track_a && n_a > 0 && !lut_a) || (track_b && n_b > 0 && !lut_b) || (want_cls && ((n_a > 0 && !cls_a) || (n_b > 0 && !cls_b))))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: an output is asked for without the table it is read from");
  const long long XY = (long long)X * Y, N = XY * Z;
  if (N > 0 && (!labels_a || !labels_b || !vol_aligned(labels_a, 4) || !vol_aligned(labels_b, 4))) UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: null or misaligned label volume");
  if (cls && ((const void*)cls == (const void*)labels_a || (const void*)cls == (const void*)labels_b)) UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: cls must not be a label volume's own buffer");
  hipStream_t s = as_stream(stream);
  if (want_cls) {                                                     // the class tables are small (n + 1 bytes): the host reads them before anything is written
    const uint8_t* tabs[2] = {cls_a, cls_b};
    const int ns[2] = {n_a, n_b};
    for (int t = 0; t < 2; ++t) {
      if (ns[t] == 0) continue;
      std::vector<uint8_t> h((size_t)ns[t]);
      UNET_HIP(ctx, hipMemcpyAsync(h.data(), tabs[t] + 1, h.size(), hipMemcpyDeviceToHost, s));
      UNET_HIP(ctx, hipStreamSynchronize(s));
      for (size_t i = 0; i < h.size(); ++i)
        if (h[i] > 5) UNET_FAIL(ctx, UNET_E_ARG, "vol_track_map: cls_%c[%zu] = %d is above 5", t ? 'b' : 'a', i + 1, (int)h[i]);
    }
  }
  if (Z == 0) return UNET_OK;
  if (per_slice) UNET_HIP(ctx, hipMemsetAsync(per_slice, 0, (size_t)Z * 6 * sizeof(int64_t), s));
  if (N == 0) return UNET_OK;
  const long long chunks = (N + TM_CHUNK - 1) / TM_CHUNK;
  const long long per = (chunks + TRACK_GRID - 1) / TRACK_GRID;
  const unsigned grid = (unsigned)((chunks + per - 1) / per);
  const int vec = ((vol_aligned(labels_a, 16) && vol_aligned(labels_b, 16)) ? TM_VEC_IN : 0) | (vol_aligned(cls, 4) ? TM_VEC_CLS : 0) | (vol_aligned(track_a, 16) ? TM_VEC_TA : 0) |
                  (vol_aligned(track_b, 16) ? TM_VEC_TB : 0);
  hipLaunchKernelGGL(track_map_kernel, dim3(grid), dim3(TPB), 0, s, labels_a, labels_b, N, (unsigned)XY, n_a, n_b, lut_a, lut_b, cls_a, cls_b, vec, per, cls, track_a, track_b,
                     reinterpret_cast<unsigned long long*>(per_slice));
  UNET_CHECK_LAUNCH(ctx, "vol_track_map"); return UNET_OK;
}

}  // extern "C"

// Where the infection sits in the lungs: every lung voxel binned by side x anatomical zone x depth shell under the lung surface.
//   the inclusive bounding box of side 1 and of side 2, and the largest squared distance under each                                                     unet_vol_side_extents
//   lung / infected voxels per (side, zone, shell) bin, infected voxels off the lungs, voxels of every lesion per (side, zone) and per shell, the smallest
//   distance of every lesion, the zone of every voxel                                                                                                 unet_vol_zone_table
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, as in kernels_lungside.hip.
// Integer arithmetic only.  The distances are compared as order-preserving 64-bit keys of their bit patterns (kernels_lungside.hip's ls_key): for the non-negative values
// and +inf that unet_vol_edt_sq writes, key order is value order, and no floating-point instruction runs.  Sums are integers per wave (ballots), per workgroup in LDS, and
// leave as 64-bit atomics; minima and maxima are taken per lane, per wave (butterflies), per workgroup in LDS and leave as one atomic: the same bits on every run.
// Both kernels walk the flat volume as kernels_lungside.hip's side_assign_kernel does: a lane holds four consecutive voxels -- one 4-byte load of sides (and of the
// infection mask), two 16-byte loads of the distances, one 16-byte load of the labels, one 4-byte store of the zone map -- when the buffers are aligned for it, one voxel
// otherwise; a grid of at most ZT_GRID workgroups strides over the items, and every trip count is uniform over a wave.
// The zone of a coordinate needs no division: with d = c - lo (flip: lo + extent - 1 - c, the coordinate counted from the other end of the range),
// q = floor(d parts / extent) clamped to 0 .. parts - 1 is the number of k in 1 .. parts - 1 with d >= ceil(k extent / parts); the host states these thresholds once per
// (side, axis, k) and the kernel keeps them in LDS.  The flip mirrors the coordinate, not the quotient: parts - 1 - floor((c - lo) parts / extent) cuts a range that is no
// multiple of `parts` at other voxels than the same range stored the other way round, and the numbering is anatomical whatever the storage.
#include "common.h"
#include "vol_common.h"

#include <cmath>
#include <cstring>

namespace {
constexpr int TPB = 256;
constexpr int ZT_GRID = 256 * 4;                                     // workgroups of either launch at the most
constexpr int ZT_BINS = 1024;                                        // (side, zone, shell) bins of a workgroup's LDS table, two counters each (8 KiB): 2 P S <= ZT_BINS
constexpr int ZT_TABLE = 4096;                                       // per-lesion counters of a workgroup's LDS table (16 KiB): n (2 P + S) <= ZT_TABLE
constexpr int ZT_LESIONS = ZT_TABLE / 3;                             // lesions of that table at the most (2 P + S >= 3): their smallest distances sit beside it
constexpr unsigned long long ZT_NONE = ~0ull;

inline unsigned long long zt_host_key(double v) { unsigned long long u; memcpy(&u, &v, 8); return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }

// what the table kernel needs of a unet_zone_spec, passed by value
struct ZtParams {
  int parts[3], flip[3], thr[2][3][7];                                // thr[s][a][k - 1] = ceil(k extent[s][a] / parts[a]), k = 1 .. parts[a] - 1
  long long org[2][3];                                                // lo[s][a], or lo[s][a] + extent[s][a] - 1 for a flipped axis: d = |c - org| on the range
  int P, S;
  unsigned long long r2key[2][3];
};

__device__ __forceinline__ unsigned long long zt_key(unsigned long long u) { return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
__device__ __forceinline__ unsigned zt_sides4(unsigned m) {            // a side byte above 2 counts as 0
  unsigned r = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { const unsigned b = (m >> (8 * k)) & 0xFFu; r |= (b <= 2u ? b : 0u) << (8 * k); }
  return r;
}
__device__ __forceinline__ int zt_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int zt_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned long long zt_wave_min64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ unsigned long long zt_wave_max64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}

__global__ void extents_init_kernel(int* __restrict__ box, unsigned long long* __restrict__ dmax) {
  const int t = threadIdx.x;
  if (t < 12) box[t] = (t & 1) ? -1 : 0x7FFFFFFF;
  if (t < 2) dmax[t] = 0ull;
}

// VEC = 4: item g = voxels [4 g, 4 g + 4) (the last item may be short: it goes voxel by voxel); VEC = 1: item g = voxel g.  Trip counts are wave-uniform.
// s_box[w][side][0 .. 5] = {min x, max x, min y, max y, min z, max z} of wave w
template <int VEC>
__global__ __launch_bounds__(TPB) void side_extents_kernel(const uint8_t* __restrict__ sides, const unsigned long long* __restrict__ d2, long long N, int X, int Y,
                                                          int* __restrict__ box, unsigned long long* __restrict__ dmax) {
  __shared__ int s_box[TPB / 64][2][6];
  __shared__ unsigned long long s_dmax[TPB / 64][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long items = (N + VEC - 1) / VEC;
  int lo[2][3], hi[2][3];
  unsigned long long dm[2] = {0ull, 0ull};
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[s][a] = 0x7FFFFFFF; hi[s][a] = -1; }
  for (long long g0 = (long long)blockIdx.x * TPB + (tid - lane); g0 < items; g0 += (long long)gridDim.x * TPB) {
    const long long g = g0 + lane, v0 = g * VEC;
    unsigned m = 0;
    bool full = false;
    if constexpr (VEC == 4) {
      full = v0 + 4 <= N;
      if (full) m = *reinterpret_cast<const unsigned*>(sides + v0);
      else for (int k = 0; k < 4; ++k) if (v0 + k < N) m |= (unsigned)sides[v0 + k] << (8 * k);
    } else {
      if (g < N) m = sides[g];
    }
    m = zt_sides4(m);
    if (m == 0) continue;                                             // no barrier and no cross-lane operation inside the loop
    unsigned long long dk[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) dk[k] = 0ull;
    if (d2) {
      if constexpr (VEC == 4) {
        if (full) {
          const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(d2 + v0), a23 = *reinterpret_cast<const ulonglong2*>(d2 + v0 + 2);
          dk[0] = a01.x; dk[1] = a01.y; dk[2] = a23.x; dk[3] = a23.y;
        } else {
          for (int k = 0; k < 4; ++k) if (v0 + k < N) dk[k] = d2[v0 + k];
        }
      } else {
        dk[0] = d2[g];
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) dk[k] = zt_key(dk[k]);
    }
    const unsigned f = (unsigned)v0, row = f / (unsigned)X;
    int x = (int)(f - row * (unsigned)X), z = (int)(row / (unsigned)Y), y = (int)(row - (unsigned)z * (unsigned)Y);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int sd = (int)((m >> (8 * k)) & 0xFFu);
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (sd == s + 1) {
          lo[s][0] = min(lo[s][0], x); hi[s][0] = max(hi[s][0], x);
          lo[s][1] = min(lo[s][1], y); hi[s][1] = max(hi[s][1], y);
          lo[s][2] = min(lo[s][2], z); hi[s][2] = max(hi[s][2], z);
          dm[s] = dk[k] > dm[s] ? dk[k] : dm[s];
        }
      if (++x == X) { x = 0; if (++y == Y) { y = 0; ++z; } }
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int l = zt_wave_min(lo[s][a]), h = zt_wave_max(hi[s][a]);
      if (lane == 0) { s_box[wave][s][2 * a] = l; s_box[wave][s][2 * a + 1] = h; }
    }
    const unsigned long long d = zt_wave_max64(dm[s]);
    if (lane == 0) s_dmax[wave][s] = d;
  }
  __syncthreads();
  if (tid < 12) {                                                     // one atomic per workgroup and field
    const int s = tid / 6, q = tid % 6;
    int v = s_box[0][s][q];
    for (int w = 1; w < TPB / 64; ++w) v = (q & 1) ? max(v, s_box[w][s][q]) : min(v, s_box[w][s][q]);
    if (q & 1) { if (v >= 0) atomicMax(box + tid, v); }
    else if (v != 0x7FFFFFFF) atomicMin(box + tid, v);
  } else if (tid < 14) {
    const int s = tid - 12;
    unsigned long long v = s_dmax[0][s];
    for (int w = 1; w < TPB / 64; ++w) v = s_dmax[w][s] > v ? s_dmax[w][s] : v;
    if (v) atomicMax(dmax + s, v);
  }
}

// s_bin[bin][0 / 1]: lung / infected voxels of the bin; s_tab: [n][2 P] voxels of a lesion per (side, zone), then [n][S] per shell; s_dmin[n].
// Every loop bound and every barrier below is uniform over the workgroup; every ballot, shuffle and butterfly runs with all 64 lanes of a wave.
template <int VEC, bool LDS_TABLE>
__global__ __launch_bounds__(TPB) void zone_table_kernel(const uint8_t* __restrict__ sides, const uint8_t* __restrict__ infection, const int32_t* __restrict__ labels, int n,
                                                        const unsigned long long* __restrict__ d2, long long N, int X, int Y, const ZtParams prm,
                                                        unsigned long long* __restrict__ table, unsigned long long* __restrict__ outside,
                                                        unsigned long long* __restrict__ lesion_zone, unsigned long long* __restrict__ lesion_shell,
                                                        unsigned long long* __restrict__ lesion_dmin, uint8_t* __restrict__ zone_map) {
  __shared__ int s_bin[2 * ZT_BINS];
  __shared__ int s_tab[LDS_TABLE ? ZT_TABLE : 1];
  __shared__ unsigned long long s_dmin[LDS_TABLE ? ZT_LESIONS : 1];
  __shared__ int s_thr[2][3][7];
  __shared__ long long s_org[2][3];
  __shared__ unsigned long long s_r2[2][3];
  __shared__ int s_out;
  const int tid = threadIdx.x, lane = tid & 63;
  const int P = prm.P, S = prm.S, P2 = 2 * P, B = P2 * S;
  const bool want_les = labels != nullptr && n > 0;
  for (int i = tid; i < 2 * B; i += TPB) s_bin[i] = 0;
  if constexpr (LDS_TABLE) {
    for (int i = tid; i < n * (P2 + S); i += TPB) s_tab[i] = 0;
    for (int i = tid; i < n; i += TPB) s_dmin[i] = ZT_NONE;
  }
  if (tid < 6) { s_org[tid / 3][tid % 3] = prm.org[tid / 3][tid % 3]; s_r2[tid / 3][tid % 3] = prm.r2key[tid / 3][tid % 3]; }
  if (tid < 42) s_thr[tid / 21][(tid % 21) / 7][tid % 7] = prm.thr[tid / 21][(tid % 21) / 7][tid % 7];
  if (tid == 0) s_out = 0;
  __syncthreads();
  const long long items = (N + VEC - 1) / VEC;
  int n_out = 0;
  for (long long g0 = (long long)blockIdx.x * TPB + (tid - lane); g0 < items; g0 += (long long)gridDim.x * TPB) {
    const long long g = g0 + lane, v0 = g * VEC;
    unsigned m = 0, inf = 0;
    bool full = false;
    if constexpr (VEC == 4) {
      full = v0 + 4 <= N;
      if (full) {
        m = *reinterpret_cast<const unsigned*>(sides + v0);
        if (infection) inf = *reinterpret_cast<const unsigned*>(infection + v0);
      } else {
        for (int k = 0; k < 4; ++k)
          if (v0 + k < N) { m |= (unsigned)sides[v0 + k] << (8 * k); if (infection) inf |= (unsigned)infection[v0 + k] << (8 * k); }
      }
    } else if (g < N) {
      m = sides[g];
      if (infection) inf = infection[g];
    }
    m = zt_sides4(m);
    unsigned zm = 0;                                                  // the zone map's bytes of this item
    if (__ballot((m | inf) != 0)) {                                   // wave-uniform: a wave with no lung voxel and no infected voxel reads neither d2 nor the labels
      int sz[VEC], sh[VEC], lab[VEC];                                 // (side, zone) 0 .. 2 P - 1 or -1 off the lungs, the shell, the lesion 1 .. n or 0
      unsigned long long dk[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) { sz[k] = -1; sh[k] = 0; lab[k] = 0; dk[k] = 0x8000000000000000ull; }          // without d2 every distance is +0.0
      if (m != 0) {
        if (d2) {
          if constexpr (VEC == 4) {
            if (full) {
              const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(d2 + v0), a23 = *reinterpret_cast<const ulonglong2*>(d2 + v0 + 2);
              dk[0] = a01.x; dk[1] = a01.y; dk[2] = a23.x; dk[3] = a23.y;
            } else {
              for (int k = 0; k < 4; ++k) if (v0 + k < N) dk[k] = d2[v0 + k];
            }
          } else {
            dk[0] = d2[g];
          }
#pragma unroll
          for (int k = 0; k < VEC; ++k) dk[k] = zt_key(dk[k]);
        }
        if (want_les) {
          if constexpr (VEC == 4) {
            if (full) {
              const int4 l4 = *reinterpret_cast<const int4*>(labels + v0);
              lab[0] = l4.x; lab[1] = l4.y; lab[2] = l4.z; lab[3] = l4.w;
            } else {
              for (int k = 0; k < 4; ++k) if (v0 + k < N) lab[k] = labels[v0 + k];
            }
          } else {
            lab[0] = labels[g];
          }
        }
        const unsigned f = (unsigned)v0, row = f / (unsigned)X;
        int c[3];
        c[0] = (int)(f - row * (unsigned)X); c[2] = (int)(row / (unsigned)Y); c[1] = (int)(row - (unsigned)c[2] * (unsigned)Y);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const int sd = (int)((m >> (8 * k)) & 0xFFu);
          if (sd) {
            const int s = sd - 1;
            int q[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              const long long d = prm.flip[a] ? s_org[s][a] - (long long)c[a] : (long long)c[a] - s_org[s][a];
              int cnt = 0;
              for (int t = 0; t + 1 < prm.parts[a]; ++t) cnt += d >= (long long)s_thr[s][a][t];
              q[a] = cnt;
            }
            sz[k] = s * P + q[0] + prm.parts[0] * (q[1] + prm.parts[1] * q[2]);
            int shell = 0;
            for (int t = 0; t + 1 < S; ++t) shell += dk[k] > s_r2[s][t];
            sh[k] = shell;
            lab[k] = (unsigned)(lab[k] - 1) < (unsigned)n ? lab[k] : 0;          // a label outside 1 .. n is ignored, never an address
            zm |= (unsigned)(1 + sz[k]) << (8 * k);
          } else {
            lab[k] = 0;                                               // in-lung voxels only
          }
          if (++c[0] == X) { c[0] = 0; if (++c[1] == Y) { c[1] = 0; ++c[2]; } }
        }
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool infected = ((inf >> (8 * k)) & 0xFFu) != 0;
        const int key = sz[k] >= 0 ? sz[k] * S + sh[k] : -1;
        n_out += infected && key < 0;
        const unsigned long long bi = __ballot(infected);
        unsigned long long pending = __ballot(key >= 0);
        while (pending) {                                             // one round per distinct bin of the wave
          const int leader = __ffsll((long long)pending) - 1;
          const int K = __shfl(key, leader, 64);
          const unsigned long long same = __ballot(key == K);
          if (lane == leader) {
            atomicAdd(s_bin + 2 * K, (int)__popcll(same));
            const int ci = (int)__popcll(same & bi);
            if (ci) atomicAdd(s_bin + 2 * K + 1, ci);
          }
          pending &= ~same;
        }
        const long long lkey = lab[k] ? (long long)(lab[k] - 1) * B + key : -1;          // n B may pass 2^31 beyond the LDS table
        pending = __ballot(lkey >= 0);
        while (pending) {                                             // one round per distinct (lesion, bin) of the wave
          const int leader = __ffsll((long long)pending) - 1;
          const long long K = __shfl(lkey, leader, 64);
          const bool mine = lkey == K;
          const unsigned long long same = __ballot(mine);
          const unsigned long long dmin = zt_wave_min64(mine ? dk[k] : ZT_NONE);
          if (lane == leader) {
            const int cnt = (int)__popcll(same), l0 = lab[k] - 1;
            if constexpr (LDS_TABLE) {
              atomicAdd(s_tab + l0 * P2 + sz[k], cnt);
              atomicAdd(s_tab + n * P2 + l0 * S + sh[k], cnt);
              atomicMin(s_dmin + l0, dmin);
            } else {
              atomicAdd(lesion_zone + (long long)l0 * P2 + sz[k], (unsigned long long)cnt);
              atomicAdd(lesion_shell + (long long)l0 * S + sh[k], (unsigned long long)cnt);
              atomicMin(lesion_dmin + l0, dmin);
            }
          }
          pending &= ~same;
        }
      }
    }
    if (zone_map) {
      if constexpr (VEC == 4) {
        if (full) *reinterpret_cast<unsigned*>(zone_map + v0) = zm;
        else for (int k = 0; k < 4; ++k) if (v0 + k < N) zone_map[v0 + k] = (uint8_t)((zm >> (8 * k)) & 0xFFu);
      } else if (g < N) {
        zone_map[g] = (uint8_t)zm;
      }
    }
  }
  n_out = vol_wave_sum(n_out);
  if (lane == 0 && n_out) atomicAdd(&s_out, n_out);
  __syncthreads();
  for (int i = tid; i < 2 * B; i += TPB) { const int v = s_bin[i]; if (v) atomicAdd(table + i, (unsigned long long)v); }
  if (tid == 0 && s_out) atomicAdd(outside, (unsigned long long)s_out);
  if constexpr (LDS_TABLE) {
    for (int i = tid; i < n * P2; i += TPB) { const int v = s_tab[i]; if (v) atomicAdd(lesion_zone + i, (unsigned long long)v); }
    for (int i = tid; i < n * S; i += TPB) { const int v = s_tab[n * P2 + i]; if (v) atomicAdd(lesion_shell + i, (unsigned long long)v); }
    for (int i = tid; i < n; i += TPB) { const unsigned long long v = s_dmin[i]; if (v != ZT_NONE) atomicMin(lesion_dmin + i, v); }
  }
}

unsigned zt_grid(long long items) {
  long long blocks = (items + TPB - 1) / TPB;
  return (unsigned)(blocks > ZT_GRID ? ZT_GRID : blocks);
}
}  // namespace

extern "C" {

int32_t unet_vol_side_extents(unet_ctx* ctx, const uint8_t* sides, const double* d2, int32_t X, int32_t Y, int32_t Z, int32_t* box, uint64_t* dmax_key, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_side_extents: a dimension is negative or the volume has 2^31 voxels or more");
  const long long N = (long long)X * Y * Z;
  if (N == 0) return UNET_OK;
  if (!sides || !box || !dmax_key || !vol_aligned(d2, 8) || !vol_aligned(box, 4) || !vol_aligned(dmax_key, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_side_extents: null or misaligned buffer");
  hipStream_t s = as_stream(stream);
  unsigned long long* dm = reinterpret_cast<unsigned long long*>(dmax_key);
  const unsigned long long* d = reinterpret_cast<const unsigned long long*>(d2);
  hipLaunchKernelGGL(extents_init_kernel, dim3(1), dim3(64), 0, s, box, dm);
  const bool vec = vol_aligned(sides, 4) && vol_aligned(d2, 16);
  if (vec) hipLaunchKernelGGL(side_extents_kernel<4>, dim3(zt_grid((N + 3) / 4)), dim3(TPB), 0, s, sides, d, N, X, Y, box, dm);
  else hipLaunchKernelGGL(side_extents_kernel<1>, dim3(zt_grid(N)), dim3(TPB), 0, s, sides, d, N, X, Y, box, dm);
  UNET_CHECK_LAUNCH(ctx, "vol_side_extents"); return UNET_OK;
}

int32_t unet_vol_zone_table(unet_ctx* ctx, const uint8_t* sides, const uint8_t* infection, const int32_t* labels, int32_t n, const double* d2, int32_t X, int32_t Y, int32_t Z,
                            const unet_zone_spec* spec, int64_t* table, int64_t* outside, int64_t* lesion_zone, int64_t* lesion_shell, uint64_t* lesion_dmin_key,
                            uint8_t* zone_map, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: a dimension is negative or the volume has 2^31 voxels or more");
  if (n < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: n is negative");
  if (!spec) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: spec is null");
  ZtParams prm;
  memset(&prm, 0, sizeof(prm));
  long long P = 1;
  for (int a = 0; a < 3; ++a) {
    if (spec->parts[a] < 1 || spec->parts[a] > UNET_VOL_ZONE_MAX_PARTS) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: parts[%d] = %d is not in 1..%d", a, spec->parts[a], UNET_VOL_ZONE_MAX_PARTS);
    if (spec->flip[a] != 0 && spec->flip[a] != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: flip[%d] = %d is not 0 or 1", a, spec->flip[a]);
    prm.parts[a] = spec->parts[a]; prm.flip[a] = spec->flip[a];
    P *= spec->parts[a];
  }
  const int S = spec->shells;
  if (S < 1 || S > UNET_VOL_ZONE_MAX_SHELLS) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: shells = %d is not in 1..%d", S, UNET_VOL_ZONE_MAX_SHELLS);
  if (2 * P * S > UNET_VOL_ZONE_MAX_BINS) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: 2 x %lld zones x %d shells are more than %d bins", P, S, UNET_VOL_ZONE_MAX_BINS);
  if (!d2 && S != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: shells = %d needs d2", S);
  if (zone_map && 2 * P > 255) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: 2 x %lld zones do not fit the zone map's byte", P);
  for (int s = 0; s < 2; ++s) {
    for (int a = 0; a < 3; ++a) {
      const long long e = spec->extent[s][a], p = spec->parts[a];
      if (e < 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: extent[%d][%d] = %lld is not positive", s, a, e);
      prm.org[s][a] = spec->flip[a] ? (long long)spec->lo[s][a] + e - 1 : (long long)spec->lo[s][a];
      for (int k = 1; k < p; ++k) prm.thr[s][a][k - 1] = (int)((k * e + p - 1) / p);
    }
    double prev = 0.0;
    for (int k = 0; k + 1 < S; ++k) {
      const double r = spec->r2[s][k];
      if (!std::isfinite(r) || r < 0.0 || r < prev) UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: r2[%d] must be finite, non-negative and ascending", s);
      prev = r;
      prm.r2key[s][k] = zt_host_key(r == 0.0 ? 0.0 : r);             // -0.0 compares as +0.0
    }
  }
  prm.P = (int)P; prm.S = S;
  const long long N = (long long)X * Y * Z;
  if (N == 0) return UNET_OK;
  if (!sides || !table || !outside || (n > 0 && (!lesion_zone || !lesion_shell || !lesion_dmin_key)) || !vol_aligned(table, 8) || !vol_aligned(outside, 8) ||
      !vol_aligned(lesion_zone, 8) || !vol_aligned(lesion_shell, 8) || !vol_aligned(lesion_dmin_key, 8) || !vol_aligned(labels, 4) || !vol_aligned(d2, 8))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_zone_table: null or misaligned buffer");
  hipStream_t st = as_stream(stream);
  const int B = (int)(2 * P * S);
  UNET_HIP(ctx, hipMemsetAsync(table, 0, (size_t)B * 2 * sizeof(int64_t), st));
  UNET_HIP(ctx, hipMemsetAsync(outside, 0, sizeof(int64_t), st));
  if (n > 0) {
    UNET_HIP(ctx, hipMemsetAsync(lesion_zone, 0, (size_t)n * (size_t)(2 * P) * sizeof(int64_t), st));
    UNET_HIP(ctx, hipMemsetAsync(lesion_shell, 0, (size_t)n * (size_t)S * sizeof(int64_t), st));
    UNET_HIP(ctx, hipMemsetAsync(lesion_dmin_key, 0xFF, (size_t)n * sizeof(uint64_t), st));
  }
  const unsigned long long* d = reinterpret_cast<const unsigned long long*>(d2);
  unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
  unsigned long long* ou = reinterpret_cast<unsigned long long*>(outside);
  unsigned long long* lz = reinterpret_cast<unsigned long long*>(lesion_zone);
  unsigned long long* lh = reinterpret_cast<unsigned long long*>(lesion_shell);
  unsigned long long* ld = reinterpret_cast<unsigned long long*>(lesion_dmin_key);
  const bool vec = vol_aligned(sides, 4) && vol_aligned(infection, 4) && vol_aligned(zone_map, 4) && vol_aligned(d2, 16) && vol_aligned(labels, 16);
  const bool lds = (long long)n * (2 * P + S) <= ZT_TABLE;
  const dim3 grid(zt_grid(vec ? (N + 3) / 4 : N));
#define ZT_LAUNCH(V, L) hipLaunchKernelGGL((zone_table_kernel<V, L>), grid, dim3(TPB), 0, st, sides, infection, labels, n, d, N, X, Y, prm, tb, ou, lz, lh, ld, zone_map)
  if (vec) { if (lds) ZT_LAUNCH(4, true); else ZT_LAUNCH(4, false); }
  else { if (lds) ZT_LAUNCH(1, true); else ZT_LAUNCH(1, false); }
#undef ZT_LAUNCH
  UNET_CHECK_LAUNCH(ctx, "vol_zone_table"); return UNET_OK;
}

}  // extern "C"

// Second-order texture of the CT under a mask: grey levels, the grey-level co-occurrence matrix (GLCM) and the grey-level run-length matrix (GLRLM)
// per group of a label volume (or one mask) and an optional region.
//   the decoded CT -> grey levels 1..Ng (0 = takes no part) + their first-order histogram per group          unet_vol_texture_quantize
//   C[g][k][a][b] += 1 for every voxel p and q = p + distance dir_k with levels a, b > 0 in one group g      unet_vol_texture_glcm
//   R[g][k][a][min(len, max_run)] += 1 for every maximal run of one level and one group along dir_k          unet_vol_texture_runs
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, decoded by vol_common.h's vol_dec.  The level of a non-NaN value is
// floor(fl(fl(v - lo) / width)), every operation rounded on its own (compiled with -ffp-contract=off like the other files that restate a float64 formula).
// GLCM: persistent workgroups of 256 lanes walk bricks of 32 x 8 x 8 voxels, x fastest.  A brick is staged in LDS with a halo of `distance` on +x, +-y and +-z (the 13
// directions all have dx >= 0), level and group per voxel, so the 13 neighbour reads of a voxel are LDS reads and a global byte is read about once.  A brick whose core
// holds no taking-part voxel is left after its levels were read (its labels never are); inside a brick a wave none of whose lanes takes part skips its 13 directions.
// While n K Ng^2 <= UNET_VOL_TEXTURE_LDS_COUNTERS the counts go to an int32 table in LDS (LDS atomics) and leave the workgroup as one 64-bit atomic per non-zero entry;
// beyond that every add is a 64-bit global atomic.  Integer atomics only, no workgroup waits for another: the same bits on every run.
// TEXTURE_GLCM_LDS=0 (make texture_loads, a measurement build that is never the product library) reads the neighbours straight from global memory instead.
#include "common.h"
#include "vol_common.h"

#include <cmath>

#ifndef TEXTURE_GLCM_LDS
#define TEXTURE_GLCM_LDS 1
#endif

namespace {
constexpr int TPB = 256;
constexpr int MAX_LEVELS = UNET_VOL_TEXTURE_MAX_LEVELS;
constexpr int MAX_DISTANCE = UNET_VOL_TEXTURE_MAX_DISTANCE;
constexpr int LDS_COUNTERS = UNET_VOL_TEXTURE_LDS_COUNTERS;          // int32 counters of a workgroup's GLCM table (32 KiB)
constexpr int MAX_RUN = 1 << 15;
constexpr int NDIR = 13;
constexpr int BX = 32, BY = 8, BZ = 8, BRICK = BX * BY * BZ;         // the brick a workgroup takes at a time: 8 voxels per lane
constexpr int GLCM_WG_PER_CU = 3;                                    // persistent workgroups of the GLCM launch per CU: 40 to 51 KiB of LDS each, three are resident in 160 KiB
// An int32 counter of the LDS table cannot overflow: one (voxel, direction) adds at most 1 to one counter, so a brick adds at most 13 * 2048 = 26,624 to any counter, and
// the table is flushed to the output every GLCM_FLUSH_BRICKS counted bricks: 65,536 * 26,624 = 1,744,830,464 < 2^31 - 1.
constexpr int GLCM_FLUSH_BRICKS = 65536;
static_assert((long long)GLCM_FLUSH_BRICKS * NDIR * BRICK < 0x7FFFFFFFLL, "the LDS counters are int32");
constexpr int TQ_TABLE = 4096;                                       // (group, level) counters of the quantize launch's LDS table (16 KiB); a workgroup sees < 2^31 voxels
constexpr long long GRID_CAP = 256 * 32;
constexpr int8_t DIRS[NDIR][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, -1, 0}, {1, 0, 1}, {1, 0, -1}, {0, 1, 1}, {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};

// the two counting kernels: `levels` says whether a voxel takes part, `labels` (null: one group) which group it is in.  (level, group) of voxel f, (0, 0) when it takes
// no part; a level above Ng or a label outside 1..n takes no part and is never an address.
__device__ __forceinline__ void tx_voxel(const uint8_t* __restrict__ levels, const int32_t* __restrict__ labels, int n, int Ng, long long f, int& a, int& g) {
  a = levels[f]; g = 0;
  if (a > Ng) a = 0;
  if (a) {
    const int l = labels ? labels[f] : 1;
    g = (unsigned)(l - 1) < (unsigned)n ? l : 0;
    if (!g) a = 0;
  }
}
// the selected directions of a launch, in ascending bit order, as voxel offsets (GLCM: already multiplied by the distance)
struct tx_dirlist { int count; int dx[NDIR], dy[NDIR], dz[NDIR]; };

// ---- (a) quantize ----------------------------------------------------------------------------------------------------------------------------------------
// A lane holds one voxel.  The lanes of a wave that share a (group, level) key are counted with one ballot (kernels_intensity.hip's ib_bands_kernel).  The loop bound and
// the barriers are uniform over the workgroup.
template <bool LDS_TABLE>
__global__ __launch_bounds__(TPB) void tq_quantize_kernel(vol_voxels src, vol_groups grp, long long N, double lo, double width, int Ng, int drop, uint8_t* __restrict__ levels,
                                                         unsigned long long* __restrict__ level_counts) {
  __shared__ int s_tab[LDS_TABLE ? TQ_TABLE : 1];
  const int tid = threadIdx.x, lane = tid & 63, n = grp.n;
  if constexpr (LDS_TABLE) {
    for (int i = tid; i < n * Ng; i += TPB) s_tab[i] = 0;
    __syncthreads();
  }
  for (long long base = (long long)blockIdx.x * TPB; base < N; base += (long long)gridDim.x * TPB) {
    const long long i = base + tid;
    const int g = i < N ? vol_group(grp, i) : 0;
    int lvl = 0;
    if (__ballot(g != 0)) {                                           // wave-uniform: most waves of a CT lie outside every lesion and never read a voxel
      if (g) {
        const double v = vol_dec(src, i);
        if (v == v) {
          const double q = floor(__ddiv_rn(__dsub_rn(v, lo), width));          // +-inf for an infinite v (lo is finite): clipped or dropped like any other q
          if (drop) { if (q >= 0.0 && q < (double)Ng) lvl = (int)q + 1; }
          else lvl = (int)fmin(fmax(q, 0.0), (double)(Ng - 1)) + 1;
        }
      }
      long long key = lvl ? (long long)(g - 1) * Ng + (lvl - 1) : -1;
      unsigned long long pending = __ballot(lvl != 0);
      while (pending) {                                               // one round per distinct key of the wave
        const int leader = __ffsll((long long)pending) - 1;
        const long long K = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == K);
        if (lane == leader) {
          const int cnt = __popcll(same);
          if constexpr (LDS_TABLE) atomicAdd(s_tab + K, cnt);
          else atomicAdd(level_counts + K, (unsigned long long)cnt);
        }
        pending &= ~same;
      }
    }
    if (i < N) levels[i] = (uint8_t)lvl;
  }
  if constexpr (LDS_TABLE) {
    __syncthreads();
    for (int i = tid; i < n * Ng; i += TPB) { const int v = s_tab[i]; if (v) atomicAdd(level_counts + i, (unsigned long long)v); }
  }
}

// ---- (b) GLCM ----------------------------------------------------------------------------------------------------------------------------------------------
// D: the distance (the halo).  SMALL: the counts fit the LDS table.  Then n Ng^2 <= 8192 too, so a staged voxel is ONE uint16: ((g - 1) << shift | (a - 1)) + 1 with
// 2^shift >= Ng the next power of two (< 2 Ng): at most n 2^shift < 16384 / Ng, and 0 = takes no part.  The largest staged brick (D = 4: 36 x 16 x 16 = 9216 voxels) is
// then 18 KiB beside the 32 KiB table: 50 KiB per workgroup.  Beyond the table a staged voxel is an int32 group and a uint8 level: 45 KiB, and no table.
// Every loop bound and every barrier is uniform over the workgroup: the brick loop, the core check and the 8 voxels of a lane, the staging loop (ceil(S / 1024) rounds of four voxels per lane), the direction list.
template <int D, bool SMALL>
__global__ __launch_bounds__(TPB) void tg_glcm_kernel(const uint8_t* __restrict__ levels, const int32_t* __restrict__ labels, int n, int X, int Y, int Z, int Ng, int shift,
                                                     tx_dirlist dl, int K, long long nbricks, int nbx, int nby, unsigned long long* __restrict__ counts) {
  constexpr int SX = BX + D, SY = BY + 2 * D, SZ = BZ + 2 * D, S = SX * SY * SZ;
  constexpr bool STAGED = TEXTURE_GLCM_LDS != 0;
  __shared__ uint16_t s_code[STAGED && SMALL ? S : 1];
  __shared__ int32_t s_grp[STAGED && !SMALL ? S : 1];
  __shared__ uint8_t s_lvl[STAGED && !SMALL ? S : 4];
  __shared__ int s_tab[SMALL ? LDS_COUNTERS : 1];
  const int tid = threadIdx.x;
  const int T = SMALL ? n * K * Ng * Ng : 0;                          // (<= LDS_COUNTERS: the host chose SMALL)
  const int amask = (1 << shift) - 1;
  if constexpr (SMALL) {
    for (int i = tid; i < T; i += TPB) s_tab[i] = 0;
    __syncthreads();
  }
  int counted = 0;                                                    // bricks counted into the table since its last flush (uniform)
  for (long long b = blockIdx.x; b < nbricks; b += gridDim.x) {
    const int bz = (int)(b / ((long long)nbx * nby)), br = (int)(b - (long long)bz * nbx * nby), by = br / nbx, bx = br - by * nbx;
    const int x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;
    if constexpr (STAGED) {
      // the core's levels first, 8 independent loads per lane: most bricks of a CT hold no taking-part voxel and end here, one memory latency after they began
      bool any = false;
#pragma unroll
      for (int j = 0; j < BRICK / TPB; ++j) {
        const int l = tid + j * TPB, gx = x0 + (l & (BX - 1)), gy = y0 + ((l >> 5) & (BY - 1)), gz = z0 + (l >> 8);
        int a = 0;
        if (gx < X && gy < Y && gz < Z) a = levels[gx + (long long)X * (gy + (long long)Y * gz)];
        any |= a != 0 && a <= Ng;
      }
      if (!__syncthreads_or(any ? 1 : 0)) continue;                   // uniform.  (Nothing reads the staged brick between this barrier and the next brick's.)
      // the brick and its halo, four voxels of a lane at a time: their level loads are issued together, the labels are read only where a level is set
      for (int r = 0; r < S; r += 4 * TPB) {                          // (uniform: ceil(S / 1024) rounds)
        const int i0 = r + tid;
        int a[4], g[4];
        long long f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * TPB, sx = i % SX, t = i / SX, sy = t % SY, sz = t / SY;
          const int gx = x0 + sx, gy = y0 + sy - D, gz = z0 + sz - D;
          a[u] = 0; g[u] = 0; f[u] = gx + (long long)X * (gy + (long long)Y * gz);
          if (i < S && gx < X && gy >= 0 && gy < Y && gz >= 0 && gz < Z) a[u] = levels[f[u]];
          if (a[u] > Ng) a[u] = 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (a[u]) {
            const int l = labels ? labels[f[u]] : 1;
            g[u] = (unsigned)(l - 1) < (unsigned)n ? l : 0;
            if (!g[u]) a[u] = 0;
          }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * TPB;
          if (i < S) {
            if constexpr (SMALL) s_code[i] = a[u] ? (uint16_t)((((g[u] - 1) << shift) | (a[u] - 1)) + 1) : (uint16_t)0;
            else { s_grp[i] = g[u]; s_lvl[i] = (uint8_t)a[u]; }
          }
        }
      }
      __syncthreads();
    }
    for (int j = 0; j < BRICK / TPB; ++j) {
      const int l = tid + j * TPB, lx = l & (BX - 1), ly = (l >> 5) & (BY - 1), lz = l >> 8;
      int a = 0, g = 0;
      [[maybe_unused]] int si = 0;
      [[maybe_unused]] const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
      if constexpr (STAGED) {
        si = lx + SX * ((ly + D) + SY * (lz + D));
        if constexpr (SMALL) { const int c = s_code[si]; if (c) { g = ((c - 1) >> shift) + 1; a = ((c - 1) & amask) + 1; } }
        else { a = s_lvl[si]; g = s_grp[si]; }
      } else {
        if (gx < X && gy < Y && gz < Z) tx_voxel(levels, labels, n, Ng, gx + (long long)X * (gy + (long long)Y * gz), a, g);
      }
      if (!__ballot(a != 0)) continue;                                // wave-uniform: none of the 64 voxels takes part
      for (int k = 0; k < dl.count; ++k) {
        int bq = 0, gq = 0;
        if constexpr (STAGED) {
          const int qi = si + dl.dx[k] + SX * (dl.dy[k] + SY * dl.dz[k]);          // inside the staged brick: 0 <= dx <= D, |dy|, |dz| <= D
          if constexpr (SMALL) { const int c = s_code[qi]; if (c) { gq = ((c - 1) >> shift) + 1; bq = ((c - 1) & amask) + 1; } }
          else { bq = s_lvl[qi]; gq = s_grp[qi]; }
        } else {
          const int qx = gx + dl.dx[k], qy = gy + dl.dy[k], qz = gz + dl.dz[k];
          if (a && qx < X && (unsigned)qy < (unsigned)Y && (unsigned)qz < (unsigned)Z) tx_voxel(levels, labels, n, Ng, qx + (long long)X * (qy + (long long)Y * qz), bq, gq);
        }
        if (a && bq && g == gq) {
          const long long idx = (((long long)(g - 1) * K + (K == 1 ? 0 : k)) * Ng + (a - 1)) * Ng + (bq - 1);
          if constexpr (SMALL) atomicAdd(s_tab + (int)idx, 1);
          else atomicAdd(counts + idx, 1ull);
        }
      }
    }
    if constexpr (STAGED) __syncthreads();                            // the staged brick was read: the next one may be written
    if constexpr (SMALL) {
      if (++counted == GLCM_FLUSH_BRICKS) {                           // uniform
        __syncthreads();
        for (int i = tid; i < T; i += TPB) { const int v = s_tab[i]; if (v) { atomicAdd(counts + i, (unsigned long long)v); s_tab[i] = 0; } }
        __syncthreads();
        counted = 0;
      }
    }
  }
  if constexpr (SMALL) {
    __syncthreads();
    for (int i = tid; i < T; i += TPB) { const int v = s_tab[i]; if (v) atomicAdd(counts + i, (unsigned long long)v); }
  }
}

// ---- (c) runs ------------------------------------------------------------------------------------------------------------------------------------------------
// A lane holds one voxel; the lane of a run's first voxel (its predecessor along the direction lies outside the volume, or differs in level or group) walks the run.
// The walk ends at the volume's border at the latest.  64-bit global atomics; a wave none of whose lanes takes part skips everything.
__global__ __launch_bounds__(TPB) void tr_runs_kernel(const uint8_t* __restrict__ levels, const int32_t* __restrict__ labels, int n, int X, int Y, int Z, int Ng, tx_dirlist dl,
                                                     int max_run, long long N, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ clamped) {
  const int K = dl.count;
  for (long long base = (long long)blockIdx.x * TPB; base < N; base += (long long)gridDim.x * TPB) {
    const long long i = base + threadIdx.x;
    int a = 0, g = 0;
    if (i < N) tx_voxel(levels, labels, n, Ng, i, a, g);
    if (!__ballot(a != 0)) continue;                                  // wave-uniform
    if (!a) continue;
    const int x = (int)(i % X), y = (int)((i / X) % Y), z = (int)(i / ((long long)X * Y));
    for (int k = 0; k < K; ++k) {
      const int dx = dl.dx[k], dy = dl.dy[k], dz = dl.dz[k];
      const long long step = dx + (long long)X * (dy + (long long)Y * dz);
      const int px = x - dx, py = y - dy, pz = z - dz;
      if (px >= 0 && (unsigned)py < (unsigned)Y && (unsigned)pz < (unsigned)Z) {
        int ap, gp;
        tx_voxel(levels, labels, n, Ng, i - step, ap, gp);
        if (ap == a && gp == g) continue;                             // the run began earlier
      }
      int len = 1, qx = x + dx, qy = y + dy, qz = z + dz;
      long long f = i + step;
      while (qx < X && (unsigned)qy < (unsigned)Y && (unsigned)qz < (unsigned)Z) {
        int aq, gq;
        tx_voxel(levels, labels, n, Ng, f, aq, gq);
        if (aq != a || gq != g) break;
        ++len; qx += dx; qy += dy; qz += dz; f += step;
      }
      const long long row = (long long)(g - 1) * K + k;
      atomicAdd(counts + (row * Ng + (a - 1)) * max_run + (min(len, max_run) - 1), 1ull);
      if (len > max_run) atomicAdd(clamped + row, 1ull);
    }
  }
}

// the checks the two counting entry points share -> 0, or the message of the refusal
const char* tx_count_refusal(int X, int Y, int Z, int n, int Ng, int directions) {
  if (!vol_dims_ok(X, Y, Z)) return "a dimension is negative or the volume has 2^31 voxels or more";
  if (n < 0) return "n is negative";
  if (Ng < 1 || Ng > MAX_LEVELS) return "Ng lies in 1 .. UNET_VOL_TEXTURE_MAX_LEVELS";
  if (directions <= 0 || (directions >> NDIR) != 0) return "directions is a non-empty set of the bits 0 .. 12";
  return nullptr;
}
tx_dirlist tx_dirs(int directions, int scale) {
  tx_dirlist dl{};
  for (int k = 0; k < NDIR; ++k)
    if ((directions >> k) & 1) { dl.dx[dl.count] = DIRS[k][0] * scale; dl.dy[dl.count] = DIRS[k][1] * scale; dl.dz[dl.count] = DIRS[k][2] * scale; ++dl.count; }
  return dl;
}
template <int D>
void tg_launch(bool small, hipStream_t s, unsigned grid, const uint8_t* levels, const int32_t* labels, int n, int X, int Y, int Z, int Ng, int shift, const tx_dirlist& dl, int K,
               long long nbricks, int nbx, int nby, unsigned long long* counts) {
  if (small) hipLaunchKernelGGL((tg_glcm_kernel<D, true>), dim3(grid), dim3(TPB), 0, s, levels, labels, n, X, Y, Z, Ng, shift, dl, K, nbricks, nbx, nby, counts);
  else hipLaunchKernelGGL((tg_glcm_kernel<D, false>), dim3(grid), dim3(TPB), 0, s, levels, labels, n, X, Y, Z, Ng, shift, dl, K, nbricks, nbx, nby, counts);
}
}  // namespace

extern "C" {

int32_t unet_vol_texture_quantize(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                                  const int32_t* labels, const uint8_t* mask, int32_t n, const uint8_t* region, double lo, double width, int32_t Ng, int32_t outside,
                                  uint8_t* levels, int64_t* level_counts, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: a dimension is negative or the volume has 2^31 voxels or more");
  if (vol_itemsize(dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: the NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64");
  if ((labels != nullptr) == (mask != nullptr)) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: exactly one of labels and mask is given");
  if (n < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: n is negative");
  if (Ng < 1 || Ng > MAX_LEVELS) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: 1 to %d levels are taken, not %d", MAX_LEVELS, Ng);
  if (!std::isfinite(lo) || !std::isfinite(width) || !(width > 0.0)) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: lo is finite and width finite and > 0");
  if (outside != 0 && outside != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: outside is 0 (clip) or 1 (drop), not %d", outside);
  const long long N = (long long)X * Y * Z;
  if ((n > 0 && !level_counts) || (reinterpret_cast<uintptr_t>(level_counts) % 8) != 0 || (N > 0 && !levels))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: null or misaligned output");
  if (N > 0 && (!vox || (reinterpret_cast<uintptr_t>(vox) % vol_itemsize(dtype)) != 0 || (labels && (reinterpret_cast<uintptr_t>(labels) % 4) != 0)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_quantize: null voxel buffer, or a buffer not aligned to its item size");
  hipStream_t s = as_stream(stream);
  if (n > 0) UNET_HIP(ctx, hipMemsetAsync(level_counts, 0, (size_t)n * Ng * sizeof(int64_t), s));
  if (N == 0) return UNET_OK;
  const vol_voxels src{vox, dtype, scaled ? 1 : 0, slope, inter};
  const vol_groups grp{labels, mask, region, n};
  unsigned long long* lc = reinterpret_cast<unsigned long long*>(level_counts);
  if ((long long)n * Ng <= TQ_TABLE) hipLaunchKernelGGL(tq_quantize_kernel<true>, dim3(vol_blocks(N, GRID_CAP, TPB)), dim3(TPB), 0, s, src, grp, N, lo, width, Ng, outside, levels, lc);
  else hipLaunchKernelGGL(tq_quantize_kernel<false>, dim3(vol_blocks(N, GRID_CAP, TPB)), dim3(TPB), 0, s, src, grp, N, lo, width, Ng, outside, levels, lc);
  UNET_CHECK_LAUNCH(ctx, "vol_texture_quantize"); return UNET_OK;
}

int32_t unet_vol_texture_glcm(unet_ctx* ctx, const uint8_t* levels, const int32_t* labels, int32_t n, int32_t X, int32_t Y, int32_t Z, int32_t Ng, int32_t distance,
                              int32_t directions, int32_t merge, int64_t* counts, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (const char* why = tx_count_refusal(X, Y, Z, n, Ng, directions)) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_glcm: %s", why);
  if (distance < 1 || distance > MAX_DISTANCE) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_glcm: the distance lies in 1 .. %d, not %d", MAX_DISTANCE, distance);
  const tx_dirlist dl = tx_dirs(directions, distance);
  const int K = merge ? 1 : dl.count;
  const long long N = (long long)X * Y * Z, table = (long long)n * K * Ng * Ng;
  if ((table > 0 && !counts) || (reinterpret_cast<uintptr_t>(counts) % 8) != 0 || (N > 0 && !levels) || (reinterpret_cast<uintptr_t>(labels) % 4) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_glcm: null or misaligned buffer");
  hipStream_t s = as_stream(stream);
  if (table > 0) UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)table * sizeof(int64_t), s));
  if (N == 0 || n == 0) return UNET_OK;
  const int nbx = (X + BX - 1) / BX, nby = (Y + BY - 1) / BY, nbz = (Z + BZ - 1) / BZ;
  const long long nbricks = (long long)nbx * nby * nbz;
  const long long resident = (long long)(ctx->num_cu > 0 ? ctx->num_cu : 256) * GLCM_WG_PER_CU;
  const unsigned grid = (unsigned)(nbricks < resident ? nbricks : resident);
  int shift = 0;
  while ((1 << shift) < Ng) ++shift;
  const bool small = table <= LDS_COUNTERS;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  switch (distance) {
    case 1: tg_launch<1>(small, s, grid, levels, labels, n, X, Y, Z, Ng, shift, dl, K, nbricks, nbx, nby, out); break;
    case 2: tg_launch<2>(small, s, grid, levels, labels, n, X, Y, Z, Ng, shift, dl, K, nbricks, nbx, nby, out); break;
    case 3: tg_launch<3>(small, s, grid, levels, labels, n, X, Y, Z, Ng, shift, dl, K, nbricks, nbx, nby, out); break;
    default: tg_launch<4>(small, s, grid, levels, labels, n, X, Y, Z, Ng, shift, dl, K, nbricks, nbx, nby, out); break;
  }
  UNET_CHECK_LAUNCH(ctx, "vol_texture_glcm"); return UNET_OK;
}

int32_t unet_vol_texture_runs(unet_ctx* ctx, const uint8_t* levels, const int32_t* labels, int32_t n, int32_t X, int32_t Y, int32_t Z, int32_t Ng, int32_t directions,
                              int32_t max_run, int64_t* counts, int64_t* clamped, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (const char* why = tx_count_refusal(X, Y, Z, n, Ng, directions)) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_runs: %s", why);
  if (max_run < 1 || max_run > MAX_RUN) UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_runs: max_run lies in 1 .. %d, not %d", MAX_RUN, max_run);
  const tx_dirlist dl = tx_dirs(directions, 1);
  const long long N = (long long)X * Y * Z, rows = (long long)n * dl.count;
  if ((rows > 0 && (!counts || !clamped)) || (reinterpret_cast<uintptr_t>(counts) % 8) != 0 || (reinterpret_cast<uintptr_t>(clamped) % 8) != 0 || (N > 0 && !levels) ||
      (reinterpret_cast<uintptr_t>(labels) % 4) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_texture_runs: null or misaligned buffer");
  hipStream_t s = as_stream(stream);
  if (rows > 0) {
    UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)rows * Ng * max_run * sizeof(int64_t), s));
    UNET_HIP(ctx, hipMemsetAsync(clamped, 0, (size_t)rows * sizeof(int64_t), s));
  }
  if (N == 0 || n == 0) return UNET_OK;
  hipLaunchKernelGGL(tr_runs_kernel, dim3(vol_blocks(N, GRID_CAP, TPB)), dim3(TPB), 0, s, levels, labels, n, X, Y, Z, Ng, dl, max_run, N, reinterpret_cast<unsigned long long*>(counts),
                     reinterpret_cast<unsigned long long*>(clamped));
  UNET_CHECK_LAUNCH(ctx, "vol_texture_runs"); return UNET_OK;
}

}  // extern "C"

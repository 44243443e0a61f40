// Marker-controlled watershed and cost-weighted geodesic distance on a volume, and the depth cost that split_lesions feeds it.
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31; outside the volume there is nothing; extents of 1 are legal.
//   unet_vol_watershed_begin / _sweeps / _end     seed a phase, n sweeps of it, unpack to the outputs and the four counts
//   unet_vol_depth_cost                           cost = floor((d2max - d2) / quantum) inside the mask, 0 outside
// cost uint32; markers int32, 1 .. 2^24 - 1 a marker, 0 none, anything else invalid: counted, treated as none, never an address; mask bytes (or null = everywhere), a
// voxel outside it takes no part and a marker outside it is ignored.  Neighbours: generate_binary_structure(3, connectivity).
// Every phase iterates one monotone operator downwards from "unreached" (~0) on a 64-bit key per voxel; marker voxels hold their seed, voxels outside the mask stay ~0:
//   HEIGHT  key = H, the pass height.  marker: cost[v].  else H[v] = min_n max(H[n], cost[v]).                                      (ws_relax_height)
//   LABEL   key = steps << 32 | label over the finished H.  marker: (0, label).  else min over the TIGHT neighbours (max(H[n], cost[v]) == H[v]) of key[n] + (1 << 32).
//           A voxel goes to the marker nearest in steps along pass-height-realising paths, the lowest label among equally near ones.     (ws_relax_label)
//   SUM     key = dist << 24 | label, dist 40 bits.  marker: (0, label).  else min_n (dist[n] + cost[v], label[n]); a candidate whose distance would pass 2^40 - 2 is
//           no candidate (dropping keeps the operator monotone, saturating would not).                                                  (ws_relax_sum)
// Why two phases for the watershed: height << k | label in one key is not monotone -- (3, label 2) < (4, label 1), but through a voxel of cost 5 they become
// (5, 2) > (5, 1) -- so its limit depends on the order of updates.  Each operator above is monotone (min and max of monotone terms; "tight" is decided on the finished
// H, a constant of the LABEL phase), the start (seeds, else ~0) is a post-fixed point, so the values only decrease over a finite set and the limit is the greatest fixed
// point below the start whatever the order of updates.
// One sweep is one launch of at most GRID_CAP persistent workgroups of 256 lanes (a BOUNDED grid: a workgroup walks the bricks b = blockIdx.x, + gridDim.x, ...) over
// 32 x 8 x 8 bricks.  A lane owns the eight voxels (lx, ly, lz = 0 .. 7) of a column of the brick: their cost, their part in the mask and their marker flag stay in its
// registers (no other lane needs them, so they are not staged).  The keys of the brick are staged in LDS with a halo of 1 (outside the volume: ~0), for LABEL the heights
// with a halo of 1 too.  The halo is frozen; a pass computes every interior voxel's relaxation from LDS into registers, a workgroup-wide flag (__syncthreads_or, which is
// also the barrier between the pass's reads and its writes) ends the loop when no voxel changed, else the changed keys are written to LDS behind a second barrier.  The loop
// ends because values only decrease over a finite set, and its limit is unique (the same argument, on the brick with a constant halo).  The interior is then written to
// the OTHER of two global key buffers: sweep s reads buffer s & 1 and writes buffer (s + 1) & 1.  A launch reads only what earlier launches wrote and every element is
// written by one lane, so every sweep, every changed[s] and the number of sweeps are the same on every run.  changed[s] = the voxels whose key sweep s lowered: one 64-bit
// integer atomic per workgroup, the only atomic of the file.  No workgroup waits for another.  Integer arithmetic only (the depth cost aside).
// Skipping.  _begin seeds BOTH buffers alike.  A brick with no voxel in the mask is never staged: both buffers keep ~0 there.  flag_s[b] = sweep s lowered a key of brick
// b; the flags are ping-ponged like the keys (sweep s reads F[s & 1], writes F[(s + 1) & 1]; _begin sets F[0] all-active).  With skip != 0 sweep s leaves out a brick
// whose own flag and 26 neighbour bricks' flags of sweep s - 1 are all clear, and clears its flag.  Call R the buffer sweep s reads and W the one it writes, f(b; R) what
// staging brick b from R produces.
//   (I) a brick whose flag of sweep s - 1 is clear holds equal content in R and W.  If it was staged in s - 1 it wrote to R exactly what it read from W; if it was skipped
//       then (I) held one sweep earlier and nothing was written since.
//   (K) a brick whose 27 flags of sweep s - 1 are clear has f(b; R) = R[b].  If it was staged in s - 1: R[b] = f(b; W), and by (I) W equals R on all 27 bricks, on which
//       alone f depends (the halo is 1 wide).  If it was skipped in s - 1: (K) held then, and by (I) the 27 bricks are the same in both buffers.
//   So skipping writes what staging would have written: W[b] = R[b] = f(b; R).  Sweep 0 skips nothing.
// After a sweep with changed == 0 both buffers are equal and further sweeps change nothing; _begin (LABEL, to fetch H) and _end take the number of sweeps run and read the
// buffer the last one wrote.
#include "common.h"
#include "vol_common.h"

namespace {
typedef unsigned long long u64;
constexpr int WS_TPB = 256;
constexpr int WS_BX = 32, WS_BY = 8, WS_BZ = 8, WS_PER_LANE = WS_BX * WS_BY * WS_BZ / WS_TPB;          // 8: the column lz = 0 .. 7 of (lx, ly) = (lane & 31, lane >> 5)
constexpr int WS_HX = WS_BX + 2, WS_HY = WS_BY + 2, WS_HZ = WS_BZ + 2, WS_HALO = WS_HX * WS_HY * WS_HZ;          // 3400 staged cells
constexpr long long GRID_CAP = 2048;                                 // persistent workgroups of a sweep: 8 per CU; 3 are resident at a time (131 VGPRs, 40 KiB of LDS each)
constexpr long long WS_FLAT_CAP = 1024;                              // workgroups of the per-voxel launches (seed, unpack, depth cost): grid-stride
constexpr u64 WS_UNREACHED = ~0ull;
constexpr uint32_t WS_H_UNREACHED = 0xFFFFFFFFu;
constexpr u64 WS_DIST_MAX = (1ull << 40) - 2;                        // the largest distance a SUM key carries
constexpr int32_t WS_LABEL_MAX = (1 << 24) - 1;
enum { WS_HEIGHT = UNET_VOL_WATERSHED_HEIGHT, WS_LABEL = UNET_VOL_WATERSHED_LABEL, WS_SUM = UNET_VOL_WATERSHED_SUM };

// ---- the relaxation of one voxel, three forms.  K (and H): arrays with a margin of 1 around every voxel that is relaxed, c the voxel's index, 1 / sy / sz the strides ----
template <typename F>
__host__ __device__ __forceinline__ void ws_each_neighbour(int conn, int sy, int sz, F f) {
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int n = (dx != 0) + (dy != 0) + (dz != 0);
        if (n == 0 || n > conn) continue;                             // generate_binary_structure(3, conn): a move along at most conn axes
        f(dx + dy * sy + dz * sz);
      }
}
__host__ __device__ __forceinline__ u64 ws_relax_height(const u64* K, int c, int sy, int sz, int conn, uint32_t cost, u64 cur) {
  u64 best = cur;
  ws_each_neighbour(conn, sy, sz, [&](int o) {
    const u64 hn = K[c + o];
    if (hn == WS_UNREACHED) return;
    const u64 v = hn > cost ? hn : (u64)cost;
    if (v < best) best = v;
  });
  return best;
}
__host__ __device__ __forceinline__ u64 ws_relax_label(const u64* K, const uint32_t* H, int c, int sy, int sz, int conn, uint32_t cost, u64 cur) {
  const uint32_t hv = H[c];
  if (hv == WS_H_UNREACHED) return cur;                                // no marker is connected: no edge is tight
  u64 best = cur;
  ws_each_neighbour(conn, sy, sz, [&](int o) {
    const u64 kn = K[c + o];
    if (kn == WS_UNREACHED) return;
    const uint32_t hn = H[c + o];
    if ((hn > cost ? hn : cost) != hv) return;                        // not tight
    const u64 cand = kn + (1ull << 32);
    if (cand < best) best = cand;
  });
  return best;
}
__host__ __device__ __forceinline__ u64 ws_relax_sum(const u64* K, int c, int sy, int sz, int conn, uint32_t cost, u64 cur) {
  u64 best = cur;
  ws_each_neighbour(conn, sy, sz, [&](int o) {
    const u64 kn = K[c + o];
    if (kn == WS_UNREACHED) return;
    const u64 dist = (kn >> 24) + cost;
    if (dist > WS_DIST_MAX) return;                                   // no candidate
    const u64 cand = (dist << 24) | (kn & 0xFFFFFFull);
    if (cand < best) best = cand;
  });
  return best;
}
__host__ __device__ __forceinline__ u64 ws_relax(int phase, const u64* K, const uint32_t* H, int c, int sy, int sz, int conn, uint32_t cost, u64 cur) {
  return phase == WS_HEIGHT ? ws_relax_height(K, c, sy, sz, conn, cost, cur) : phase == WS_LABEL ? ws_relax_label(K, H, c, sy, sz, conn, cost, cur)
                                                                                               : ws_relax_sum(K, c, sy, sz, conn, cost, cur);
}
__host__ __device__ __forceinline__ bool ws_marker_ok(int32_t m) { return m >= 1 && m <= WS_LABEL_MAX; }
// the seed of a voxel: inmask and marker as the launch found them
__host__ __device__ __forceinline__ u64 ws_seed(int phase, bool inmask, int32_t m, uint32_t cost) {
  if (!inmask || !ws_marker_ok(m)) return WS_UNREACHED;
  return phase == WS_HEIGHT ? (u64)cost : (u64)(uint32_t)m;          // LABEL: steps 0, SUM: distance 0
}

// ---- bricks ----------------------------------------------------------------------------------------------------------------------------------------------------------
struct ws_dims { int X, Y, Z, NBX, NBY, NBZ; long long N, nb; };
inline ws_dims ws_dims_make(int X, int Y, int Z) {
  const int NBX = (X + WS_BX - 1) / WS_BX, NBY = (Y + WS_BY - 1) / WS_BY, NBZ = (Z + WS_BZ - 1) / WS_BZ;
  return {X, Y, Z, NBX, NBY, NBZ, (long long)X * Y * Z, (long long)NBX * NBY * NBZ};
}
// the brick-activity rule: brick b is staged when its own flag or one of its 26 neighbour bricks' flags of the previous sweep is set
__host__ __device__ inline bool ws_brick_active(const uint8_t* flags, const ws_dims& d, long long b) {
  const long long row = b / d.NBX;
  const int bx = (int)(b - row * d.NBX), bz = (int)(row / d.NBY), by = (int)(row - (long long)bz * d.NBY);
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = bx + dx, y = by + dy, z = bz + dz;
        if (x < 0 || x >= d.NBX || y < 0 || y >= d.NBY || z < 0 || z >= d.NBZ) continue;
        if (flags[x + (long long)d.NBX * (y + (long long)d.NBY * z)]) return true;
      }
  return false;
}

// the workspace: key buffers A and B, the heights, brick-in-mask bytes, two flag arrays, the per-workgroup partial counts (4 int64 each)
struct ws_layout { size_t A, B, H, bmask, F0, F1, part, total; };
inline ws_layout ws_layout_of(const ws_dims& d) {
  ws_layout L;
  const size_t keys = vol_pad16((size_t)d.N * 8), hts = vol_pad16((size_t)d.N * 4), fl = vol_pad16((size_t)d.nb);
  L.A = 0; L.B = keys; L.H = 2 * keys; L.bmask = L.H + hts; L.F0 = L.bmask + fl; L.F1 = L.F0 + fl; L.part = L.F1 + fl;
  L.total = L.part + (size_t)WS_FLAT_CAP * 4 * sizeof(long long);
  return L;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WS_TPB) void ws_seed_kernel(const uint32_t* __restrict__ cost, const int32_t* __restrict__ markers, const uint8_t* __restrict__ mask, ws_dims d,
                                                        int phase, const u64* prev, u64* A, u64* B, uint32_t* __restrict__ H, uint8_t* __restrict__ bmask,
                                                        long long* __restrict__ part) {
  __shared__ long long s_w[WS_TPB / 64];
  long long invalid = 0;
  for (long long f = (long long)blockIdx.x * WS_TPB + threadIdx.x; f < d.N; f += (long long)gridDim.x * WS_TPB) {
    if (phase == WS_LABEL) {                                          // the finished heights, before this lane overwrites the element they come from
      const u64 h = prev[f];
      H[f] = h == WS_UNREACHED ? WS_H_UNREACHED : (uint32_t)h;
    }
    const int32_t m = markers[f];
    const bool inmask = !mask || mask[f] != 0;
    if (m != 0 && !ws_marker_ok(m)) ++invalid;
    const u64 k = ws_seed(phase, inmask, m, cost[f]);
    A[f] = k; B[f] = k;
    if (inmask) {
      const long long row = f / d.X;
      const int x = (int)(f - row * d.X), z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
      bmask[(x / WS_BX) + (long long)d.NBX * ((y / WS_BY) + (long long)d.NBY * (z / WS_BZ))] = 1;          // (every writer stores the same byte)
    }
  }
  const long long t = vol_block_sum<long long, WS_TPB>(invalid, s_w);
  if (threadIdx.x == 0) part[4 * blockIdx.x + 3] = t;
}

__global__ __launch_bounds__(WS_TPB) void ws_sweep_kernel(const u64* __restrict__ R, u64* __restrict__ W, const uint32_t* __restrict__ cost,
                                                         const int32_t* __restrict__ markers, const uint8_t* __restrict__ mask, const uint32_t* __restrict__ Hg, ws_dims d,
                                                         int phase, int conn, int skip, const uint8_t* __restrict__ bmask, const uint8_t* __restrict__ FR,
                                                         uint8_t* __restrict__ FW, u64* __restrict__ changed) {
  __shared__ u64 s_k[WS_HALO];
  __shared__ uint32_t s_h[WS_HALO];
  __shared__ int s_w[WS_TPB / 64];
  const int t = threadIdx.x, lx = t & (WS_BX - 1), ly = t >> 5;
  long long total = 0;                                                // the same in every lane
  for (long long b = blockIdx.x; b < d.nb; b += gridDim.x) {
    if (!bmask[b] || (skip && !ws_brick_active(FR, d, b))) {          // workgroup-uniform
      if (t == 0) FW[b] = 0;
      continue;
    }
    const long long brow = b / d.NBX;
    const int bx = (int)(b - brow * d.NBX), bz = (int)(brow / d.NBY), by = (int)(brow - (long long)bz * d.NBY);
    const int x0 = bx * WS_BX, y0 = by * WS_BY, z0 = bz * WS_BZ;
    for (int i = t; i < WS_HALO; i += WS_TPB) {                       // keys (and heights) with their halo; outside the volume: unreached
      const int hx = i % WS_HX, hr = i / WS_HX, hy = hr % WS_HY, hz = hr / WS_HY;
      const int x = x0 + hx - 1, y = y0 + hy - 1, z = z0 + hz - 1;
      const bool in = x >= 0 && x < d.X && y >= 0 && y < d.Y && z >= 0 && z < d.Z;
      const long long f = x + (long long)d.X * (y + (long long)d.Y * z);
      s_k[i] = in ? R[f] : WS_UNREACHED;
      if (phase == WS_LABEL) s_h[i] = in ? Hg[f] : WS_H_UNREACHED;
    }
    uint32_t c[WS_PER_LANE];
    u64 cur[WS_PER_LANE], orig[WS_PER_LANE];
    unsigned live = 0, inside = 0;                                    // bit j: voxel j is relaxed / lies in the volume
    const int x = x0 + lx, y = y0 + ly;
#pragma unroll
    for (int j = 0; j < WS_PER_LANE; ++j) {
      const int z = z0 + j;
      c[j] = 0; orig[j] = WS_UNREACHED;
      if (x < d.X && y < d.Y && z < d.Z) {
        const long long f = x + (long long)d.X * (y + (long long)d.Y * z);
        inside |= 1u << j;
        c[j] = cost[f];
        orig[j] = R[f];
        if ((!mask || mask[f] != 0) && !ws_marker_ok(markers[f])) live |= 1u << j;
      }
      cur[j] = orig[j];
    }
    __syncthreads();
    for (;;) {
      u64 nw[WS_PER_LANE];
      int any = 0;
#pragma unroll
      for (int j = 0; j < WS_PER_LANE; ++j) {
        nw[j] = cur[j];
        if ((live >> j) & 1u) {
          nw[j] = ws_relax(phase, s_k, s_h, (lx + 1) + WS_HX * ((ly + 1) + WS_HY * (j + 1)), WS_HX, WS_HX * WS_HY, conn, c[j], cur[j]);
          any |= nw[j] != cur[j];
        }
      }
      if (!__syncthreads_or(any)) break;                              // every lane has read what it needs of this pass
#pragma unroll
      for (int j = 0; j < WS_PER_LANE; ++j)
        if (nw[j] != cur[j]) { cur[j] = nw[j]; s_k[(lx + 1) + WS_HX * ((ly + 1) + WS_HY * (j + 1))] = nw[j]; }
      __syncthreads();
    }
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < WS_PER_LANE; ++j)
      if ((inside >> j) & 1u) {
        W[x + (long long)d.X * (y + (long long)d.Y * (z0 + j))] = cur[j];          // the whole interior: W holds the state of two sweeps ago
        cnt += cur[j] != orig[j];
      }
    const int bt = vol_block_sum<int, WS_TPB>(cnt, s_w);              // (its barrier also stands between this brick's last LDS read and the next brick's staging)
    if (t == 0) FW[b] = bt != 0;
    total += bt;
    __syncthreads();                                                  // s_w is read by every lane before the next brick's sum writes it
  }
  if (t == 0 && total) atomicAdd(changed, (u64)total);               // integer sums: exact in any order
}

// unpack: keys -> outputs, and per workgroup the counts reached / unreached in the mask / overflowed
__global__ __launch_bounds__(WS_TPB) void ws_unpack_kernel(const u64* __restrict__ K, const uint32_t* __restrict__ Hg, const uint8_t* __restrict__ mask, ws_dims d, int phase,
                                                          int conn, int32_t* __restrict__ labels, uint32_t* __restrict__ height, uint32_t* __restrict__ steps,
                                                          u64* __restrict__ distance, long long* __restrict__ part) {
  __shared__ long long s_w[WS_TPB / 64];
  long long reached = 0, unreached = 0, overflowed = 0;
  for (long long f = (long long)blockIdx.x * WS_TPB + threadIdx.x; f < d.N; f += (long long)gridDim.x * WS_TPB) {
    const u64 k = K[f];
    const bool inmask = !mask || mask[f] != 0, got = k != WS_UNREACHED;
    if (phase == WS_HEIGHT) {
      height[f] = got ? (uint32_t)k : WS_H_UNREACHED;
    } else if (phase == WS_LABEL) {
      labels[f] = got ? (int32_t)(uint32_t)k : 0;
      steps[f] = got ? (uint32_t)(k >> 32) : WS_H_UNREACHED;
      if (height) height[f] = Hg[f];
    } else {
      labels[f] = got ? (int32_t)(k & 0xFFFFFFull) : 0;
      distance[f] = k >> 24;                                          // unreached: 2^40 - 1
    }
    if (got) ++reached;
    else if (inmask) {
      ++unreached;
      if (phase == WS_SUM) {                                          // beside a reached neighbour: only the distance limit can have kept it out
        const long long row = f / d.X;
        const int x = (int)(f - row * d.X), z = (int)(row / d.Y), y = (int)(row - (long long)z * d.Y);
        bool beside = false;
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int n = (dx != 0) + (dy != 0) + (dz != 0), xx = x + dx, yy = y + dy, zz = z + dz;
              if (n == 0 || n > conn || xx < 0 || xx >= d.X || yy < 0 || yy >= d.Y || zz < 0 || zz >= d.Z) continue;
              if (K[xx + (long long)d.X * (yy + (long long)d.Y * zz)] != WS_UNREACHED) beside = true;
            }
        if (beside) ++overflowed;
      }
    }
  }
  const long long r = vol_block_sum<long long, WS_TPB>(reached, s_w);
  __syncthreads();
  const long long u = vol_block_sum<long long, WS_TPB>(unreached, s_w);
  __syncthreads();
  const long long o = vol_block_sum<long long, WS_TPB>(overflowed, s_w);
  if (threadIdx.x == 0) { part[4 * blockIdx.x] = r; part[4 * blockIdx.x + 1] = u; part[4 * blockIdx.x + 2] = o; }
}
// one workgroup: the partial counts of `groups` workgroups -> counts[4], added in index order
__global__ __launch_bounds__(WS_TPB) void ws_counts_kernel(const long long* __restrict__ part, int groups, long long* __restrict__ counts) {
  if (threadIdx.x < 4) {
    long long t = 0;
    for (int g = 0; g < groups; ++g) t += part[4 * g + threadIdx.x];
    counts[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(WS_TPB) void ws_depth_cost_kernel(const double* __restrict__ d2, const uint8_t* __restrict__ mask, long long N, double d2max, double quantum,
                                                              uint32_t* __restrict__ cost) {
  for (long long f = (long long)blockIdx.x * WS_TPB + threadIdx.x; f < N; f += (long long)gridDim.x * WS_TPB) {
    uint32_t c = 0;
    if (!mask || mask[f] != 0) {
      const double q = floor(__ddiv_rn(__dsub_rn(d2max, d2[f]), quantum));          // two rounded operations; floor is exact
      c = q >= 4294967294.0 ? 0xFFFFFFFEu : (q > 0.0 ? (uint32_t)q : 0u);          // (a NaN compares false twice: 0)
    }
    cost[f] = c;
  }
}

inline bool ws_phase_ok(int p) { return p == WS_HEIGHT || p == WS_LABEL || p == WS_SUM; }
}  // namespace

extern "C" {

size_t unet_vol_watershed_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!vol_dims_ok(X, Y, Z) || (long long)X * Y * Z == 0) return 0;
  return ws_layout_of(ws_dims_make(X, Y, Z)).total;
}

int32_t unet_vol_watershed_begin(unet_ctx* ctx, const uint32_t* cost, const int32_t* markers, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t phase,
                                 int32_t done, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_begin: a dimension is negative or the volume has 2^31 voxels or more");
  if (!ws_phase_ok(phase)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_begin: phase %d is not HEIGHT, LABEL or SUM", phase);
  if (done < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_begin: done %d is negative", done);
  const ws_dims d = ws_dims_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!cost || !markers || !ws || !vol_aligned(cost, 4) || !vol_aligned(markers, 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_begin: null or misaligned buffer");
  const ws_layout L = ws_layout_of(d);
  if (ws_bytes < L.total || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_begin: workspace too small or not 16-byte aligned");
  if (vol_overlap(cost, (size_t)d.N * 4, ws, L.total) || vol_overlap(markers, (size_t)d.N * 4, ws, L.total) || (mask && vol_overlap(mask, (size_t)d.N, ws, L.total)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_begin: an input overlaps the workspace");
  hipStream_t s = as_stream(stream);
  uint8_t* base = static_cast<uint8_t*>(ws);
  u64 *A = reinterpret_cast<u64*>(base + L.A), *B = reinterpret_cast<u64*>(base + L.B);
  UNET_HIP(ctx, hipMemsetAsync(base + L.bmask, 0, (size_t)d.nb, s));
  UNET_HIP(ctx, hipMemsetAsync(base + L.F0, 1, (size_t)d.nb, s));       // sweep 0 reads F0: all-active
  hipLaunchKernelGGL(ws_seed_kernel, dim3(vol_blocks(d.N, WS_FLAT_CAP, WS_TPB)), dim3(WS_TPB), 0, s, cost, markers, mask, d, phase, (done & 1) ? B : A, A, B,
                     reinterpret_cast<uint32_t*>(base + L.H), base + L.bmask, reinterpret_cast<long long*>(base + L.part));
  UNET_CHECK_LAUNCH(ctx, "vol_watershed_begin"); return UNET_OK;
}

int32_t unet_vol_watershed_sweeps(unet_ctx* ctx, const uint32_t* cost, const int32_t* markers, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t first,
                                  int32_t n, int32_t phase, int32_t connectivity, int32_t skip, int64_t* changed, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: a dimension is negative or the volume has 2^31 voxels or more");
  if (!ws_phase_ok(phase)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: phase %d is not HEIGHT, LABEL or SUM", phase);
  if (connectivity < 1 || connectivity > 3) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: connectivity %d is not 1, 2 or 3", connectivity);
  if (first < 0 || n < 0 || (long long)first + n > 0x7FFFFFFFLL) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: first %d or n %d is negative (or their sum overflows)", first, n);
  if (skip != 0 && skip != 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: skip %d is not 0 or 1", skip);
  const ws_dims d = ws_dims_make(X, Y, Z);
  if (d.N == 0 || n == 0) return UNET_OK;
  if (!cost || !markers || !changed || !ws || !vol_aligned(cost, 4) || !vol_aligned(markers, 4) || !vol_aligned(changed, 8))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: null or misaligned buffer");
  const ws_layout L = ws_layout_of(d);
  if (ws_bytes < L.total || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: workspace too small or not 16-byte aligned");
  if (vol_overlap(cost, (size_t)d.N * 4, ws, L.total) || vol_overlap(markers, (size_t)d.N * 4, ws, L.total) || (mask && vol_overlap(mask, (size_t)d.N, ws, L.total)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: an input overlaps the workspace");
  const size_t cb = (size_t)n * 8;
  if (vol_overlap(changed + first, cb, ws, L.total) || vol_overlap(changed + first, cb, cost, (size_t)d.N * 4) || vol_overlap(changed + first, cb, markers, (size_t)d.N * 4) ||
      (mask && vol_overlap(changed + first, cb, mask, (size_t)d.N)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_sweeps: changed overlaps an input or the workspace");
  hipStream_t s = as_stream(stream);
  uint8_t* base = static_cast<uint8_t*>(ws);
  u64* K[2] = {reinterpret_cast<u64*>(base + L.A), reinterpret_cast<u64*>(base + L.B)};
  uint8_t* F[2] = {base + L.F0, base + L.F1};
  UNET_HIP(ctx, hipMemsetAsync(changed + first, 0, cb, s));
  const unsigned grid = (unsigned)(d.nb < GRID_CAP ? d.nb : GRID_CAP);
  for (int sw = first; sw < first + n; ++sw)
    hipLaunchKernelGGL(ws_sweep_kernel, dim3(grid), dim3(WS_TPB), 0, s, K[sw & 1], K[(sw + 1) & 1], cost, markers, mask, reinterpret_cast<const uint32_t*>(base + L.H), d, phase,
                       connectivity, skip, base + L.bmask, F[sw & 1], F[(sw + 1) & 1], reinterpret_cast<u64*>(changed) + sw);
  UNET_CHECK_LAUNCH(ctx, "vol_watershed_sweeps"); return UNET_OK;
}

int32_t unet_vol_watershed_end(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t phase, int32_t done, int32_t connectivity, int32_t* labels,
                               uint32_t* height, uint32_t* steps, uint64_t* distance, int64_t* counts, const void* ws, size_t ws_bytes, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: a dimension is negative or the volume has 2^31 voxels or more");
  if (!ws_phase_ok(phase)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: phase %d is not HEIGHT, LABEL or SUM", phase);
  if (connectivity < 1 || connectivity > 3) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: connectivity %d is not 1, 2 or 3", connectivity);
  if (done < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: done %d is negative", done);
  const bool want_l = phase != WS_HEIGHT, want_h = phase == WS_HEIGHT, want_s = phase == WS_LABEL, want_d = phase == WS_SUM;
  if ((labels != nullptr) != want_l || (steps != nullptr) != want_s || (distance != nullptr) != want_d || (want_h && !height) || (want_d && height))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: HEIGHT writes height; LABEL labels, steps and optionally height; SUM labels and distance; nothing else may be passed");
  if (!counts || !vol_aligned(counts, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: counts is null or misaligned");
  const ws_dims d = ws_dims_make(X, Y, Z);
  hipStream_t s = as_stream(stream);
  if (d.N == 0) { UNET_HIP(ctx, hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s)); return UNET_OK; }
  if (!ws || !vol_aligned(labels, 4) || !vol_aligned(height, 4) || !vol_aligned(steps, 4) || !vol_aligned(distance, 8)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: null or misaligned buffer");
  const ws_layout L = ws_layout_of(d);
  if (ws_bytes < L.total || !vol_aligned(ws, 16)) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: workspace too small or not 16-byte aligned");
  const void* outs[5] = {labels, height, steps, distance, counts};
  const size_t out_bytes[5] = {(size_t)d.N * 4, (size_t)d.N * 4, (size_t)d.N * 4, (size_t)d.N * 8, 32};
  for (int o = 0; o < 5; ++o) {
    if (!outs[o]) continue;
    if (vol_overlap(outs[o], out_bytes[o], ws, L.total) || (mask && vol_overlap(outs[o], out_bytes[o], mask, (size_t)d.N)))
      UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: an output overlaps the mask or the workspace");
    for (int p = o + 1; p < 5; ++p)
      if (outs[p] && vol_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) UNET_FAIL(ctx, UNET_E_ARG, "vol_watershed_end: two outputs overlap");
  }
  const uint8_t* base = static_cast<const uint8_t*>(ws);
  long long* part = reinterpret_cast<long long*>(const_cast<uint8_t*>(base) + L.part);
  const unsigned grid = vol_blocks(d.N, WS_FLAT_CAP, WS_TPB);          // the grid of _begin: its partial counts of invalid markers are summed with this launch's
  hipLaunchKernelGGL(ws_unpack_kernel, dim3(grid), dim3(WS_TPB), 0, s, reinterpret_cast<const u64*>(base + ((done & 1) ? L.B : L.A)),
                     reinterpret_cast<const uint32_t*>(base + L.H), mask, d, phase, connectivity, labels, height, steps, reinterpret_cast<u64*>(distance), part);
  hipLaunchKernelGGL(ws_counts_kernel, dim3(1), dim3(WS_TPB), 0, s, part, (int)grid, reinterpret_cast<long long*>(counts));
  UNET_CHECK_LAUNCH(ctx, "vol_watershed_end"); return UNET_OK;
}

int32_t unet_vol_depth_cost(unet_ctx* ctx, const double* d2, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, double d2max, double quantum, uint32_t* cost, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_depth_cost: a dimension is negative or the volume has 2^31 voxels or more");
  if (!(quantum > 0.0) || !(quantum < INFINITY) || !(d2max >= 0.0) || !(d2max < INFINITY)) UNET_FAIL(ctx, UNET_E_ARG, "vol_depth_cost: quantum must be positive and d2max >= 0, both finite");
  const long long N = (long long)X * Y * Z;
  if (N == 0) return UNET_OK;
  if (!d2 || !cost || !vol_aligned(d2, 8) || !vol_aligned(cost, 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_depth_cost: null or misaligned buffer");
  if (vol_overlap(cost, (size_t)N * 4, d2, (size_t)N * 8) || (mask && vol_overlap(cost, (size_t)N * 4, mask, (size_t)N)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_depth_cost: the output overlaps an input");
  hipLaunchKernelGGL(ws_depth_cost_kernel, dim3(vol_blocks(N, WS_FLAT_CAP, WS_TPB)), dim3(WS_TPB), 0, as_stream(stream), d2, mask, N, d2max, quantum, cost);
  UNET_CHECK_LAUNCH(ctx, "vol_depth_cost"); return UNET_OK;
}

}  // extern "C"

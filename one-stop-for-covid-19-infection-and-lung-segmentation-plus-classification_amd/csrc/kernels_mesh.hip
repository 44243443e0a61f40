// The surface of a mask, a label volume or a scalar volume as an indexed triangle mesh (bit-exact against tests/mesh_oracle.py).
// Marching tetrahedra on the Freudenthal split: the cube between lattice points p and p + (1, 1, 1) is cut into six tetrahedra, one per axis order; every tetrahedron edge
// runs from a lattice point q to q + d, d one of seven directions (edge types 0..6), so a vertex belongs to (q, type), its id is the rank of that pair, and nothing is welded.
// Launches (phase boundaries are kernel boundaries; no workgroup ever waits for another one inside a launch; no atomics at all):
//   mesh_count_kernel      one lane per lattice point, the samples of a chunk and its halo staged in LDS: the flag byte of the point (bit e: edge type e is crossed and both ends exist), the triangle count of the cell it
//                          starts (0..12), and the two sums of its chunk of CHUNK points.  A wave whose 64 cells are all inside or all outside writes zeros and moves on.
//   mesh_scan_kernel       one workgroup: chunk sums -> exclusive offsets in place, the two totals as int64
//   mesh_vertices_kernel   a chunk per workgroup: the popcounts of the flag bytes are scanned again in LDS; every crossed edge writes its vertex at its rank
//   mesh_triangles_kernel  a chunk of cells per workgroup: the counts are scanned again for the triangle offsets; the vertex offsets of the four rows of points the chunk's
//                          cells own edges in ((y, z), (y + 1, z), (y, z + 1), (y + 1, z + 1)) are rebuilt in LDS from the flag bytes; every non-empty cell writes its triangles
//   mesh_measure_kernel    per triangle: area and signed volume in float64 from the stored float32 vertices
// Compiled with -ffp-contract=off; the __d*_rn forms keep every float64 operation a rounded one either way.
#include "vol_trilinear.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int PER = 8;                                               // flag / count bytes per lane of a scan: one 8-byte load
#ifndef MESH_COUNT_LDS
#define MESH_COUNT_LDS 1                                              // 0: the measurement build `make mesh_loads` (overlapping loads on every row length)
#endif
constexpr int CHUNK = TPB * PER;                                     // lattice points per workgroup: 2048 (tests/test_gpu_mesh.py states it)

// the lattice: the volume [X, Y, Z] with `pad` layers of outside samples around it; lattice point (i, j, k) is voxel (i - pad, j - pad, k - pad)
struct ms_lat { int X, Y, Z, pad, PX, PY, PZ; long long PXY, NP, NPpad; };
struct ms_in { vol_voxels src; int kind, select; double iso, pad_value; };          // kind 0: uint8 mask, 1: int32 labels, 2: scalar volume

// tetrahedron n: corners v0 = 0, v1, v2, v3 = 7 as cube corners c = dx + 2 dy + 4 dz (axis orders xyz, xzy, yxz, yzx, zxy, zyx)
__constant__ uint8_t MS_V1[6] = {1, 1, 2, 2, 4, 4};
__constant__ uint8_t MS_V2[6] = {3, 5, 3, 6, 5, 6};
// a tetrahedron's six edges (lower corner, upper corner): the code of a vertex in MS_TABLE
__constant__ uint8_t MS_PAIR_LO[6] = {0, 0, 0, 1, 1, 2};
__constant__ uint8_t MS_PAIR_HI[6] = {1, 2, 3, 2, 3, 3};
// edge type of a direction d as cube-corner bits: (1,0,0) (0,1,0) (1,1,0) (0,0,1) (1,0,1) (0,1,1) (1,1,1) -> 0 1 3 2 4 5 6
__constant__ uint8_t MS_TYPE_OF[8] = {0, 0, 1, 3, 2, 4, 5, 6};
__constant__ uint8_t MS_DIR_OF[7] = {1, 2, 4, 3, 5, 6, 7};
// word[n][case] = number of triangles | code of vertex j << (4 + 3 j); vertices 0..2 are the first triangle, 3..5 the second.  Derived by the winding rule in
// tests/mesh_oracle.py (packed_table) and printed in DESIGN.md section 4z; tests/test_mesh_host.py compares this text with the derivation.
__constant__ uint32_t MS_TABLE[6][16] = {
    {0, 2177, 3585, 1847570, 5521, 2820738, 857602, 5665, 4769, 2430082, 2756226, 3729, 1323410, 4481, 1281, 0},
    {0, 1281, 4481, 2304530, 3729, 1905922, 2691714, 4769, 5665, 2885250, 1381762, 5521, 2240018, 3585, 2177, 0},
    {0, 1281, 4481, 2304530, 3729, 1905922, 2691714, 4769, 5665, 2885250, 1381762, 5521, 2240018, 3585, 2177, 0},
    {0, 2177, 3585, 1847570, 5521, 2820738, 857602, 5665, 4769, 2430082, 2756226, 3729, 1323410, 4481, 1281, 0},
    {0, 2177, 3585, 1847570, 5521, 2820738, 857602, 5665, 4769, 2430082, 2756226, 3729, 1323410, 4481, 1281, 0},
    {0, 1281, 4481, 2304530, 3729, 1905922, 2691714, 4769, 5665, 2885250, 1381762, 5521, 2240018, 3585, 2177, 0}};

__device__ __forceinline__ bool ms_voxel(const ms_lat& L, int i, int j, int k, long long* f) {
  const int x = i - L.pad, y = j - L.pad, z = k - L.pad;
  if ((unsigned)x >= (unsigned)L.X || (unsigned)y >= (unsigned)L.Y || (unsigned)z >= (unsigned)L.Z) return false;          // a virtual sample
  *f = x + (long long)L.X * (y + (long long)L.Y * z);
  return true;
}
__device__ __forceinline__ unsigned ms_inside(const ms_in& in, const ms_lat& L, int i, int j, int k) {
  long long f;
  if (!ms_voxel(L, i, j, k, &f)) return 0u;                           // pad_value <= iso: a virtual sample is outside
  if (in.kind == 0) return static_cast<const uint8_t*>(in.src.p)[f] != 0 ? 1u : 0u;
  if (in.kind == 1) { const int l = static_cast<const int32_t*>(in.src.p)[f]; return (in.select ? l == in.select : l != 0) ? 1u : 0u; }
  return vol_dec(in.src, f) > in.iso ? 1u : 0u;                        // (a NaN is outside)
}
__device__ __forceinline__ double ms_value(const ms_in& in, const ms_lat& L, int i, int j, int k) {
  long long f;
  return ms_voxel(L, i, j, k, &f) ? vol_dec(in.src, f) : in.pad_value;
}
__device__ __forceinline__ void ms_ijk(const ms_lat& L, long long q, int* i, int* j, int* k) {          // q < NP < 2^31: 32-bit divisions
  const unsigned uq = (unsigned)q, pxy = (unsigned)L.PXY, px = (unsigned)L.PX;
  const unsigned kk = uq / pxy, r = uq - kk * pxy, jj = r / px;
  *k = (int)kk; *j = (int)jj; *i = (int)(r - jj * px);
}
// the column of four samples at (i; j, j1; k, k1): bit 2 dy + 4 dz
__device__ __forceinline__ unsigned ms_column(const ms_in& in, const ms_lat& L, int i, int j, int j1, int k, int k1) {
  return ms_inside(in, L, i, j, k) | (ms_inside(in, L, i, j1, k) << 2) | (ms_inside(in, L, i, j, k1) << 4) | (ms_inside(in, L, i, j1, k1) << 6);
}
// which of +x, +y, +z neighbours exist (bits 0, 1, 2)
__device__ __forceinline__ unsigned ms_exist(const ms_lat& L, int i, int j, int k) { return (i + 1 < L.PX ? 1u : 0u) | (j + 1 < L.PY ? 2u : 0u) | (k + 1 < L.PZ ? 4u : 0u); }
__device__ __forceinline__ unsigned ms_case(unsigned c8, int n) {
  return (c8 & 1u) | (((c8 >> MS_V1[n]) & 1u) << 1) | (((c8 >> MS_V2[n]) & 1u) << 2) | (((c8 >> 7) & 1u) << 3);
}
__device__ __forceinline__ int ms_bytesum(unsigned w) { return (int)((w * 0x01010101u) >> 24); }

// exclusive prefix of c over the workgroup (the total in *total); s_w: TPB / 64 words, reusable from one call to the next
__device__ __forceinline__ int ms_block_scan(int c, int* s_w, int* total) {
  int inc = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if ((int)(threadIdx.x & 63) >= o) inc += t; }
  __syncthreads();                                                    // the previous call's sums have been read
  if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
  __syncthreads();
  int before = inc - c, tot = 0;
#pragma unroll
  for (int w = 0; w < TPB / 64; ++w) { const int t = s_w[w]; if (w < (int)(threadIdx.x >> 6)) before += t; tot += t; }
  *total = tot;
  return before;
}
__device__ __forceinline__ uint2 ms_load8(const uint8_t* p, long long base, long long npad) {          // base % 8 == 0, npad % 16 == 0: inside or outside as a whole
  return base < npad ? *reinterpret_cast<const uint2*>(p + base) : make_uint2(0u, 0u);
}
__device__ __forceinline__ unsigned ms_byte(const uint2& w, int b) { return ((b < 4 ? w.x : w.y) >> (8 * (b & 3))) & 0xFFu; }

// ---- count ----------------------------------------------------------------------------------------------------------------------------------------------------------------
// Samples staged in LDS where a row fits; otherwise overlapping loads served by L1 / L2: a lane reads the four samples of its own column and takes the next column from
// lane + 1 (only lane 63 loads it).
__global__ __launch_bounds__(TPB) void mesh_count_kernel(ms_in in, ms_lat L, uint8_t* __restrict__ flags, uint8_t* __restrict__ counts, int32_t* __restrict__ vsum,
                                                         int32_t* __restrict__ tsum) {
  __shared__ int s_w[TPB / 64];
  const long long c0 = (long long)blockIdx.x * CHUNK;
  const int lane = threadIdx.x & 63;
#if MESH_COUNT_LDS
  // The inside bytes of the two z planes' ranges [c0 + dz PXY, + CHUNK + PX + 1] are staged once per workgroup and the eight corners are read from LDS: 18 % faster than
  // overlapping loads on 512 x 512 x 301.  A corner index that runs past a row or plane end reads a sample of the next row: only where `ex` masks
  // the result.  Rows longer than CHUNK - 1 points do not fit and take the loads below.
  __shared__ uint8_t s_in[2][2 * CHUNK];
  const bool staged = L.PX + 1 <= CHUNK;                              // (uniform) the halo fits
  if (staged) {
    const int span = CHUNK + L.PX + 1;
    for (int r = 0; r < 2; ++r)
      for (int u = threadIdx.x; u < span; u += TPB) {
        const long long q = c0 + r * L.PXY + u;
        unsigned v = 0;
        if (q < L.NP) { int i, j, k; ms_ijk(L, q, &i, &j, &k); v = ms_inside(in, L, i, j, k); }
        s_in[r][u] = (uint8_t)v;
      }
    __syncthreads();
  }
#endif
  int nv = 0, nt = 0;
  for (int it = 0; it < PER; ++it) {                                  // (the trip count is the same for every lane)
    const long long q = c0 + it * TPB + threadIdx.x;
    const bool live = q < L.NP;
    int i = 0, j = 0, k = 0;
    unsigned col = 0;
    if (live) ms_ijk(L, q, &i, &j, &k);
#if MESH_COUNT_LDS
    if (staged) {
      const int u = it * TPB + threadIdx.x;
      if (live) col = s_in[0][u] | ((unsigned)s_in[0][u + L.PX] << 2) | ((unsigned)s_in[1][u] << 4) | ((unsigned)s_in[1][u + L.PX] << 6);
    } else
#endif
    if (live) col = ms_column(in, L, i, j, min(j + 1, L.PY - 1), k, min(k + 1, L.PZ - 1));
    unsigned nb = __shfl_down(col, 1, 64);                            // lane + 1 holds (i + 1, j, k) whenever that point exists and lane < 63
    if (live) {
      if (i + 1 >= L.PX) nb = col;                                    // no +x neighbour: nothing crosses, and the cell does not exist
#if MESH_COUNT_LDS
      else if (staged) {
        const int u = it * TPB + threadIdx.x + 1;
        nb = s_in[0][u] | ((unsigned)s_in[0][u + L.PX] << 2) | ((unsigned)s_in[1][u] << 4) | ((unsigned)s_in[1][u + L.PX] << 6);
      }
#endif
      else if (lane == 63) nb = ms_column(in, L, i + 1, j, min(j + 1, L.PY - 1), k, min(k + 1, L.PZ - 1));
    }
    const unsigned c8 = col | (nb << 1);                              // bit c = dx + 2 dy + 4 dz
    const bool mixed = live && c8 != 0u && c8 != 0xFFu;
    if (__ballot(mixed) == 0ull) {                                    // nearly every wave of a real volume
      if (live) { flags[q] = 0; counts[q] = 0; }
      continue;
    }
    unsigned fl = 0, cnt = 0;
    if (mixed) {
      const unsigned ex = ms_exist(L, i, j, k);
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        const unsigned d = MS_DIR_OF[e];
        if ((d & ~ex) == 0u && (((c8 >> d) ^ c8) & 1u)) fl |= 1u << e;
      }
      if (ex == 7u) {
#pragma unroll
        for (int n = 0; n < 6; ++n) cnt += MS_TABLE[n][ms_case(c8, n)] & 15u;
      }
    }
    if (live) { flags[q] = (uint8_t)fl; counts[q] = (uint8_t)cnt; }
    nv += __popc(fl); nt += (int)cnt;
  }
  int tv, tt;
  ms_block_scan(nv, s_w, &tv);
  ms_block_scan(nt, s_w, &tt);
  if (threadIdx.x == 0) { vsum[blockIdx.x] = tv; tsum[blockIdx.x] = tt; }
}

// one workgroup; blockIdx.x selects the array: chunk sums -> exclusive offsets in place (they are only used when the total is below 2^31), the total -> totals[blockIdx.x]
__global__ __launch_bounds__(1024) void mesh_scan_kernel(int32_t* __restrict__ vsum, int32_t* __restrict__ tsum, int nb, long long* __restrict__ totals) {
  __shared__ long long s_part[1024];
  int32_t* a = blockIdx.x == 0 ? vsum : tsum;
  const int per = (nb + 1023) / 1024;
  const int lo = (int)min((long long)nb, (long long)threadIdx.x * per), hi = (int)min((long long)nb, (long long)lo + per);
  long long s = 0;
  for (int i = lo; i < hi; ++i) s += a[i];
  s_part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int i = 0; i < 1024; ++i) { const long long t = s_part[i]; s_part[i] = run; run += t; }
    totals[blockIdx.x] = run;
  }
  __syncthreads();
  long long run = s_part[threadIdx.x];
  for (int i = lo; i < hi; ++i) { const int t = a[i]; a[i] = (int32_t)run; run += t; }
}

// ---- vertices -------------------------------------------------------------------------------------------------------------------------------------------------------------
struct ms_mat { double m[12]; };
__global__ __launch_bounds__(TPB) void mesh_vertices_kernel(ms_in in, ms_lat L, ms_mat M, const uint8_t* __restrict__ flags, const int32_t* __restrict__ vbase,
                                                            float* __restrict__ vertices, long long cap) {
  __shared__ int s_w[TPB / 64];
  const long long base = (long long)blockIdx.x * CHUNK + (long long)threadIdx.x * PER;
  const uint2 w = ms_load8(flags, base, L.NPpad);
  const int c = __popc(w.x & 0x7F7F7F7Fu) + __popc(w.y & 0x7F7F7F7Fu);
  int tot;
  long long at = (long long)vbase[blockIdx.x] + ms_block_scan(c, s_w, &tot);
  if (c == 0) return;
  for (int b = 0; b < PER; ++b) {
    const unsigned fl = ms_byte(w, b) & 0x7Fu;
    if (!fl) continue;
    const long long q = base + b;
    if (q >= L.NP) break;
    int i, j, k;
    ms_ijk(L, q, &i, &j, &k);
    double a = 0.0;
    if (in.kind == 2) a = ms_value(in, L, i, j, k);
    for (int e = 0; e < 7; ++e) {
      if (!((fl >> e) & 1u)) continue;
      if (at < cap) {
        const int d = MS_DIR_OF[e];
        const int dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
        double t = 0.5;
        if (in.kind == 2) {
          const double bv = ms_value(in, L, min(i + dx, L.PX - 1), min(j + dy, L.PY - 1), min(k + dz, L.PZ - 1));
          if (isfinite(a) && isfinite(bv)) t = __ddiv_rn(__dsub_rn(in.iso, a), __dsub_rn(bv, a));
        }
        const double cx = __dadd_rn((double)(i - L.pad), __dmul_rn(t, (double)dx));
        const double cy = __dadd_rn((double)(j - L.pad), __dmul_rn(t, (double)dy));
        const double cz = __dadd_rn((double)(k - L.pad), __dmul_rn(t, (double)dz));
#pragma unroll
        for (int r = 0; r < 3; ++r)
          vertices[3 * at + r] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(M.m[4 * r], cx), __dmul_rn(M.m[4 * r + 1], cy)), __dmul_rn(M.m[4 * r + 2], cz)), M.m[4 * r + 3]);
      }
      ++at;
    }
  }
}

// ---- triangles ------------------------------------------------------------------------------------------------------------------------------------------------------------
// The cells of chunk [c0, c0 + CHUNK) own edges at the points of four ranges [s_r, s_r + CHUNK], s_r = c0 + (r & 1) PX + (r >> 1) PX PY.  The vertex offset of every point
// of a range is rebuilt from the chunk base below s_r: two passes of CHUNK flag bytes from the start of that chunk (s_r + CHUNK lies below the end of the second pass);
// running on over a chunk boundary is right because vbase[c + 1] = vbase[c] + the sum of chunk c.
__global__ __launch_bounds__(TPB) void mesh_triangles_kernel(ms_in in, ms_lat L, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ counts,
                                                             const int32_t* __restrict__ vbase, const int32_t* __restrict__ tbase, int32_t* __restrict__ triangles,
                                                             int32_t* __restrict__ groups, long long cap) {
  __shared__ int s_w[TPB / 64];
  __shared__ int s_off[4][CHUNK + 1];
  const long long c0 = (long long)blockIdx.x * CHUNK;
  const long long base = c0 + (long long)threadIdx.x * PER;
  const uint2 cw = ms_load8(counts, base, L.NPpad);
  const int c = ms_bytesum(cw.x) + ms_bytesum(cw.y);
  int tot;
  long long at = (long long)tbase[blockIdx.x] + ms_block_scan(c, s_w, &tot);
  if (tot == 0) return;                                               // (the same for every lane) nearly every chunk of a real volume
  for (int r = 0; r < 4; ++r) {
    const long long s_r = c0 + (r & 1) * (long long)L.PX + (r >> 1) * L.PXY;
    if (s_r >= L.NP) continue;                                        // (uniform) no cell of this chunk has a point there
    const long long ci = s_r / CHUNK;
    long long carry = vbase[ci];
    for (int pass = 0; pass < 2; ++pass) {
      const long long pb = (ci + pass) * CHUNK + (long long)threadIdx.x * PER;
      const uint2 w = ms_load8(flags, pb, L.NPpad);
      int ptot;
      long long off = carry + ms_block_scan(__popc(w.x & 0x7F7F7F7Fu) + __popc(w.y & 0x7F7F7F7Fu), s_w, &ptot);
#pragma unroll
      for (int b = 0; b < PER; ++b) {
        const long long idx = pb + b - s_r;
        if (idx >= 0 && idx <= CHUNK) s_off[r][idx] = (int)off;
        off += __popc(ms_byte(w, b) & 0x7Fu);
      }
      carry += ptot;
    }
  }
  __syncthreads();
  if (c == 0) return;
  for (int b = 0; b < PER; ++b) {
    if (!ms_byte(cw, b)) continue;
    const long long q = base + b;
    if (q >= L.NP) break;
    int i, j, k;
    ms_ijk(L, q, &i, &j, &k);
    if (ms_exist(L, i, j, k) != 7u) continue;                         // (mesh_count_kernel never counts such a cell)
    const unsigned c8 = ms_column(in, L, i, j, j + 1, k, k + 1) | (ms_column(in, L, i + 1, j, j + 1, k, k + 1) << 1);
    const int local = (int)(q - c0);
    for (int n = 0; n < 6; ++n) {
      const unsigned cs = ms_case(c8, n);
      const unsigned word = MS_TABLE[n][cs];
      const int ntri = (int)(word & 15u);
      const unsigned corner[4] = {0u, MS_V1[n], MS_V2[n], 7u};
      for (int t = 0; t < ntri; ++t, ++at) {
        if (at >= cap) continue;
        int id[3];
        unsigned first_in = 0;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const unsigned code = (word >> (4 + 3 * (3 * t + v))) & 7u;
          const unsigned klo = MS_PAIR_LO[code], khi = MS_PAIR_HI[code];
          const unsigned lo = corner[klo], hi = corner[khi];
          const unsigned e = MS_TYPE_OF[hi ^ lo];                     // lo's bits are a subset of hi's: the direction is their difference
          const long long qo = q + (lo & 1u) + ((lo >> 1) & 1u) * (long long)L.PX + ((lo >> 2) & 1u) * L.PXY;
          const unsigned fl = flags[qo];
          id[v] = s_off[lo >> 1][local + (int)(lo & 1u)] + __popc(fl & ((1u << e) - 1u));
          if (v == 0) first_in = ((cs >> klo) & 1u) ? lo : hi;
        }
        triangles[3 * at] = id[0]; triangles[3 * at + 1] = id[1]; triangles[3 * at + 2] = id[2];
        if (groups) {
          int g = 1;
          if (in.kind == 1) {
            long long f = 0;
            g = ms_voxel(L, i + (int)(first_in & 1u), j + (int)((first_in >> 1) & 1u), k + (int)((first_in >> 2) & 1u), &f) ? static_cast<const int32_t*>(in.src.p)[f] : 0;
          }
          groups[at] = g;
        }
      }
    }
  }
}

// ---- measure --------------------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ms_det2(double a, double b, double c, double d) { return __dsub_rn(__dmul_rn(a, b), __dmul_rn(c, d)); }          // fl(fl(a b) - fl(c d))
__global__ __launch_bounds__(TPB) void mesh_measure_kernel(const float* __restrict__ vertices, long long nv, const int32_t* __restrict__ triangles, long long nt,
                                                           double* __restrict__ area, double* __restrict__ volume) {
  const long long t = (long long)blockIdx.x * TPB + threadIdx.x;
  if (t >= nt) return;
  double p[3][3];
  bool ok = true;
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const long long id = triangles[3 * t + v];
    const bool in = id >= 0 && id < nv;                               // an index outside the vertex array is never an address: the triangle measures NaN
    ok = ok && in;
#pragma unroll
    for (int r = 0; r < 3; ++r) p[v][r] = in ? (double)vertices[3 * id + r] : 0.0;
  }
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  double u[3], w[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) { u[r] = __dsub_rn(p[1][r], p[0][r]); w[r] = __dsub_rn(p[2][r], p[0][r]); }
  const double cx = ms_det2(u[1], w[2], u[2], w[1]), cy = ms_det2(u[2], w[0], u[0], w[2]), cz = ms_det2(u[0], w[1], u[1], w[0]);
  if (area) area[t] = ok ? __dmul_rn(0.5, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz)))) : nan;
  const double nx = ms_det2(p[1][1], p[2][2], p[1][2], p[2][1]), ny = ms_det2(p[1][2], p[2][0], p[1][0], p[2][2]), nz = ms_det2(p[1][0], p[2][1], p[1][1], p[2][0]);
  if (volume) volume[t] = ok ? __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(p[0][0], nx), __dmul_rn(p[0][1], ny)), __dmul_rn(p[0][2], nz)), 6.0) : nan;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------------------------
// the lattice of a volume, or false: a negative extent, or 2^31 lattice points or more (each factor is below 2^31 + 2, so the products are tested one at a time)
inline bool ms_lattice(int X, int Y, int Z, int closed, ms_lat* L) {
  if (X < 0 || Y < 0 || Z < 0) return false;
  const int pad = closed ? 1 : 0;
  const long long PX = (long long)X + 2 * pad, PY = (long long)Y + 2 * pad, PZ = (long long)Z + 2 * pad;
  const bool none = X == 0 || Y == 0 || Z == 0;
  if (!none && (PX * PY >= 0x80000000LL || PX * PY * PZ >= 0x80000000LL)) return false;
  L->X = X; L->Y = Y; L->Z = Z; L->pad = pad;
  L->PX = none ? 0 : (int)PX; L->PY = none ? 0 : (int)PY; L->PZ = none ? 0 : (int)PZ;
  L->PXY = none ? 0 : PX * PY; L->NP = none ? 0 : PX * PY * PZ; L->NPpad = (L->NP + 15) / 16 * 16;
  return true;
}
inline bool ms_has_cells(const ms_lat& L) { return L.NP > 0 && L.PX >= 2 && L.PY >= 2 && L.PZ >= 2; }          // an unpadded extent of 1: no cells, an empty mesh
inline long long ms_chunks(const ms_lat& L) { return (L.NP + CHUNK - 1) / CHUNK; }
inline size_t ms_base_bytes(const ms_lat& L) { return (size_t)(((ms_chunks(L) + 1) * sizeof(int32_t) + 15) / 16 * 16); }
inline size_t ms_ws_bytes(const ms_lat& L) { return ms_has_cells(L) ? 2 * (size_t)L.NPpad + 2 * ms_base_bytes(L) : 0; }

struct ms_args { ms_in in; ms_lat L; uint8_t* flags; uint8_t* counts; int32_t* vbase; int32_t* tbase; };
// the checks count and emit share; 0: refused (the message is set), 1: go on, 2: nothing to do (no voxels, or no cells)
int ms_check(unet_ctx* ctx, const char* what, const void* src, int kind, int dtype, int X, int Y, int Z, int scaled, double slope, double inter, double iso, int select,
             int closed, double pad_value, void* ws, size_t ws_bytes, ms_args* a) {
  if (!ms_lattice(X, Y, Z, closed, &a->L)) { if (ctx) { char b[256]; snprintf(b, sizeof(b), "%s: %d x %d x %d is negative or its lattice has 2^31 points or more", what, X, Y, Z); ctx->err = b; } return 0; }
  const char* bad = nullptr;
  if (kind < 0 || kind > 2) bad = "kind is 0 (uint8 mask), 1 (int32 labels) or 2 (scalar volume)";
  else if (kind == 0 && dtype != 2) bad = "a mask is uint8 (datatype code 2)";
  else if (kind == 1 && dtype != 8) bad = "a label volume is int32 (datatype code 8)";
  else if (vol_itemsize(dtype) == 0) bad = "unknown datatype code";
  else if (!std::isfinite(iso) || !std::isfinite(pad_value)) bad = "iso and pad_value are finite";
  else if (pad_value > iso) bad = "pad_value > iso: the virtual layer must be outside";
  else if (select < 0) bad = "select < 0";
  else if (scaled && (std::isnan(slope) || std::isnan(inter))) bad = "slope and inter are numbers";
  if (bad) { if (ctx) { char b[256]; snprintf(b, sizeof(b), "%s: %s", what, bad); ctx->err = b; } return 0; }
  if (!ms_has_cells(a->L)) return 2;
  if (!src || (reinterpret_cast<uintptr_t>(src) % (uintptr_t)vol_itemsize(dtype)) != 0 || !ws || (reinterpret_cast<uintptr_t>(ws) % 16) != 0 || ws_bytes < ms_ws_bytes(a->L)) {
    if (ctx) { char b[256]; snprintf(b, sizeof(b), "%s: null or misaligned buffer (the volume to its element size, the workspace to 16 bytes), or a workspace below unet_vol_mesh_ws_bytes", what); ctx->err = b; }
    return 0;
  }
  a->in.src = {src, dtype, scaled ? 1 : 0, slope, inter};
  a->in.kind = kind; a->in.select = select; a->in.iso = iso; a->in.pad_value = pad_value;
  a->flags = static_cast<uint8_t*>(ws);
  a->counts = a->flags + a->L.NPpad;
  a->vbase = reinterpret_cast<int32_t*>(a->counts + a->L.NPpad);
  a->tbase = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(a->vbase) + ms_base_bytes(a->L));
  return 1;
}
}  // namespace

extern "C" {

size_t unet_vol_mesh_ws_bytes(int32_t X, int32_t Y, int32_t Z, int32_t closed) {
  ms_lat L;
  return ms_lattice(X, Y, Z, closed, &L) ? ms_ws_bytes(L) : 0;
}

int32_t unet_vol_mesh_count(unet_ctx* ctx, const void* src, int32_t kind, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                            double iso, int32_t select, int32_t closed, double pad_value, void* ws, size_t ws_bytes, int64_t* totals, void* stream) {
  if (!ctx || !totals || (reinterpret_cast<uintptr_t>(totals) % 8) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_mesh_count: null context, or totals null or not 8-byte aligned");
  ms_args a;
  const int go = ms_check(ctx, "vol_mesh_count", src, kind, dtype, X, Y, Z, scaled, slope, inter, iso, select, closed, pad_value, ws, ws_bytes, &a);
  if (go == 0) return UNET_E_ARG;
  hipStream_t s = as_stream(stream);
  if (go == 2) { UNET_HIP(ctx, hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s)); return UNET_OK; }
  const int nb = (int)ms_chunks(a.L);
  if (a.L.NPpad > a.L.NP) {                                           // the scans read whole 8-byte words
    UNET_HIP(ctx, hipMemsetAsync(a.flags + a.L.NP, 0, (size_t)(a.L.NPpad - a.L.NP), s));
    UNET_HIP(ctx, hipMemsetAsync(a.counts + a.L.NP, 0, (size_t)(a.L.NPpad - a.L.NP), s));
  }
  hipLaunchKernelGGL(mesh_count_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, a.in, a.L, a.flags, a.counts, a.vbase, a.tbase);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(2), dim3(1024), 0, s, a.vbase, a.tbase, nb, reinterpret_cast<long long*>(totals));
  UNET_CHECK_LAUNCH(ctx, "vol_mesh_count"); return UNET_OK;
}

int32_t unet_vol_mesh_emit(unet_ctx* ctx, const void* src, int32_t kind, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                           double iso, int32_t select, int32_t closed, double pad_value, const double* M, const void* ws, size_t ws_bytes, float* vertices,
                           int64_t capacity_v, int32_t* triangles, int32_t* groups, int64_t capacity_t, void* stream) {
  if (!ctx || !M) UNET_FAIL(ctx, UNET_E_ARG, "vol_mesh_emit: null context or matrix");
  ms_mat mat;
  for (int i = 0; i < 12; ++i) {
    if (!std::isfinite(M[i])) UNET_FAIL(ctx, UNET_E_ARG, "vol_mesh_emit: matrix entry %d is not finite", i);
    mat.m[i] = M[i];
  }
  if (capacity_v < 0 || capacity_t < 0 || capacity_v >= 0x80000000LL || capacity_t >= 0x80000000LL)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_mesh_emit: a capacity is negative or 2^31 or more");
  if ((capacity_v > 0 && !vertices) || (capacity_t > 0 && !triangles) || (reinterpret_cast<uintptr_t>(vertices) % 4) != 0 || (reinterpret_cast<uintptr_t>(triangles) % 4) != 0 ||
      (reinterpret_cast<uintptr_t>(groups) % 4) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_mesh_emit: null or misaligned output (4 bytes)");
  ms_args a;
  const int go = ms_check(ctx, "vol_mesh_emit", src, kind, dtype, X, Y, Z, scaled, slope, inter, iso, select, closed, pad_value, const_cast<void*>(ws), ws_bytes, &a);
  if (go == 0) return UNET_E_ARG;
  if (go == 2) return UNET_OK;
  hipStream_t s = as_stream(stream);
  const int nb = (int)ms_chunks(a.L);
  if (capacity_v > 0) hipLaunchKernelGGL(mesh_vertices_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, a.in, a.L, mat, a.flags, a.vbase, vertices, (long long)capacity_v);
  if (capacity_t > 0)
    hipLaunchKernelGGL(mesh_triangles_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, a.in, a.L, a.flags, a.counts, a.vbase, a.tbase, triangles, groups, (long long)capacity_t);
  UNET_CHECK_LAUNCH(ctx, "vol_mesh_emit"); return UNET_OK;
}

int32_t unet_vol_mesh_measure(unet_ctx* ctx, const float* vertices, int64_t nv, const int32_t* triangles, int64_t nt, double* area, double* signed_volume, void* stream) {
  if (!ctx || nv < 0 || nt < 0 || nv >= 0x80000000LL || nt >= 0x80000000LL) UNET_FAIL(ctx, UNET_E_ARG, "vol_mesh_measure: null context, or a count that is negative or 2^31 or more");
  if (nt == 0) return UNET_OK;
  if (!triangles || (nv > 0 && !vertices) || (reinterpret_cast<uintptr_t>(vertices) % 4) != 0 || (reinterpret_cast<uintptr_t>(triangles) % 4) != 0 ||
      (reinterpret_cast<uintptr_t>(area) % 8) != 0 || (reinterpret_cast<uintptr_t>(signed_volume) % 8) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_mesh_measure: null or misaligned buffer (vertices and triangles 4 bytes, area and signed_volume 8)");
  hipLaunchKernelGGL(mesh_measure_kernel, dim3((unsigned)((nt + TPB - 1) / TPB)), dim3(TPB), 0, as_stream(stream), vertices, (long long)nv, triangles, (long long)nt, area,
                     signed_volume);
  UNET_CHECK_LAUNCH(ctx, "vol_mesh_measure"); return UNET_OK;
}

}  // extern "C"

// Connected components of a mask volume on the device: labels, per-component statistics, filtering by a keep table.
//   skimage.measure.label(mask != 0, connectivity=c) / scipy.ndimage.label(mask, generate_binary_structure(3, c))          unet_vol_label
//   scipy.ndimage.label with that structure's z = -1, +1 planes cleared: components inside every axial slice                                          unet_vol_label_planar
//   skimage.measure.regionprops' area / bbox / centroid sums, as exact integers                                              unet_vol_component_stats
//   skimage.morphology.remove_small_objects, "keep the k largest" (the keep table is the caller's)                          unet_vol_filter_components
// The volume is [X, Y, Z] in Fortran order (f = x + X (y + Y z), what unet_vol_unslice writes); a component's number is the rank of the smallest C-order
// index k = (x Y + y) Z + z among its voxels, so the union-find below runs on C-order KEYS: labels[f] holds the key of the voxel's parent, a smaller key
// always wins a union, and a set's root is its first voxel in scikit-image's scan order.
// Launches (phase boundaries are kernel boundaries; no workgroup ever waits for another one inside a launch):
//   cc_local_kernel    union-find in LDS over a 64 x 8 x 8 brick; every voxel leaves with the key of its brick-local root (-1: background)
//   cc_merge_kernel    the voxels on the low faces of every brick: lock-free union (atomicMin on a root's parent word) with their neighbours in other bricks
//   cc_flatten_kernel  every voxel -> the key of its root; a root raises its flag in a key-indexed byte array
//   cc_count / cc_scan / cc_number   prefix sum over the flags: the root with the r-th smallest key gets number r, left in its own word as -(r + 1)
//   cc_final_kernel    every voxel takes its root's number; background -> 0
// Everything is integer arithmetic: the result is the same on every run.
#include "common.h"
#include "vol_common.h"

#include <climits>

namespace {
constexpr int TPB = 256;
constexpr int BX = 64, BY = 8, BZ = 8, BRICK = BX * BY * BZ;          // brick: 16 voxels along x per lane, 4 lanes per row, 64 rows
constexpr int CHUNK = TPB * 64;                                      // flag bytes per workgroup of the prefix sum (64 contiguous bytes per lane)

struct cc_dims { int X, Y, Z, YZ; long long XY, N; };
__device__ __forceinline__ long long cc_f(const cc_dims& d, int x, int y, int z) { return x + (long long)d.X * (y + (long long)d.Y * z); }
__device__ __forceinline__ int cc_key(const cc_dims& d, int x, int y, int z) { return (x * d.Y + y) * d.Z + z; }
__device__ __forceinline__ long long cc_key_to_f(const cc_dims& d, int k) {
  const int x = k / d.YZ, r = k - x * d.YZ;
  const int y = r / d.Z, z = r - y * d.Z;
  return cc_f(d, x, y, z);
}
__device__ __forceinline__ void cc_f_to_xyz(const cc_dims& d, long long f, int* x, int* y, int* z) {
  const int zz = (int)(f / d.XY);
  const int r = (int)(f - (long long)zz * d.XY);
  *z = zz; *y = r / d.X; *x = r - (*y) * d.X;
}
// neighbour offset (dx, dy, dz) belongs to connectivity c when it moves along at most c axes
__device__ __forceinline__ bool cc_conn(int dx, int dy, int dz, int c) { return (dx != 0) + (dy != 0) + (dz != 0) <= c; }
// the planar predicate (unet_vol_label_planar): the same rule inside one axial slice -- c = 1, 2: 4, 8 neighbours; nothing joins two slices
__device__ __forceinline__ bool cc_conn_planar(int dx, int dy, int dz, int c) { return dz == 0 && (dx != 0) + (dy != 0) <= c; }
__device__ __forceinline__ bool cc_joined(int dx, int dy, int dz, int c, int planar) { return planar ? cc_conn_planar(dx, dy, dz, c) : cc_conn(dx, dy, dz, c); }

// ---- (a) brick-local union-find in LDS -------------------------------------------------------------------------------------------------------
// local index l = (lx * 8 + ly) * 8 + lz: the same order as the global key inside a brick, so the smallest l of a set is its smallest key.
// sidx pads one word per 1024: the four lanes of a row sit 1024 words apart and would share a bank.
__device__ __forceinline__ int sidx(int l) { return l + (l >> 10); }
__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(int* P, int a) {
  int p = lds_load(&P[sidx(a)]);
  while (p != a) {
    const int g = lds_load(&P[sidx(p)]);
    if (g != p) atomicMin(&P[sidx(a)], g);                            // halving: a parent only ever decreases and stays inside the set
    a = p; p = g;
  }
  return a;
}
__device__ __forceinline__ void lds_union(int* P, int a, int b) {
  while (true) {
    a = lds_find(P, a); b = lds_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&P[sidx(a)], b);                        // a failed attempt means another lane linked a first: carry its link on
    if (old == a) return;
    a = old;
  }
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void cc_local_kernel(const uint8_t* __restrict__ mask, cc_dims d, int conn, int planar, int invert, int nbx, int nby, int32_t* __restrict__ labels) {
  __shared__ int P[BRICK + 4];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
  const int seg = tid & 3, ly = (tid >> 2) & 7, lz = tid >> 5;
  const int gx0 = bx * BX + seg * 16, gy = by * BY + ly, gz = bz * BZ + lz;
  const bool row_in = gy < d.Y && gz < d.Z;
  const long long f0 = cc_f(d, gx0, gy, gz);
  unsigned fg = 0;                                                    // bit i: voxel gx0 + i is foreground
  if (VEC) {
    uint4 w = make_uint4(0, 0, 0, 0);
    if (row_in && gx0 < d.X) w = *reinterpret_cast<const uint4*>(mask + f0);          // X % 16 == 0: a 16-voxel segment is inside or outside as a whole
    const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) fg |= ((ws[i >> 2] >> (8 * (i & 3))) & 0xFFu) ? (1u << i) : 0u;
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) fg |= (row_in && gx0 + i < d.X && mask[f0 + i]) ? (1u << i) : 0u;
  }
  if (invert) {                                                       // the complement (unet_vol_fill_holes): only the voxels inside the volume turn
    const int in = row_in ? min(max(d.X - gx0, 0), 16) : 0;
    fg = ~fg & ((1u << in) - 1u);
  }
  const int l0 = ((seg * 16) * BY + ly) * BZ + lz;                    // lx = seg * 16 + i -> l = l0 + 64 i
#pragma unroll
  for (int i = 0; i < 16; ++i) P[sidx(l0 + 64 * i)] = ((fg >> i) & 1u) ? l0 + 64 * i : -1;
  __syncthreads();
  for (int i = 0; i < 16; ++i) {
    if (!((fg >> i) & 1u)) continue;
    const int lx = seg * 16 + i, l = l0 + 64 * i;
    for (int o = 14; o < 27; ++o) {                                  // the 13 offsets after (0, 0, 0) in (dx, dy, dz) order: each pair once
      const int dx = o / 9 - 1, dy = (o / 3) % 3 - 1, dz = o % 3 - 1;
      if (!cc_joined(dx, dy, dz, conn, planar)) continue;
      const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
      if (nx >= BX || ny < 0 || ny >= BY || nz < 0 || nz >= BZ) continue;
      const int nl = (nx * BY + ny) * BZ + nz;
      if (lds_load(&P[sidx(nl)]) < 0) continue;
      lds_union(P, l, nl);
    }
  }
  __syncthreads();
  int out[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    out[i] = -1;
    if ((fg >> i) & 1u) {
      const int r = lds_find(P, l0 + 64 * i);
      out[i] = cc_key(d, bx * BX + (r >> 6), by * BY + ((r >> 3) & 7), bz * BZ + (r & 7));
    }
  }
  if (VEC) {
    if (row_in && gx0 < d.X) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<int4*>(labels + f0 + 4 * j) = make_int4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (row_in && gx0 + i < d.X) labels[f0 + i] = out[i];
  }
}

// ---- (b) merge across brick faces, edges and corners -------------------------------------------------------------------------------------------
// Parent words are read at agent scope: another XCD's L2 may hold an older line.  An older value is an older ancestor of the same set, never a wrong one.
__device__ __forceinline__ int g_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int32_t* labels, const cc_dims& d, int k) {
  while (true) {
    const int p = g_load(labels + cc_key_to_f(d, k));
    if (p == k) return k;
    k = p;
  }
}
__device__ __forceinline__ void g_union(int32_t* labels, const cc_dims& d, int a, int b) {
  while (true) {
    a = g_find(labels, d, a); b = g_find(labels, d, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(labels + cc_key_to_f(d, a), b);         // device scope; every failure means another thread linked a: progress
    if (old == a) return;
    a = old;
  }
}
// one thread per voxel of the planes x = 64 i, y = 8 j, z = 8 k (i, j, k >= 1): its nine neighbours one step DOWN that axis.  Two adjacent voxels of
// different bricks differ in the brick coordinate of at least one axis; there the higher one lies on such a plane and the lower one is among its nine.
__global__ __launch_bounds__(TPB) void cc_merge_kernel(int32_t* labels, cc_dims d, int conn, int planar, long long PX, long long PY, long long PZ) {
  const long long total = PX + PY + PZ;
  for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
    int axis, x, y, z;
    if (i < PX) { axis = 0; z = (int)(i % d.Z); const long long r = i / d.Z; y = (int)(r % d.Y); x = ((int)(r / d.Y) + 1) * BX; }
    else if (i < PX + PY) { const long long j = i - PX; axis = 1; x = (int)(j % d.X); const long long r = j / d.X; z = (int)(r % d.Z); y = ((int)(r / d.Z) + 1) * BY; }
    else { const long long j = i - PX - PY; axis = 2; x = (int)(j % d.X); const long long r = j / d.X; y = (int)(r % d.Y); z = ((int)(r / d.Y) + 1) * BZ; }
    const int a = g_load(labels + cc_f(d, x, y, z));
    if (a < 0) continue;
    for (int u = -1; u <= 1; ++u)
      for (int v = -1; v <= 1; ++v) {
        const int dx = axis == 0 ? -1 : u, dy = axis == 1 ? -1 : (axis == 0 ? u : v), dz = axis == 2 ? -1 : v;
        if (!cc_joined(dx, dy, dz, conn, planar)) continue;
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        if (nx < 0 || nx >= d.X || ny < 0 || ny >= d.Y || nz < 0 || nz >= d.Z) continue;
        const int bk = g_load(labels + cc_f(d, nx, ny, nz));
        if (bk < 0) continue;
        g_union(labels, d, a, bk);
      }
  }
}

// ---- (c) flatten: four voxels (16 bytes of labels) per lane ---------------------------------------------------------------------------------------
// Nothing links sets any more.  A lane overwrites its own words with their roots while others still walk through them: they read the old parent or
// the root, both ancestors; a word that is not a root at the start of this launch never holds its own key.
__global__ __launch_bounds__(TPB) void cc_flatten_kernel(int32_t* labels, cc_dims d, uint8_t* __restrict__ flags) {
  const long long quads = (d.N + 3) / 4;
  for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < quads; q += (long long)gridDim.x * TPB) {
    const long long f0 = 4 * q;
    const bool full = f0 + 3 < d.N;
    int v[4] = {-1, -1, -1, -1};
    if (full) { const int4 w = *reinterpret_cast<const int4*>(labels + f0); v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w; }
    else for (int i = 0; f0 + i < d.N; ++i) v[i] = labels[f0 + i];
    int x, y, z;
    cc_f_to_xyz(d, f0, &x, &y, &z);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (v[i] >= 0) {
        const int r = g_find(labels, d, v[i]);
        v[i] = r;
        if (r == cc_key(d, x, y, z)) flags[r] = 1;
      }
      if (++x == d.X) { x = 0; if (++y == d.Y) { y = 0; ++z; } }
    }
    if (full) *reinterpret_cast<int4*>(labels + f0) = make_int4(v[0], v[1], v[2], v[3]);
    else for (int i = 0; f0 + i < d.N; ++i) labels[f0 + i] = v[i];
  }
}

// ---- (d) number the roots: prefix sum over the key-indexed flags (bytes 0 / 1; the array is padded with zeros to a multiple of 16) ------------------
__device__ __forceinline__ int bytesum(unsigned w) { return (int)((w * 0x01010101u) >> 24); }
__device__ __forceinline__ int lane_flags(const uint8_t* flags, long long base, long long npad, uint4* w) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w[j] = make_uint4(0, 0, 0, 0);
    if (base + 16 * j < npad) w[j] = *reinterpret_cast<const uint4*>(flags + base + 16 * j);
    c += bytesum(w[j].x) + bytesum(w[j].y) + bytesum(w[j].z) + bytesum(w[j].w);
  }
  return c;
}
__global__ __launch_bounds__(TPB) void cc_count_kernel(const uint8_t* __restrict__ flags, long long npad, int32_t* __restrict__ bsum) {
  __shared__ int s_w[TPB / 64];
  uint4 w[4];
  const int c = lane_flags(flags, (long long)blockIdx.x * CHUNK + threadIdx.x * 64, npad, w);
  const int t = vol_block_sum<int, TPB>(c, s_w);
  if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}
// one workgroup: chunk sums -> exclusive offsets in place, the total -> n_out
__global__ __launch_bounds__(1024) void cc_scan_kernel(int32_t* __restrict__ bsum, int nb, int32_t* __restrict__ n_out) {
  __shared__ int s_part[1024];
  const int per = (nb + 1023) / 1024;
  const int lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += bsum[i];
  s_part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < 1024; ++i) { const int t = s_part[i]; s_part[i] = run; run += t; }
    *n_out = run;
  }
  __syncthreads();
  int run = s_part[threadIdx.x];
  for (int i = lo; i < hi; ++i) { const int t = bsum[i]; bsum[i] = run; run += t; }
}
// the root with key k and rank r (1-based, by key) leaves -(r + 1) in its own word: negative, and not the background's -1
__global__ __launch_bounds__(TPB) void cc_number_kernel(const uint8_t* __restrict__ flags, long long npad, const int32_t* __restrict__ bsum, cc_dims d,
                                                       int32_t* __restrict__ labels) {
  __shared__ int s_w[TPB / 64];
  uint4 w[4];
  const long long base = (long long)blockIdx.x * CHUNK + threadIdx.x * 64;
  const int c = lane_flags(flags, base, npad, w);
  int inc = c;                                                       // inclusive scan over the wave, then over the four waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if ((int)(threadIdx.x & 63) >= o) inc += t; }
  if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
  __syncthreads();
  int before = bsum[blockIdx.x] + inc - c;
  for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) before += s_w[k];
  if (c == 0) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned ws[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((ws[i >> 2] >> (8 * (i & 3))) & 0xFFu) {
        ++before;
        labels[cc_key_to_f(d, (int)(base + 16 * j + i))] = -(before + 1);
      }
  }
}

// ---- (e) final labels ---------------------------------------------------------------------------------------------------------------------------
// A root's word holds -(r + 1) until its own lane has turned it into r; a reader of a root word takes either form.
__global__ __launch_bounds__(TPB) void cc_final_kernel(int32_t* labels, cc_dims d) {
  const long long quads = (d.N + 3) / 4;
  for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < quads; q += (long long)gridDim.x * TPB) {
    const long long f0 = 4 * q;
    const bool full = f0 + 3 < d.N;
    int v[4] = {-1, -1, -1, -1};
    if (full) { const int4 w = *reinterpret_cast<const int4*>(labels + f0); v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w; }
    else for (int i = 0; f0 + i < d.N; ++i) v[i] = labels[f0 + i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (v[i] == -1) v[i] = 0;
      else if (v[i] < -1) v[i] = -v[i] - 1;
      else { const int r = g_load(labels + cc_key_to_f(d, v[i])); v[i] = r < 0 ? -r - 1 : r; }
    }
    if (full) *reinterpret_cast<int4*>(labels + f0) = make_int4(v[0], v[1], v[2], v[3]);
    else for (int i = 0; f0 + i < d.N; ++i) labels[f0 + i] = v[i];
  }
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------------------------
struct comp_stat { long long count, sx, sy, sz; int x0, x1, y0, y1, z0, z1, pad0, pad1; };          // unet_hip.h: 64 bytes per component
static_assert(sizeof(comp_stat) == 64, "component record is 64 bytes");
struct comp_acc { int label; int cnt; long long sx, sy, sz; int x0, x1, y0, y1, z0, z1; };
__device__ __forceinline__ void stat_emit(comp_stat* st, const comp_acc& a) {
  comp_stat* s = st + (a.label - 1);
  atomicAdd(reinterpret_cast<unsigned long long*>(&s->count), (unsigned long long)a.cnt);
  atomicAdd(reinterpret_cast<unsigned long long*>(&s->sx), (unsigned long long)a.sx);
  atomicAdd(reinterpret_cast<unsigned long long*>(&s->sy), (unsigned long long)a.sy);
  atomicAdd(reinterpret_cast<unsigned long long*>(&s->sz), (unsigned long long)a.sz);
  atomicMin(&s->x0, a.x0); atomicMax(&s->x1, a.x1);
  atomicMin(&s->y0, a.y0); atomicMax(&s->y1, a.y1);
  atomicMin(&s->z0, a.z0); atomicMax(&s->z1, a.z1);
}
__device__ __forceinline__ void acc_voxel(comp_acc& a, int x, int y, int z) {
  a.cnt += 1; a.sx += x; a.sy += y; a.sz += z;
  a.x0 = min(a.x0, x); a.x1 = max(a.x1, x); a.y0 = min(a.y0, y); a.y1 = max(a.y1, y); a.z0 = min(a.z0, z); a.z1 = max(a.z1, z);
}
__device__ __forceinline__ comp_acc acc_empty() { return {0, 0, 0, 0, 0, INT_MAX, -1, INT_MAX, -1, INT_MAX, -1}; }
__global__ void stat_init_kernel(comp_stat* st, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st[i] = {0, 0, 0, 0, INT_MAX, -1, INT_MAX, -1, INT_MAX, -1, 0, 0};
}
// four voxels per lane; the lane's first label is summed in registers, then the lanes of a wave that hold the same label are summed with shuffles (two
// rounds: a wave inside one component, or on the border of two, sends one set of atomics); whatever is left goes out per lane.
__global__ __launch_bounds__(TPB) void cc_stats_kernel(const int32_t* __restrict__ labels, cc_dims d, int n, comp_stat* st) {
  const long long quads = (d.N + 3) / 4;
  const int lane = threadIdx.x & 63;
  for (long long q0 = (long long)blockIdx.x * TPB + (threadIdx.x - lane); q0 < quads; q0 += (long long)gridDim.x * TPB) {          // wave-uniform trip count
    const long long q = q0 + lane, f0 = 4 * q;
    int v[4] = {0, 0, 0, 0};
    if (q < quads) {
      if (f0 + 3 < d.N) { const int4 w = *reinterpret_cast<const int4*>(labels + f0); v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w; }
      else for (int i = 0; f0 + i < d.N; ++i) v[i] = labels[f0 + i];
    }
    comp_acc a = acc_empty();
    if (v[0] | v[1] | v[2] | v[3]) {
      int x, y, z;
      cc_f_to_xyz(d, f0, &x, &y, &z);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int l = v[i];
        if ((unsigned)(l - 1) < (unsigned)n) {                        // a label outside 1..n is ignored, never an address
          if (a.label == 0) a.label = l;
          if (l == a.label) acc_voxel(a, x, y, z);
          else { comp_acc one = acc_empty(); one.label = l; acc_voxel(one, x, y, z); stat_emit(st, one); }
        }
        if (++x == d.X) { x = 0; if (++y == d.Y) { y = 0; ++z; } }
      }
    }
    for (int round = 0; round < 2; ++round) {
      const unsigned long long pending = __ballot(a.label != 0);
      if (!pending) break;
      const int leader = __ffsll((long long)pending) - 1;
      const int L = __shfl(a.label, leader, 64);
      const bool part = a.label == L;
      comp_acc r = part ? a : acc_empty();
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        r.cnt += __shfl_xor(r.cnt, o, 64);
        r.sx += __shfl_xor(r.sx, o, 64); r.sy += __shfl_xor(r.sy, o, 64); r.sz += __shfl_xor(r.sz, o, 64);
        r.x0 = min(r.x0, __shfl_xor(r.x0, o, 64)); r.x1 = max(r.x1, __shfl_xor(r.x1, o, 64));
        r.y0 = min(r.y0, __shfl_xor(r.y0, o, 64)); r.y1 = max(r.y1, __shfl_xor(r.y1, o, 64));
        r.z0 = min(r.z0, __shfl_xor(r.z0, o, 64)); r.z1 = max(r.z1, __shfl_xor(r.z1, o, 64));
      }
      if (lane == leader) { r.label = L; stat_emit(st, r); }
      if (part) a.label = 0;
    }
    if (a.label != 0) stat_emit(st, a);
  }
}

// ---- filter: mask[v] = keep[labels[v]], and the set voxels of every slice of [z0, z1) ---------------------------------------------------------------
// A slice is X * Y contiguous voxels.  V = 16: four 16-byte label loads and one 16-byte mask store per lane.
template <int V>
__global__ __launch_bounds__(TPB) void cc_filter_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ keep, int n, long long XY, int bps, int z0, int z1,
                                                       uint8_t* __restrict__ mask, unsigned long long* __restrict__ counts) {
  __shared__ int s_w[TPB / 64];
  const int z = blockIdx.x / bps, part = blockIdx.x - z * bps;
  const long long base = (long long)z * XY;
  int cnt = 0;
  for (long long i = ((long long)part * TPB + threadIdx.x) * V; i < XY; i += (long long)bps * TPB * V) {
    int l[V]; uint8_t b[V];
    if constexpr (V == 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int4 w = *reinterpret_cast<const int4*>(labels + base + i + 4 * j); l[4 * j] = w.x; l[4 * j + 1] = w.y; l[4 * j + 2] = w.z; l[4 * j + 3] = w.w; }
    } else l[0] = labels[base + i];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      b[k] = ((unsigned)l[k] <= (unsigned)n && keep[l[k]]) ? 1 : 0;     // a label outside 0..n is dropped, never an address
      cnt += b[k];
    }
    if constexpr (V == 16) {
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = (unsigned)b[4 * j] | ((unsigned)b[4 * j + 1] << 8) | ((unsigned)b[4 * j + 2] << 16) | ((unsigned)b[4 * j + 3] << 24);
      *reinterpret_cast<uint4*>(mask + base + i) = make_uint4(w[0], w[1], w[2], w[3]);
    } else mask[base + i] = b[0];
  }
  const int t = vol_block_sum<int, TPB>(cnt, s_w);
  if (threadIdx.x == 0 && t && z >= z0 && z < z1) atomicAdd(counts + (z - z0), (unsigned long long)t);          // integer sums: exact in any order
}

inline cc_dims cc_make(int X, int Y, int Z) { return {X, Y, Z, (int)((long long)Y * Z), (long long)X * Y, (long long)X * Y * Z}; }
inline size_t cc_flag_bytes(long long N) { return (size_t)((N + 15) / 16 * 16); }
inline long long cc_chunks(long long N) { return (N + CHUNK - 1) / CHUNK; }
constexpr long long GRID_CAP = 256 * 32;                             // grid-stride launches: 32 workgroups per CU
}  // namespace

// the launches behind unet_vol_label / unet_vol_label_planar / unet_vol_fill_holes (invert: the components of the mask's ZERO voxels); connectivity is the caller's to check
int32_t k_vol_label(unet_ctx* ctx, const uint8_t* mask, int X, int Y, int Z, int connectivity, int planar, int invert, int32_t* labels, int32_t* n_out, void* ws, size_t ws_bytes,
                    hipStream_t s) {
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_label: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  const cc_dims d = cc_make(X, Y, Z);
  if (d.N == 0) { UNET_HIP(ctx, hipMemsetAsync(n_out, 0, sizeof(int32_t), s)); return UNET_OK; }
  if (!mask || !labels || !ws) UNET_FAIL(ctx, UNET_E_ARG, "vol_label: bad args");
  if (ws_bytes < unet_vol_label_ws_bytes(X, Y, Z) || (reinterpret_cast<uintptr_t>(ws) % 16) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_label: workspace too small or not 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(labels) % 16) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_label: labels is not 16-byte aligned");
  uint8_t* flags = static_cast<uint8_t*>(ws);
  const size_t npad = cc_flag_bytes(d.N);
  int32_t* bsum = reinterpret_cast<int32_t*>(flags + npad);
  const int nb = (int)cc_chunks(d.N);
  UNET_HIP(ctx, hipMemsetAsync(flags, 0, npad, s));
  const int nbx = (X + BX - 1) / BX, nby = (Y + BY - 1) / BY, nbz = (Z + BZ - 1) / BZ;
  const long long bricks = (long long)nbx * nby * nbz;
  if (bricks > 0x7FFFFFFFLL) UNET_FAIL(ctx, UNET_E_ARG, "vol_label: too many bricks");
  if ((X % 16) == 0 && (reinterpret_cast<uintptr_t>(mask) % 16) == 0)
    hipLaunchKernelGGL(cc_local_kernel<true>, dim3((unsigned)bricks), dim3(TPB), 0, s, mask, d, connectivity, planar, invert, nbx, nby, labels);
  else
    hipLaunchKernelGGL(cc_local_kernel<false>, dim3((unsigned)bricks), dim3(TPB), 0, s, mask, d, connectivity, planar, invert, nbx, nby, labels);
  const long long PX = (long long)(nbx - 1) * Y * Z, PY = (long long)(nby - 1) * X * Z, PZ = (long long)(nbz - 1) * X * Y;
  if (PX + PY + PZ > 0) hipLaunchKernelGGL(cc_merge_kernel, dim3(vol_blocks(PX + PY + PZ, GRID_CAP, TPB)), dim3(TPB), 0, s, labels, d, connectivity, planar, PX, PY, PZ);
  const long long quads = (d.N + 3) / 4;
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(vol_blocks(quads, GRID_CAP, TPB)), dim3(TPB), 0, s, labels, d, flags);
  hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, flags, (long long)npad, bsum);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(1024), 0, s, bsum, nb, n_out);
  hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)nb), dim3(TPB), 0, s, flags, (long long)npad, bsum, d, labels);
  hipLaunchKernelGGL(cc_final_kernel, dim3(vol_blocks(quads, GRID_CAP, TPB)), dim3(TPB), 0, s, labels, d);
  UNET_CHECK_LAUNCH(ctx, "vol_label"); return UNET_OK;
}

extern "C" {

size_t unet_vol_label_ws_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!vol_dims_ok(X, Y, Z)) return 0;
  const long long N = (long long)X * Y * Z;
  if (N == 0) return 0;
  return cc_flag_bytes(N) + (size_t)((cc_chunks(N) * sizeof(int32_t) + 15) / 16 * 16);
}

int32_t unet_vol_label(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, int32_t* labels, int32_t* n_out, void* ws, size_t ws_bytes,
                       void* stream) {
  if (!ctx || !n_out) UNET_FAIL(ctx, UNET_E_ARG, "vol_label: bad args");
  if (connectivity < 1 || connectivity > 3) UNET_FAIL(ctx, UNET_E_ARG, "vol_label: connectivity %d is not 1 (6 neighbours), 2 (18) or 3 (26)", connectivity);
  return k_vol_label(ctx, mask, X, Y, Z, connectivity, 0, 0, labels, n_out, ws, ws_bytes, as_stream(stream));
}

int32_t unet_vol_label_planar(unet_ctx* ctx, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, int32_t* labels, int32_t* n_out, void* ws, size_t ws_bytes,
                              void* stream) {
  if (!ctx || !n_out) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_planar: bad args");
  if (connectivity < 1 || connectivity > 2) UNET_FAIL(ctx, UNET_E_ARG, "vol_label_planar: connectivity %d is not 1 (4 neighbours in the slice) or 2 (8)", connectivity);
  return k_vol_label(ctx, mask, X, Y, Z, connectivity, 1, 0, labels, n_out, ws, ws_bytes, as_stream(stream));
}

int32_t unet_vol_component_stats(unet_ctx* ctx, const int32_t* labels, int32_t X, int32_t Y, int32_t Z, int32_t n, void* stats, void* stream) {
  if (!ctx || n < 0 || !vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_component_stats: bad args");
  const cc_dims d = cc_make(X, Y, Z);
  if (n == 0 || d.N == 0) return UNET_OK;
  if (!labels || !stats || (reinterpret_cast<uintptr_t>(labels) % 16) != 0 || (reinterpret_cast<uintptr_t>(stats) % 8) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_component_stats: null or misaligned buffer (labels 16 bytes, stats 8)");
  hipStream_t s = as_stream(stream);
  comp_stat* st = static_cast<comp_stat*>(stats);
  hipLaunchKernelGGL(stat_init_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s, st, n);
  hipLaunchKernelGGL(cc_stats_kernel, dim3(vol_blocks((d.N + 3) / 4, GRID_CAP, TPB)), dim3(TPB), 0, s, labels, d, n, st);
  UNET_CHECK_LAUNCH(ctx, "vol_component_stats"); return UNET_OK;
}

int32_t unet_vol_filter_components(unet_ctx* ctx, const int32_t* labels, const uint8_t* keep, int32_t n, int32_t X, int32_t Y, int32_t Z, int32_t z0, int32_t z1, uint8_t* mask,
                                   int64_t* counts, void* stream) {
  if (!ctx || n < 0 || !keep || !vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_filter_components: bad args");
  if (z0 < 0 || z1 > Z || z1 < z0 || (z1 > z0 && !counts)) UNET_FAIL(ctx, UNET_E_ARG, "vol_filter_components: slice range [%d, %d) leaves the %d slices", z0, z1, Z);
  hipStream_t s = as_stream(stream);
  if (z1 > z0) UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)(z1 - z0) * sizeof(int64_t), s));
  const cc_dims d = cc_make(X, Y, Z);
  if (d.N == 0) return UNET_OK;
  if (!labels || !mask) UNET_FAIL(ctx, UNET_E_ARG, "vol_filter_components: bad args");
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  const bool vec = (d.XY % 16) == 0 && (reinterpret_cast<uintptr_t>(labels) % 16) == 0 && (reinterpret_cast<uintptr_t>(mask) % 16) == 0;
  const long long per = vec ? (long long)TPB * 16 : TPB;
  long long bps = (d.XY + per - 1) / per;
  bps = bps > 64 ? 64 : bps;
  if (vec) hipLaunchKernelGGL(cc_filter_kernel<16>, dim3((unsigned)(bps * Z)), dim3(TPB), 0, s, labels, keep, n, d.XY, (int)bps, z0, z1, mask, cnt);
  else hipLaunchKernelGGL(cc_filter_kernel<1>, dim3((unsigned)(bps * Z)), dim3(TPB), 0, s, labels, keep, n, d.XY, (int)bps, z0, z1, mask, cnt);
  UNET_CHECK_LAUNCH(ctx, "vol_filter_components"); return UNET_OK;
}

}  // extern "C"

// Bottleneck-feature PCA and KMeans (cluster.py: the reference's PCA(1000) + KMeans(2) over conv2d_9 taps, T1:1386-1496), on the device.
//   col_mean  mu[j] = (1/n) sum_i x[i][j]                           fp64 accumulation, one thread per column, rows in order
//   gemm NT   C[m x p] = (A - 1 mu_a^T)(B - 1 mu_b^T)^T              reduction over the contiguous axis d (Gram matrix, transform)
//   gemm TN   O[k x d] = W^T (X - 1 mu^T),  W n x k                    reduction over the sample axis n (PCA components)
//   kmeans    labels / per-cluster fp64 sums and counts / inertia of one Lloyd step, one workgroup
// The two products share one MFMA tile core: a 128 x 128 output tile per workgroup, four waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x2_f32 blocks, the
// strict fp32 family of kernels_conv_mfma.hip: A[m = l31][k = hi], B[k = hi][n = l31], D row (r&3)+8(r>>2)+4hi, column l31).  Operands are staged
// through LDS as [k][m] in K blocks of 32, the means subtracted in fp32 as they are staged ((float)mu); NT transposes while staging, TN stores rows as
// they come.  The fp32 MFMA accumulators hold one K block (32 products) and are then added into fp64 registers, so the fp32 part of the error stays at
// the scale of 32 terms whatever d is.  Split-K: blockIdx.y is a K slab, each slab writes fp64 partials, and a second kernel adds the slabs in slab
// order (and mirrors the symmetric form) -- every reduction has a fixed order, there are no atomics, reruns are bit-identical.  64-bit addressing
// throughout: a row offset is row * (long long)ld.
#include "common.h"

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int TB = 128, KB = 32, THREADS = 256;
constexpr int LDS_LD = TB + 4;                 // [k][m] staging stride: rows k and k + 8 (the two lane halves of one MFMA step) sit 32 banks apart
constexpr long long MAX_PARTIAL_BYTES = 1LL << 30;

struct Split {
  long long tm, tp, tiles, slabs, kslab;
};

// tile grid and K slabs of a product: enough workgroups for the 256 CUs, slabs a multiple of KB and >= 256 long, partials <= 1 GiB
Split plan_split(long long m, long long p, long long K, bool sym) {
  Split s;
  s.tm = (m + TB - 1) / TB; s.tp = (p + TB - 1) / TB;
  s.tiles = sym ? s.tm * (s.tm + 1) / 2 : s.tm * s.tp;
  long long want = (1024 + s.tiles - 1) / s.tiles;
  const long long by_len = (K + 255) / 256;
  if (want > by_len) want = by_len;
  const long long by_mem = MAX_PARTIAL_BYTES / (m * p * 8 > 0 ? m * p * 8 : 1);
  if (want > by_mem) want = by_mem;
  if (want < 1) want = 1;
  const long long per = (K + want - 1) / want;
  s.kslab = (per + KB - 1) / KB * KB;
  s.slabs = (K + s.kslab - 1) / s.kslab;
  if (s.slabs < 1) s.slabs = 1;
  return s;
}
bool needs_partials(const Split& s, bool sym) { return sym || s.slabs > 1; }

// TN = false: operand rows are the output index, K contiguous (x[row * ld + k]); the mean is indexed by k.
// TN = true : operand rows are K, the output index contiguous (x[k * ld + col]); the mean is indexed by the column.
template <bool TN>
__device__ __forceinline__ void load_operand(const float* __restrict__ x, long long ld, const double* __restrict__ mu, long long rows, long long r0,
                                             long long kb, long long kend, bool vec, float v[16]) {
  const int t = threadIdx.x;
  if (!TN) {
    const int k4 = t & 7, rr = t >> 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long row = r0 + rr + 32 * r, k = kb + 4 * k4;
      if (vec && row < rows && k + 3 < kend) {
        const float4 q = *reinterpret_cast<const float4*>(x + row * ld + k);
        v[4 * r + 0] = q.x; v[4 * r + 1] = q.y; v[4 * r + 2] = q.z; v[4 * r + 3] = q.w;
        if (mu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * r + e] -= (float)mu[k + e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * r + e] = (row < rows && k + e < kend) ? x[row * ld + k + e] - (mu ? (float)mu[k + e] : 0.f) : 0.f;
      }
    }
  } else {
    const int c4 = t & 31, kk = t >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long k = kb + kk + 8 * r, col = r0 + 4 * c4;
      if (vec && k < kend && col + 3 < rows) {
        const float4 q = *reinterpret_cast<const float4*>(x + k * ld + col);
        v[4 * r + 0] = q.x; v[4 * r + 1] = q.y; v[4 * r + 2] = q.z; v[4 * r + 3] = q.w;
        if (mu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[4 * r + e] -= (float)mu[col + e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * r + e] = (k < kend && col + e < rows) ? x[k * ld + col + e] - (mu ? (float)mu[col + e] : 0.f) : 0.f;
      }
    }
  }
}

template <bool TN>
__device__ __forceinline__ void store_operand(float* s, const float v[16]) {
  const int t = threadIdx.x;
  if (!TN) {
    const int k4 = t & 7, rr = t >> 3;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[(4 * k4 + e) * LDS_LD + rr + 32 * r] = v[4 * r + e];
  } else {
    const int c4 = t & 31, kk = t >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) *reinterpret_cast<float4*>(&s[(kk + 8 * r) * LDS_LD + 4 * c4]) = make_float4(v[4 * r], v[4 * r + 1], v[4 * r + 2], v[4 * r + 3]);
  }
}

// out = part (fp64 partials [slab][m][p]) when `part` is set, else the output itself (out_f64 ? double : float, leading dimension ldc)
template <bool TN>
__global__ __launch_bounds__(THREADS) void feat_gemm_kernel(const float* __restrict__ a, long long lda, const double* __restrict__ mu_a,
                                                             const float* __restrict__ b, long long ldb, const double* __restrict__ mu_b, long long m,
                                                             long long p, long long K, long long kslab, long long tiles_m, int sym, int vec,
                                                             double* __restrict__ part, void* __restrict__ out, long long ldc, int out_f64) {
  __shared__ float As[KB * LDS_LD];
  __shared__ float Bs[KB * LDS_LD];
  long long tm, tp;
  if (sym) {                                                     // upper-triangle tile pairs tm <= tp, row by row
    long long t = blockIdx.x;
    tm = 0;
    while (t >= tiles_m - tm) { t -= tiles_m - tm; ++tm; }
    tp = tm + t;
  } else {
    tm = (long long)blockIdx.x % tiles_m; tp = (long long)blockIdx.x / tiles_m;   // tm fastest: neighbouring workgroups share the B tile
  }
  const long long i0 = tm * TB, j0 = tp * TB;
  const long long slab = blockIdx.y, kbeg = slab * kslab;
  const long long kend = kbeg + kslab < K ? kbeg + kslab : K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wm = wave >> 1, wp = wave & 1;

  f32x16 acc[2][2];
  double acc64[2][2][16];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[x][y][r] = 0.f; acc64[x][y][r] = 0.0; }
    }

  float va[16], vb[16];
  load_operand<TN>(a, lda, mu_a, m, i0, kbeg, kend, vec, va);
  load_operand<TN>(b, ldb, mu_b, p, j0, kbeg, kend, vec, vb);
  for (long long kb = kbeg; kb < kend; kb += KB) {
    __syncthreads();
    store_operand<TN>(As, va);
    store_operand<TN>(Bs, vb);
    __syncthreads();
    if (kb + KB < kend) {                                        // the next block's loads fly under this block's MFMAs
      load_operand<TN>(a, lda, mu_a, m, i0, kb + KB, kend, vec, va);
      load_operand<TN>(b, ldb, mu_b, p, j0, kb + KB, kend, vec, vb);
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int k = hi * 8 + (t & 7) + (t >> 3) * 16;            // lane half hi covers k in {8hi..8hi+7, 16+8hi..16+8hi+7}: all 32 once
      const float a0 = As[k * LDS_LD + wm * 64 + l31], a1 = As[k * LDS_LD + wm * 64 + 32 + l31];
      const float b0 = Bs[k * LDS_LD + wp * 64 + l31], b1 = Bs[k * LDS_LD + wp * 64 + 32 + l31];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc64[x][y][r] += (double)acc[x][y][r]; acc[x][y][r] = 0.f; }
      }
  }

#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const long long gj = j0 + wp * 64 + y * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long gi = i0 + wm * 64 + x * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (gi < m && gj < p) {
          if (part) part[(slab * m + gi) * p + gj] = acc64[x][y][r];
          else if (out_f64) static_cast<double*>(out)[gi * ldc + gj] = acc64[x][y][r];
          else static_cast<float*>(out)[gi * ldc + gj] = (float)acc64[x][y][r];
        }
      }
    }
}

// out[i][j] = sum over slabs, in slab order, of part[s][i][j]; the symmetric form reads the upper triangle for both (i, j) and (j, i)
__global__ __launch_bounds__(256) void feat_reduce_kernel(const double* __restrict__ part, long long slabs, long long m, long long p, int sym,
                                                           void* __restrict__ out, long long ldc, int out_f64) {
  const long long total = m * p;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long i = e / p, j = e - i * p;
    const long long ii = (sym && i > j) ? j : i, jj = (sym && i > j) ? i : j;
    double v = 0.0;
    for (long long s = 0; s < slabs; ++s) v += part[(s * m + ii) * p + jj];
    if (out_f64) static_cast<double*>(out)[i * ldc + j] = v;
    else static_cast<float*>(out)[i * ldc + j] = (float)v;
  }
}

__global__ __launch_bounds__(256) void col_mean_kernel(const float* __restrict__ x, long long ldx, long long n, long long d, double* __restrict__ mu) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= d) return;
  double s = 0.0;
  for (long long i = 0; i < n; ++i) s += (double)x[i * ldx + j];
  mu[j] = s / (double)n;
}

// One Lloyd step in ONE workgroup (so every reduction has one fixed order without a second launch).  Phase 1: wave w takes points w, w + 16, ...; the
// squared distance to each centre is summed in fp64 over lane-strided coordinates, then a butterfly across the wave; the lowest index wins a tie.
// Phase 2: thread j owns column j of every cluster sum and adds the points of that cluster in point order; threads < k count; the inertia is a
// per-thread strided sum of the distances followed by a fixed LDS tree.
constexpr int KM_THREADS = 1024;
__global__ __launch_bounds__(KM_THREADS) void kmeans_step_kernel(const float* __restrict__ pts, long long ldp, long long n, long long p,
                                                                  const double* __restrict__ cen, int k, int* __restrict__ labels,
                                                                  double* __restrict__ dist, double* __restrict__ sums, long long* __restrict__ counts,
                                                                  double* __restrict__ inertia) {
  __shared__ double red[KM_THREADS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long i = wave; i < n; i += KM_THREADS / 64) {
    const float* x = pts + i * ldp;
    double best = 0.0;
    int bl = 0;
    for (int c = 0; c < k; ++c) {
      const double* cc = cen + (long long)c * p;
      double s = 0.0;
      for (long long j = lane; j < p; j += 64) {
        const double df = (double)x[j] - cc[j];
        s = fma(df, df, s);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (c == 0 || s < best) { best = s; bl = c; }
    }
    if (lane == 0) { labels[i] = bl; dist[i] = best; }
  }
  __threadfence();
  __syncthreads();
  for (long long j = threadIdx.x; j < p; j += KM_THREADS)
    for (int c = 0; c < k; ++c) {
      double s = 0.0;
      for (long long i = 0; i < n; ++i)
        if (labels[i] == c) s += (double)pts[i * ldp + j];
      sums[(long long)c * p + j] = s;
    }
  for (int c = threadIdx.x; c < k; c += KM_THREADS) {
    long long cnt = 0;
    for (long long i = 0; i < n; ++i) cnt += labels[i] == c;
    counts[c] = cnt;
  }
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += KM_THREADS) s += dist[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = KM_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *inertia = red[0];
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// ---- routing (routed.py: a new slice's cluster, T1:1386-1496 applied to one batch) -----------------------------------------------------------------
// proj[i][r] = sum_t (x_i[t] - mu[t]) comps[r][t] over the tap in (h, w, c) order, then labels[i] = argmin_c ||proj_i - centre_c||^2.  n is small (one
// predict batch), k <= ~1000, d up to 512 * 32 * 32: the product streams comps once per 64 rows.  Launch 1 (route_partial_kernel): a workgroup owns 32
// components x (up to) 64 rows x one K slab; its four waves take the slab's K blocks of 32 round-robin, each block one 16-step run of
// v_mfma_f32_32x32x2_f32 (lane (l31, hi) loads 16 contiguous terms t = kb + 16 hi + 0..15 of component r0 + l31 and of row i0 + l31: step s pairs them,
// so a block covers its 32 terms once) whose fp32 result is added into fp64; the waves fold in a fixed tree ((w0 + w1) + (w2 + w3)) and the workgroup
// writes one fp64 partial per (slab, row, component).  Launch 2 (route_assign_kernel): one workgroup per row adds the slabs in slab order, rounds to
// fp32 (the points unet_kmeans_step sees), and takes fp64 squared distances by direct differences: thread-strided over components, then a fixed LDS
// tree; the lowest index wins a tie.  The slab plan depends on (d, k) alone and a row's arithmetic never on its neighbours, so route(x)[i] is
// bit-identical to route(x[i:i+1]).
constexpr int RT_CT = 32, RT_WAVES = 4, RT_NC_MAX = 16;
constexpr long long RT_TARGET_WG = 2048;

struct RoutePlan {
  long long tiles_k, slabs, kslab;
};
RoutePlan route_plan(long long d, long long k) {
  RoutePlan p;
  p.tiles_k = (k + RT_CT - 1) / RT_CT;
  const long long blocks = (d + KB - 1) / KB;
  long long want = (RT_TARGET_WG + p.tiles_k - 1) / p.tiles_k;
  const long long by_len = (blocks + 4 * RT_WAVES - 1) / (4 * RT_WAVES);       // >= 4 K blocks per wave
  if (want > by_len) want = by_len;
  if (want < 1) want = 1;
  p.kslab = (blocks + want - 1) / want * KB;
  p.slabs = (d + p.kslab - 1) / p.kslab;
  return p;
}

// 16 terms t0..t0+15 of tap row `row` (NHWC view, pixel stride ld, row stride hw * ld), the fp32 mean subtracted; zero past n or d
template <typename T>
__device__ __forceinline__ void route_load_x(const T* __restrict__ x, long long rs, int c, long long ld, const float* __restrict__ mu, long long n,
                                             long long d, long long row, long long t0, bool vec, float v[16]) {
  if (vec && row < n && t0 + 16 <= d) {                        // c % 16 == 0: the 16 terms are 16 channels of one pixel
    const long long pix = t0 / c;
    const T* p = x + row * rs + pix * ld + (t0 - pix * c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 a = ld4(p + 4 * q);
      v[4 * q + 0] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
    }
    if (mu) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 m = *reinterpret_cast<const float4*>(mu + t0 + 4 * q);
        v[4 * q + 0] -= m.x; v[4 * q + 1] -= m.y; v[4 * q + 2] -= m.z; v[4 * q + 3] -= m.w;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const long long t = t0 + e;
      if (row < n && t < d) {
        const long long pix = t / c;
        v[e] = ld1(x + row * rs + pix * ld + (t - pix * c)) - (mu ? mu[t] : 0.f);
      } else {
        v[e] = 0.f;
      }
    }
  }
}

// 16 terms t0..t0+15 of component r (dense k x d); zero past k or d
__device__ __forceinline__ void route_load_w(const float* __restrict__ w, long long k, long long d, long long r, long long t0, bool vec, float v[16]) {
  if (vec && r < k && t0 + 16 <= d) {
    const float* p = w + r * d + t0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 a = *reinterpret_cast<const float4*>(p + 4 * q);
      v[4 * q + 0] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = (r < k && t0 + e < d) ? w[r * d + t0 + e] : 0.f;
  }
}

// part[(slab * n + i) * k + r]: the fp64 partial of row i, component r over K slab `slab`.  NT row tiles of 32 (NT * 32 rows per workgroup).
template <typename T, int NT>
__global__ __launch_bounds__(RT_WAVES * 64) void route_partial_kernel(const T* __restrict__ x, long long rs, int c, long long ld, int vec_x,
                                                                       const float* __restrict__ w, const float* __restrict__ mu, int vec_w, long long n,
                                                                       long long d, long long k, long long kslab, double* __restrict__ part) {
  __shared__ double red[2 * NT * 16 * 64];                   // two waves' fp64 accumulators [wave pair][j][lane]; reused as the [row][component] tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
  const long long r0 = (long long)blockIdx.x * RT_CT, slab = blockIdx.y, i0 = (long long)blockIdx.z * (32 * NT);
  const long long kbeg = slab * kslab, kend = kbeg + kslab < d ? kbeg + kslab : d;
  f32x16 acc[NT];
  double acc64[NT][16];
#pragma unroll
  for (int y = 0; y < NT; ++y)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[y][r] = 0.f; acc64[y][r] = 0.0; }

  float va[16], vb[NT][16];
  long long kb = kbeg + (long long)wave * KB;
  if (kb < kend) {
    route_load_w(w, k, d, r0 + l31, kb + 16 * hi, vec_w, va);
#pragma unroll
    for (int y = 0; y < NT; ++y) route_load_x(x, rs, c, ld, mu, n, d, i0 + 32 * y + l31, kb + 16 * hi, vec_x, vb[y]);
  }
  for (; kb < kend; kb += RT_WAVES * KB) {
    float ca[16], cb[NT][16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      ca[e] = va[e];
#pragma unroll
      for (int y = 0; y < NT; ++y) cb[y][e] = vb[y][e];
    }
    const long long kn = kb + RT_WAVES * KB;
    if (kn < kend) {                                           // the wave's next block loads under this block's MFMAs
      route_load_w(w, k, d, r0 + l31, kn + 16 * hi, vec_w, va);
#pragma unroll
      for (int y = 0; y < NT; ++y) route_load_x(x, rs, c, ld, mu, n, d, i0 + 32 * y + l31, kn + 16 * hi, vec_x, vb[y]);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int y = 0; y < NT; ++y) acc[y] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s], cb[y][s], acc[y], 0, 0, 0);
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc64[y][r] += (double)acc[y][r]; acc[y][r] = 0.f; }
  }

  // fixed fold: w0 += w1, w2 += w3, then w0 += w2
  if (wave & 1) {
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((wave >> 1) * NT * 16 + y * 16 + r) * 64 + lane] = acc64[y][r];
  }
  __syncthreads();
  if (!(wave & 1)) {
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc64[y][r] += red[((wave >> 1) * NT * 16 + y * 16 + r) * 64 + lane];
  }
  __syncthreads();
  if (wave == 2) {
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(y * 16 + r) * 64 + lane] = acc64[y][r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc64[y][r] += red[(y * 16 + r) * 64 + lane];
  }
  __syncthreads();
  if (wave == 0) {                                             // D row (r&3) + 8(r>>2) + 4hi = component, column l31 = row: stage as [row][component]
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(32 * y + l31) * RT_CT + (r & 3) + 8 * (r >> 2) + 4 * hi] = acc64[y][r];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 32 * NT * RT_CT; e += RT_WAVES * 64) {
    const long long i = i0 + e / RT_CT, r = r0 + e % RT_CT;
    if (i < n && r < k) part[(slab * n + i) * k + r] = red[e];
  }
}

// one workgroup per row: proj (fp32) = the slabs added in slab order; fp64 squared distances to every centre; lowest-index argmin
constexpr int RA_THREADS = 256;
__global__ __launch_bounds__(RA_THREADS) void route_assign_kernel(const double* __restrict__ part, long long slabs, long long n, long long k,
                                                                  const double* __restrict__ cen, int nc, float* __restrict__ proj,
                                                                  int* __restrict__ labels, double* __restrict__ dist) {
  __shared__ double red[RT_NC_MAX * RA_THREADS];
  const long long i = blockIdx.x;
  double s[RT_NC_MAX];
#pragma unroll
  for (int cc = 0; cc < RT_NC_MAX; ++cc) s[cc] = 0.0;
  for (long long r = threadIdx.x; r < k; r += RA_THREADS) {
    double v = 0.0;
    for (long long sl = 0; sl < slabs; ++sl) v += part[(sl * n + i) * k + r];
    const float pf = (float)v;
    if (proj) proj[i * k + r] = pf;
#pragma unroll
    for (int cc = 0; cc < RT_NC_MAX; ++cc)
      if (cc < nc) {
        const double df = (double)pf - cen[(long long)cc * k + r];
        s[cc] = fma(df, df, s[cc]);
      }
  }
#pragma unroll
  for (int cc = 0; cc < RT_NC_MAX; ++cc)
    if (cc < nc) red[cc * RA_THREADS + threadIdx.x] = s[cc];
  __syncthreads();
  for (int wdt = RA_THREADS / 2; wdt >= 1; wdt >>= 1) {
    if ((int)threadIdx.x < wdt)
      for (int cc = 0; cc < nc; ++cc) red[cc * RA_THREADS + threadIdx.x] += red[cc * RA_THREADS + threadIdx.x + wdt];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double best = red[0];
    int bl = 0;
    for (int cc = 1; cc < nc; ++cc)
      if (red[cc * RA_THREADS] < best) { best = red[cc * RA_THREADS]; bl = cc; }
    labels[i] = bl;
    dist[i] = best;
  }
}


template <bool TN>
int32_t run_gemm(unet_ctx* ctx, const char* what, const float* a, long long lda, const double* mu_a, const float* b, long long ldb, const double* mu_b,
                 long long m, long long p, long long K, bool sym, void* c, long long ldc, int32_t c_dtype, void* ws, size_t ws_bytes, void* stream) {
  const Split s = plan_split(m, p, K, sym);
  const bool use_part = needs_partials(s, sym);
  const size_t need = use_part ? (size_t)(s.slabs * m * p * 8) : 0;
  if (use_part && (!ws || ws_bytes < need)) UNET_FAIL(ctx, UNET_E_ARG, "%s: workspace of %zu bytes is smaller than the %zu the shape needs", what, ws_bytes, need);
  if (s.tiles > 0x7fffffffLL || s.slabs > 65535) UNET_FAIL(ctx, UNET_E_SHAPE, "%s: %lld x %lld x %lld is too large a product", what, m, p, K);
  const int vec = aligned16(a) && aligned16(b) && lda % 4 == 0 && ldb % 4 == 0;
  double* part = use_part ? static_cast<double*>(ws) : nullptr;
  hipLaunchKernelGGL(feat_gemm_kernel<TN>, dim3((unsigned)s.tiles, (unsigned)s.slabs), dim3(THREADS), 0, as_stream(stream), a, lda, mu_a, b, ldb, mu_b, m,
                     p, K, s.kslab, s.tm, (int)sym, vec, part, c, ldc, (int)(c_dtype == UNET_FEAT_OUT_F64));
  UNET_CHECK_LAUNCH(ctx, what);
  if (use_part) {
    long long blocks = (m * p + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(feat_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), part, s.slabs, m, p, (int)sym, c, ldc,
                       (int)(c_dtype == UNET_FEAT_OUT_F64));
    UNET_CHECK_LAUNCH(ctx, what);
  }
  return UNET_OK;
}
}  // namespace

extern "C" {

int32_t unet_feat_col_mean(unet_ctx* ctx, const float* x, int64_t ldx, int64_t n, int64_t d, double* mu, void* stream) {
  if (!x || !mu || n < 1 || d < 1 || ldx < d) UNET_FAIL(ctx, UNET_E_ARG, "feat_col_mean: bad args (x, mu non-null; n, d >= 1; ldx >= d)");
  hipLaunchKernelGGL(col_mean_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, as_stream(stream), x, (long long)ldx, (long long)n, (long long)d, mu);
  UNET_CHECK_LAUNCH(ctx, "feat_col_mean");
  return UNET_OK;
}

size_t unet_feat_gemm_nt_workspace(int64_t m, int64_t p, int64_t d, int32_t sym) {
  if (m < 1 || p < 1 || d < 1) return 0;
  const Split s = plan_split(m, p, d, sym != 0);
  return needs_partials(s, sym != 0) ? (size_t)(s.slabs * m * p * 8) : 0;
}

int32_t unet_feat_gemm_nt(unet_ctx* ctx, const float* a, int64_t lda, const double* mu_a, const float* b, int64_t ldb, const double* mu_b, int64_t m,
                          int64_t p, int64_t d, int32_t sym, void* c, int64_t ldc, int32_t c_dtype, void* ws, size_t ws_bytes, void* stream) {
  if (!a || !b || !c || m < 1 || p < 1 || d < 1 || lda < d || ldb < d || ldc < p || (c_dtype != UNET_FEAT_OUT_F32 && c_dtype != UNET_FEAT_OUT_F64))
    UNET_FAIL(ctx, UNET_E_ARG, "feat_gemm_nt: bad args (a, b, c non-null; m, p, d >= 1; lda, ldb >= d; ldc >= p; c_dtype F32 or F64)");
  if (sym && (a != b || lda != ldb || mu_a != mu_b || m != p))
    UNET_FAIL(ctx, UNET_E_ARG, "feat_gemm_nt: the symmetric form needs a == b, lda == ldb, mu_a == mu_b and m == p");
  return run_gemm<false>(ctx, "feat_gemm_nt", a, lda, mu_a, b, ldb, mu_b, m, p, d, sym != 0, c, ldc, c_dtype, ws, ws_bytes, stream);
}

size_t unet_feat_gemm_tn_workspace(int64_t k, int64_t d, int64_t n) {
  if (k < 1 || d < 1 || n < 1) return 0;
  const Split s = plan_split(k, d, n, false);
  return needs_partials(s, false) ? (size_t)(s.slabs * k * d * 8) : 0;
}

int32_t unet_feat_gemm_tn(unet_ctx* ctx, const float* w, int64_t ldw, const float* x, int64_t ldx, const double* mu, int64_t n, int64_t k, int64_t d,
                          void* out, int64_t ldo, int32_t out_dtype, void* ws, size_t ws_bytes, void* stream) {
  if (!w || !x || !out || n < 1 || k < 1 || d < 1 || ldw < k || ldx < d || ldo < d || (out_dtype != UNET_FEAT_OUT_F32 && out_dtype != UNET_FEAT_OUT_F64))
    UNET_FAIL(ctx, UNET_E_ARG, "feat_gemm_tn: bad args (w, x, out non-null; n, k, d >= 1; ldw >= k; ldx, ldo >= d; out_dtype F32 or F64)");
  return run_gemm<true>(ctx, "feat_gemm_tn", w, ldw, nullptr, x, ldx, mu, k, d, n, false, out, ldo, out_dtype, ws, ws_bytes, stream);
}

int32_t unet_kmeans_step(unet_ctx* ctx, const float* pts, int64_t ldp, int64_t n, int64_t p, const double* centres, int32_t k, int32_t* labels,
                         double* dist, double* sums, int64_t* counts, double* inertia, void* stream) {
  if (!pts || !centres || !labels || !dist || !sums || !counts || !inertia || n < 1 || p < 1 || ldp < p || k < 1)
    UNET_FAIL(ctx, UNET_E_ARG, "kmeans_step: bad args (every pointer non-null; n, p, k >= 1; ldp >= p)");
  hipLaunchKernelGGL(kmeans_step_kernel, dim3(1), dim3(KM_THREADS), 0, as_stream(stream), pts, (long long)ldp, (long long)n, (long long)p, centres, (int)k,
                     labels, dist, sums, reinterpret_cast<long long*>(counts), inertia);
  UNET_CHECK_LAUNCH(ctx, "kmeans_step");
  return UNET_OK;
}

size_t unet_cluster_route_workspace(int64_t n, int64_t d, int32_t k) {
  if (n < 1 || d < 1 || k < 1) return 0;
  const RoutePlan p = route_plan(d, k);
  return (size_t)(p.slabs * n * (long long)k * 8);
}

int32_t unet_cluster_route(unet_ctx* ctx, const void* tap, int32_t tap_bf16, int64_t n, int32_t h, int32_t w, int32_t c, int64_t ld,
                           const float* comps_hwc, const float* mu_hwc, int32_t k, const double* centres, int32_t nc, float* proj, int32_t* labels,
                           double* dist, void* ws, size_t ws_bytes, void* stream) {
  if (!tap || !comps_hwc || !centres || !labels || !dist || n < 1 || h < 1 || w < 1 || c < 1 || ld < c || k < 1 || nc < 1 || nc > RT_NC_MAX)
    UNET_FAIL(ctx, UNET_E_ARG, "cluster_route: bad args (tap, comps, centres, labels, dist non-null; n, h, w, c, k >= 1; ld >= c; 1 <= nc <= %d)", RT_NC_MAX);
  const long long d = (long long)h * w * c, rs = (long long)h * w * ld;
  const RoutePlan p = route_plan(d, k);
  const size_t need = (size_t)(p.slabs * n * (long long)k * 8);
  if (!ws || ws_bytes < need) UNET_FAIL(ctx, UNET_E_ARG, "cluster_route: workspace of %zu bytes is smaller than the %zu the shape needs", ws_bytes, need);
  const long long tiles_n = (n + 63) / 64;
  if (p.tiles_k > 0x7fffffffLL || p.slabs > 65535 || tiles_n > 65535 || n > 0x7fffffffLL)
    UNET_FAIL(ctx, UNET_E_SHAPE, "cluster_route: n = %lld, d = %lld, k = %d is too large", (long long)n, d, k);
  const int vec_x = c % 16 == 0 && ld % 4 == 0 && aligned16(tap) && (!mu_hwc || aligned16(mu_hwc));
  const int vec_w = d % 4 == 0 && aligned16(comps_hwc);
  double* part = static_cast<double*>(ws);
  const bool two = n > 32;
  const dim3 grid((unsigned)p.tiles_k, (unsigned)p.slabs, (unsigned)(two ? tiles_n : n > 0 ? (n + 31) / 32 : 1));
  const dim3 block(RT_WAVES * 64);
  if (tap_bf16) {
    const unet_bf16* x = static_cast<const unet_bf16*>(tap);
    if (two) hipLaunchKernelGGL((route_partial_kernel<unet_bf16, 2>), grid, block, 0, as_stream(stream), x, rs, (int)c, (long long)ld, vec_x, comps_hwc, mu_hwc, vec_w, (long long)n, d, (long long)k, p.kslab, part);
    else hipLaunchKernelGGL((route_partial_kernel<unet_bf16, 1>), grid, block, 0, as_stream(stream), x, rs, (int)c, (long long)ld, vec_x, comps_hwc, mu_hwc, vec_w, (long long)n, d, (long long)k, p.kslab, part);
  } else {
    const float* x = static_cast<const float*>(tap);
    if (two) hipLaunchKernelGGL((route_partial_kernel<float, 2>), grid, block, 0, as_stream(stream), x, rs, (int)c, (long long)ld, vec_x, comps_hwc, mu_hwc, vec_w, (long long)n, d, (long long)k, p.kslab, part);
    else hipLaunchKernelGGL((route_partial_kernel<float, 1>), grid, block, 0, as_stream(stream), x, rs, (int)c, (long long)ld, vec_x, comps_hwc, mu_hwc, vec_w, (long long)n, d, (long long)k, p.kslab, part);
  }
  UNET_CHECK_LAUNCH(ctx, "cluster_route");
  hipLaunchKernelGGL(route_assign_kernel, dim3((unsigned)n), dim3(RA_THREADS), 0, as_stream(stream), part, p.slabs, (long long)n, (long long)k, centres, (int)nc,
                     proj, labels, dist);
  UNET_CHECK_LAUNCH(ctx, "cluster_route");
  return UNET_OK;
}

}  // extern "C"

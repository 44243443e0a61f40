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

}  // extern "C"

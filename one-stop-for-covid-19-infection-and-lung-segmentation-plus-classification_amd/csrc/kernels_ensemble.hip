// Several models (and one model under the square's eight symmetries) on one CT volume (volume.segment_volume_ensemble / vote_volume):
//   the symmetries of a slice batch and their inverses, a pure copy                                                        unet_vol_dihedral
//   the weighted mean of the members' canvases, every product, sum and the one division rounded on its own                 unet_vol_canvas_axpy, unet_vol_canvas_div
//   the mean probability in patient space: unet_vol_unslice's sampler (vol_sample.h) without the threshold                 unet_vol_unslice_prob
//   member m's mask as bit m of one 32-bit vote word per voxel                                                              unet_vol_vote_pack
//   vote words -> consensus mask, vote counts, per-slice counts, member volumes, the pair matrix, the vote histogram        unet_vol_vote_reduce
// Copies, integer sums and float32 operations that numpy performs one at a time: bit-exact against tests/ensemble_oracle.py, the same on every run.
// Compiled with -ffp-contract=off (csrc/Makefile), and the mean spells its roundings out (__fmul_rn, __fadd_rn, __fdiv_rn): no product is fused into a sum.
#include "common.h"
#include "vol_common.h"
#include "vol_sample.h"

namespace {
constexpr int TPB = 256;
typedef unsigned long long u64;

// ---- the eight symmetries of the square: dst[i][j] = src[si][sj] ---------------------------------------------------------------------------------
// codes 0, 2, 4, 5 keep rows as rows: si = (flip_i ? d - 1 - i : i), sj = (flip_j ? d - 1 - j : j): both sides run along a row (backwards at worst)
// codes 1, 3, 6, 7 transpose:         si = (flip_a ? d - 1 - j : j), sj = (flip_b ? d - 1 - i : i): through a 32 x 33 LDS tile, rows on both sides
//   rot90 [i][j] = m[j][d-1-i]   rot180 m[d-1-i][d-1-j]   rot270 m[d-1-j][i]   hflip m[i][d-1-j]   vflip m[d-1-i][j]   transpose m[j][i]   antitranspose m[d-1-j][d-1-i]
struct dih_map { int transposed, flip_a, flip_b; };
inline dih_map dih_code(int code) {
  switch (code) {
    case 0: return {0, 0, 0};
    case 1: return {1, 0, 1};
    case 2: return {0, 1, 1};
    case 3: return {1, 1, 0};
    case 4: return {0, 0, 1};
    case 5: return {0, 1, 0};
    case 6: return {1, 0, 0};
    default: return {1, 1, 1};
  }
}
__global__ __launch_bounds__(TPB) void dih_rows_kernel(const uint32_t* __restrict__ src, long long total, int d, int flip_i, int flip_j, uint32_t* __restrict__ dst) {
  const long long P = (long long)d * d;
  for (long long idx = (long long)blockIdx.x * TPB + threadIdx.x; idx < total; idx += (long long)gridDim.x * TPB) {
    const long long img = idx / P;
    const int r = (int)(idx - img * P);
    const int i = r / d, j = r - i * d;
    const int si = flip_i ? d - 1 - i : i, sj = flip_j ? d - 1 - j : j;
    dst[idx] = src[img * P + (long long)si * d + sj];
  }
}
constexpr int DIH_TILE = 32;
__global__ __launch_bounds__(TPB) void dih_transpose_kernel(const uint32_t* __restrict__ src, int n, int d, int flip_a, int flip_b, uint32_t* __restrict__ dst) {
  __shared__ uint32_t tile[DIH_TILE][DIH_TILE + 1];                  // + 1: the column reads below fall on 32 different banks
  const int tx = threadIdx.x & (DIH_TILE - 1), ty = threadIdx.x / DIH_TILE;          // 32 x 8
  const int i0 = blockIdx.y * DIH_TILE, j0 = blockIdx.x * DIH_TILE;                  // the destination tile: rows i0.., columns j0..
  const long long P = (long long)d * d;
  for (int img = blockIdx.z; img < n; img += gridDim.z) {
    // source row si belongs to destination column j, source column sj to destination row i: tile[j - j0][i - i0], read along sj
#pragma unroll
    for (int r = ty; r < DIH_TILE; r += TPB / DIH_TILE) {
      const int j = j0 + r, i = i0 + tx;
      if (i < d && j < d) {
        const int si = flip_a ? d - 1 - j : j, sj = flip_b ? d - 1 - i : i;
        tile[r][tx] = src[img * P + (long long)si * d + sj];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < DIH_TILE; r += TPB / DIH_TILE) {
      const int i = i0 + r, j = j0 + tx;
      if (i < d && j < d) dst[img * P + (long long)i * d + j] = tile[tx][r];
    }
    __syncthreads();
  }
}

// ---- the weighted mean of canvases: acc = first ? w c : acc + w c, then acc / wsum; one rounding per operation ------------------------------------
template <int V>
__global__ __launch_bounds__(TPB) void canvas_axpy_kernel(const float* __restrict__ c, float w, float* __restrict__ acc, long long count, int first) {
  for (long long q = ((long long)blockIdx.x * TPB + threadIdx.x) * V; q < count; q += (long long)gridDim.x * TPB * V) {
    if constexpr (V == 4) {
      const float4 x = *reinterpret_cast<const float4*>(c + q);
      float4 a = make_float4(__fmul_rn(w, x.x), __fmul_rn(w, x.y), __fmul_rn(w, x.z), __fmul_rn(w, x.w));
      if (!first) {
        const float4 o = *reinterpret_cast<const float4*>(acc + q);
        a = make_float4(__fadd_rn(o.x, a.x), __fadd_rn(o.y, a.y), __fadd_rn(o.z, a.z), __fadd_rn(o.w, a.w));
      }
      *reinterpret_cast<float4*>(acc + q) = a;
    } else {
      const float a = __fmul_rn(w, c[q]);
      acc[q] = first ? a : __fadd_rn(acc[q], a);
    }
  }
}
template <int V>
__global__ __launch_bounds__(TPB) void canvas_div_kernel(float* __restrict__ acc, float denom, long long count) {
  for (long long q = ((long long)blockIdx.x * TPB + threadIdx.x) * V; q < count; q += (long long)gridDim.x * TPB * V) {
    if constexpr (V == 4) {
      const float4 o = *reinterpret_cast<const float4*>(acc + q);
      *reinterpret_cast<float4*>(acc + q) = make_float4(__fdiv_rn(o.x, denom), __fdiv_rn(o.y, denom), __fdiv_rn(o.z, denom), __fdiv_rn(o.w, denom));
    } else {
      acc[q] = __fdiv_rn(acc[q], denom);
    }
  }
}

// ---- canvas -> the float32 probability of every voxel: vol_unslice_kernel without the comparison ---------------------------------------------------
template <int V>
__global__ __launch_bounds__(TPB) void vol_unslice_prob_kernel(const float* __restrict__ canvas, int S, int X, int Y, int z0, float* __restrict__ prob) {
  const int li = blockIdx.y;
  const float* p = canvas + (long long)li * S * S;
  const int XV = X / V;
  for (int q = blockIdx.x * TPB + threadIdx.x; q < XV * Y; q += gridDim.x * TPB) {
    const int y = q / XV, x0 = (q - y * XV) * V;
    float b[V];
#pragma unroll
    for (int k = 0; k < V; ++k) b[k] = vol_unslice_px(p, S, X, Y, x0 + k, y);
    float* dst = prob + ((long long)(z0 + li) * Y + y) * X + x0;
    if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = make_float4(b[0], b[1], b[2], b[3]);
    else dst[0] = b[0];
  }
}

// ---- votes ---------------------------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(TPB) void vote_pack_kernel(const uint8_t* __restrict__ mask, int member, int first, uint32_t* __restrict__ words, long long nvox) {
  for (long long q = ((long long)blockIdx.x * TPB + threadIdx.x) * V; q < nvox; q += (long long)gridDim.x * TPB * V) {
    if constexpr (V == 4) {
      const uchar4 m = *reinterpret_cast<const uchar4*>(mask + q);
      uint4 w = make_uint4((uint32_t)(m.x != 0) << member, (uint32_t)(m.y != 0) << member, (uint32_t)(m.z != 0) << member, (uint32_t)(m.w != 0) << member);
      if (!first) {
        const uint4 o = *reinterpret_cast<const uint4*>(words + q);
        w = make_uint4(o.x | w.x, o.y | w.y, o.z | w.z, o.w | w.w);
      }
      *reinterpret_cast<uint4*>(words + q) = w;
    } else {
      const uint32_t w = (uint32_t)(mask[q] != 0) << member;
      words[q] = first ? w : (words[q] | w);
    }
  }
}

// One lane per voxel, a wave never leaves its slice (blockIdx.y strides over z, blockIdx.x over the slice).  Everything a wave adds comes from ballots:
//   counts[z]     popcount of the ballot of the consensus bit; per wave in a register, per block and slice in LDS, one global atomic per block and slice
//   hist[k]       for every distinct vote count k in the wave, the popcount of the ballot of (votes == k)
//   pair[a][b]    for every bit a with a non-empty ballot and b >= a, the popcount of the ballot of (w >> a) & (w >> b) & 1; lane b keeps row a's entry b, so a row
//                 goes to LDS in one atomic instruction.  Only b >= a is kept; vote_finish_kernel mirrors it and copies the diagonal to member_voxels.
// A wave whose words are all zero writes its zeros and counts its lanes into hist[0]; nothing else.  LDS sums are int32 (a block sees fewer than 2^31 voxels);
// the flush is one 64-bit atomic per non-zero entry and block.
__global__ __launch_bounds__(TPB) void vote_reduce_kernel(const uint32_t* __restrict__ words, int M, int XY, int Z, int min_votes, uint8_t* __restrict__ mask,
                                                         uint8_t* __restrict__ votes, u64* __restrict__ counts, u64* __restrict__ pair, u64* __restrict__ hist) {
  __shared__ int s_pair[32 * 32];
  __shared__ int s_hist[33];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int k = tid; k < 32 * 32; k += TPB) s_pair[k] = 0;
  if (tid < 33) s_hist[tid] = 0;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const uint32_t low = M >= 32 ? 0xFFFFFFFFu : ((1u << M) - 1u);      // bits at or above M (a caller error) take no part
  int zeros = 0;                                                      // wave-uniform: voxels with no vote seen by this wave
  for (int z = blockIdx.y; z < Z; z += gridDim.y) {
    const long long zoff = (long long)z * XY;
    int cnt = 0;                                                      // wave-uniform: consensus voxels of this slice seen by this wave
    for (int base = blockIdx.x * TPB; base < XY; base += gridDim.x * TPB) {          // block-uniform bounds: every lane reaches every ballot
      const int q = base + tid;
      const bool valid = q < XY;
      const uint32_t w = valid ? (words[zoff + q] & low) : 0u;
      const u64 any = __ballot(w != 0u);
      if (any == 0ull) {
        if (valid) { mask[zoff + q] = 0; if (votes) votes[zoff + q] = 0; }
        zeros += __popcll(__ballot(valid));
        continue;
      }
      const int pc = __popc(w);
      const bool on = pc >= min_votes;
      if (valid) { mask[zoff + q] = on ? 1 : 0; if (votes) votes[zoff + q] = (uint8_t)pc; }
      cnt += __popcll(__ballot(on));
      zeros += __popcll(__ballot(valid && w == 0u));
      u64 rem = any;                                                  // the vote counts present in this wave, one ballot each
      while (rem) {
        const int k = __shfl(pc, __ffsll((long long)rem) - 1, 64);
        const u64 same = __ballot(w != 0u && pc == k);
        if (lane == 0) atomicAdd(&s_hist[k], __popcll(same));
        rem &= ~same;
      }
      for (int a = 0; a < M; ++a) {
        if (__ballot((w >> a) & 1u) == 0ull) continue;
        int v = 0;
        for (int b = a; b < M; ++b) {
          const int c = __popcll(__ballot((w >> a) & (w >> b) & 1u));
          if (lane == b) v = c;
        }
        if (v) atomicAdd(&s_pair[a * 32 + lane], v);                  // (v != 0 only on lanes a <= lane < M)
      }
    }
    if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0 && s_cnt) { atomicAdd(counts + z, (u64)s_cnt); s_cnt = 0; }
    __syncthreads();
  }
  if (lane == 0 && zeros) atomicAdd(&s_hist[0], zeros);
  __syncthreads();
  for (int k = tid; k < 32 * 32; k += TPB) {
    const int a = k >> 5, b = k & 31;
    if (s_pair[k] && b >= a && b < M) atomicAdd(pair + (long long)a * M + b, (u64)s_pair[k]);
  }
  if (tid <= M && s_hist[tid]) atomicAdd(hist + tid, (u64)s_hist[tid]);
}
__global__ void vote_finish_kernel(int M, u64* __restrict__ pair, u64* __restrict__ member_voxels) {
  const int k = threadIdx.x;                                          // one block of 32 x 32
  const int a = k >> 5, b = k & 31;
  if (a < M && b < M) {
    if (b < a) pair[a * M + b] = pair[b * M + a];
    if (a == b) member_voxels[a] = pair[a * M + a];
  }
}
}  // namespace

extern "C" {

int32_t unet_vol_dihedral(unet_ctx* ctx, const float* src, int32_t n, int32_t d, int32_t code, float* dst, void* stream) {
  if (!ctx) UNET_FAIL(ctx, UNET_E_ARG, "vol_dihedral: bad args");
  if (code < 0 || code > 7) UNET_FAIL(ctx, UNET_E_ARG, "vol_dihedral: code %d is not one of 0..7 (id, rot90, rot180, rot270, hflip, vflip, transpose, antitranspose)", code);
  if (n < 0 || d < 0 || (long long)d * d > 0x3FFFFFFFLL) UNET_FAIL(ctx, UNET_E_ARG, "vol_dihedral: %d slices of %d x %d are negative or too large", n, d, d);
  const long long total = (long long)n * d * d;
  if (total == 0) return UNET_OK;
  if (!src || !dst || !vol_aligned(src, 4) || !vol_aligned(dst, 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_dihedral: null or misaligned buffer");
  if (vol_overlap(src, (size_t)total * 4, dst, (size_t)total * 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_dihedral: dst must not be (or overlap) src");
  hipStream_t s = as_stream(stream);
  const dih_map m = dih_code(code);
  const uint32_t* in = reinterpret_cast<const uint32_t*>(src);
  uint32_t* out = reinterpret_cast<uint32_t*>(dst);
  if (!m.transposed) {
    hipLaunchKernelGGL(dih_rows_kernel, dim3(vol_blocks(total, 2048, TPB)), dim3(TPB), 0, s, in, total, d, m.flip_a, m.flip_b, out);
  } else {
    const unsigned tiles = (unsigned)((d + DIH_TILE - 1) / DIH_TILE);
    if (tiles > 65535u) UNET_FAIL(ctx, UNET_E_ARG, "vol_dihedral: %d x %d is too large for the transposing codes", d, d);
    hipLaunchKernelGGL(dih_transpose_kernel, dim3(tiles, tiles, (unsigned)(n < 1024 ? n : 1024)), dim3(TPB), 0, s, in, n, d, m.flip_a, m.flip_b, out);
  }
  UNET_CHECK_LAUNCH(ctx, "vol_dihedral"); return UNET_OK;
}

int32_t unet_vol_canvas_axpy(unet_ctx* ctx, const float* canvas, float w, float* acc, int64_t count, int32_t first, void* stream) {
  if (!ctx || count < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_canvas_axpy: bad args");
  if (count == 0) return UNET_OK;
  if (!canvas || !acc || !vol_aligned(canvas, 4) || !vol_aligned(acc, 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_canvas_axpy: null or misaligned buffer");
  if (vol_overlap(canvas, (size_t)count * 4, acc, (size_t)count * 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_canvas_axpy: acc must not be (or overlap) the canvas");
  hipStream_t s = as_stream(stream);
  if ((count % 4) == 0 && vol_aligned(canvas, 16) && vol_aligned(acc, 16))
    hipLaunchKernelGGL(canvas_axpy_kernel<4>, dim3(vol_blocks(count / 4, 2048, TPB)), dim3(TPB), 0, s, canvas, w, acc, (long long)count, first ? 1 : 0);
  else
    hipLaunchKernelGGL(canvas_axpy_kernel<1>, dim3(vol_blocks(count, 2048, TPB)), dim3(TPB), 0, s, canvas, w, acc, (long long)count, first ? 1 : 0);
  UNET_CHECK_LAUNCH(ctx, "vol_canvas_axpy"); return UNET_OK;
}

int32_t unet_vol_canvas_div(unet_ctx* ctx, float* acc, float denom, int64_t count, void* stream) {
  if (!ctx || count < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_canvas_div: bad args");
  if (count == 0) return UNET_OK;
  if (!acc || !vol_aligned(acc, 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_canvas_div: null or misaligned buffer");
  hipStream_t s = as_stream(stream);
  if ((count % 4) == 0 && vol_aligned(acc, 16)) hipLaunchKernelGGL(canvas_div_kernel<4>, dim3(vol_blocks(count / 4, 2048, TPB)), dim3(TPB), 0, s, acc, denom, (long long)count);
  else hipLaunchKernelGGL(canvas_div_kernel<1>, dim3(vol_blocks(count, 2048, TPB)), dim3(TPB), 0, s, acc, denom, (long long)count);
  UNET_CHECK_LAUNCH(ctx, "vol_canvas_div"); return UNET_OK;
}

int32_t unet_vol_unslice_prob(unet_ctx* ctx, const float* canvas, int32_t S, int32_t X, int32_t Y, int32_t Z, int32_t z0, int32_t z1, float* prob, void* stream) {
  if (!ctx) UNET_FAIL(ctx, UNET_E_ARG, "vol_unslice_prob: bad args");
  if (!vol_dims_ok_or_empty(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_unslice_prob: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  if (X == 0 || Y == 0 || Z == 0) return UNET_OK;
  if (!canvas || !prob || !vol_aligned(canvas, 4) || !vol_aligned(prob, 4) || S < 1 || (long long)S * S > 0x3FFFFFFFLL) UNET_FAIL(ctx, UNET_E_ARG, "vol_unslice_prob: bad args");
  if (z0 < 0 || z1 > Z || z1 <= z0) UNET_FAIL(ctx, UNET_E_ARG, "vol_unslice_prob: slice range [%d, %d) is empty or leaves the %d slices", z0, z1, Z);
  const int n = z1 - z0;
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(prob, 0, (size_t)X * Y * Z * sizeof(float), s));                   // the trimmed slices stay 0
  if ((X % 4) == 0 && vol_aligned(prob, 16)) hipLaunchKernelGGL(vol_unslice_prob_kernel<4>, dim3(vol_blocks((long long)(X / 4) * Y, 256, TPB), n), dim3(TPB), 0, s, canvas, S, X, Y, z0, prob);
  else hipLaunchKernelGGL(vol_unslice_prob_kernel<1>, dim3(vol_blocks((long long)X * Y, 1024, TPB), n), dim3(TPB), 0, s, canvas, S, X, Y, z0, prob);
  UNET_CHECK_LAUNCH(ctx, "vol_unslice_prob"); return UNET_OK;
}

int32_t unet_vol_vote_pack(unet_ctx* ctx, const uint8_t* mask, int32_t member, int32_t first, uint32_t* words, int64_t nvox, void* stream) {
  if (!ctx || nvox < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_pack: bad args");
  if (member < 0 || member > 31) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_pack: member %d is not one of 0..31", member);
  if (nvox == 0) return UNET_OK;
  if (!mask || !words || !vol_aligned(words, 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_pack: null or misaligned buffer");
  if (vol_overlap(mask, (size_t)nvox, words, (size_t)nvox * 4)) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_pack: the words must not overlap the mask");
  hipStream_t s = as_stream(stream);
  if ((nvox % 4) == 0 && vol_aligned(mask, 4) && vol_aligned(words, 16))
    hipLaunchKernelGGL(vote_pack_kernel<4>, dim3(vol_blocks(nvox / 4, 2048, TPB)), dim3(TPB), 0, s, mask, member, first ? 1 : 0, words, (long long)nvox);
  else
    hipLaunchKernelGGL(vote_pack_kernel<1>, dim3(vol_blocks(nvox, 2048, TPB)), dim3(TPB), 0, s, mask, member, first ? 1 : 0, words, (long long)nvox);
  UNET_CHECK_LAUNCH(ctx, "vol_vote_pack"); return UNET_OK;
}

int32_t unet_vol_vote_reduce(unet_ctx* ctx, const uint32_t* words, int32_t M, int32_t X, int32_t Y, int32_t Z, int32_t min_votes, uint8_t* mask, uint8_t* votes,
                             int64_t* counts, int64_t* member_voxels, int64_t* pair, int64_t* hist, void* stream) {
  if (!ctx) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_reduce: bad args");
  if (M < 1 || M > 32) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_reduce: %d members are outside 1..32", M);
  if (min_votes < 1 || min_votes > M) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_reduce: min_votes %d is outside 1..%d", min_votes, M);
  if (!vol_dims_ok_or_empty(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_reduce: %d x %d x %d is negative or has 2^31 voxels or more", X, Y, Z);
  const long long N = (long long)X * Y * Z;                         // (< 2^31: checked above)
  if (N == 0) return UNET_OK;
  if (!words || !mask || !counts || !member_voxels || !pair || !hist) UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_reduce: null buffer");
  if (!vol_aligned(words, 4) || !vol_aligned(counts, 8) || !vol_aligned(member_voxels, 8) || !vol_aligned(pair, 8) || !vol_aligned(hist, 8))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_reduce: misaligned buffer (words 4 bytes, the int64 outputs 8)");
  if (vol_overlap(words, (size_t)N * 4, mask, (size_t)N) || (votes && (vol_overlap(words, (size_t)N * 4, votes, (size_t)N) || vol_overlap(mask, (size_t)N, votes, (size_t)N))))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_vote_reduce: words, mask and votes must not overlap");
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)Z * sizeof(int64_t), s));
  UNET_HIP(ctx, hipMemsetAsync(pair, 0, (size_t)M * M * sizeof(int64_t), s));
  UNET_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)(M + 1) * sizeof(int64_t), s));
  const int XY = X * Y;
  const unsigned gx = vol_blocks(XY, 256, TPB);
  const unsigned gy_cap = 2048u / gx;                                 // at most 2048 workgroups: 8 per CU
  const unsigned gy = (unsigned)Z < gy_cap ? (unsigned)Z : gy_cap;
  hipLaunchKernelGGL(vote_reduce_kernel, dim3(gx, gy), dim3(TPB), 0, s, words, M, XY, Z, min_votes, mask, votes, reinterpret_cast<u64*>(counts), reinterpret_cast<u64*>(pair),
                     reinterpret_cast<u64*>(hist));
  hipLaunchKernelGGL(vote_finish_kernel, dim3(1), dim3(1024), 0, s, M, reinterpret_cast<u64*>(pair), reinterpret_cast<u64*>(member_voxels));
  UNET_CHECK_LAUNCH(ctx, "vol_vote_reduce"); return UNET_OK;
}

}  // extern "C"

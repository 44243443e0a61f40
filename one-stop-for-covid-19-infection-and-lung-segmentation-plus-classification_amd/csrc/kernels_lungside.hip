// Left and right lung: the per-voxel assignment of a lung mask to the nearer of two seeds, and the per-side tables of an infection mask.
//   sides[v] = 0 off the mask, else the side of the seed with the smaller squared distance (a tie: the seed whose side is 1), + voxels per side value     unet_vol_side_assign
//   voxels per side value, infected voxels per side value, voxels of every lesion per side value, the same per slice                                    unet_vol_side_table
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, as in kernels_components.hip.
// Integer arithmetic only.  The distances are compared as order-preserving 64-bit keys of their bit patterns (vol_common.h's vol_d2ord on the bits): for the non-negative
// values and +inf that unet_vol_edt_sq writes, key order is value order, and no floating-point instruction runs.  Sums are integers per lane, per wave (ballots /
// butterflies), per workgroup in LDS, and leave as 64-bit atomics: the same bits on every run.
// Assign: a lane holds four consecutive voxels -- one 4-byte load of the mask, two 16-byte loads of each distance stream, one 4-byte store -- when the buffers are
// aligned for it, one voxel otherwise.  A wave whose mask bytes are all zero never reads a distance.
// Table: kernels_intensity.hip's layout -- chunk c = ST_CHUNK voxels of one slice, a workgroup walks a contiguous range of chunks, the per-slice counters leave LDS when
// its slice changes -- and its ballot-per-key loop for the (lesion, side) table: one add per distinct key of a wave.
#include "common.h"
#include "vol_common.h"

namespace {
constexpr int TPB = 256;
constexpr long long GRID_CAP = 256 * 32;
constexpr int ST_TABLE = 4096;                                       // (lesion, side) counters of a workgroup's LDS table (16 KiB): 3 n <= ST_TABLE
constexpr int ST_CHUNK = TPB * 16;                                   // voxels of a slice a workgroup takes at a time
constexpr int ST_GRID = 256 * 4;                                     // workgroups of the table launch

__device__ __forceinline__ unsigned long long ls_key(unsigned long long u) { return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
// the side of a mask voxel: `first` (the seed whose side is 1) wins a tie
__device__ __forceinline__ int ls_side(unsigned long long a, unsigned long long b, int side_a, int side_b) {
  const unsigned long long ka = ls_key(a), kb = ls_key(b);
  return side_a == 1 ? (ka <= kb ? side_a : side_b) : (kb <= ka ? side_b : side_a);
}
// VEC = 4: item g = voxels [4 g, 4 g + 4) (the last item may be short: it goes voxel by voxel); VEC = 1: item g = voxel g.  Trip counts are wave-uniform.
template <int VEC>
__global__ __launch_bounds__(TPB) void side_assign_kernel(const uint8_t* __restrict__ mask, const unsigned long long* __restrict__ d2a, const unsigned long long* __restrict__ d2b,
                                                         long long N, int side_a, int side_b, uint8_t* __restrict__ sides, unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[TPB / 64][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long items = (N + VEC - 1) / VEC;
  int c1 = 0, c2 = 0, c0 = 0;
  for (long long g0 = (long long)blockIdx.x * TPB + (tid - lane); g0 < items; g0 += (long long)gridDim.x * TPB) {
    const long long g = g0 + lane, v0 = g * VEC;
    if constexpr (VEC == 4) {
      const bool full = v0 + 4 <= N;
      unsigned m = 0;
      if (full) m = *reinterpret_cast<const unsigned*>(mask + v0);
      else for (int k = 0; k < 4; ++k) if (v0 + k < N) m |= (unsigned)mask[v0 + k] << (8 * k);
      unsigned out = 0;
      if (__ballot(m != 0)) {                                         // wave-uniform: a wave off the mask reads no distance
        if (m != 0) {
          unsigned long long a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
          if (full) {
            const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(d2a + v0), a23 = *reinterpret_cast<const ulonglong2*>(d2a + v0 + 2);
            const ulonglong2 b01 = *reinterpret_cast<const ulonglong2*>(d2b + v0), b23 = *reinterpret_cast<const ulonglong2*>(d2b + v0 + 2);
            a[0] = a01.x; a[1] = a01.y; a[2] = a23.x; a[3] = a23.y;
            b[0] = b01.x; b[1] = b01.y; b[2] = b23.x; b[3] = b23.y;
          } else {
            for (int k = 0; k < 4; ++k) if (v0 + k < N) { a[k] = d2a[v0 + k]; b[k] = d2b[v0 + k]; }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if ((m >> (8 * k)) & 0xFFu) {
              const int sd = ls_side(a[k], b[k], side_a, side_b);
              out |= (unsigned)sd << (8 * k);
              c1 += sd == 1; c2 += sd == 2;
            }
        }
      }
      if (full) { *reinterpret_cast<unsigned*>(sides + v0) = out; c0 += 4; }
      else for (int k = 0; k < 4; ++k) if (v0 + k < N) { sides[v0 + k] = (uint8_t)((out >> (8 * k)) & 0xFFu); c0 += 1; }
    } else {
      const bool in = g < N;
      const unsigned m = in ? mask[g] : 0u;
      int sd = 0;
      if (__ballot(m != 0)) {
        if (m != 0) { sd = ls_side(d2a[g], d2b[g], side_a, side_b); c1 += sd == 1; c2 += sd == 2; }
      }
      if (in) { sides[g] = (uint8_t)sd; c0 += 1; }
    }
  }
  c0 -= c1 + c2;                                                      // c0 counted every voxel written
  c0 = vol_wave_sum(c0); c1 = vol_wave_sum(c1); c2 = vol_wave_sum(c2);
  if (lane == 0) { s_cnt[wave][0] = c0; s_cnt[wave][1] = c1; s_cnt[wave][2] = c2; }
  __syncthreads();
  if (tid < 3) {
    long long t = 0;
    for (int w = 0; w < TPB / 64; ++w) t += s_cnt[w][tid];
    if (t) atomicAdd(counts + tid, (unsigned long long)t);
  }
}

// s_slice / s_tot: {lung L, lung R, infected outside, infected L, infected R, side 0} of the current slice / of everything this workgroup saw.
// Every loop bound and every barrier below is uniform over the workgroup.
template <bool LDS_TABLE>
__global__ __launch_bounds__(TPB) void side_table_kernel(const uint8_t* __restrict__ sides, const uint8_t* __restrict__ infection, const int32_t* __restrict__ labels, int n,
                                                        long long XY, int Z, int cps, long long per, unsigned long long* __restrict__ totals,
                                                        unsigned long long* __restrict__ lesion_side, unsigned long long* __restrict__ per_slice) {
  __shared__ int s_tab[LDS_TABLE ? ST_TABLE : 1];
  __shared__ int s_slice[6];
  __shared__ long long s_tot[6];
  const int tid = threadIdx.x, lane = tid & 63;
  const bool want_les = labels != nullptr && n > 0;
  if constexpr (LDS_TABLE) for (int i = tid; i < 3 * n; i += TPB) s_tab[i] = 0;
  if (tid < 6) { s_slice[tid] = 0; s_tot[tid] = 0; }
  __syncthreads();
  const long long chunks = (long long)cps * Z;
  const long long c0 = (long long)blockIdx.x * per, c1 = min(chunks, c0 + per);
  for (long long c = c0; c < c1; ++c) {
    const int z = (int)(c / cps);
    const long long i0 = (c - (long long)z * cps) * ST_CHUNK, base = (long long)z * XY;
    for (int k = 0; k < ST_CHUNK / TPB; ++k) {
      const long long i = i0 + (long long)k * TPB + tid;
      const bool in = i < XY;
      int sd = 0, inf = 0, l = 0;
      if (in) {
        sd = sides[base + i];
        if (sd > 2) sd = 0;                                           // a value above 2 counts as 0
        inf = infection ? (infection[base + i] != 0) : 0;
        if (want_les) { l = labels[base + i]; l = (unsigned)(l - 1) < (unsigned)n ? l : 0; }
      }
      const unsigned long long bin = __ballot(in);
      if (!bin) continue;
      const unsigned long long b1 = __ballot(sd == 1), b2 = __ballot(sd == 2), bi = __ballot(inf != 0);
      unsigned long long pending = __ballot(l != 0);
      if (lane == 0) {
        const int n1 = (int)__popcll(b1), n2 = (int)__popcll(b2);
        const int v[6] = {n1, n2, (int)__popcll(bi & ~(b1 | b2)), (int)__popcll(bi & b1), (int)__popcll(bi & b2), (int)__popcll(bin) - n1 - n2};
#pragma unroll
        for (int q = 0; q < 6; ++q) if (v[q]) atomicAdd(s_slice + q, v[q]);
      }
      const long long key = l ? (long long)(l - 1) * 3 + sd : -1;     // 3 n may pass 2^31 beyond the LDS table
      while (pending) {                                               // one round per distinct key of the wave
        const int leader = __ffsll((long long)pending) - 1;
        const long long K = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == K);
        if (lane == leader) {
          const int cnt = __popcll(same);
          if constexpr (LDS_TABLE) atomicAdd(s_tab + K, cnt);
          else atomicAdd(lesion_side + K, (unsigned long long)cnt);
        }
        pending &= ~same;
      }
    }
    if (c + 1 == c1 || (int)((c + 1) / cps) != z) {                   // the slice ends here for this workgroup
      __syncthreads();
      if (tid < 6) {
        const int v = s_slice[tid];
        if (v && per_slice && tid < 5) atomicAdd(per_slice + (long long)z * 6 + tid, (unsigned long long)v);
        s_tot[tid] += v;
        s_slice[tid] = 0;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid < 6) {                                                      // totals [2][3]: row 0 = sides by value, row 1 = infected by the side under them
    const int slot[6] = {1, 2, 3, 4, 5, 0};
    const long long v = s_tot[tid];
    if (v) atomicAdd(totals + slot[tid], (unsigned long long)v);
  }
  if constexpr (LDS_TABLE)
    for (int i = tid; i < 3 * n; i += TPB) { const int v = s_tab[i]; if (v) atomicAdd(lesion_side + i, (unsigned long long)v); }
}
}  // namespace

extern "C" {

int32_t unet_vol_side_assign(unet_ctx* ctx, const uint8_t* mask, const double* d2_a, const double* d2_b, int32_t X, int32_t Y, int32_t Z, int32_t side_a, int32_t side_b,
                             uint8_t* sides, int64_t* counts, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_side_assign: a dimension is negative or the volume has 2^31 voxels or more");
  if (!((side_a == 1 && side_b == 2) || (side_a == 2 && side_b == 1))) UNET_FAIL(ctx, UNET_E_ARG, "vol_side_assign: side_a, side_b are 1 and 2 in either order, not %d, %d", side_a, side_b);
  const long long N = (long long)X * Y * Z;
  if (N == 0) return UNET_OK;
  if (!mask || !d2_a || !d2_b || !sides || !counts || !vol_aligned(d2_a, 8) || !vol_aligned(d2_b, 8) || !vol_aligned(counts, 8))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_side_assign: null or misaligned buffer");
  if (sides == mask) UNET_FAIL(ctx, UNET_E_ARG, "vol_side_assign: sides must not be the mask's own buffer");
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s));
  const unsigned long long* a = reinterpret_cast<const unsigned long long*>(d2_a);
  const unsigned long long* b = reinterpret_cast<const unsigned long long*>(d2_b);
  unsigned long long* cn = reinterpret_cast<unsigned long long*>(counts);
  const bool vec = vol_aligned(mask, 4) && vol_aligned(sides, 4) && vol_aligned(d2_a, 16) && vol_aligned(d2_b, 16);
  const long long items = vec ? (N + 3) / 4 : N;
  long long blocks = (items + TPB - 1) / TPB;
  if (blocks > GRID_CAP) blocks = GRID_CAP;
  if (vec) hipLaunchKernelGGL(side_assign_kernel<4>, dim3((unsigned)blocks), dim3(TPB), 0, s, mask, a, b, N, side_a, side_b, sides, cn);
  else hipLaunchKernelGGL(side_assign_kernel<1>, dim3((unsigned)blocks), dim3(TPB), 0, s, mask, a, b, N, side_a, side_b, sides, cn);
  UNET_CHECK_LAUNCH(ctx, "vol_side_assign"); return UNET_OK;
}

int32_t unet_vol_side_table(unet_ctx* ctx, const uint8_t* sides, const uint8_t* infection, const int32_t* labels, int32_t n, int32_t X, int32_t Y, int32_t Z, int64_t* totals,
                            int64_t* lesion_side, int64_t* per_slice, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_side_table: a dimension is negative or the volume has 2^31 voxels or more");
  if (n < 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_side_table: n is negative");
  const long long XY = (long long)X * Y, N = XY * Z;
  if (N == 0) return UNET_OK;
  if (!sides || !totals || (n > 0 && !lesion_side) || !vol_aligned(totals, 8) || !vol_aligned(lesion_side, 8) || !vol_aligned(per_slice, 8) || !vol_aligned(labels, 4))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_side_table: null or misaligned buffer");
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(totals, 0, 6 * sizeof(int64_t), s));
  if (n > 0) UNET_HIP(ctx, hipMemsetAsync(lesion_side, 0, (size_t)n * 3 * sizeof(int64_t), s));
  if (per_slice) UNET_HIP(ctx, hipMemsetAsync(per_slice, 0, (size_t)Z * 6 * sizeof(int64_t), s));
  const int cps = (int)((XY + ST_CHUNK - 1) / ST_CHUNK);
  const long long chunks = (long long)cps * Z;
  const long long per = (chunks + ST_GRID - 1) / ST_GRID;
  const unsigned grid = (unsigned)((chunks + per - 1) / per);
  unsigned long long* tt = reinterpret_cast<unsigned long long*>(totals);
  unsigned long long* ls = reinterpret_cast<unsigned long long*>(lesion_side);
  unsigned long long* ps = reinterpret_cast<unsigned long long*>(per_slice);
  if ((long long)n * 3 <= ST_TABLE) hipLaunchKernelGGL(side_table_kernel<true>, dim3(grid), dim3(TPB), 0, s, sides, infection, labels, n, XY, Z, cps, per, tt, ls, ps);
  else hipLaunchKernelGGL(side_table_kernel<false>, dim3(grid), dim3(TPB), 0, s, sides, infection, labels, n, XY, Z, cps, per, tt, ls, ps);
  UNET_CHECK_LAUNCH(ctx, "vol_side_table"); return UNET_OK;
}

}  // extern "C"

// Rank filters of a CT volume: dst[v] = the element of rank `rank` among src[v + o], o in a footprint of radius R <= 2      unet_vol_rank_filter
// Median, minimum, maximum, percentile and flat grey erosion / dilation are all this one selection.  A rank filter selects and never computes: the stored bits of the
// selected element leave unchanged, no float arithmetic happens anywhere, and the result equals scipy.ndimage.rank_filter element for element.
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31.  Elements are ordered by a 32-bit key: an unsigned integer is its own key, a signed one
// has its sign bit flipped, a float32 is bits ^ (sign ? 0xFFFFFFFF : 0x80000000) -- NaNs with the sign bit lowest, -inf .. -0 < +0 .. +inf, the other NaNs highest.
// Persistent workgroups of 256 lanes walk bricks of 32 x 8 x 8 voxels, x fastest.  A brick is staged in LDS with a halo of R on all sides, already as keys and with the
// border mode applied while staging (the edge voxel, the constant, or scipy's reflect), so the selection knows no border and a global element is read about once:
// 36 x 12 x 12 keys = 20.25 KiB at R = 2, 34 x 10 x 10 = 13.3 KiB at R = 1.  The 32 lanes of a half-wave read 32 consecutive keys of one staged row: no bank conflict.
// Selection, per voxel: one pass over the n keys of the footprint gives the smallest and the largest key -- ranks 0 and n - 1 end there, and so does a voxel whose
// footprint holds one value.  Every other rank is a bisection over the key's bits: the answer is the largest value c with #{key < c} <= rank, found one bit at a time
// from the highest bit in which the smallest and the largest key differ (all keys agree above it), each bit one count over the n staged keys: at most 8, 16 or 32
// rounds by the element's width, and as few as the local range of the CT needs.  A footprint of up to 27 keys is read into registers once and counted there (twice as
// fast at the 27-box median as re-reading the brick every round); larger footprints, and the end ranks, which read every key once anyway, count from the staged brick.
// One launch, no atomics, no workgroup waits for another, every voxel written by one lane: the same bits on every run.
#include "common.h"
#include "vol_common.h"

namespace {
constexpr int TPB = 256;
constexpr int MAX_R = UNET_VOL_RANK_MAX_RADIUS;
constexpr int MAX_N = (2 * MAX_R + 1) * (2 * MAX_R + 1) * (2 * MAX_R + 1);          // 125 offsets at the most
constexpr int BX = 32, BY = 8, BZ = 8, BRICK = BX * BY * BZ;         // the brick a workgroup takes at a time: 8 voxels per lane
constexpr long long GRID_CAP = 256 * 8;                              // persistent workgroups of a launch: 8 per CU are resident at R = 1 (32 waves, 13.3 KiB of LDS each), 7 at R = 2 (20.25 KiB each)
constexpr int REG_SMALL = 8, REG_LARGE = 27;                         // footprints of up to this many keys are bisected in registers (the 7-voxel cross; the 19 and the 27-box)
static_assert(MAX_R == 2, "the staged brick and the footprint word are laid out for R <= 2");

// the footprint of a launch: n offsets into the staged brick, relative to a voxel's own key, in ascending bit order
struct rf_offsets { int n; int off[MAX_N]; };

template <int EB> struct rf_elem;
template <> struct rf_elem<1> { using type = uint8_t; };
template <> struct rf_elem<2> { using type = uint16_t; };
template <> struct rf_elem<4> { using type = uint32_t; };

inline int rf_itemsize(int dt) { return dt == 64 ? 0 : vol_itemsize(dt); }          // (float64 is refused: the keys are 32 bits)
inline uint32_t rf_flip(int dt) { return dt == 256 ? 0x80u : dt == 4 ? 0x8000u : dt == 8 ? 0x80000000u : 0u; }
// stored bits <-> key (flip: the sign bit of a signed integer type, 0 for an unsigned one)
__host__ __device__ __forceinline__ uint32_t rf_key(uint32_t raw, uint32_t flip, int is_float) {
  return is_float ? raw ^ ((raw >> 31) ? 0xFFFFFFFFu : 0x80000000u) : raw ^ flip;
}
__host__ __device__ __forceinline__ uint32_t rf_unkey(uint32_t key, uint32_t flip, int is_float) {
  return is_float ? key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu) : key ^ flip;
}
// coordinate g of an axis of n voxels -> the voxel read there, or -1 for the constant
__device__ __forceinline__ int rf_border(long long g, int n, int mode) {
  if (g >= 0 && g < n) return (int)g;
  if (mode == UNET_FILTER_NEAREST) return g < 0 ? 0 : n - 1;
  if (mode == UNET_FILTER_CONSTANT) return -1;
  const long long m = 2LL * n;                                        // reflect: (d c b a | a b c d | d c b a), period 2 n -- any distance, so extents 1 and 2 under R = 2 too
  long long p = g % m;
  if (p < 0) p += m;
  return (int)(p >= n ? m - 1 - p : p);
}

// The key of rank `rank` among keys that all lie in lo .. hi, lo < hi: the largest c with #{key < c} <= rank, one bit at a time from the highest bit in which lo and hi
// differ (all keys agree above it, and lo has a 0 there).  below(c) counts the keys under c.
template <class Below>
__device__ __forceinline__ uint32_t rf_bisect(uint32_t lo, uint32_t hi, int rank, Below below) {
  const int hb = 31 - __clz((int)(lo ^ hi));
  uint32_t res = lo & ~((2u << hb) - 1u);                             // (hb = 31: 2u << 31 = 0, the mask is all ones, res = 0)
  for (int bit = hb; bit >= 0; --bit) {
    const uint32_t cand = res | (1u << bit);
    if (below(cand) <= rank) res = cand;
  }
  return res;
}

// NREG > 0: the footprint's n <= NREG keys are read into registers once and every round counts there; NREG = 0: every round re-reads them from the staged brick.
// Every loop bound that holds a barrier is uniform over the workgroup: the brick loop and the staging loop.  The selection holds none, so its lanes may differ in rounds.
template <int R, int EB, int NREG>
__global__ __launch_bounds__(TPB) void rf_rank_kernel(const void* __restrict__ src, void* __restrict__ dst, int X, int Y, int Z, rf_offsets fp, int rank, int mode,
                                                     uint32_t cval_key, uint32_t flip, int is_float, long long nbricks, int nbx, int nby) {
  constexpr int SX = BX + 2 * R, SY = BY + 2 * R, SZ = BZ + 2 * R, S = SX * SY * SZ;
  using T = typename rf_elem<EB>::type;
  __shared__ uint32_t s_key[S];
  const T* __restrict__ in = static_cast<const T*>(src);
  T* __restrict__ out = static_cast<T*>(dst);
  const int tid = threadIdx.x, n = fp.n;
  for (long long b = blockIdx.x; b < nbricks; b += gridDim.x) {
    const int bz = (int)(b / ((long long)nbx * nby)), br = (int)(b - (long long)bz * nbx * nby), by = br / nbx, bx = br - by * nbx;
    const int x0 = bx * BX, y0 = by * BY, z0 = bz * BZ;
    for (int i = tid; i < S; i += TPB) {                              // the brick and its halo as keys, the border applied here
      const int sx = i % SX, t = i / SX, sy = t % SY, sz = t / SY;
      const int px = rf_border((long long)x0 + sx - R, X, mode), py = rf_border((long long)y0 + sy - R, Y, mode), pz = rf_border((long long)z0 + sz - R, Z, mode);
      uint32_t k = cval_key;
      if ((px | py | pz) >= 0) k = rf_key((uint32_t)in[px + (long long)X * (py + (long long)Y * pz)], flip, is_float);          // (0 <= p < extent on every axis)
      s_key[i] = k;
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < BRICK / TPB; ++j) {
      const int l = tid + j * TPB, lx = l & (BX - 1), ly = (l >> 5) & (BY - 1), lz = l >> 8;
      const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
      if (gx < X && gy < Y && gz < Z) {
        const int c = (lx + R) + SX * ((ly + R) + SY * (lz + R));     // c + off stays inside the staged brick: |dx|, |dy|, |dz| <= R
        uint32_t res;
        if constexpr (NREG > 0) {
          uint32_t key[NREG];                                         // padded with the largest key, which is never below a candidate (off[k] = 0 for k >= n: the voxel's own key is read)
#pragma unroll
          for (int k = 0; k < NREG; ++k) { const uint32_t v = s_key[c + fp.off[k]]; key[k] = k < n ? v : 0xFFFFFFFFu; }
          uint32_t lo = key[0], hi = key[0];
#pragma unroll
          for (int k = 1; k < NREG; ++k) { lo = key[k] < lo ? key[k] : lo; hi = (k < n && key[k] > hi) ? key[k] : hi; }
          res = rank == 0 ? lo : hi;
          if (rank != 0 && rank != n - 1 && lo != hi)
            res = rf_bisect(lo, hi, rank, [&](uint32_t cand) {
              int below = 0;
#pragma unroll
              for (int k = 0; k < NREG; ++k) below += key[k] < cand ? 1 : 0;
              return below;
            });
        } else {
          uint32_t lo = 0xFFFFFFFFu, hi = 0u;
          for (int k = 0; k < n; ++k) {
            const uint32_t v = s_key[c + fp.off[k]];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
          }
          res = rank == 0 ? lo : hi;
          if (rank != 0 && rank != n - 1 && lo != hi)
            res = rf_bisect(lo, hi, rank, [&](uint32_t cand) {
              int below = 0;
              for (int k = 0; k < n; ++k) below += s_key[c + fp.off[k]] < cand ? 1 : 0;
              return below;
            });
        }
        out[gx + (long long)X * (gy + (long long)Y * gz)] = (T)rf_unkey(res, flip, is_float);
      }
    }
    __syncthreads();                                                  // the staged brick was read: the next one may be written
  }
}

template <int R, int EB, int NREG>
void rf_launch_n(hipStream_t s, unsigned grid, const void* src, void* dst, int X, int Y, int Z, const rf_offsets& fp, int rank, int mode, uint32_t cval_key, uint32_t flip,
                 int is_float, long long nbricks, int nbx, int nby) {
  hipLaunchKernelGGL((rf_rank_kernel<R, EB, NREG>), dim3(grid), dim3(TPB), 0, s, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
}
// Which selection a launch takes, from its footprint and rank.  An end rank reads every key once whatever holds it, and beyond REG_LARGE keys the registers run out:
// the staged brick serves both.  A rank in between re-reads its keys once per bit: up to REG_SMALL or REG_LARGE keys go to registers (measured: DESIGN.md section 4ad).
template <int R, int EB>
void rf_launch(hipStream_t s, unsigned grid, const void* src, void* dst, int X, int Y, int Z, const rf_offsets& fp, int rank, int mode, uint32_t cval_key, uint32_t flip,
               int is_float, long long nbricks, int nbx, int nby) {
  const bool end_rank = rank == 0 || rank == fp.n - 1;
  if (end_rank || fp.n > REG_LARGE) rf_launch_n<R, EB, 0>(s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
  else if (fp.n <= REG_SMALL) rf_launch_n<R, EB, REG_SMALL>(s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
  else rf_launch_n<R, EB, REG_LARGE>(s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
}
template <int R>
void rf_launch_r(int eb, hipStream_t s, unsigned grid, const void* src, void* dst, int X, int Y, int Z, const rf_offsets& fp, int rank, int mode, uint32_t cval_key,
                 uint32_t flip, int is_float, long long nbricks, int nbx, int nby) {
  if (eb == 1) rf_launch<R, 1>(s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
  else if (eb == 2) rf_launch<R, 2>(s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
  else rf_launch<R, 4>(s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
}
}  // namespace

extern "C" {

int32_t unet_vol_rank_filter(unet_ctx* ctx, const void* src, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t R, uint64_t fp_lo, uint64_t fp_hi, int32_t rank,
                             int32_t mode, uint64_t cval_bits, void* dst, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: a dimension is negative or the volume has 2^31 voxels or more");
  const int eb = rf_itemsize(dtype);
  if (eb == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: the NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16 (64 is not taken: ask for float32)");
  if (R < 1 || R > MAX_R) UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: the radius lies in 1 .. %d, not %d", MAX_R, R);
  const int side = 2 * R + 1, cube = side * side * side;             // 27 or 125 bits
  if (cube < 64 ? (fp_hi != 0 || (fp_lo >> cube) != 0) : (fp_hi >> (cube - 64)) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: the footprint has a bit at or above (2 R + 1)^3 = %d", cube);
  const int n = __builtin_popcountll(fp_lo) + __builtin_popcountll(fp_hi);
  if (n < 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: the footprint is empty");
  if (rank < 0 || rank >= n) UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: the rank lies in 0 .. %d (the footprint's voxels less one), not %d", n - 1, rank);
  if (mode != UNET_FILTER_NEAREST && mode != UNET_FILTER_CONSTANT && mode != UNET_FILTER_REFLECT)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: mode is 0 (nearest), 1 (constant) or 2 (reflect), not %d", mode);
  if ((cval_bits >> (8 * eb)) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: cval_bits holds more than the %d bytes of an element", eb);
  const long long N = (long long)X * Y * Z;
  if (N == 0) return UNET_OK;
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst), bytes = (uintptr_t)N * eb;
  if (!src || !dst || a % eb != 0 || d % eb != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: null buffer, or a buffer not aligned to its element");
  if (a < d + bytes && d < a + bytes) UNET_FAIL(ctx, UNET_E_ARG, "vol_rank_filter: src and dst overlap (a voxel's neighbours must be read as they were)");
  const int SX = BX + 2 * R, SY = BY + 2 * R;
  rf_offsets fp{};
  for (int bit = 0; bit < cube; ++bit)
    if (((bit < 64 ? fp_lo >> bit : fp_hi >> (bit - 64)) & 1) != 0) {
      const int dx = bit % side - R, dy = (bit / side) % side - R, dz = bit / (side * side) - R;
      fp.off[fp.n++] = dx + SX * (dy + SY * dz);
    }
  const int is_float = dtype == 16 ? 1 : 0;
  const uint32_t flip = rf_flip(dtype), cval_key = rf_key((uint32_t)cval_bits, flip, is_float);
  const int nbx = (X + BX - 1) / BX, nby = (Y + BY - 1) / BY, nbz = (Z + BZ - 1) / BZ;
  const long long nbricks = (long long)nbx * nby * nbz;
  const unsigned grid = (unsigned)(nbricks < GRID_CAP ? nbricks : GRID_CAP);
  hipStream_t s = as_stream(stream);
  if (R == 1) rf_launch_r<1>(eb, s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
  else rf_launch_r<2>(eb, s, grid, src, dst, X, Y, Z, fp, rank, mode, cval_key, flip, is_float, nbricks, nbx, nby);
  UNET_CHECK_LAUNCH(ctx, "vol_rank_filter"); return UNET_OK;
}

}  // extern "C"

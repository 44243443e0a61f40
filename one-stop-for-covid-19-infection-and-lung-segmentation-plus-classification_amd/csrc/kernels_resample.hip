// A volume put onto another grid: spacing, shape, an oblique affine, a signed axis permutation.
//   elements of 1, 2, 4 or 8 bytes moved untouched from the nearest source voxel                                       unet_vol_resample_nearest
//   the decoded voxels (vol_common.h's vol_dec) blended trilinearly -> float64 / float32 / a uint8 mask      unet_vol_resample_linear
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31 on both sides.  M (12 doubles, row-major 3 x 4, in the kernel arguments) maps an output
// voxel index to a source voxel coordinate: s_r = ((M[r][0] i + M[r][1] j) + M[r][2] k) + M[r][3], every operation a rounded float64 one (-ffp-contract=off and the
// __d*_rn forms: numpy restates them bit for bit).  A coordinate becomes an integer only after it was found inside [-1, n] as a double: |s| = 1e300 or a NaN (inf - inf
// of an overflowing M) never reaches a conversion.
// One lane per output voxel, and ONE per-voxel function (rs_near / rs_lin) under two lane-to-voxel mappings, so the mapping never changes a bit of the result:
//   rs_direct_kernel   x along the lanes; a bounded grid strides the output.  Taken when source x depends most on output x (the largest |M[0][c]| is c = 0): a wave's
//                      loads run along source x, forwards or backwards, and its stores are one run.
//   rs_tiled_kernel    source x depends most on output axis a = 1 or 2, at least TILED_MIN voxels long (an axis permutation, a rotation past 45 degrees): a workgroup owns 64 x 64 outputs (x, a) of one
//                      plane; its waves first put `a` along the lanes -- the loads run along source x --, leave the values in LDS, and then store them with x along the
//                      lanes.  Both sides of a wave are runs of consecutive elements; the tile's row pitch is an odd number of dwords (8-byte elements: 130 dwords, which
//                      ds_read_b64's 64 banks also take without a conflict).
// A lane whose neighbours all lie outside (mode 1) loads nothing, so a wave of such lanes issues no load.  No atomics, no scratch buffers, plain vector stores.
#include "common.h"
#include "vol_trilinear.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int TILE = 64;
constexpr long long GRID_CAP = 256 * 32;

struct rs_geom { rs_mat M; int X, Y, Z, mode; };

// ---- nearest and linear: the coordinate and both samplers are vol_trilinear.h's, the decode vol_common.h's (shared with kernels_register.hip and kernels_deform.hip) --------
template <typename T>
struct rs_near {
  rs_geom g; const T* src; T cval;
  __device__ __forceinline__ T operator()(int i, int j, int k) const {
    const double s[3] = {rs_coord(g.M, 0, i, j, k), rs_coord(g.M, 1, i, j, k), rs_coord(g.M, 2, i, j, k)};
    return rs_nearest_at<T>(src, g.X, g.Y, g.Z, g.mode, cval, s);
  }
};

template <typename D>
struct rs_lin {
  rs_geom g; vol_voxels src; double cval;
  __device__ __forceinline__ D operator()(int i, int j, int k) const {
    const double s[3] = {rs_coord(g.M, 0, i, j, k), rs_coord(g.M, 1, i, j, k), rs_coord(g.M, 2, i, j, k)};
    return rs_store<D>(rs_linear_at(src, g.X, g.Y, g.Z, g.mode, cval, s));
  }
};

// ---- the two mappings ------------------------------------------------------------------------------------------------------------------------------------
template <typename T, typename Op>
__global__ __launch_bounds__(TPB) void rs_direct_kernel(Op op, T* __restrict__ dst, int X2, int Y2, int Z2) {
  const long long outs = (long long)X2 * Y2 * Z2;
  for (long long o = (long long)blockIdx.x * TPB + threadIdx.x; o < outs; o += (long long)gridDim.x * TPB) {
    const long long c = o / X2;
    const int i = (int)(o - c * X2), k = (int)(c / Y2), j = (int)(c - (long long)k * Y2);
    dst[o] = op(i, j, k);
  }
}

// tile t = (bx, ba, b): outputs x in [64 bx, 64 bx + 64), axis a in [64 ba, 64 ba + 64), the third axis at b.  The trip count and both barriers are uniform over the workgroup.
template <typename T, typename Op>
__global__ __launch_bounds__(TPB) void rs_tiled_kernel(Op op, T* __restrict__ dst, int X2, int Y2, int Z2, int a, int tx, int ta, long long tiles) {
  constexpr int PAD = sizeof(T) >= 4 ? 1 : 4 / (int)sizeof(T);
  __shared__ T tile[TILE][TILE + PAD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nA = a == 1 ? Y2 : Z2;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int bx = (int)(t % tx);
    const long long rest = t / tx;
    const int ba = (int)(rest % ta), b = (int)(rest / ta);
    const int x0 = bx * TILE, a0 = ba * TILE;
    const int av = a0 + lane;
    for (int r = w; r < TILE; r += TPB / 64) {
      const int x = x0 + r;
      if (x < X2 && av < nA) tile[r][lane] = a == 1 ? op(x, av, b) : op(x, b, av);
    }
    __syncthreads();
    const int xv = x0 + lane;
    for (int r = w; r < TILE; r += TPB / 64) {
      const int ar = a0 + r;
      if (xv < X2 && ar < nA) {
        const int j = a == 1 ? ar : b, k = a == 1 ? b : ar;
        dst[xv + (long long)X2 * (j + (long long)Y2 * k)] = tile[lane][r];
      }
    }
    __syncthreads();
  }
}

// the output axis that source x depends on most (ties to the lower axis); 0 also when that axis has fewer than TILED_MIN voxels: a 64 x 64 tile would then load with
// a few lanes of every wave (a choice by the shape, not measured)
constexpr int TILED_MIN = 16;
inline int rs_lane_axis(const double* M, int Y2, int Z2) {
  int a = 0;
  for (int c = 1; c < 3; ++c) if (fabs(M[c]) > fabs(M[a])) a = c;
  if ((a == 1 && Y2 < TILED_MIN) || (a == 2 && Z2 < TILED_MIN)) a = 0;
  return a;
}
template <typename T, typename Op>
void rs_launch(const Op& op, void* dst, int X2, int Y2, int Z2, int a, hipStream_t s) {
  if (a == 0) {
    hipLaunchKernelGGL((rs_direct_kernel<T, Op>), dim3(vol_blocks((long long)X2 * Y2 * Z2, GRID_CAP, TPB)), dim3(TPB), 0, s, op, static_cast<T*>(dst), X2, Y2, Z2);
    return;
  }
  const int tx = (X2 + TILE - 1) / TILE, ta = ((a == 1 ? Y2 : Z2) + TILE - 1) / TILE;
  const long long tiles = (long long)tx * ta * (a == 1 ? Z2 : Y2);
  hipLaunchKernelGGL((rs_tiled_kernel<T, Op>), dim3((unsigned)(tiles > GRID_CAP ? GRID_CAP : tiles)), dim3(TPB), 0, s, op, static_cast<T*>(dst), X2, Y2, Z2, a, tx, ta, tiles);
}
inline bool rs_fill_geom(rs_geom& g, const double* M, int X, int Y, int Z, int mode) {
  for (int i = 0; i < 12; ++i) { if (!std::isfinite(M[i])) return false; g.M.m[i] = M[i]; }
  g.X = X; g.Y = Y; g.Z = Z; g.mode = mode;
  return true;
}
}  // namespace

extern "C" {

int32_t unet_vol_resample_nearest(unet_ctx* ctx, const void* src, int32_t elem_bytes, int32_t X, int32_t Y, int32_t Z, const double* M, int32_t mode, uint64_t cval_bits,
                                  void* dst, int32_t X2, int32_t Y2, int32_t Z2, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok_or_empty(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_nearest: a source dimension is negative or the source has 2^31 voxels or more");
  if (!rs_out_ok(X2, Y2, Z2)) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_nearest: an output of %d x %d x %d (every extent is at least 1, fewer than 2^31 voxels)", X2, Y2, Z2);
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_nearest: elements of %d bytes, not 1, 2, 4 or 8", elem_bytes);
  if (mode < 0 || mode > 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_nearest: mode %d is not 0 (nearest edge) or 1 (constant)", mode);
  const bool empty = (long long)X * Y * Z == 0;
  if (empty && mode == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_nearest: the source has no voxels and mode 0 has no edge to repeat");
  rs_geom g{};
  if (!M || !rs_fill_geom(g, M, X, Y, Z, mode)) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_nearest: M is 12 finite doubles");
  if ((!empty && (!src || (reinterpret_cast<uintptr_t>(src) % elem_bytes) != 0)) || !dst || (reinterpret_cast<uintptr_t>(dst) % elem_bytes) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_nearest: a null buffer, or one not aligned to its element size");
  hipStream_t s = as_stream(stream);
  const int a = rs_lane_axis(M, Y2, Z2);
  switch (elem_bytes) {
    case 1: rs_launch<uint8_t>(rs_near<uint8_t>{g, static_cast<const uint8_t*>(src), (uint8_t)cval_bits}, dst, X2, Y2, Z2, a, s); break;
    case 2: rs_launch<uint16_t>(rs_near<uint16_t>{g, static_cast<const uint16_t*>(src), (uint16_t)cval_bits}, dst, X2, Y2, Z2, a, s); break;
    case 4: rs_launch<uint32_t>(rs_near<uint32_t>{g, static_cast<const uint32_t*>(src), (uint32_t)cval_bits}, dst, X2, Y2, Z2, a, s); break;
    default: rs_launch<uint64_t>(rs_near<uint64_t>{g, static_cast<const uint64_t*>(src), (uint64_t)cval_bits}, dst, X2, Y2, Z2, a, s); break;
  }
  UNET_CHECK_LAUNCH(ctx, "vol_resample_nearest"); return UNET_OK;
}

int32_t unet_vol_resample_linear(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, const double* M,
                                 int32_t mode, double cval, void* dst, int32_t dst_dtype, int32_t X2, int32_t Y2, int32_t Z2, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok_or_empty(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: a source dimension is negative or the source has 2^31 voxels or more");
  if (!rs_out_ok(X2, Y2, Z2)) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: an output of %d x %d x %d (every extent is at least 1, fewer than 2^31 voxels)", X2, Y2, Z2);
  if (vol_itemsize(dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: the NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64");
  if (dst_dtype != 64 && dst_dtype != 16 && dst_dtype != 2) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: dst_dtype %d is not 64 (float64), 16 (float32) or 2 (uint8 mask)", dst_dtype);
  if (mode < 0 || mode > 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: mode %d is not 0 (nearest edge) or 1 (constant)", mode);
  const bool empty = (long long)X * Y * Z == 0;
  if (empty && mode == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: the source has no voxels and mode 0 has no edge to repeat");
  rs_geom g{};
  if (!M || !rs_fill_geom(g, M, X, Y, Z, mode)) UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: M is 12 finite doubles");
  if ((!empty && (!vox || (reinterpret_cast<uintptr_t>(vox) % vol_itemsize(dtype)) != 0)) || !dst || (reinterpret_cast<uintptr_t>(dst) % vol_itemsize(dst_dtype)) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_resample_linear: a null buffer, or one not aligned to its element size");
  const vol_voxels sv{vox, dtype, scaled ? 1 : 0, slope, inter};
  hipStream_t s = as_stream(stream);
  const int a = rs_lane_axis(M, Y2, Z2);
  switch (dst_dtype) {
    case 64: rs_launch<double>(rs_lin<double>{g, sv, cval}, dst, X2, Y2, Z2, a, s); break;
    case 16: rs_launch<float>(rs_lin<float>{g, sv, cval}, dst, X2, Y2, Z2, a, s); break;
    default: rs_launch<uint8_t>(rs_lin<uint8_t>{g, sv, cval}, dst, X2, Y2, Z2, a, s); break;
  }
  UNET_CHECK_LAUNCH(ctx, "vol_resample_linear"); return UNET_OK;
}

}  // extern "C"

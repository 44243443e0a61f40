// A picture of a segmented CT volume: the raw NIfTI voxels already on the device, decoded as get_fdata() decodes them, and up to four label volumes.
//   the maximum / minimum of the CT and the largest label of every column of a slab along one axis                                 unet_vol_project
//   one RGB canvas of up to 64 tiles: a windowed, colour-mapped plane per tile with the label layers blended and outlined on top     unet_vol_render
// Volumes are [X, Y, Z] in Fortran order (f = x + X (y + Y z)), X Y Z < 2^31, decoded by vol_common.h's vol_dec.
// Projection: max / min travel as the order-preserving 64-bit keys of vol_common.h (-0.0 below +0.0, a NaN never enters), so the result does not depend on the
// order of the walk.  Along y or z a lane owns one x and walks the slab: every load of a wave is one run of consecutive voxels.  Along x a wave owns one (y, z) column, its
// lanes stride x (consecutive voxels again), the 64 partial results meet in a butterfly of __shfl_xor and lane 0 stores.
// Canvas: a lane owns one canvas pixel, a workgroup 256 consecutive pixels of one canvas row; the tile list sits in the kernel arguments (no copy, nothing to synchronise)
// and the row test of the tile search is uniform over the workgroup.  Axial and coronal tiles put x along the lanes.  The sample positions, the blend of the four
// neighbours and the window are float64 operations rounded one by one (-ffp-contract=off and the __d*_rn forms: numpy restates them bit for bit); labels are sampled
// nearest; a lane whose label is <= 0 in every layer reads no neighbour and blends nothing.  Stores: the four lanes of a group hold 12 bytes; where the canvas row starts on
// a 4-byte boundary and all four write, three of them store one assembled dword each, otherwise every writing lane stores its three bytes.  Nothing is written past a row.
#include "common.h"
#include "vol_common.h"

#include <cmath>

namespace {
constexpr int TPB = 256;
constexpr int MAX_TILES = UNET_RENDER_MAX_TILES;
constexpr int MAX_LAYERS = UNET_RENDER_MAX_LAYERS;
constexpr long long GRID_CAP = 256 * 32;

__device__ __forceinline__ int rd_label(const void* p, int i32, long long i) { return i32 ? static_cast<const int32_t*>(p)[i] : (int)static_cast<const uint8_t*>(p)[i]; }

// ---- (a) projection -------------------------------------------------------------------------------------------------------------------------------------
struct pj_args {
  vol_voxels src;
  const void* lab[MAX_LAYERS]; void* lab_out[MAX_LAYERS]; int lab_i32[MAX_LAYERS]; int n_lab;
  double* out;
  int X, Y, Z, axis, a, b, mode;
};
__device__ __forceinline__ unsigned long long pj_none(int mode) { return mode ? ~0ull : 0ull; }
__device__ __forceinline__ unsigned long long pj_pick(unsigned long long acc, unsigned long long k, int mode) { return mode ? min(acc, k) : max(acc, k); }
__device__ __forceinline__ double pj_value(unsigned long long key, int mode) { return key == pj_none(mode) ? __longlong_as_double(0x7FF8000000000000ll) : vol_ord2d(key); }
__device__ __forceinline__ void pj_store_label(void* out, int i32, long long o, int m) {
  if (i32) static_cast<int32_t*>(out)[o] = m; else static_cast<uint8_t*>(out)[o] = (uint8_t)m;
}

// along y (axis 1: outputs [X, Z]) or z (axis 2: outputs [X, Y]): output o = x + X q, one lane each; the slab is walked with a stride of X or X Y voxels
__global__ __launch_bounds__(TPB) void pj_walk_kernel(pj_args A) {
  const int n2 = A.axis == 1 ? A.Z : A.Y;
  const long long outs = (long long)A.X * n2, XY = (long long)A.X * A.Y;
  const long long step = A.axis == 1 ? (long long)A.X : XY, qstride = A.axis == 1 ? XY : (long long)A.X;
  for (long long o = (long long)blockIdx.x * TPB + threadIdx.x; o < outs; o += (long long)gridDim.x * TPB) {
    const long long q = o / A.X, base = (o - q * A.X) + qstride * q;
    unsigned long long key = pj_none(A.mode);
    for (int k = A.a; k < A.b; ++k) {
      const double v = vol_dec(A.src, base + step * k);
      if (v == v) key = pj_pick(key, vol_d2ord(v), A.mode);
    }
    A.out[o] = pj_value(key, A.mode);
    for (int l = 0; l < A.n_lab; ++l) {
      if (!A.lab[l]) continue;
      int m = rd_label(A.lab[l], A.lab_i32[l], base + step * A.a);
      for (int k = A.a + 1; k < A.b; ++k) m = max(m, rd_label(A.lab[l], A.lab_i32[l], base + step * k));
      pj_store_label(A.lab_out[l], A.lab_i32[l], o, m);
    }
  }
}

// along x (axis 0: outputs [Y, Z]): one wave per column c = y + Y z, lanes stride x; every trip count below is wave-uniform
__global__ __launch_bounds__(TPB) void pj_wave_kernel(pj_args A) {
  const int lane = threadIdx.x & 63;
  const long long cols = (long long)A.Y * A.Z, waves = (long long)gridDim.x * (TPB / 64);
  for (long long c = ((long long)blockIdx.x * TPB + threadIdx.x) >> 6; c < cols; c += waves) {
    const long long base = c * A.X;
    unsigned long long key = pj_none(A.mode);
    for (int x = A.a + lane; x < A.b; x += 64) {
      const double v = vol_dec(A.src, base + x);
      if (v == v) key = pj_pick(key, vol_d2ord(v), A.mode);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = pj_pick(key, __shfl_xor(key, o, 64), A.mode);
    if (lane == 0) A.out[c] = pj_value(key, A.mode);
    for (int l = 0; l < A.n_lab; ++l) {
      if (!A.lab[l]) continue;                                        // (uniform)
      int m = (int)0x80000000;
      for (int x = A.a + lane; x < A.b; x += 64) m = max(m, rd_label(A.lab[l], A.lab_i32[l], base + x));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
      if (lane == 0) pj_store_label(A.lab_out[l], A.lab_i32[l], c, m);
    }
  }
}

// ---- (b) canvas ---------------------------------------------------------------------------------------------------------------------------------------
struct rd_layer { const void* labels; const uint8_t* palette; int i32, P, fill, outline; };
struct rd_args {
  vol_voxels src;
  int X, Y;
  int lo[3], n[3];                                                    // the region and its extents
  double wlo, whi;
  const uint8_t* table;
  int interp, fill_bg;
  unsigned bg;                                                        // r | g << 8 | b << 16
  int n_layers, n_tiles;
  rd_layer layer[MAX_LAYERS];
  unet_render_tile tile[MAX_TILES];
  uint8_t* canvas;
  int H, W;
};
// min(int(floor((j + 0.5) n / w)), n - 1)
__device__ __forceinline__ int rd_near(int j, int n, int w) {
  return min((int)floor(__ddiv_rn(__dmul_rn((double)j + 0.5, (double)n), (double)w)), n - 1);
}
// (j + 0.5) n / w - 0.5
__device__ __forceinline__ double rd_pos(int j, int n, int w) { return __dsub_rn(__ddiv_rn(__dmul_rn((double)j + 0.5, (double)n), (double)w), 0.5); }

__global__ __launch_bounds__(TPB) void rd_canvas_kernel(rd_args A) {
  const int cy = blockIdx.y, cx = blockIdx.x * TPB + threadIdx.x, lane = threadIdx.x & 63;
  int ti = -1;
  for (int t = 0; t < A.n_tiles; ++t) {                               // (the tiles do not overlap: at most one holds the pixel)
    const unet_render_tile& T = A.tile[t];
    if (cy < T.y0 || cy >= T.y0 + T.h) continue;                      // uniform over the workgroup
    if (cx >= T.x0 && cx < T.x0 + T.w) ti = t;
  }
  const bool write = cx < A.W && (ti >= 0 || A.fill_bg);
  unsigned rgb = A.bg;
  if (ti >= 0) {
    const unet_render_tile T = A.tile[ti];
    const int j = cx - T.x0, i = cy - T.y0;
    const long long XY = (long long)A.X * A.Y;
    // image (row r, column c) of the tile's plane = voxel org + c su - r sv: column along the first in-plane axis, row against the second (np.rot90 of the slice)
    const int nu = T.axis == 0 ? A.n[1] : A.n[0], nv = T.axis == 2 ? A.n[1] : A.n[2];
    const int ulo = T.axis == 0 ? A.lo[1] : A.lo[0], vlo = T.axis == 2 ? A.lo[1] : A.lo[2];
    const long long su = T.axis == 0 ? (long long)A.X : 1ll, sv = T.axis == 2 ? (long long)A.X : XY;
    const long long sa = T.axis == 0 ? 1ll : (T.axis == 1 ? (long long)A.X : XY);
    const long long org = (long long)T.index * sa + (long long)ulo * su + (long long)(vlo + nv - 1) * sv;
    const int c = rd_near(j, nu, T.w), r = rd_near(i, nv, T.h);
    double val;
    if (A.interp == 0) {
      val = vol_dec(A.src, org + c * su - r * sv);
    } else {
      const double u = rd_pos(j, nu, T.w), v = rd_pos(i, nv, T.h);
      const double fu = floor(u), fv = floor(v), fx = __dsub_rn(u, fu), fy = __dsub_rn(v, fv);
      const int xi = (int)fu, yi = (int)fv;
      const int c0 = max(0, min(xi, nu - 1)), c1 = max(0, min(xi + 1, nu - 1)), r0 = max(0, min(yi, nv - 1)), r1 = max(0, min(yi + 1, nv - 1));
      const double p00 = vol_dec(A.src, org + c0 * su - r0 * sv), p01 = vol_dec(A.src, org + c1 * su - r0 * sv);
      const double p10 = vol_dec(A.src, org + c0 * su - r1 * sv), p11 = vol_dec(A.src, org + c1 * su - r1 * sv);
      const double top = __dadd_rn(p00, __dmul_rn(__dsub_rn(p01, p00), fx)), bot = __dadd_rn(p10, __dmul_rn(__dsub_rn(p11, p10), fx));
      val = __dadd_rn(top, __dmul_rn(__dsub_rn(bot, top), fy));
    }
    const double t = __ddiv_rn(__dsub_rn(val, A.wlo), __dsub_rn(A.whi, A.wlo));
    const int g = !(t > 0.0) ? 0 : (t >= 1.0 ? 255 : (int)floor(__dadd_rn(__dmul_rn(t, 255.0), 0.5)));          // (a NaN fails t > 0)
    unsigned cr = A.table[3 * g], cg = A.table[3 * g + 1], cb = A.table[3 * g + 2];
    const bool border = j == 0 || i == 0 || j == T.w - 1 || i == T.h - 1;          // a neighbour outside the tile counts as label 0
    int cm = 0, cp = 0, rm = 0, rp = 0;
    bool have = false;
    const long long vi = org + c * su - r * sv;
    for (int l = 0; l < A.n_layers; ++l) {
      const rd_layer& Y = A.layer[l];
      const int L = rd_label(Y.labels, Y.i32, vi);
      if (L <= 0) continue;
      bool edge = border;
      if (!edge) {
        if (!have) { cm = rd_near(j - 1, nu, T.w); cp = rd_near(j + 1, nu, T.w); rm = rd_near(i - 1, nv, T.h); rp = rd_near(i + 1, nv, T.h); have = true; }
        edge = rd_label(Y.labels, Y.i32, org + cm * su - r * sv) != L || rd_label(Y.labels, Y.i32, org + cp * su - r * sv) != L ||
               rd_label(Y.labels, Y.i32, org + c * su - rm * sv) != L || rd_label(Y.labels, Y.i32, org + c * su - rp * sv) != L;
      }
      const unsigned a = (unsigned)(edge ? Y.outline : Y.fill);
      if (a == 0) continue;
      const uint8_t* pc = Y.palette + 3 * (1 + (L - 1) % (Y.P - 1));          // 1 .. P - 1: never an address outside the palette
      cr = (pc[0] * a + cr * (255u - a) + 127u) / 255u;
      cg = (pc[1] * a + cg * (255u - a) + 127u) / 255u;
      cb = (pc[2] * a + cb * (255u - a) + 127u) / 255u;
    }
    rgb = cr | cg << 8 | cb << 16;
  }
  // every lane of the workgroup arrives here
  const unsigned long long wmask = __ballot(write);
  const unsigned nxt = __shfl_down(rgb, 1, 64);
  const bool aligned = ((reinterpret_cast<uintptr_t>(A.canvas) + (unsigned long long)cy * A.W * 3ull) & 3ull) == 0;          // cx of a group's first lane is a multiple of 4: 12 bytes
  const bool quad = aligned && ((wmask >> (lane & ~3)) & 0xFull) == 0xFull;
  uint8_t* px = A.canvas + ((long long)cy * A.W + cx) * 3;
  const int q = lane & 3;
  if (quad) {                                                         // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
    if (q < 3) *reinterpret_cast<unsigned*>(px + q) = q == 0 ? (rgb | nxt << 24) : (q == 1 ? (rgb >> 8 | nxt << 16) : (rgb >> 16 | nxt << 8));
  } else if (write) {
    px[0] = (uint8_t)rgb; px[1] = (uint8_t)(rgb >> 8); px[2] = (uint8_t)(rgb >> 16);
  }
}
}  // namespace

extern "C" {

int32_t unet_vol_project(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, int32_t axis, int32_t a,
                         int32_t b, int32_t mode, const void* const* labels, const int32_t* label_dtypes, void* const* label_planes, int32_t n_labels, double* plane,
                         void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_project: a dimension is negative or the volume has 2^31 voxels or more");
  if (vol_itemsize(dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_project: the NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64");
  if (axis < 0 || axis > 2) UNET_FAIL(ctx, UNET_E_ARG, "vol_project: axis %d is not 0, 1 or 2", axis);
  if (mode < 0 || mode > 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_project: mode %d is not 0 (max) or 1 (min)", mode);
  const int len = axis == 0 ? X : (axis == 1 ? Y : Z);
  if (a < 0 || a >= b || b > len) UNET_FAIL(ctx, UNET_E_ARG, "vol_project: the slab [%d, %d) is empty or leaves the axis of %d voxels", a, b, len);
  if (n_labels < 0 || n_labels > MAX_LAYERS || (n_labels > 0 && (!labels || !label_dtypes || !label_planes)))
    UNET_FAIL(ctx, UNET_E_ARG, "vol_project: 0 to %d label volumes are taken, not %d (or a null list)", MAX_LAYERS, n_labels);
  if ((long long)X * Y * Z == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_project: the volume has no voxels");
  if (!vox || (reinterpret_cast<uintptr_t>(vox) % vol_itemsize(dtype)) != 0 || !plane || (reinterpret_cast<uintptr_t>(plane) % 8) != 0)
    UNET_FAIL(ctx, UNET_E_ARG, "vol_project: null voxel buffer or plane, or a buffer not aligned to its item size");
  pj_args A{};
  A.src = vol_voxels{vox, dtype, scaled ? 1 : 0, slope, inter};
  A.n_lab = n_labels;
  for (int l = 0; l < n_labels; ++l) {
    if (!labels[l]) continue;                                         // a null volume: nothing is read or written for it
    if (label_dtypes[l] != 2 && label_dtypes[l] != 8) UNET_FAIL(ctx, UNET_E_ARG, "vol_project: label volume %d has datatype code %d, not 2 (uint8) or 8 (int32)", l, label_dtypes[l]);
    const int i32 = label_dtypes[l] == 8;
    if (!label_planes[l] || (i32 && ((reinterpret_cast<uintptr_t>(labels[l]) % 4) != 0 || (reinterpret_cast<uintptr_t>(label_planes[l]) % 4) != 0)))
      UNET_FAIL(ctx, UNET_E_ARG, "vol_project: label volume %d has no plane, or an int32 buffer is not 4-byte aligned", l);
    A.lab[l] = labels[l]; A.lab_out[l] = label_planes[l]; A.lab_i32[l] = i32;
  }
  A.out = plane;
  A.X = X; A.Y = Y; A.Z = Z; A.axis = axis; A.a = a; A.b = b; A.mode = mode;
  hipStream_t s = as_stream(stream);
  if (axis == 0) hipLaunchKernelGGL(pj_wave_kernel, dim3(vol_blocks((long long)Y * Z * 64, GRID_CAP, TPB)), dim3(TPB), 0, s, A);
  else hipLaunchKernelGGL(pj_walk_kernel, dim3(vol_blocks((long long)X * (axis == 1 ? Z : Y), GRID_CAP, TPB)), dim3(TPB), 0, s, A);
  UNET_CHECK_LAUNCH(ctx, "vol_project"); return UNET_OK;
}

int32_t unet_vol_render(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, const int32_t* roi,
                        double lo, double hi, const uint8_t* table, int32_t interp, int32_t background, int32_t fill_background, const unet_render_layer* layers,
                        int32_t n_layers, const unet_render_tile* tiles, int32_t n_tiles, uint8_t* canvas, int32_t H, int32_t W, void* stream) {
  if (!ctx) return UNET_E_ARG;
  if (!vol_dims_ok(X, Y, Z)) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: a dimension is negative or the volume has 2^31 voxels or more");
  if (vol_itemsize(dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: the NIfTI datatype code is not one of 2, 256, 4, 512, 8, 768, 16, 64");
  if (n_tiles < 0 || n_tiles > MAX_TILES || (n_tiles > 0 && !tiles)) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: 0 to %d tiles are taken, not %d (or a null list)", MAX_TILES, n_tiles);
  if (n_layers < 0 || n_layers > MAX_LAYERS || (n_layers > 0 && !layers)) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: 0 to %d layers are taken, not %d (or a null list)", MAX_LAYERS, n_layers);
  if (!roi) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: no region");
  const int dims[3] = {X, Y, Z};
  for (int d = 0; d < 3; ++d)
    if (roi[2 * d] < 0 || roi[2 * d] >= roi[2 * d + 1] || roi[2 * d + 1] > dims[d])
      UNET_FAIL(ctx, UNET_E_ARG, "vol_render: the region [%d, %d) of axis %d is empty or leaves the volume's %d voxels", roi[2 * d], roi[2 * d + 1], d, dims[d]);
  if (!(hi > lo)) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: the window needs lo < hi (and no NaN)");
  if (interp < 0 || interp > 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: interp %d is not 0 (nearest) or 1 (linear)", interp);
  if (background < 0 || background > 0xFFFFFF) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: the background is 0xRRGGBB");
  if (H < 0 || W < 0 || (long long)H * W * 3 >= 0x80000000LL) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: a canvas of %d x %d", H, W);
  if (!vox || (reinterpret_cast<uintptr_t>(vox) % vol_itemsize(dtype)) != 0 || !table) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: null voxel buffer or colour table, or voxels not aligned to their item size");
  rd_args A{};
  A.src = vol_voxels{vox, dtype, scaled ? 1 : 0, slope, inter};
  A.X = X; A.Y = Y;
  for (int d = 0; d < 3; ++d) { A.lo[d] = roi[2 * d]; A.n[d] = roi[2 * d + 1] - roi[2 * d]; }
  A.wlo = lo; A.whi = hi; A.table = table; A.interp = interp; A.fill_bg = fill_background ? 1 : 0;
  A.bg = (unsigned)((background >> 16) & 0xFF) | (unsigned)(background & 0xFF00) | (unsigned)(background & 0xFF) << 16;
  A.n_layers = n_layers; A.n_tiles = n_tiles;
  for (int l = 0; l < n_layers; ++l) {
    const unet_render_layer& Y_ = layers[l];
    if (Y_.dtype != 2 && Y_.dtype != 8) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: layer %d has datatype code %d, not 2 (uint8) or 8 (int32)", l, Y_.dtype);
    if (!Y_.labels || (Y_.dtype == 8 && (reinterpret_cast<uintptr_t>(Y_.labels) % 4) != 0)) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: layer %d has no label volume, or int32 labels off their alignment", l);
    if (!Y_.palette || Y_.palette_size < 2) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: layer %d needs a palette of at least 2 colours, not %d", l, Y_.palette_size);
    if (Y_.fill_alpha < 0 || Y_.fill_alpha > 255 || Y_.outline_alpha < 0 || Y_.outline_alpha > 255) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: layer %d has an alpha outside 0..255", l);
    A.layer[l] = rd_layer{Y_.labels, Y_.palette, Y_.dtype == 8, Y_.palette_size, Y_.fill_alpha, Y_.outline_alpha};
  }
  for (int t = 0; t < n_tiles; ++t) {
    const unet_render_tile& T = tiles[t];
    if (T.axis < 0 || T.axis > 2) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: tile %d has axis %d", t, T.axis);
    if (T.index < roi[2 * T.axis] || T.index >= roi[2 * T.axis + 1]) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: tile %d shows plane %d, outside the region of axis %d", t, T.index, T.axis);
    if (T.w < 1 || T.h < 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: tile %d is %d x %d pixels", t, T.w, T.h);
    if (T.x0 < 0 || T.y0 < 0 || (long long)T.x0 + T.w > W || (long long)T.y0 + T.h > H) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: tile %d leaves the canvas", t);
    for (int k = 0; k < t; ++k) {
      const unet_render_tile& K = tiles[k];
      if (T.x0 < K.x0 + K.w && K.x0 < T.x0 + T.w && T.y0 < K.y0 + K.h && K.y0 < T.y0 + T.h) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: tiles %d and %d overlap", k, t);
    }
    A.tile[t] = T;
  }
  if (H == 0 || W == 0) return UNET_OK;
  if (!canvas) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: no canvas");
  if (H > 65535) UNET_FAIL(ctx, UNET_E_ARG, "vol_render: a canvas of more than 65535 rows");
  A.canvas = canvas; A.H = H; A.W = W;
  hipLaunchKernelGGL(rd_canvas_kernel, dim3((unsigned)((W + TPB - 1) / TPB), (unsigned)H), dim3(TPB), 0, as_stream(stream), A);
  UNET_CHECK_LAUNCH(ctx, "vol_render"); return UNET_OK;
}

}  // extern "C"

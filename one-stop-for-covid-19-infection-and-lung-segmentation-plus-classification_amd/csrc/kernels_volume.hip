// A CT volume on the device, from the raw NIfTI voxel buffer to the slice batch and back ("volume path"):
//   read_nii / read_nii_demo, first half (T1:285-297, 317-337):  get_fdata -> np.rot90 -> keep slices [z0, z1) -> cv2.resize(float64 slice, (S, S), INTER_AREA)
//                                                                 -> (img - min)/(max - min), np.uint8(img * 255), img[img > 0] = 1         unet_vol_slices_f64
//   the inverse of crop -> resize -> fuse -> resize (T1:352-358, 486): model probabilities back onto the S x S canvas                        unet_vol_paste_back
//   canvas -> patient space: resample to [Y, X], undo the rot90, threshold, count                                                             unet_vol_unslice
// Bit-exact against tests/volume_oracle.py, which restates OpenCV's resize.cpp for 64-bit float images (cv2 is not in this image: parity unpinned, like CLAHE).
// Compiled with -ffp-contract=off (csrc/Makefile): every product and sum below is rounded on its own, as the C++ / numpy expressions it restates are.
#include "common.h"
#include "vol_common.h"
#include "vol_sample.h"

namespace {
constexpr int TPB = 256;

// ---- typed voxel access: NIfTI-1 datatype codes, Fortran order [X, Y, Z] -------------------------------------------------------------------
struct vol_src { const void* p; int dt, X, Y; int scaled; double slope, inter; };          // vol_common.h's vol_voxels and the slice extents, in the order the kernels take them
__device__ __forceinline__ double vol_dec(const vol_src& s, long long i) { return vol_dec(vol_voxels{s.p, s.dt, s.scaled, s.slope, s.inter}, i); }
// pixel (row i, column j) of slice z after np.rot90: vol[x = j, y = Y - 1 - i, z]; a row of the image is contiguous in x
__device__ __forceinline__ double vol_px(const vol_src& s, long long zoff, int i, int j) { return vol_dec(s, zoff + (long long)(s.Y - 1 - i) * s.X + j); }

// computeResizeAreaTab for one destination index (the same table kernels_pre.hip rebuilds for uint8 images)
struct vspan { int s1, s2; float a_left, a_mid, a_right; bool left, right; };
__device__ __forceinline__ vspan vol_area_cells(int d, double scale, int ssize) {
  vspan r;
  const double f1 = d * scale, f2 = f1 + scale;
  const double cell = fmin(scale, ssize - f1);
  int s1 = (int)ceil(f1), s2 = (int)floor(f2);
  s2 = min(s2, ssize - 1);
  s1 = min(s1, s2);
  r.s1 = s1; r.s2 = s2;
  r.left = (s1 - f1) > 1e-3;
  r.a_left = (float)((s1 - f1) / cell);
  r.a_mid = (float)(1.0 / cell);
  r.right = (f2 - s2) > 1e-3;
  r.a_right = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
  return r;
}
// the bilinear pair of one destination index with INTER_AREA's coefficients (float32, not fixed point: the 64-bit float path); `clamp` = the x-axis borders
__device__ __forceinline__ void vol_linear_coef(int d, int ssize, double scale, double inv_scale, bool clamp, int* so, float* c0, float* c1) {
  int s = (int)floor(d * scale);
  float f = (float)((d + 1) - (s + 1) * inv_scale);
  f = f <= 0.f ? 0.f : f - floorf(f);
  if (clamp) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  }
  *so = s; *c0 = 1.f - f; *c1 = f;
}

// cv2.resize(slice, (S, S), INTER_AREA) of a float64 [sh = Y, sw = X] image: destination pixel (dy, dx)
__device__ double vol_resize_px(const vol_src& s, long long zoff, int dy, int dx, int S) {
  const int sw = s.X, sh = s.Y;
  if (sw == S && sh == S) return vol_px(s, zoff, dy, dx);                                   // dsize == ssize: a copy
  const double inv_x = (double)S / sw, inv_y = (double)S / sh;
  const double scale_x = 1.0 / inv_x, scale_y = 1.0 / inv_y;
  if (scale_x >= 1.0 && scale_y >= 1.0) {
    const int isx = (int)rint(scale_x), isy = (int)rint(scale_y);
    if (fabs(scale_x - isx) < 2.220446049250313e-16 && fabs(scale_y - isy) < 2.220446049250313e-16) {
      double sum = 0.0;                                                                     // resizeAreaFast_: float64 sum in source order, then * float32 (1 / area)
      for (int ky = 0; ky < isy; ++ky)
        for (int kx = 0; kx < isx; ++kx) sum = sum + vol_px(s, zoff, dy * isy + ky, dx * isx + kx);
      return sum * (double)(1.f / (float)(isx * isy));
    }
    const vspan xs = vol_area_cells(dx, scale_x, sw), ys = vol_area_cells(dy, scale_y, sh);      // ResizeArea_: x table first, then the rows
    double acc = 0.0; bool first = true;
    const int y_lo = ys.left ? ys.s1 - 1 : ys.s1, y_hi = ys.right ? ys.s2 : ys.s2 - 1;
    for (int sy = y_lo; sy <= y_hi; ++sy) {
      const double beta = (double)((sy < ys.s1) ? ys.a_left : (sy < ys.s2 ? ys.a_mid : ys.a_right));
      double buf = 0.0;
      if (xs.left) buf = buf + vol_px(s, zoff, sy, xs.s1 - 1) * (double)xs.a_left;
      for (int sx = xs.s1; sx < xs.s2; ++sx) buf = buf + vol_px(s, zoff, sy, sx) * (double)xs.a_mid;
      if (xs.right) buf = buf + vol_px(s, zoff, sy, xs.s2) * (double)xs.a_right;
      acc = first ? beta * buf : acc + beta * buf;
      first = false;
    }
    return acc;
  }
  int sx, sy; float a0, a1, b0, b1;                                                          // an up-scaling axis: the bilinear code with the area coefficients
  vol_linear_coef(dx, sw, scale_x, inv_x, true, &sx, &a0, &a1);
  vol_linear_coef(dy, sh, scale_y, inv_y, false, &sy, &b0, &b1);
  const int x1 = min(sx + 1, sw - 1);
  const int r0 = max(0, min(sy, sh - 1)), r1 = max(0, min(sy + 1, sh - 1));
  const double h0 = vol_px(s, zoff, r0, sx) * (double)a0 + vol_px(s, zoff, r0, x1) * (double)a1;
  const double h1 = vol_px(s, zoff, r1, sx) * (double)a0 + vol_px(s, zoff, r1, x1) * (double)a1;
  return h0 * (double)b0 + h1 * (double)b1;
}

// per-slice words behind the float64 images: [min key, max key, any NaN, any voxel != the first]
constexpr int VOL_STATE = 4;
__global__ void vol_state_init_kernel(unsigned long long* st, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { st[VOL_STATE * i] = ~0ull; st[VOL_STATE * i + 1] = 0ull; st[VOL_STATE * i + 2] = 0ull; st[VOL_STATE * i + 3] = 0ull; }
}
// pass 1 (blockIdx.y = kept slice): the resized float64 image, its min / max (one ordered-integer atomic pair per workgroup: exact, min / max do not round), and --
// while the slice's voxels are on their way through the caches anyway -- whether any voxel differs from the first (np.unique(slice).size == 1)
__global__ __launch_bounds__(TPB) void vol_resize_kernel(vol_src s, int z0, int S, double* __restrict__ img, unsigned long long* __restrict__ st) {
  __shared__ double s_mn[TPB / 64], s_mx[TPB / 64];
  __shared__ int s_flag[2];
  const int li = blockIdx.y, tid = threadIdx.x;
  const long long zoff = (long long)(z0 + li) * s.X * s.Y;
  const int P = S * S;
  if (tid < 2) s_flag[tid] = 0;
  __syncthreads();
  double mn = INFINITY, mx = -INFINITY; bool nan = false;
  for (int idx = blockIdx.x * TPB + tid; idx < P; idx += gridDim.x * TPB) {
    const int dy = idx / S, dx = idx - dy * S;
    const double v = vol_resize_px(s, zoff, dy, dx, S);
    img[(long long)li * P + idx] = v;
    if (v != v) nan = true; else { mn = fmin(mn, v); mx = fmax(mx, v); }
  }
  const double first = vol_dec(s, zoff);
  bool differs = false;
  const long long SP = (long long)s.X * s.Y;
  for (long long i = (long long)blockIdx.x * TPB + tid; i < SP; i += (long long)gridDim.x * TPB) {
    const double v = vol_dec(s, zoff + i);
    differs |= (v != first) && !(v != v && first != first);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mn = fmin(mn, __shfl_xor(mn, o, 64)); mx = fmax(mx, __shfl_xor(mx, o, 64)); }
  if ((tid & 63) == 0) { s_mn[tid >> 6] = mn; s_mx[tid >> 6] = mx; }
  if (nan) s_flag[0] = 1;
  if (differs) s_flag[1] = 1;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < TPB / 64; ++w) { mn = fmin(mn, s_mn[w]); mx = fmax(mx, s_mx[w]); }
    unsigned long long* q = st + (long long)VOL_STATE * li;
    if (mn <= mx) { atomicMin(q, vol_d2ord(mn)); atomicMax(q + 1, vol_d2ord(mx)); }
    if (s_flag[0]) atomicOr(q + 2, 1ull);
    if (s_flag[1]) atomicOr(q + 3, 1ull);
  }
}

// pass 2 over the float64 images: (img - min)/(max - min) in float64 as numpy does -> float32; np.uint8(img * 255) (truncation; NaN -> 0); the lung form
// img[img > 0] = 1 -> np.uint8(img * 255).  V = pixels per thread (4: 2 x 16-byte loads, one 16-byte and two 4-byte stores)
struct vol_mm { double mn, mx, d; };
__device__ __forceinline__ vol_mm vol_minmax(const unsigned long long* st, int li) {
  const unsigned long long* q = st + (long long)VOL_STATE * li;
  double mn = vol_ord2d(q[0]), mx = vol_ord2d(q[1]);
  if (q[2]) mn = mx = __longlong_as_double(0x7FF8000000000000ll);                              // numpy's min / max propagate a NaN
  return {mn, mx, mx - mn};
}
template <int V>
__global__ __launch_bounds__(TPB) void vol_outputs_kernel(const double* __restrict__ img, const unsigned long long* __restrict__ st, int P, float* __restrict__ f32,
                                                         uint8_t* __restrict__ u8, uint8_t* __restrict__ lung, int32_t* __restrict__ uniform, double* __restrict__ minmax) {
  const int li = blockIdx.y;
  const vol_mm m = vol_minmax(st, li);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (uniform) uniform[li] = st[(long long)VOL_STATE * li + 3] ? 0 : 1;
    if (minmax) { minmax[2 * li] = m.mn; minmax[2 * li + 1] = m.mx; }
  }
  const long long base = (long long)li * P;
  for (int q0 = (blockIdx.x * TPB + threadIdx.x) * V; q0 < P; q0 += gridDim.x * TPB * V) {
    double v[V]; float o[V]; uint8_t b[V], l[V];
    if constexpr (V == 4) {
      const double2 a = *reinterpret_cast<const double2*>(img + base + q0), c = *reinterpret_cast<const double2*>(img + base + q0 + 2);
      v[0] = a.x; v[1] = a.y; v[2] = c.x; v[3] = c.y;
    } else v[0] = img[base + q0];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double nrm = __ddiv_rn(__dsub_rn(v[k], m.mn), m.d);
      o[k] = (float)nrm;
      b[k] = (uint8_t)(int)__dmul_rn(nrm, 255.0);
      l[k] = nrm > 0.0 ? (uint8_t)255 : b[k];
    }
    if constexpr (V == 4) {
      if (f32) *reinterpret_cast<float4*>(f32 + base + q0) = make_float4(o[0], o[1], o[2], o[3]);
      if (u8) *reinterpret_cast<uchar4*>(u8 + base + q0) = make_uchar4(b[0], b[1], b[2], b[3]);
      if (lung) *reinterpret_cast<uchar4*>(lung + base + q0) = make_uchar4(l[0], l[1], l[2], l[3]);
    } else {
      if (f32) f32[base + q0] = o[0];
      if (u8) u8[base + q0] = b[0];
      if (lung) lung[base + q0] = l[0];
    }
  }
}

constexpr int PASTE_SLICES = 64;                                    // slices per launch: their rectangles travel as a kernel argument (2 KiB)
struct paste_rects { int r[PASTE_SLICES][8]; };
__global__ __launch_bounds__(TPB) void vol_paste_kernel(const float* __restrict__ prob, int d, paste_rects rc, int img0, float* __restrict__ canvas, int S) {
  const int li = blockIdx.y;
  const int idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= S * S) return;
  const int r = idx / S, c = idx - r * S;
  const float* p = prob + (long long)(img0 + li) * d * d;
  const int* R = rc.r[li];
  float out = 0.0f;
  if (R[2] <= 0 && R[6] <= 0) {                                      // no rectangles: the slice fell through uncropped (T1:347) -> the whole canvas
    out = vol_bilerp(p, d, d, (c + 0.5) * d / S - 0.5, (r + 0.5) * d / S - 0.5);
  } else {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int x = R[4 * k], y = R[4 * k + 1], w = R[4 * k + 2], h = R[4 * k + 3];
      if (w <= 0 || h <= 0 || c < x || c >= x + w || r < y || r >= y + h) continue;
      const double u = (c - x + 0.5) * 125.0 / w - 0.5 + 125.0 * k, v = (r - y + 0.5) * 250.0 / h - 0.5;      // fused 250 x 250 coordinates
      const float val = vol_bilerp(p, d, d, (u + 0.5) * d / 250.0 - 0.5, (v + 0.5) * d / 250.0 - 0.5);
      out = fmaxf(out, val);                                         // overlap: the larger value wins (probabilities are >= 0)
    }
  }
  canvas[(long long)(img0 + li) * S * S + idx] = out;
}

// canvas -> [Y, X] with the same sampler, rot90 undone, thresholded: mask[x + X (y + Y z)] = p > t; per-slice integer counts.  V voxels (consecutive in x) per thread
template <int V>
__global__ __launch_bounds__(TPB) void vol_unslice_kernel(const float* __restrict__ canvas, int S, float t, int X, int Y, int z0, uint8_t* __restrict__ mask,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt;
  const int li = blockIdx.y;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const float* p = canvas + (long long)li * S * S;
  const int XV = X / V;
  int cnt = 0;
  for (int q = blockIdx.x * TPB + threadIdx.x; q < XV * Y; q += gridDim.x * TPB) {
    const int y = q / XV, x0 = (q - y * XV) * V;
    uint8_t b[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      b[k] = vol_unslice_px(p, S, X, Y, x0 + k, y) > t ? 1 : 0;
      cnt += b[k];
    }
    uint8_t* dst = mask + ((long long)(z0 + li) * Y + y) * X + x0;
    if constexpr (V == 4) *reinterpret_cast<uchar4*>(dst) = make_uchar4(b[0], b[1], b[2], b[3]);
    else dst[0] = b[0];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(counts + li, (unsigned long long)s_cnt);            // integer sums: exact in any order
}

}  // namespace

extern "C" {

size_t unet_vol_slices_ws_bytes(int32_t n, int32_t S) {
  return (n > 0 && S > 0) ? (size_t)n * S * S * sizeof(double) + (size_t)n * VOL_STATE * sizeof(unsigned long long) : 0;
}

int32_t unet_vol_slices_f64(unet_ctx* ctx, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, int32_t z0, int32_t z1,
                            int32_t S, float* img_f32, uint8_t* img_u8, uint8_t* lung_u8, int32_t* uniform, double* minmax, void* ws, size_t ws_bytes, void* stream) {
  if (!ctx || !vox || X < 1 || Y < 1 || Z < 1 || S < 1 || !ws) UNET_FAIL(ctx, UNET_E_ARG, "vol_slices_f64: bad args");
  if (vol_itemsize(dtype) == 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_slices_f64: NIfTI datatype code %d is not one of 2, 256, 4, 512, 8, 768, 16, 64", dtype);
  if (z0 < 0 || z1 > Z || z1 <= z0) UNET_FAIL(ctx, UNET_E_SHAPE, "vol_slices_f64: slice range [%d, %d) is empty or leaves the %d slices", z0, z1, Z);
  if ((long long)S * S > 0x3FFFFFFFLL || (long long)X * Y > 0x3FFFFFFFLL) UNET_FAIL(ctx, UNET_E_SHAPE, "vol_slices_f64: slice too large");
  if ((reinterpret_cast<uintptr_t>(vox) % vol_itemsize(dtype)) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_slices_f64: the voxel buffer is not aligned to its item size");
  const int n = z1 - z0, P = S * S;
  if (ws_bytes < unet_vol_slices_ws_bytes(n, S) || (reinterpret_cast<uintptr_t>(ws) % 16) != 0) UNET_FAIL(ctx, UNET_E_ARG, "vol_slices_f64: workspace too small or not 16-byte aligned");
  hipStream_t s = as_stream(stream);
  double* img = static_cast<double*>(ws);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(img + (size_t)n * P);
  const vol_src src{vox, dtype, X, Y, scaled ? 1 : 0, slope, inter};
  hipLaunchKernelGGL(vol_state_init_kernel, dim3((n + 63) / 64), dim3(64), 0, s, st, n);
  hipLaunchKernelGGL(vol_resize_kernel, dim3(vol_blocks(P, 1024, TPB), n), dim3(TPB), 0, s, src, z0, S, img, st);
  const bool vec = (P % 4) == 0 && (!img_f32 || reinterpret_cast<uintptr_t>(img_f32) % 16 == 0) && (!img_u8 || reinterpret_cast<uintptr_t>(img_u8) % 4 == 0) &&
                   (!lung_u8 || reinterpret_cast<uintptr_t>(lung_u8) % 4 == 0);
  if (vec) hipLaunchKernelGGL(vol_outputs_kernel<4>, dim3(vol_blocks(P / 4, 256, TPB), n), dim3(TPB), 0, s, img, st, P, img_f32, img_u8, lung_u8, uniform, minmax);
  else hipLaunchKernelGGL(vol_outputs_kernel<1>, dim3(vol_blocks(P, 1024, TPB), n), dim3(TPB), 0, s, img, st, P, img_f32, img_u8, lung_u8, uniform, minmax);
  UNET_CHECK_LAUNCH(ctx, "vol_slices_f64"); return UNET_OK;
}

int32_t unet_vol_paste_back(unet_ctx* ctx, const float* prob, int32_t n, int32_t d, const int32_t* rects, float* canvas, int32_t S, void* stream) {
  if (!ctx || !prob || !canvas || n < 1 || d < 1 || S < 1 || (long long)S * S > 0x3FFFFFFFLL) UNET_FAIL(ctx, UNET_E_ARG, "vol_paste_back: bad args");
  for (int i = 0; rects && i < n; ++i)                                // rects is a HOST array [n][2][4]: (x, y, w, h) of the two lungs; w <= 0 or h <= 0 = absent
    for (int k = 0; k < 2; ++k) {
      const int32_t* r = rects + 8 * i + 4 * k;
      if (r[2] <= 0 || r[3] <= 0) continue;
      if (r[0] < 0 || r[1] < 0 || (long long)r[0] + r[2] > S || (long long)r[1] + r[3] > S)
        UNET_FAIL(ctx, UNET_E_SHAPE, "vol_paste_back: rectangle %d of slice %d = (%d, %d, %d, %d) leaves the %d x %d canvas", k, i, r[0], r[1], r[2], r[3], S, S);
    }
  hipStream_t s = as_stream(stream);
  for (int i0 = 0; i0 < n; i0 += PASTE_SLICES) {
    const int cnt = (n - i0) < PASTE_SLICES ? (n - i0) : PASTE_SLICES;
    paste_rects rc;
    for (int i = 0; i < cnt; ++i)
      for (int k = 0; k < 8; ++k) {
        const int32_t* r = rects ? rects + 8 * (i0 + i) + (k & 4) : nullptr;
        rc.r[i][k] = (r && r[2] > 0 && r[3] > 0) ? r[k & 3] : 0;
      }
    hipLaunchKernelGGL(vol_paste_kernel, dim3((unsigned)(((long long)S * S + TPB - 1) / TPB), (unsigned)cnt), dim3(TPB), 0, s, prob, d, rc, i0, canvas, S);
  }
  UNET_CHECK_LAUNCH(ctx, "vol_paste_back"); return UNET_OK;
}

int32_t unet_vol_unslice(unet_ctx* ctx, const float* canvas, int32_t S, float threshold, int32_t X, int32_t Y, int32_t Z, int32_t z0, int32_t z1, uint8_t* mask,
                         int64_t* counts, void* stream) {
  if (!ctx || !canvas || !mask || !counts || S < 1 || X < 1 || Y < 1 || Z < 1) UNET_FAIL(ctx, UNET_E_ARG, "vol_unslice: bad args");
  if (z0 < 0 || z1 > Z || z1 <= z0) UNET_FAIL(ctx, UNET_E_SHAPE, "vol_unslice: slice range [%d, %d) is empty or leaves the %d slices", z0, z1, Z);
  if ((long long)X * Y > 0x3FFFFFFFLL || (long long)S * S > 0x3FFFFFFFLL) UNET_FAIL(ctx, UNET_E_SHAPE, "vol_unslice: slice too large");
  const int n = z1 - z0;
  hipStream_t s = as_stream(stream);
  UNET_HIP(ctx, hipMemsetAsync(mask, 0, (size_t)X * Y * Z, s));                                 // the trimmed slices stay 0
  UNET_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)n * sizeof(int64_t), s));
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  if ((X % 4) == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0)
    hipLaunchKernelGGL(vol_unslice_kernel<4>, dim3(vol_blocks((long long)(X / 4) * Y, 256, TPB), n), dim3(TPB), 0, s, canvas, S, threshold, X, Y, z0, mask, cnt);
  else
    hipLaunchKernelGGL(vol_unslice_kernel<1>, dim3(vol_blocks((long long)X * Y, 1024, TPB), n), dim3(TPB), 0, s, canvas, S, threshold, X, Y, z0, mask, cnt);
  UNET_CHECK_LAUNCH(ctx, "vol_unslice"); return UNET_OK;
}

}  // extern "C"

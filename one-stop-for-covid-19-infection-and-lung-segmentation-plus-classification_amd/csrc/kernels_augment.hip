// Random flip + affine augmentation of a training batch (augment.py: the reference's imgaug `seq`, T1:547-583), applied on the device.
//   dst_img[i]  = warp_bilinear(src_img[idx[i]], mats[i])     NHWC, c channels, taps outside the source read 0
//   dst_mask[i] = warp_nearest(src_mask[idx[i]], mats[i])     one channel, floor(s + 0.5), 0 outside
// mats[i] = the inverse map [m00 m01 m02 m10 m11 m12]: output pixel (x, y) -> source (m00 x + m01 y + m02, m10 x + m11 y + m12), pixel centres at
// integers.  HBM-bound: one lane = one output pixel with all of its channels, a wave = 64 consecutive x of one row (coalesced stores), a workgroup =
// a 64 x 4 tile of ONE sample, so the sample number and its six matrix values are wave-uniform.  Reads go through L2 / MALL (a rotated tile is a
// parallelogram in the source: no LDS staging).  The source coordinate is evaluated in fp64 from the fp32 table (4 FMAs per pixel, free in an
// HBM-bound kernel): it matches the float64 restatement to ~1e-13 px, and identity / flip rows -- integer coordinates -- copy or reverse bit for bit.
#include "common.h"

namespace {
constexpr int TILE_X = 64, TILE_Y = 4, TPB = TILE_X * TILE_Y;
constexpr long long MAX_BLOCKS_PER_LAUNCH = 1LL << 23;   // grid x stays far below 2^32 work-items

// C > 0: channel count known at compile time (1: the U-Net's CT slices, 3: the classifier's RGB); C == 0: runtime `cdyn`
template <int C>
__global__ __launch_bounds__(TPB) void augment_kernel(const float* __restrict__ src_img, const float* __restrict__ src_mask, const long long* __restrict__ idx,
                                                      const float* __restrict__ mats, float* __restrict__ dst_img, float* __restrict__ dst_mask, int h, int w,
                                                      int cdyn, int tiles_x, int tiles_per_sample, long long s0) {
  const int c = C > 0 ? C : cdyn;
  const long long i = s0 + (long long)blockIdx.x / tiles_per_sample;      // output sample (workgroup-uniform)
  const int t = (int)((long long)blockIdx.x % tiles_per_sample);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int x = tx * TILE_X + (int)(threadIdx.x % TILE_X), y = ty * TILE_Y + (int)(threadIdx.x / TILE_X);
  if (x >= w || y >= h) return;
  const long long si = idx ? idx[i] : i;                                   // source sample
  const long long plane = (long long)h * w, pix = (long long)y * w + x;
  const float* m = mats + i * 6;
  const double xs = fma((double)m[0], (double)x, fma((double)m[1], (double)y, (double)m[2]));
  const double ys = fma((double)m[3], (double)x, fma((double)m[4], (double)y, (double)m[5]));

  // image: bilinear, the four taps each read 0 outside [0, w) x [0, h)
  const float* S = src_img + si * plane * c;
  float* D = dst_img + (i * plane + pix) * c;
  if (xs > -1.0 && xs < (double)w && ys > -1.0 && ys < (double)h) {        // (false for NaN: a degenerate row writes zeros)
    const double fx = floor(xs), fy = floor(ys);
    const int x0 = (int)fx, y0 = (int)fy;
    const float ax = (float)(xs - fx), ay = (float)(ys - fy);
    const bool vx0 = x0 >= 0, vx1 = x0 + 1 < w, vy0 = y0 >= 0, vy1 = y0 + 1 < h;
    const long long o00 = ((long long)y0 * w + x0) * c, o10 = o00 + (long long)w * c;
    if (C > 0) {
#pragma unroll
      for (int ch = 0; ch < (C > 0 ? C : 1); ++ch) {
        const float v00 = (vy0 && vx0) ? S[o00 + ch] : 0.f, v01 = (vy0 && vx1) ? S[o00 + c + ch] : 0.f;
        const float v10 = (vy1 && vx0) ? S[o10 + ch] : 0.f, v11 = (vy1 && vx1) ? S[o10 + c + ch] : 0.f;
        const float top = v00 + ax * (v01 - v00), bot = v10 + ax * (v11 - v10);       // a + t (b - a): t = 0 returns a exactly
        D[ch] = top + ay * (bot - top);
      }
    } else {
      for (int ch = 0; ch < c; ++ch) {
        const float v00 = (vy0 && vx0) ? S[o00 + ch] : 0.f, v01 = (vy0 && vx1) ? S[o00 + c + ch] : 0.f;
        const float v10 = (vy1 && vx0) ? S[o10 + ch] : 0.f, v11 = (vy1 && vx1) ? S[o10 + c + ch] : 0.f;
        const float top = v00 + ax * (v01 - v00), bot = v10 + ax * (v11 - v10);
        D[ch] = top + ay * (bot - top);
      }
    }
  } else {
    for (int ch = 0; ch < c; ++ch) D[ch] = 0.f;
  }

  // mask: nearest neighbour, one channel
  if (dst_mask) {
    const double rx = floor(xs + 0.5), ry = floor(ys + 0.5);
    float v = 0.f;
    if (rx >= 0.0 && rx < (double)w && ry >= 0.0 && ry < (double)h) v = src_mask[si * plane + (long long)ry * w + (long long)rx];
    dst_mask[i * plane + pix] = v;
  }
}

template <int C>
int32_t launch_augment(unet_ctx* ctx, const float* src_img, const float* src_mask, const int64_t* idx, const float* mats, float* dst_img, float* dst_mask,
                       int64_t n, int32_t h, int32_t w, int32_t c, void* stream) {
  const int tiles_x = (w + TILE_X - 1) / TILE_X;
  const long long tps = (long long)tiles_x * ((h + TILE_Y - 1) / TILE_Y);
  const long long per = MAX_BLOCKS_PER_LAUNCH / tps;                        // samples per launch (>= 1: checked by the caller)
  for (long long s0 = 0; s0 < n; s0 += per) {
    const long long cnt = n - s0 < per ? n - s0 : per;
    hipLaunchKernelGGL(augment_kernel<C>, dim3((unsigned)(cnt * tps)), dim3(TPB), 0, as_stream(stream), src_img, src_mask,
                       reinterpret_cast<const long long*>(idx), mats, dst_img, dst_mask, (int)h, (int)w, (int)c, tiles_x, (int)tps, s0);
    UNET_CHECK_LAUNCH(ctx, "augment_samples");
  }
  return UNET_OK;
}
}  // namespace

extern "C" {

int32_t unet_augment_samples(unet_ctx* ctx, const float* src_img, const float* src_mask, const int64_t* idx, const float* mats, float* dst_img, float* dst_mask,
                             int64_t n, int32_t h, int32_t w, int32_t c, void* stream) {
  if (!src_img || !mats || !dst_img || n < 1 || h < 1 || w < 1 || c < 1 || c > 4096 || (!src_mask) != (!dst_mask))
    UNET_FAIL(ctx, UNET_E_ARG, "augment_samples: bad args (src_img, mats, dst_img non-null; n, h, w, c >= 1, c <= 4096; src_mask and dst_mask both set or both null)");
  const long long tps = (long long)((w + TILE_X - 1) / TILE_X) * ((h + TILE_Y - 1) / TILE_Y);
  if (tps > MAX_BLOCKS_PER_LAUNCH) UNET_FAIL(ctx, UNET_E_ARG, "augment_samples: %d x %d is too large an image", (int)h, (int)w);
  if (c == 1) return launch_augment<1>(ctx, src_img, src_mask, idx, mats, dst_img, dst_mask, n, h, w, c, stream);
  if (c == 3) return launch_augment<3>(ctx, src_img, src_mask, idx, mats, dst_img, dst_mask, n, h, w, c, stream);
  return launch_augment<0>(ctx, src_img, src_mask, idx, mats, dst_img, dst_mask, n, h, w, c, stream);
}

}  // extern "C"

// The sampler of the volume path's way back (paste-back and canvas -> patient space), shared by kernels_volume.hip and kernels_ensemble.hip so that the probability
// unet_vol_unslice_prob writes is, by construction, the value unet_vol_unslice compares against its threshold.  Both files are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace {
// ---- bilinear sample with half-pixel centres, clamped to the edge: coordinates in float64, the blend in float32 in this fixed order -----------------
//   fx = float32(u - floor(u));  top = p00 + (p01 - p00) * fx;  bot = p10 + (p11 - p10) * fx;  value = top + (bot - top) * fy      (a constant map stays that constant exactly)
__device__ __forceinline__ float vol_bilerp(const float* __restrict__ p, int w, int h, double u, double v) {
  const double fu = floor(u), fv = floor(v);
  const float fx = (float)(u - fu), fy = (float)(v - fv);
  const int xi = (int)fu, yi = (int)fv;
  const int x0 = max(0, min(xi, w - 1)), x1 = max(0, min(xi + 1, w - 1)), y0 = max(0, min(yi, h - 1)), y1 = max(0, min(yi + 1, h - 1));
  const float p00 = p[(long long)y0 * w + x0], p01 = p[(long long)y0 * w + x1], p10 = p[(long long)y1 * w + x0], p11 = p[(long long)y1 * w + x1];
  const float top = __fadd_rn(p00, __fmul_rn(__fsub_rn(p01, p00), fx)), bot = __fadd_rn(p10, __fmul_rn(__fsub_rn(p11, p10), fx));
  return __fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), fy));
}

// voxel (x, y) of a kept slice from its S x S canvas p: the canvas resampled to [Y, X] and np.rot90 undone (image row i = Y - 1 - y, column x)
__device__ __forceinline__ float vol_unslice_px(const float* __restrict__ p, int S, int X, int Y, int x, int y) {
  const int i = Y - 1 - y;
  const double v = (i + 0.5) * S / Y - 0.5;
  const double u = (x + 0.5) * S / X - 0.5;
  return vol_bilerp(p, S, S, u, v);
}
}  // namespace

// One map's sum of squared errors, the kernel the per-frame loss (frame_loss.hip: mval_frame_loss / _points) and the weighted
// training loss (loss_weighted.hip: mval_weighted_mse_fwd / _points_fwd) share: both must give the same bits per map.
//   one workgroup per map: d = h - g and d * d in float32 (torch's (h - gt) ** 2), summed in float64 -> per_map[m]
// No atomics and a fixed pixel -> lane assignment.  The assignment is the same whether the maps can be loaded as float4 or not
// (an unaligned base, hh * wh % 4 != 0): lane t adds the groups of four pixels t, t + 256, ..., a short last group padded with
// zeros.  g is read, or rendered from the joint's pixel position (gt_heatmap.h) under the map's own sigma where one is given.
#pragma once
#include "mval_common.h"
#include "gt_heatmap.h"

#define FL_THREADS 256

// four pixels of a map from pixel p on; past the map's end: 0
__device__ __forceinline__ float4 fl_load4(const float* __restrict__ map, int p, int hw, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(map + p);
  float4 r;
  r.x = map[p];
  r.y = p + 1 < hw ? map[p + 1] : 0.f;
  r.z = p + 2 < hw ? map[p + 2] : 0.f;
  r.w = p + 3 < hw ? map[p + 3] : 0.f;
  return r;
}

__device__ __forceinline__ float fl_render(int p, int hw, int wh, double px, double py, double two_s2) {
  return p < hw ? mval_gt_heatmap_pixel(p % wh, p / wh, px, py, two_s2) : 0.f;
}

// four ground-truth pixels from pixel p on: read (POINTS false) or rendered
template <bool POINTS>
__device__ __forceinline__ float4 fl_truth4(const float* __restrict__ gm, int p, int hw, int wh, bool vec, double px, double py,
                                            double two_s2) {
  if (!POINTS) return fl_load4(gm, p, hw, vec);
  float4 b;
  b.x = fl_render(p, hw, wh, px, py, two_s2);
  b.y = fl_render(p + 1, hw, wh, px, py, two_s2);
  b.z = fl_render(p + 2, hw, wh, px, py, two_s2);
  b.w = fl_render(p + 3, hw, wh, px, py, two_s2);
  return b;
}

// A map is skipped -- neither read nor rendered, per_map[m] = +0.0 -- where valid (u8, may be NULL) is 0 or weight (f32, may be
// NULL) is 0.  sig (may be NULL): sigma per map, 2 sigma^2 = 2.0 * (s * s) with each product rounded on its own, as the host forms
// two_s2 and as mse_two_s2 (loss_metric.hip) does.
template <bool POINTS>
__global__ __launch_bounds__(FL_THREADS) void frame_loss_map_kernel(const float* __restrict__ h, const float* __restrict__ g,
                                                                    const double* __restrict__ pt, double two_s2,
                                                                    const double* __restrict__ sig,
                                                                    const uint8_t* __restrict__ valid,
                                                                    const float* __restrict__ weight,
                                                                    double* __restrict__ per_map, int hh, int wh) {
  __shared__ double red[FL_THREADS / MVAL_WAVE];
  const int64_t m = blockIdx.x;
  if ((valid && !valid[m]) || (weight && weight[m] == 0.f)) {  // (uniform over the workgroup)
    if (threadIdx.x == 0) per_map[m] = 0.0;
    return;
  }
  const int hw = hh * wh;
  const float* hm = h + m * hw;
  const float* gm = POINTS ? nullptr : g + m * hw;
  const bool vec = (hw & 3) == 0 && (((uintptr_t)hm | (uintptr_t)gm) & 15) == 0;
  double px = 0.0, py = 0.0;
  if (POINTS) {
    px = pt[m * 2];
    py = pt[m * 2 + 1];
    if (sig) two_s2 = __dmul_rn(2.0, __dmul_rn(sig[m], sig[m]));
  }
  double acc = 0.0;
  for (int p = threadIdx.x * 4; p < hw; p += FL_THREADS * 4) {
    const float4 a = fl_load4(hm, p, hw, vec);
    const float4 b = fl_truth4<POINTS>(gm, p, hw, wh, vec, px, py, two_s2);
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    // (double)(d * d): the float32 square is rounded on its own, nothing to contract into an fma (mse_partial_kernel)
    acc += (double)(d0 * d0) + (double)(d1 * d1) + (double)(d2 * d2) + (double)(d3 * d3);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) per_map[m] = (red[0] + red[1]) + (red[2] + red[3]);
}

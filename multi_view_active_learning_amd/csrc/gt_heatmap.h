// One pixel of a Gaussian ground-truth heat-map (dataset.py:198-207), shared by the kernel that writes the maps
// (preprocess.hip, mval_gt_heatmaps) and the one that only compares against them (frame_loss.hip,
// mval_frame_loss_points): both must give the same bits.
#pragma once
#include <hip/hip_runtime.h>

// (float) exp(-((x - px)^2 + (y - py)^2) / (2 sigma^2)): float64, each operation rounded separately, as torch
// evaluates sum((grid - labels) ** 2) / (2 sigma^2).  two_s2 = 2.0 * (sigma * sigma), computed by the host.
__device__ __forceinline__ float mval_gt_heatmap_pixel(int x, int y, double px, double py, double two_s2) {
  const double dx = (double)x - px, dy = (double)y - py;
  return (float)exp(-__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) / two_s2);
}

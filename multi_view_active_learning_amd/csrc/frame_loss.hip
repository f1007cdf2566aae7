// Per-frame heat-map loss of a whole batch (the CLUSTER pass, reference strategy.py:173-187):
//   out[b] = sum over the maps m of frame b with valid[m] != 0 of sum over pixels (h - g)^2 / (hh * wh)
// = pose_2d_mse_single_batch (pose_estimators/loss.py:22-24) of every frame at once.  g is read
// (mval_frame_loss) or rendered from the joint's pixel position (mval_frame_loss_points, the expression of
// mval_gt_heatmaps: gt_heatmap.h), so the two forms give the same bits.
//
//   kernel 1  frame_loss_map_kernel (frame_loss_map.h, shared with the weighted training loss), one workgroup per map:
//             d = h - g and d * d in float32 (torch's (h - gt) ** 2), summed in float64 ->
//             per_map[m], the map's sum of squared errors (0 for a masked map, which is not read)
//   kernel 2  one thread per frame: its per_map entries added in ascending map order, / (hh * wh) in float64,
//             rounded to float32 once
// No atomics and a fixed pixel -> lane assignment: a frame's bits do not depend on the batch around it.  The
// assignment is the same whether the maps can be loaded as float4 or not (an unaligned base, hh * wh % 4 != 0):
// lane t adds the groups of four pixels t, t + 256, ..., a short last group padded with zeros.
// HBM-bound: 2 * n * hh * wh * 4 bytes per call (half that for the points form, which pays a float64 exp per pixel).
#include "frame_loss_map.h"

__global__ __launch_bounds__(MVAL_WAVE) void frame_loss_sum_kernel(const double* __restrict__ per_map, float* __restrict__ out,
                                                                   int64_t n_frames, int maps_per_frame, double pixels) {
  const int64_t b = (int64_t)blockIdx.x * MVAL_WAVE + threadIdx.x;
  if (b >= n_frames) return;
  const double* p = per_map + b * maps_per_frame;
  double acc = 0.0;
  for (int m = 0; m < maps_per_frame; m++) acc += p[m];
  out[b] = (float)(acc / pixels);
}

extern "C" size_t mval_frame_loss_workspace_bytes(int64_t n_frames, int maps_per_frame) {
  if (n_frames <= 0 || maps_per_frame <= 0) return 0;
  return (size_t)n_frames * (size_t)maps_per_frame * sizeof(double);
}

template <bool POINTS>
static int frame_loss_launch(const char* name, const float* h, const float* g, const double* pt, double sigma,
                             const uint8_t* valid, float* out, double* per_map, int64_t n_frames, int maps_per_frame, int hh,
                             int wh, void* stream) {
  MVAL_REQUIRE(n_frames >= 0 && maps_per_frame > 0 && hh > 0 && wh > 0 && (int64_t)hh * wh <= INT32_MAX - 4 * FL_THREADS,
               "%s: bad dims", name);
  MVAL_REQUIRE(n_frames * maps_per_frame <= INT32_MAX, "%s: %lld maps exceed one launch", name,
               (long long)(n_frames * maps_per_frame));
  if (n_frames == 0) return 0;
  MVAL_REQUIRE(h && (POINTS ? (const void*)pt : (const void*)g) && out && per_map, "%s: null argument", name);
  MVAL_REQUIRE(!POINTS || sigma > 0, "%s: sigma must be positive", name);
  hipStream_t s = mval_stream(stream);
  hipLaunchKernelGGL((frame_loss_map_kernel<POINTS>), dim3((unsigned)(n_frames * maps_per_frame)), dim3(FL_THREADS), 0, s, h, g,
                     pt, 2.0 * (sigma * sigma), (const double*)nullptr, valid, (const float*)nullptr, per_map, hh, wh);
  MVAL_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(frame_loss_sum_kernel, dim3((unsigned)((n_frames + MVAL_WAVE - 1) / MVAL_WAVE)), dim3(MVAL_WAVE), 0, s,
                     per_map, out, n_frames, maps_per_frame, (double)hh * (double)wh);
  MVAL_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int mval_frame_loss(const float* heatmaps, const float* gt, const uint8_t* valid, float* out, double* per_map,
                               int64_t n_frames, int maps_per_frame, int hh, int wh, void* stream) {
  return frame_loss_launch<false>("mval_frame_loss", heatmaps, gt, nullptr, 1.0, valid, out, per_map, n_frames,
                                  maps_per_frame, hh, wh, stream);
}

extern "C" int mval_frame_loss_points(const float* heatmaps, const double* pt, double sigma, const uint8_t* valid, float* out,
                                      double* per_map, int64_t n_frames, int maps_per_frame, int hh, int wh, void* stream) {
  return frame_loss_launch<true>("mval_frame_loss_points", heatmaps, nullptr, pt, sigma, valid, out, per_map, n_frames,
                                 maps_per_frame, hh, wh, stream);
}

// Per-frame heat-map loss of a whole batch (the CLUSTER pass, reference strategy.py:173-187):
//   out[b] = sum over the maps m of frame b with valid[m] != 0 of sum over pixels (h - g)^2 / (hh * wh)
// = pose_2d_mse_single_batch (pose_estimators/loss.py:22-24) of every frame at once.  g is read
// (mval_frame_loss) or rendered from the joint's pixel position (mval_frame_loss_points, the expression of
// mval_gt_heatmaps: gt_heatmap.h), so the two forms give the same bits.
//
//   kernel 1  one workgroup per map: d = h - g and d * d in float32 (torch's (h - gt) ** 2), summed in float64 ->
//             per_map[m], the map's sum of squared errors (0 for a masked map, which is not read)
//   kernel 2  one thread per frame: its per_map entries added in ascending map order, / (hh * wh) in float64,
//             rounded to float32 once
// No atomics and a fixed pixel -> lane assignment: a frame's bits do not depend on the batch around it.  The
// assignment is the same whether the maps can be loaded as float4 or not (an unaligned base, hh * wh % 4 != 0):
// lane t adds the groups of four pixels t, t + 256, ..., a short last group padded with zeros.
// HBM-bound: 2 * n * hh * wh * 4 bytes per call (half that for the points form, which pays a float64 exp per pixel).
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

template <bool POINTS>
__global__ __launch_bounds__(FL_THREADS) void frame_loss_map_kernel(const float* __restrict__ h, const float* __restrict__ g,
                                                                    const double* __restrict__ pt, double two_s2,
                                                                    const uint8_t* __restrict__ valid,
                                                                    double* __restrict__ per_map, int hh, int wh) {
  __shared__ double red[FL_THREADS / MVAL_WAVE];
  const int64_t m = blockIdx.x;
  if (valid && !valid[m]) {  // (uniform over the workgroup)
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
  }
  double acc = 0.0;
  for (int p = threadIdx.x * 4; p < hw; p += FL_THREADS * 4) {
    const float4 a = fl_load4(hm, p, hw, vec);
    float4 b;
    if (POINTS) {
      b.x = fl_render(p, hw, wh, px, py, two_s2);
      b.y = fl_render(p + 1, hw, wh, px, py, two_s2);
      b.z = fl_render(p + 2, hw, wh, px, py, two_s2);
      b.w = fl_render(p + 3, hw, wh, px, py, two_s2);
    } else {
      b = fl_load4(gm, p, hw, vec);
    }
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    // (double)(d * d): the float32 square is rounded on its own, nothing to contract into an fma (mse_partial_kernel)
    acc += (double)(d0 * d0) + (double)(d1 * d1) + (double)(d2 * d2) + (double)(d3 * d3);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) per_map[m] = (red[0] + red[1]) + (red[2] + red[3]);
}

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
                     pt, 2.0 * (sigma * sigma), valid, per_map, hh, wh);
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

// Weighted training loss with online hard key-point mining (no counterpart in the reference):
//   S[m]    = sum over the pixels of map m of (h - g)^2           float32 squares, float64 sum (frame_loss_map.h)
//   l[m]    = (double)w[m] * S[m]                                  per_map, one rounding
//   per image n: its J values l[n, .] ranked in the order of argmax_better (numeric_order.h: NaN first, ties to the lowest
//           joint); the first topk are selected (topk == 0: all); wsel[m] = selected ? w[m] : 0
//   T[n]    = sum of the selected l[n, j], ascending j, sequential float64
//   loss    = (float)((sum of T[n], ascending n, sequential float64) / (N * hh * wh))
//   grad_h  = ((2 (h - g)) * (grad_out / (float)(N * hh * wh))) * wsel[m], every product rounded on its own
// g is read (mval_weighted_mse_fwd / _bwd) or rendered from the joint's pixel position (mval_weighted_mse_points_fwd / _bwd, the
// expression of mval_gt_heatmaps: gt_heatmap.h) under a scalar sigma or one per map.  A map with w == 0 (forward) or wsel == 0
// (backward) is neither read nor rendered: S = +0.0, grad_h = +0.0f.
//
//   kernel A  frame_loss_map_kernel (frame_loss_map.h, shared with mval_frame_loss): one workgroup per map -> S
//   kernel B  one wave per image: l, ranks by counting (J^2 compares per image), wsel, T[n]
//   kernel B' one wave: the T[n] added in ascending n -> loss
//   kernel C  backward, workgroups stride over the maps, float4 where a map allows it
// No atomics; the bits of T[n] do not depend on the other images of the batch.
// HBM-bound: forward 2 * lead * hh * wh * 4 bytes read (half that for the points form), backward the same read plus
// lead * hh * wh * 4 written; maps that do not count are skipped.
#include "frame_loss_map.h"
#include "numeric_order.h"

#define WL_THREADS 256

// lanes of a wave take the joints j0 + lane of image n in chunks of 64; lane 0 adds each chunk's selected terms in order
__global__ __launch_bounds__(MVAL_WAVE) void weighted_select_kernel(const double* __restrict__ S, const float* __restrict__ w,
                                                                    int topk, double* __restrict__ per_map,
                                                                    float* __restrict__ wsel, double* __restrict__ T, int J) {
  __shared__ double term[MVAL_WAVE];
  __shared__ uint8_t picked[MVAL_WAVE];
  const int64_t base = (int64_t)blockIdx.x * J;
  double acc = 0.0;
  for (int j0 = 0; j0 < J; j0 += MVAL_WAVE) {
    const int j = j0 + threadIdx.x;
    if (j < J) {
      const float wj = w[base + j];
      const double lj = __dmul_rn((double)wj, S[base + j]);
      int rank = 0;  // how many joints of this image come before j
      if (topk > 0)
        for (int k = 0; k < J; k++) rank += k != j && argmax_better(__dmul_rn((double)w[base + k], S[base + k]), k, lj, j);
      const bool sel = topk == 0 || rank < topk;
      per_map[base + j] = lj;
      wsel[base + j] = sel ? wj : 0.0f;
      term[threadIdx.x] = lj;
      picked[threadIdx.x] = sel;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = J - j0 < MVAL_WAVE ? J - j0 : MVAL_WAVE;
      for (int k = 0; k < n; k++)
        if (picked[k]) acc = __dadd_rn(acc, term[k]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) T[blockIdx.x] = acc;
}

__global__ __launch_bounds__(MVAL_WAVE) void weighted_total_kernel(const double* __restrict__ T, float* __restrict__ out,
                                                                   int64_t n_images, double denom) {
  __shared__ double part[MVAL_WAVE];
  double acc = 0.0;
  for (int64_t n0 = 0; n0 < n_images; n0 += MVAL_WAVE) {
    if (n0 + threadIdx.x < n_images) part[threadIdx.x] = T[n0 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = n_images - n0 < MVAL_WAVE ? (int)(n_images - n0) : MVAL_WAVE;
      for (int k = 0; k < n; k++) acc = __dadd_rn(acc, part[k]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = n_images > 0 ? (float)(acc / denom) : 0.0f;
}

__device__ __forceinline__ float wl_grad(float a, float b, float gs, float ws) {
  return __fmul_rn(__fmul_rn(__fmul_rn(2.0f, __fsub_rn(a, b)), gs), ws);
}

template <bool POINTS>
__global__ __launch_bounds__(WL_THREADS) void weighted_bwd_kernel(const float* __restrict__ h, const float* __restrict__ g,
                                                                  const double* __restrict__ pt, double two_s2,
                                                                  const double* __restrict__ sig, const float* __restrict__ wsel,
                                                                  const float* __restrict__ grad_out, float* __restrict__ gh,
                                                                  int64_t lead, int hh, int wh, float denom) {
  const float gs = grad_out[0] / denom;  // d(sum/denom), as mse_bwd_kernel forms it
  const int hw = hh * wh;
  for (int64_t m = blockIdx.x; m < lead; m += gridDim.x) {
    const float ws = wsel[m];  // (uniform over the workgroup)
    const float* hm = h + m * hw;
    const float* gm = POINTS ? nullptr : g + m * hw;
    float* om = gh + m * hw;
    const bool skip = ws == 0.f;
    // the stores are float4 where the output allows it, the loads where the inputs do too
    const bool vec_out = (hw & 3) == 0 && ((uintptr_t)om & 15) == 0;
    const bool vec = vec_out && (((uintptr_t)hm | (uintptr_t)gm) & 15) == 0;
    double px = 0.0, py = 0.0, t = two_s2;
    if (POINTS && !skip) {
      px = pt[m * 2];
      py = pt[m * 2 + 1];
      if (sig) t = __dmul_rn(2.0, __dmul_rn(sig[m], sig[m]));
    }
    for (int p = threadIdx.x * 4; p < hw; p += WL_THREADS * 4) {
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!skip) {
        const float4 a = fl_load4(hm, p, hw, vec);
        const float4 b = fl_truth4<POINTS>(gm, p, hw, wh, vec, px, py, t);
        r.x = wl_grad(a.x, b.x, gs, ws);
        r.y = wl_grad(a.y, b.y, gs, ws);
        r.z = wl_grad(a.z, b.z, gs, ws);
        r.w = wl_grad(a.w, b.w, gs, ws);
      }
      if (vec_out) {
        *reinterpret_cast<float4*>(om + p) = r;
      } else {
        om[p] = r.x;
        if (p + 1 < hw) om[p + 1] = r.y;
        if (p + 2 < hw) om[p + 2] = r.z;
        if (p + 3 < hw) om[p + 3] = r.w;
      }
    }
  }
}

extern "C" size_t mval_weighted_mse_workspace_bytes(int64_t n_images, int n_joints) {
  if (n_images <= 0 || n_joints <= 0) return 0;
  return ((size_t)n_images * (size_t)n_joints + (size_t)n_images) * sizeof(double);  // S [lead], T [n_images]
}

// The checks the four entries share; the points forms add MSE_POINTS_REQUIRE's (loss_metric.hip) on sigma.
#define WL_REQUIRE_DIMS(name)                                                                                           \
  do {                                                                                                                  \
    MVAL_REQUIRE(n_images >= 0 && n_joints > 0 && hh > 0 && wh > 0, "%s: bad dims", name);                              \
    MVAL_REQUIRE((int64_t)hh * wh <= INT32_MAX - 4 * FL_THREADS, "%s: a map of %d x %d exceeds one launch", name, hh, wh); \
    MVAL_REQUIRE(n_images <= INT32_MAX / n_joints, "%s: %lld x %d maps exceed one launch", name, (long long)n_images,   \
                 n_joints);                                                                                             \
    MVAL_REQUIRE(n_images * n_joints <= INT64_MAX / ((int64_t)hh * wh), "%s: %lld maps of %d x %d overflow", name,      \
                 (long long)(n_images * n_joints), hh, wh);                                                             \
  } while (0)

template <bool POINTS>
static int weighted_fwd_launch(const char* name, const float* h, const float* g, const double* pt, double sigma,
                               const double* sigma_per_map, const float* weight, int topk, float* out, double* per_map,
                               float* wsel, void* ws, int64_t n_images, int n_joints, int hh, int wh, void* stream) {
  WL_REQUIRE_DIMS(name);
  MVAL_REQUIRE(topk >= 0 && topk <= n_joints, "%s: topk %d is not in [0, %d]", name, topk, n_joints);
  MVAL_REQUIRE(out, "%s: null argument", name);
  MVAL_REQUIRE(n_images == 0 || (h && (POINTS ? (const void*)pt : (const void*)g) && weight && per_map && wsel && ws),
               "%s: null argument", name);
  MVAL_REQUIRE(!POINTS || sigma_per_map || sigma > 0, "%s: sigma must be positive", name);
  hipStream_t s = mval_stream(stream);
  double* S = reinterpret_cast<double*>(ws);
  double* T = S + n_images * n_joints;
  if (n_images > 0) {
    hipLaunchKernelGGL((frame_loss_map_kernel<POINTS>), dim3((unsigned)(n_images * n_joints)), dim3(FL_THREADS), 0, s, h, g, pt,
                       2.0 * (sigma * sigma), sigma_per_map, (const uint8_t*)nullptr, weight, S, hh, wh);
    MVAL_CHECK_LAUNCH_STAGE(name, "/maps");
    hipLaunchKernelGGL(weighted_select_kernel, dim3((unsigned)n_images), dim3(MVAL_WAVE), 0, s, S, weight, topk, per_map, wsel, T,
                       n_joints);
    MVAL_CHECK_LAUNCH_STAGE(name, "/select");
  }
  hipLaunchKernelGGL(weighted_total_kernel, dim3(1), dim3(MVAL_WAVE), 0, s, T, out, n_images,
                     (double)n_images * (double)hh * (double)wh);
  MVAL_CHECK_LAUNCH_STAGE(name, "/total");
  return 0;
}

template <bool POINTS>
static int weighted_bwd_launch(const char* name, const float* h, const float* g, const double* pt, double sigma,
                               const double* sigma_per_map, const float* wsel, const float* grad_out, float* grad_h,
                               int64_t n_images, int n_joints, int hh, int wh, void* stream) {
  WL_REQUIRE_DIMS(name);
  MVAL_REQUIRE(n_images == 0 || (h && (POINTS ? (const void*)pt : (const void*)g) && wsel && grad_out && grad_h),
               "%s: null argument", name);
  MVAL_REQUIRE(!POINTS || sigma_per_map || sigma > 0, "%s: sigma must be positive", name);
  if (n_images == 0) return 0;
  const int64_t lead = n_images * n_joints;
  hipLaunchKernelGGL((weighted_bwd_kernel<POINTS>), dim3((unsigned)(lead < 65536 ? lead : 65536)), dim3(WL_THREADS), 0,
                     mval_stream(stream), h, g, pt, 2.0 * (sigma * sigma), sigma_per_map, wsel, grad_out, grad_h, lead, hh, wh,
                     (float)((double)n_images * (double)hh * (double)wh));
  MVAL_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int mval_weighted_mse_fwd(const float* h, const float* g, const float* weight, int topk, float* out, double* per_map,
                                     float* wsel, void* ws, int64_t n_images, int n_joints, int hh, int wh, void* stream) {
  return weighted_fwd_launch<false>("mval_weighted_mse_fwd", h, g, nullptr, 1.0, nullptr, weight, topk, out, per_map, wsel, ws,
                                    n_images, n_joints, hh, wh, stream);
}

extern "C" int mval_weighted_mse_points_fwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                                            const float* weight, int topk, float* out, double* per_map, float* wsel, void* ws,
                                            int64_t n_images, int n_joints, int hh, int wh, void* stream) {
  return weighted_fwd_launch<true>("mval_weighted_mse_points_fwd", h, nullptr, pt, sigma, sigma_per_map, weight, topk, out,
                                   per_map, wsel, ws, n_images, n_joints, hh, wh, stream);
}

extern "C" int mval_weighted_mse_bwd(const float* h, const float* g, const float* wsel, const float* grad_out, float* grad_h,
                                     int64_t n_images, int n_joints, int hh, int wh, void* stream) {
  return weighted_bwd_launch<false>("mval_weighted_mse_bwd", h, g, nullptr, 1.0, nullptr, wsel, grad_out, grad_h, n_images,
                                    n_joints, hh, wh, stream);
}

extern "C" int mval_weighted_mse_points_bwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                                            const float* wsel, const float* grad_out, float* grad_h, int64_t n_images,
                                            int n_joints, int hh, int wh, void* stream) {
  return weighted_bwd_launch<true>("mval_weighted_mse_points_bwd", h, nullptr, pt, sigma, sigma_per_map, wsel, grad_out, grad_h,
                                   n_images, n_joints, hh, wh, stream);
}

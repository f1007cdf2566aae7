// Masked heat-map MSE (K8, reference pose_estimators/loss.py:14-20) forward/backward and
// MKPE / MPJPE (K15, reference utils/evaluation.py:198-208).  HBM-bound streaming kernels.
// The MSE kernels take the ground truth either from memory (mval_masked_mse_fwd/_bwd) or render it per pixel from the
// joint's position (mval_masked_mse_points_fwd/_bwd: the expression of mval_gt_heatmaps, gt_heatmap.h).  Both forms are
// one template, so grid, element -> thread map and accumulation order are the same by construction and the points form
// has the read form's bits on the maps mval_gt_heatmaps writes.
#include "mval_common.h"
#include "gt_heatmap.h"

#define MSE_BLOCKS 1024

// Where the ground truth of the points form comes from: pt [lead][2] f64, and 2 sigma^2 of map m -- from sig[m] where sig
// is given (2.0 * (s * s), each product rounded on its own, as the host forms two_s2 for mval_gt_heatmaps), else two_s2.
struct MsePoints {
  const double* pt;
  const double* sig;
  double two_s2;
  int wh;
};

__device__ __forceinline__ double mse_two_s2(const MsePoints& q, int64_t m) {
  return q.sig ? __dmul_rn(2.0, __dmul_rn(q.sig[m], q.sig[m])) : q.two_s2;
}

// pixel p of map m
__device__ __forceinline__ float mse_render(const MsePoints& q, int p, double px, double py, double two_s2) {
  return mval_gt_heatmap_pixel(p % q.wh, p / q.wh, px, py, two_s2);
}

template <bool POINTS>
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ h, const float* __restrict__ g,
                                                          const MsePoints q, const uint8_t* __restrict__ valid,
                                                          double* __restrict__ ws, int64_t lead, int64_t hw) {
  __shared__ double red[4];
  double acc = 0.0;
  const int64_t total = lead * hw;
  const bool vec = (hw & 3) == 0 && (((uintptr_t)h | (uintptr_t)g) & 15) == 0;  // (points form: g == nullptr)
  if (vec) {
    const int64_t n4 = total >> 2;
    const float4* h4 = reinterpret_cast<const float4*>(h);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      if (valid && !valid[(i << 2) / hw]) continue;  // a masked map is neither read nor rendered
      float4 a = h4[i], b;
      if (POINTS) {
        const int64_t m = (i << 2) / hw;  // hw % 4 == 0: the four pixels are of one map
        const int p = (int)((i << 2) - m * hw);
        const double px = q.pt[m * 2], py = q.pt[m * 2 + 1], t = mse_two_s2(q, m);
        b.x = mse_render(q, p, px, py, t);
        b.y = mse_render(q, p + 1, px, py, t);
        b.z = mse_render(q, p + 2, px, py, t);
        b.w = mse_render(q, p + 3, px, py, t);
      } else {
        b = g4[i];
      }
      float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
      acc += (double)(d0 * d0) + (double)(d1 * d1) + (double)(d2 * d2) + (double)(d3 * d3);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      if (valid && !valid[i / hw]) continue;
      float b;
      if (POINTS) {
        const int64_t m = i / hw;
        b = mse_render(q, (int)(i - m * hw), q.pt[m * 2], q.pt[m * 2 + 1], mse_two_s2(q, m));
      } else {
        b = g[i];
      }
      float d = h[i] - b;
      acc += (double)(d * d);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void mse_final_kernel(const double* __restrict__ ws, float* __restrict__ out, int nb,
                                                        double denom) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += ws[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / denom);
}

template <bool POINTS>
static int mse_fwd_launch(const char* name, const float* h, const float* g, const MsePoints& q, const uint8_t* valid,
                          float* out, double* ws, int64_t lead, int64_t hw, double denom, void* stream) {
  int64_t total = lead * hw;
  int nb = (int)((total / 4 + 255) / 256);
  if (nb < 1) nb = 1;
  if (nb > MSE_BLOCKS) nb = MSE_BLOCKS;
  hipLaunchKernelGGL((mse_partial_kernel<POINTS>), dim3(nb), dim3(256), 0, mval_stream(stream), h, g, q, valid, ws, lead, hw);
  MVAL_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, mval_stream(stream), ws, out, nb, denom);
  MVAL_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int mval_masked_mse_fwd(const float* h, const float* g, const uint8_t* valid, float* out, double* ws,
                                   int64_t lead, int64_t hw, double denom, void* stream) {
  MVAL_REQUIRE(lead >= 0 && hw > 0 && denom != 0.0, "mval_masked_mse_fwd: bad dims");
  return mse_fwd_launch<false>("mval_masked_mse_fwd", h, g, MsePoints{nullptr, nullptr, 0.0, 0}, valid, out, ws, lead, hw, denom,
                               stream);
}

template <bool POINTS>
__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ h, const float* __restrict__ g,
                                                      const MsePoints q, const uint8_t* __restrict__ valid,
                                                      const float* __restrict__ grad_out, float* __restrict__ gh,
                                                      int64_t lead, int64_t hw, float denom) {
  const float gs = grad_out[0] / denom;  // d(sum/denom)
  const int64_t total = lead * hw;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    bool ok = !valid || valid[i / hw];
    if (POINTS) {  // rendered again, not kept from the forward; a masked map is not rendered
      float r = 0.0f;
      if (ok) {
        const int64_t m = i / hw;
        float d = h[i] - mse_render(q, (int)(i - m * hw), q.pt[m * 2], q.pt[m * 2 + 1], mse_two_s2(q, m));
        r = (2.0f * d) * gs;
      }
      gh[i] = r;
    } else {
      float d = h[i] - g[i];
      gh[i] = ok ? (2.0f * d) * gs : 0.0f;
    }
  }
}

template <bool POINTS>
static int mse_bwd_launch(const char* name, const float* h, const float* g, const MsePoints& q, const uint8_t* valid,
                          const float* grad_out, float* grad_h, int64_t lead, int64_t hw, double denom, void* stream) {
  int64_t total = lead * hw;
  if (total == 0) return 0;
  int nb = (int)((total + 255) / 256);
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL((mse_bwd_kernel<POINTS>), dim3(nb), dim3(256), 0, mval_stream(stream), h, g, q, valid, grad_out, grad_h,
                     lead, hw, (float)denom);
  MVAL_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int mval_masked_mse_bwd(const float* h, const float* g, const uint8_t* valid, const float* grad_out,
                                   float* grad_h, int64_t lead, int64_t hw, double denom, void* stream) {
  MVAL_REQUIRE(lead >= 0 && hw > 0 && denom != 0.0, "mval_masked_mse_bwd: bad dims");
  return mse_bwd_launch<false>("mval_masked_mse_bwd", h, g, MsePoints{nullptr, nullptr, 0.0, 0}, valid, grad_out, grad_h, lead, hw,
                               denom, stream);
}

// The points form.  A map's pixel index is an int and lead * hh * wh must not overflow; sigma_per_map lives on the device
// and cannot be looked at here without a synchronise: its callers check it where it still is on the host (_lib.py).
#define MSE_POINTS_REQUIRE(name)                                                                                         \
  do {                                                                                                                   \
    MVAL_REQUIRE(lead >= 0 && hh > 0 && wh > 0 && denom != 0.0, name ": bad dims");                                      \
    MVAL_REQUIRE((int64_t)hh * wh <= INT32_MAX - 4 * 256, name ": a map of %d x %d exceeds one launch", hh, wh);         \
    MVAL_REQUIRE(lead <= INT64_MAX / ((int64_t)hh * wh), name ": %lld maps of %d x %d overflow", (long long)lead, hh, wh); \
    MVAL_REQUIRE(sigma_per_map || sigma > 0, name ": sigma must be positive");                                           \
  } while (0)

extern "C" int mval_masked_mse_points_fwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                                          const uint8_t* valid, float* out, double* ws, int64_t lead, int hh, int wh,
                                          double denom, void* stream) {
  MSE_POINTS_REQUIRE("mval_masked_mse_points_fwd");
  MVAL_REQUIRE(out && ws && (lead == 0 || (h && pt)), "mval_masked_mse_points_fwd: null argument");
  return mse_fwd_launch<true>("mval_masked_mse_points_fwd", h, nullptr, MsePoints{pt, sigma_per_map, 2.0 * (sigma * sigma), wh},
                              valid, out, ws, lead, (int64_t)hh * wh, denom, stream);
}

extern "C" int mval_masked_mse_points_bwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                                          const uint8_t* valid, const float* grad_out, float* grad_h, int64_t lead, int hh,
                                          int wh, double denom, void* stream) {
  MSE_POINTS_REQUIRE("mval_masked_mse_points_bwd");
  MVAL_REQUIRE(lead == 0 || (h && pt && grad_out && grad_h), "mval_masked_mse_points_bwd: null argument");
  return mse_bwd_launch<true>("mval_masked_mse_points_bwd", h, nullptr, MsePoints{pt, sigma_per_map, 2.0 * (sigma * sigma), wh},
                              valid, grad_out, grad_h, lead, (int64_t)hh * wh, denom, stream);
}

// ---- MKPE ------------------------------------------------------------------------------
// d_sj = sqrt(sum_c valid ? (pred[s,j,c] - gt[s,c,j])^2 : 0)   (float32, c = 0,1,2 in order)
__device__ __forceinline__ float mkpe_d(const float* pred, const float* gt, const float* valid, int64_t s, int j,
                                        int J, int gt_rows) {
  bool ok = valid[s * J + j] != 0.0f;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float d = pred[(s * J + j) * 3 + c] - gt[(s * gt_rows + c) * J + j];
    acc += ok ? d * d : 0.f;
  }
  return sqrtf(acc);
}

__global__ void mkpe_per_sample_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                       const float* __restrict__ valid, float* __restrict__ per_sample, int64_t S,
                                       int J, int gt_rows) {
  int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  float acc = 0.f;
  for (int j = 0; j < J; j++) acc += mkpe_d(pred, gt, valid, s, j, J, gt_rows) / valid[s * J + j];  // 0/0 -> NaN
  per_sample[s] = acc / (float)J;
}

__global__ void mkpe_total_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                  const float* __restrict__ valid, float* __restrict__ out, int64_t S, int J,
                                  int gt_rows) {
  __shared__ float mk[1024];
  int j = threadIdx.x;
  if (j < J) {
    float kpe = 0.f, cnt = 0.f;  // kpe = kpe + d ; count = count + valid  (sample order)
    for (int64_t s = 0; s < S; s++) {
      kpe += mkpe_d(pred, gt, valid, s, j, J, gt_rows);
      cnt += valid[s * J + j];
    }
    mk[j] = kpe / cnt;
  }
  __syncthreads();
  if (j == 0) {
    float acc = 0.f;
    for (int k = 0; k < J; k++) acc += mk[k];
    out[0] = acc / (float)J;
  }
}

extern "C" int mval_mkpe(const float* pred, const float* gt, const float* valid, float* out, float* per_sample,
                         int64_t S, int J, int gt_rows, void* stream) {
  MVAL_REQUIRE(S >= 0 && J > 0 && J <= 1024 && gt_rows >= 3, "mval_mkpe: bad dims");
  if (S > 0 && per_sample) {
    hipLaunchKernelGGL(mkpe_per_sample_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, mval_stream(stream), pred,
                       gt, valid, per_sample, S, J, gt_rows);
    MVAL_CHECK_LAUNCH("mval_mkpe/per_sample");
  }
  if (out) {
    hipLaunchKernelGGL(mkpe_total_kernel, dim3(1), dim3(((J + 63) / 64) * 64), 0, mval_stream(stream), pred, gt, valid,
                       out, S, J, gt_rows);
    MVAL_CHECK_LAUNCH("mval_mkpe/total");
  }
  return 0;
}

// ---- 3-D PCK / PCKh --------------------------------------------------------------------------
// utils/evaluation.py:150-195 (compute_3d_pckh / compute_3d_pck), the counters of _evaluate_all
// (strategy.py:638-649).  Distances are float32 with torch's operation order -- ((dx^2 + dy^2) + dz^2),
// every operation rounded separately (no FMA contraction), then sqrt -- because the result is an
// integer count of strict `<` comparisons:
//   mode 0 (PCK):  valid joints only; hit when (double)dis < threshold[t]; counts[j] = #valid samples
//   mode 1 (PCKh): every joint; hit when dis < (float32)(head * (float)threshold[t]) with head = the
//                  distance between gt joints 0 and 1; counts[j] = S
// One workgroup per (threshold, joint); integer sums, so the result is order-independent.
__device__ __forceinline__ float pck_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

__global__ __launch_bounds__(256) void pck3d_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                    const float* __restrict__ valid,
                                                    const double* __restrict__ thresholds, int mode,
                                                    long long* __restrict__ hits, long long* __restrict__ counts,
                                                    int64_t S, int J, int gt_rows) {
  __shared__ long long sh[2][256];
  const int j = blockIdx.x, t = blockIdx.y;
  const double thr = thresholds[t];
  long long h = 0, c = 0;
  for (int64_t s = threadIdx.x; s < S; s += 256) {
    const float* g = gt + s * gt_rows * J;
    const float* pr = pred + (s * J + j) * 3;
    if (mode == 0 && valid[s * J + j] == 0.0f) continue;
    const float dis = pck_dist(pr[0], pr[1], pr[2], g[j], g[J + j], g[2 * J + j]);
    c++;
    if (mode == 0) {
      h += (double)dis < thr;
    } else {
      const float head = pck_dist(g[0], g[J], g[2 * J], g[1], g[J + 1], g[2 * J + 1]);
      h += dis < __fmul_rn(head, (float)thr);
    }
  }
  sh[0][threadIdx.x] = h;
  sh[1][threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    hits[(int64_t)t * J + j] = sh[0][0];
    if (t == 0) counts[j] = sh[1][0];
  }
}

extern "C" int mval_pck3d(const float* pred, const float* gt, const float* valid, const double* thresholds, int T,
                          int mode, long long* hits, long long* counts, int64_t S, int J, int gt_rows, void* stream) {
  MVAL_REQUIRE(pred && gt && thresholds && hits && counts && S >= 0 && J >= 2 && T > 0 && gt_rows >= 3 &&
                   (mode == 1 || (mode == 0 && valid)),
               "mval_pck3d: bad arguments");
  hipLaunchKernelGGL(pck3d_kernel, dim3(J, T), dim3(256), 0, mval_stream(stream), pred, gt, valid, thresholds, mode, hits,
                     counts, S, J, gt_rows);
  MVAL_CHECK_LAUNCH("mval_pck3d");
  return 0;
}

// ---- 2-D PCKh --------------------------------------------------------------------------------
// utils/evaluation.py:65-93 (compute_pckh), the counter of _evaluate_2d_pckh (strategy.py:548-582).  float32 with torch's
// operation order, every operation rounded separately, as above:
//   head = sqrt((g[kp0].x - g[kp1].x)^2 + (g[kp0].y - g[kp1].y)^2) ; d = (float32)(head * (float)threshold[t])
//   dis  = sqrt((p.x - g.x)^2 + (p.y - g.y)^2) ; hit when dis < d (strict; a NaN on either side is no hit)
// over every image and every joint below n_keypoints (the reference has no validity mask here).  Laid out as pck3d_kernel:
// one workgroup per (joint, threshold), each thread walks the samples in steps of 256; integer sums.
__device__ __forceinline__ float pck_dist2(float ax, float ay, float bx, float by) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by);
  return __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
}

__global__ __launch_bounds__(256) void pckh2d_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const double* __restrict__ thresholds, int kp0, int kp1,
                                                     long long* __restrict__ hits, int64_t S, int J, int n_keypoints) {
  __shared__ long long sh[256];
  const int j = blockIdx.x, t = blockIdx.y;
  const float thr = (float)thresholds[t];
  long long h = 0;
  for (int64_t s = threadIdx.x; s < S; s += 256) {
    const float* g = gt + s * J * 2;
    const float* pr = pred + (s * J + j) * 2;
    const float head = pck_dist2(g[2 * kp0], g[2 * kp0 + 1], g[2 * kp1], g[2 * kp1 + 1]);
    h += pck_dist2(pr[0], pr[1], g[2 * j], g[2 * j + 1]) < __fmul_rn(head, thr);
  }
  sh[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) hits[(int64_t)t * n_keypoints + j] = sh[0];
}

extern "C" int mval_pckh2d(const float* pred, const float* gt, const double* thresholds, int T, int kp0, int kp1,
                           long long* hits, int64_t S, int J, int n_keypoints, void* stream) {
  MVAL_REQUIRE(S >= 0 && J >= 2 && T > 0 && T <= 65535 && kp0 >= 0 && kp0 < J && kp1 >= 0 && kp1 < J && n_keypoints >= 1 &&
                   n_keypoints <= J,
               "mval_pckh2d: bad arguments (S %lld, J %d, T %d, kp0 %d, kp1 %d, n_keypoints %d)", (long long)S, J, T, kp0, kp1,
               n_keypoints);
  MVAL_REQUIRE(thresholds && hits && (S == 0 || (pred && gt)), "mval_pckh2d: pred, gt, thresholds and hits must not be NULL");
  hipLaunchKernelGGL(pckh2d_kernel, dim3(n_keypoints, T), dim3(256), 0, mval_stream(stream), pred, gt, thresholds, kp0, kp1,
                     hits, S, J, n_keypoints);
  MVAL_CHECK_LAUNCH("mval_pckh2d");
  return 0;
}

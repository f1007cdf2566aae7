// Keypoint decode kernels: hard arg-max (K9) and soft-arg-max (K10).
// HBM-bound: each heat-map is read exactly once (J*hh*wh*4 bytes per frame x view).
// One 64-lane wave per map, float4 loads, wave reduction with first-index tie-break.
#include "mval_common.h"
#include "numeric_order.h"  // argmax_better: torch.argmax's order

// the flat arg-max of one map by one wave, in every lane
__device__ __forceinline__ int wave_argmax(const float* __restrict__ p, int npix, int lane) {
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  if ((npix & 3) == 0 && ((uintptr_t)p & 15) == 0) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (int i = lane; i < (npix >> 2); i += 64) {
      float4 q = p4[i];
      int base = i << 2;
      if (argmax_better(q.x, base, bv, bi)) { bv = q.x; bi = base; }
      if (argmax_better(q.y, base + 1, bv, bi)) { bv = q.y; bi = base + 1; }
      if (argmax_better(q.z, base + 2, bv, bi)) { bv = q.z; bi = base + 2; }
      if (argmax_better(q.w, base + 3, bv, bi)) { bv = q.w; bi = base + 3; }
    }
  } else {
    for (int i = lane; i < npix; i += 64) {
      float q = p[i];
      if (argmax_better(q, i, bv, bi)) { bv = q; bi = i; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float ov = __shfl_xor(bv, o, 64);
    int oi = __shfl_xor(bi, o, 64);
    if (argmax_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  return bi == 0x7fffffff ? 0 : bi;  // all -inf (argmax_better never fired): first element
}

__global__ __launch_bounds__(256) void argmax_decode_kernel(
    const float* __restrict__ hm, const uint8_t* __restrict__ valid, int64_t* __restrict__ kp2d,
    int64_t n_maps, int V, int J, int npix, int stride, int split_width) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= n_maps) return;
  const int j = (int)(map % J);
  const int64_t b = map / ((int64_t)V * J);
  if (valid && !valid[b * J + j]) {
    if (lane == 0) { kp2d[map * 2] = 0; kp2d[map * 2 + 1] = 0; }
    return;
  }
  const int bi = wave_argmax(hm + map * (int64_t)npix, npix, lane);
  if (lane == 0) {
    kp2d[map * 2] = (int64_t)(bi % split_width) * stride;
    kp2d[map * 2 + 1] = (int64_t)(bi / split_width) * stride;
  }
}

extern "C" int mval_argmax_decode(const float* heatmaps, const uint8_t* valid, int64_t* kp2d, int B, int V,
                                  int J, int hh, int wh, int stride, int split_width, void* stream) {
  MVAL_REQUIRE(B >= 0 && V > 0 && J > 0 && hh > 0 && wh > 0 && split_width > 0, "mval_argmax_decode: bad dims");
  int64_t n_maps = (int64_t)B * V * J;
  if (n_maps == 0) return 0;
  dim3 grid((unsigned)((n_maps + 3) / 4));
  hipLaunchKernelGGL(argmax_decode_kernel, grid, dim3(256), 0, mval_stream(stream), heatmaps, valid, kp2d, n_maps, V,
                     J, hh * wh, stride, split_width);
  MVAL_CHECK_LAUNCH("mval_argmax_decode");
  return 0;
}

// ---- key-points from the arg-max keys the heat-map layer's epilogue kept (mval_common.h) ------------------------------------
// one wave per map: its MVAL_ARGMAX_SLOTS partial keys -> the largest -> the flat arg-max, in every lane
__device__ __forceinline__ unsigned keys_argmax(const unsigned long long* __restrict__ keys, int64_t map, int J, int lane) {
  const int j = (int)(map % J);
  unsigned long long k = 0ull;
  static_assert(MVAL_ARGMAX_SLOTS % 64 == 0, "whole waves over a row");
#pragma unroll
  for (int i = 0; i < MVAL_ARGMAX_SLOTS / 64; i++) {
    const unsigned long long v = keys[((map / J) * MVAL_ARGMAX_SLOTS + i * 64 + lane) * J + j];  // [image][slot][joint]
    k = v > k ? v : k;
  }
  k = mval_key_group_max(k, 32);
  return k == 0ull ? 0u : 0xffffffffu - (unsigned)k;
}

__global__ __launch_bounds__(256) void argmax_from_keys_kernel(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                               int64_t* __restrict__ kp2d, int64_t n_maps, int V, int J, int stride,
                                                               int split_width) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= n_maps) return;
  const int j = (int)(map % J);
  const int64_t b = map / ((int64_t)V * J);
  const unsigned bi = keys_argmax(keys, map, J, lane);
  if (lane != 0) return;
  const bool inval = valid && !valid[b * J + j];
  kp2d[map * 2] = inval ? 0 : (int64_t)(bi % (unsigned)split_width) * stride;
  kp2d[map * 2 + 1] = inval ? 0 : (int64_t)(bi / (unsigned)split_width) * stride;
}

extern "C" int mval_argmax_from_keys(const uint64_t* keys, const uint8_t* valid, int64_t* kp2d, int B, int V, int J, int stride,
                                     int split_width, void* stream) {
  MVAL_REQUIRE(keys && kp2d && B >= 0 && V > 0 && J > 0 && split_width > 0, "mval_argmax_from_keys: bad arguments");
  const int64_t n_maps = (int64_t)B * V * J;
  if (n_maps == 0) return 0;
  hipLaunchKernelGGL(argmax_from_keys_kernel, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, mval_stream(stream),
                     reinterpret_cast<const unsigned long long*>(keys), valid, kp2d, n_maps, V, J, stride, split_width);
  MVAL_CHECK_LAUNCH("mval_argmax_from_keys");
  return 0;
}

// ---- box-scaled key-points (utils/evaluation.py:45-58, the hard arg-max branch of get_pred_coordinates) --------------------
// float32 as torch computes it, every operation rounded on its own (no FMA contraction): the result is compared bit for bit.
// Both quirks of the reference are kept: the flat index is split by shape[2] (= hh) for x AND y, and x is scaled by the
// box's (bottom - top) over wh, y by its (right - left) over hh.
__device__ __forceinline__ void pred_coordinates_put(float* __restrict__ xy, const float* __restrict__ box, unsigned bi, int hh, int wh) {
  xy[0] = __fmul_rn((float)(bi % (unsigned)hh), __fdiv_rn(__fsub_rn(box[3], box[1]), (float)wh));
  xy[1] = __fmul_rn((float)(bi / (unsigned)hh), __fdiv_rn(__fsub_rn(box[2], box[0]), (float)hh));
}

__global__ __launch_bounds__(256) void pred_coordinates_kernel(const float* __restrict__ hm, const float* __restrict__ boxes,
                                                               float* __restrict__ xy, int64_t n_maps, int J, int hh, int wh) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= n_maps) return;
  const int npix = hh * wh;
  const int bi = wave_argmax(hm + map * (int64_t)npix, npix, lane);
  if (lane == 0) pred_coordinates_put(xy + map * 2, boxes + (map / J) * 4, (unsigned)bi, hh, wh);
}

__global__ __launch_bounds__(256) void pred_coordinates_from_keys_kernel(const unsigned long long* __restrict__ keys,
                                                                         const float* __restrict__ boxes, float* __restrict__ xy,
                                                                         int64_t n_maps, int J, int hh, int wh) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= n_maps) return;
  const unsigned bi = keys_argmax(keys, map, J, lane);
  if (lane == 0) pred_coordinates_put(xy + map * 2, boxes + (map / J) * 4, bi, hh, wh);
}

// (a map of 2^24 pixels or more would make (float)(idx / hh) inexact, and hh * wh must fit an int)
#define MVAL_PRED_COORD_DIMS(N, J, hh, wh) ((N) >= 0 && (J) > 0 && (hh) > 0 && (wh) > 0 && (int64_t)(hh) * (wh) < (1 << 24))

extern "C" int mval_pred_coordinates(const float* heatmaps, const float* boxes, float* xy, int64_t N, int J, int hh, int wh,
                                     void* stream) {
  MVAL_REQUIRE(MVAL_PRED_COORD_DIMS(N, J, hh, wh), "mval_pred_coordinates: bad dims");
  const int64_t n_maps = N * J;
  if (n_maps == 0) return 0;
  MVAL_REQUIRE(heatmaps && boxes && xy, "mval_pred_coordinates: heatmaps, boxes and xy must not be NULL");
  MVAL_REQUIRE((n_maps + 3) / 4 <= 0x7fffffff, "mval_pred_coordinates: too many maps");
  hipLaunchKernelGGL(pred_coordinates_kernel, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, mval_stream(stream), heatmaps,
                     boxes, xy, n_maps, J, hh, wh);
  MVAL_CHECK_LAUNCH("mval_pred_coordinates");
  return 0;
}

extern "C" int mval_pred_coordinates_from_keys(const uint64_t* keys, const float* boxes, float* xy, int64_t N, int J, int hh,
                                               int wh, void* stream) {
  MVAL_REQUIRE(MVAL_PRED_COORD_DIMS(N, J, hh, wh), "mval_pred_coordinates_from_keys: bad dims");
  const int64_t n_maps = N * J;
  if (n_maps == 0) return 0;
  MVAL_REQUIRE(keys && boxes && xy, "mval_pred_coordinates_from_keys: keys, boxes and xy must not be NULL");
  MVAL_REQUIRE((n_maps + 3) / 4 <= 0x7fffffff, "mval_pred_coordinates_from_keys: too many maps");
  hipLaunchKernelGGL(pred_coordinates_from_keys_kernel, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, mval_stream(stream),
                     reinterpret_cast<const unsigned long long*>(keys), boxes, xy, n_maps, J, hh, wh);
  MVAL_CHECK_LAUNCH("mval_pred_coordinates_from_keys");
  return 0;
}

// ---- soft-argmax ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void soft_argmax_kernel(const float* __restrict__ hm, float* __restrict__ out,
                                                          int64_t n_maps, int hh, int wh, float scale) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= n_maps) return;
  const int npix = hh * wh;
  const float* p = hm + map * (int64_t)npix;
  float m = -INFINITY;
  for (int i = lane; i < npix; i += 64) m = fmaxf(m, p[i]);
  m = wave_max(m);
  float s = 0.f, sx = 0.f, sy = 0.f;
  for (int i = lane; i < npix; i += 64) {
    float e = expf(p[i] - m);
    int y = i / wh, x = i - y * wh;
    s += e;
    sx += e * (float)x;
    sy += e * (float)y;
  }
  s = wave_sum(s);
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  if (lane == 0) {
    out[map * 2] = (sx / s) * scale;
    out[map * 2 + 1] = (sy / s) * scale;
  }
}

extern "C" int mval_soft_argmax(const float* heatmaps, float* kp2d, int64_t n_maps, int hh, int wh, float scale,
                                void* stream) {
  MVAL_REQUIRE(n_maps >= 0 && hh > 0 && wh > 0, "mval_soft_argmax: bad dims");
  if (n_maps == 0) return 0;
  dim3 grid((unsigned)((n_maps + 3) / 4));
  hipLaunchKernelGGL(soft_argmax_kernel, grid, dim3(256), 0, mval_stream(stream), heatmaps, kp2d, n_maps, hh, wh,
                     scale);
  MVAL_CHECK_LAUNCH("mval_soft_argmax");
  return 0;
}

// ---- peak gate: which maps have a peak of at least min_peak (utils.triangulation.peak_mask) ---------------------------------
// One streaming read of the maps, one wave per map like the decode above.  `x >= min_peak` is false for a NaN, so a map
// of NaNs is absent; the wave-wide OR is a ballot.
__global__ __launch_bounds__(256) void peak_mask_kernel(const float* __restrict__ hm, uint8_t* __restrict__ out, int64_t n_maps,
                                                        int npix, float min_peak) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= n_maps) return;
  const float* p = hm + map * (int64_t)npix;
  bool hit = false;
  if ((npix & 3) == 0 && ((uintptr_t)p & 15) == 0) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (int i = lane; i < (npix >> 2); i += 64) {
      const float4 q = p4[i];
      hit |= (q.x >= min_peak) | (q.y >= min_peak) | (q.z >= min_peak) | (q.w >= min_peak);
    }
  } else {
    for (int i = lane; i < npix; i += 64) hit |= p[i] >= min_peak;
  }
  const bool any = __ballot(hit) != 0ull;
  if (lane == 0) out[map] = any ? 1 : 0;
}

extern "C" int mval_peak_mask(const float* heatmaps, float min_peak, uint8_t* out, int64_t n_maps, int hh, int wh, void* stream) {
  MVAL_REQUIRE(n_maps >= 0 && hh > 0 && wh > 0 && (int64_t)hh * wh <= 0x7fffffff, "mval_peak_mask: bad dims");
  if (n_maps == 0) return 0;
  MVAL_REQUIRE(heatmaps && out, "mval_peak_mask: heatmaps and out must not be NULL");
  MVAL_REQUIRE((n_maps + 3) / 4 <= 0x7fffffff, "mval_peak_mask: too many maps");
  hipLaunchKernelGGL(peak_mask_kernel, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, mval_stream(stream), heatmaps, out,
                     n_maps, hh * wh, min_peak);
  MVAL_CHECK_LAUNCH("mval_peak_mask");
  return 0;
}

// ---- sub-pixel refinement of the hard arg-max ----------------------------------------------------------------
// One THREAD per map: the arg-max is known (kp2d), what is left is nine loads around it and a few dozen float64 operations, so
// the launch is latency-bound on B*V*J independent small problems and a wave per map would idle 63 lanes.  The point is checked
// against the map before any load; every decision (sgn, accept) is taken on float64 values computed without FMA contraction, in
// the order the definition writes them, so that a host float64 evaluation takes the same decisions.
struct refine_offset { double ox, oy; };

__device__ __forceinline__ refine_offset refine_quarter(const double (&n)[3][3]) {
  const double dx = n[1][2] - n[1][0], dy = n[2][1] - n[0][1];  // (float32 values in float64: exact)
  return {dx > 0.0 ? 0.25 : dx < 0.0 ? -0.25 : 0.0, dy > 0.0 ? 0.25 : dy < 0.0 ? -0.25 : 0.0};
}

__device__ __forceinline__ refine_offset refine_taylor(const double (&n)[3][3]) {
#pragma clang fp contract(off)
  if (!(n[1][1] > 0.0)) return {0.0, 0.0};
  double L[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) L[r][c] = log(fmax(n[r][c], 1e-10));
  const double gx = 0.5 * (L[1][2] - L[1][0]), gy = 0.5 * (L[2][1] - L[0][1]);
  const double dxx = L[1][2] - 2.0 * L[1][1] + L[1][0], dyy = L[2][1] - 2.0 * L[1][1] + L[0][1];
  const double dxy = 0.25 * (L[2][2] - L[2][0] - L[0][2] + L[0][0]);
  const double det = dxx * dyy - dxy * dxy;
  const double ox = -(dyy * gx - dxy * gy) / det, oy = -(dxx * gy - dxy * gx) / det;
  const bool ok = dxx < 0.0 && det > 0.0 && fabs(ox) <= 1.0 && fabs(oy) <= 1.0;  // (every comparison is false for a NaN)
  return ok ? refine_offset{ox, oy} : refine_offset{0.0, 0.0};
}

__global__ __launch_bounds__(256) void refine_keypoints_kernel(int method, const float* __restrict__ hm, const int64_t* __restrict__ kp2d,
                                                               const uint8_t* __restrict__ valid, float* __restrict__ out,
                                                               float* __restrict__ conf, int64_t n_maps, int V, int J, int hh, int wh,
                                                               int stride) {
#pragma clang fp contract(off)
  const int64_t map = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (map >= n_maps) return;
  float2 xy = make_float2(0.f, 0.f);
  float peak = 0.f;
  if (!valid || valid[(map / ((int64_t)V * J)) * J + map % J]) {
    const int64_t kx = kp2d[map * 2], ky = kp2d[map * 2 + 1];
    const int64_t px = kx / stride, py = ky / stride;
    if (kx < 0 || ky < 0 || px >= wh || py >= hh) {  // not a point of this map (a decode split by another width): handed through, nothing loaded
      xy = make_float2((float)kx, (float)ky);
      peak = __builtin_nanf("");
    } else {
      const float* p = hm + map * ((int64_t)hh * wh) + py * wh + px;
      peak = p[0];
      refine_offset o = {0.0, 0.0};
      if (px >= 1 && px <= wh - 2 && py >= 1 && py <= hh - 2) {
        double n[3][3];
        bool finite = true;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int c = 0; c < 3; c++) {
            n[r][c] = (double)p[(r - 1) * wh + (c - 1)];
            finite = finite && fabs(n[r][c]) < INFINITY;  // (false for a NaN)
          }
        if (finite) o = method == MVAL_REFINE_QUARTER ? refine_quarter(n) : refine_taylor(n);
      }
      xy = make_float2((float)(((double)px + o.ox) * (double)stride), (float)(((double)py + o.oy) * (double)stride));
    }
  }
  reinterpret_cast<float2*>(out)[map] = xy;
  if (conf) conf[map] = peak;
}

extern "C" int mval_refine_keypoints(int method, const float* heatmaps, const int64_t* kp2d, const uint8_t* valid, float* out,
                                     float* conf, int B, int V, int J, int hh, int wh, int stride, void* stream) {
  MVAL_REQUIRE(method == MVAL_REFINE_QUARTER || method == MVAL_REFINE_TAYLOR, "mval_refine_keypoints: method %d is neither MVAL_REFINE_QUARTER nor MVAL_REFINE_TAYLOR", method);
  MVAL_REQUIRE(B >= 0 && V > 0 && J > 0 && hh > 0 && wh > 0 && (int64_t)hh * wh <= 0x7fffffff && stride > 0, "mval_refine_keypoints: bad dims");
  const int64_t n_maps = (int64_t)B * V * J;
  if (n_maps == 0) return 0;
  MVAL_REQUIRE(heatmaps && kp2d && out, "mval_refine_keypoints: heatmaps, kp2d and out must not be NULL");
  MVAL_REQUIRE(((uintptr_t)out & 7) == 0, "mval_refine_keypoints: out must be 8-byte aligned");
  MVAL_REQUIRE((n_maps + 255) / 256 <= 0x7fffffff, "mval_refine_keypoints: too many maps");
  hipLaunchKernelGGL(refine_keypoints_kernel, dim3((unsigned)((n_maps + 255) / 256)), dim3(256), 0, mval_stream(stream), method, heatmaps,
                     kp2d, valid, out, conf, n_maps, V, J, hh, wh, stride);
  MVAL_CHECK_LAUNCH("mval_refine_keypoints");
  return 0;
}

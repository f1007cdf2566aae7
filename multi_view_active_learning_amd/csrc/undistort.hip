// Undistortion of decoded key-points: the inverse of the reference's lens-distortion polynomial
// (utils/triangulation.py:433-456), one launch between the decode and the triangulation.
// One THREAD per entry (frame, view, joint), joints fastest: the lanes of a wave mostly share one (frame, view), so their
// loads of K and dist hit the same lines.  A few float64 operations per Newton iteration and at most 16 of them: the launch
// is latency-bound on B*V*J independent small problems.  No LDS, 64-bit indexing.  Every decision (zero coefficients, det J,
// convergence) is taken on float64 values computed without FMA contraction, in the order include/mval_hip.h writes them, so
// that a host float64 evaluation (tests/undistort_oracle.py) takes the same decisions.
#include "mval_common.h"

template <int MASK, typename KP>
__global__ __launch_bounds__(256) void undistort_keypoints_kernel(const KP* __restrict__ kp2d, const double* __restrict__ K,
                                                                  const double* __restrict__ dist, const uint8_t* __restrict__ valid,
                                                                  const uint8_t* __restrict__ mask, float* __restrict__ out,
                                                                  int32_t* __restrict__ status, int64_t n, int V, int J) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t bv = e / J;  // (frame, view)
  const int64_t b = bv / V;
  const int j = (int)(e - bv * J);
  float2 xy = make_float2(0.f, 0.f);
  int32_t st = 0;
  const bool present = (!valid || valid[b * J + j]) && (MASK != MASK_VIEWS || mask[bv]) && (MASK != MASK_VIEW_JOINT || mask[e]);
  if (present) {  // (nothing of an absent entry is read: neither its key-point nor, for an absent view, K and dist)
    const KP kx = kp2d[e * 2], ky = kp2d[e * 2 + 1];
    xy = make_float2((float)kx, (float)ky);  // handed through: zero coefficients, fold, no convergence
    const double* d = dist + bv * 5;
    const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4];
    if (!(k1 == 0.0 && k2 == 0.0 && p1 == 0.0 && p2 == 0.0 && k3 == 0.0)) {
      const double* Kv = K + bv * 9;
      const double K00 = Kv[0], K01 = Kv[1], K02 = Kv[2], K10 = Kv[3], K11 = Kv[4], K12 = Kv[5];
      const double a = (double)kx - K02, c = (double)ky - K12;
      const double detK = K00 * K11 - K01 * K10;
      const double tx = (K11 * a - K01 * c) / detK, ty = (K00 * c - K10 * a) / detK;
      double x = tx, y = ty;
      st = MVAL_UNDISTORT_NOCONV;
      for (int k = 1; k <= MVAL_UNDISTORT_MAX_ITERS; k++) {
        const double xx = x * x, yy = y * y, xy2 = x * y;
        const double r = xx + yy, r2 = r * r, r3 = r2 * r;
        const double radial = 1.0 + k1 * r + k2 * r2 + k3 * r3;
        const double slope = k1 + 2.0 * k2 * r + 3.0 * k3 * r2;  // d radial / d r
        // (the reference overwrites x with its distorted value before it forms y's cross term: 2 p2 xd y, not 2 p2 x y)
        const double xd = x * radial + 2.0 * p1 * xy2 + p2 * (r + 2.0 * xx);
        const double yd = y * radial + 2.0 * p2 * xd * y + p1 * (r + 2.0 * yy);
        const double fx = xd - tx, fy = yd - ty;
        const double jxx = radial + 2.0 * xx * slope + 2.0 * p1 * y + 6.0 * p2 * x;   // d xd / d x
        const double jxy = 2.0 * xy2 * slope + 2.0 * p1 * x + 2.0 * p2 * y;            // d xd / d y
        const double jyx = 2.0 * xy2 * slope + 2.0 * p1 * x + 2.0 * p2 * y * jxx;      // d yd / d x
        const double jyy = radial + 2.0 * yy * slope + 6.0 * p1 * y + 2.0 * p2 * (xd + y * jxy);  // d yd / d y
        const double detJ = jxx * jyy - jxy * jyx;
        if (!(detJ > 0.0 && detJ < INFINITY)) {  // (false for a NaN) the map folds over here, or the input was no point
          st = MVAL_UNDISTORT_FOLD;
          break;
        }
        const double dx = (jyy * fx - jxy * fy) / detJ, dy = (jxx * fy - jyx * fx) / detJ;
        x = x - dx;
        y = y - dy;
        const double tol = 1e-13 * (1.0 + fmax(fabs(x), fabs(y)));
        if (fabs(dx) <= tol && fabs(dy) <= tol) {  // max(|dx|, |dy|) <= tol, and false for a NaN step
          st = k;
          break;
        }
      }
      if (st > 0) xy = make_float2((float)(K00 * x + K01 * y + K02), (float)(K10 * x + K11 * y + K12));
    }
  }
  reinterpret_cast<float2*>(out)[e] = xy;
  status[e] = st;
}

extern "C" int mval_undistort_keypoints(const void* kp2d, int kp_is_f32, const double* K, const double* dist, const uint8_t* valid,
                                        const uint8_t* mask, int mask_kind, float* out, int32_t* status, int B, int V, int J,
                                        void* stream) {
  MVAL_REQUIRE(V >= 1 && V <= MVAL_PAIRS_MAX_VIEWS, "mval_undistort_keypoints: 1..%d views, got %d", MVAL_PAIRS_MAX_VIEWS, V);
  MVAL_REQUIRE(J >= 1 && B >= 0, "mval_undistort_keypoints: bad dims");
  MVAL_REQUIRE_MASK("mval_undistort_keypoints", mask, mask_kind);
  if (B == 0) return 0;
  MVAL_REQUIRE(kp2d && K && dist && out && status, "mval_undistort_keypoints: kp2d, K, dist, out and status must not be NULL");
  MVAL_REQUIRE(((uintptr_t)K | (uintptr_t)dist | (uintptr_t)out) % 8 == 0, "mval_undistort_keypoints: K, dist and out must be 8-byte aligned");
  MVAL_REQUIRE((uintptr_t)kp2d % (kp_is_f32 ? 4 : 8) == 0 && (uintptr_t)status % 4 == 0, "mval_undistort_keypoints: kp2d or status is not aligned");
  const int64_t n = (int64_t)B * V * J;
  MVAL_REQUIRE((n + 255) / 256 <= 0x7fffffff, "mval_undistort_keypoints: too many entries");
  const dim3 grid((unsigned)((n + 255) / 256));
  const hipStream_t s = mval_stream(stream);
  with_mask_kind(mask_kind, [&](auto M) {
    constexpr int MASK = decltype(M)::value;
    if (kp_is_f32)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(undistort_keypoints_kernel<MASK, float>), grid, dim3(256), 0, s, (const float*)kp2d, K, dist,
                         valid, mask, out, status, n, V, J);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(undistort_keypoints_kernel<MASK, int64_t>), grid, dim3(256), 0, s, (const int64_t*)kp2d, K,
                         dist, valid, mask, out, status, n, V, J);
  });
  MVAL_CHECK_LAUNCH("mval_undistort_keypoints");
  return 0;
}

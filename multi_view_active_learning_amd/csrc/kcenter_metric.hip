// Core-set selection under the l1, cosine and Chebyshev metrics: the greedy k-center of kcenter.hip (reference
// utils/coreset.py:49-95, which hands ``metric`` to sklearn.metrics.pairwise_distances) for three more distance forms.
//
// Same device design as kcenter.hip: features transposed once to [D][n_obs] (thread = row, 8-byte lanes contiguous), the
// centre in LDS, ONE launch per greedy step that first folds the previous step's per-workgroup (max, index) partials, no
// host round trip; first maximum wins ties, NaN is a maximum and propagates through the minimum (kcenter_common.h).
//
// The forms, float64, one accumulator per (row, centre), feature index k = 0 .. D-1 in that order:
//   l1         d = sum_k |x_k - c_k|                  (scipy's cdist "cityblock", what sklearn's manhattan_distances calls)
//   chebyshev  d = max_k |x_k - c_k|                  (scipy's cdist "chebyshev"; a NaN term makes d NaN here)
//   cosine     d = clip(1 - xh . ch, 0, 2)            (sklearn's cosine_distances) with xh = x / |x|: every row is
//              divided ONCE by its norm sqrt(sum_k x_k^2) -- a norm below 10 * DBL_EPSILON (a zero row) is replaced by 1,
//              sklearn's normalize() -- and the normalised table takes the transposed table's place, so a step reads as
//              many bytes as the Euclidean one.  No zeroing of a row's distance to itself (the reference passes two
//              different arrays, so sklearn's ``X is Y`` diagonal fix never applies).
// Products and sums are NOT contracted into fma in this file: every operation rounds once, as the numpy restatement
// (tests/coreset_metric_oracle.py) does, so the two agree bit for bit; l1 and chebyshev have no products at all.
#include <float.h>

#include "kcenter_common.h"

#pragma clang fp contract(off)

template <int M>
__device__ __forceinline__ double kcm_fold(double acc, double x, double c) {
  if (M == MVAL_KC_COSINE) return acc + x * c;
  const double a = fabs(x - c);
  if (M == MVAL_KC_L1) return acc + a;
  return (a > acc || a != a) ? a : acc;  // maximum that keeps a NaN (np.maximum)
}
template <int M>
__device__ __forceinline__ double kcm_finish(double acc) {
  if (M != MVAL_KC_COSINE) return acc;
  const double t = 1.0 - acc;  // sklearn: S *= -1; S += 1; clip(S, 0, 2) -- a NaN stays
  return t < 0.0 ? 0.0 : (t > 2.0 ? 2.0 : t);
}

// [n][D] -> [D][n]; cosine: each row divided by its norm first (norms[i] keeps the divisor)
template <int M>
__global__ __launch_bounds__(KC_THREADS) void kcm_transpose_kernel(const double* __restrict__ feat,
                                                                   double* __restrict__ featT,
                                                                   double* __restrict__ norms, int64_t n, int D) {
  int64_t i = (int64_t)blockIdx.x * KC_THREADS + threadIdx.x;
  if (i >= n) return;
  double nrm = 1.0;
  if (M == MVAL_KC_COSINE) {
    double s = 0.0;
    for (int d = 0; d < D; d++) {
      double x = feat[i * D + d];
      s = s + x * x;
    }
    nrm = sqrt(s);
    if (nrm < 10.0 * DBL_EPSILON) nrm = 1.0;
    norms[i] = nrm;
  }
  for (int d = 0; d < D; d++) {
    double x = feat[i * D + d];
    featT[(int64_t)d * n + i] = M == MVAL_KC_COSINE ? x / nrm : x;
  }
}

// min over the labeled centres (coreset.py:64-67), 4 centres per pass over a row
template <int M>
__global__ __launch_bounds__(KC_THREADS) void kcm_init_kernel(const double* __restrict__ featT,
                                                              const int64_t* __restrict__ labeled, int64_t n_labeled,
                                                              double* __restrict__ min_d, int have_min,
                                                              KcPartial* __restrict__ part, int64_t n, int D) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* cen = reinterpret_cast<double*>(smem_raw);  // [4][D]
  __shared__ KcPartial sh[KC_THREADS / 64];
  KcPartial best;
  best.val = -INFINITY;
  best.idx = INT64_MAX;
  for (int64_t i0 = (int64_t)blockIdx.x * KC_THREADS; i0 < n; i0 += (int64_t)gridDim.x * KC_THREADS) {
    const int64_t i = i0 + threadIdx.x;
    const bool live = i < n;
    double md = (have_min && live) ? min_d[i] : INFINITY;
    bool first = !have_min;
    for (int64_t c0 = 0; c0 < n_labeled; c0 += 4) {
      int nc = (int)min((int64_t)4, n_labeled - c0);
      __syncthreads();
      for (int t = threadIdx.x; t < nc * D; t += KC_THREADS) cen[t] = featT[(int64_t)(t % D) * n + labeled[c0 + t / D]];
      __syncthreads();
      if (live) {
        double d0 = 0, d1 = 0, d2 = 0, d3 = 0;
        for (int d = 0; d < D; d++) {
          double x = featT[(int64_t)d * n + i];
          d0 = kcm_fold<M>(d0, x, cen[d]);
          if (nc > 1) d1 = kcm_fold<M>(d1, x, cen[D + d]);
          if (nc > 2) d2 = kcm_fold<M>(d2, x, cen[2 * D + d]);
          if (nc > 3) d3 = kcm_fold<M>(d3, x, cen[3 * D + d]);
        }
        double dd[4] = {d0, d1, d2, d3};
        for (int k = 0; k < nc; k++) {
          double t = kcm_finish<M>(dd[k]);
          md = first ? t : np_minimum(md, t);
          first = false;
        }
      }
    }
    if (live) {
      min_d[i] = md;
      if (kc_better(md, i, best.val, best.idx)) { best.val = md; best.idx = i; }
    }
  }
  KcPartial r = kc_block_reduce(best, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

template <int M>
__global__ __launch_bounds__(KC_THREADS) void kcm_step_kernel(const double* __restrict__ featT,
                                                              double* __restrict__ min_d,
                                                              const KcPartial* __restrict__ part_in, int n_part_in,
                                                              KcPartial* __restrict__ part_out,
                                                              int64_t* __restrict__ picks, int step, int64_t n, int D) {
  __shared__ KcPartial sh[KC_THREADS / 64];
  __shared__ double cen[KC_MAX_D];
  // (1) global arg-max of the previous pass, redundantly per workgroup
  KcPartial b;
  b.val = -INFINITY;
  b.idx = INT64_MAX;
  for (int t = threadIdx.x; t < n_part_in; t += KC_THREADS) {
    KcPartial q = part_in[t];
    if (kc_better(q.val, q.idx, b.val, b.idx)) b = q;
  }
  b = kc_block_reduce(b, sh);
  const int64_t ind = b.idx;
  if (blockIdx.x == 0 && threadIdx.x == 0) picks[step] = ind;
  for (int d = threadIdx.x; d < D; d += KC_THREADS) cen[d] = featT[(int64_t)d * n + ind];
  __syncthreads();
  // (2) min_d = minimum(min_d, dist(., centre)) on this workgroup's rows + next partial
  KcPartial best;
  best.val = -INFINITY;
  best.idx = INT64_MAX;
  for (int64_t i = (int64_t)blockIdx.x * KC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KC_THREADS) {
    double acc = 0.0;
    for (int d = 0; d < D; d++) acc = kcm_fold<M>(acc, featT[(int64_t)d * n + i], cen[d]);
    double md = np_minimum(min_d[i], kcm_finish<M>(acc));
    min_d[i] = md;
    if (kc_better(md, i, best.val, best.idx)) { best.val = md; best.idx = i; }
  }
  KcPartial r = kc_block_reduce(best, sh);
  if (threadIdx.x == 0) part_out[blockIdx.x] = r;
}

template <int M>
static int kcm_select(const double* feat, int64_t n_obs, int D, const int64_t* labeled, int64_t n_labeled, int n_select,
                      int have_min_dist, double* row_norms, double* min_dist, int64_t* picks, void* ws, hipStream_t s) {
  double* featT = reinterpret_cast<double*>(ws);
  KcPartial* part = reinterpret_cast<KcPartial*>(featT + (size_t)n_obs * D);
  part = reinterpret_cast<KcPartial*>(((uintptr_t)part + 15) & ~(uintptr_t)15);
  const int nb = kc_blocks(n_obs);
  hipLaunchKernelGGL(kcm_transpose_kernel<M>, dim3((unsigned)((n_obs + KC_THREADS - 1) / KC_THREADS)), dim3(KC_THREADS),
                     0, s, feat, featT, row_norms, n_obs, D);
  MVAL_CHECK_LAUNCH("mval_kcenter_select_metric/transpose");
  hipLaunchKernelGGL(kcm_init_kernel<M>, dim3(nb), dim3(KC_THREADS), (size_t)4 * D * sizeof(double), s, featT, labeled,
                     n_labeled, min_dist, have_min_dist, part, n_obs, D);
  MVAL_CHECK_LAUNCH("mval_kcenter_select_metric/init");
  for (int t = 0; t < n_select; t++) {
    KcPartial* pin = part + (t & 1) * KC_MAX_BLOCKS;
    KcPartial* pout = part + ((t + 1) & 1) * KC_MAX_BLOCKS;
    hipLaunchKernelGGL(kcm_step_kernel<M>, dim3(nb), dim3(KC_THREADS), 0, s, featT, min_dist, pin, nb, pout, picks, t,
                       n_obs, D);
  }
  MVAL_CHECK_LAUNCH("mval_kcenter_select_metric/step");
  return 0;
}

extern "C" int mval_kcenter_select_metric(int metric, const double* feat, int64_t n_obs, int D, const int64_t* labeled,
                                          int64_t n_labeled, int n_select, int have_min_dist, double* row_norms,
                                          double* min_dist, int64_t* picks, void* ws, void* stream) {
  if (metric == MVAL_KC_EUCLIDEAN)
    return mval_kcenter_select(feat, n_obs, D, labeled, n_labeled, n_select, have_min_dist, row_norms, min_dist, picks, ws,
                               stream);
  MVAL_REQUIRE(metric == MVAL_KC_L1 || metric == MVAL_KC_COSINE || metric == MVAL_KC_CHEBYSHEV,
               "mval_kcenter_select_metric: unknown metric id %d (MVAL_KC_EUCLIDEAN %d, MVAL_KC_L1 %d, MVAL_KC_COSINE %d, "
               "MVAL_KC_CHEBYSHEV %d)", metric, MVAL_KC_EUCLIDEAN, MVAL_KC_L1, MVAL_KC_COSINE, MVAL_KC_CHEBYSHEV);
  MVAL_REQUIRE(n_obs > 0 && D > 0 && D <= KC_MAX_D && n_select >= 0 && n_labeled >= 0,
               "mval_kcenter_select_metric: bad dims");
  hipStream_t s = mval_stream(stream);
  if (metric == MVAL_KC_L1)
    return kcm_select<MVAL_KC_L1>(feat, n_obs, D, labeled, n_labeled, n_select, have_min_dist, row_norms, min_dist, picks,
                                  ws, s);
  if (metric == MVAL_KC_COSINE)
    return kcm_select<MVAL_KC_COSINE>(feat, n_obs, D, labeled, n_labeled, n_select, have_min_dist, row_norms, min_dist,
                                      picks, ws, s);
  return kcm_select<MVAL_KC_CHEBYSHEV>(feat, n_obs, D, labeled, n_labeled, n_select, have_min_dist, row_norms, min_dist,
                                       picks, ws, s);
}

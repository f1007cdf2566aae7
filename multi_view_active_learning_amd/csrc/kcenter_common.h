// Shared by the greedy k-center translation units (kcenter.hip: sklearn's expanded Euclidean form; kcenter_metric.hip:
// l1, cosine, Chebyshev): the launch shape, the per-workgroup (max, index) partial and its ordering.
#pragma once
#include "mval_common.h"

#define KC_THREADS 256
#define KC_MAX_BLOCKS 1024
#define KC_MAX_D 512

struct KcPartial {
  double val;
  int64_t idx;
};

__device__ __forceinline__ bool kc_better(double v, int64_t i, double bv, int64_t bi) {
  bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (vn) return i < bi;
  return (v > bv) || (v == bv && i < bi);
}
__device__ __forceinline__ double np_minimum(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a < b ? a : b;
}

__device__ __forceinline__ KcPartial kc_block_reduce(KcPartial p, KcPartial* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    double ov = __shfl_xor(p.val, o, 64);
    long long oi = __shfl_xor((long long)p.idx, o, 64);
    if (kc_better(ov, oi, p.val, p.idx)) { p.val = ov; p.idx = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
  __syncthreads();
  KcPartial r = sh[0];
  for (int w = 1; w < KC_THREADS / 64; w++)
    if (kc_better(sh[w].val, sh[w].idx, r.val, r.idx)) r = sh[w];
  __syncthreads();
  return r;
}

static int kc_blocks(int64_t n) {
  int64_t nb = (n + KC_THREADS - 1) / KC_THREADS;
  if (nb > KC_MAX_BLOCKS) nb = KC_MAX_BLOCKS;
  if (nb < 1) nb = 1;
  return (int)nb;
}

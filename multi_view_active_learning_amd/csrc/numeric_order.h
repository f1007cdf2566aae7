// The two orders the post stage reproduces bit for bit, each written once: numpy's pairwise summation and torch.argmax's
// comparison.  np.mean / np.std (csrc/triangulate.hip, csrc/scoring.hip) and the hard arg-max (csrc/decode.hip,
// csrc/scoring.hip) agree with the reference only as long as every user goes through these.
#pragma once

// numpy's pairwise summation (np.add.reduce on a contiguous vector of T), so that np.mean(...) / np.std(...) in the
// reference are reproduced bit for bit given equal addends.
template <typename T>
__device__ T np_pairwise_sum(const T* a, int n) {
  if (n < 8) {
    T r = 0;
    for (int i = 0; i < n; i++) r += a[i];
    return r;
  }
  if (n <= 128) {
    T r[8];
    for (int k = 0; k < 8; k++) r[k] = a[k];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int k = 0; k < 8; k++) r[k] += a[i + k];
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum<T>(a, n2) + np_pairwise_sum<T>(a + n2, n - n2);
}

// order of torch.argmax: NaN is the maximum; ties -> lowest flat index.  True when (v, i) comes before (bv, bi).
// (T: float for heat-map values, double for the per-map losses loss_weighted.hip ranks)
template <typename T>
__device__ __forceinline__ bool argmax_better(T v, int i, T bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (vn) return i < bi;
  return (v > bv) || (v == bv && i < bi);
}

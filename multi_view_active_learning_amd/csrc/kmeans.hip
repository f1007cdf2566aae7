// SAL pose-cluster KMeans fit (reference strategy.py:38-52: sklearn.cluster.KMeans(NUM_CLUSTERS,
// random_state=RANDOM_SEED).fit on root-relative poses), sklearn 1.7.2 semantics, float64 throughout.
//
// One call = one initialisation: prologue -> greedy k-means++ seeding -> Lloyd iterations -> final E-step
// and inertia.  Every step is a launch on the caller's stream; the data never leaves the device.  The host
// draws all random numbers (first index + (K-1)*L uniforms) beforehand, so nothing here is random.
//
//   prologue   transpose X to [D][n]; column mean and variance (tol_abs = tol * mean(var)); centre
//              X (row-major and transposed copies) and its row squared norms
//   seeding    2 launches per centre:
//                km_pp_cand   (grid)  distances of the L candidates to every row in sklearn's expanded form
//                             max(0, (-2 x.c + |c|^2) + |x|^2), minimum with the running closest distance,
//                             per-workgroup partial potentials
//                km_pp_search (1 WG)  per-candidate potentials -> first minimum = the chosen centre; then for
//                             each uniform u the first row whose inclusive prefix sum of the closest
//                             distance reaches u * potential (np.searchsorted left), clipped to n-1
//              the closest distance of the chosen candidate is never copied: the next km_pp_cand reads it
//              from the candidate buffer of the previous step (double-buffered)
//   Lloyd      3 launches per iteration, each a no-op once the device-side `done` flag is set:
//                km_assign    (grid)  first-minimum argmin of |c_k|^2 - 2 x.c_k, changed-label count, direct
//                             |x - c_label|^2, per-workgroup cluster sums (256 rows in row order)
//                km_reduce    (grid)  workgroup partials -> cluster sums / counts, in workgroup order
//                km_update    (1 WG)  empty-cluster relocation, averaging, centre shift, convergence test
//              the host reads `done` every KM_CHECK_EVERY iterations (one stream sync), never per iteration
//   finish     final E-step unless the labels converged strictly, inertia, centres + mean
//
// Reduction orders are fixed (no atomics on values), so two fits of the same input give identical bits.
#include "mval_common.h"

#define KM_THREADS 256
#define KM_MAX_D 512
#define KM_MAX_L 16
#define KM_MAX_KD 3840  // 2 * K * D doubles of LDS in km_assign (60 KiB)
#define KM_CHECK_EVERY 16

struct KmState {
  double tol_abs;
  double inertia;
  int iter;         // Lloyd iterations run so far
  int done;         // 1: converged or max_iter reached (every later Lloyd launch returns at once)
  int strict;       // 1: labels unchanged in the last iteration (no final E-step)
  int n_iter;       // sklearn's n_iter_ (i + 1)
  int best_slot;    // seeding: index into the previous step's candidates of the chosen one
  int pad;
};

struct KmWs {
  double* XT;       // [D][n] centred
  double* Xc;       // [n][D] centred
  double* xnorm;    // [n]
  double* mean;     // [D]
  double* var;      // [D]
  double* dcand;    // [2][L][n] seeding candidate distances
  double* ppart;    // [L][nb] seeding partial potentials
  int64_t* cand;    // [L]
  double* cen;      // [K][D] current centres (centred)
  double* dist;     // [n] |x - c_old[label]|^2 (relocation) / inertia terms
  double* part;     // [nb][K*D + K + 1] Lloyd partials: sums, counts, changed
  double* red;      // [K*D + K + 1]
  KmState* st;
};

static int km_blocks(int64_t n) { return (int)((n + KM_THREADS - 1) / KM_THREADS); }

static size_t km_align(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t km_layout(int64_t n, int D, int K, int L, char* base, KmWs* w) {
  const int64_t nb = km_blocks(n);
  const size_t E = (size_t)K * D + K + 1;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += km_align(bytes);
    return p;
  };
  KmWs t;
  t.XT = (double*)take((size_t)n * D * 8);
  t.Xc = (double*)take((size_t)n * D * 8);
  t.xnorm = (double*)take((size_t)n * 8);
  t.mean = (double*)take((size_t)D * 8);
  t.var = (double*)take((size_t)D * 8);
  t.dcand = (double*)take((size_t)2 * L * n * 8);
  t.ppart = (double*)take((size_t)L * nb * 8);
  t.cand = (int64_t*)take((size_t)L * 8);
  t.cen = (double*)take((size_t)K * D * 8);
  t.dist = (double*)take((size_t)n * 8);
  t.part = (double*)take((size_t)nb * E * 8);
  t.red = (double*)take(E * 8);
  t.st = (KmState*)take(sizeof(KmState));
  if (w) *w = t;
  return off + 256;
}

// fixed-order workgroup sum (wave butterfly, then the 4 wave sums in order); every thread gets the result
__device__ __forceinline__ double km_block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < KM_THREADS / 64; w++) r += sh[w];
  __syncthreads();
  return r;
}

// ---- prologue ----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(KM_THREADS) void km_transpose_kernel(const double* __restrict__ X, double* __restrict__ XT,
                                                                  int64_t n, int D) {
  const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
  if (i >= n) return;
  for (int d = 0; d < D; d++) XT[(int64_t)d * n + i] = X[i * D + d];
}

// one workgroup per column: mean, then the variance about it (np.var: mean of squared deviations)
__global__ __launch_bounds__(KM_THREADS) void km_colstats_kernel(const double* __restrict__ XT, double* __restrict__ mean,
                                                                 double* __restrict__ var, int64_t n) {
  __shared__ double sh[KM_THREADS / 64];
  const double* col = XT + (int64_t)blockIdx.x * n;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += KM_THREADS) s += col[i];
  const double m = km_block_sum(s, sh) / (double)n;
  double q = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += KM_THREADS) {
    const double t = col[i] - m;
    q += t * t;
  }
  const double v = km_block_sum(q, sh) / (double)n;
  if (threadIdx.x == 0) {
    mean[blockIdx.x] = m;
    var[blockIdx.x] = v;
  }
}

// centre both copies in place; row squared norms of the centred rows; labels start at -1 (sklearn's labels_old)
__global__ __launch_bounds__(KM_THREADS) void km_center_kernel(double* __restrict__ XT,
                                                               double* __restrict__ Xc, const double* __restrict__ mean,
                                                               double* __restrict__ xnorm, int* __restrict__ labels,
                                                               int64_t n, int D) {
  const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int d = 0; d < D; d++) {
    const double x = XT[(int64_t)d * n + i] - mean[d];
    XT[(int64_t)d * n + i] = x;
    Xc[i * D + d] = x;
    s += x * x;
  }
  xnorm[i] = s;
  labels[i] = -1;
}

// state reset, tol_abs, first candidate = the host's first index
__global__ void km_setup_kernel(const double* __restrict__ var, KmState* st, int64_t* cand, int64_t first_idx, double tol,
                                int D) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int d = 0; d < D; d++) s += var[d];
  st->tol_abs = tol == 0.0 ? 0.0 : (s / (double)D) * tol;
  st->inertia = 0.0;
  st->iter = 0;
  st->done = 0;
  st->strict = 0;
  st->n_iter = 0;
  st->best_slot = 0;
  cand[0] = first_idx;
}

// ---- k-means++ seeding --------------------------------------------------------------------------------------

// dout[l][i] = minimum(closest[i], max(0, (-2 x_i.c_l + |c_l|^2) + |x_i|^2)); closest = din[best_slot] (or +inf on
// the first step); ppart[l][block] = workgroup sum of dout[l]
__global__ __launch_bounds__(KM_THREADS) void km_pp_cand_kernel(const double* __restrict__ XT, const double* __restrict__ Xc,
                                                                const double* __restrict__ xnorm,
                                                                const int64_t* __restrict__ cand, int nc,
                                                                const double* __restrict__ din, double* __restrict__ dout,
                                                                double* __restrict__ ppart, const KmState* __restrict__ st,
                                                                int first, int64_t n, int D) {
  __shared__ double sh[KM_THREADS / 64];
  __shared__ double cn[KM_MAX_L];
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* c = reinterpret_cast<double*>(smem_raw);  // [nc][D]
  for (int t = threadIdx.x; t < nc * D; t += KM_THREADS) c[t] = Xc[cand[t / D] * D + t % D];
  if (threadIdx.x < nc) cn[threadIdx.x] = xnorm[cand[threadIdx.x]];
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
  const bool live = i < n;
  const double closest = (first || !live) ? INFINITY : din[(int64_t)st->best_slot * n + i];
  const double xx = live ? xnorm[i] : 0.0;
  for (int l = 0; l < nc; l++) {
    double v = 0.0;
    if (live) {
      double dot = 0.0;
      for (int d = 0; d < D; d++) dot = fma(XT[(int64_t)d * n + i], c[l * D + d], dot);
      double t = -2.0 * dot;
      t += cn[l];
      t += xx;
      t = t > 0.0 ? t : 0.0;
      v = closest < t ? closest : t;
      dout[(int64_t)l * n + i] = v;
    }
    const double s = km_block_sum(v, sh);
    if (threadIdx.x == 0) ppart[(int64_t)l * gridDim.x + blockIdx.x] = s;
  }
}

// inclusive-prefix search of one wave: first position p in [0, len) with carry + prefix(vals[0..p]) >= target.
// Returns p (or -1) and leaves in *carry the total before p (or the running total when not found).
__device__ int km_wave_search(const double* vals, int64_t len, double target, double* carry) {
  const int lane = threadIdx.x & 63;
  double run = *carry;
  for (int64_t b0 = 0; b0 < len; b0 += 64) {
    double v = (b0 + lane < len) ? vals[b0 + lane] : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    const double incl = run + v;
    const unsigned long long hit = __ballot((b0 + lane < len) && incl >= target);
    if (hit) {
      const int p = __ffsll((long long)hit) - 1;
      double excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = run;
      *carry = __shfl(excl, p, 64);
      return (int)(b0 + p);
    }
    run = __shfl(incl, 63, 64);
  }
  *carry = run;
  return -1;
}

// (1) potentials of the previous step's nc_prev candidates, first minimum wins -> picks[step - 1];
// (2) unless step == K: for each of the L uniforms the searchsorted index of u * potential in the prefix sums
//     of the chosen candidate's closest distances -> cand[0..L)
__global__ __launch_bounds__(KM_THREADS) void km_pp_search_kernel(const double* __restrict__ ppart, int nb, int nc_prev,
                                                                  const double* __restrict__ dprev,
                                                                  int64_t* __restrict__ cand, int64_t* __restrict__ picks,
                                                                  const double* __restrict__ rand_u, int L, int step, int K,
                                                                  KmState* __restrict__ st, int64_t n) {
  __shared__ double sh[KM_THREADS / 64];
  __shared__ double pot[KM_MAX_L];
  for (int l = 0; l < nc_prev; l++) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += KM_THREADS) s += ppart[(int64_t)l * nb + b];
    s = km_block_sum(s, sh);
    if (threadIdx.x == 0) pot[l] = s;
  }
  __syncthreads();
  int best = 0;
  for (int l = 1; l < nc_prev; l++)
    if (pot[l] < pot[best]) best = l;
  const double cur = pot[best];
  const int64_t chosen = cand[best];
  __syncthreads();  // every thread has read cand[] before it is overwritten below
  if (threadIdx.x == 0) {
    picks[step - 1] = chosen;
    st->best_slot = best;
  }
  if (step >= K) return;
  const double* closest = dprev + (int64_t)best * n;
  const double* bpart = ppart + (int64_t)best * nb;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = wave; j < L; j += KM_THREADS / 64) {
    const double target = rand_u[(int64_t)(step - 1) * L + j] * cur;
    double carry = 0.0;
    int64_t idx = n - 1;
    const int blk = km_wave_search(bpart, nb, target, &carry);
    if (blk >= 0) {
      // rows from the found workgroup on; its row-order prefix may round below the workgroup-order one
      const int64_t r0 = (int64_t)blk * KM_THREADS;
      const int p = km_wave_search(closest + r0, n - r0, target, &carry);
      if (p >= 0) idx = r0 + p;
    }
    if (lane == 0) cand[j] = idx;
  }
}

// ---- Lloyd iteration -------------------------------------------------------------------------------------------

// mode 0: Lloyd E-step + partial M-step (labels, changed count, dist, cluster sums / counts per workgroup)
// mode 1: final pass: re-assign unless the iteration converged strictly, then dist = |x - c_label|^2 (inertia terms)
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(const double* __restrict__ XT, const double* __restrict__ Xc,
                                                               const double* __restrict__ cen, int* __restrict__ labels,
                                                               double* __restrict__ dist, double* __restrict__ part,
                                                               const KmState* __restrict__ st, int mode, int64_t n, int D,
                                                               int K) {
  if (mode == 0 && st->done) return;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* c = reinterpret_cast<double*>(smem_raw);  // [K][D]
  double* acc = c + K * D;                           // [K][D] (mode 0)
  __shared__ double cc[KM_THREADS];
  __shared__ double cnt[KM_THREADS];
  __shared__ int lab[KM_THREADS];
  __shared__ double sh[KM_THREADS / 64];
  for (int t = threadIdx.x; t < K * D; t += KM_THREADS) {
    c[t] = cen[t];
    if (mode == 0) acc[t] = 0.0;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += KM_THREADS) {
    double s = 0.0;
    for (int d = 0; d < D; d++) s += c[k * D + d] * c[k * D + d];
    cc[k] = s;
    cnt[k] = 0.0;
  }
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * KM_THREADS;
  const int64_t i = r0 + threadIdx.x;
  const bool live = i < n;
  const bool reassign = mode == 0 || !st->strict;
  int changed = 0;
  if (live) {
    int bk = labels[i];
    if (reassign) {
      const int old = bk;
      double best = 0.0;
      bk = 0;
      for (int k0 = 0; k0 < K; k0 += 4) {
        const int nk = min(4, K - k0);
        double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
        for (int d = 0; d < D; d++) {
          const double x = XT[(int64_t)d * n + i];
          d0 = fma(x, c[k0 * D + d], d0);
          if (nk > 1) d1 = fma(x, c[(k0 + 1) * D + d], d1);
          if (nk > 2) d2 = fma(x, c[(k0 + 2) * D + d], d2);
          if (nk > 3) d3 = fma(x, c[(k0 + 3) * D + d], d3);
        }
        const double dd[4] = {d0, d1, d2, d3};
        for (int q = 0; q < nk; q++) {
          const double v = cc[k0 + q] - 2.0 * dd[q];
          if (k0 + q == 0 || v < best) {
            best = v;
            bk = k0 + q;
          }
        }
      }
      changed = bk != old;
      labels[i] = bk;
    }
    double s = 0.0;
    for (int d = 0; d < D; d++) {
      const double t = XT[(int64_t)d * n + i] - c[bk * D + d];
      s += t * t;
    }
    dist[i] = s;
    lab[threadIdx.x] = bk;
  }
  if (mode != 0) {
    const double s = km_block_sum(live ? dist[i] : 0.0, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
    return;
  }
  const double nchanged = km_block_sum((double)changed, sh);  // (also the barrier for lab[])
  const int rows = (int)min((int64_t)KM_THREADS, n - r0);
  const size_t E = (size_t)K * D + K + 1;
  double* out = part + (size_t)blockIdx.x * E;
  // cluster sums: thread d owns column d of every cluster, rows added in row order
  // (loads of 16 rows are issued before their adds: the adds stay in row order, the loads overlap)
  for (int d = threadIdx.x; d < D; d += KM_THREADS) {
    const double* xr = Xc + r0 * D + d;
    int r = 0;
    for (; r + 16 <= rows; r += 16) {
      double v[16];
#pragma unroll
      for (int q = 0; q < 16; q++) v[q] = xr[(int64_t)(r + q) * D];
#pragma unroll
      for (int q = 0; q < 16; q++) acc[lab[r + q] * D + d] += v[q];
    }
    for (; r < rows; r++) acc[lab[r] * D + d] += xr[(int64_t)r * D];
  }
  if (threadIdx.x == 0)
    for (int r = 0; r < rows; r++) cnt[lab[r]] += 1.0;
  __syncthreads();
  for (int t = threadIdx.x; t < K * D; t += KM_THREADS) out[t] = acc[t];
  for (int k = threadIdx.x; k < K; k += KM_THREADS) out[K * D + k] = cnt[k];
  if (threadIdx.x == 0) out[K * D + K] = nchanged;
}

// red[e] = sum over workgroups (in order) of part[b][e]
__global__ __launch_bounds__(KM_THREADS) void km_reduce_kernel(const double* __restrict__ part, double* __restrict__ red,
                                                               const KmState* __restrict__ st, int nb, int E) {
  if (st->done) return;
  const int e = blockIdx.x * KM_THREADS + threadIdx.x;
  if (e >= E) return;
  double s = 0.0;
  int b = 0;
  for (; b + 16 <= nb; b += 16) {  // 16 loads in flight, adds in workgroup order
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; q++) v[q] = part[(size_t)(b + q) * E + e];
#pragma unroll
    for (int q = 0; q < 16; q++) s += v[q];
  }
  for (; b < nb; b++) s += part[(size_t)b * E + e];
  red[e] = s;
}

// M-step tail (one workgroup): relocation of empty clusters (_relocate_empty_clusters_dense), averaging
// (_average_centers, in-place order included), centre shift, convergence test
__global__ __launch_bounds__(KM_THREADS) void km_update_kernel(const double* __restrict__ Xc, const int* __restrict__ labels,
                                                               const double* __restrict__ dist, double* __restrict__ red,
                                                               double* __restrict__ cen,
                                                               KmState* __restrict__ st, int max_iter, int64_t n, int D,
                                                               int K) {
  if (st->done) return;
  __shared__ double wsh[KM_THREADS / 64];
  __shared__ int64_t ish[KM_THREADS / 64];
  __shared__ double shift[KM_THREADS];
  __shared__ int far_pick[KM_THREADS];
  __shared__ int empty[KM_THREADS];
  double* sums = red;
  double* cnt = red + (size_t)K * D;
  const double changed = red[(size_t)K * D + K];
  int n_empty = 0;
  for (int k = 0; k < K; k++)
    if (cnt[k] == 0.0) {
      if (threadIdx.x == 0) empty[n_empty] = k;
      n_empty++;
    }
  __syncthreads();
  if (n_empty > 0) {
    // farthest points from their old centres, largest first (lower index on equal distances)
    double prev_v = INFINITY;
    int64_t prev_i = -1;
    double maxd = 0.0;
    for (int e = 0; e < n_empty; e++) {
      double bv = -1.0;
      int64_t bi = INT64_MAX;
      for (int64_t i = threadIdx.x; i < n; i += KM_THREADS) {
        const double v = dist[i];
        const bool after = v < prev_v || (v == prev_v && i > prev_i);
        if (after && (v > bv || (v == bv && i < bi))) {
          bv = v;
          bi = i;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const long long oi = __shfl_xor((long long)bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      __syncthreads();
      if ((threadIdx.x & 63) == 0) {
        wsh[threadIdx.x >> 6] = bv;
        ish[threadIdx.x >> 6] = bi;
      }
      __syncthreads();
      bv = wsh[0];
      bi = ish[0];
      for (int w = 1; w < KM_THREADS / 64; w++)
        if (wsh[w] > bv || (wsh[w] == bv && ish[w] < bi)) {
          bv = wsh[w];
          bi = ish[w];
        }
      if (e == 0) maxd = bv;
      if (threadIdx.x == 0) far_pick[e] = (int)bi;
      prev_v = bv;
      prev_i = bi;
    }
    __syncthreads();
    if (maxd != 0.0) {  // all distances 0 (more clusters than distinct rows): relocation is pointless
      for (int e = 0; e < n_empty; e++) {
        const int k = empty[e];
        const int64_t far = far_pick[e];
        const int old = labels[far];
        for (int d = threadIdx.x; d < D; d += KM_THREADS) {
          const double x = Xc[far * D + d];
          sums[(size_t)old * D + d] -= x;
          sums[(size_t)k * D + d] = x;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
          cnt[k] = 1.0;
          cnt[old] -= 1.0;
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();
  int am = 0;
  for (int k = 1; k < K; k++)
    if (cnt[k] > cnt[am]) am = k;
  // _average_centers works in place, cluster by cluster: an empty cluster takes the row of the largest one as
  // it is at that moment (already averaged only if it comes first)
  for (int d = threadIdx.x; d < D; d += KM_THREADS) {
    for (int k = 0; k < K; k++) {
      if (cnt[k] > 0.0) {
        const double alpha = 1.0 / cnt[k];
        sums[(size_t)k * D + d] *= alpha;
      } else {
        sums[(size_t)k * D + d] = sums[(size_t)am * D + d];
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += KM_THREADS) {
    double s = 0.0;
    for (int d = 0; d < D; d++) {
      const double t = sums[(size_t)k * D + d] - cen[(size_t)k * D + d];
      s += t * t;
    }
    shift[k] = sqrt(s);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < K * D; t += KM_THREADS) {
    cen[t] = sums[t];
  }
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int k = 0; k < K; k++) tot += shift[k] * shift[k];
    const int it = st->iter;
    if (changed == 0.0) {
      st->strict = 1;
      st->done = 1;
      st->n_iter = it + 1;
    } else if (tot <= st->tol_abs) {
      st->done = 1;
      st->n_iter = it + 1;
    } else if (it + 1 >= max_iter) {
      st->done = 1;
      st->n_iter = it + 1;
    }
    st->iter = it + 1;
  }
}

// ---- finish -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(KM_THREADS) void km_finish_kernel(const double* __restrict__ part, int nb,
                                                               const double* __restrict__ cen, const double* __restrict__ mean,
                                                               double* __restrict__ centers, double* __restrict__ inertia,
                                                               int* __restrict__ n_iter, KmState* __restrict__ st, int D,
                                                               int K) {
  __shared__ double sh[KM_THREADS / 64];
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += KM_THREADS) s += part[b];
  s = km_block_sum(s, sh);
  for (int t = threadIdx.x; t < K * D; t += KM_THREADS) centers[t] = cen[t] + mean[t % D];
  if (threadIdx.x == 0) {
    st->inertia = s;
    inertia[0] = s;
    n_iter[0] = st->n_iter;
  }
}

// initial centres: rows of the centred data at the seeding picks, or init - mean
__global__ void km_init_centers_kernel(const double* __restrict__ Xc, const int64_t* __restrict__ picks,
                                       const double* __restrict__ init, const double* __restrict__ mean,
                                       double* __restrict__ cen, int D, int K) {
  for (int t = threadIdx.x; t < K * D; t += blockDim.x) {
    const int k = t / D, d = t % D;
    cen[t] = init ? init[t] - mean[d] : Xc[picks[k] * D + d];
  }
}

extern "C" size_t mval_kmeans_workspace_bytes(int64_t n, int D, int K, int L) {
  if (n <= 0 || D <= 0 || K <= 0 || L <= 0) return 0;
  return km_layout(n, D, K, L, nullptr, nullptr);
}

extern "C" int mval_kmeans_fit(const double* X, int64_t n, int D, int K, const double* init_centers, int64_t first_idx,
                               const double* rand_u, int L, int max_iter, double tol, double* centers, int* labels,
                               double* inertia, int* n_iter, int64_t* init_idx, void* ws, void* stream) {
  MVAL_REQUIRE(X && centers && labels && inertia && n_iter && init_idx && ws, "mval_kmeans_fit: NULL argument");
  MVAL_REQUIRE(n > 0 && n <= INT32_MAX && D > 0 && D <= KM_MAX_D && K > 0 && K <= KM_THREADS && n >= K &&
                   (int64_t)K * D <= KM_MAX_KD,
               "mval_kmeans_fit: bad dims (n=%lld D=%d K=%d; need K <= n, K <= %d, D <= %d, K*D <= %d)", (long long)n, D,
               K, KM_THREADS, KM_MAX_D, KM_MAX_KD);
  MVAL_REQUIRE(max_iter > 0 && tol >= 0.0, "mval_kmeans_fit: bad max_iter=%d / tol=%g", max_iter, tol);
  MVAL_REQUIRE(init_centers || (L > 0 && L <= KM_MAX_L && first_idx >= 0 && first_idx < n && (rand_u || K == 1)),
               "mval_kmeans_fit: k-means++ needs 0 <= first_idx < n, 1 <= L <= %d and rand_u", KM_MAX_L);
  if (init_centers) L = 1;
  MVAL_REQUIRE((int64_t)L * D <= 2 * KM_MAX_KD, "mval_kmeans_fit: L*D=%lld candidate rows exceed LDS", (long long)L * D);
  hipStream_t s = mval_stream(stream);
  KmWs w;
  km_layout(n, D, K, L, reinterpret_cast<char*>(((uintptr_t)ws + 255) & ~(uintptr_t)255), &w);
  const int nb = km_blocks(n);
  const int E = K * D + K + 1;

  hipLaunchKernelGGL(km_transpose_kernel, dim3(nb), dim3(KM_THREADS), 0, s, X, w.XT, n, D);
  hipLaunchKernelGGL(km_colstats_kernel, dim3(D), dim3(KM_THREADS), 0, s, w.XT, w.mean, w.var, n);
  hipLaunchKernelGGL(km_center_kernel, dim3(nb), dim3(KM_THREADS), 0, s, w.XT, w.Xc, w.mean, w.xnorm, labels, n, D);
  hipLaunchKernelGGL(km_setup_kernel, dim3(1), dim3(64), 0, s, w.var, w.st, w.cand, init_centers ? 0 : first_idx, tol, D);
  MVAL_CHECK_LAUNCH("mval_kmeans_fit/prologue");

  if (!init_centers) {
    double* dbuf[2] = {w.dcand, w.dcand + (size_t)L * n};
    hipLaunchKernelGGL(km_pp_cand_kernel, dim3(nb), dim3(KM_THREADS), (size_t)D * 8, s, w.XT, w.Xc, w.xnorm, w.cand, 1,
                       (const double*)nullptr, dbuf[0], w.ppart, w.st, 1, n, D);
    for (int c = 1; c <= K; c++) {
      const int nc_prev = c == 1 ? 1 : L;
      hipLaunchKernelGGL(km_pp_search_kernel, dim3(1), dim3(KM_THREADS), 0, s, w.ppart, nb, nc_prev, dbuf[(c - 1) & 1],
                         w.cand, init_idx, rand_u, L, c, K, w.st, n);
      if (c == K) break;
      hipLaunchKernelGGL(km_pp_cand_kernel, dim3(nb), dim3(KM_THREADS), (size_t)L * D * 8, s, w.XT, w.Xc, w.xnorm, w.cand,
                         L, dbuf[(c - 1) & 1], dbuf[c & 1], w.ppart, w.st, 0, n, D);
    }
    MVAL_CHECK_LAUNCH("mval_kmeans_fit/seeding");
  } else {
    // -1: no seeding picks
    MVAL_REQUIRE(hipMemsetAsync(init_idx, 0xff, (size_t)K * sizeof(int64_t), s) == hipSuccess,
                 "mval_kmeans_fit: clearing init_idx failed");
  }
  hipLaunchKernelGGL(km_init_centers_kernel, dim3(1), dim3(KM_THREADS), 0, s, w.Xc, init_idx, init_centers, w.mean, w.cen,
                     D, K);
  MVAL_CHECK_LAUNCH("mval_kmeans_fit/init_centers");

  const size_t lds = (size_t)2 * K * D * 8;
  for (int it = 0; it < max_iter; it++) {
    hipLaunchKernelGGL(km_assign_kernel, dim3(nb), dim3(KM_THREADS), lds, s, w.XT, w.Xc, w.cen, labels, w.dist, w.part,
                       w.st, 0, n, D, K);
    hipLaunchKernelGGL(km_reduce_kernel, dim3((E + KM_THREADS - 1) / KM_THREADS), dim3(KM_THREADS), 0, s, w.part, w.red,
                       w.st, nb, E);
    hipLaunchKernelGGL(km_update_kernel, dim3(1), dim3(KM_THREADS), 0, s, w.Xc, labels, w.dist, w.red, w.cen,
                       w.st, max_iter, n, D, K);
    MVAL_CHECK_LAUNCH("mval_kmeans_fit/lloyd");
    if ((it + 1) % KM_CHECK_EVERY == 0 && it + 1 < max_iter) {
      int done = 0;
      if (hipMemcpyAsync(&done, &w.st->done, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess) {
        mval_set_error("mval_kmeans_fit: convergence check failed: %s", hipGetErrorString(hipGetLastError()));
        return -2;
      }
      if (done) break;
    }
  }
  hipLaunchKernelGGL(km_assign_kernel, dim3(nb), dim3(KM_THREADS), (size_t)K * D * 8, s, w.XT, w.Xc, w.cen, labels,
                     w.dist, w.part, w.st, 1, n, D, K);
  hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(KM_THREADS), 0, s, w.part, nb, w.cen, w.mean, centers, inertia,
                     n_iter, w.st, D, K);
  MVAL_CHECK_LAUNCH("mval_kmeans_fit/finish");
  return 0;
}

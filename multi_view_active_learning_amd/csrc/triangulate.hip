// Batched pairwise-RANSAC DLT triangulation + reprojection error (K11), XE metric (K12).
//
// Replaces the per-sample / per-joint / per-pair NumPy loop of the reference
// (utils/triangulation.py:209-233, 260-338, 341-384): C(V,2)+1 LAPACK SVD calls per joint.
//
// Mapping: one (frame, joint) problem per group of PG lanes (PG = pow2 >= C(V,2), <= 64);
// lane p of a group triangulates view pair p and votes inliers over all V views; a
// butterfly picks the first pair with the largest inlier set; the final DLT over the
// sorted inlier views is solved redundantly by the group and written by its lane 0.
//
// The DLT null vector is computed WITHOUT an SVD library and without forming A^T A (which
// squares the condition number: entries of A reach 1e5): rows of the 2n x 4 system are
// folded into a 4x4 upper-triangular R with Givens rotations (backward stable, streaming,
// no 2n-sized array), then a one-sided Jacobi (Hestenes) iteration on R yields the right
// singular vector of the smallest singular value to high relative accuracy.  All float64.
// Latency/ALU-bound; bytes are negligible (V*J*2 ints + V*12 doubles per frame).
//
// Two entries.  mval_triangulate_ransac walks all C(V,2) pairs in lexicographic order (V <= 11: C(V,2) <= 64 = the
// reference's n_iters).  mval_triangulate_ransac_pairs walks an explicit pair table in table order (V <= 32, up to
// C(32,2) = 496 pairs): the pairs the reference drew from python's RNG (utils/triangulation.py:279-282, drawn on the
// host by utils.triangulation.draw_view_pairs), or the lexicographic list of a rig whose pairs all fit a larger
// n_iters.  Up to 64 pairs keep the grouping above; beyond, one wave per problem and lane p takes pairs p, p + 64, ...
// Both kernels are built from the same two stages, vote_pair (a lane triangulates one pair and votes) and
// finish_problem (final DLT over the winner's inlier views), and differ only in where a lane's pairs come from and in
// the width of the reduction key; the host entries share `triangulate` (argument checks, mask kind and key-point dtype
// dispatch, frame_reduce_kernel).
//
// Presence masks (include/mval_hip.h): the `_masked` entries take (mask, mask_kind) and run the MASK instantiation of the same
// kernels; MASKED in a kernel means MASK != MASK_NONE.  MASK is a template parameter: the MASK_NONE instantiations, which the
// unmasked entries and the `_masked` ones with MVAL_MASK_NONE run, compile to the code they were without it.
//
// Frames with missing views: MASK_VIEWS, mask = view_valid [B,V] u8.  A frame's present views are the bits of `present`; a
// pair with an absent view sits out, the vote and the "no usable pair" fallback run over present views only, and nothing of
// an absent view (key-point row, matrix) is read.
//
// Joints missing from single views: MASK_VIEW_JOINT, mask = view_joint_valid [B,V,J] u8.  `present` is then a property of the
// problem (frame, joint), folded from the joint's column of the mask;
// everything a lane does with it is what it does with a frame's word.  A valid joint with fewer than two present views is
// written like an invalid one, and frame_reduce_kernel runs over the USED joints (valid, two or more views) -- which are
// the joints with joint_inliers > 0, a winning pair being part of its own inlier set.
//
// Confidence weights and the winning set (mval_triangulate_ransac_weighted): EXT, a second template parameter
// beside MASK.  EXT_NONE is what the four entries above run: those instantiations compile to the code they were without it.
// EXT_SET also writes the winning inlier set of every problem as a bit mask.  EXT_WEIGHTED multiplies the two DLT rows of view v
// by its weight w_v, in the pair solve and in the final solve; an entry whose weight is not finite and > 0 is absent, so the
// kernels then run masked over `present & usable` whatever MASK is (MASK only says how `present` is read); among hypotheses
// with equally many inliers the larger sum of weights wins, then the lower pair position.  The vote and joint_err stay
// unweighted.  Weights are read again where they are needed (V floats per problem, cached) instead of being kept in registers
// beside finish_problem's error list.
#include "mval_common.h"
#include "numeric_order.h"  // np_pairwise_sum: np.mean's order

#define MAXV 11  // C(11,2) = 55 <= 64 = n_iters: beyond that the reference samples pairs randomly
static_assert(MVAL_PAIRS_MAX_VIEWS == 32, "the inlier mask is 32 bits wide");
static_assert(MVAL_PAIRS_MAX_PAIRS == MVAL_PAIRS_MAX_VIEWS * (MVAL_PAIRS_MAX_VIEWS - 1) / 2 && MVAL_PAIRS_MAX_PAIRS < 512,
              "the reduction key keeps the table position in 9 bits");

struct R4 {
  double r[4][4];  // upper triangular (lower part kept zero)
};

__device__ __forceinline__ void r4_zero(R4& m) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) m.r[i][j] = 0.0;
}

// fold one row a[0..3] into R with 4 Givens rotations
__device__ __forceinline__ void r4_add_row(R4& m, double a0, double a1, double a2, double a3) {
  double a[4] = {a0, a1, a2, a3};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double x = m.r[i][i], y = a[i];
    if (y != 0.0) {
      double h = hypot(x, y);
      double c = x / h, s = y / h;
      m.r[i][i] = h;
      a[i] = 0.0;
#pragma unroll
      for (int j = i + 1; j < 4; j++) {
        double rj = m.r[i][j], aj = a[j];
        m.r[i][j] = c * rj + s * aj;
        a[j] = c * aj - s * rj;
      }
    }
  }
}

// right singular vector of the smallest singular value of the 4x4 matrix R
__device__ __forceinline__ void r4_null_vector(const R4& m, double x[4]) {
  double g[4][4], v[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      g[i][j] = m.r[i][j];
      v[i][j] = (i == j) ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          al = fma(g[k][p], g[k][p], al);
          be = fma(g[k][q], g[k][q], be);
          ga = fma(g[k][p], g[k][q], ga);
        }
        if (fabs(ga) > 1e-17 * sqrt(al * be) && ga != 0.0) {
          rotated = true;
          double zeta = (be - al) / (2.0 * ga);
          double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            double gp = g[k][p], gq = g[k][q];
            g[k][p] = c * gp - s * gq;
            g[k][q] = s * gp + c * gq;
            double vp = v[k][p], vq = v[k][q];
            v[k][p] = c * vp - s * vq;
            v[k][q] = s * vp + c * vq;
          }
        }
      }
    }
    if (!rotated) break;
  }
  double best = INFINITY;
  int bi = 3;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    double n = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) n = fma(g[k][j], g[k][j], n);
    if (n < best) { best = n; bi = j; }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) x[k] = (bi == 0) ? v[k][0] : (bi == 1) ? v[k][1] : (bi == 2) ? v[k][2] : v[k][3];
}

__device__ __forceinline__ void add_view_rows(R4& m, const double* __restrict__ P, double px, double py) {
  // utils/triangulation.py:357-361: x*P[2,:] - P[0,:] ; y*P[2,:] - P[1,:]
  r4_add_row(m, px * P[8] - P[0], px * P[9] - P[1], px * P[10] - P[2], px * P[11] - P[3]);
  r4_add_row(m, py * P[8] - P[4], py * P[9] - P[5], py * P[10] - P[6], py * P[11] - P[7]);
}

// the same rows scaled by the view's weight: every element formed as above, then multiplied once (w = 1: the same bits)
__device__ __forceinline__ void add_view_rows(R4& m, const double* __restrict__ P, double px, double py, double w) {
  r4_add_row(m, (px * P[8] - P[0]) * w, (px * P[9] - P[1]) * w, (px * P[10] - P[2]) * w, (px * P[11] - P[3]) * w);
  r4_add_row(m, (py * P[8] - P[4]) * w, (py * P[9] - P[5]) * w, (py * P[10] - P[6]) * w, (py * P[11] - P[7]) * w);
}

__device__ __forceinline__ void dehomogenise(const double h[4], double X[3]) {
  double w = (h[3] == 0.0) ? 1.0 : h[3];  // utils/triangulation.py:397-399
  X[0] = h[0] / w;
  X[1] = h[1] / w;
  X[2] = h[2] / w;
}

// utils/triangulation.py:371-384,459-477: 1/2 * || pt - pi(P [X;1]) ||
__device__ __forceinline__ double reproj_err(const double* __restrict__ P, const double X[3], double px, double py) {
  double u = fma(X[2], P[2], fma(X[1], P[1], X[0] * P[0])) + P[3];
  double v = fma(X[2], P[6], fma(X[1], P[5], X[0] * P[4])) + P[7];
  double w = fma(X[2], P[10], fma(X[1], P[9], X[0] * P[8])) + P[11];
  if (w == 0.0) w = 1.0;
  double dx = px - u / w, dy = py - v / w;
  return 0.5 * sqrt(dx * dx + dy * dy);
}

// stage 1 of one lane: triangulate the view pair (a, c) and vote over all V views -> inlier mask (a and c always in it)
// (MASKED: over the views of `present` only; WT: the pair's rows weighted by wb[v * J])
template <bool MASKED = false, bool WT = false, typename KP>
__device__ __forceinline__ unsigned vote_pair(const double* __restrict__ Pb, const KP* __restrict__ kb, int V, int J,
                                              int a, int c, double eps, unsigned present = 0u,
                                              const float* __restrict__ wb = nullptr) {
  R4 m;
  r4_zero(m);
  if (WT) {
    add_view_rows(m, Pb + a * 12, (double)kb[(int64_t)a * J * 2], (double)kb[(int64_t)a * J * 2 + 1], (double)wb[(int64_t)a * J]);
    add_view_rows(m, Pb + c * 12, (double)kb[(int64_t)c * J * 2], (double)kb[(int64_t)c * J * 2 + 1], (double)wb[(int64_t)c * J]);
  } else {
    add_view_rows(m, Pb + a * 12, (double)kb[(int64_t)a * J * 2], (double)kb[(int64_t)a * J * 2 + 1]);
    add_view_rows(m, Pb + c * 12, (double)kb[(int64_t)c * J * 2], (double)kb[(int64_t)c * J * 2 + 1]);
  }
  double h[4], X[3];
  r4_null_vector(m, h);
  dehomogenise(h, X);
  unsigned mask = (1u << a) | (1u << c);
  for (int v = 0; v < V; v++) {
    if (MASKED && !(present >> v & 1)) continue;
    double e = reproj_err(Pb + v * 12, X, (double)kb[(int64_t)v * J * 2], (double)kb[(int64_t)v * J * 2 + 1]);
    if (e < eps) mask |= 1u << v;
  }
  return mask;
}

// stage 2, one lane per problem: final DLT on the sorted inlier views `win`, its mean reprojection error and the count
// (NMAX: the most views a caller's `win` can name; WT: the rows weighted by wb[v * J], the errors and their mean are not)
template <int NMAX, bool WT = false, typename KP>
__device__ __forceinline__ void finish_problem(const double* __restrict__ Pb, const KP* __restrict__ kb, int V, int J,
                                               unsigned win, bool is_valid, double* __restrict__ X3,
                                               double* __restrict__ err_out, int32_t* __restrict__ inl_out,
                                               const float* __restrict__ wb = nullptr) {
  if (!is_valid) {
    X3[0] = X3[1] = X3[2] = 0.0;
    *err_out = 0.0;
    *inl_out = 0;
    return;
  }
  R4 m;
  r4_zero(m);
  for (int v = 0; v < V; v++) {
    if (!(win >> v & 1)) continue;
    if (WT) add_view_rows(m, Pb + v * 12, (double)kb[(int64_t)v * J * 2], (double)kb[(int64_t)v * J * 2 + 1], (double)wb[(int64_t)v * J]);
    else add_view_rows(m, Pb + v * 12, (double)kb[(int64_t)v * J * 2], (double)kb[(int64_t)v * J * 2 + 1]);
  }
  double h[4], X[3];
  r4_null_vector(m, h);
  dehomogenise(h, X);
  double errs[NMAX];
  int n = 0;
  for (int v = 0; v < V; v++)
    if (win >> v & 1)
      errs[n++] = reproj_err(Pb + v * 12, X, (double)kb[(int64_t)v * J * 2], (double)kb[(int64_t)v * J * 2 + 1]);
  X3[0] = X[0];
  X3[1] = X[1];
  X3[2] = X[2];
  *err_out = np_pairwise_sum(errs, n) / (double)n;
  *inl_out = n;
}

// the present views of a frame as bits (vv: the frame's row of view_valid, V <= 32)
__device__ __forceinline__ unsigned present_views(const uint8_t* __restrict__ vv, int V) {
  unsigned m = 0;
  for (int v = 0; v < V; v++)
    if (vv[v]) m |= 1u << v;
  return m;
}

// the present views of one problem as bits: of its frame (MASK_VIEWS, mask [B,V]) or of its joint in that frame
// (MASK_VIEW_JOINT, mask [B,V,J])
template <int MASK>
__device__ __forceinline__ unsigned present_of(const uint8_t* __restrict__ mask, int64_t b, int j, int V, int J) {
  if (MASK == MASK_VIEWS) return present_views(mask + b * V, V);
  unsigned m = 0;
  if (MASK == MASK_VIEW_JOINT)
    for (int v = 0; v < V; v++)
      if (mask[(b * V + v) * J + j]) m |= 1u << v;
  return m;
}

// What a kernel does beyond the four original entries, and the arguments that takes (the kernels' last parameter; none for
// EXT_NONE).  inlier_mask [B*J] may be NULL under EXT_WEIGHTED.
enum { EXT_NONE = 0, EXT_SET = 1, EXT_WEIGHTED = 2 };
template <int EXT>
struct TriExt {};
template <>
struct TriExt<EXT_SET> {
  int32_t* inlier_mask;
};
template <>
struct TriExt<EXT_WEIGHTED> {
  int32_t* inlier_mask;
  const float* weights;
};

__device__ __forceinline__ unsigned all_views(int V) { return (V >= 32) ? 0xffffffffu : ((1u << V) - 1u); }

// the views of `present` whose weight is usable, finite and > 0 (wb: the problem's weights, + v * J); the weight of an absent
// view is not read
__device__ __forceinline__ unsigned usable_views(const float* __restrict__ wb, unsigned present, int V, int J) {
  unsigned m = 0;
  for (int v = 0; v < V; v++) {
    if (!(present >> v & 1)) continue;
    const float w = wb[(int64_t)v * J];
    if (isfinite(w) && w > 0.f) m |= 1u << v;
  }
  return m;
}

// S of a hypothesis: the sum of its views' weights, views ascending, float64
__device__ __forceinline__ double set_weight(const float* __restrict__ wb, unsigned set, int V, int J) {
  double s = 0.0;
  for (int v = 0; v < V; v++)
    if (set >> v & 1) s += (double)wb[(int64_t)v * J];
  return s;
}

// the weighted ranking of two hypotheses (key = count << SHIFT | (positions - 1 - position), S): more inliers, then the larger
// S, then the lower position.  No set (key -1) loses to any.
template <int SHIFT>
__device__ __forceinline__ bool ranks_before(int ka, double sa, int kb, double sb) {
  if ((ka >> SHIFT) != (kb >> SHIFT)) return ka > kb;
  if (sa != sb) return sa > sb;
  return ka > kb;
}

// All C(V,2) pairs in lexicographic order, pair p on lane p of the problem's group (V <= MAXV: n_pairs <= 64).
// MASKED: lane p keeps its pair and sits out when one of its views is absent; the pairs that take part are the
// lexicographic pairs of the present views in the same relative order, so the key picks the winner the unmasked
// kernel picks on the frame's present views alone.  Fewer than two present views: the problem is written as an
// invalid joint's (frame_reduce_kernel marks the frame).  MASK_VIEW_JOINT: the same with the problem's own `present`.
template <int MASK, int EXT, typename KP>
__global__ __launch_bounds__(64) void ransac_dlt_kernel(const KP* __restrict__ kp2d, const double* __restrict__ proj,
                                                         const uint8_t* __restrict__ valid,
                                                         const uint8_t* __restrict__ view_valid,
                                                         double* __restrict__ kp3d, double* __restrict__ joint_err,
                                                         int32_t* __restrict__ joint_inliers, int64_t n_prob, int V,
                                                         int J, int n_pairs, int PG, double eps, TriExt<EXT> ext) {
  const int lane = threadIdx.x;
  const int grp = lane / PG, p = lane % PG;
  const int64_t prob = (int64_t)blockIdx.x * (64 / PG) + grp;
  const bool live = prob < n_prob;
  const int64_t pr = live ? prob : 0;
  const int64_t b = pr / J;
  const int j = (int)(pr % J);
  const bool is_valid = live && (!valid || valid[b * J + j]);
  const double* Pb = proj + b * V * 12;
  const KP* kb = kp2d + (b * V * (int64_t)J + j) * 2;  // + v * J * 2

  constexpr bool WT = EXT == EXT_WEIGHTED;
  constexpr bool MASKED = MASK != MASK_NONE || WT;
  unsigned present = present_of<MASK>(view_valid, b, j, V, J);
  const float* wb = nullptr;  // + v * J
  if constexpr (WT) {
    wb = ext.weights + b * V * (int64_t)J + j;
    present = usable_views(wb, MASK == MASK_NONE ? all_views(V) : present, V, J);
  }

  unsigned mask = 0;
  bool voted = false;
  if (p < n_pairs) {
    int a = 0, rem = p;
    while (rem >= V - 1 - a) { rem -= V - 1 - a; a++; }
    const int c = a + 1 + rem;
    voted = !MASKED || ((present >> a & 1) && (present >> c & 1));
    if (voted) mask = vote_pair<MASKED, WT>(Pb, kb, V, J, a, c, eps, present, wb);
  }
  // first pair with the strictly largest set: key = count * 64 + (63 - p), maximise
  int key = voted ? __popc(mask) * 64 + (63 - p) : -1;
  int best = key;
  if constexpr (WT) {  // (count, S, position): the key travels with its S
    double best_s = voted ? set_weight(wb, mask, V, J) : 0.0;
    for (int o = PG >> 1; o > 0; o >>= 1) {
      const int k = __shfl_xor(best, o, 64);
      const double s = __shfl_xor(best_s, o, 64);
      if (ranks_before<6>(k, s, best, best_s)) { best = k; best_s = s; }
    }
  } else {
    for (int o = PG >> 1; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  }
  unsigned win = (key == best) ? mask : 0u;
  for (int o = PG >> 1; o > 0; o >>= 1) win |= __shfl_xor(win, o, 64);

  if (p != 0 || !live) return;
  // (MASKED, two or more present views: at least one pair voted, so `win` is never the unmasked kernel's empty set)
  const bool used = is_valid && (!MASKED || __popc(present) >= 2);
  finish_problem<MAXV, WT>(Pb, kb, V, J, win, used, kp3d + pr * 3, joint_err + pr, joint_inliers + pr, wb);
  if constexpr (EXT != EXT_NONE)
    if (ext.inlier_mask) ext.inlier_mask[pr] = used ? (int32_t)win : 0;
}

// The same two stages over an explicit pair table (pairs_stride = P * 2 per problem, 0 for one shared table).  A lane
// walks its pairs in ascending table position and keeps the first strictly larger set, the butterfly then prefers the
// lowest position among equal counts: the winner is the first position with the largest set (utils/triangulation.py
// :299-300).  key = count * 512 + (511 - position) <= 32 * 512 + 511.  An entry that names a view >= V takes no part.
// MASKED: neither does one that names an absent view, and the fallback is all PRESENT views.
template <int MASK, int EXT, typename KP>
__global__ __launch_bounds__(64) void ransac_pairs_kernel(const KP* __restrict__ kp2d, const double* __restrict__ proj,
                                                           const uint8_t* __restrict__ valid,
                                                           const uint8_t* __restrict__ view_valid,
                                                           const uint8_t* __restrict__ pairs, int64_t pairs_stride,
                                                           double* __restrict__ kp3d, double* __restrict__ joint_err,
                                                           int32_t* __restrict__ joint_inliers, int64_t n_prob, int V,
                                                           int J, int P, int PG, double eps, TriExt<EXT> ext) {
  const int lane = threadIdx.x;
  const int grp = lane / PG, p0 = lane % PG;
  const int64_t prob = (int64_t)blockIdx.x * (64 / PG) + grp;
  const bool live = prob < n_prob;
  const int64_t pr = live ? prob : 0;
  const int64_t b = pr / J;
  const int j = (int)(pr % J);
  const bool is_valid = live && (!valid || valid[b * J + j]);
  const double* Pb = proj + b * V * 12;
  const KP* kb = kp2d + (b * V * (int64_t)J + j) * 2;  // + v * J * 2
  const uint8_t* tab = pairs + pr * pairs_stride;
  constexpr bool WT = EXT == EXT_WEIGHTED;
  constexpr bool MASKED = MASK != MASK_NONE || WT;
  unsigned present = present_of<MASK>(view_valid, b, j, V, J);
  const float* wb = nullptr;  // + v * J
  if constexpr (WT) {
    wb = ext.weights + b * V * (int64_t)J + j;
    present = usable_views(wb, MASK == MASK_NONE ? all_views(V) : present, V, J);
  }

  int key = -1;
  unsigned mask = 0;
  double key_s = 0.0;  // (WT) S of the lane's best set
  if (is_valid)  // (an invalid joint has no table: the reference skips it before the draw)
    for (int p = p0; p < P; p += 64) {  // PG < 64 means P <= PG: one trip
      int a = tab[p * 2], c = tab[p * 2 + 1];
      if (a >= V || c >= V) continue;
      if (MASKED && !((present >> a & 1) && (present >> c & 1))) continue;
      unsigned m = vote_pair<MASKED, WT>(Pb, kb, V, J, a, c, eps, present, wb);
      int k = __popc(m) * 512 + (511 - p);
      if constexpr (WT) {  // (a later trip has the higher position: it wins on count or on S alone)
        const double s = set_weight(wb, m, V, J);
        if (ranks_before<9>(k, s, key, key_s)) { key = k; key_s = s; mask = m; }
      } else {
        if ((k >> 9) > (key >> 9)) { key = k; mask = m; }  // key = -1 >> 9 = -1: any set beats none
      }
    }
  int best = key;
  if constexpr (WT) {
    double best_s = key_s;
    for (int o = PG >> 1; o > 0; o >>= 1) {
      const int k = __shfl_xor(best, o, 64);
      const double s = __shfl_xor(best_s, o, 64);
      if (ranks_before<9>(k, s, best, best_s)) { best = k; best_s = s; }
    }
  } else {
    for (int o = PG >> 1; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  }
  unsigned win = (key == best) ? mask : 0u;
  for (int o = PG >> 1; o > 0; o >>= 1) win |= __shfl_xor(win, o, 64);

  if (p0 != 0 || !live) return;
  if (best < 0) win = MASKED ? present : all_views(V);  // no usable pair: all views (:303-304)
  const bool used = is_valid && (!MASKED || __popc(present) >= 2);
  finish_problem<MVAL_PAIRS_MAX_VIEWS, WT>(Pb, kb, V, J, win, used, kp3d + pr * 3, joint_err + pr, joint_inliers + pr, wb);
  if constexpr (EXT != EXT_NONE)
    if (ext.inlier_mask) ext.inlier_mask[pr] = used ? (int32_t)win : 0;
}

// per frame: metric = np.mean(errs of valid joints), inlier_count = min (utils/triangulation.py:226,231)
// MASKED: a frame with a valid joint and fewer than two present views gets metric NaN and inlier_count -2 (the reference
// asserts len(points) >= 2 inside the first valid joint, :268); without a valid joint it stays -1 (np.min([]) comes
// without any assert).
// MASK_VIEW_JOINT: mean and min run over the used joints, those with joint_inliers > 0 (a valid joint with fewer than two
// present views was written with 0, as an invalid one); a valid joint but no used one: metric NaN, inlier_count -2.
template <int MASK>
__global__ void frame_reduce_kernel(const double* __restrict__ joint_err, const int32_t* __restrict__ joint_inliers,
                                    const uint8_t* __restrict__ valid, const uint8_t* __restrict__ view_valid,
                                    double* __restrict__ metric, int32_t* __restrict__ inlier_count, int B, int V, int J) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (MASK == MASK_VIEWS && __popc(present_views(view_valid + (int64_t)b * V, V)) < 2) {
    bool any = false;
    for (int j = 0; j < J; j++) any |= !valid || valid[(int64_t)b * J + j];
    metric[b] = NAN;
    inlier_count[b] = any ? -2 : -1;
    return;
  }
  double buf[512];
  int n = 0, mn = 0x7fffffff;
  bool any = false;
  for (int j = 0; j < J; j++) {
    if (valid && !valid[(int64_t)b * J + j]) continue;
    any = true;
    if (MASK == MASK_VIEW_JOINT && joint_inliers[(int64_t)b * J + j] <= 0) continue;
    buf[n++] = joint_err[(int64_t)b * J + j];
    mn = min(mn, joint_inliers[(int64_t)b * J + j]);
  }
  metric[b] = n ? np_pairwise_sum(buf, n) / (double)n : NAN;
  inlier_count[b] = n ? mn : (MASK == MASK_VIEW_JOINT && any) ? -2 : -1;
}

// frame_reduce_kernel of the mask kind: the last launch of the triangulation entries and of mval_refine_points_3d
static void launch_frame_reduce(const double* joint_err, const int32_t* joint_inliers, const uint8_t* valid,
                                const uint8_t* mask, int mask_kind, double* metric, int32_t* inlier_count, int B, int V, int J,
                                hipStream_t s) {
  with_mask_kind(mask_kind, [&](auto K) {
    hipLaunchKernelGGL(frame_reduce_kernel<decltype(K)::value>, dim3((B + 63) / 64), dim3(64), 0, s, joint_err, joint_inliers,
                       valid, mask, metric, inlier_count, B, V, J);
  });
}

// The one place where the two optional arguments of mval_triangulate_ransac_weighted pick an instantiation: f gets EXT as a
// std::integral_constant and the kernels' last argument (with_mask_kind's way).
template <typename F>
static inline void with_ext(const float* weights, int32_t* inlier_mask, F&& f) {
  if (weights) f(std::integral_constant<int, EXT_WEIGHTED>{}, TriExt<EXT_WEIGHTED>{inlier_mask, weights});
  else if (inlier_mask) f(std::integral_constant<int, EXT_SET>{}, TriExt<EXT_SET>{inlier_mask});
  else f(std::integral_constant<int, EXT_NONE>{}, TriExt<EXT_NONE>{});
}

// The five triangulation entries: `name` is the one that was called, `pairs` its table or nullptr for the lexicographic
// kernel, `weights` and `joint_inlier_mask` nullptr for the four entries that have neither.  Argument checks, the grid of PG-lane
// groups, the entry's kernel for the mask kind, EXT and the key-point type, and frame_reduce_kernel -- in its used-joints form
// under weights, whose unusable entries make presence a property of the problem whatever the mask kind.
static int triangulate(const char* name, const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                       const uint8_t* mask, int mask_kind, const uint8_t* pairs, int P, int pairs_shared, double* kp3d,
                       double* joint_err, int32_t* joint_inliers, double* metric, int32_t* inlier_count, int B, int V, int J,
                       double eps, void* stream, const float* weights = nullptr, int32_t* joint_inlier_mask = nullptr) {
  MVAL_REQUIRE(V >= 2, "%s: need >= 2 views in the rig (the reference asserts len(points) >= 2)", name);
  if (pairs) {
    MVAL_REQUIRE(V <= MVAL_PAIRS_MAX_VIEWS, "%s: at most %d views (the inlier mask is 32 bits wide)", name, MVAL_PAIRS_MAX_VIEWS);
    MVAL_REQUIRE(P >= 1 && P <= MVAL_PAIRS_MAX_PAIRS, "%s: need a pair table of 1..%d pairs", name, MVAL_PAIRS_MAX_PAIRS);
  } else {
    MVAL_REQUIRE(V <= MAXV, "%s: V > 11 takes a pair table (the reference samples pairs from python's RNG there)", name);
  }
  MVAL_REQUIRE_MASK(name, mask, mask_kind);
  MVAL_REQUIRE(J >= 1 && J <= 512 && B >= 0, "%s: bad dims", name);
  if (B == 0) return 0;
  const int n_pairs = pairs ? P : V * (V - 1) / 2;
  int PG = 1;  // lanes per problem: pow2 >= n_pairs, one wave beyond 64 pairs
  while (PG < n_pairs && PG < 64) PG <<= 1;
  const int64_t stride = pairs_shared ? 0 : (int64_t)P * 2;
  const int64_t n_prob = (int64_t)B * J;
  const int per_block = 64 / PG;
  const dim3 grid((unsigned)((n_prob + per_block - 1) / per_block));
  const hipStream_t s = mval_stream(stream);
  with_mask_kind(mask_kind, [&](auto K) {
    constexpr int MASK = decltype(K)::value;
    with_ext(weights, joint_inlier_mask, [&](auto E, auto ext) {
      constexpr int EXT = decltype(E)::value;
      const auto launch = [&](auto* kp) {
        if (pairs)
          hipLaunchKernelGGL(HIP_KERNEL_NAME(ransac_pairs_kernel<MASK, EXT>), grid, dim3(64), 0, s, kp, proj, valid, mask, pairs,
                             stride, kp3d, joint_err, joint_inliers, n_prob, V, J, P, PG, eps, ext);
        else
          hipLaunchKernelGGL(HIP_KERNEL_NAME(ransac_dlt_kernel<MASK, EXT>), grid, dim3(64), 0, s, kp, proj, valid, mask, kp3d,
                             joint_err, joint_inliers, n_prob, V, J, n_pairs, PG, eps, ext);
      };
      if (kp_is_f32) launch((const float*)kp2d);
      else launch((const int64_t*)kp2d);
    });
  });
  MVAL_CHECK_LAUNCH(name);
  launch_frame_reduce(joint_err, joint_inliers, valid, mask, weights ? MASK_VIEW_JOINT : mask_kind, metric, inlier_count, B, V, J, s);
  MVAL_CHECK_LAUNCH_STAGE(name, "/reduce");
  return 0;
}

extern "C" int mval_triangulate_ransac(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                       double* kp3d, double* joint_err, int32_t* joint_inliers, double* metric,
                                       int32_t* inlier_count, int B, int V, int J, double eps, void* stream) {
  return triangulate("mval_triangulate_ransac", kp2d, kp_is_f32, proj, valid, nullptr, MASK_NONE, nullptr, 0, 0, kp3d, joint_err,
                     joint_inliers, metric, inlier_count, B, V, J, eps, stream);
}

extern "C" int mval_triangulate_ransac_masked(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                              const uint8_t* mask, int mask_kind, double* kp3d, double* joint_err,
                                              int32_t* joint_inliers, double* metric, int32_t* inlier_count, int B, int V,
                                              int J, double eps, void* stream) {
  return triangulate("mval_triangulate_ransac_masked", kp2d, kp_is_f32, proj, valid, mask, mask_kind, nullptr, 0, 0, kp3d,
                     joint_err, joint_inliers, metric, inlier_count, B, V, J, eps, stream);
}

// (a NULL table is the pairs entries' own fault: `triangulate` would take it for the lexicographic kernel)
extern "C" int mval_triangulate_ransac_pairs(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                             const uint8_t* pairs, int P, int pairs_shared, double* kp3d,
                                             double* joint_err, int32_t* joint_inliers, double* metric,
                                             int32_t* inlier_count, int B, int V, int J, double eps, void* stream) {
  MVAL_REQUIRE(pairs, "mval_triangulate_ransac_pairs: need a pair table (pairs is NULL)");
  return triangulate("mval_triangulate_ransac_pairs", kp2d, kp_is_f32, proj, valid, nullptr, MASK_NONE, pairs, P, pairs_shared,
                     kp3d, joint_err, joint_inliers, metric, inlier_count, B, V, J, eps, stream);
}

extern "C" int mval_triangulate_ransac_pairs_masked(const void* kp2d, int kp_is_f32, const double* proj,
                                                    const uint8_t* valid, const uint8_t* mask, int mask_kind,
                                                    const uint8_t* pairs, int P, int pairs_shared, double* kp3d,
                                                    double* joint_err, int32_t* joint_inliers, double* metric,
                                                    int32_t* inlier_count, int B, int V, int J, double eps, void* stream) {
  MVAL_REQUIRE(pairs, "mval_triangulate_ransac_pairs_masked: need a pair table (pairs is NULL)");
  return triangulate("mval_triangulate_ransac_pairs_masked", kp2d, kp_is_f32, proj, valid, mask, mask_kind, pairs, P,
                     pairs_shared, kp3d, joint_err, joint_inliers, metric, inlier_count, B, V, J, eps, stream);
}

// Both kernels, any mask kind, with per-entry weights and / or the winning set handed out.  Neither given: the
// `_masked` entry of the same table, call for call.
extern "C" int mval_triangulate_ransac_weighted(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                                const uint8_t* mask, int mask_kind, const uint8_t* pairs, int P,
                                                int pairs_shared, const float* weights, double* kp3d, double* joint_err,
                                                int32_t* joint_inliers, int32_t* joint_inlier_mask, double* metric,
                                                int32_t* inlier_count, int B, int V, int J, double eps, void* stream) {
  MVAL_REQUIRE(((uintptr_t)weights | (uintptr_t)joint_inlier_mask) % 4 == 0,
               "mval_triangulate_ransac_weighted: weights or joint_inlier_mask is not 4-byte aligned");
  return triangulate("mval_triangulate_ransac_weighted", kp2d, kp_is_f32, proj, valid, mask, mask_kind, pairs, P, pairs_shared,
                     kp3d, joint_err, joint_inliers, metric, inlier_count, B, V, J, eps, stream, weights, joint_inlier_mask);
}

// ---- 3-D refinement (not in the reference) ---------------------------------------------------------------
// Every triangulated joint is moved from its DLT point X0 to the minimiser of the reprojection error over its support set S:
// the present views whose reproj_err at X0 is finite and < eps (with weights: and whose weight is finite and > 0) -- the
// vote's test, taken again at the final point (not the winning set mval_triangulate_ransac_weighted can hand out: the support
// set is defined at the DLT point, whichever entry made it).
//   E(X) = 1/2 sum_{v in S} w_v |p_v - pi(P_v [X; 1])|^2,  two smooth residuals per view.
// One lane per problem, like mval_refine_keypoints: no LDS, no atomics, nothing indexed by a loaded value; the loops run over
// v < V <= 32 in ascending order, so a problem's bits do not depend on its place in the batch.  Levenberg-Marquardt in float64
// with the analytic 2x3 Jacobian, the 3x3 system (A + lam diag A) d = g solved in registers (LDL^T; a pivot that is not > 0
// counts as a rejected step).  One iteration = one trial point = one pass over S that gives E, A and g there.
// The accept test E(X + d) <= E(X) cannot tell two points apart that are closer than about 1e-6 mm (the cost moves by less
// than its own rounding there), so near the minimum the decisions are taken by the last bit of E.  The solver's arithmetic
// is therefore part of the definition: the operations below in the order written, one IEEE operation each, no FMA
// contraction (refine_normal, refine_solve and the loop), with the correctly rounded float64 division and square root.  The
// float64 oracle on the host (tests/refine3d_oracle.py) follows the same order and takes the same decisions.
struct Normal3 {
  double E, a00, a01, a02, a11, a12, a22, g0, g1, g2;
  bool front;  // every support view has depth > 0
};

template <typename KP>
__device__ __forceinline__ void refine_normal(const double* __restrict__ Pb, const KP* __restrict__ kb,
                                              const float* __restrict__ wb, int V, int J, unsigned S, const double X[3],
                                              Normal3& n) {
#pragma clang fp contract(off)
  n.E = n.a00 = n.a01 = n.a02 = n.a11 = n.a12 = n.a22 = n.g0 = n.g1 = n.g2 = 0.0;
  n.front = true;
  for (int v = 0; v < V; v++) {
    if (!(S >> v & 1)) continue;
    const double* P = Pb + v * 12;
    const double px = (double)kb[(int64_t)v * J * 2], py = (double)kb[(int64_t)v * J * 2 + 1];
    const double wt = wb ? (double)wb[(int64_t)v * J] : 1.0;
    const double h0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double h1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double h2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    n.front = n.front && h2 > 0.0;
    const double u = h0 / h2, w = h1 / h2;
    const double rx = px - u, ry = py - w;
    const double x0 = (P[0] - u * P[8]) / h2, x1 = (P[1] - u * P[9]) / h2, x2 = (P[2] - u * P[10]) / h2;
    const double y0 = (P[4] - w * P[8]) / h2, y1 = (P[5] - w * P[9]) / h2, y2 = (P[6] - w * P[10]) / h2;
    n.a00 += wt * (x0 * x0 + y0 * y0);
    n.a01 += wt * (x0 * x1 + y0 * y1);
    n.a02 += wt * (x0 * x2 + y0 * y2);
    n.a11 += wt * (x1 * x1 + y1 * y1);
    n.a12 += wt * (x1 * x2 + y1 * y2);
    n.a22 += wt * (x2 * x2 + y2 * y2);
    n.g0 += wt * (x0 * rx + y0 * ry);
    n.g1 += wt * (x1 * rx + y1 * ry);
    n.g2 += wt * (x2 * rx + y2 * ry);
    n.E += wt * (rx * rx + ry * ry);
  }
  n.E *= 0.5;
}

// (A + lam diag A) d = g by LDL^T; false when a pivot is not > 0 or the step is not finite
__device__ __forceinline__ bool refine_solve(const Normal3& n, double lam, double d[3]) {
#pragma clang fp contract(off)
  const double m00 = n.a00 + lam * n.a00, m11 = n.a11 + lam * n.a11, m22 = n.a22 + lam * n.a22;
  const double d0 = m00;
  if (!(d0 > 0.0)) return false;
  const double l10 = n.a01 / d0, l20 = n.a02 / d0;
  const double d1 = m11 - l10 * n.a01;
  if (!(d1 > 0.0)) return false;
  const double l21 = (n.a12 - l20 * n.a01) / d1;
  const double d2 = m22 - l20 * n.a02 - l21 * l21 * d1;
  if (!(d2 > 0.0)) return false;
  const double y0 = n.g0, y1 = n.g1 - l10 * y0, y2 = n.g2 - l20 * y0 - l21 * y1;
  d[2] = y2 / d2;
  d[1] = y1 / d1 - l21 * d[2];
  d[0] = y0 / d0 - l10 * d[1] - l20 * d[2];
  return isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
}

template <int MASK, typename KP>
__global__ __launch_bounds__(64) void refine_points_3d_kernel(
    const KP* __restrict__ kp2d, const double* __restrict__ proj, const uint8_t* __restrict__ valid,
    const uint8_t* __restrict__ mask, const float* __restrict__ weights, const double* __restrict__ kp3d,
    const double* __restrict__ joint_err, double* __restrict__ kp3d_out, double* __restrict__ joint_err_out,
    int32_t* __restrict__ joint_support, int32_t* __restrict__ joint_status, int64_t n_prob, int V, int J, double eps) {
  const int64_t pr = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (pr >= n_prob) return;
  const int64_t b = pr / J;
  const int j = (int)(pr % J);
  const double* Pb = proj + b * V * 12;
  const KP* kb = kp2d + (b * V * (int64_t)J + j) * 2;                        // + v * J * 2
  const float* wb = weights ? weights + b * V * (int64_t)J + j : nullptr;  // + v * J
  double X[3] = {kp3d[pr * 3], kp3d[pr * 3 + 1], kp3d[pr * 3 + 2]};
  double err = joint_err[pr];
  int status = 0;

  unsigned S = 0;
  if ((!valid || valid[pr]) && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2])) {
    const unsigned present = MASK == MASK_NONE ? ((V >= 32) ? 0xffffffffu : ((1u << V) - 1u)) : present_of<MASK>(mask, b, j, V, J);
    for (int v = 0; v < V; v++) {
      if (!(present >> v & 1)) continue;
      const double e = reproj_err(Pb + v * 12, X, (double)kb[(int64_t)v * J * 2], (double)kb[(int64_t)v * J * 2 + 1]);
      bool in = isfinite(e) && e < eps;
      if (in && wb) {
        const float w = wb[(int64_t)v * J];
        in = isfinite(w) && w > 0.f;
      }
      if (in) S |= 1u << v;
    }
  }
  const int n = __popc(S);

  if (n >= 2) {
#pragma clang fp contract(off)
    double lam = 1e-3;
    Normal3 cur;
    refine_normal(Pb, kb, wb, V, J, S, X, cur);
    status = -MVAL_REFINE3D_MAX_ITERS;
    for (int k = 1; k <= MVAL_REFINE3D_MAX_ITERS; k++) {
      double d[3], Xt[3];
      Normal3 t;
      bool ok = refine_solve(cur, lam, d);
      if (ok) {
        Xt[0] = X[0] + d[0];
        Xt[1] = X[1] + d[1];
        Xt[2] = X[2] + d[2];
        refine_normal(Pb, kb, wb, V, J, S, Xt, t);
        ok = t.front && t.E <= cur.E;  // (a NaN cost compares false)
      }
      if (ok) {
        X[0] = Xt[0];
        X[1] = Xt[1];
        X[2] = Xt[2];
        cur = t;
        lam = fmax(lam / 10.0, 1e-9);
        if (sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) <= 1e-8 * (1.0 + sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]))) {
          status = k;
          break;
        }
      } else {
        lam *= 10.0;
        if (lam > 1e12) {  // no damping lowers the cost: the iterate is at the float64 floor
          status = k;
          break;
        }
      }
    }
    double errs[MVAL_PAIRS_MAX_VIEWS];
    int m = 0;
    for (int v = 0; v < V; v++)
      if (S >> v & 1)
        errs[m++] = reproj_err(Pb + v * 12, X, (double)kb[(int64_t)v * J * 2], (double)kb[(int64_t)v * J * 2 + 1]);
    err = np_pairwise_sum(errs, m) / (double)m;
  }
  kp3d_out[pr * 3] = X[0];
  kp3d_out[pr * 3 + 1] = X[1];
  kp3d_out[pr * 3 + 2] = X[2];
  joint_err_out[pr] = err;
  joint_support[pr] = n;
  joint_status[pr] = status;
}

extern "C" int mval_refine_points_3d(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                     const uint8_t* mask, int mask_kind, const float* weights, const double* kp3d,
                                     const double* joint_err, const int32_t* joint_inliers, double* kp3d_out,
                                     double* joint_err_out, int32_t* joint_support, int32_t* joint_status, double* metric,
                                     int32_t* inlier_count, int B, int V, int J, double eps, void* stream) {
  MVAL_REQUIRE(V >= 2 && V <= MVAL_PAIRS_MAX_VIEWS, "mval_refine_points_3d: 2..%d views (the support set is 32 bits wide)", MVAL_PAIRS_MAX_VIEWS);
  MVAL_REQUIRE(J >= 1 && J <= 512 && B >= 0, "mval_refine_points_3d: bad dims");
  MVAL_REQUIRE_MASK("mval_refine_points_3d", mask, mask_kind);
  if (B == 0) return 0;
  MVAL_REQUIRE(kp2d && proj && kp3d && joint_err && joint_inliers, "mval_refine_points_3d: an input is NULL");
  MVAL_REQUIRE(kp3d_out && joint_err_out && joint_support && joint_status && metric && inlier_count, "mval_refine_points_3d: an output is NULL");
  MVAL_REQUIRE(kp3d_out != kp3d && joint_err_out != joint_err, "mval_refine_points_3d: the outputs must not alias the inputs");
  MVAL_REQUIRE(((uintptr_t)proj | (uintptr_t)kp3d | (uintptr_t)joint_err | (uintptr_t)kp3d_out | (uintptr_t)joint_err_out | (uintptr_t)metric) % 8 == 0,
               "mval_refine_points_3d: a float64 array is not 8-byte aligned");
  MVAL_REQUIRE(((uintptr_t)kp2d % (kp_is_f32 ? 4 : 8)) == 0 && ((uintptr_t)weights | (uintptr_t)joint_inliers | (uintptr_t)joint_support | (uintptr_t)joint_status | (uintptr_t)inlier_count) % 4 == 0,
               "mval_refine_points_3d: a 4-byte array is not aligned");
  const hipStream_t s = mval_stream(stream);
  const int64_t n_prob = (int64_t)B * J;
  const dim3 grid((unsigned)((n_prob + 63) / 64));
  with_mask_kind(mask_kind, [&](auto K) {
    constexpr int MASK = decltype(K)::value;
    if (kp_is_f32)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_points_3d_kernel<MASK, float>), grid, dim3(64), 0, s, (const float*)kp2d, proj,
                         valid, mask, weights, kp3d, joint_err, kp3d_out, joint_err_out, joint_support, joint_status, n_prob, V,
                         J, eps);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(refine_points_3d_kernel<MASK, int64_t>), grid, dim3(64), 0, s, (const int64_t*)kp2d,
                         proj, valid, mask, weights, kp3d, joint_err, kp3d_out, joint_err_out, joint_support, joint_status,
                         n_prob, V, J, eps);
  });
  MVAL_CHECK_LAUNCH("mval_refine_points_3d");
  // the frame's metric over the new joint errors; joint_inliers are RANSAC's, so inlier_count comes out as it was
  launch_frame_reduce(joint_err_out, joint_inliers, valid, mask, mask_kind, metric, inlier_count, B, V, J, s);
  MVAL_CHECK_LAUNCH("mval_refine_points_3d/reduce");
  return 0;
}

// ---- XE metric (utils/triangulation.py:236-257) ---------------------------------------
// one wave per (frame, view, joint) map; float64 like the reference's rendered target.
// MASKED: the maps of an absent view are neither read nor written, and xe_sum_kernel leaves them out of its serial sum --
// the sum the unmasked entry makes over the frame's present views alone.  MASK_VIEW_JOINT: the same per map, the mask
// [B,V,J] being laid out like the maps.
template <int MASK>
__global__ __launch_bounds__(256) void xe_kernel(const double* __restrict__ kp3d, const double* __restrict__ proj,
                                                 const float* __restrict__ hm, const uint8_t* __restrict__ view_valid,
                                                 double* __restrict__ per_map, int64_t n_maps, int V, int J, int hh,
                                                 int wh, double sigma) {
  const int lane = threadIdx.x & 63;
  const int64_t map = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (map >= n_maps) return;
  const int j = (int)(map % J);
  const int v = (int)((map / J) % V);
  const int64_t b = map / ((int64_t)V * J);
  if (MASK == MASK_VIEWS && !view_valid[b * V + v]) return;
  if (MASK == MASK_VIEW_JOINT && !view_valid[map]) return;
  const double* P = proj + (b * V + v) * 12;
  const double* X = kp3d + (b * J + j) * 3;
  double u = X[0] * P[0] + X[1] * P[1] + X[2] * P[2] + P[3];
  double vv = X[0] * P[4] + X[1] * P[5] + X[2] * P[6] + P[7];
  double w = X[0] * P[8] + X[1] * P[9] + X[2] * P[10] + P[11];
  if (w == 0.0) w = 1.0;
  const double kx = u / w, ky = vv / w;
  const double inv = 1.0 / (2.0 * sigma * sigma);
  const float* p = hm + map * (int64_t)hh * wh;
  double acc = 0.0;
  for (int i = lane; i < hh * wh; i += 64) {
    int y = i / wh, x = i - y * wh;
    double dx = (double)x - kx, dy = (double)y - ky;
    double t = exp(-(dx * dx + dy * dy) * inv);
    double d = (double)p[i] - t;
    acc = fma(d, d, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) per_map[map] = acc / (double)(hh * wh);
}

template <int MASK>
__global__ void xe_sum_kernel(const double* __restrict__ per_map, const uint8_t* __restrict__ view_valid,
                              double* __restrict__ out, int B, int V, int J) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;  // the reference accumulates view-major, joint-minor, left to right
  if (MASK == MASK_VIEWS) {
    for (int v = 0; v < V; v++)
      if (view_valid[(int64_t)b * V + v])
        for (int j = 0; j < J; j++) s += per_map[((int64_t)b * V + v) * J + j];
  } else if (MASK == MASK_VIEW_JOINT) {
    const int VJ = V * J;
    for (int i = 0; i < VJ; i++)
      if (view_valid[(int64_t)b * VJ + i]) s += per_map[(int64_t)b * VJ + i];
  } else {
    const int VJ = V * J;
    for (int i = 0; i < VJ; i++) s += per_map[(int64_t)b * VJ + i];
  }
  out[b] = s;
}

// The two XE entries: `name` is the one that was called.
static int reprojection_xe(const char* name, const double* kp3d, const double* proj, const float* heatmaps, const uint8_t* mask,
                           int mask_kind, double* out, double* ws, int B, int V, int J, int hh, int wh, double sigma,
                           void* stream) {
  MVAL_REQUIRE(B >= 0 && V > 0 && J > 0 && hh > 0 && wh > 0 && sigma > 0, "%s: bad dims", name);
  MVAL_REQUIRE_MASK(name, mask, mask_kind);
  if (B == 0) return 0;
  const int64_t n_maps = (int64_t)B * V * J;
  return with_mask_kind(mask_kind, [&](auto K) {
    constexpr int MASK = decltype(K)::value;
    hipLaunchKernelGGL(xe_kernel<MASK>, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, mval_stream(stream), kp3d, proj,
                       heatmaps, mask, ws, n_maps, V, J, hh, wh, sigma);
    MVAL_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(xe_sum_kernel<MASK>, dim3((B + 63) / 64), dim3(64), 0, mval_stream(stream), ws, mask, out, B, V, J);
    MVAL_CHECK_LAUNCH_STAGE(name, "/sum");
    return 0;
  });
}

extern "C" int mval_reprojection_xe(const double* kp3d, const double* proj, const float* heatmaps, double* out,
                                    double* ws, int B, int V, int J, int hh, int wh, double sigma, void* stream) {
  return reprojection_xe("mval_reprojection_xe", kp3d, proj, heatmaps, nullptr, MASK_NONE, out, ws, B, V, J, hh, wh, sigma, stream);
}

extern "C" int mval_reprojection_xe_masked(const double* kp3d, const double* proj, const float* heatmaps, const uint8_t* mask,
                                           int mask_kind, double* out, double* ws, int B, int V, int J, int hh, int wh,
                                           double sigma, void* stream) {
  return reprojection_xe("mval_reprojection_xe_masked", kp3d, proj, heatmaps, mask, mask_kind, out, ws, B, V, J, hh, wh, sigma,
                         stream);
}

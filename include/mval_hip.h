/*
 * mval_hip.h -- C ABI of libmval_hip.so: the MI355X (gfx950) implementation of the
 * data-parallel hot path of facebookresearch/multi_view_active_learning.
 *
 * The reference has NO native layer: its boundary is a Python call surface.
 * Each entry point below therefore cites the reference *Python call site* it replaces
 * (paths relative to the reference root), and multi_view_active_learning_amd/_lib.py is the
 * ctypes binding a maintainer would use (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer borrowed from the
 *     caller (who keeps it alive until the stream has drained); nothing is allocated
 *     inside a launcher except via caller-provided workspaces;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it and
 *     graph-capturable (no synchronisation, no allocation inside);
 *   - return 0 on success, negative on error; mval_last_error() gives the message of the
 *     last failing call on the calling thread;
 *   - tensors are dense row-major with the shapes given in brackets.
 */
#ifndef MVAL_HIP_H
#define MVAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int mval_version(void);
const char* mval_last_error(void);

/* ------------------------------------------------------------------------------------
 * Keypoint decode
 * ---------------------------------------------------------------------------------- */

/* utils/evaluation.py:13-30 get_scaled_pred_corrdinates -- hard arg-max per (frame, view,
 * joint) map, first index on ties (NaN counts as maximum, like torch.argmax), then
 *   x = (idx % split_width) * stride ; y = (idx / split_width) * stride.
 * The reference passes shape[2] (= hh) as split_width for BOTH (its non-square quirk,
 * SURVEY A.2); pass wh for the geometrically correct split.  Invalid joints -> (0, 0).
 *   heatmaps [B,V,J,hh,wh] f32 ; valid [B,J] u8 or NULL ; kp2d [B,V,J,2] i64 (x,y). */
int mval_argmax_decode(const float* heatmaps, const uint8_t* valid, int64_t* kp2d,
                       int B, int V, int J, int hh, int wh, int stride, int split_width, void* stream);
/* The same key-points from the arg-max keys of mval_net_forward_keys (no read of the heat-maps):
 *   keys [B*V][MVAL_ARGMAX_SLOTS][J] u64 ; valid [B,J] u8 or NULL ; kp2d [B,V,J,2] i64 (x,y). */
int mval_argmax_from_keys(const uint64_t* keys, const uint8_t* valid, int64_t* kp2d, int B, int V, int J,
                          int stride, int split_width, void* stream);

/* utils/evaluation.py:45-58 get_pred_coordinates, hard arg-max branch (called from strategy.py:784-789) -- the same
 * arg-max (first index on ties, NaN counts as maximum), scaled by the image's box (left, top, right, bottom):
 *   x = f32(idx % hh) * ((box[3] - box[1]) / f32(wh)) ; y = f32(idx / hh) * ((box[2] - box[0]) / f32(hh))
 * in float32, the subtraction, the division and the multiply each rounded on its own, so the result equals torch's bit
 * for bit.  Both are the reference's: the split by shape[2] (= hh) for x and y, and the swapped box extents (x scaled by
 * the vertical extent, y by the horizontal one).
 *   heatmaps [N,J,hh,wh] f32 ; boxes [N,4] f32 ; xy [N,J,2] f32 (x,y) ; hh * wh < 2^24. */
int mval_pred_coordinates(const float* heatmaps, const float* boxes, float* xy, int64_t N, int J, int hh, int wh, void* stream);
/* The same from the arg-max keys of mval_net_forward_keys (no read of the heat-maps):
 *   keys [N][MVAL_ARGMAX_SLOTS][J] u64, as mval_argmax_from_keys reads them. */
int mval_pred_coordinates_from_keys(const uint64_t* keys, const float* boxes, float* xy, int64_t N, int J, int hh, int wh,
                                    void* stream);

/* utils/triangulation.py:191-200 (kornia.spatial_soft_argmax2d(hm, normalized_coordinates=False)
 * * stride): softmax over hh*wh, expectation of the pixel grid; kp2d [n_maps,2] f32 (x,y)*scale. */
int mval_soft_argmax(const float* heatmaps, float* kp2d, int64_t n_maps, int hh, int wh, float scale, void* stream);

/* Sub-pixel refinement of the hard arg-max (not in the reference; DESIGN.md 6.4 holds the definition).  The peak of a map is
 * (px, py) = kp2d / stride; with the peak interior (1 <= px <= wh-2, 1 <= py <= hh-2) and its 3x3 neighbourhood n finite, in
 * float64:
 *   MVAL_REFINE_QUARTER: ox = 0.25 sgn(n[1][2] - n[1][0]), oy = 0.25 sgn(n[2][1] - n[0][1])   (HRNet's evaluation shift)
 *   MVAL_REFINE_TAYLOR:  with L = log(max(n, 1e-10)), g and H the central first and second differences of L at the peak,
 *                        (ox, oy) = -H^-1 g, taken iff n[1][1] > 0, dxx < 0, det H > 0, |ox| <= 1 and |oy| <= 1
 *                        (DARK's Taylor step without its Gaussian pre-blur)
 * and (0, 0) otherwise.  out = f32((px + ox) * stride), f32((py + oy) * stride), rounded once; conf = the map's value at the
 * peak.  No FMA contraction: a float64 evaluation on the host takes the same sgn and accept decisions.
 *   heatmaps [B,V,J,hh,wh] f32 ; kp2d [B,V,J,2] i64, the hard decode (px*stride, py*stride) as mval_argmax_decode,
 *   mval_argmax_from_keys and the scoring kernels write it WITH split_width = wh ; valid [B,J] u8 or NULL (invalid joints ->
 *   (0, 0), conf 0) ; out [B,V,J,2] f32 (x,y) ; conf [B,V,J] f32 or NULL.
 * One thread per map, nine loads, no second read of the maps.  A kp2d entry that is no point of its map (negative, px >= wh or
 * py >= hh: a decode split by hh on a non-square map can give one) is checked BEFORE any load and handed through as
 * (f32(kp2d.x), f32(kp2d.y)) with conf NaN.  method outside {1, 2}, stride <= 0 or bad dimensions return an error and launch
 * nothing; B = 0 returns 0. */
#define MVAL_REFINE_QUARTER 1
#define MVAL_REFINE_TAYLOR 2
int mval_refine_keypoints(int method, const float* heatmaps, const int64_t* kp2d, const uint8_t* valid,
                          float* out, float* conf, int B, int V, int J, int hh, int wh, int stride, void* stream);

/* Peak gate: out[m] = 1 iff some element of map m is >= min_peak, else 0 (a comparison: a map of NaNs gives 0; exact, no
 * tolerance).  heatmaps [n_maps,hh,wh] f32 ; out [n_maps] u8.  One read of the maps.  With n_maps = B*V*J in the maps' own
 * order the result is a view_joint_valid [B,V,J] for the `_masked` entries below (MVAL_MASK_VIEW_JOINT). */
int mval_peak_mask(const float* heatmaps, float min_peak, uint8_t* out, int64_t n_maps, int hh, int wh, void* stream);

/* ------------------------------------------------------------------------------------
 * Flip test (not in the reference; HRNet's and Simple Baselines' TEST.FLIP_TEST / TEST.SHIFT_HEATMAP)
 * ---------------------------------------------------------------------------------- */

/* out[r][x] = in[r][W - 1 - x] for n_rows rows of W floats (an NCHW batch is N * 3 * H rows): a bit copy.  out must not
 * overlap in.  n_rows = 0 returns 0. */
int mval_mirror_images(const float* in, float* out, int64_t n_rows, int W, void* stream);
/* The merge of a forward on the images (hm) with a forward on the mirrored images (hm_mirrored), both [N][J][hh][wh] f32:
 * HRNet's flip_back, then its SHIFT_HEATMAP, then the average.  With p = pairs[j], the channel of joint j's mirror twin
 * (pairs [J] i32 on the DEVICE, pairs[j] == j for a centre joint; an entry outside [0, J) is read as j),
 *   merged[n][j][y][x] = (hm[n][j][y][x] + f) * 0.5f ,  f = hm_mirrored[n][p][y][wh - 1 - x]               (shift == 0)
 *                                                        f = hm_mirrored[n][p][y][min(wh - x, wh - 1)]      (shift != 0:
 * the flipped-back map moved one column to the right, column 0 keeping its own value) -- in float32, one add and then one
 * multiply, each rounded on its own, so a host float32 evaluation in that order gives the same bits.
 * argmax_keys: NULL, or [N][MVAL_ARGMAX_SLOTS][J] u64 that receives the keys of `merged` as mval_net_forward_keys documents
 * them (every slot of every map is written here, the unused ones with 0: no clear needed beforehand), so
 * mval_argmax_from_keys on them equals mval_argmax_decode on `merged`.
 * merged must overlap neither input (the inputs may be one tensor).  N = 0 returns 0 before any pointer check; J >= 1 and
 * hh * wh < 2^24.  One launch, two reads and one write per element. */
int mval_flip_merge_heatmaps(const float* hm, const float* hm_mirrored, const int32_t* pairs, int shift, float* merged,
                             uint64_t* argmax_keys, int64_t N, int J, int hh, int wh, void* stream);

/* ------------------------------------------------------------------------------------
 * Triangulation
 * ---------------------------------------------------------------------------------- */

/* utils/triangulation.py:209-233 + :260-338 _triangulate_ransac + :341-368 _triangulate_dlt +
 * :371-384 _calc_reprojection_error_matrix, batched over (frame, joint), float64, SVD-free
 * (Givens QR of the 2n x 4 DLT system, then one-sided Jacobi on the 4x4 R factor).
 * Deterministic pair order (V <= 11), first strictly larger inlier set wins, the sampled
 * pair is always an inlier, final solve on the sorted inlier views.
 *   kp2d [B,V,J,2] i64 (kp_is_f32 = 0) or f32 (kp_is_f32 = 1) ; proj [B,V,3,4] f64 ;
 *   valid [B,J] u8 or NULL ;
 *   kp3d [B,J,3] f64 (0 for invalid joints) ; joint_err [B,J] f64 mean inlier reprojection
 *   error ; joint_inliers [B,J] i32 ; metric [B] f64 = numpy-order mean of joint_err over
 *   valid joints (NaN if none) ; inlier_count [B] i32 = min over valid joints (-1 if none:
 *   the reference raises ValueError there, the host wrapper does the same). */
int mval_triangulate_ransac(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                            double* kp3d, double* joint_err, int32_t* joint_inliers, double* metric,
                            int32_t* inlier_count, int B, int V, int J, double eps, void* stream);

/* The same for rigs of up to 32 views, over an explicit table of view pairs walked IN TABLE ORDER: the winner is the
 * first table position with the strictly largest inlier set (utils/triangulation.py:299-300).  When C(V,2) exceeds
 * n_iters the reference shuffles the pair list with python's `random` and keeps the first n_iters (:279-282, from
 * V = 12 on at the default 64); the host draws those pairs in the reference's order
 * (utils.triangulation.draw_view_pairs) and the device does the arithmetic.
 *   pairs [B*J,P,2] u8 (pairs_shared = 0: one table per problem; the rows of an invalid joint are not read) or
 *   [1,P,2] u8 (pairs_shared = 1: one table for every problem, e.g. all C(V,2) pairs in lexicographic order, which
 *   gives mval_triangulate_ransac's results bit for bit) ; 1 <= P <= 496 = C(32,2) ; each entry a view index < V
 *   (a pair naming a view >= V takes no part in the vote; with no usable pair all views are inliers, :303-304).
 *   2 <= V <= 32 (the inlier mask is 32 bits wide): outside it returns an error and launches nothing.
 *   Every other argument and output as mval_triangulate_ransac. */
#define MVAL_PAIRS_MAX_VIEWS 32
#define MVAL_PAIRS_MAX_PAIRS 496
int mval_triangulate_ransac_pairs(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                  const uint8_t* pairs, int P, int pairs_shared, double* kp3d, double* joint_err,
                                  int32_t* joint_inliers, double* metric, int32_t* inlier_count, int B, int V, int J,
                                  double eps, void* stream);

/* utils/triangulation.py:236-257 _compute_xe: sum over (view, joint) of
 * mean_px (hm - exp(-|grid - kp|^2 / (2 sigma^2)))^2 with kp the reprojection of kp3d
 * (input-pixel units on the heat-map grid, as the reference does).  out [B] f64 ;
 * ws [B*V*J] f64 scratch. */
int mval_reprojection_xe(const double* kp3d, const double* proj, const float* heatmaps, double* out, double* ws,
                         int B, int V, int J, int hh, int wh, double sigma, void* stream);

/* Presence masks.  The four `_masked` entries below -- and mval_refine_points_3d and mval_undistort_keypoints -- take
 * `const uint8_t* mask, int mask_kind` and compute what their unmasked sibling computes on the views that are present.  mask_kind must be one of the three values
 * and (mask_kind == MVAL_MASK_NONE) == (mask == NULL); anything else is an error and nothing is launched.
 *
 * MVAL_MASK_NONE: no mask.  The entry runs what its unmasked sibling runs (which forwards here), bit for bit.
 *
 * MVAL_MASK_VIEWS: mask = view_valid [B,V] u8, nonzero = the view is present in that frame.  For every frame the result is
 *   what the unmasked entry gives on that frame's present views alone, bit for bit.  All frames of a batch go through one
 *   launch, however their present sets differ.  Per frame with n present views: n < 2 and at least one valid joint ->
 *   inlier_count -2, metric NaN, kp3d / joint_err / joint_inliers 0 (the reference asserts len(points) >= 2 inside the first
 *   valid joint; the host wrapper raises AssertionError); no valid joint -> inlier_count -1 and metric NaN whatever n is.
 *   joint_inliers counts present views only.
 *
 * MVAL_MASK_VIEW_JOINT: mask = view_joint_valid [B,V,J] u8, nonzero = joint j is usable in view v of frame b.  The present
 *   views are a property of the PROBLEM (frame, joint): for a valid joint with two or more present views the result is what
 *   the unmasked entry gives on that joint's present views alone (B = 1, J = 1), bit for bit.  All problems of a batch go
 *   through one launch however their sets differ.  A valid joint with fewer than two present views is written like an invalid
 *   joint: kp3d, joint_err, joint_inliers 0.  metric (mean) and inlier_count (min) of a frame run over its USED joints: valid
 *   and two or more present views.  A used joint has joint_inliers >= 2 (the winning pair is in its own set), so
 *   joint_inliers > 0 is the used mask.  No valid joint -> inlier_count -1; a valid joint but no used joint -> -2; metric NaN
 *   in both.
 *
 * Nothing of an absent view / entry is read: it never votes, is never an inlier or part of a walked pair, is skipped by the
 * final DLT, and its key-point row, projection matrix (MVAL_MASK_VIEWS) and heat-maps may hold anything, NaN included. */
#define MVAL_MASK_NONE 0
#define MVAL_MASK_VIEWS 1
#define MVAL_MASK_VIEW_JOINT 2

/* mval_triangulate_ransac under a mask (2 <= V <= 11): lane p keeps its lexicographic pair and sits out when one of its views
 * is absent; the vote runs over present views.  Every other argument and output as mval_triangulate_ransac. */
int mval_triangulate_ransac_masked(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                   const uint8_t* mask, int mask_kind, double* kp3d, double* joint_err,
                                   int32_t* joint_inliers, double* metric, int32_t* inlier_count, int B, int V, int J,
                                   double eps, void* stream);

/* mval_triangulate_ransac_pairs under a mask (2 <= V <= 32): the table names ORIGINAL view indices; an entry naming an absent
 * view, or a view >= V (the host pads the shorter rows of a per-problem table with 255), takes no part; with no usable pair
 * all PRESENT views are inliers.  Every other argument and output as mval_triangulate_ransac_pairs. */
int mval_triangulate_ransac_pairs_masked(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                         const uint8_t* mask, int mask_kind, const uint8_t* pairs, int P, int pairs_shared,
                                         double* kp3d, double* joint_err, int32_t* joint_inliers, double* metric,
                                         int32_t* inlier_count, int B, int V, int J, double eps, void* stream);

/* Confidence-weighted triangulation and RANSAC's winning inlier set (not in the reference; DESIGN.md 6.7 holds the definition).
 * One entry for both kernels: pairs == NULL walks all C(V,2) pairs as mval_triangulate_ransac_masked does (2 <= V <= 11),
 * otherwise the table as mval_triangulate_ransac_pairs_masked does (2 <= V <= 32; P, pairs_shared as there).
 *   joint_inlier_mask [B,J] i32 or NULL: bit v is set when view v is in the winning set the final DLT ran over; 0 for a joint
 *       that is invalid or not used.  Its population count is joint_inliers.
 *   weights [B,V,J] f32 or NULL.
 * weights == NULL: every other output is bit for bit what the `_masked` entry of the same mask_kind and table writes.
 * weights != NULL: an entry (b, v, j) is USABLE when its weight is finite and > 0, and its effective presence is "present under
 *   (mask, mask_kind)" AND usable.  The call then has the semantics of MVAL_MASK_VIEW_JOINT with that effective mask, whichever
 *   mask_kind came in: an unusable entry never votes, is never an inlier or part of a walked pair; "no usable pair: all views"
 *   means all effectively present views; a valid joint with fewer than two of them is written like an invalid one; metric and
 *   inlier_count run over the used joints (a valid joint but no used one: -2 and NaN; no valid joint: -1), which under
 *   MVAL_MASK_VIEWS gives a frame with fewer than two present views its -2 / -1 as ever.  Nothing of an entry the mask calls
 *   absent is read, its weight included.
 *   Both DLT rows of view v -- in the pair solve of every hypothesis and in the final solve -- are multiplied by (double)w_v,
 *   every element formed as without weights and then multiplied once: a weight of exactly 1.0f gives the unweighted bits.
 *   The vote (error < eps) is unweighted, and joint_err stays the unweighted mean error of the inlier views, in pixels.
 *   Ranking of hypotheses: more inliers; among equal counts the larger S = sum of w_v over the set (views ascending, float64);
 *   among equal S the lower pair position.  With all weights equal this is the unweighted ranking.
 * A problem's bits do not depend on its place in the batch.  Arguments are checked as the `_masked` entries check theirs; weights
 * and joint_inlier_mask must be 4-byte aligned. */
int mval_triangulate_ransac_weighted(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid,
                                     const uint8_t* mask, int mask_kind, const uint8_t* pairs, int P, int pairs_shared,
                                     const float* weights, double* kp3d, double* joint_err, int32_t* joint_inliers,
                                     int32_t* joint_inlier_mask, double* metric, int32_t* inlier_count, int B, int V, int J,
                                     double eps, void* stream);

/* mval_reprojection_xe under a mask: the maps of an absent view / entry are not read, their ws slots are not written, and the
 * serial view-major, joint-minor sum skips them.  A frame without a present view / entry gives 0. */
int mval_reprojection_xe_masked(const double* kp3d, const double* proj, const float* heatmaps, const uint8_t* mask,
                                int mask_kind, double* out, double* ws, int B, int V, int J, int hh, int wh, double sigma,
                                void* stream);

/* 3-D refinement of the triangulated joints (not in the reference, whose direct_optimization has no defined result;
 * DESIGN.md 6.5 holds the definition).  One extra launch between a triangulation entry and the metrics.  Per problem (frame,
 * joint), with X0 = kp3d the triangulation's point:
 *   S = the present views v whose half-distance error at X0, 1/2 |p_v - pi(P_v [X0; 1])| -- the vote's own -- is finite and
 *       < eps, and, with weights, whose w_v is finite and > 0.  Presence is read as the triangulation entries read it: valid
 *       [B,J] u8 or NULL, and (mask, mask_kind) as under "Presence masks" above; nothing of an absent view or entry is read.
 *   Not refined -- kp3d_out = X0 bit for bit, joint_err_out = joint_err, joint_status 0 -- when the joint is invalid, X0 is
 *       non-finite or |S| < 2.
 *   Otherwise kp3d_out = the minimiser of E(X) = 1/2 sum_{v in S} w_v |p_v - pi(P_v [X; 1])|^2 (w_v = 1 without weights) by
 *       Levenberg-Marquardt in float64, views ascending: lam = 1e-3; an iteration solves (A + lam diag A) d = g and tries
 *       X + d, accepted iff E does not rise and every view of S has depth > 0 there; accepted: lam = max(lam / 10, 1e-9),
 *       and converged when |d| <= 1e-8 (1 + |X|); rejected: lam *= 10, and converged when lam > 1e12 (no damping lowers the
 *       cost).  joint_status = k > 0: converged in iteration k; -MVAL_REFINE3D_MAX_ITERS: the cap was reached, the point
 *       found so far is kept.  joint_err_out = the mean over S of the half-distance error at kp3d_out.
 *   joint_support [B,J] i32 = |S| (0 for an invalid joint).
 *   metric [B] f64, inlier_count [B] i32: the frame reduction of the triangulation entries over joint_err_out and the
 *       unchanged joint_inliers [B,J] i32 -- inlier_count comes out as the triangulation wrote it.
 *   kp2d [B,V,J,2] i64 | f32 (kp_is_f32) ; proj [B,V,3,4] f64 ; weights [B,V,J] f32 or NULL ; kp3d, kp3d_out [B,J,3] f64 ;
 *   joint_err, joint_err_out [B,J] f64.  The outputs must not alias the inputs.
 *   The accept test is decided by the last bit of E once two points are closer than about 1e-6 mm, so the solver's arithmetic
 *   is part of the definition: per view h_i = P_i0 X0 + P_i1 X1 + P_i2 X2 + P_i3 (left to right), u = h0 / h2, v = h1 / h2,
 *   r = (px - u, py - v), jx_k = (P_0k - u P_2k) / h2, jy_k = (P_1k - v P_2k) / h2; a_kl += w (jx_k jx_l + jy_k jy_l),
 *   g_k += w (jx_k rx + jy_k ry), E += w (rx rx + ry ry), E halved at the end; LDL^T without pivoting; one IEEE float64
 *   operation each, no FMA contraction (csrc/triangulate.hip: refine_normal, refine_solve).
 * One lane per problem; a problem's bits do not depend on the rest of the batch.  V outside 2..32, a mask_kind outside 0..2
 * or not matching `mask`, NULL or misaligned arrays return an error and launch nothing; B = 0 returns 0. */
#define MVAL_REFINE3D_MAX_ITERS 32
int mval_refine_points_3d(const void* kp2d, int kp_is_f32, const double* proj, const uint8_t* valid, const uint8_t* mask,
                          int mask_kind, const float* weights, const double* kp3d, const double* joint_err,
                          const int32_t* joint_inliers, double* kp3d_out, double* joint_err_out, int32_t* joint_support,
                          int32_t* joint_status, double* metric, int32_t* inlier_count, int B, int V, int J, double eps,
                          void* stream);

/* Undistortion of the decoded key-points (not in the reference, whose post stage takes the distorted peaks for pinhole
 * observations; DESIGN.md 6.6 holds the definition).  One launch between the decode (with its refinement) and a triangulation
 * entry: the inverse of the reference's forward model (utils/triangulation.py:433-456), per entry (frame, view, joint) in float64
 *   d(x, y) = (xd, yd):  xd = x q + 2 p1 x y + p2 (r + 2 x^2),  yd = y q + 2 p2 xd y + p1 (r + 2 y^2),
 *             r = x^2 + y^2,  q = 1 + k1 r + k2 r^2 + k3 r^3
 *     (yd's cross term holds xd, not x: the reference overwrites x with its distorted value before it forms y, :444-453, and the
 *      training targets sit where THAT model puts them; for p2 = 0 it is the Brown-Conrady polynomial of cv2.projectPoints),
 *   pixel = K2 d(x, y) + c  with K2 = [K00 K01; K10 K11], c = (K02, K12): the six numbers of K the forward model reads.
 *   kp2d [B,V,J,2] i64 | f32 (kp_is_f32), pixels (x, y) ; K [B,V,3,3] f64, the view's intrinsics after crop and resize ;
 *   dist [B,V,5] f64 = k1, k2, p1, p2, k3 ; valid [B,J] u8 or NULL ; (mask, mask_kind) as under "Presence masks" above ;
 *   out [B,V,J,2] f32 (x,y) ; status [B,V,J] i32.
 * Not processed -- out (0, 0), status 0: an invalid joint, an absent view or entry.  Nothing of an absent entry is read, and
 *   under MVAL_MASK_VIEWS the K and dist of an absent view may hold anything, NaN included.
 * Handed through -- out = f32(kp2d) bit for bit:
 *   status 0: all five coefficients are exactly 0 (K is not read);
 *   status MVAL_UNDISTORT_FOLD: det J was not > 0, or not finite, at some iterate -- beyond the fold-over of a strong barrel
 *     lens, a NaN or inf input, a singular K2;
 *   status MVAL_UNDISTORT_NOCONV: MVAL_UNDISTORT_MAX_ITERS iterations did not converge.
 * Otherwise status = k >= 1, the Newton iteration that converged, and out = f32(K00 x + K01 y + K02), f32(K10 x + K11 y + K12),
 *   rounded once.  A handed-through entry still takes part in the triangulation, at its distorted position, as every entry does
 *   without this stage; status is how a caller finds it.
 * The arithmetic is part of the definition (the fold and convergence decisions of a host float64 evaluation are then the
 * device's): a = px - K02, b = py - K12, D = K00 K11 - K01 K10, (tx, ty) = ((K11 a - K01 b) / D, (K00 b - K10 a) / D);
 * (x, y) = (tx, ty); iteration k = 1 .. MVAL_UNDISTORT_MAX_ITERS: xx = x x, yy = y y, xy = x y, r = xx + yy, r2 = r r, r3 = r2 r,
 *   q = 1 + k1 r + k2 r2 + k3 r3,  s = k1 + 2 k2 r + 3 k3 r2,
 *   xd = x q + 2 p1 xy + p2 (r + 2 xx),  yd = y q + 2 p2 xd y + p1 (r + 2 yy),  fx = xd - tx,  fy = yd - ty,
 *   jxx = q + 2 xx s + 2 p1 y + 6 p2 x,  jxy = 2 xy s + 2 p1 x + 2 p2 y,                      (d xd / dx, d xd / dy)
 *   jyx = 2 xy s + 2 p1 x + 2 p2 y jxx,  jyy = q + 2 yy s + 6 p1 y + 2 p2 (xd + y jxy),       (d yd / dx, d yd / dy)
 *   det J = jxx jyy - jxy jyx, tested BEFORE the step;  dx = (jyy fx - jxy fy) / det J,  dy = (jxx fy - jyx fx) / det J,
 *   x -= dx, y -= dy;  converged iff max(|dx|, |dy|) <= 1e-13 (1 + max(|x|, |y|)) at the new (x, y).
 * Sums and products left to right as written (2 p1 xy = (2 p1) xy), one IEEE float64 operation each, no FMA contraction
 * (csrc/undistort.hip).
 * One thread per entry; an entry's bits do not depend on the rest of the batch.  V outside 1..32, a mask_kind outside 0..2 or
 * not matching `mask`, NULL or misaligned arrays return an error and launch nothing; B = 0 returns 0.  The launch runs on
 * `stream` and adds no host synchronisation. */
#define MVAL_UNDISTORT_MAX_ITERS 16
#define MVAL_UNDISTORT_FOLD (-1)
#define MVAL_UNDISTORT_NOCONV (-2)
int mval_undistort_keypoints(const void* kp2d, int kp_is_f32, const double* K, const double* dist, const uint8_t* valid,
                             const uint8_t* mask, int mask_kind, float* out, int32_t* status, int B, int V, int J, void* stream);

/* ------------------------------------------------------------------------------------
 * Uncertainty scorers (strategy.py:1149-1215)
 * ---------------------------------------------------------------------------------- */
enum { MVAL_SCORE_HP = 0, MVAL_SCORE_MPE = 1, MVAL_SCORE_BSB = 2 };
enum { MVAL_REDUCE_AVG_F64 = 0, MVAL_REDUCE_AVG_F32 = 1, MVAL_REDUCE_STD_F64 = 2, MVAL_REDUCE_STD_F32 = 3 };

/* Per-map statistic, one heat-map read:
 *   HP  (strategy.py:1185-1187)  1 - max(row_softmax(map))           (row-wise softmax: SURVEY A.9)
 *   MPE (strategy.py:1168-1175)  entropy of softmax over the local peaks
 *        (skimage.feature.peak_local_max(map, min_distance=2): 5x5 maxima strictly above
 *        map.min(), 2-px border excluded, sorted by descending value -- equal values in row-major
 *        order, where the library's order is numpy's unstable argsort --, plateau spacing; equal to
 *        scikit-image 0.18.3 on every map without tied candidates: tests/golden/peaks_skimage.npz)
 *   BSB (strategy.py:1202-1208)  |p0 - p1| of the two highest local peaks of row_softmax(map)
 *   heatmaps [n_maps,hh,wh] f32 ; stat [n_maps] f32 ; n_peaks [n_maps] i32 (MPE/BSB: peaks after the spacing pass, any number
 *   of candidates -- maps with more than 2048 are redone by a second pass; 0 for HP).  BSB with fewer than two peaks: NaN
 *   (the reference raises IndexError). */
int mval_score_maps(int kind, const float* heatmaps, float* stat, int32_t* n_peaks,
                    int64_t n_maps, int hh, int wh, void* stream);

/* The same statistic AND the hard arg-max key-point of every map (utils/evaluation.py:13-30, as mval_argmax_decode)
 * from ONE staged read of each heat-map: what a scoring pass of strategy.py:1027-1090 needs per map.
 *   heatmaps [B,V,J,hh,wh] f32 ; valid [B,J] u8 or NULL (invalid joints -> key-point (0, 0); their statistic is
 *   still written, mval_score_reduce skips it) ; stat, n_peaks [B*V*J] ; kp2d [B,V,J,2] i64 (x, y). */
int mval_score_decode_maps(int kind, const float* heatmaps, const uint8_t* valid, float* stat, int32_t* n_peaks,
                           int64_t* kp2d, int B, int V, int J, int hh, int wh, int stride, int split_width, void* stream);

/* ALL THREE statistics AND (kp2d non-NULL) the hard arg-max key-point of every map from one staged read of each heat-map:
 * what comparing the strategies on one pool needs per map.  Every output equals, bit for bit, what the single-kind entries
 * above write (each statistic runs the same float operations in the same order); a map whose candidate list overflows
 * for one statistic has that statistic alone redone by the second pass.
 *   heatmaps [B,V,J,hh,wh] f32 ; valid [B,J] u8 or NULL (only read for kp2d) ;
 *   stat [3][B*V*J] f32: MVAL_SCORE_HP, _MPE, _BSB in that order ; n_peaks [2][B*V*J] i32: MPE, BSB (as mval_score_maps
 *   writes them) ; kp2d [B,V,J,2] i64 (x, y) or NULL = no decode (stride and split_width are ignored then). */
int mval_score_decode_maps_all(const float* heatmaps, const uint8_t* valid, float* stat, int32_t* n_peaks, int64_t* kp2d,
                               int B, int V, int J, int hh, int wh, int stride, int split_width, void* stream);

/* AVG / STD over the valid (view, joint) maps of each frame in the reference's python /
 * numpy evaluation order and precision (strategy.py:1151-1155,1188-1193,1210-1215;
 * SURVEY A.8).  per_map [B,V,J] f32 ; valid [B,J] u8 or NULL ; out [B] f64. */
int mval_score_reduce(const float* per_map, const uint8_t* valid, double* out, int B, int V, int J,
                      int mode, void* stream);

/* mval_score_reduce under a mask ("Presence masks" above): the statistics of absent maps are not read; same loop order
 * (views outer, joints inner) and precision per mode.  MVAL_MASK_VIEWS: n = valid joints x present views, and a frame gives
 * what mval_score_reduce gives on its present views alone.  MVAL_MASK_VIEW_JOINT: a map counts when its joint is valid and
 * its own entry is nonzero, n = the entries left, and a frame gives what mval_score_reduce gives on the compacted list
 * (V = 1, J = n).  n = 0 -> NaN. */
int mval_score_reduce_masked(const float* per_map, const uint8_t* valid, const uint8_t* mask, int mask_kind, double* out,
                             int B, int V, int J, int mode, void* stream);

/* ------------------------------------------------------------------------------------
 * Loss / metric
 * ---------------------------------------------------------------------------------- */

/* pose_estimators/loss.py:14-20: out = sum(valid ? (h-g)^2 : 0) / denom.
 *   h,g [lead,hw] f32 ; valid [lead] u8 or NULL ; out [1] f32 ; ws >= 2048 doubles. */
int mval_masked_mse_fwd(const float* h, const float* g, const uint8_t* valid, float* out, double* ws,
                        int64_t lead, int64_t hw, double denom, void* stream);
/* d loss / d h = grad_out * 2 (h-g) valid / denom.  grad_out [1] f32 ; grad_h [lead,hw] f32. */
int mval_masked_mse_bwd(const float* h, const float* g, const uint8_t* valid, const float* grad_out,
                        float* grad_h, int64_t lead, int64_t hw, double denom, void* stream);
/* The same two against ground truth that is rendered per pixel instead of read (training from key-point targets):
 *   pt [lead][2] f64 (x, y in heat-map pixels) ; map m is what mval_gt_heatmaps(pt + 2 m, 1, sigma_m, hh, wh) writes, with
 *   sigma_m = sigma_per_map[m] where sigma_per_map (device, [lead] f64) is non-NULL, else sigma.  The sigma in use must be > 0: the
 *   scalar is checked here, the array by whoever uploads it (a launcher does not synchronise); 2 sigma^2 = 2.0 * (sigma * sigma) in
 *   separately rounded float64, as the host forms it for mval_gt_heatmaps.
 * Bit-identical to mval_masked_mse_fwd/_bwd on those maps: same grid, element -> thread map, float64 accumulation order and final
 * kernel; the float4 walk where hh * wh % 4 == 0 and h is 16-byte aligned, else the scalar walk.  A masked map is neither rendered nor
 * counted (its points may be NaN) and gets grad_h = +0.0f.  The backward renders the ground truth again; nothing is kept between the
 * two.  hh * wh <= INT32_MAX - 1024.  Other arguments, ws and lead == 0 as in the read form. */
int mval_masked_mse_points_fwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                               const uint8_t* valid, float* out, double* ws, int64_t lead, int hh, int wh, double denom,
                               void* stream);
int mval_masked_mse_points_bwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                               const uint8_t* valid, const float* grad_out, float* grad_h, int64_t lead, int hh, int wh,
                               double denom, void* stream);

/* Workspace bytes of one mval_frame_loss / mval_frame_loss_points call (0 for non-positive sizes). */
size_t mval_frame_loss_workspace_bytes(int64_t n_frames, int maps_per_frame);
/* pose_estimators/loss.py:22-24 for every frame of a batch (the CLUSTER pass, strategy.py:173-187):
 *   out[b] = (float)( sum over the maps m of frame b with valid[m] != 0, sum over pixels (h - g)^2 / (hh * wh) ).
 *   heatmaps, gt [n_frames][maps_per_frame][hh][wh] f32 ; valid [n_frames * maps_per_frame] u8 or NULL ; out [n_frames] f32 ;
 *   per_map: ws >= mval_frame_loss_workspace_bytes, holds every map's sum of squared errors afterwards (0 for a masked map).
 * h - g and its square are float32 (torch's (h - gt) ** 2), the sums float64 in a fixed order without atomics: a map's
 * pixels, then a frame's maps in ascending order, / (hh * wh), one rounding to float32.  A frame's result does not depend on
 * the batch it is in or on its place there.  Two launches. */
int mval_frame_loss(const float* heatmaps, const float* gt, const uint8_t* valid, float* out, double* per_map,
                    int64_t n_frames, int maps_per_frame, int hh, int wh, void* stream);
/* The same with the ground truth rendered per pixel instead of read: pt [n_frames * maps_per_frame][2] f64 (x, y in heat-map
 * pixels), the maps mval_gt_heatmaps(pt, sigma, hh, wh) writes -- bit-identical to mval_frame_loss on them. */
int mval_frame_loss_points(const float* heatmaps, const double* pt, double sigma, const uint8_t* valid, float* out,
                           double* per_map, int64_t n_frames, int maps_per_frame, int hh, int wh, void* stream);

/* Workspace bytes of one mval_weighted_mse_fwd / _points_fwd call (0 for non-positive sizes). */
size_t mval_weighted_mse_workspace_bytes(int64_t n_images, int n_joints);
/* The training loss with per-joint weights and online hard key-point mining (no counterpart in the reference; HRNet's
 * USE_TARGET_WEIGHT and JointsOHKMMSELoss).  lead = n_images * n_joints maps m = n * n_joints + j:
 *   S[m]    = sum over the map's pixels of (h - g)^2: float32 difference and square, float64 sum, in mval_frame_loss's pixel ->
 *             lane assignment and order (the same kernel), so S[m] has the bits of that entry's per_map[m]
 *   l[m]    = (double)weight[m] * S[m], one rounding                                            -> per_map [lead] f64
 *   per image its n_joints values l are ranked in torch.argmax's order (NaN first, ties to the lowest joint); the first topk are
 *   selected, all of them for topk == 0: wsel[m] = selected ? weight[m] : 0.0f                  -> wsel [lead] f32
 *   T[n]    = sum of the selected l[n][j], ascending j, sequential float64
 *   out[0]  = (float)( (sum of T[n], ascending n, sequential float64) / (n_images * hh * wh) )  -> out [1] f32
 * The divisor omits n_joints as mval_masked_mse_fwd's callers' does, and there is no division by topk: topk == n_joints is the
 * weighted loss and a smaller topk only removes terms (HRNet divides by topk and carries a factor 0.5).  The weight multiplies
 * the squared error: HRNet's target_weight t scales prediction and target, which is weight = t * t.
 *   h, g [n_images][n_joints][hh][wh] f32 ; weight [lead] f32, finite and >= 0 (the caller's duty: a launcher does not synchronise) ;
 *   0 <= topk <= n_joints ; ws >= mval_weighted_mse_workspace_bytes.
 * A map with weight == 0 is not read, S = +0.0: NaNs under a zero weight do not reach the loss.  A NaN l ranks first and makes
 * the loss NaN.  No atomics: T[n] does not depend on the other images.  n_images == 0: out = 0, nothing else is touched.
 * Three launches. */
int mval_weighted_mse_fwd(const float* h, const float* g, const float* weight, int topk, float* out, double* per_map,
                          float* wsel, void* ws, int64_t n_images, int n_joints, int hh, int wh, void* stream);
/* grad_h = ((2 (h - g)) * gs) * wsel[m] with gs = grad_out[0] / (float)(n_images * hh * wh), float32, every product rounded on
 * its own; a map with wsel == 0 is not read and gets +0.0f.  With weights in {0, 1} and topk == 0 the bits of mval_masked_mse_bwd
 * under that mask.  grad_out [1] f32 ; wsel [lead] f32 from the forward ; grad_h [lead][hh][wh] f32. */
int mval_weighted_mse_bwd(const float* h, const float* g, const float* wsel, const float* grad_out, float* grad_h,
                          int64_t n_images, int n_joints, int hh, int wh, void* stream);
/* The same two against ground truth rendered per pixel: pt, sigma and sigma_per_map as in mval_masked_mse_points_fwd (a scalar
 * sigma must be > 0, an array is its uploader's to check) -- bit-identical to the read form on the maps mval_gt_heatmaps writes.
 * A map that does not count is not rendered (its point may be NaN).  hh * wh <= INT32_MAX - 1024. */
int mval_weighted_mse_points_fwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                                 const float* weight, int topk, float* out, double* per_map, float* wsel, void* ws,
                                 int64_t n_images, int n_joints, int hh, int wh, void* stream);
int mval_weighted_mse_points_bwd(const float* h, const double* pt, double sigma, const double* sigma_per_map,
                                 const float* wsel, const float* grad_out, float* grad_h, int64_t n_images, int n_joints, int hh,
                                 int wh, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-view input pipeline (dataset/dataset.py:158-220 prepare_single_view, pixel work only)
 * ------------------------------------------------------------------------------------------- */
typedef struct mval_view_desc {
  const uint8_t* img;               /* decoded RGB image [h0][w0][3] (device) */
  int32_t h0, w0;
  int32_t left, top, right, bottom; /* square / scaled box (utils/triangulation.py:96-134); may leave the image */
  int64_t tmp_off;                  /* byte offset of this view's [bottom-top][in_w][3] slab in the workspace's temp part.  The slabs must not
                                     * overlap and must end inside the rows the workspace was sized for; usually they lie back to back from 0
                                     * (multiples of in_w * 3).  tmp_off need NOT be 4-byte aligned: the vertical pass reads 4 bytes at a time
                                     * where the slab is aligned and byte by byte where it is not, with the same result (tested with first
                                     * offsets 1, 2, 3: tests/test_gpu_preprocess_edges.py) */
} mval_view_desc;
/* ws >= mval_prepare_views_workspace_bytes(n_views, sum of the views' crop heights, in_w, in_h). */
size_t mval_prepare_views_workspace_bytes(int n_views, int64_t total_crop_rows, int in_w, int in_h);
/* BGR flip + zero-filled crop + PIL LANCZOS resize (Pillow's 8-bit fixed-point algorithm, bit-exact) +
 * ImageNet normalisation: out [n_views][3][in_h][in_w] f32.  views: DEVICE array.
 *   max_crop_h / max_crop_w must be at least every view's crop height (bottom - top) / crop width (right - left).  With a smaller value
 *   the results are undefined, though the kernels still write nothing outside out and ws.
 *   The largest accepted box: ceil(3 * max(1, max_crop_w / in_w, max_crop_h / in_h)) * 2 + 1 <= 64 filter taps, i.e. checked per axis and
 *   a crop / in ratio of at most 31 / 3 on either (661 -> 64, 2645 -> 256).  A larger box returns -1 and mval_last_error() names the box,
 *   the tap limit and the input size; nothing is launched. */
int mval_prepare_views(const mval_view_desc* views, int n_views, int max_crop_h, int max_crop_w, int in_w, int in_h,
                       float* out, void* ws, void* stream);
/* Gaussian ground-truth heat-maps (dataset.py:198-207): pt [n][2] f64 (x, y in heat-map pixels) ->
 * out [n][h][w] f32 = (float) exp(-((x - px)^2 + (y - py)^2) / (2 sigma^2)) evaluated in float64. */
int mval_gt_heatmaps(const double* pt, int64_t n, double sigma, int h, int w, float* out, void* stream);

/* The training split (dataset.py:212-213): resize to uint8, RandAugment (dataset/augmentation.py), then the normalisation.
 *
 * mval_resize_views_u8: mval_prepare_views up to the resized BYTES: out [n_views][in_h][in_w][3] u8 in the reference's channel order
 * (position 0 = blue: the image Pillow is handed).  Same views, limits and workspace (mval_prepare_views_workspace_bytes) as
 * mval_prepare_views; mval_normalize_views_u8 of its output gives mval_prepare_views' output bit for bit. */
int mval_resize_views_u8(const mval_view_desc* views, int n_views, int max_crop_h, int max_crop_w, int in_w, int in_h,
                         uint8_t* out, void* ws, void* stream);
/* normalize_image (utils/triangulation.py:137-145): img [n_views][h][w][3] u8 -> out [n_views][3][h][w] f32 = (float)((img / 255.0 - mean[ch]) /
 * std[ch]) evaluated in float64 per channel POSITION. */
int mval_normalize_views_u8(const uint8_t* img, int n_views, int h, int w, float* out, void* stream);

/* One op of a view's RandAugment list.  Every op is Pillow's (12.2.0), on channel positions, bit for bit:
 *   AUTOCONTRAST ImageOps.autocontrast    EQUALIZE ImageOps.equalize    INVERT ImageOps.invert
 *   POSTERIZE    ImageOps.posterize(max(1, int(p[0])))                  SOLARIZE ImageOps.solarize(threshold p[0])
 *   COLOR / CONTRAST / BRIGHTNESS / SHARPNESS   ImageEnhance.<op>(img).enhance(p[0])
 *   ROTATE       Image.rotate(angle, BICUBIC): p[0..5] = the affine coefficients Pillow builds on the host (output pixel centre -> input
 *                position: xin = p0 (x + 0.5) + p1 (y + 0.5) + p2, yin = p3 (x + 0.5) + p4 (y + 0.5) + p5); an angle that is 0 mod 360 is NONE
 *   NONE         the view is left as it is at this step */
enum { MVAL_AUG_NONE = 0, MVAL_AUG_AUTOCONTRAST = 1, MVAL_AUG_EQUALIZE = 2, MVAL_AUG_INVERT = 3, MVAL_AUG_POSTERIZE = 4, MVAL_AUG_SOLARIZE = 5,
       MVAL_AUG_COLOR = 6, MVAL_AUG_CONTRAST = 7, MVAL_AUG_BRIGHTNESS = 8, MVAL_AUG_SHARPNESS = 9, MVAL_AUG_ROTATE = 10 };
typedef struct mval_aug_op {
  int32_t kind;
  int32_t reserved;
  double p[6];
} mval_aug_op;
/* ws >= mval_augment_views_workspace_bytes(n_views, h, w) (0 for a non-positive argument). */
size_t mval_augment_views_workspace_bytes(int n_views, int h, int w);
/* In place on img [n_views][h][w][3] u8: view v runs ops[v][0], ops[v][1], ... ops[v][n_steps - 1] (ops: DEVICE array [n_views][n_steps]).
 * step_kinds: HOST array [n_steps]; bit MVAL_AUG_<kind> of entry k set iff some view runs that kind at step k -- it decides which passes are
 * launched (at most seven per step, whatever n_views is); a kind present on the device but missing there is skipped. */
int mval_augment_views(uint8_t* img, const mval_aug_op* ops, const uint32_t* step_kinds, int n_views, int n_steps, int h, int w,
                       void* ws, void* stream);
/* The target side of ROTATE (not in the reference as published: its Rotate drops the rotated maps, dataset/augmentation.py:19-25; this is what
 * the line evidently meant).  In place on maps [n_views][maps_per_view][h][w] f32: at step k, a view whose op is MVAL_AUG_ROTATE has every one of
 * its maps turned by Pillow's Image.rotate(angle, BICUBIC) on a mode-"F" image of h x w, bit for bit (ImagingGenericTransform with
 * bicubic_filter32F: float32 coefficient sums along a row, float64 polynomial, float64 between the rows, a float32 cast without a clip; a
 * position outside the map gives +0.0f); any other kind leaves the view's maps alone.  ops: the DEVICE array [n_views][n_steps] of
 * mval_augment_views, with p[0..5] built for the MAP's h, w; step_kinds: the HOST array [n_steps] -- a step without the MVAL_AUG_ROTATE bit
 * launches nothing.  ws >= mval_rotate_maps_workspace_bytes(...) (a second copy of maps; 0 for a non-positive argument).
 * Limits, checked: n_views <= 65535, maps_per_view <= 65535 (grid dimensions), h * w <= 2^28.  A null pointer, a non-positive size or a size
 * past these returns -1 with a message and launches nothing. */
size_t mval_rotate_maps_workspace_bytes(int n_views, int maps_per_view, int h, int w);
int mval_rotate_maps(float* maps, const mval_aug_op* ops, const uint32_t* step_kinds, int n_views, int n_steps, int maps_per_view, int h, int w,
                     void* ws, void* stream);

/* utils/evaluation.py:198-208 compute_mkpe over S samples: pred [S,J,3] f32, gt [S,gt_rows,J]
 * f32 (rows 0..2 used), valid [S,J] f32 ; out [1] f32 = mean_j (sum_s d_sj / sum_s valid_sj) ;
 * per_sample [S] f32 = the same metric evaluated on each sample alone (strategy.py:1134). */
int mval_mkpe(const float* pred, const float* gt, const float* valid, float* out, float* per_sample,
              int64_t S, int J, int gt_rows, void* stream);
/* 3-D PCK / PCKh counters (utils/evaluation.py:150-195 compute_3d_pckh / compute_3d_pck, called from
 * strategy.py:638-649).  pred [S,J,3], gt [S,gt_rows,J] (rows 0..2 = x,y,z), valid [S,J] (mode 0) f32;
 * thresholds [T] f64 (device).  mode 0 = PCK in mm over valid joints, mode 1 = PCKh (threshold x the
 * distance between gt joints 0 and 1, every joint).  hits [T,J] and counts [J] are int64; the fraction
 * hits/counts is formed by the caller.  float32 distances with torch's operation order, so the counts
 * equal the reference's. */
int mval_pck3d(const float* pred, const float* gt, const float* valid, const double* thresholds, int T, int mode,
               long long* hits, long long* counts, int64_t S, int J, int gt_rows, void* stream);
/* 2-D PCKh counters (utils/evaluation.py:65-93 compute_pckh, called from strategy.py:579-581).  pred, gt [S,J,2] f32
 * (x,y per image and joint); thresholds [T] f64 (device), T <= 65535.  A joint is hit when its distance to the ground
 * truth is strictly below (float32)(head * (float)threshold[t]), head = the distance between gt joints kp0 and kp1 of the
 * same image; a NaN on either side is no hit; every image and every joint below n_keypoints counts (no validity mask).
 * hits [T,n_keypoints] int64; the fraction hits / S is formed by the caller.  float32 with torch's operation order, so
 * the counts equal the reference's.  Requires J >= 2, 0 <= kp0, kp1 < J, 1 <= n_keypoints <= J. */
int mval_pckh2d(const float* pred, const float* gt, const double* thresholds, int T, int kp0, int kp1,
                long long* hits, int64_t S, int J, int n_keypoints, void* stream);

/* ------------------------------------------------------------------------------------
 * Core-set selection (utils/coreset.py:35-95)
 * ---------------------------------------------------------------------------------- */

/* utils/coreset.py:35-47: pose [n,J,rows] f64 ([joint][coord], rows >= 3) ->
 * feat [n,3J] f64 = [x_0-x_r .. , y_0-y_r .. , z_0-z_r ..]. */
int mval_coreset_features(const double* pose, double* feat, int64_t n, int J, int rows, int root, void* stream);

/* strategy.py:981-989 (cluster-balanced pseudo-labelling): label [n] i32 = index of the nearest of K
 * cluster centres [K,D] f64 for every feature row feat [n,D] f64 (first minimum, as KMeans.predict). */
int mval_nearest_center(const double* feat, const double* centers, int64_t n, int D, int K, int* label, void* stream);

/* Workspace bytes of one mval_kmeans_fit call (0 for non-positive sizes). */
size_t mval_kmeans_workspace_bytes(int64_t n, int D, int K, int L);

/* strategy.py:38-52 KMeans(SAL.NUM_CLUSTERS, random_state=RANDOM_SEED).fit(kp_values): ONE initialisation of
 * sklearn 1.7.2's KMeans (Lloyd, unit weights) on X [n,D] f64, float64 throughout, fixed reduction order
 * (bit-reproducible).  Fits on X - mean(X) and adds the mean back; tol_abs = tol * mean(var(X, axis=0)).
 *   init_centers [K,D] f64, or NULL for greedy k-means++ seeding with the host's draws: first_idx (the first
 *   centre) and rand_u [(K-1)*L] f64 (L = n_local_trials uniforms per further centre, in sklearn's order);
 *   centers [K,D] f64 ; labels [n] i32 ; inertia [1] f64 ; n_iter [1] i32 (sklearn's n_iter_) ;
 *   init_idx [K] i64 = the seeding picks (-1 with init_centers) ; ws >= mval_kmeans_workspace_bytes.
 * Empty clusters are relocated to the farthest rows, largest distance first (lower index on equal distances).
 * Limits: K <= n, K <= 256, D <= 512, K*D <= 3840, L <= 16.  Unlike the other entry points this one
 * synchronises `stream` every 16 Lloyd iterations to stop once converged (not graph-capturable). */
int mval_kmeans_fit(const double* X, int64_t n, int D, int K, const double* init_centers, int64_t first_idx,
                    const double* rand_u, int L, int max_iter, double tol, double* centers, int* labels,
                    double* inertia, int* n_iter, int64_t* init_idx, void* ws, void* stream);

size_t mval_kcenter_workspace_bytes(int64_t n_obs, int D);

/* utils/coreset.py:49-95 greedy k-center on feat [n_obs,D] f64 with sklearn's expanded
 * Euclidean form  sqrt(max(0, (-2 x.c + |x|^2) + |c|^2)).
 *   labeled [n_labeled] i64 row indices (may be NULL/0) ;
 *   have_min_dist != 0: min_dist [n_obs] already holds the running minimum (continuation) ;
 *   row_norms [n_obs] f64 scratch ; picks [n_select] i64 ; ws >= mval_kcenter_workspace_bytes.
 * First maximum wins ties; nothing is masked (duplicates possible, as in the reference).
 * n_labeled == 0 with have_min_dist == 0: every distance starts at +inf, so the first pick is row 0 (the
 * reference's np.argmax(None) == 0); n_select == 0 leaves picks untouched and min_dist initialised. */
int mval_kcenter_select(const double* feat, int64_t n_obs, int D, const int64_t* labeled, int64_t n_labeled,
                        int n_select, int have_min_dist, double* row_norms, double* min_dist,
                        int64_t* picks, void* ws, void* stream);

/* The distance forms of mval_kcenter_select_metric (sklearn's names: "euclidean"/"l2", "manhattan"/"l1"/"cityblock",
 * "cosine", "chebyshev"). */
#define MVAL_KC_EUCLIDEAN 0
#define MVAL_KC_L1 1
#define MVAL_KC_COSINE 2
#define MVAL_KC_CHEBYSHEV 3

/* mval_kcenter_select under another distance: same arguments, same workspace (mval_kcenter_workspace_bytes), same
 * tie / NaN / empty-set rules.  float64, one accumulator, feature index 0 .. D-1 in that order, nothing contracted to fma:
 *   MVAL_KC_EUCLIDEAN  forwards to mval_kcenter_select ;
 *   MVAL_KC_L1         d = sum_k |x_k - c_k| ;
 *   MVAL_KC_CHEBYSHEV  d = max_k |x_k - c_k| ;
 *   MVAL_KC_COSINE     sklearn's cosine_distances: every row is divided once by sqrt(sum_k x_k^2) (a norm below
 *                      10 * DBL_EPSILON, e.g. of a zero row, counts as 1), then d = clip(1 - xh.ch, 0, 2); a row's
 *                      distance to itself is whatever that rounds to, it is not zeroed.
 *   row_norms [n_obs] f64: receives the divisors under MVAL_KC_COSINE, is left untouched under L1 / CHEBYSHEV.
 * Any other metric id fails with a message (mval_last_error). */
int mval_kcenter_select_metric(int metric, const double* feat, int64_t n_obs, int D, const int64_t* labeled,
                               int64_t n_labeled, int n_select, int have_min_dist, double* row_norms, double* min_dist,
                               int64_t* picks, void* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * Heat-map network forward (pose_estimators/hrnet.py:468-501, pose_resnet.py:139-153)
 * ---------------------------------------------------------------------------------- */

/* One fused operator:  out = act(((bn(conv(in)) + res1) + res2))  [nearest-upsampled by 2^up].
 * Activations are NHWC f32 (NCHW for the network input / heat-map output).  Offsets are in
 * floats from the workspace base; -1 = absent.  Weights are in the packed fragment order
 * written by mval_pack_conv_weights; scale/shift are the folded eval-mode BatchNorm
 * (y = x * scale + shift, torch's batch_norm inference formula) or (1, bias). */
enum { MVAL_OP_CONV = 0, MVAL_OP_MAXPOOL = 1, MVAL_OP_DECONV = 2, MVAL_OP_BLOCK = 3, MVAL_OP_TO_P2 = 4, MVAL_OP_BNECK = 5, MVAL_OP_STEM_P2 = 6, MVAL_OP_FUSE_UP = 7 };
enum { MVAL_ALGO_DIRECT = 0, MVAL_ALGO_MFMA = 1, MVAL_ALGO_MFMA_BF3 = 2, MVAL_ALGO_MFMA_H2 = 3, MVAL_ALGO_MFMA_P2 = 4 };
enum { MVAL_PACK_HWIO = 0, MVAL_PACK_MFMA16 = 1, MVAL_PACK_MFMA16_BF3 = 2, MVAL_PACK_MFMA16_H2 = 3 };

typedef struct mval_op {
  int32_t kind;      /* MVAL_OP_*: conv, maxpool (k, stride, pad), transposed conv k4 s2 p1 */
  int32_t algo;      /* MVAL_ALGO_*: which kernel family (and weight packing) the op uses */
  int32_t k, stride, pad;
  int32_t cin, cout;
  int32_t hin, win, hout, wout; /* hout/wout BEFORE the fused upsample */
  int32_t up;        /* log2 upsample factor applied on store (res1/res2/out are at hout<<up) */
  int32_t relu;
  int32_t in_nchw, out_nchw;
  int64_t in_off, out_off, res1_off, res2_off;
  int64_t w_off, scale_off, shift_off; /* floats from the params base */
  int32_t phase, lane; /* scheduling hints: ops of one phase on different lanes are independent
                          (HRNet branches / fuse outputs) and run on separate HIP streams; all
                          lanes join at a phase change.  0/0 = plain in-order execution. */
  /* Activation scales of the fp16-split kernels (MVAL_ALGO_MFMA_H2).  Float offsets into the workspace of
   * n_images rows of MVAL_AMAX_ROW dwords, one row per image of an activation tensor (per image, so that a frame's
   * heat-maps do not depend on the rest of the batch): row[0] = number of partial maxima that follow, row[1..] =
   * bits of max |x| over the part of the image each producing wave wrote (plain stores, no atomics, nothing to
   * zero between forwards); the maximum of the partials is the image's max |x|.  0 = none.  out_amax_off: the op
   * writes the rows of its output (any algo); in_amax_off: the rows of the op's input, required by
   * MVAL_ALGO_MFMA_H2 (single-op callers fill them with mval_amax). */
  int64_t in_amax_off, out_amax_off;
  /* MVAL_OP_BLOCK (hrnet.py:19-52, a whole BasicBlock in one launch, csrc/conv_block.hip):
   *   out = relu(bn2(conv3x3(relu(bn1(conv3x3(in))))) + in),  cin = cout in {32, 48, 64}, k 3, stride 1, pad 1,
   * algo MVAL_ALGO_MFMA_H2.  w_off / scale_off / shift_off are conv1 + bn1, these three conv2 + bn2 (both
   * weights packed MVAL_PACK_MFMA16_H2); res1_off must equal in_off (or be -1). */
  int64_t w2_off, scale2_off, shift2_off;
  /* MVAL_ALGO_MFMA_P2 (csrc/conv_p2.h): the op reads AND writes "P2" activations -- each fp32 value kept as the pair
   * of fp16 planes the fp16-split MFMA consumes, halves [n][plane h,l][C/8][H][W][8] at in_off / res1_off / res2_off /
   * out_off (4 bytes per element, so the float offsets and sizes are those of the fp32 tensor), the per-image rows at
   * in_amax_off / res1_amax_off / res2_amax_off / out_amax_off carrying 2^-s in their last dword.  out_nchw != 0:
   * the output is fp32 NCHW instead (the heat-map layer).  bound_off: params offset of two floats
   * [A = max_c |scale_c| * sum |w_c|, B = max_c |shift_c|], the output's magnitude bound (bound2_off: conv2 of a
   * MVAL_OP_BLOCK).  Weights are packed MVAL_PACK_MFMA16_H2. */
  int64_t bound_off, bound2_off, res1_amax_off, res2_amax_off;
  /* MVAL_OP_TO_P2: format change at the head of a P2 plan -- the fp32 NHWC tensor at in_off ([n][hin][win][cin], its
   * rows [count, partials ...] at in_amax_off, as every NHWC producer keeps them) becomes P2 planes at out_off with
   * their rows at out_amax_off. */
  /* MVAL_OP_BNECK (hrnet.py:75-95, a whole Bottleneck with 64 planes in one launch, csrc/conv_bneck_p2.hip; algo
   * MVAL_ALGO_MFMA_P2 only):
   *   out = relu(bn3(conv1x1(relu(bn2(conv3x3(relu(bn1(conv1x1(in)))))))) + res1),  cin in {64, 256}, cout = 256, stride 1.
   * w_off / scale_off / shift_off / bound_off are conv1 + bn1 (cin -> 64), the *2 fields conv2 + bn2 (64 -> 64, 3x3),
   * these four conv3 + bn3 (64 -> 256); res1_off / res1_amax_off: the 256-channel residual (the block's input or its
   * downsample branch), required. */
  int64_t w3_off, scale3_off, shift3_off, bound3_off;
  /* MVAL_OP_STEM_P2 (hrnet.py:303-310, the two stride-2 stem convs in one launch, csrc/conv_stem_p2.hip; algo
   * MVAL_ALGO_MFMA_P2 only):  out = relu(bn2(conv3x3 s2(relu(bn1(conv3x3 s2(image))))))  from the fp32 NCHW network input
   * (in_off = -1, cin = 3, hin x win multiples of 4) to 64 channels of P2 planes at out_off (hout = hin / 4) with rows at
   * out_amax_off.  w_off: conv1's weights packed MVAL_PACK_HWIO, scale_off / shift_off / bound_off: bn1 and its bound;
   * the *2 fields: conv2 (packed MVAL_PACK_MFMA16_H2) + bn2.  in_amax_off: n_images P2 rows the launch fills with the
   * images' max |x| (a small pass over the input first). */
  /* MVAL_OP_FUSE_UP (hrnet.py:424-447, the up-sampling terms of one fuse-layer output in one launch,
   * csrc/conv_fuse_up_p2.hip; algo MVAL_ALGO_MFMA_P2 only):
   *   out = act(((res1 + up(bn(conv1x1(t_0)))) + up(bn(conv1x1(t_1)))) [+ up(bn(conv1x1(t_2)))])   (left to right, fp32)
   * cout in {32, 64} channels at hout x wout (= hin x win here); res1_off / res1_amax_off: the partial sum so far (required);
   * n_terms in {2, 3}; term j: P2 input of t_cin[j] channels at (hout >> t_up[j]) x (wout >> t_up[j]) at t_in_off[j] with rows at
   * t_in_amax_off[j], 1x1 weights packed MVAL_PACK_MFMA16_H2 at t_w_off[j], folded BN at t_scale_off[j] / t_shift_off[j], bound
   * [A, B] at t_bound_off[j]; relu: the activation of the sum. */
  int32_t n_terms, t_cin[3], t_up[3];
  int32_t no_stem;   /* 1: a 3-channel NCHW stem conv runs on the generic direct kernel, not the stem kernel (the all-direct plan) */
  int64_t t_in_off[3], t_in_amax_off[3], t_w_off[3], t_scale_off[3], t_shift_off[3], t_bound_off[3];
} mval_op;

/* Weight packing.  MVAL_PACK_HWIO: [k*k][cin][cout] (direct kernels, deconv);
 * MVAL_PACK_MFMA16: v_mfma_f32_16x16x4_f32 B-fragment order
 * [k*k][cin/16][cout/16][lane 0..63][4] with lane = (cin_quad << 4) | cout_lane, cin and
 * cout zero-padded to multiples of 16;
 * MVAL_PACK_MFMA16_BF3: the exact three-way bf16 split of every weight in
 * v_mfma_f32_16x16x32_bf16 B-fragment order [k*k][cin/32][cout/16][plane h,m,l][lane][8 bf16]
 * (conv_mfma_split.hip);
 * MVAL_PACK_MFMA16_H2: the two-way fp16 split of every weight times a power of two chosen so that max |w| lands in
 * [2^13, 2^14), same fragment order with two planes [k*k][cin/32][cout/16][plane h,l][lane][8 fp16], followed by
 * a 4-float trailer whose first float is the inverse of that power of two (the conv epilogue multiplies by it).
 * `transposed`: 0 = Conv2d weight [cout,cin,k,k]; 1 = ConvTranspose2d
 * weight [cin,cout,k,k] as the direct kernel reads it; 2 = a [cin,cout,k,k] tensor with the taps
 * flipped: the data-gradient form of a Conv2d weight (pass cout' = cin, cin' = cout) and the
 * forward form of a ConvTranspose2d weight on the MFMA kernels, which run MVAL_OP_DECONV as a
 * stride-1 conv over the zero-dilated input (pass cout, cin as stored).  A ConvTranspose2d's data
 * gradient is a plain conv with its weight read as [cout' = cin][cin' = cout]: transposed = 0. */
size_t mval_packed_weight_floats(int pack, int cout, int cin, int k);
int mval_pack_conv_weights(int pack, int transposed, const float* w, float* packed, int cout, int cin, int k,
                           void* stream);
/* Many MVAL_PACK_MFMA16_BF3 packings in ONE launch (a training plan re-packs every conv weight after each optimizer
 * step, strategy.py:478-484).  jobs_dev: n_jobs descriptors IN DEVICE MEMORY (w / packed are device pointers, mode =
 * the `transposed` argument above); first_block_dev[j] = 256-thread blocks of the jobs before j, a job has
 * (k * k * ceil(cin / 32) * ceil(cout / 16) * 512 + 255) / 256 blocks; total_blocks = their sum. */
typedef struct mval_pack_job {
  const float* w;
  void* packed;
  int mode, cout, cin, k;
} mval_pack_job;
int mval_pack_bf3_jobs(const mval_pack_job* jobs_dev, const int* first_block_dev, int n_jobs, int total_blocks, void* stream);
/* The same for a mix of both splits: a job with bit 8 of `mode` set (mode | 0x100) is packed MVAL_PACK_MFMA16_H2
 * (its max |w| is taken first, in the same call: three launches in all), the others MVAL_PACK_MFMA16_BF3; a job's block
 * count is the same for both. */
int mval_pack_split_jobs(const mval_pack_job* jobs_dev, const int* first_block_dev, int n_jobs, int total_blocks, void* stream);
/* scale = gamma / sqrt(var + eps) ; shift = beta - mean * scale  (all [c] f32). */
int mval_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                 float* scale, float* shift, int c, void* stream);

/* Writes the max-magnitude rows (see mval_op; [n_images][MVAL_AMAX_ROW] dwords) of a tensor of n_images images of
 * per_image consecutive floats each: for tensors that did not come out of an op of the plan. */
#define MVAL_AMAX_ROW 4096
#define MVAL_P2_ROW 512 /* dwords per (tensor, image) row of a P2 activation: 256 partial-maximum slots ... 2^-s in the last one */
int mval_amax(const float* x, int64_t per_image, int n_images, uint32_t* rows, void* stream);
/* fp32 NHWC [n][H][W][C] (C % 8 == 0) whose rows_in ([count, partials ...], as every NHWC producer keeps them) hold
 * its per-image max |x| -> P2 planes (csrc/conv_p2.h) and their rows ([P2 partial slots ... 2^-s]; zero-initialised
 * by the caller once).  And back (tests, network boundaries). */
int mval_nhwc_to_p2(const float* x, const uint32_t* rows_in, void* planes, uint32_t* rows, int n_images, int H, int W, int C,
                    void* stream);
int mval_p2_to_nhwc(const void* planes, const uint32_t* rows, float* out, int n_images, int H, int W, int C, void* stream);

/* 1 when the MFMA kernel family has a configuration for this op geometry (the plan builder
 * asks before choosing MVAL_ALGO_MFMA / MVAL_PACK_MFMA16), else 0. */
int mval_op_mfma_supported(const mval_op* op, int n_images);
/* Same question for a given MVAL_ALGO_* (MFMA, MFMA_BF3 or MFMA_H2). */
int mval_op_algo_supported(const mval_op* op, int n_images, int algo);
/* Which kernel mval_op_launch runs an MVAL_OP_CONV with MVAL_ALGO_DIRECT on: 3 or 7 = the stem kernel of that size (csrc/conv_stem.hip:
 * 3 NCHW input channels, k 3 or 7, stride 2, pad k / 2, cout % 4 == 0, no up-sampling, residual or NCHW output, weights and input
 * patch within 64 KB of LDS), 0 = the generic direct kernel (also when op->no_stem is set, or for any other kind or algo).  Host
 * arithmetic: the predicate the launcher itself asks; no HIP call. */
int mval_conv_stem_covers(const mval_op* op);

/* Which kernel of the split-MFMA conv family (csrc/conv_mfma_split.hip: MVAL_ALGO_MFMA_BF3 / _H2) a launch of the library runs on: the
 * launcher's own dispatch up to, but without, the launch.  Host arithmetic only (no GPU needed, nothing is launched).
 *   pl .. g      the kernel's template arguments: planes (3 = bf16x3, 2 = fp16x2), kernel size (2 = the 2x2 parity conv), stride, cout
 *                waves, pixel waves, cout sub-tiles and pixel sub-tiles per wave, 32-channel chunks per stage
 *   variant      MVAL_SPLIT_*: 6 or 10 staging slots per thread, row sharing (3x3 stride 1, 16-wide tiles), two chunks per stage (g = 2)
 *   th, tw, tn   tile rows x columns x images; odd = 1: th x tw is no power of two (magic-divide decode, tn = 1)
 *   precise      separate accumulator for the correction products (training forward)
 *   grid_x/y/z   pixel tiles, cout groups, parities (4 = the four parity convs of a transposed conv / parity data gradient in one launch)
 *   bn_part_ok   the tile form and the epilogue options allow the batch-statistics partials (given room for them);
 *   bn_part      the launch asks for them and keeps them (mval_train_forward's convs with BatchNorm) */
enum { MVAL_SPLIT_NE6 = 0, MVAL_SPLIT_NE10 = 1, MVAL_SPLIT_ROW_SHARING = 2, MVAL_SPLIT_TWO_CHUNK = 3 };
typedef struct mval_split_form {
  int32_t pl, ks, s, wn, wm, nt, ms, g;
  int32_t variant;
  int32_t th, tw, tn, odd;
  int32_t precise;
  int32_t grid_x, grid_y, grid_z;
  int32_t bn_part_ok, bn_part;
} mval_split_form;
/* `use` = how the library builds the launch from `op` (geometry in FORWARD terms: x [N,hin,win,cin] -> z [N,hout,wout,cout]):
 *   MVAL_SPLIT_USE_OP            mval_op_launch of the op (conv, stride-2 1x1, transposed conv k4 s2 p1; up / relu / out_nchw and
 *                                res1_off / res2_off >= 0 as the op has them)
 *   MVAL_SPLIT_USE_TRAIN_FWD     the same conv as mval_train_forward runs it before its BatchNorm (raw z, precise, partials requested)
 *   MVAL_SPLIT_USE_DGRAD         mval_conv_dgrad_scaled of the conv (res1_off >= 0: accumulate)
 *   MVAL_SPLIT_USE_DGRAD_PARITY  mval_conv_dgrad_parity of the conv (res1_off >= 0: accumulate)
 * algo: MVAL_ALGO_MFMA_BF3 or MVAL_ALGO_MFMA_H2.  Returns 1 and fills *form, or 0 where the library has no split kernel for the launch. */
enum { MVAL_SPLIT_USE_OP = 0, MVAL_SPLIT_USE_TRAIN_FWD = 1, MVAL_SPLIT_USE_DGRAD = 2, MVAL_SPLIT_USE_DGRAD_PARITY = 3 };
int mval_conv_split_form(int use, const mval_op* op, int n_images, int algo, mval_split_form* form);

/* The same question for the exact-fp32 MFMA conv (csrc/conv_mfma.hip: MVAL_ALGO_MFMA), the kernel every other conv is judged against: which
 * instance of conv_mfma_kernel a launch of the library runs on.  Host arithmetic only (no GPU needed, nothing is launched).
 *   ks .. ne     the kernel's template arguments: kernel size, stride, channels per chunk (16 / 32), cout waves, pixel waves, cout sub-tiles
 *                and pixel sub-tiles per wave, staging slots per thread (4 / 6 / 10; 0 = the generic single-buffered staging loop)
 *   th, tw, tn   tile rows x columns x images (powers of two; th * tw * tn = 16 * ms * wm)
 *   dil          2 = the input is read as if zero-dilated by 2 (data gradient of a stride-2 conv, forward of a transposed conv)
 *   nbuf         LDS patch buffers: 2 = double-buffered chunks, 1 = one chunk or the generic staging
 *   grid_x/y     pixel tiles, cout groups
 *   bn_part_ok   the tile form and the epilogue options allow the batch-statistics partials (given room for them);
 *   bn_part      the launch asks for them and keeps them (mval_train_forward's convs with BatchNorm; never a transposed conv)
 * `use` as for mval_conv_split_form.  For MVAL_OP_DECONV (k4 s2 p1), MVAL_SPLIT_USE_OP and _TRAIN_FWD answer the stride-1 k4 conv over the
 * zero-dilated input and MVAL_SPLIT_USE_DGRAD the k4 stride-2 conv mval_train_backward runs as its data gradient; MVAL_SPLIT_USE_DGRAD_PARITY
 * has no exact-fp32 form.  Returns 1 and fills *form, or 0 where the library has no exact-fp32 MFMA kernel for the launch. */
typedef struct mval_mfma_form {
  int32_t ks, s, kc, wn, wm, nt, ms, ne;
  int32_t th, tw, tn;
  int32_t dil;
  int32_t nbuf;
  int32_t grid_x, grid_y;
  int32_t bn_part_ok, bn_part;
} mval_mfma_form;
int mval_conv_mfma_form(int use, const mval_op* op, int n_images, mval_mfma_form* form);

/* The same question for the P2 conv (csrc/conv_p2.hip: MVAL_ALGO_MFMA_P2), the kernel of the default inference and training plans: which
 * instance of conv_p2_kernel a launch of the library runs on and by which runtime path.  Host arithmetic only (no GPU needed, nothing is
 * launched, the device is not asked for anything -- so the form carries no workgroup count, which depends on the occupancy).
 *   ks .. bsum   the kernel's template arguments: kernel size (2 = one 2x2 parity conv), stride, 32-channel chunks per stage, cout waves,
 *                pixel waves, cout sub-tiles and pixel sub-tiles per wave, the power-of-two tile width, row sharing, the epilogue (0 P2
 *                planes, 1 up-sampled P2 planes, 2 fp32 NCHW, 3 raw fp32 NHWC), the odd tile width (0 = none), the paired remainder stage of
 *                48 input channels, BatchNorm + ReLU applied while staging, the BatchNorm backward's sums kept by a data gradient
 *   th, tile_w   the tile's rows and columns (tile_w = ow if set, else tw)
 *   flat         a 1x1 conv whose H x W map runs as one row of H * W pixels (tiles_x / tiles_y are those of that row)
 *   in_sub       a stride-2 1x1 conv run as the stride-1 kernel over every second input pixel
 *   parities     4 = the form is launched four times, once per output parity (a transposed conv), else 1
 *   groups       cout groups (the grid's y); tiles_x, tiles_y, tiles_total = tiles_x * tiles_y * n_images: the tiles the workgroups walk
 *   smem_bytes, threads   dynamic LDS and threads of a workgroup
 * `use` as for mval_conv_split_form, the op's geometry in FORWARD terms:
 *   MVAL_SPLIT_USE_OP            mval_op_launch of the op; for MVAL_OP_DECONV (k4 s2 p1) the 2x2 stride-1 parity conv over the input grid that
 *                                is launched four times (the launches differ in pads and weights only)
 *   MVAL_SPLIT_USE_TRAIN_FWD     the conv as mval_train_forward runs its fwd_p2 ops (raw fp32 NHWC output, statistics partials requested);
 *                                res1_off == -2 asks for the form that applies the producer's BatchNorm + ReLU while staging (zin_rel)
 *   MVAL_SPLIT_USE_DGRAD         the data gradient as mval_train_backward runs it on these kernels (channels swapped, stride 1, fp32 NHWC
 *                                output; res1_off >= 0: accumulate); only stride-1 convs have one
 *   MVAL_SPLIT_USE_DGRAD_PARITY  no P2 form: 0
 * Returns 1 and fills *form, or 0 where the library has no P2 kernel for the launch. */
typedef struct mval_p2_form {
  int32_t ks, s, g, wn, wm, nt, ms, tw, rs, epi, ow, k48, inz, bsum;
  int32_t th, tile_w;
  int32_t flat, in_sub, parities;
  int32_t groups;
  int32_t tiles_x, tiles_y, tiles_total;
  int32_t smem_bytes, threads;
} mval_p2_form;
int mval_conv_p2_form(int use, const mval_op* op, int n_images, mval_p2_form* form);
/* The tiling of the four fused P2 launches as mval_op_launch runs them -- MVAL_OP_BLOCK (csrc/conv_block_p2.hip), MVAL_OP_BNECK
 * (conv_bneck_p2.hip), MVAL_OP_STEM_P2 (conv_stem_p2.hip), MVAL_OP_FUSE_UP (conv_fuse_up_p2.hip) --, read from each launcher's own dry run: host
 * arithmetic only, no GPU needed.  Fills th, tile_w (the output tile: 8 x 16 for the block and the Bottleneck, 2 x 16 for the stem, what the
 * fuse-up launcher picks for the channel count and width -- its six instances differ in (cout, th, tile_w)), tiles_x, tiles_y, tiles_total,
 * groups = 1, parities = 1, smem_bytes (the dynamic LDS of the launch) and threads; every other field is 0.  Returns 1, or 0 where
 * mval_op_algo_supported(op, n_images, MVAL_ALGO_MFMA_P2) does not hold or the op is of another kind. */
int mval_fused_p2_form(const mval_op* op, int n_images, mval_p2_form* form);

int mval_op_launch(const mval_op* op, int n_images, float* workspace, const float* params,
                   const float* net_input, float* net_output, void* stream);

void* mval_net_create(const mval_op* ops, int n_ops);
void mval_net_destroy(void* net);
/* Branch concurrency of mval_net_forward: 1 or -1 = fork / join over private streams (a new net's default),
 * 0 = every op on the caller's stream.  Both forms can be
 * captured into a hipGraph (the fork / join uses events recorded on the capturing stream).  The side streams and
 * events are per device and shared by all nets: ONE forward (or training pass) in flight per device at a time. */
int mval_net_set_multi_stream(void* net, int mode);
int mval_net_forward(void* net, int n_images, float* workspace, const float* params,
                     const float* input_nchw, float* output_nchw, void* stream);
/* Decode from the heat-map layer's epilogue (hrnet.py:344-350,500 / pose_resnet.py final_layer -> utils/evaluation.py:13-30):
 * the same forward, and the kernel that stores the NCHW heat-maps also keeps 64-bit arg-max keys of what it stores in
 * argmax_keys [n_images][MVAL_ARGMAX_SLOTS][joints] (device; zeroed here first): every wave leaves the best key of its
 * part of a map in its own slot of the map (plain stores; more partials per map than slots -- maps above ~8 000
 * pixels -- fold with atomicMax).  key: high word = the stored value as an order-preserving unsigned (NaN highest,
 * -0 == +0), low word = ~flat index, so the largest key is torch.argmax's choice, first index on ties.
 * mval_argmax_from_keys reduces them and yields the key-points mval_argmax_decode would compute from a second read of
 * the maps (bit-equal).  mval_net_keeps_argmax_keys: 1 when the plan's heat-map layer runs on a kernel that does this
 * (the MFMA families; not the generic direct kernels), else mval_net_forward_keys fails. */
#define MVAL_ARGMAX_SLOTS 128
int mval_net_keeps_argmax_keys(void* net);
int mval_net_forward_keys(void* net, int n_images, float* workspace, const float* params,
                          const float* input_nchw, float* output_nchw, uint64_t* argmax_keys, void* stream);
/* Same, with a hipEvent recorded on `stream` around every op; blocks until the stream has
 * drained and writes the elapsed milliseconds of each op to ms_per_op [n_ops] (HOST pointer).
 * Measurement only (not graph-capturable). */
int mval_net_forward_timed(void* net, int n_images, float* workspace, const float* params,
                           const float* input_nchw, float* output_nchw, void* stream, float* ms_per_op);
/* Algorithmic FLOPs (2*MAC) of one op for n_images. */
double mval_op_flops(const mval_op* op, int n_images);

/* ------------------------------------------------------------------------------------
 * Training step of the heat-map network (strategy.py:460-487: forward in train mode,
 * ``batch_loss.backward()``); the optimizer stays in PyTorch (Adam, strategy.py:405).
 * ---------------------------------------------------------------------------------- */

/* Train-mode BatchNorm statistics of z [M, C] (NHWC rows): mean, invstd = 1/sqrt(biased var +
 * eps); running stats updated in place with `momentum` and the unbiased variance (torch).
 * ws >= 512 * C * 2 doubles. */
int mval_bn_batch_stats(const float* z, int64_t M, int C, float eps, float momentum, float* mean, float* invstd,
                        float* running_mean, float* running_var, double* ws, void* stream);
/* The same statistics from per-(channel, conv workgroup) partials part[C][tiles][2] (float64 sum, sum of squares) that the
 * training forward's conv epilogues keep while they store z (mval_train_forward): no second pass over z. */
int mval_bn_finalize_stats(const double* part, int tiles, int64_t M, int C, float eps, float momentum, float* mean,
                           float* invstd, float* running_mean, float* running_var, void* stream);
/* out = act(((z*alpha + (beta - mean*alpha)) nearest-upsampled 2^up) + res1 + res2), alpha = invstd*gamma. */
int mval_bn_apply_fwd(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      const float* res1, const float* res2, float* out, int N, int H, int W, int C, int up, int relu,
                      void* stream);
/* The same, and the max |out| of the tensor left in amax_row ([count, partial maxima ...], >= 513 dwords; NULL = as
 * above): the activation scale of the fp16-split convs that read `out` in training (ONE row per tensor there). */
int mval_bn_apply_fwd_amax(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* res1, const float* res2, float* out, int N, int H, int W, int C, int up, int relu,
                           uint32_t* amax_row, void* stream);
/* The same, and (relu_mask != NULL) the bits (out > 0) of every float4 of `out` in one byte each: relu_mask[i / 4] for the float4
 * that starts at element i (N*Ho*Wo*C/4 bytes) -- what mval_bn_bwd_fused_mask needs of `out`. */
int mval_bn_apply_fwd_mask(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* res1, const float* res2, float* out, int N, int H, int W, int C, int up, int relu,
                           uint32_t* amax_row, uint8_t* relu_mask, void* stream);
/* The same, and the output ALSO as P2 planes (csrc/conv_p2.h: [n][plane][C/8][Ho][Wo][8] fp16 pairs, rows p2_rows[n][MVAL_P2_ROW]) for
 * the P2 convs of the training forward; the tensor's scale comes from the a-priori bound |bn(z)| <= |gamma| sqrt(M - 1) + |beta|
 * (Samuelson) plus the residuals' exact maxima (res*_row: their magnitude rows, required with a residual).  out may be NULL. */
int mval_bn_apply_fwd_p2(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         const float* res1, const float* res2, float* out, void* p2_planes, uint32_t* p2_rows, int N, int H, int W,
                         int C, int up, int relu, uint32_t* amax_row, uint8_t* relu_mask, const uint32_t* res1_row,
                         const uint32_t* res2_row, void* stream);
/* The same with residuals that exist as P2 planes only (same shape as the output; res*_p2_rows: their rows, 2^-s in the scale slot):
 * res1 / res1_p2 are alternatives (both NULL: no residual); the magnitude rows res*_row stay required for the output's scale. */
int mval_bn_apply_fwd_p2_res(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             const float* res1, const float* res2, float* out, void* p2_planes, uint32_t* p2_rows, int N, int H, int W,
                             int C, int up, int relu, uint32_t* amax_row, uint8_t* relu_mask, const uint32_t* res1_row,
                             const uint32_t* res2_row, const void* res1_p2, const uint32_t* res1_p2_rows, const void* res2_p2,
                             const uint32_t* res2_p2_rows, void* stream);
/* Backward of the above: masks gout by (out > 0) when relu, adds it into gres1/gres2 (stores it
 * instead where `overwrite` bit 0 / bit 1 is set: the first writer of a gradient slot), window-sums
 * it to the conv resolution, then (has_bn) dgamma/dbeta and dz = gamma*invstd*(g - dbeta/M -
 * xhat*dgamma/M) written to gz; without BN gz is the masked/window-summed gradient and dbeta its
 * per-channel sum (bias gradient).  ws >= 512*C*2 doubles, sums >= 2*C floats. */
int mval_bn_bwd(const float* gout, const float* out, const float* z, const float* mean, const float* invstd,
                const float* gamma, float* gres1, float* gres2, float* gz, float* dgamma, float* dbeta, double* ws,
                float* sums, int N, int H, int W, int C, int up, int relu, int has_bn, int overwrite, void* stream);
/* The same, and max |gz| left in gz_amax_row (has_bn only; the scale of the fp16-split data-gradient conv). */
int mval_bn_bwd_amax(const float* gout, const float* out, const float* z, const float* mean, const float* invstd,
                     const float* gamma, float* gres1, float* gres2, float* gz, float* dgamma, float* dbeta, double* ws,
                     float* sums, int N, int H, int W, int C, int up, int relu, int has_bn, int overwrite,
                     uint32_t* gz_amax_row, void* stream);
/* Backward of out = act(bn(z) + res1 + res2) without upsample, BatchNorm present, C % 4 == 0: the results of
 * mval_bn_bwd_amax with one tensor write and one to two tensor reads fewer -- the reduction pass does not write the
 * masked gradient (the apply pass re-reads it from the residual slot this op wrote first, or from gout with the mask
 * re-derived), and a ReLU without residuals takes its mask from z (`out` may be NULL then; beta is needed for it). */
int mval_bn_bwd_fused(const float* gout, const float* out, const float* z, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, float* gres1, float* gres2, float* gz, float* dgamma,
                      float* dbeta, double* ws, float* sums, int N, int H, int W, int C, int relu, int overwrite,
                      uint32_t* gz_amax_row, void* stream);
/* The same with the ReLU mask of an op WITH residuals taken from the bytes mval_bn_apply_fwd_mask kept (relu_mask != NULL: `out`
 * is not read; a sixteenth of its bytes). */
int mval_bn_bwd_fused_mask(const float* gout, const float* out, const uint8_t* relu_mask, const float* z, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, float* gres1, float* gres2, float* gz,
                           float* dgamma, float* dbeta, double* ws, float* sums, int N, int H, int W, int C, int relu, int overwrite,
                           uint32_t* gz_amax_row, void* stream);
/* mval_bn_bwd_fused_mask, and (dz_planes != NULL) dz ALSO as P2 planes [n][plane][C/8][H][W][8] + rows dz_rows[n][MVAL_P2_ROW] for the
 * data-gradient conv on the P2 kernels; gmax_ws >= 512 floats, bound_slot one dword of scratch; gz may be NULL then. */
int mval_bn_bwd_fused_p2(const float* gout, const float* out, const uint8_t* relu_mask, const float* z, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, float* gres1, float* gres2, float* gz,
                         float* dgamma, float* dbeta, double* ws, float* sums, int N, int H, int W, int C, int relu, int overwrite,
                         uint32_t* gz_amax_row, void* dz_planes, uint32_t* dz_rows, float* gmax_ws, uint32_t* bound_slot, void* stream);
/* Weight gradient dw [cout][cin][k][k] of a conv: x NHWC (NCHW when x_nchw), dz NHWC.
 * ws >= mval_conv_wgrad_workspace_floats(cin, cout, k) floats. */
size_t mval_conv_wgrad_workspace_floats(int cin, int cout, int k);
int mval_conv_wgrad(const float* x, const float* dz, float* dw, float* ws, int N, int Hin, int Win, int Cin,
                    int Hout, int Wout, int Cout, int k, int stride, int pad, int x_nchw, void* stream);
/* The same; with both magnitude rows ([count, partials], one row per tensor) the split kernels use the fp16x2 form. */
int mval_conv_wgrad_scaled(const float* x, const float* dz, float* dw, float* ws, int N, int Hin, int Win, int Cin,
                           int Hout, int Wout, int Cout, int k, int stride, int pad, int x_nchw,
                           const uint32_t* x_amax_row, const uint32_t* dz_amax_row, void* stream);
/* Which kernel those two entries run the weight gradient on -- the decision of the launcher itself, host arithmetic, no HIP call:
 *   SPLIT    the split-bf16 / fp16 kernel (csrc/conv_wgrad_bf3.hip; NHWC x, pad k / 2, mval_conv_wgrad_split_covers)
 *   STEM     the stem kernel (NCHW x of 3 channels, k 3 or 7, stride 2, pad k / 2, cout a multiple of 16 up to 64)
 *   MFMA     the exact-fp32 kernel (NHWC x, cin % 4 == 0 and >= 16; 1x1 / 3x3 at stride 1 or 2 with pad k / 2, or k4 s2 p1)
 *   DIRECT   the generic kernel for whatever is left, up to 64 * 2048 outputs k * k * cin * cout
 *   REFUSED  more outputs than that (or bad dimensions): the entries return -1 */
enum { MVAL_WGRAD_REFUSED = 0, MVAL_WGRAD_SPLIT = 1, MVAL_WGRAD_STEM = 2, MVAL_WGRAD_MFMA = 3, MVAL_WGRAD_DIRECT = 4 };
int mval_conv_wgrad_path(int cin, int cout, int k, int stride, int pad, int x_nchw);
int mval_slab_reduce(const float* slabs, int S, int64_t n, float* out, int accumulate, void* stream);
/* Backward of MaxPool2d(k, stride, pad) (pose_resnet.py:35 under autograd): gin (+)= gout routed to the
 * first maximum of each window in ATen's scan order (NaN wins); x / gin NHWC [N,Hin,Win,C], gout
 * [N,Hout,Wout,C], C % 4 == 0; accumulate = 0 stores. */
int mval_maxpool_bwd(const float* gout, const float* x, float* gin, int N, int Hin, int Win, int C, int Hout,
                     int Wout, int k, int stride, int pad, int accumulate, void* stream);
/* Data gradient of a conv (geometry given in FORWARD terms: x [N,hin,win,cin] -> z
 * [N,hout,wout,cout], k/stride/pad): dx (+)= conv(dz zero-dilated by the stride, flipped W^T).
 * w_packed: mval_pack_conv_weights(pack, transposed = 2, w, ..., cout' = cin, cin' = cout, k);
 * ones / zeros: >= cin floats of 1.0 / 0.0; algo = MVAL_ALGO_MFMA needs cout % 16 == 0,
 * MVAL_ALGO_MFMA_BF3 cout % 32 == 0 (or 48) and k = 3, or k = 1 with stride 1. */
int mval_conv_dgrad(const float* dz, const float* w_packed, const float* ones, const float* zeros, float* dx,
                    int accumulate, int N, int hin, int win, int cin, int hout, int wout, int cout, int k,
                    int stride, int pad, int algo, void* stream);
/* Data gradient of Conv2d(k3, s2, p1) with even hin / win as four 2x2 stride-1 convs over dz, one per parity of dx, in ONE
 * launch (16 tap-pixels per dz pixel instead of the zero-dilated form's 36; the fp16 split applies).  algo: MVAL_ALGO_MFMA_BF3
 * or _H2 (then dz_amax_row); w_packed: mval_pack_conv_weights(pack, transposed = 4, w, ..., cout' = cin, cin' = cout, k = 4)
 * from the conv's own [cout][cin][3][3] weight.  _supported: 1 when a kernel exists for the shape. */
/* 1 when the split weight-gradient kernel that can read x as P2 planes covers the conv (3x3 stride 1 / 2, wide 1x1; cin % 8 == 0). */
int mval_conv_wgrad_p2_covers(int cin, int cout, int k, int stride);
/* 1 when the split weight-gradient kernel covers the conv at all (it can then read dz as P2 planes when cout % 8 == 0). */
int mval_conv_wgrad_split_covers(int cin, int cout, int k, int stride);
/* 1 when the training forward's P2 conv can apply its producer's BatchNorm + ReLU while staging (3x3 stride 1; mval_train_op.zin_rel). */
int mval_conv_p2_inz_supported(int cin, int cout, int h, int w, int n);
/* 1 when a 3x3 stride-1 data gradient (cin = the conv's cout, cout = its cin, h x w = its input map) can keep those sums. */
int mval_conv_p2_bsum_supported(int cin, int cout, int h, int w, int n);
/* Data-gradient launches of mval_train_backward* that really kept those sums (the flag is a request: without room for the partials the
   plain form runs and the producer's backward reduces on its own) since the library was loaded or last reset; reset != 0 zeroes the
   count after reading it.  Host side only. */
int mval_train_bsum_launches(int reset);
int mval_conv_dgrad_parity_supported(int N, int hin, int win, int cin, int hout, int wout, int cout, int algo);
int mval_conv_dgrad_parity(const float* dz, const float* w_packed, const float* ones, const float* zeros, float* dx,
                           int accumulate, int N, int hin, int win, int cin, int hout, int wout, int cout, int algo,
                           const uint32_t* dz_amax_row, void* stream);
/* The same with algo = MVAL_ALGO_MFMA_H2 allowed (stride 1): dz_amax_row = the magnitude row of dz (one row for the
 * tensor), w_packed in MVAL_PACK_MFMA16_H2 form (with its trailer). */
int mval_conv_dgrad_scaled(const float* dz, const float* w_packed, const float* ones, const float* zeros, float* dx,
                           int accumulate, int N, int hin, int win, int cin, int hout, int wout, int cout, int k,
                           int stride, int pad, int algo, const uint32_t* dz_amax_row, void* stream);

/* One operator of the training graph: the forward geometry / arena offsets (`op`, as in
 * inference, weights packed for the forward kernel at op.w_off; op.shift_off = bias for a conv
 * without BatchNorm) plus what backward needs.  Offsets are floats into `arena` (activations,
 * no reuse), `garena` (activation gradients, same layout) and `params`.  garena is NOT zero-filled:
 * `first_touch` marks the gradient slots this op writes FIRST in backward order (bit 0 data
 * gradient, bit 1 res1, bit 2 res2): those are stored, later writers accumulate; the caller
 * zero-fills only slots that no op writes and places the loss gradient in the last op's gout.
 * op.kind may be MVAL_OP_CONV, MVAL_OP_MAXPOOL (no parameters) or MVAL_OP_DECONV (k4 s2 p1 with
 * BatchNorm, MVAL_ALGO_MFMA; wd_off = its weight packed as a Conv2d weight, transposed = 0). */
typedef struct mval_train_op {
  mval_op op;
  int64_t z_off;      /* raw conv output at conv resolution (arena); unused when has_bn == 0 */
  int64_t gin_off, gout_off, gres1_off, gres2_off; /* garena; -1 = no gradient needed */
  int64_t wd_off;     /* params: weights packed for the data-gradient conv (-1: none) */
  int32_t has_bn, dgrad_algo, first_touch;
  int32_t dgrad_form; /* 0: plain (stride 2: dz read zero-dilated); 1: Conv2d(k3, s2, p1) on even sizes as four 2x2 parity convs
                       * (mval_conv_dgrad_parity; wd_off packed with transposed = 4, k = 4) */
  float* gamma; float* beta; float* running_mean; float* running_var; /* device pointers */
  float* mean; float* invstd;            /* saved batch statistics [cout] */
  float* dweight; float* dgamma; float* dbeta; /* gradient outputs (dbeta = bias grad w/o BN) */
  /* fp16-split kernels in training (op.algo / dgrad_algo == MVAL_ALGO_MFMA_H2): magnitude rows ([count, partials],
   * ONE row per tensor, >= 513 dwords each, float offsets into `arena`; 0 = none).  op.in_amax_off = the row of the
   * op's INPUT activation (written by its producer's out_amax_off); out_amax_off = where this op's BatchNorm apply
   * leaves max |out|; gz_amax_off = the row of the op's dz scratch (written by its BatchNorm backward, read by its
   * data-gradient conv). */
  int64_t out_amax_off, gz_amax_off;
  /* > 0: float offset into `arena` of N*hout*wout*cout/4 BYTES -- the forward apply keeps (out > 0) of every float4 as four
   * bits of one byte there and the backward takes the ReLU mask from it instead of reading `out` (ops with relu, a residual
   * and no upsample; 0 = none). */
  int64_t mask_off;
  /* Round 4: the training forward's convs on the P2 kernels (csrc/conv_p2.hip, raw fp32 NHWC z out + batch-statistics partials).
   * fwd_p2 != 0: this op's conv reads its input as P2 planes at in_p2_off with rows at in_p2_rows_off (float offsets into `arena`;
   * weights packed MVAL_PACK_MFMA16_H2 at op.w_off).  out_p2_off > 0: this op's BatchNorm apply ALSO writes its output as P2 planes
   * there (rows at out_p2_rows_off, n_images * MVAL_P2_ROW dwords, zero-initialised once by the caller); res1_amax_off /
   * res2_amax_off: the magnitude rows ([count, partials]) of its residuals, needed for the P2 scale (0: none / no residual). */
  int32_t fwd_p2;
  int32_t p2_flags; /* bit 0: this op's weight gradient reads its input from the P2 planes (mval_conv_wgrad_p2_covers); bit 1: this op's
                     * apply writes ONLY the P2 planes (every consumer of its output reads those: no fp32 NHWC copy);
                     * bit 6: this op's BatchNorm backward is round 3's pair (masked copy + in-place dz; reads `out`: not with bits 1 - 3);
                     * bit 7: this op's batch statistics come from the separate pass over z, not from its conv's epilogue partials
                     * (bits 6 / 7 / 13 are the caller's decisions: the library reads no environment variable) */
  int64_t in_p2_off, in_p2_rows_off, out_p2_off, out_p2_rows_off, res1_amax_off, res2_amax_off;
  /* p2_flags bit 3: with bit 2 -- the weight gradient reads dz from the planes as well, so the BatchNorm backward writes no fp32 dz.
   * p2_flags bit 2: the op's data gradient runs on the P2 kernels (stride 1): its BatchNorm backward ALSO writes dz as P2 planes into the
   * scratch at gz_p2_off (float offset into `arena`: planes of the largest dz, then n_images * MVAL_P2_ROW row dwords (zeroed once by the
   * caller), then 512 floats + 64 dwords of reduction scratch), and mval_conv_p2 reads them with the data-gradient packing at wd_off. */
  int64_t gz_p2_off, gz_p2_rows_off;
  /* p2_flags bit 4 / bit 5: the forward apply reads res1 / res2 from that activation's P2 planes at res1_p2_off / res2_p2_off (rows at
   * res*_p2_rows_off) -- the residual's producer then writes no fp32 copy when its other readers take the planes too. */
  int64_t res1_p2_off, res1_p2_rows_off, res2_p2_off, res2_p2_rows_off;
  /* Round 6: BatchNorm apply inside the consumer.  z_out != 0: this op's forward apply is NOT run -- its output (ReLU, no residual, no
   * upsample, planes only) has exactly one reader, the 3x3 stride-1 P2 conv `zin_rel` ops away, whose forward staging and whose weight
   * gradient's staging compute relu(BatchNorm(z)) from this op's raw z, batch statistics and affine parameters on the way into LDS
   * (csrc/conv_p2.h P2Args::in_z, conv_wgrad_bf3.hip XZ: the same arithmetic, scale and split as the apply pass -- bit-identical operands).
   * zin_rel != 0 (the reader): ops[i + zin_rel] is that producer (zin_rel < 0: it precedes the reader in the list).  mval_train_backward*
   * may be called on a sub-range of the list: `ops` must then point INTO the full op list whenever an op of the range has zin_rel != 0,
   * because the producer may lie before ops[0] and is dereferenced there. */
  int32_t zin_rel, z_out;  /* p2_flags bit 12 (MVAL_TRAIN_BSUM, with zin_rel == -1): this op's data gradient -- the ONLY writer of its
                            * producer's output gradient -- also keeps the BatchNorm backward reduction of what it writes (P2Args::bs_z), and the
                            * producer's backward skips that pass */
} mval_train_op;
/* p2_flags bits 0 - 7 (the prose at the fields above says when each applies): */
#define MVAL_TRAIN_WGRAD_X_P2 1     /* the weight gradient reads the op's input from the P2 planes */
#define MVAL_TRAIN_OUT_P2_ONLY 2    /* the apply writes ONLY the P2 planes of the op's output: no fp32 NHWC copy */
#define MVAL_TRAIN_DGRAD_P2 4       /* the data gradient runs on the P2 kernels: the BatchNorm backward also writes dz as P2 planes */
#define MVAL_TRAIN_WGRAD_DZ_P2 8    /* with MVAL_TRAIN_DGRAD_P2: the weight gradient reads dz from the planes too, no fp32 dz is written */
#define MVAL_TRAIN_RES1_P2 16       /* the forward apply reads res1 from that activation's P2 planes (res1_p2_off) */
#define MVAL_TRAIN_RES2_P2 32       /* the forward apply reads res2 from that activation's P2 planes (res2_p2_off) */
#define MVAL_TRAIN_BN_BWD_PAIR 64   /* the BatchNorm backward is round 3's pair (reads `out`): not with bits 1 - 3 */
#define MVAL_TRAIN_STATS_PASS 128   /* batch statistics by the separate pass over z, not from the conv's epilogue partials */
#define MVAL_TRAIN_BSUM 4096
/* p2_flags bit 13: this op's weight gradient runs on the exact-fp32 kernels even where the split kernel covers it (the exact-fp32 plan). */
#define MVAL_TRAIN_WGRAD_FP32 8192

/* ones_off / zeros_off: params offsets of >= max(cout) floats of 1.0 / 0.0.
 * ws: ws_doubles >= 512*maxC*2 doubles.  With room for cout * (conv workgroups) * 2 doubles of an op (about
 * n_images*hout*wout*cout / 16 for the 32-pixel tiles, less for larger ones) that op's batch statistics come from its
 * conv epilogue; ops whose partials do not fit run the separate statistics pass. */
int mval_train_forward(const mval_train_op* ops, int n_ops, int n_images, float* arena, const float* params,
                       int64_t ones_off, int64_t zeros_off, const float* input_nchw, float* output_nchw,
                       double* ws, int64_t ws_doubles, float momentum, float eps, void* stream);
/* gz: scratch >= max over ops of N*hout*wout*cout floats; wsf: >= max wgrad workspace;
 * sums: >= 2*maxC floats.  The gradient w.r.t. the network output must already be in garena at
 * the last op's gout_off (NHWC). */
int mval_train_backward(const mval_train_op* ops, int n_ops, int n_images, float* arena, float* garena,
                        const float* params, int64_t ones_off, int64_t zeros_off, const float* input_nchw,
                        float* gz, float* wsf, double* ws, float* sums, void* stream);
/* Round 5: the same two passes with the independent lanes of a phase (mval_op.phase / .lane: HRNet branches, hrnet.py:199-287) on
 * separate HIP streams, joined on `stream` at every phase change and before returning.  An op runs on side stream op.lane (1 ..
 * n_lanes - 1 <= 3) in the forward if p2_flags carries MVAL_TRAIN_LANE_FWD, in the backward if it carries MVAL_TRAIN_LANE_BWD -- the
 * caller sets the backward bit only for phases in which every gradient slot (gin / gres1 / gres2) has all its writers on ONE lane, so
 * the first-touch / accumulate order of every slot is the serial one and the results are bit-identical to mval_train_forward /
 * mval_train_backward.  Every scratch buffer holds n_lanes slices (lane l at base + l * its per-lane size); the per-op dz plane
 * scratch (gz_p2_off ...) must be distinct per lane as well.  One pass per device at a time (the side streams are per device). */
#define MVAL_TRAIN_LANE_FWD 256
#define MVAL_TRAIN_LANE_BWD 512
/* With MVAL_TRAIN_LANE_BWD on the ops of a phase whose lanes DO share gradient slots (a fuse layer's chains, a transition), EVERY op
 * of that phase -- lane 0 included -- carries MVAL_TRAIN_LANE_ORD: each kernel that writes a gradient slot then waits for the slot's
 * previous writer of the phase (list order) through an event, so the slot's store / accumulate order stays the one-stream order. */
#define MVAL_TRAIN_LANE_ORD 1024
/* MVAL_TRAIN_LANE_FREE on every op of a backward call: the lanes do not join at phase changes; they fork once and join once per call,
 * and every op also waits for the last writer of the gradient slot it READS (its own output's gradient).  Same results. */
#define MVAL_TRAIN_LANE_FREE 2048
int mval_train_forward_lanes(const mval_train_op* ops, int n_ops, int n_images, float* arena, const float* params,
                             int64_t ones_off, int64_t zeros_off, const float* input_nchw, float* output_nchw,
                             double* ws, int64_t ws_doubles_per_lane, int n_lanes, float momentum, float eps, void* stream);
int mval_train_backward_lanes(const mval_train_op* ops, int n_ops, int n_images, float* arena, float* garena,
                              const float* params, int64_t ones_off, int64_t zeros_off, const float* input_nchw,
                              float* gz, float* wsf, double* ws, float* sums, int n_lanes, int64_t gz_floats_per_lane,
                              int64_t wsf_floats_per_lane, int64_t ws_doubles_per_lane, int64_t sums_floats_per_lane, void* stream);

/* ---- optimizer step (replaces torch.optim.Adam.step, /root/reference/strategy.py:405-407 and :479) -------------------
 * Adam over MANY tensors in one launch, arithmetic = torch/optim/adam.py _single_tensor_adam in float32:
 *   g = grad (+ weight_decay * p);  m += (1 - beta1) (g - m);  v = v beta2 + (1 - beta2) g g;
 *   p -= step_size * m / (sqrt(v) / bias_correction2_sqrt + eps)
 * with step_size = lr / (1 - beta1^t) and bias_correction2_sqrt = sqrt(1 - beta2^t) evaluated by the caller in double (as
 * python does) and passed as float32 (as torch casts python scalars).  jobs_dev: n_jobs descriptors IN DEVICE MEMORY (device
 * pointers to `count` contiguous float32 each; 16-byte aligned pointers take the vector path); first_block_dev[j] = blocks of
 * the jobs before j, a job has ceil(count / mval_adam_block_elems()) blocks; total_blocks = their sum.  In place. */
typedef struct mval_adam_job {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t count;
} mval_adam_job;
int mval_adam_block_elems(void);
int mval_adam_step(const mval_adam_job* jobs_dev, const int* first_block_dev, int n_jobs, int total_blocks, float one_minus_beta1,
                   float beta2, float one_minus_beta2, float eps, float weight_decay, float step_size, float bias_correction2_sqrt,
                   void* stream);

/* Bound-slack probe of the P2 training tensors (reference has no counterpart: a guard of this implementation's number format;
 * /root/reference/strategy.py:460-487 is the step it watches).  mval_p2_plane_stats measures one P2 tensor ([n][plane][C/8][HW][8] fp16 planes,
 * rows of MVAL_P2_ROW dwords per image) into out4 (device, zeroed by the caller): [0] float bits of 2^-s of image 0, [1] float bits of
 * max |h + l| in scaled units (the a-priori bound sits in [2^13, 2^14) there), [2] number of non-zero values below 2^-3 scaled (fewer than
 * 22 significand bits kept), [3] number of non-zero values.  mval_train_p2_probe(dev_out, n_ops): while dev_out != NULL every
 * mval_train_forward / mval_train_backward call measures the P2 planes it writes -- op i's output planes into dev_out[i][0][4], its dz
 * planes into dev_out[i][1][4] (i = position in the forward's op list; backward calls on a sub-range pass their base through
 * mval_train_timing_base) -- NULL / 0 switches it off. */
int mval_p2_plane_stats(const void* planes, const uint32_t* rows, int n_images, int channels, int hw, uint32_t* out4, void* stream);
int mval_train_p2_probe(uint32_t* dev_out, int n_ops);

/* Measurement only (bench.py, training workload): with a non-NULL HOST array of 6 floats every later
 * mval_train_forward / mval_train_backward call brackets its launches with hipEvents and ADDS the elapsed
 * milliseconds per kernel family -- [conv forward, BN statistics, BN apply, BN backward, weight gradient, data
 * gradient] -- synchronising the stream at the end of the call; NULL switches it off again. */
int mval_train_timing(float* ms_per_family);
/* The same plus a per-operator breakdown into a HOST array [n_ops][6]; mval_train_timing_base(first_op) tells a
 * mval_train_backward call on a sub-range of the op list where that range starts. */
int mval_train_timing_ops(float* ms_per_family, float* ms_per_op_family, int n_ops);
int mval_train_timing_base(int first_op);

#ifdef __cplusplus
}
#endif
#endif /* MVAL_HIP_H */

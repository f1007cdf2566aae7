"""TEST INFRASTRUCTURE ONLY -- float64 numpy restatement of ``mval_triangulate_ransac_weighted``, written from
its definition.  A helper, not a test module.

One problem (frame, joint): its key-points p_v, matrices P_v, the ordered list of view pairs it walks, its present views and,
optionally, per-view weights w_v (float32).

* usable: w_v finite and > 0.  Effective presence = present AND usable; without weights, = present.
* a pair takes part when both its views are below V and effectively present.  Its hypothesis X is the DLT null vector
  (``np.linalg.svd``) of its two views' rows -- x P[2] - P[0], y P[2] - P[1], each multiplied by float64(w_v) -- and its set the
  pair itself plus every effectively present view with half-distance error < eps (unweighted).
* ranking: more views in the set; then the larger S = sum of w_v over the set, views ascending, accumulated in float64; then the
  lower position in the list.  Without weights: more views, then the lower position.
* no pair took part: the set is every effectively present view (the table kernel's fallback).
* the point is the weighted DLT over the winning set, views ascending; joint_error the unweighted mean error over the set.
* a joint that is invalid or has fewer than two effectively present views is unused: point, error, count and mask 0.
* frame: metric = mean of joint_error and inlier_count = min of the counts over the frame's used joints.  No used joint:
  metric NaN and inlier_count -1 without a valid joint, else -2 when the call is masked per problem (weights or
  view_joint_valid) or the frame has fewer than two present views (view_valid).
"""
from __future__ import annotations

import itertools

import numpy as np


def half_distance(P, X, p):
    """1/2 |p - pi(P [X; 1])|, w == 0 -> 1."""
    h = P[:, :3] @ X + P[:, 3]
    w = h[2] if h[2] != 0.0 else 1.0
    return 0.5 * np.sqrt((p[0] - h[0] / w) ** 2 + (p[1] - h[1] / w) ** 2)


def dlt_rows(P, p, w=1.0):
    return np.stack([p[0] * P[2] - P[0], p[1] * P[2] - P[1]]) * np.float64(w)


def dlt(proj, pts, views, weights=None):
    """-> (X (3,), A, singular values) of the (weighted) DLT over ``views``, ascending as handed in."""
    A = np.concatenate([dlt_rows(proj[v], pts[v], 1.0 if weights is None else weights[v]) for v in views])
    _, s, vh = np.linalg.svd(A)
    h = vh[3]
    return h[:3] / (h[3] if h[3] != 0.0 else 1.0), A, s


def usable(weights):
    w = np.asarray(weights, np.float32)
    return np.isfinite(w) & (w > 0)


def set_weight(weights, views):
    s = np.float64(0.0)
    for v in views:  # ascending, one float64 addition each
        s = s + np.float64(np.float32(weights[v]))
    return s


def bits(views):
    return int(sum(1 << int(v) for v in views))


def solve_problem(proj, pts, eps, pairs, present=None, weights=None, valid=True):
    """proj (V, 3, 4), pts (V, 2), pairs: ordered (a, c) list, present (V,) bool or None, weights (V,) or None ->
    dict(point, error, count, mask, used, position (the winner's, None for the fallback), hypotheses: list of
    dict(position, views, count, S, margin = min |e - eps| over its votes), sigma_ratio of the final system)."""
    proj, pts = np.asarray(proj, np.float64), np.asarray(pts, np.float64)
    V = len(proj)
    eff = np.ones(V, bool) if present is None else np.asarray(present, bool).copy()
    if weights is not None:
        eff &= usable(weights)
        weights = np.asarray(weights, np.float32)
    out = dict(point=np.zeros(3), error=0.0, count=0, mask=0, used=False, position=None, hypotheses=[], sigma_ratio=None)
    if not valid or eff.sum() < 2:
        return out
    hyps = []
    for pos, (a, c) in enumerate(pairs):
        a, c = int(a), int(c)
        if a >= V or c >= V or not (eff[a] and eff[c]):
            continue
        X, _, _ = dlt(proj, pts, (a, c), weights)
        views, margin = {a, c}, np.inf
        for v in np.flatnonzero(eff):
            e = half_distance(proj[v], X, pts[v])
            margin = min(margin, abs(e - eps))
            if e < eps:
                views.add(int(v))
        views = sorted(views)
        hyps.append(dict(position=pos, views=views, count=len(views), S=set_weight(weights, views) if weights is not None else None,
                         margin=float(margin)))
    if hyps:
        if weights is None:
            win = min(hyps, key=lambda h: (-h["count"], h["position"]))
        else:
            win = min(hyps, key=lambda h: (-h["count"], -h["S"], h["position"]))
        views, out["position"] = win["views"], win["position"]
    else:
        views = [int(v) for v in np.flatnonzero(eff)]
    X, _, s = dlt(proj, pts, views, weights)
    out.update(point=X, error=float(np.mean([half_distance(proj[v], X, pts[v]) for v in views])), count=len(views), mask=bits(views),
               used=True, hypotheses=hyps, sigma_ratio=float(s[0] / (s[2] - s[3])))
    return out


def lexicographic_pairs(v):
    return list(itertools.combinations(range(v), 2))


def triangulate(kp2d, proj, eps, valid=None, pairs=None, view_valid=None, view_joint_valid=None, weights=None):
    """kp2d (B, V, J, 2), proj (B, V, 3, 4), pairs None (all pairs, lexicographic) | (1, P, 2) | (B, J, P, 2) ->
    dict of keypoints_3d (B, J, 3), joint_error (B, J), joint_inliers, joint_inlier_mask (B, J) int64 (bits as unsigned),
    metric (B,), inlier_count (B,), joint_used (B, J) bool, problems: {(b, j): solve_problem's dict}."""
    kp2d, proj = np.asarray(kp2d, np.float64), np.asarray(proj, np.float64)
    b, v, j = kp2d.shape[:3]
    valid = np.ones((b, j), bool) if valid is None else np.asarray(valid).reshape(b, j) != 0
    out = dict(keypoints_3d=np.zeros((b, j, 3)), joint_error=np.zeros((b, j)), joint_inliers=np.zeros((b, j), np.int32),
               joint_inlier_mask=np.zeros((b, j), np.int64), metric=np.full(b, np.nan), inlier_count=np.zeros(b, np.int32),
               joint_used=np.zeros((b, j), bool), problems={})
    per_problem = weights is not None or view_joint_valid is not None
    for bi in range(b):
        for ji in range(j):
            present = None
            if view_joint_valid is not None:
                present = np.asarray(view_joint_valid)[bi, :, ji] != 0
            elif view_valid is not None:
                present = np.asarray(view_valid)[bi] != 0
            if pairs is None:
                tab = lexicographic_pairs(v)
            else:
                tab = np.asarray(pairs)
                tab = tab[0] if tab.ndim == 3 else tab[bi, ji]
            with np.errstate(all="ignore"):
                r = solve_problem(proj[bi], kp2d[bi, :, ji], eps, tab, present, None if weights is None else np.asarray(weights)[bi, :, ji],
                                  bool(valid[bi, ji]))
            out["problems"][bi, ji] = r
            out["keypoints_3d"][bi, ji], out["joint_error"][bi, ji] = r["point"], r["error"]
            out["joint_inliers"][bi, ji], out["joint_inlier_mask"][bi, ji], out["joint_used"][bi, ji] = r["count"], r["mask"], r["used"]
        used = out["joint_used"][bi]
        if used.any():
            out["metric"][bi] = np.mean(out["joint_error"][bi][used])
            out["inlier_count"][bi] = out["joint_inliers"][bi][used].min()
        else:
            few = view_valid is not None and (np.asarray(view_valid)[bi] != 0).sum() < 2
            out["inlier_count"][bi] = -2 if valid[bi].any() and (per_problem or few) else -1
    return out


_ORACLE = {}


def oracle_of(name, weighted=True):
    """The oracle's result on a generated case (tests/golden/weighted_tri_cases.py), without its weights for ``weighted`` False:
    computed once, shared by the host and the GPU tests, and left unchanged."""
    import weighted_tri_cases as wc

    key = (name, weighted)
    if key not in _ORACLE:
        d = wc.build(wc.weighted_tri_cases()[name])
        _ORACLE[key] = triangulate(d["kp2d"], d["proj"], wc.EPS, d["valid"], d["pairs"], d["view_valid"], d["view_joint_valid"],
                                   d["weights"] if weighted else None)
    return _ORACLE[key]

"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the 3-D refinement ``mval_refine_points_3d``, written
from its definition, and a long-double minimiser of the same cost.  A helper, not a test module.

The problem of one joint: its DLT point X0, its 2-D key-points p_v and its matrices P_v.

* support set S: the present views whose half-distance error at X0, 1/2 |p_v - pi(P_v [X0; 1])| (the vote's
  ``reproj_err``, with its w == 0 -> 1 guard), is finite and < eps; with weights also w_v finite and > 0.
* not refined (status 0, X0 handed through): the joint is invalid, X0 is non-finite or |S| < 2.
* otherwise Levenberg-Marquardt on E(X) = 1/2 sum_{v in S} w_v |p_v - pi(P_v [X; 1])|^2, float64, views ascending:
  lam = 1e-3; per iteration solve (A + lam diag A) d = g with A = sum w J^T J, g = sum w J^T r, try X + d; the step is
  accepted iff every support view has depth > 0 there and E does not rise; accepted -> lam = max(lam / 10, 1e-9) and
  converged (status = iteration) when |d| <= 1e-8 (1 + |X|); rejected -> lam *= 10 and converged when lam > 1e12.
  MAX_ITERS iterations without either: the point so far, status -MAX_ITERS.
* joint_error of a refined joint: the mean over S (ascending) of the half-distance error at the refined point.

Near the minimum the accept test is decided by the last bit of E (two points closer than about 1e-6 mm have costs that differ
by less than their rounding), so the definition fixes the solver's arithmetic: the expressions of ``_normal_equations`` and
``_solve`` in the order written, one IEEE float64 operation each.  They are evaluated here in numpy scalars, which neither fuse
nor reorder anything.
"""
from __future__ import annotations

import numpy as np

MAX_ITERS = 32  # MVAL_REFINE3D_MAX_ITERS (include/mval_hip.h)
LAMBDA_0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-9, 1e12
STEP_TOL = 1e-8


def half_distance(P, X, p):
    """utils/triangulation.py:371-384 for one view: 1/2 |p - pi(P [X; 1])|, w == 0 -> 1."""
    h = P[:, :3] @ X + P[:, 3]
    w = h[2] if h[2] != 0.0 else 1.0
    return 0.5 * np.sqrt((p[0] - h[0] / w) ** 2 + (p[1] - h[1] / w) ** 2)


def support_set(proj, pts, X0, eps, present=None, weights=None):
    """The views of S, ascending.  proj (V, 3, 4), pts (V, 2), present (V,) bool or None, weights (V,) or None; nothing of an
    absent view is read."""
    out = []
    for v in range(len(proj)):
        if present is not None and not present[v]:
            continue
        with np.errstate(all="ignore"):
            e = half_distance(proj[v], X0, pts[v])
        if not (np.isfinite(e) and e < eps):
            continue
        if weights is not None and not (np.isfinite(weights[v]) and weights[v] > 0):
            continue
        out.append(v)
    return out


def _normal_equations(proj, pts, w, X, dtype=np.float64):
    """E, A (its six entries a00 a01 a02 a11 a12 a22), g and whether every view has depth > 0 at X: scalar arithmetic in the
    order the definition states, one IEEE operation after the other -- no fused multiply-add, no library sum."""
    f = dtype
    a00 = a01 = a02 = a11 = a12 = a22 = g0 = g1 = g2 = E = f(0)
    front = True
    x0, x1, x2 = (f(t) for t in X)
    for P, p, wt in zip(proj, pts, w):
        (p00, p01, p02, p03), (p10, p11, p12, p13), (p20, p21, p22, p23) = ((f(t) for t in row) for row in P)
        px, py, wt = f(p[0]), f(p[1]), f(wt)
        h0 = p00 * x0 + p01 * x1 + p02 * x2 + p03
        h1 = p10 * x0 + p11 * x1 + p12 * x2 + p13
        h2 = p20 * x0 + p21 * x1 + p22 * x2 + p23
        front = front and bool(h2 > 0)
        u, v = h0 / h2, h1 / h2
        rx, ry = px - u, py - v
        jx0, jx1, jx2 = (p00 - u * p20) / h2, (p01 - u * p21) / h2, (p02 - u * p22) / h2
        jy0, jy1, jy2 = (p10 - v * p20) / h2, (p11 - v * p21) / h2, (p12 - v * p22) / h2
        a00 = a00 + wt * (jx0 * jx0 + jy0 * jy0)
        a01 = a01 + wt * (jx0 * jx1 + jy0 * jy1)
        a02 = a02 + wt * (jx0 * jx2 + jy0 * jy2)
        a11 = a11 + wt * (jx1 * jx1 + jy1 * jy1)
        a12 = a12 + wt * (jx1 * jx2 + jy1 * jy2)
        a22 = a22 + wt * (jx2 * jx2 + jy2 * jy2)
        g0 = g0 + wt * (jx0 * rx + jy0 * ry)
        g1 = g1 + wt * (jx1 * rx + jy1 * ry)
        g2 = g2 + wt * (jx2 * rx + jy2 * ry)
        E = E + wt * (rx * rx + ry * ry)
    return E * f(0.5), (a00, a01, a02, a11, a12, a22), (g0, g1, g2), front


def _solve(A, g, lam):
    """(A + lam diag A) d = g by LDL^T without pivoting, in the definition's order; None when a pivot is not > 0 or the step is
    not finite."""
    a00, a01, a02, a11, a12, a22 = A
    d0 = a00 + lam * a00
    if not d0 > 0:
        return None
    l10, l20 = a01 / d0, a02 / d0
    d1 = (a11 + lam * a11) - l10 * a01
    if not d1 > 0:
        return None
    l21 = (a12 - l20 * a01) / d1
    d2 = (a22 + lam * a22) - l20 * a02 - l21 * l21 * d1
    if not d2 > 0:
        return None
    y0 = g[0]
    y1 = g[1] - l10 * y0
    y2 = g[2] - l20 * y0 - l21 * y1
    s2 = y2 / d2
    s1 = y1 / d1 - l21 * s2
    s0 = y0 / d0 - l10 * s1 - l20 * s2
    d = np.array([s0, s1, s2])
    return d if np.all(np.isfinite(d)) else None


def _norm3(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def levenberg_marquardt(proj, pts, w, X0, max_iters=MAX_ITERS):
    """-> (X, status) for the views handed in (all of them in S)."""
    X = np.array(X0, dtype=np.float64)
    lam = np.float64(LAMBDA_0)
    with np.errstate(all="ignore"):
        E, A, g, _ = _normal_equations(proj, pts, w, X)
        for k in range(1, max_iters + 1):
            d = _solve(A, g, lam)
            ok = d is not None
            if ok:
                Et, At, gt, front = _normal_equations(proj, pts, w, X + d)
                ok = front and bool(Et <= E)
            if ok:
                X, E, A, g = X + d, Et, At, gt
                lam = max(lam / 10.0, LAMBDA_MIN)
                if _norm3(d) <= STEP_TOL * (1.0 + _norm3(X)):
                    return X, k
            else:
                lam = lam * 10.0
                if lam > LAMBDA_MAX:
                    return X, k
    return X, -max_iters


def cost(proj, pts, w, X):
    """E(X) in float64 over the views handed in."""
    with np.errstate(all="ignore"):
        return float(_normal_equations(np.asarray(proj, np.float64), np.asarray(pts, np.float64), np.asarray(w, np.float64),
                                       np.asarray(X, np.float64))[0])


def refine_point(proj, pts, X0, eps, valid=True, present=None, weights=None, max_iters=MAX_ITERS):
    """One problem -> (X, status, S, joint_error or None).  joint_error None: not refined, the DLT value stays."""
    proj, pts, X0 = np.asarray(proj, np.float64), np.asarray(pts, np.float64), np.asarray(X0, np.float64)
    if not valid:
        return X0.copy(), 0, [], None
    S = support_set(proj, pts, X0, eps, present, weights) if np.all(np.isfinite(X0)) else []
    if len(S) < 2:
        return X0.copy(), 0, S, None
    w = np.ones(len(S)) if weights is None else np.asarray(weights, np.float64)[S]
    X, status = levenberg_marquardt(proj[S], pts[S], w, X0, max_iters)
    return X, status, S, float(np.mean([half_distance(proj[v], X, pts[v]) for v in S]))


def refine_batch(kp2d, proj, kp3d, joint_err, eps, valid=None, view_valid=None, view_joint_valid=None, weights=None):
    """kp2d (B, V, J, 2), proj (B, V, 3, 4), kp3d (B, J, 3), joint_err (B, J) -> dict of keypoints_3d, joint_error,
    joint_support (int32), joint_status (int32), support (B, V, J) bool."""
    kp2d, proj, kp3d = np.asarray(kp2d), np.asarray(proj, np.float64), np.asarray(kp3d, np.float64)
    b, v, j = kp2d.shape[:3]
    out = {"keypoints_3d": kp3d.copy(), "joint_error": np.array(joint_err, np.float64), "joint_support": np.zeros((b, j), np.int32),
           "joint_status": np.zeros((b, j), np.int32), "support": np.zeros((b, v, j), bool)}
    for bi in range(b):
        for ji in range(j):
            present = None
            if view_joint_valid is not None:
                present = np.asarray(view_joint_valid)[bi, :, ji] != 0
            elif view_valid is not None:
                present = np.asarray(view_valid)[bi] != 0
            X, status, S, err = refine_point(proj[bi], kp2d[bi, :, ji].astype(np.float64), kp3d[bi, ji], eps,
                                             valid is None or bool(np.asarray(valid)[bi, ji]), present,
                                             None if weights is None else np.asarray(weights)[bi, :, ji])
            out["keypoints_3d"][bi, ji] = X
            out["joint_support"][bi, ji], out["joint_status"][bi, ji] = len(S), status
            out["support"][bi, S, ji] = True
            if err is not None:
                out["joint_error"][bi, ji] = err
    return out


def minimise_longdouble(proj, pts, w, X_start, max_iters=200):
    """The minimiser of E over the views handed in, to long-double accuracy: Gauss-Newton directions solved in double from
    residuals and a gradient evaluated in ``np.longdouble``, until the step is < 1e-16 relative (a step that raises E is
    halved).  Returns the point rounded to float64 and the last relative step."""
    ld = np.longdouble
    proj, pts, w = np.asarray(proj, ld), np.asarray(pts, ld), np.asarray(w, ld)
    X = np.asarray(X_start, ld)
    rel = np.inf
    for _ in range(max_iters):
        E, (a00, a01, a02, a11, a12, a22), g, _ = _normal_equations(proj, pts, w, X, ld)
        A = np.array([[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]], np.float64)
        d = np.linalg.solve(A, np.array(g, np.float64)).astype(ld)
        for _ in range(60):
            if _normal_equations(proj, pts, w, X + d, ld)[0] <= E:
                break
            d = d / 2
        else:
            d = d * 0
        X = X + d
        rel = float(np.sqrt(d @ d) / (1 + np.sqrt(X @ X)))
        if rel < 1e-16:
            break
    return X.astype(np.float64), rel

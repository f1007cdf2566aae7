"""Host oracle of the key-point undistortion (include/mval_hip.h: mval_undistort_keypoints): the solver in numpy
float64 SCALARS, one operation at a time in the header's order -- python evaluates sums and products left to right as the kernel's
C++ does, and numpy scalars never contract to an FMA --, so that the fold and convergence decisions are the device's.  Nothing here
needs the device."""
from __future__ import annotations

import numpy as np

MAX_ITERS = 16  # MVAL_UNDISTORT_MAX_ITERS
FOLD, NOCONV = -1, -2  # MVAL_UNDISTORT_FOLD, MVAL_UNDISTORT_NOCONV
F = np.float64


def distort(x, y, dist):
    """The reference's forward polynomial (utils/triangulation.py:443-453) on normalised coordinates, operation for operation as
    the solver evaluates it -> (xd, yd, jxx, jyy, jxy): the distorted point and the symmetric Jacobian."""
    k1, k2, p1, p2, k3 = (F(c) for c in dist)
    xx, yy, xy = x * x, y * y, x * y
    r = xx + yy
    r2 = r * r
    r3 = r2 * r
    q = F(1.0) + k1 * r + k2 * r2 + k3 * r3
    s = k1 + F(2.0) * k2 * r + F(3.0) * k3 * r2
    xd = x * q + F(2.0) * p1 * xy + p2 * (r + F(2.0) * xx)
    yd = y * q + F(2.0) * p2 * xd * y + p1 * (r + F(2.0) * yy)  # (xd, not x: the reference has overwritten x by then, :444-453)
    jxx = q + F(2.0) * xx * s + F(2.0) * p1 * y + F(6.0) * p2 * x
    jxy = F(2.0) * xy * s + F(2.0) * p1 * x + F(2.0) * p2 * y
    jyx = F(2.0) * xy * s + F(2.0) * p1 * x + F(2.0) * p2 * y * jxx
    jyy = q + F(2.0) * yy * s + F(6.0) * p1 * y + F(2.0) * p2 * (xd + y * jxy)
    return xd, yd, jxx, jxy, jyx, jyy


def det_jacobian(x, y, dist):
    """det J of the forward polynomial at the normalised point (x, y)."""
    _, _, jxx, jxy, jyx, jyy = distort(F(x), F(y), dist)
    return float(jxx * jyy - jxy * jyx)


def undistort_point(px, py, K, dist):
    """One present entry: (px, py) the key-point as float64 (an int64 or float32 value is exact in it), K (3, 3), dist (5,) ->
    (x, y, status, dets): the undistorted PIXEL in float64 (None, None where the point is handed through) and the det J of every
    iterate that was evaluated, the failing one last."""
    dist = [F(c) for c in dist]
    if all(c == 0.0 for c in dist):
        return None, None, 0, []
    K00, K01, K02, K10, K11, K12 = (F(K[0][0]), F(K[0][1]), F(K[0][2]), F(K[1][0]), F(K[1][1]), F(K[1][2]))
    with np.errstate(all="ignore"):
        a, c = F(px) - K02, F(py) - K12
        detK = K00 * K11 - K01 * K10
        tx, ty = (K11 * a - K01 * c) / detK, (K00 * c - K10 * a) / detK
        x, y = tx, ty
        dets = []
        for k in range(1, MAX_ITERS + 1):
            xd, yd, jxx, jxy, jyx, jyy = distort(x, y, dist)
            fx, fy = xd - tx, yd - ty
            det = jxx * jyy - jxy * jyx
            dets.append(float(det))
            if not (det > 0.0 and det < np.inf):
                return None, None, FOLD, dets
            dx, dy = (jyy * fx - jxy * fy) / det, (jxx * fy - jyx * fx) / det
            x, y = x - dx, y - dy
            tol = F(1e-13) * (F(1.0) + max(abs(x), abs(y)))
            if abs(dx) <= tol and abs(dy) <= tol:  # max(|dx|, |dy|) <= tol, and false for a NaN step
                return float(K00 * x + K01 * y + K02), float(K10 * x + K11 * y + K12), k, dets
        return None, None, NOCONV, dets


def present(b, v, j, valid=None, view_valid=None, view_joint_valid=None):
    """-> (B, V, J) bool: the entries the stage processes."""
    m = np.ones((b, v, j), bool)
    if valid is not None:
        m &= np.asarray(valid).astype(bool).reshape(b, 1, j)
    if view_valid is not None:
        m &= np.asarray(view_valid).astype(bool).reshape(b, v, 1)
    if view_joint_valid is not None:
        m &= np.asarray(view_joint_valid).astype(bool).reshape(b, v, j)
    return m


def undistort_batch(kp, K, dist, valid=None, view_valid=None, view_joint_valid=None):
    """kp (B, V, J, 2) int64 | float32, K (B, V, 3, 3), dist (B, V, 5) -> dict: out64 (B, V, J, 2) float64 -- the undistorted pixel
    before its one rounding to float32; f64(f32(kp)) where handed through, 0 where not processed --, out (B, V, J, 2) float32,
    status (B, V, J) int32, dets: {(b, v, j): [det J, ...]} of the entries that ran the solver."""
    b, v, j = kp.shape[:3]
    m = present(b, v, j, valid, view_valid, view_joint_valid)
    out64, status, dets = np.zeros((b, v, j, 2)), np.zeros((b, v, j), np.int32), {}
    for bi, vi, ji in zip(*np.nonzero(m)):
        px, py = kp[bi, vi, ji]
        x, y, st, d = undistort_point(np.float64(px), np.float64(py), K[bi, vi], dist[bi, vi])
        status[bi, vi, ji] = st
        if d:
            dets[(int(bi), int(vi), int(ji))] = d
        out64[bi, vi, ji] = (x, y) if st > 0 else (np.float64(np.float32(px)), np.float64(np.float32(py)))
    return dict(out64=out64, out=out64.astype(np.float32), status=status, dets=dets)

"""The sub-pixel decode in numpy float64, written from its definition alone -- the reference the device kernel
``mval_refine_keypoints`` is held to (a helper, not a test module).

``refine_map(h, stride, method, valid=True, peak=None)`` -> ``(x, y, conf, status, margin)`` for one map ``h`` (hh, wh) float32.
``peak`` = (px, py) stands in for the map's own arg-max, as the kernel is handed it: a flat neighbourhood of nine equal values is
never around an arg-max of its own map (its first element comes earlier and is as large), so only a given peak reaches it.

* ``x``, ``y``: np.float32, ``(px + ox) * stride`` and ``(py + oy) * stride`` evaluated in float64 and rounded once; ``conf``:
  np.float32, the stored value at the peak.  The flat arg-max (first index on ties, a NaN counts as the maximum: np.argmax's own
  rule) is split BY THE WIDTH.
* ``status``: why the offset is what it is -- "ok" (a refined offset), "border" (peak on the rim), "nonfinite" (one of the nine
  neighbours is NaN or inf), "nonpos" (taylor, peak <= 0), "notmax" (taylor, ``dxx < 0 and det > 0`` fails), "far" (taylor, an offset
  beyond one pixel), "invalid" (the joint is marked invalid: (0, 0), conf 0).
* ``margin``: how far taylor's accept decision was from flipping.  Accepted: ``min(-dxx, det, 1-|ox|, 1-|oy|)`` (> 0).  Rejected:
  minus the LARGEST violation among ``dxx``, ``-det``, ``|ox|-1``, ``|oy|-1`` (<= 0) -- an evaluation that differs from this one in the
  last bit of a logarithm still rejects as long as its most violated condition stays violated.  ``-inf`` where no evaluation can
  come out differently: a flat neighbourhood (nine equal values have nine equal logarithms whatever their last bit, so every
  difference is exactly 0 and ``dxx < 0`` is false), or a violation that is not a finite number.  ``inf`` for every map whose
  offset does not come out of the accept decision (quarter, border, nonfinite, nonpos, invalid): there all arithmetic is exact.
"""
import numpy as np

METHODS = ("quarter", "taylor")
STATUSES = ("ok", "border", "nonfinite", "nonpos", "notmax", "far", "invalid")


def _sgn(d):
    return 1.0 if d > 0.0 else -1.0 if d < 0.0 else 0.0


def _taylor(n):
    """n (3, 3) float64, finite -> (ox, oy, status, margin)."""
    if n[1][1] <= 0.0:
        return 0.0, 0.0, "nonpos", np.inf
    with np.errstate(all="ignore"):
        L = np.log(np.maximum(n, 1e-10))
        gx = 0.5 * (L[1][2] - L[1][0])
        gy = 0.5 * (L[2][1] - L[0][1])
        dxx = L[1][2] - 2.0 * L[1][1] + L[1][0]
        dyy = L[2][1] - 2.0 * L[1][1] + L[0][1]
        dxy = 0.25 * (L[2][2] - L[2][0] - L[0][2] + L[0][0])
        det = dxx * dyy - dxy * dxy
        ox = -(dyy * gx - dxy * gy) / det
        oy = -(dxx * gy - dxy * gx) / det
        is_max = bool(dxx < 0.0 and det > 0.0)
        near = bool(abs(ox) <= 1.0 and abs(oy) <= 1.0)  # (False for a NaN)
        if is_max and near:
            return float(ox), float(oy), "ok", float(min(-dxx, det, 1.0 - abs(ox), 1.0 - abs(oy)))
        if bool((n == n[1][1]).all()):
            return 0.0, 0.0, "notmax", -np.inf
        worst = max(v for v in (dxx, -det, abs(ox) - 1.0, abs(oy) - 1.0) if v == v)  # (a NaN is no measure of anything)
        return 0.0, 0.0, "far" if is_max else "notmax", -float(worst)


def refine_map(h, stride, method, valid=True, peak=None):
    if method not in METHODS:
        raise ValueError(method)
    h = np.asarray(h)
    assert h.dtype == np.float32 and h.ndim == 2
    if not valid:
        return np.float32(0.0), np.float32(0.0), np.float32(0.0), "invalid", np.inf
    hh, wh = h.shape
    idx = int(np.argmax(h))
    px, py = (idx % wh, idx // wh) if peak is None else (int(peak[0]), int(peak[1]))
    assert 0 <= px < wh and 0 <= py < hh
    conf = h[py, px]
    ox, oy, status, margin = 0.0, 0.0, "border", np.inf
    if 1 <= px <= wh - 2 and 1 <= py <= hh - 2:
        n = h[py - 1:py + 2, px - 1:px + 2].astype(np.float64)
        if not np.isfinite(n).all():
            status = "nonfinite"
        elif method == "quarter":
            ox, oy, status = 0.25 * _sgn(n[1][2] - n[1][0]), 0.25 * _sgn(n[2][1] - n[0][1]), "ok"
        else:
            ox, oy, status, margin = _taylor(n)
    x = np.float32((np.float64(px) + np.float64(ox)) * np.float64(stride))
    y = np.float32((np.float64(py) + np.float64(oy)) * np.float64(stride))
    return x, y, conf, status, margin


def refine_batch(hm, stride, method, valid=None, kp2d=None):
    """hm (B, V, J, hh, wh) float32, valid (B, J) or None, kp2d (B,V,J,2) int64 or None: the peaks times the stride, in place of
    the maps' own arg-max -> kp (B,V,J,2) f32, conf (B,V,J) f32, status (B,V,J) object,
    margin (B,V,J) f64."""
    b, v, j = hm.shape[:3]
    kp = np.zeros((b, v, j, 2), np.float32)
    conf = np.zeros((b, v, j), np.float32)
    status = np.empty((b, v, j), object)
    margin = np.zeros((b, v, j), np.float64)
    for bi in range(b):
        for vi in range(v):
            for ji in range(j):
                ok = True if valid is None else bool(valid[bi, ji])
                kp[bi, vi, ji, 0], kp[bi, vi, ji, 1], conf[bi, vi, ji], status[bi, vi, ji], margin[bi, vi, ji] = refine_map(
                    hm[bi, vi, ji], stride, method, ok, None if kp2d is None else kp2d[bi, vi, ji] // stride)
    return kp, conf, status, margin


def hard_decode(hm, stride, valid=None):
    """The int64 hard decode split by the width, (B, V, J, 2): what ``mval_refine_keypoints`` takes as input."""
    b, v, j, hh, wh = hm.shape
    idx = hm.reshape(b, v, j, -1).argmax(-1)
    kp = np.stack([idx % wh, idx // wh], -1).astype(np.int64) * stride
    if valid is not None:
        kp[np.broadcast_to((np.asarray(valid) == 0)[:, None, :], (b, v, j))] = 0
    return kp


def dlt(points, proj):
    """numpy float64 DLT of one joint: points (V, 2), proj (V, 3, 4) -> (3,)."""
    a = np.concatenate([points[:, :1] * proj[:, 2] - proj[:, 0], points[:, 1:] * proj[:, 2] - proj[:, 1]]).astype(np.float64)
    x = np.linalg.svd(a)[2][-1]
    return x[:3] / x[3]


# ---- the branch fixtures: each 3x3 block sits in a 5x5 zero map with the peak at (2, 2) --------------------------------------
BLOCK_OK = [[.5, .5, .75], [.875, 1, .125], [.875, .875, .25]]  # taylor -> (1.44477572, 2.61690243) px
BLOCK_FAR = [[.875, .25, .5], [.75, 1, .875], [.125, .875, .75]]
BLOCK_NOTMAX = [[.125, .75, .5], [.75, 1, .5], [.875, .875, .25]]
BLOCK_PLATEAU = [[1.0] * 3] * 3  # dxx == 0
OK_TAYLOR_PX = (1.44477572, 2.61690243)


def block_map(block, hh=5, wh=5, at=(2, 2)):
    m = np.zeros((hh, wh), np.float32)
    m[at[1] - 1:at[1] + 2, at[0] - 1:at[0] + 2] = np.asarray(block, np.float32)
    return m

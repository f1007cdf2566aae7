"""Seeded cases of the 2-D PCKh goldens (pckh2d.npz, written by make_pckh2d_golden.py from the real reference) and a NumPy
float32 restatement of the two reference functions they pin: the hard arg-max branch of ``get_pred_coordinates``
(utils/evaluation.py:45-58) and ``compute_pckh`` (utils/evaluation.py:65-93).  Everything here is rebuilt from seeds; the
.npz holds only what the reference returned."""
from __future__ import annotations

import numpy as np

THRESHOLDS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)  # the default of compute_pckh_figure
J = 19
f32 = np.float32


# ---- the restatement ----------------------------------------------------------------------------------------------------
def np_pred_coordinates(hm, boxes):
    """hm (N,J,hh,wh) f32, boxes (N,4) f32 -> (N,J,2) f32: flat arg-max (first index on ties, NaN counts as the maximum: both
    numpy's and torch's), split by hh for x AND y, x scaled by (box[3] - box[1]) / wh, y by (box[2] - box[0]) / hh; float32,
    every operation rounded on its own."""
    hm, boxes = np.asarray(hm, f32), np.asarray(boxes, f32)
    n, j, hh, wh = hm.shape
    idx = hm.reshape(n, j, hh * wh).argmax(axis=2)
    sx = (boxes[:, 3] - boxes[:, 1]) / f32(wh)
    sy = (boxes[:, 2] - boxes[:, 0]) / f32(hh)
    x = (idx % hh).astype(f32) * sx[:, None]
    y = (idx // hh).astype(f32) * sy[:, None]
    out = np.stack([x, y], axis=-1)
    assert out.dtype == f32
    return out


def np_pckh_hits(pred, gt, thresholds, num_keypoints, kp0=0, kp1=1):
    """pred, gt (S,J,2) f32 -> hits (T, num_keypoints) int64: dis < head * float32(threshold), strict, all in float32."""
    pred, gt = np.asarray(pred, f32), np.asarray(gt, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        h = gt[:, kp0] - gt[:, kp1]
        head = np.sqrt(h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1])
        e = pred[:, :num_keypoints] - gt[:, :num_keypoints]
        dis = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1])
        assert head.dtype == f32 and dis.dtype == f32
        return np.stack([(dis < (head * f32(t))[:, None]).sum(axis=0) for t in thresholds]).astype(np.int64).reshape(-1, num_keypoints)


def np_pckh(pred, gt, thresholds, num_keypoints, kp0=0, kp1=1):
    """-> (T, num_keypoints) f64 fractions: int / int, as the reference's ``k / count``."""
    return np_pckh_hits(pred, gt, thresholds, num_keypoints, kp0, kp1) / np.float64(np.asarray(pred).shape[0])


def split(a, sizes):
    """(S, ...) -> the list of batches the reference's [batch][image] indexing walks."""
    assert sum(sizes) == a.shape[0]
    edges = np.cumsum([0] + list(sizes))
    return [a[lo:hi] for lo, hi in zip(edges[:-1], edges[1:])]


# ---- metric cases: name -> dict(pred, gt (S,J,2) f32, batches, num_keypoints, kp0, kp1) -------------------------------------
def _noisy():
    rng = np.random.default_rng(20241)
    gt = rng.uniform(20.0, 236.0, (37, J, 2)).astype(f32)
    pred = (gt + rng.standard_normal((37, J, 2)) * 4.0).astype(f32)
    return dict(pred=pred, gt=gt, batches=(16, 16, 5), num_keypoints=J, kp0=0, kp1=1)


def _ties():
    """Integer coordinates; heads of length 5, 10 and 20 along x, along y and as a 3-4-5 triangle; joint offsets of integer
    length m = head * t for thresholds t of the default ten (and m - 1, m + 1 beside them), so that ``dis`` lands exactly on
    ``head * t``: the strict ``<`` and the float32 rounding of ``head * float32(t)`` decide.  float32(0.1), (0.3) and (0.7)
    are not the doubles: 10 * float32(0.3) = 3.00000011920928955 lies exactly half way between two float32 and rounds to
    3.0 (even), so a joint at distance 3 is no hit, while the same product left unrounded in double would be above 3."""
    rng = np.random.default_rng(20242)
    pred, gt = [], []
    for length in (5, 10, 20):
        nsteps = 5 if length == 5 else 10
        step = length // nsteps
        for variant in range(6):
            g = rng.integers(40, 200, (J, 2)).astype(np.int64)
            head = [(length, 0), (0, length), (3 * length // 5, 4 * length // 5)][variant % 3]
            g[1] = g[0] + head
            p = g.copy()
            p[1] = g[1] + head  # dis == head: no hit at t = 1.0, nor below
            for i in range(2, J):
                m = step * ((i - 2) % nsteps + 1) + (0, 0, 0, -1, 1, 0)[variant]
                if variant == 5 and m % 5 == 0:
                    off = (3 * m // 5, -4 * m // 5)
                else:
                    off = [(m, 0), (0, m), (-m, 0), (0, -m)][(i + variant) % 4]
                p[i] = g[i] + off
            pred.append(p)
            gt.append(g)
    pred, gt = np.stack(pred).astype(f32), np.stack(gt).astype(f32)
    return dict(pred=pred, gt=gt, batches=(7, 7, 4), num_keypoints=J, kp0=0, kp1=1)


def _degenerate():
    """num_keypoints 5 < J, head between joints 2 and 5; image 0 has head length 0 and predictions ON the ground truth
    (d = 0: nothing hits, not even dis = 0); image 1 carries a NaN and a +inf prediction among the counted joints."""
    rng = np.random.default_rng(20243)
    gt = rng.uniform(30.0, 220.0, (6, J, 2)).astype(f32)
    pred = (gt + rng.standard_normal((6, J, 2)) * 6.0).astype(f32)
    gt[0, 5] = gt[0, 2]
    gt[0, 1] = gt[0, 0]  # (the default head, joints 0 and 1, is 0 in this image too)
    pred[0] = gt[0]
    pred[1, 0, 0] = np.nan
    pred[1, 1, 1] = np.inf
    pred[1, 3] = gt[1, 3]  # dis = 0 under a positive head: a hit at every threshold
    return dict(pred=pred, gt=gt, batches=(2, 4), num_keypoints=5, kp0=2, kp1=5)


def metric_cases():
    return {"noisy": _noisy(), "ties": _ties(), "degenerate": _degenerate()}


# ---- decode cases ---------------------------------------------------------------------------------------------------------
DECODE_SIZES = ((8, 6), (64, 64), (64, 48), (96, 72))  # (hh, wh)
DECODE_BOXES = np.array([[0.0, 0.0, 256.0, 256.0], [12.5, 30.25, 212.5, 230.25], [10.0, 20.0, 110.0, 180.0]], f32)  # the last is not square


def decode_name(hh, wh):
    return "decode_%dx%d" % (hh, wh)


def decode_case(hh, wh):
    """-> (hm (3,5,hh,wh) f32, boxes (3,4) f32).  Joint 0: one peak at row 5/8 hh, column 4/6 wh (row 5, column 4 of the 8 x 6
    map); joint 1: two equal peaks, the first flat index wins; joint 2: the peak is the last pixel, flat index >= hh * (wh - 1),
    where the quirk's idx / hh is largest; joint 3: a constant map (index 0); joint 4: a peak at a seeded place."""
    rng = np.random.default_rng(20244 + hh * 1000 + wh)
    n, j = DECODE_BOXES.shape[0], 5
    hm = (rng.random((n, j, hh, wh)) * 0.1).astype(f32)
    for b in range(n):
        hm[b, 0, 5 * hh // 8, 4 * wh // 6] = 1.0
        r = sorted(rng.choice(hh * wh, 2, replace=False))
        hm[b, 1].reshape(-1)[r] = 1.0
        hm[b, 2, hh - 1, wh - 1] = 1.0
        hm[b, 3] = 0.25
        hm[b, 4].reshape(-1)[rng.integers(hh * wh)] = 1.0
    return hm, DECODE_BOXES.copy()


# ---- the pass case: what _evaluate_2d_pckh sees at world size 1 ---------------------------------------------------------------
PASS_BATCHES = ((2, 4), (2, 4), (1, 4))  # (B, V)
PASS_HW = 16


def pass_case():
    """-> (loader, heatmaps): per batch a dict of host arrays (images (B,V,3,8,8) f32, square_box (B,V,4) f32, 2d_after_crop
    (B,V,19,2) f32) and the (B*V,19,16,16) f32 maps a model returns for it, one planted peak per map.  The ground truth is the
    peak's box-scaled place plus Gaussian noise of 8 % of the box side, so that the ten thresholds separate the joints."""
    rng = np.random.default_rng(20245)
    loader, maps = [], []
    for b, v in PASS_BATCHES:
        n = b * v
        hm = (rng.random((n, J, PASS_HW, PASS_HW)) * 0.1).astype(f32)
        peak = rng.integers(PASS_HW * PASS_HW, size=(n, J))
        for i in range(n):
            for k in range(J):
                hm[i, k].reshape(-1)[peak[i, k]] = 1.0
        side = rng.choice(np.array([64.0, 100.0, 130.5], f32), n)
        lt = rng.integers(0, 50, (n, 2)).astype(f32)
        box = np.concatenate([lt, lt + side[:, None]], axis=1).astype(f32)
        place = np.stack([peak % PASS_HW, peak // PASS_HW], axis=-1) * (side[:, None, None] / PASS_HW)
        gt = (place + rng.standard_normal((n, J, 2)) * 0.08 * side[:, None, None]).astype(f32)
        loader.append({"images": np.zeros((b, v, 3, 8, 8), f32), "square_box": box.reshape(b, v, 4),
                       "2d_after_crop": gt.reshape(b, v, J, 2)})
        maps.append(hm)
    return loader, maps

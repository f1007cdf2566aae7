"""NumPy oracle of the weighted training loss (include/mval_hip.h: mval_weighted_mse_fwd), steps 2-5 of its contract
written out literally with Python loops.  A helper, not a test module.

  S (N, J) float64: every map's sum of squared errors (given: the tests take the device's own, whose bits are pinned elsewhere)
  l = float64(w) * S                                       per_map_loss
  per image the J values l ranked with NaN first and ties to the lowest joint; the first topk selected (0: all)   select
  T[n] = the selected l[n, j] added in ascending j; loss = float32(sum of T[n] in ascending n / denom)              loss_value
  grad = ((2 * (h - g)) * (grad_out / float32(denom))) * wsel in float32, +0.0 where wsel == 0                       gradient
"""
import numpy as np


def better(v, i, bv, bi):
    """The order of torch.argmax (csrc/numeric_order.h: argmax_better): True when (v, i) comes before (bv, bi)."""
    vn, bn = v != v, bv != bv
    if vn != bn:
        return bool(vn)
    if vn:
        return i < bi
    return bool(v > bv) or bool(v == bv and i < bi)


def per_map_loss(w, S):
    w = np.asarray(w, dtype=np.float32)
    S = np.asarray(S, dtype=np.float64)
    out = np.empty(S.shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in np.ndindex(S.shape):
            out[idx] = np.float64(w[idx]) * S[idx]
    return out


def select(l, w, topk):
    """l, w (N, J) -> (selected (N, J) bool, wsel (N, J) float32)."""
    l = np.asarray(l, dtype=np.float64)
    w = np.asarray(w, dtype=np.float32)
    n_images, n_joints = l.shape
    assert 0 <= topk <= n_joints
    sel = np.zeros(l.shape, dtype=bool)
    for n in range(n_images):
        for j in range(n_joints):
            rank = 0
            for k in range(n_joints):
                if k != j and better(l[n, k], k, l[n, j], j):
                    rank += 1
            sel[n, j] = topk == 0 or rank < topk
    wsel = np.where(sel, w, np.float32(0.0)).astype(np.float32)
    return sel, wsel


def loss_value(l, sel, denom):
    l = np.asarray(l, dtype=np.float64)
    total = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(l.shape[0]):
            t = np.float64(0.0)
            for j in range(l.shape[1]):
                if sel[n, j]:
                    t = t + l[n, j]
            total = total + t
        return np.float32(total / np.float64(denom)) if l.shape[0] else np.float32(0.0)


def forward(w, S, topk, denom):
    """(loss float32, l (N, J) float64, wsel (N, J) float32) of weights w and per-map sums S."""
    l = per_map_loss(w, S)
    sel, wsel = select(l, w, topk)
    return loss_value(l, sel, denom), l, wsel


def gradient(h, g, wsel, grad_out, denom):
    """h, g (N, J, hw) float32, wsel (N, J) float32 -> grad_h (N, J, hw) float32; a map with wsel == 0 is +0.0 whatever it holds."""
    h = np.asarray(h, dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    gs = np.float32(grad_out) / np.float32(denom)
    out = np.zeros(h.shape, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(h.shape[0]):
            for j in range(h.shape[1]):
                if wsel[n, j] != 0:  # (a NaN weight counts)
                    d = (h[n, j] - g[n, j]).astype(np.float32)
                    out[n, j] = (((np.float32(2.0) * d).astype(np.float32) * gs).astype(np.float32) * wsel[n, j]).astype(np.float32)
    return out

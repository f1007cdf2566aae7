"""TEST INFRASTRUCTURE ONLY -- CPU restatement (pure numpy) of the reference's core-set selector, utils/coreset.py:49-95,
under the metrics it hands to ``sklearn.metrics.pairwise_distances`` besides "euclidean":

* "manhattan" / "l1" / "cityblock" -> scipy's cdist "cityblock":  d = sum_k |x_k - c_k|
* "chebyshev"                      -> scipy's cdist "chebyshev":  d = max_k |x_k - c_k|
* "cosine"                         -> sklearn's cosine_distances: rows divided by their norm sqrt(sum_k x_k^2) (a norm
  below 10 * eps counts as 1: sklearn's ``normalize``), then d = clip(1 - xh . ch, 0, 2); no zeroing of a row's distance
  to itself (the reference passes two different arrays).

Every sum runs over the feature index k = 0 .. D-1 in that order with ONE accumulator per (row, centre) and every
operation rounds once -- the loops are over k, vectorised over the rows only.  That order reproduces the reference's l1 and
Chebyshev distances bit for bit (tests/golden/coreset_metric.npz); its cosine distances go through BLAS and differ from
these by rounding.  Chebyshev keeps a NaN term (np.maximum); scipy would drop it, but sklearn refuses non-finite input
before scipy sees it, so the reference defines nothing there.
"""
from __future__ import annotations

import numpy as np

ALIASES = {"euclidean": "euclidean", "l2": "euclidean", "manhattan": "l1", "l1": "l1", "cityblock": "l1",
           "cosine": "cosine", "chebyshev": "chebyshev"}
NEW_FORMS = ("l1", "cosine", "chebyshev")


def stacked_features(pool_pose, labeled_pose, root_idx):
    """utils/coreset.py:35-47 on arrays: pool (n, J, >=3) rows first, labeled (l, J, >=3) rows last; per pose the
    coordinates 0..2 minus the root joint's, flattened coordinate-major, float64."""
    out = []
    for p in (pool_pose, labeled_pose):
        p = np.asarray(p, dtype=np.float64)[:, :, 0:3].transpose(0, 2, 1)  # (n, 3, J)
        out.append((p - p[:, :, root_idx:root_idx + 1]).reshape(len(p), 3 * p.shape[2]))
    return np.concatenate(out, axis=0)


def normalise_rows(feat):
    """sklearn.preprocessing.normalize(feat) with the sum of squares taken in feature order."""
    feat = np.asarray(feat, dtype=np.float64)
    s = np.zeros(len(feat))
    for k in range(feat.shape[1]):
        s = s + feat[:, k] * feat[:, k]
    norms = np.sqrt(s)
    norms[norms < 10 * np.finfo(np.float64).eps] = 1.0
    return feat / norms[:, None]


def prepare(feat, metric):
    """The table the distances are taken on: the features, row-normalised for cosine."""
    form = ALIASES[metric]
    assert form in NEW_FORMS, metric
    feat = np.asarray(feat, dtype=np.float64)
    return normalise_rows(feat) if form == "cosine" else feat


def distances(table, centre_rows, metric):
    """(n, C) distances of every row of ``table`` (from ``prepare``) to its rows ``centre_rows``."""
    form = ALIASES[metric]
    centre_rows = list(centre_rows)
    if len(centre_rows) > 16:  # (cache-sized groups of centres: the same numbers, several times faster)
        return np.concatenate([distances(table, centre_rows[i:i + 16], metric) for i in range(0, len(centre_rows), 16)], axis=1)
    cen = table[centre_rows]
    acc = np.zeros((len(table), len(cen)))
    t = np.empty_like(acc)
    with np.errstate(invalid="ignore"):
        for k in range(table.shape[1]):
            x, c = table[:, k:k + 1], cen[None, :, k]
            if form == "cosine":
                acc += np.multiply(x, c, out=t)
            elif form == "l1":
                acc += np.abs(np.subtract(x, c, out=t), out=t)
            else:
                np.maximum(acc, np.abs(np.subtract(x, c, out=t), out=t), out=acc)
        if form == "cosine":
            acc = np.clip(1.0 - acc, 0.0, 2.0)
    return acc


def kcenter_greedy(feat, labeled_idx, n_select, metric, min_d=None):
    """utils/coreset.py:49-95 on an explicit feature table.  Returns (picks, min_distances (n,) or None, gaps): per step
    the relative gap (top1 - top2) / top1 of ``min_distances`` (inf where there is no finite pair).  Labeled rows take part
    in min / arg-max; nothing is masked; without any distance yet np.argmax(None) == 0.  ``min_d``: a running minimum to
    continue from (coreset.py:59-69)."""
    table = prepare(feat, metric)
    labeled_idx = list(labeled_idx)
    min_d = None if min_d is None else np.array(min_d, dtype=np.float64)
    if labeled_idx:
        d = np.min(distances(table, labeled_idx, metric), axis=1)
        min_d = d if min_d is None else np.minimum(min_d, d)
    picks, gaps = [], []
    for _ in range(n_select):
        ind = int(np.argmax(min_d))  # np.argmax(None) == 0; a NaN is the maximum
        gaps.append(relative_gap(min_d))
        d = distances(table, [ind], metric)[:, 0]
        min_d = d if min_d is None else np.minimum(min_d, d)
        picks.append(ind)
    return picks, min_d, gaps


def relative_gap(min_d):
    """(top1 - top2) / top1 of a min_distances vector; inf without two finite values or with top1 == 0."""
    if min_d is None:
        return float("inf")
    m = np.asarray(min_d, dtype=np.float64).ravel()
    if m.size < 2 or not np.isfinite(m).all():
        return float("inf")
    top = np.partition(m, -2)[-2:]
    return float((top[1] - top[0]) / top[1]) if top[1] > 0 else float("inf")

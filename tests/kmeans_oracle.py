"""TEST INFRASTRUCTURE ONLY -- plain numpy float64 restatement of ONE initialisation of scikit-learn 1.7.2's KMeans
(unit sample weights, dense X, algorithm "lloyd").  The random numbers are arguments, as for ``mval_kmeans_fit``.

* ``plusplus``  follows ``sklearn.cluster._kmeans._kmeans_plusplus`` on the centred X: the expanded distance
  max(0, (-2 x.c + |c|^2) + |x|^2), ``np.cumsum`` + ``np.searchsorted`` (left) clipped to n - 1, first minimum of the
  candidate potentials.
* ``lloyd``     follows ``_kmeans_single_lloyd`` as ``KMeans.fit`` calls it (X and the init centred by the column
  mean, tol_abs = tol * mean(var)): first-minimum argmin of |c|^2 - 2 x.c, ``_relocate_empty_clusters_dense``
  (farthest rows from their old centre largest first, lower index on ties), ``_average_centers`` in its in-place order,
  strict convergence tested before the tol test, the final E-step unless the labels converged strictly.

Everything is the obvious sequential code over whole arrays; nothing here knows of workgroups, tiles or partial sums.
Both functions also report how close the input came to a decision that rounding could turn (the "gaps"), so that a
test can require its input to be well away from one instead of loosening a comparison.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

INF = float("inf")

PlusPlus = namedtuple("PlusPlus", "picks pot_gap search_gap candidates")
Lloyd = namedtuple("Lloyd", "centers labels inertia n_iter gap info")


def _centred(x):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    return x - mean, mean


def _expanded_sq_dists(xc, xnorm, rows):
    """sklearn's _euclidean_distances(X[rows], X, squared=True): (len(rows), n)."""
    c = xc[rows]
    d = -2.0 * (c @ xc.T)
    d += (c * c).sum(axis=1)[:, None]
    d += xnorm[None, :]
    np.maximum(d, 0.0, out=d)
    return d


def plusplus(x, k, first_idx, rand_u, n_trials):
    """Greedy k-means++ picks.  Returns PlusPlus(picks (k,), pot_gap, search_gap, candidates):

    pot_gap     smallest (pot_l - pot_best) / pot_l over the steps and over the candidates l that are another ROW than
                the winner (0: two different rows tie in potential; inf: never a second row)
    search_gap  smallest distance of a target u * potential from the two prefix sums that bracket it, relative to the
                potential (0: the target lies exactly on a prefix sum)
    candidates  per step the ``n_trials`` candidate rows (after the clip)"""
    xc, _ = _centred(x)
    n = xc.shape[0]
    xnorm = (xc * xc).sum(axis=1)
    picks = [int(first_idx)]
    closest = _expanded_sq_dists(xc, xnorm, [int(first_idx)])[0]
    pot = closest.sum()
    u = np.asarray(rand_u if rand_u is not None else [], dtype=np.float64).reshape(k - 1, n_trials)
    pot_gap = search_gap = INF
    cands = []
    for c in range(1, k):
        targets = u[c - 1] * pot
        prefix = np.cumsum(closest)
        cand = np.searchsorted(prefix, targets)  # side="left"
        for t, i in zip(targets, cand):
            near = [abs(prefix[i] - t)] if i < n else []
            if i > 0:
                near.append(abs(t - prefix[min(i, n) - 1]))
            if pot > 0:
                search_gap = min(search_gap, min(near) / pot)
        cand = np.minimum(cand, n - 1)
        d = np.minimum(closest[None, :], _expanded_sq_dists(xc, xnorm, cand))
        pots = d.sum(axis=1)
        best = int(np.argmin(pots))  # first minimum
        for l in range(n_trials):
            if cand[l] != cand[best]:
                pot_gap = min(pot_gap, (pots[l] - pots[best]) / pots[l] if pots[l] > 0 else 0.0)
        pot = pots[best]
        closest = d[best]
        picks.append(int(cand[best]))
        cands.append([int(i) for i in cand])
    return PlusPlus(np.asarray(picks, dtype=np.int64), float(pot_gap), float(search_gap), cands)


def _assign(xc, xnorm, cen):
    """First-minimum argmin of |c|^2 - 2 x.c and the smallest gap between a row's best and second-best value, relative
    to |x|^2 + the larger of the two |c|^2 (the size of the numbers whose rounding decides the comparison)."""
    cc = (cen * cen).sum(axis=1)
    v = cc[None, :] - 2.0 * (xc @ cen.T)
    labels = np.argmin(v, axis=1).astype(np.int32)
    if cen.shape[0] < 2:
        return labels, INF
    two = np.argpartition(v, 1, axis=1)[:, :2]
    rows = np.arange(len(v))
    v0, v1 = v[rows, two[:, 0]], v[rows, two[:, 1]]
    scale = xnorm + np.maximum(cc[two[:, 0]], cc[two[:, 1]])
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(scale > 0, np.abs(v1 - v0) / scale, 0.0)
    return labels, float(g.min())


def lloyd(x, init_centers, max_iter, tol):
    """Lloyd iterations from ``init_centers``.  Returns Lloyd(centers, labels (int32), inertia, n_iter, gap, info):

    gap   smallest relative gap between a row's best and second-best centre over every E-step (the final one included)
    info  dict: ``ended`` ("strict" | "tol" | "max_iter"), per iteration ``n_empty``, ``changed`` and ``shift_tot``,
          ``relocated`` (per iteration the (far row, its old cluster, the empty cluster) triples), ``reloc_gap``
          (smallest relative gap between two successive farthest distances that are not exact duplicates rows),
          ``fallback`` (per iteration the clusters that took the largest cluster's row in _average_centers),
          ``tol_abs``, ``tol_margin`` (smallest |shift_tot - tol_abs| / tol_abs over the iterations whose labels
          changed), ``labels_last_iter`` (the labels before the final E-step)"""
    x = np.asarray(x, dtype=np.float64)
    xc, mean = _centred(x)
    n, dim = xc.shape
    xnorm = (xc * xc).sum(axis=1)
    cen = np.array(init_centers, dtype=np.float64) - mean
    k = cen.shape[0]
    tol_abs = 0.0 if tol == 0 else float(np.mean(np.var(x, axis=0)) * tol)
    labels_old = np.full(n, -1, dtype=np.int32)
    info = dict(ended="max_iter", n_empty=[], changed=[], shift_tot=[], relocated=[], fallback=[], reloc_gap=INF,
                tol_abs=tol_abs, tol_margin=INF)
    gap = INF
    strict = False
    n_iter = 0
    labels = labels_old
    for it in range(max_iter):
        labels, g = _assign(xc, xnorm, cen)
        gap = min(gap, g)
        sums = np.zeros((k, dim))
        np.add.at(sums, labels, xc)  # unbuffered: rows are added one by one in row order
        cnt = np.bincount(labels, minlength=k).astype(np.float64)
        empty = np.flatnonzero(cnt == 0)
        moved = []
        if len(empty):
            dist = ((xc - cen[labels]) ** 2).sum(axis=1)
            if dist.max() != 0:
                order = np.lexsort((np.arange(n), -dist))  # largest first, lower index on equal distances
                for a, b in zip(order[:len(empty)], order[1:len(empty) + 1]):
                    if not np.array_equal(xc[a], xc[b]):
                        info["reloc_gap"] = min(info["reloc_gap"], (dist[a] - dist[b]) / dist[a])
                for e, far in zip(empty, order[:len(empty)]):
                    old = int(labels[far])
                    sums[old] -= xc[far]
                    sums[e] = xc[far]
                    cnt[e] = 1.0
                    cnt[old] -= 1.0
                    moved.append((int(far), old, int(e)))
        am = int(np.argmax(cnt))
        new = sums
        fell = []
        for j in range(k):  # in place: an empty cluster copies the largest one's row as it is at that moment
            if cnt[j] > 0:
                new[j] *= 1.0 / cnt[j]
            else:
                new[j] = new[am]
                fell.append(j)
        shift = np.sqrt(((new - cen) ** 2).sum(axis=1))
        tot = float((shift ** 2).sum())
        cen = new
        n_iter = it + 1
        changed = int((labels != labels_old).sum())
        info["n_empty"].append(len(empty))
        info["changed"].append(changed)
        info["shift_tot"].append(tot)
        info["relocated"].append(moved)
        info["fallback"].append(fell)
        if changed == 0:
            strict = True
            info["ended"] = "strict"
            break
        if tol_abs > 0:
            info["tol_margin"] = min(info["tol_margin"], abs(tot - tol_abs) / tol_abs)
        if tot <= tol_abs:
            info["ended"] = "tol"
            break
        labels_old = labels
    info["labels_last_iter"] = labels.copy()
    if not strict:
        labels, g = _assign(xc, xnorm, cen)
        gap = min(gap, g)
    inertia = float(((xc - cen[labels]) ** 2).sum())
    return Lloyd(cen + mean, labels, inertia, n_iter, float(gap), info)


def fit(x, k, first_idx, rand_u, n_trials, max_iter, tol):
    """Seeding then Lloyd, as one ``mval_kmeans_fit`` call without an array init: (PlusPlus, Lloyd)."""
    x = np.asarray(x, dtype=np.float64)
    pp = plusplus(x, k, first_idx, rand_u, n_trials)
    return pp, lloyd(x, x[pp.picks], max_iter, tol)

"""Deterministic inputs of the KMeans goldens (tests/golden/make_kmeans_golden.py -> kmeans.npz).

Every case is regenerated from numpy's ``default_rng`` where it is used; only the results are stored."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np


def kmeans_cases():
    """name -> dict(n, d, k, kind, kwargs): kind "modes" (pose modes plus noise, as cases.sal_filter_inputs),
    "gauss" (unstructured), "dups" (6 distinct rows, exact arithmetic), "far_init" (array init with one centre far from the data:
    its cluster is empty after the first assignment and takes the farthest row)."""
    return OrderedDict(
        c1_small=dict(seed=101, n=60, d=57, k=4, kind="modes", kwargs=dict(random_state=0)),
        c2_k10=dict(seed=102, n=300, d=57, k=10, kind="modes", kwargs=dict(random_state=1307)),
        c3_interhand_ninit3=dict(seed=103, n=5000, d=126, k=10, kind="modes", kwargs=dict(n_init=3, random_state=7)),
        c4_panoptic_50k=dict(seed=104, n=50000, d=57, k=10, kind="modes", kwargs=dict(random_state=1307)),
        c5_gauss_50k=dict(seed=105, n=50000, d=57, k=10, kind="gauss", kwargs=dict(random_state=1307)),
        c6_duplicates=dict(seed=106, n=32, d=9, k=8, kind="dups", kwargs=dict(random_state=3)),
        c7_array_init=dict(seed=107, n=500, d=57, k=5, kind="far_init", kwargs=dict()),
        c8_randomstate=dict(seed=108, n=1000, d=57, k=6, kind="modes", kwargs=dict(n_init=2, random_state="rs:123")),
    )


STRUCTURED = ("c1_small", "c2_k10", "c3_interhand_ninit3", "c4_panoptic_50k", "c6_duplicates", "c7_array_init",
              "c8_randomstate")


def kmeans_inputs(c):
    """(X (n, d) float64, KMeans keyword arguments) of a case; ``random_state="rs:<seed>"`` becomes a fresh
    ``np.random.RandomState(seed)`` and an array init is built here."""
    rng = np.random.default_rng(c["seed"])
    n, d, k = c["n"], c["d"], c["k"]
    if c["kind"] == "modes" or c["kind"] == "far_init":
        modes = rng.normal(0, 300, (k, d))
        x = modes[rng.integers(0, k, n)] + rng.normal(0, 40, (n, d))
    elif c["kind"] == "gauss":
        x = rng.normal(0, 100, (n, d))
    elif c["kind"] == "dups":
        # small integers and n = 32 rows: the mean, the centred rows and every distance are exact in float64, so a
        # duplicate is at distance exactly 0 and the later k-means++ picks are not decided by rounding noise
        distinct = rng.integers(-20, 21, (6, d)).astype(np.float64)
        x = distinct[np.concatenate([np.arange(6), rng.integers(0, 6, n - 6)])]
    else:
        raise ValueError(c["kind"])
    kw = dict(c["kwargs"])
    rs = kw.get("random_state")
    if isinstance(rs, str) and rs.startswith("rs:"):
        kw["random_state"] = np.random.RandomState(int(rs[3:]))
    if c["kind"] == "far_init":
        init = x[rng.choice(n, k, replace=False)].copy()
        init[k - 1] = 1e4
        kw["init"] = init
    return np.ascontiguousarray(x, dtype=np.float64), kw


# ---- the reference's own fit: ActiveLearningStrategy.__init__ on a cluster file (strategy.py:38-52) ----------------
CLUSTER_FILE_CASE = dict(seed=111, n=400, j=19, clusters=6, random_seed=1307, data_type="panoptic")


def cluster_file_contents(c=CLUSTER_FILE_CASE):
    """The SAL cluster file: JSON ``{guid: (4, J) pose}`` (rows x, y, z, confidence), pose modes plus noise."""
    rng = np.random.default_rng(c["seed"])
    modes = rng.normal(0, 300, (c["clusters"], 3, c["j"]))
    kp = modes[rng.integers(0, c["clusters"], c["n"])] + rng.normal(0, 40, (c["n"], 3, c["j"]))
    conf = np.ones((c["n"], 1, c["j"]))
    poses = np.concatenate([kp, conf], axis=1)
    return OrderedDict(("%d-%d" % (i % 4, i), poses[i].tolist()) for i in range(c["n"]))


def heldout_rows(x, seed=909, n=400):
    """Rows the fit has not seen: perturbed copies of the first fitted rows (for predict)."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(x[rng.integers(0, x.shape[0], n)] + rng.normal(0, 60, (n, x.shape[1])))


HELDOUT_CASE = "c2_k10"

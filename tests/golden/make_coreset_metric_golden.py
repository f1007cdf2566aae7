"""Generate tests/golden/coreset_metric.npz: the REAL reference's ``CoreSet(sal, al, root, metric=...)
.select_batch(N)`` (utils/coreset.py:13-95, sklearn ``pairwise_distances``) on the cases of coreset_metric_cases.py.

Run in the build container only (needs scikit-learn, scipy and the reference tree through oracle.ref_harness):

    python tests/golden/make_coreset_metric_golden.py

Per case: the picks (row indices), per greedy step the relative gap (top1 - top2) / top1 of the reference's
``min_distances`` at the moment of its arg-max, and -- for the two small shapes -- the final ``min_distances``.  No
feature table is stored.  A case in which any step's gap is below coreset_metric_cases.MIN_GAP is REFUSED (change the
seed, not the floor): a pick decided by less than that is not a property of the metric.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

import coreset_metric_cases as cmc  # noqa: E402
from coreset_metric_oracle import relative_gap  # noqa: E402
from oracle import ref_harness  # noqa: E402


def versions():
    import scipy
    import sklearn

    return json.dumps(dict(numpy=np.__version__, sklearn=sklearn.__version__, scipy=scipy.__version__))


def run_reference(ns, c):
    """The reference's select_batch with its update_distances watched: before every single-centre update,
    ``min_distances`` is the vector its np.argmax was just taken on."""
    sal, al = cmc.build(c)
    keys = list(sal.keys())
    with contextlib.redirect_stdout(io.StringIO()):  # (the constructor prints poses)
        cs = ns.coreset.CoreSet(sal, al, c["root"], metric=c["metric"])
        gaps = []
        orig = cs.update_distances

        def watched(cluster_centers, **kw):
            if cs.min_distances is not None and len(cluster_centers) == 1:
                gaps.append(relative_gap(cs.min_distances))
            return orig(cluster_centers, **kw)

        cs.update_distances = watched
        picked = cs.select_batch(c["select"])
    picks = np.array([keys.index(k) for k in picked], dtype=np.int64)
    assert len(gaps) == c["select"]
    return picks, np.array(gaps), np.asarray(cs.min_distances, dtype=np.float64).ravel()


def main():
    ns = ref_harness.load()
    out = {"versions": np.array(versions())}
    for name, c in cmc.coreset_metric_cases().items():
        picks, gaps, md = run_reference(ns, c)
        if not (gaps.min() >= cmc.MIN_GAP):
            raise SystemExit(f"{name}: relative gap {gaps.min():.3e} at step {int(gaps.argmin())} is below {cmc.MIN_GAP:g}: "
                             "change the case's seed")
        out[name + "/picks"] = picks
        out[name + "/gaps"] = gaps
        if c["shape"] in cmc.STORES_MIN_DISTANCES:
            out[name + "/min_distances"] = md
        print(f"{name}: picks[:5]={picks[:5].tolist()} smallest relative gap {gaps.min():.3e}")
    path = os.path.join(HERE, "coreset_metric.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

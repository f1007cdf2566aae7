"""Generate tests/golden/kmeans.npz: scikit-learn's KMeans on the cases of kmeans_cases.py, and the REAL
reference's ``ActiveLearningStrategy.__init__`` fit on a SAL cluster file.

Run in the build container only (needs scikit-learn, and /root/reference for the reference step):

    python tests/golden/make_kmeans_golden.py

Per case: centres, labels (uint8), inertia, n_iter and the k-means++ picks of every initialisation (recorded by
wrapping sklearn's ``_kmeans_plusplus`` during the fit; -1 rows for an array init).  Inputs are not stored:
kmeans_cases.py regenerates them with numpy's default_rng.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import kmeans_cases  # noqa: E402


def versions():
    import sklearn

    return json.dumps(dict(numpy=np.__version__, sklearn=sklearn.__version__))


def fit_sklearn(x, k, kw):
    """sklearn KMeans(k, **kw).fit(x) with every k-means++ initialisation's indices recorded."""
    import warnings

    from sklearn.cluster import KMeans
    from sklearn.cluster import _kmeans as skk

    picks = []
    orig = skk._kmeans_plusplus

    def recording(*a, **kwa):
        centers, indices = orig(*a, **kwa)
        picks.append(np.asarray(indices, dtype=np.int64).copy())
        return centers, indices

    skk._kmeans_plusplus = recording
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            km = KMeans(k, **kw).fit(x)
    finally:
        skk._kmeans_plusplus = orig
    if not picks:
        picks = [np.full(k, -1, dtype=np.int64)]
    warned = any("Number of distinct clusters" in str(m.message) for m in w)
    return km, np.stack(picks), warned


def gen_cases(out):
    for name, c in kmeans_cases.kmeans_cases().items():
        x, kw = kmeans_cases.kmeans_inputs(c)
        km, picks, warned = fit_sklearn(x, c["k"], kw)
        assert km.labels_.max() < 256
        out[name + "/centers"] = km.cluster_centers_
        out[name + "/labels"] = km.labels_.astype(np.uint8)
        out[name + "/inertia"] = np.float64(km.inertia_)
        out[name + "/n_iter"] = np.int64(km.n_iter_)
        out[name + "/init_idx"] = picks
        out[name + "/warned"] = np.int64(warned)
        if name == kmeans_cases.HELDOUT_CASE:
            out[name + "/heldout_predict"] = km.predict(kmeans_cases.heldout_rows(x)).astype(np.uint8)
        print(f"{name}: n_iter={km.n_iter_} inertia={km.inertia_:.6e} inits={len(picks)} warned={warned}")


def gen_reference_init(out):
    """[reference] the reference's ActiveLearningStrategy.__init__ with EXPR_TYPE="SAL" on a temporary cluster
    file: its ``self.kmeans`` centres and labels."""
    from oracle import ref_harness

    c = kmeans_cases.CLUSTER_FILE_CASE
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "clusters.json")
        with open(path, "w") as f:
            json.dump(kmeans_cases.cluster_file_contents(), f)
        st = ref_harness.make_strategy(
            "HP", EXPR_TYPE="SAL", RANDOM_SEED=c["random_seed"], **{"SAL.CLUSTER_FILE_PATH": path,
                                                                    "SAL.NUM_CLUSTERS": c["clusters"],
                                                                    "DATA.TYPE": c["data_type"]})
    out["reference_init/centers"] = st.kmeans.cluster_centers_
    out["reference_init/labels"] = st.kmeans.labels_.astype(np.uint8)
    print(f"reference_init: n_iter={st.kmeans.n_iter_} inertia={st.kmeans.inertia_:.6e}")


def main():
    out = {"versions": np.array(versions())}
    gen_cases(out)
    gen_reference_init(out)
    np.savez_compressed(os.path.join(HERE, "kmeans.npz"), **out)


if __name__ == "__main__":
    main()

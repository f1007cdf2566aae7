"""Device KMeans (csrc/kmeans.hip, utils/kmeans.py) against scikit-learn 1.7.2 and the reference's own SAL fit
(tests/golden/kmeans.npz, sal_filter.json).  Reads only committed goldens."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import cases
import kmeans_cases

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(G, "kmeans.npz")))


def _fit(name):
    from multi_view_active_learning_amd.utils.kmeans import KMeans

    c = kmeans_cases.kmeans_cases()[name]
    x, kw = kmeans_cases.kmeans_inputs(c)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        km = KMeans(c["k"], **kw).fit(x)
    return x, km, w


def _check_inertia(got, want, x, rel):
    floor = 1e-20 * x.shape[0] * float(np.abs(x).max()) ** 2  # (an all-duplicates fit has inertia ~1e-28)
    assert abs(got - want) <= rel * max(abs(want), floor), (got, want)


@pytest.mark.parametrize("name", kmeans_cases.STRUCTURED)
def test_structured_fit_matches_sklearn(dev, golden, name):
    x, km, w = _fit(name)
    np.testing.assert_array_equal(km.init_indices_, golden[name + "/init_idx"])
    np.testing.assert_array_equal(km.labels_, golden[name + "/labels"].astype(np.int32))
    assert km.labels_.dtype == np.int32
    assert km.n_iter_ == int(golden[name + "/n_iter"])
    assert km.cluster_centers_.dtype == np.float64
    np.testing.assert_allclose(km.cluster_centers_, golden[name + "/centers"], rtol=0, atol=1e-9 * np.abs(x).max())
    _check_inertia(km.inertia_, float(golden[name + "/inertia"]), x, 1e-10)
    warned = any("Number of distinct clusters" in str(m.message) for m in w)
    assert warned == bool(golden[name + "/warned"])


def test_duplicates_warn_like_sklearn(dev):
    from multi_view_active_learning_amd.utils.kmeans import ConvergenceWarning

    _, km, w = _fit("c6_duplicates")
    msgs = [m for m in w if issubclass(m.category, ConvergenceWarning)]
    assert len(msgs) == 1
    assert str(msgs[0].message) == ("Number of distinct clusters (6) found smaller than n_clusters (8). "
                                    "Possibly due to duplicate points in X.")


def test_unstructured_fit_matches_sklearn_inertia(dev, golden):
    """Unstructured Gaussian rows: Voronoi near-ties make labels order-sensitive; seeding and the objective agree."""
    name = "c5_gauss_50k"
    x, km, _ = _fit(name)
    np.testing.assert_array_equal(km.init_indices_, golden[name + "/init_idx"])
    _check_inertia(km.inertia_, float(golden[name + "/inertia"]), x, 1e-6)


def test_fit_is_bit_reproducible_and_accepts_device_tensors(dev):
    from multi_view_active_learning_amd.utils.kmeans import KMeans

    x, kw = kmeans_cases.kmeans_inputs(kmeans_cases.kmeans_cases()["c5_gauss_50k"])
    a = KMeans(10, random_state=5, max_iter=40).fit(x)
    b = KMeans(10, random_state=5, max_iter=40).fit(torch.from_numpy(x).to(dev))
    assert a.cluster_centers_.tobytes() == b.cluster_centers_.tobytes()
    np.testing.assert_array_equal(a.labels_, b.labels_)
    assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_


def test_predict_matches_nearest_center_and_sklearn(dev, golden):
    from multi_view_active_learning_amd import _lib

    name = kmeans_cases.HELDOUT_CASE
    x, km, _ = _fit(name)
    held = kmeans_cases.heldout_rows(x)
    got = km.predict(held)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, golden[name + "/heldout_predict"].astype(np.int32))
    direct = _lib.nearest_center(torch.from_numpy(held).to(dev), torch.from_numpy(km.cluster_centers_).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, direct)
    np.testing.assert_array_equal(km.predict(torch.from_numpy(held).to(dev)), got)
    np.testing.assert_array_equal(km.fit_predict(x), km.labels_)


def _sal_features(sal):
    feats = []
    for g in sal["pred_3d_keypoints"]:
        kp = np.array(sal["pred_3d_keypoints"][g]).T
        feats.append((kp[0:3, :] - kp[0:3, 2:3]).flatten())
    return np.asarray(feats)


@pytest.mark.parametrize("name", [n for n, c in cases.sal_filter_cases().items() if c["use_clusters"]])
def test_sal_filter_centres_fitted_on_device(dev, name):
    """The centres of sal_filter.json (sklearn KMeans(K, n_init=3, random_state=seed) in the generator) are
    reproduced on the device, and the pseudo-label filter fed with the fitted KMeans picks the golden guids."""
    import random

    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils.kmeans import KMeans

    with open(os.path.join(G, "sal_filter.json")) as f:
        want = json.load(f)[name]
    c = cases.sal_filter_cases()[name]
    sal, done = cases.sal_filter_inputs(c)
    feats = _sal_features(sal)
    km = KMeans(c["clusters"], n_init=3, random_state=c["seed"]).fit(feats)
    np.testing.assert_allclose(km.cluster_centers_, np.asarray(want["centers"]), rtol=0, atol=1e-9 * np.abs(feats).max())
    cfg = get_default_configs()
    cfg.AL.STRATEGY = "HP"
    cfg.SAL.INLIER_THRESHOLD = c["thr"]
    cfg.SAL.NUM_CLUSTERS = c["clusters"]
    st = ActiveLearningStrategy(cfg)
    al = st.select_al_guids(sal, c["al_num"])
    random.seed(c["seed"])
    assert st.select_sal_guids(sal, al, done, c["pseudo_num"], km, device=dev) == want["sal_guids"]
    assert st.select_sal_guids(sal, al, done, c["pseudo_num"], km.cluster_centers_, device=dev) == want["sal_guids"]


def test_strategy_kmeans_equals_reference_init(dev, golden, tmp_path):
    """ActiveLearningStrategy(cfg).kmeans on a SAL cluster file == the reference __init__'s self.kmeans."""
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    c = kmeans_cases.CLUSTER_FILE_CASE
    path = tmp_path / "clusters.json"
    path.write_text(json.dumps(kmeans_cases.cluster_file_contents()))
    cfg = get_default_configs()
    cfg.EXPR_TYPE = "SAL"
    cfg.RANDOM_SEED = c["random_seed"]
    cfg.DATA.TYPE = c["data_type"]
    cfg.SAL.NUM_CLUSTERS = c["clusters"]
    cfg.SAL.CLUSTER_FILE_PATH = str(path)
    st = ActiveLearningStrategy(cfg)
    assert "_kmeans" not in st.__dict__  # __init__ does no new work
    km = st.kmeans
    assert st.kmeans is km
    want = golden["reference_init/centers"]
    np.testing.assert_allclose(km.cluster_centers_, want, rtol=0, atol=1e-9 * np.abs(want).max())
    np.testing.assert_array_equal(km.labels_, golden["reference_init/labels"].astype(np.int32))


def test_device_errors(dev):
    from multi_view_active_learning_amd.utils.kmeans import KMeans

    x = torch.randn(20, 6, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="n_samples=20 should be >= n_clusters=21"):
        KMeans(21).fit(x)
    bad = x.clone()
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        KMeans(3).fit(bad)
    with pytest.raises(NotImplementedError):
        KMeans(3).fit(x, sample_weight=np.ones(20))

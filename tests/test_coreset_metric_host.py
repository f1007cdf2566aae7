"""CPU (no GPU): core-set selection under the l1, cosine and Chebyshev metrics -- the numpy restatement
(coreset_metric_oracle.py) against the REAL reference's results (golden/coreset_metric.npz), the C-ABI's new entry and
constants, and the accepted metric names.

Bounds.  l1 and Chebyshev: the restatement's feature-order loop IS what scipy's cdist computes, so ``min_distances`` are
compared for bit equality.  Cosine: sklearn takes the dot products with BLAS, whose summation order is not the
restatement's; distances lie in [0, 2], a dot product of unit rows has D <= 126 terms of magnitude <= 1, so two
evaluations differ by at most gamma_D ~ 126 * 1.1e-16 = 1.4e-14, the two normalisations (a few ulp each) bring that
under 3e-14, and the bound used is 1e-13 absolute -- under four times that.  Picks are compared for equality under every
metric: the generator refuses a case whose top two ``min_distances`` are closer than 1e-9 (relative) at any step."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import coreset_metric_cases as cmc
import coreset_metric_oracle as cmo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
COSINE_ATOL = 1e-13


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "coreset_metric.npz"))


@pytest.fixture(scope="module")
def lib():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("name", list(cmc.coreset_metric_cases()))
def test_restatement_vs_reference_golden(golden, name):
    c = cmc.coreset_metric_cases()[name]
    pool, lab = cmc.arrays(c)
    feat = cmo.stacked_features(pool, lab, c["root"])
    picks, md, gaps = cmo.kcenter_greedy(feat, range(c["n"], c["n"] + c["l"]), c["select"], c["metric"])
    assert golden[name + "/gaps"].min() >= cmc.MIN_GAP
    assert picks == golden[name + "/picks"].tolist()
    if c["shape"] in cmc.STORES_MIN_DISTANCES:
        want = golden[name + "/min_distances"]
        if cmo.ALIASES[c["metric"]] == "cosine":
            assert np.abs(md - want).max() <= COSINE_ATOL
        else:
            np.testing.assert_array_equal(md, want)
    else:
        assert name + "/min_distances" not in golden


@pytest.mark.parametrize("alias", list(cmc.ALIAS_OF))
def test_alias_cases_equal_manhattan(golden, alias):
    a, b = alias + "/" + cmc.ALIAS_SHAPE, cmc.ALIAS_OF[alias] + "/" + cmc.ALIAS_SHAPE
    for f in ("picks", "gaps", "min_distances"):
        np.testing.assert_array_equal(golden[a + "/" + f], golden[b + "/" + f])


def test_golden_is_small_and_complete(golden):
    assert os.path.getsize(os.path.join(G, "coreset_metric.npz")) < 1 << 20
    for name, c in cmc.coreset_metric_cases().items():
        assert golden[name + "/picks"].shape == (c["select"],) and golden[name + "/gaps"].shape == (c["select"],)
    v = json.loads(str(golden["versions"]))
    assert v["sklearn"] and v["scipy"] and v["numpy"]


def test_restatement_small_properties():
    """What the device tests rely on, checked on the restatement itself: a zero row is at cosine distance exactly 1 from
    every row; rows that are power-of-two multiples normalise to the same bits; identical rows tie at every step."""
    rng = np.random.default_rng(0)
    f = rng.standard_normal((20, 9)) * 300.0
    f[3] = 0.0
    f[7] = f[5] * 4.0
    f[8] = f[5] * 0.125
    t = cmo.prepare(f, "cosine")
    np.testing.assert_array_equal(t[5], t[7])
    np.testing.assert_array_equal(t[5], t[8])
    np.testing.assert_array_equal(t[3], np.zeros(9))
    d = cmo.distances(t, range(20), "cosine")
    assert (d[3] == 1.0).all() and (d[:, 3] == 1.0).all()
    np.testing.assert_array_equal(d[:, 5], d[:, 7])
    same = np.repeat(rng.standard_normal((1, 9)) * 300.0, 12, axis=0)
    for m in ("manhattan", "cosine", "chebyshev"):
        assert cmo.kcenter_greedy(same, [10, 11], 5, m)[0] == [0] * 5


def test_header_and_library_export_the_metric_entry(lib):
    hdr = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    assert re.search(r"\bint\s+mval_kcenter_select_metric\s*\(\s*int\s+metric\b", hdr)
    assert hasattr(lib, "mval_kcenter_select_metric") and hasattr(lib, "mval_kcenter_select")
    assert hasattr(lib, "mval_kcenter_workspace_bytes")


def test_metric_constants_are_mirrored():
    from multi_view_active_learning_amd import _lib

    hdr = open(os.path.join(REPO, "include", "mval_hip.h")).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))

    ids = [define("MVAL_KC_" + n) for n in ("EUCLIDEAN", "L1", "COSINE", "CHEBYSHEV")]
    assert ids == [_lib.KC_EUCLIDEAN, _lib.KC_L1, _lib.KC_COSINE, _lib.KC_CHEBYSHEV]
    assert len(set(ids)) == 4


def test_accepted_names_map_aliases_to_one_id():
    from multi_view_active_learning_amd import _lib

    want = {"euclidean": _lib.KC_EUCLIDEAN, "l2": _lib.KC_EUCLIDEAN, "manhattan": _lib.KC_L1, "l1": _lib.KC_L1,
            "cityblock": _lib.KC_L1, "cosine": _lib.KC_COSINE, "chebyshev": _lib.KC_CHEBYSHEV}
    assert _lib.KC_METRIC_IDS == want
    for name, mid in want.items():
        assert _lib.kcenter_metric_id(name) == mid
    assert set(cmo.ALIASES) == set(want)  # the restatement knows the same names


@pytest.mark.parametrize("bad", ["minkowski", "Cosine", "", "linf", None, 2])
def test_unknown_metric_name_raises_before_any_device_work(bad):
    """NotImplementedError naming the accepted names -- from the constructor, from_tensors and the binding, before any
    of them touches the device (this test runs without one)."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.coreset import CoreSet

    pose = np.zeros((2, 3, 3))
    for call in (lambda: CoreSet({0: pose[0]}, {1: pose[1]}, 0, metric=bad),
                 lambda: CoreSet.from_tensors(pose, pose, 0, metric=bad),
                 lambda: _lib.kcenter_select(None, None, 1, metric=bad)):
        with pytest.raises(NotImplementedError) as e:
            call()
        for name in ("euclidean", "l2", "manhattan", "l1", "cityblock", "cosine", "chebyshev"):
            assert repr(name) in str(e.value)


def test_unknown_metric_id_fails_with_a_message(lib):
    """The C entry checks the id before anything else: no pointer is read (all NULL here), rc != 0 and a message."""
    null = ctypes.c_void_p(0)
    lib.mval_last_error.restype = ctypes.c_char_p
    for bad in (4, -1, 99):
        rc = lib.mval_kcenter_select_metric(ctypes.c_int(bad), null, ctypes.c_longlong(8), ctypes.c_int(3), null, ctypes.c_longlong(0),
                                            ctypes.c_int(0), ctypes.c_int(0), null, null, null, null, null)
        assert rc != 0
        msg = lib.mval_last_error().decode()
        assert "unknown metric id %d" % bad in msg and "mval_kcenter_select_metric" in msg


def test_default_config_keeps_the_euclidean_metric():
    from multi_view_active_learning_amd.config import get_default_configs

    cfg = get_default_configs()
    assert cfg.AL.CORESET_METRIC == "euclidean"
    cfg.merge_from_list(["AL.CORESET_METRIC", "cosine"])
    assert cfg.AL.CORESET_METRIC == "cosine"

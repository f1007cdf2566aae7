"""Host tests (no GPU) of the confidence-weighted triangulation: the float64 oracle (weighted_tri_oracle.py)
against the real reference's results at unit weights, the input conditions of every generated case (weighted_tri_cases.py) --
asserted here, on the CPU, so a device mismatch in test_gpu_weighted_tri.py cannot be blamed on a knife-edge decision --, the
oracle's own properties (tie-break, accuracy), the config validator, the ValueError paths and the new symbol."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cases
import view_joint_mask_cases as vjc
import weighted_tri_cases as wc
import weighted_tri_oracle as wo
from weighted_tri_oracle import oracle_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
MARGIN = 1e-3  # px: every vote's |e - eps|
S_GAP = 1e-9  # relative: two ranking sums of different sets among the top count
SIGMA_RATIO = 2.9e3  # sigma_1 / (sigma_3 - sigma_4) of a final system: the worst the existing goldens record

def test_oracle_reproduces_the_reference_at_unit_weights():
    """triangulation_synth.npz and view_joint_mask.npz are the real reference's results.  With all-ones weights (and with none)
    the oracle gives them under the tolerances the GPU tests hold the device to against the same files: points 1e-6 mm
    (+ 1e-9 relative on the synth file, as test_gpu_hotpath.py), errors and metric 1e-9 relative, counts exact."""
    z = np.load(os.path.join(G, "triangulation_synth.npz"))
    for name, c in cases.triangulation_cases().items():
        proj = np.stack([cases.synth.ring_cameras(c["v"], c["h"], c["w"], seed=c["seed"] + 100 * i) for i in range(c["b"])])
        valid = np.ones((c["b"], c["j"]), dtype=bool)
        valid[:, list(c["invalid"])] = False
        kp = z[name + "/keypoints_2d"]
        for w in (None, np.ones(kp.shape[:3], dtype=np.float32)):
            r = wo.triangulate(kp, proj, 5.0, valid, weights=w)
            np.testing.assert_array_equal(r["inlier_count"], z[name + "/inlier_count"])
            np.testing.assert_allclose(r["keypoints_3d"], z[name + "/keypoints_3d"], rtol=1e-9, atol=1e-6)
            np.testing.assert_allclose(r["metric"], z[name + "/metric"], rtol=1e-9)
    for name, c in vjc.view_joint_mask_cases().items():
        g = vjc.load_golden(os.path.join(G, "view_joint_mask.npz"), name)
        proj = np.stack([cases.synth.ring_cameras(c["v"], c["h"], c["w"], seed=c["seed"] + 100 * i) for i in range(c["b"])])
        mask, valid, kp = vjc.view_joint_valid(c), vjc.valid_joints(c), g["keypoints_2d"]
        pairs = g["pairs"] if c["v"] > 11 else None
        for w in (None, np.ones(kp.shape[:3], dtype=np.float32)):
            r = wo.triangulate(kp, proj, vjc.EPS, valid, pairs, view_joint_valid=mask, weights=w)
            np.testing.assert_array_equal(r["joint_inliers"], g["joint_inliers"])
            np.testing.assert_array_equal(r["inlier_count"], g["inlier_count"])
            np.testing.assert_array_equal(r["joint_used"], vjc.used(c))
            np.testing.assert_allclose(r["keypoints_3d"], g["keypoints_3d"], rtol=0, atol=1e-6)
            np.testing.assert_allclose(r["joint_error"], g["joint_error"], rtol=1e-9)
            np.testing.assert_allclose(r["metric"], g["metric"], rtol=1e-9)


def check_conditions(r):
    """The three input conditions on an oracle result -> (min margin, min relative S gap, max sigma ratio)."""
    margin, gap, ratio = np.inf, np.inf, 0.0
    for p in r["problems"].values():
        if not p["used"]:
            continue
        ratio = max(ratio, p["sigma_ratio"])
        hyps = p["hypotheses"]
        if not hyps:
            continue
        margin = min(margin, min(h["margin"] for h in hyps))
        top = [h for h in hyps if h["count"] == max(h["count"] for h in hyps)]
        if top[0]["S"] is None:
            continue
        for i, a in enumerate(top):
            for b in top[i + 1:]:
                if a["views"] != b["views"]:
                    gap = min(gap, abs(a["S"] - b["S"]) / max(a["S"], b["S"]))
    return margin, gap, ratio


@pytest.mark.parametrize("name", list(wc.weighted_tri_cases()))
def test_generated_cases_meet_the_input_conditions(name):
    """Every vote at least 1e-3 px off eps; among the hypotheses with the top count two ranking sums are from identical sets or
    differ by more than 1e-9 relative; every weighted final system no worse conditioned than 2.9e3.  Weighted and unweighted
    (the unweighted run is the baseline of the comparisons below and of the GPU tests)."""
    kind = wc.weighted_tri_cases()[name]["kind"]
    for weighted in (True, False) if kind != "unusable" else (True,):  # (``unusable``: key-points that only the weights keep out)
        margin, gap, ratio = check_conditions(oracle_of(name, weighted))
        print(name, "weighted" if weighted else "unweighted", "margin %.3g px, S gap %.3g, sigma ratio %.3g" % (margin, gap, ratio))
        assert margin >= MARGIN and gap > S_GAP and ratio <= SIGMA_RATIO, (name, weighted, margin, gap, ratio)
    d = wc.build(wc.weighted_tri_cases()[name])
    w = d["weights"][np.isfinite(d["weights"]) & (d["weights"] > 0)]
    if wc.weighted_tri_cases()[name]["kind"] == "random" and wc.weighted_tri_cases()[name]["low"] > 0:
        assert w.min() < 1e-2 and w.max() > 0.9  # the weights span 1e-3 .. 1
    assert d["kp2d"].dtype == np.float32 and d["weights"].dtype == np.float32


def test_tie_break_changes_the_winning_pair():
    """Case ``tie``, joint 0: six hypotheses of two inliers each.  Unweighted, position 0 (views 0, 1) wins; weighted, the
    heaviest set {2, 3} at position 5 -- another pair, another point."""
    plain, weighted = oracle_of("tie", False).get("problems")[0, 0], oracle_of("tie").get("problems")[0, 0]
    assert [h["count"] for h in weighted["hypotheses"]] == [2] * 6
    assert (plain["position"], plain["mask"]) == (0, 0b0011) and (weighted["position"], weighted["mask"]) == (5, 0b1100)
    assert np.linalg.norm(plain["point"] - weighted["point"]) > 100.0
    # another joint of the case, whose sets do not tie, keeps its winner
    assert oracle_of("tie", False)["problems"][0, 1]["mask"] == oracle_of("tie")["problems"][0, 1]["mask"]


def test_unusable_weights_leave_joints_unused():
    r = oracle_of("unusable")
    assert r["joint_used"].tolist() == [[False, True, False], [False, False, False], [False, False, False]]
    assert r["inlier_count"].tolist()[1:] == [-2, -2] and np.isnan(r["metric"][1:]).all() and r["inlier_count"][0] >= 2
    assert not r["keypoints_3d"][0, 0].any() and r["joint_inlier_mask"][0, 0] == 0


def test_weights_lower_the_error_of_the_noisy_view_case():
    """Accuracy claim (CPU oracle): 4 views, sigma 0.7 px in three and 4 px in the fourth, weights 0.7 / sigma;
    the mean 3-D error with weights is below the one without, and single points move by more than 1 mm."""
    d = wc.build(wc.weighted_tri_cases()["noisy4"])
    plain, weighted = oracle_of("noisy4", False), oracle_of("noisy4")
    e_plain = np.linalg.norm(plain["keypoints_3d"] - d["gt"], axis=-1).mean()
    e_weighted = np.linalg.norm(weighted["keypoints_3d"] - d["gt"], axis=-1).mean()
    print("noisy4: mean 3-D error %.3f mm unweighted, %.3f mm weighted" % (e_plain, e_weighted))
    assert e_weighted < e_plain
    assert np.linalg.norm(plain["keypoints_3d"] - weighted["keypoints_3d"], axis=-1).max() > 1.0


def test_check_triangulation_weights_and_the_config_fields():
    from multi_view_active_learning_amd.config import check_triangulation_weights, get_default_configs

    cfg = get_default_configs()
    assert cfg.AL.TRIANGULATION_WEIGHTS == cfg.EVAL.TRIANGULATION_WEIGHTS == "none"
    assert check_triangulation_weights("none") == check_triangulation_weights(None) == "none"
    assert check_triangulation_weights("conf", "taylor") == check_triangulation_weights("conf", "quarter") == "conf"
    t = torch.ones((1, 2, 3))
    assert check_triangulation_weights(t) is t and check_triangulation_weights(t, "taylor") is t
    with pytest.raises(ValueError, match="decode refinement"):
        check_triangulation_weights("conf")
    for bad in ("peak", "", 1.0, [1.0], True):
        with pytest.raises(ValueError, match="'none', 'conf'"):
            check_triangulation_weights(bad, "taylor")
    cfg.merge_from_list(["AL.TRIANGULATION_WEIGHTS", "conf", "EVAL.TRIANGULATION_WEIGHTS", "conf"])
    assert cfg.AL.TRIANGULATION_WEIGHTS == cfg.EVAL.TRIANGULATION_WEIGHTS == "conf"


def test_wrappers_take_the_new_arguments():
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils import triangulation

    for fn in (triangulation.triangulate_batch, triangulation.triangulation):
        params = inspect.signature(fn).parameters
        assert params["weights"].default is None and params["return_inlier_mask"].default is False
    params = inspect.signature(_lib.triangulate_ransac_weighted).parameters
    assert list(params)[:7] == ["kp2d", "proj", "valid", "b", "v", "j", "eps"]
    for kw in ("pairs", "view_valid", "view_joint_valid", "weights", "want_inlier_mask"):
        assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY, kw


def test_value_errors_come_before_any_device_work():
    """The new argument is checked before the heat-maps are looked at (None stands in for them)."""
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch, triangulation

    with pytest.raises(ValueError, match="decode refinement"):
        triangulate_batch(None, None, 4, None, weights="conf")
    with pytest.raises(ValueError, match="'none', 'conf'"):
        triangulate_batch(None, None, 4, None, weights="peak", refine="taylor")
    with pytest.raises(ValueError, match="'none', 'conf'"):
        triangulate_batch(None, None, 4, None, weights=0.5)
    with pytest.raises(ValueError, match="decode refinement"):
        triangulation(torch.zeros((2, 3, 4, 4)), torch.zeros((2, 3, 4)), 4, torch.ones(3), weights="conf")


def test_strategy_reads_the_fields_with_the_guard():
    """AL.TRIANGULATION_WEIGHTS "conf" without AL.DECODE_REFINE is refused before the batch is looked at; both fields
    are read with the ``in`` guard of the other opt-in fields (a config without them reads as "none")."""
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    cfg = get_default_configs()
    cfg.AL.TRIANGULATION_WEIGHTS = "conf"
    with pytest.raises(ValueError, match="decode refinement"):
        ActiveLearningStrategy(cfg)._score_columns(torch.zeros((2, 3, 4, 4)), {}, ("TRIANGULATION",))
    cfg.AL.TRIANGULATION_WEIGHTS = "none"
    cfg.EVAL.TRIANGULATION_WEIGHTS = "conf"
    with pytest.raises(ValueError, match="decode refinement"):
        ActiveLearningStrategy(cfg).evaluate_mkpe([], None)
    cfg.EVAL.TRIANGULATION_WEIGHTS = "sharp"
    with pytest.raises(ValueError, match="'none', 'conf'"):
        ActiveLearningStrategy(cfg).evaluate_mkpe([], None)
    src = inspect.getsource(ActiveLearningStrategy)
    assert src.count('"TRIANGULATION_WEIGHTS" in cfg.AL') == 1 and src.count('"TRIANGULATION_WEIGHTS" in ev') == 1


def test_new_entry_is_declared_and_exported():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    n = "mval_triangulate_ransac_weighted"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mval_hip.h")).read(), flags=re.S)
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr)
    assert decl is not None, n + " is not declared in include/mval_hip.h"
    assert hasattr(_lib.lib(), n), n + " is not exported"
    f = _lib._views_entry(n)
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert f.restype is ctypes.c_int and len(f.argtypes) == len(args) == 21
    # the `_pairs_masked` entry's arguments plus the weights and the set, where the issue puts them
    masked = [" ".join(a.split()) for a in re.search(r"\bmval_triangulate_ransac_pairs_masked\s*\(([^)]*)\)", hdr).group(1).split(",")]
    assert [a for a in args if a not in ("const float* weights", "int32_t* joint_inlier_mask")] == masked
    assert args.index("const float* weights") == 9 and args.index("int32_t* joint_inlier_mask") == 13

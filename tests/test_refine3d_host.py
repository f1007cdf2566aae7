"""Host tests (no GPU) of the 3-D refinement: the new entry in the header and the library and its argument
checks, the four config fields and their validator, the float64 oracle of tests/refine3d_oracle.py against the goldens
(tests/golden/refine3d.npz: the long-double minimum of every problem), and where ``triangulate_batch`` and the scoring and
evaluation passes reach the refinement -- never under the default configuration."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import refine3d_cases as rc  # noqa: E402
import refine3d_oracle as ro  # noqa: E402

CASES = rc.refine3d_cases()
KINDS = ("i64", "f32")


@pytest.fixture(scope="module")
def golden():
    return rc.load_golden()


# ---- the entry -------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_and_exported():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    text = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+mval_refine_points_3d\s*\(([^)]*)\)", hdr)
    assert decl, "mval_refine_points_3d is not declared in include/mval_hip.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["const void* kp2d", "int kp_is_f32", "const double* proj", "const uint8_t* valid", "const uint8_t* mask", "int mask_kind",
                    "const float* weights", "const double* kp3d", "const double* joint_err", "const int32_t* joint_inliers",
                    "double* kp3d_out", "double* joint_err_out", "int32_t* joint_support", "int32_t* joint_status", "double* metric",
                    "int32_t* inlier_count", "int B", "int V", "int J", "double eps", "void* stream"]
    assert hasattr(_lib.lib(), "mval_refine_points_3d"), "mval_refine_points_3d is not exported"
    assert len(_lib._VIEWS_ARGTYPES["mval_refine_points_3d"]) == len(args)
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))  # noqa: E731
    assert (_lib.MASK_NONE, _lib.MASK_VIEWS, _lib.MASK_VIEW_JOINT) == (define("MVAL_MASK_NONE"), define("MVAL_MASK_VIEWS"), define("MVAL_MASK_VIEW_JOINT")) == (0, 1, 2)
    assert _lib.REFINE3D_MAX_ITERS == define("MVAL_REFINE3D_MAX_ITERS") == ro.MAX_ITERS == 32


def test_entry_rejects_bad_arguments_without_a_launch():
    """V outside 2..32, bad dimensions, a mask kind outside 0..2 or not matching the mask pointer, NULL and misaligned arrays are
    errors before anything touches a device; B = 0 returns 0."""
    import ctypes as C

    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    f = _lib._views_entry("mval_refine_points_3d")
    p = lambda a: C.c_void_p(a)  # noqa: E731  (never dereferenced: every call below fails its checks or is the B = 0 no-op)

    def call(b=1, v=4, j=5, mask=0, kind=0, weights=0, ptr=0x1000, kp3d_out=0x2000, jerr_out=0x3000, kp=0x4000, f32=0):
        return f(p(kp), f32, p(ptr), p(0), p(mask), kind, p(weights), p(ptr), p(ptr), p(ptr), p(kp3d_out), p(jerr_out), p(ptr), p(ptr), p(ptr),
                 p(ptr), b, v, j, 5.0, p(0))

    assert call(b=0) == 0
    bad = (dict(v=1), dict(v=33), dict(j=0), dict(j=513), dict(b=-1), dict(kind=3), dict(kind=-1), dict(kind=1), dict(kind=2),
           dict(mask=0x5000), dict(ptr=0), dict(kp3d_out=0), dict(jerr_out=0), dict(kp=0), dict(kp3d_out=0x1000), dict(jerr_out=0x1000),
           dict(kp3d_out=0x2004), dict(jerr_out=0x3004), dict(ptr=0x1004), dict(kp=0x4004), dict(kp=0x4002, f32=1), dict(weights=0x6002))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"mval_refine_points_3d" in _lib.lib().mval_last_error()


def test_check_refine_3d():
    from multi_view_active_learning_amd.config import REFINE_3D_WEIGHTS, REFINE_3DS, check_refine_3d, get_default_configs

    cfg = get_default_configs()
    assert cfg.AL.REFINE_3D == cfg.EVAL.REFINE_3D == cfg.AL.REFINE_3D_WEIGHTS == cfg.EVAL.REFINE_3D_WEIGHTS == "none"
    assert REFINE_3DS == ("none", "lm") and REFINE_3D_WEIGHTS == ("none", "conf")
    assert check_refine_3d("none") == ("none", "none") == check_refine_3d("none", None)
    assert check_refine_3d("lm") == ("lm", "none") == check_refine_3d("lm", None) == check_refine_3d("lm", "none", "taylor")
    for decode in ("quarter", "taylor"):
        assert check_refine_3d("lm", "conf", decode) == ("lm", "conf")
    w = torch.ones(1, 2, 3)
    assert check_refine_3d("lm", w)[1] is w
    for bad in ("", "LM", "huber", "direct_optimization", None, 1, True):
        with pytest.raises(ValueError, match="'none', 'lm'"):
            check_refine_3d(bad)
    for bad in ("", "CONF", "huber", 1, True):
        with pytest.raises(ValueError, match="'none', 'conf'"):
            check_refine_3d("lm", bad)
    with pytest.raises(ValueError, match="decode refinement"):
        check_refine_3d("lm", "conf")
    with pytest.raises(ValueError, match="decode refinement"):
        check_refine_3d("lm", "conf", "none")
    for weights in ("conf", w):
        with pytest.raises(ValueError, match="without a 3-D refinement"):
            check_refine_3d("none", weights, "taylor")


# ---- the oracle against the goldens ---------------------------------------------------------------------------------------------
def test_golden_records_its_platform(golden):
    assert str(golden["meta/numpy_version"])
    bits, nmant, precision = golden["meta/longdouble"]
    assert nmant >= 63 and float(golden["meta/longdouble_eps"]) < 2e-19  # the minimum was computed wider than float64
    tol = rc.tolerances(golden)
    assert sorted(tol) == [2, 3, 4, 8, 12, 32]
    assert all(0 < t < 1e-4 for t in tol.values()), tol  # mm: the float64 floor of these rigs, DESIGN.md 6.5


def _oracle(golden, name, kind):
    d = rc.build(CASES[name])
    g = lambda key: golden[f"{name}/{kind}/{key}"]  # noqa: E731
    np.testing.assert_array_equal(d["kp_" + kind], g("kp"))  # the seeded inputs are the stored ones (NaN == NaN here)
    np.testing.assert_array_equal(d["proj"], golden[f"{name}/proj"])
    return d, g, ro.refine_batch(g("kp"), d["proj"], g("x0"), g("err0"), rc.EPS, d["valid"], d["view_valid"], d["view_joint_valid"], d["weights"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_against_the_long_double_minimum(golden, name, kind):
    c = CASES[name]
    d, g, r = _oracle(golden, name, kind)
    np.testing.assert_array_equal(r["support"], g("support"))
    np.testing.assert_array_equal(r["joint_support"], g("support").sum(axis=1))
    refined = r["joint_status"] != 0
    np.testing.assert_array_equal(refined, g("status") != 0)
    np.testing.assert_array_equal(refined, d["valid"] & (g("support").sum(axis=1) >= 2))
    assert (r["joint_status"][refined] > 0).all()  # every one of them converges below the cap
    assert r["joint_status"].max(initial=0) <= ro.MAX_ITERS
    # not refined: X0 and its error bit for bit, status 0
    assert r["keypoints_3d"][~refined].tobytes() == g("x0")[~refined].tobytes()
    assert r["joint_error"][~refined].tobytes() == g("err0")[~refined].tobytes()
    assert not g("x0")[~d["valid"]].any() and not r["joint_support"][~d["valid"]].any()
    if refined.any():
        tol = rc.tolerances(golden)[c["v"]]
        gap = np.linalg.norm(r["keypoints_3d"] - g("xmin"), axis=-1)[refined]
        print(f"{name}/{kind}: {refined.sum()} refined, iterations {r['joint_status'][refined].min()}..{r['joint_status'][refined].max()}, "
              f"gap to the long-double minimum max {gap.max():.2e} mm, tolerance {tol:.2e} mm")
        assert gap.max() <= tol
        np.testing.assert_allclose(gap, g("gap_oracle")[refined], rtol=0, atol=tol)
        # descent, and the recomputed joint error is the mean half-distance over S at the refined point
        for bi, ji in zip(*np.nonzero(refined)):
            S = np.flatnonzero(g("support")[bi, :, ji])
            w = np.ones(len(S)) if d["weights"] is None else d["weights"][bi, S, ji]
            pts = g("kp")[bi, S, ji].astype(np.float64)
            assert ro.cost(d["proj"][bi, S], pts, w, r["keypoints_3d"][bi, ji]) <= ro.cost(d["proj"][bi, S], pts, w, g("x0")[bi, ji]) * (1 + 1e-12)
            want = np.mean([ro.half_distance(d["proj"][bi, v], r["keypoints_3d"][bi, ji], g("kp")[bi, v, ji].astype(np.float64)) for v in S])
            assert r["joint_error"][bi, ji] == pytest.approx(want, rel=1e-12)


def test_cases_cover_what_they_are_for(golden):
    """The moved view is in nobody's support set, masks and weights take views out, and some problems are left unrefined for each
    of the three reasons (invalid, fewer than two views in S, fewer than two present)."""
    for kind in KINDS:
        for name in ("v4", "v8", "v12", "v32", "v8_view_joint"):
            sup = golden[f"{name}/{kind}/support"]
            for bi in range(sup.shape[0]):
                assert not sup[bi, bi % sup.shape[1]].any() and sup[bi].any()
        assert not golden[f"v2_split/{kind}/status"].any() and (golden[f"v2_split/{kind}/inliers0"] == 2).all()
        assert (golden[f"v2_split/{kind}/support"].sum(axis=1) < 2).all()
        d = rc.build(CASES["v4_weighted"])
        sup, st = golden[f"v4_weighted/{kind}/support"], golden[f"v4_weighted/{kind}/status"]
        assert not sup[~(np.isfinite(d["weights"]) & (d["weights"] > 0))].any()
        assert st[0, 4] == 0 and sup[0, :, 4].sum() == 1 and d["valid"][0, 4]
        d = rc.build(CASES["v4_views"])
        assert not golden[f"v4_views/{kind}/support"][~d["view_valid"]].any() and np.isnan(d["proj"][~d["view_valid"]]).all()
        d = rc.build(CASES["v8_view_joint"])
        assert not golden[f"v8_view_joint/{kind}/support"][~d["view_joint_valid"]].any()
        assert golden[f"v8_view_joint/{kind}/status"][1, 2] == 0 and golden[f"v8_view_joint/{kind}/inliers0"][1, 2] == 0
        assert np.isnan(d["kp_f32"][~d["view_joint_valid"]]).all()


def test_oracle_beats_the_dlt_on_the_unequal_radius_rig():
    """Cameras at 1500 / 3000 / 4500 / 6000 mm, 300 problems, grid-snapped points: the oracle's mean error to the
    true joints is 12.05 mm against the DLT's 17.05 mm -- the inequality the GPU test asserts holds on the host with a clear
    margin for the seed it uses."""
    from oracle import geometry

    proj, joints, kp = rc.accuracy_rig()
    b, v, j = kp.shape[:3]
    x0, err0 = np.zeros((b, j, 3)), np.zeros((b, j))
    for bi in range(b):
        for ji in range(j):
            x0[bi, ji], err0[bi, ji], _ = geometry.triangulate_ransac(proj[bi], kp[bi, :, ji].astype(np.float64), 64, rc.EPS)
    r = ro.refine_batch(kp, proj, x0, err0, rc.EPS)
    dlt, lm = np.linalg.norm(x0 - joints, axis=-1), np.linalg.norm(r["keypoints_3d"] - joints, axis=-1)
    print("unequal-radius rig: mean error DLT %.3f mm, lm %.3f mm, better in %.0f %%, iterations %d..%d" % (
        dlt.mean(), lm.mean(), 100 * (lm < dlt).mean(), r["joint_status"].min(), r["joint_status"].max()))
    assert (r["joint_status"] > 0).all() and (r["joint_support"] == 4).all()
    assert lm.mean() < 0.8 * dlt.mean()
    assert dlt.mean() == pytest.approx(17.054, abs=2e-3) and lm.mean() == pytest.approx(12.052, abs=2e-3)


# ---- where the refinement is reached ------------------------------------------------------------------------------------------------
def _fake_post_stage(monkeypatch, calls):
    """triangulate_batch on host tensors: every ``_lib`` call it can make here is recorded and answered with zeros."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils import triangulation

    monkeypatch.setattr(triangulation, "_device_of", lambda hm: hm.device)

    def argmax_decode(hm, valid, b, v, j, hh, wh, stride, split_width):
        calls.append(("argmax_decode",))
        return torch.zeros((b, v, j, 2), dtype=torch.int64)

    def refine_keypoints(hm, kp2d, valid, b, v, j, hh, wh, stride, method):
        calls.append(("refine_keypoints", method))
        return torch.zeros((b, v, j, 2), dtype=torch.float32), torch.full((b, v, j), 0.5, dtype=torch.float32)

    def which(view_valid, view_joint_valid):  # the mask a call got, as the tail of its record
        return () if view_valid is None and view_joint_valid is None else ("views",) if view_joint_valid is None else ("view_joint",)

    def triangulate_ransac(kp2d, proj, valid, b, v, j, eps, *, view_valid=None, view_joint_valid=None):
        assert view_valid is None or view_joint_valid is None
        calls.append(("triangulate_ransac", eps) + which(view_valid, view_joint_valid))
        return (torch.zeros((b, j, 3), dtype=torch.float64), torch.zeros((b, j), dtype=torch.float64), torch.full((b, j), 2, dtype=torch.int32),
                torch.zeros((b,), dtype=torch.float64), torch.full((b,), 2, dtype=torch.int32))

    def refine_points_3d(kp2d, proj, valid, kp3d, joint_err, joint_inliers, b, v, j, eps, view_valid=None, view_joint_valid=None, weights=None):
        calls.append(("refine_points_3d", eps, kp2d.dtype, "vv" if view_valid is not None else "vj" if view_joint_valid is not None else None,
                      None if weights is None else (weights.dtype, tuple(weights.shape), float(weights.flatten()[0]))))
        return (torch.ones((b, j, 3), dtype=torch.float64), torch.ones((b, j), dtype=torch.float64), torch.full((b, j), v, dtype=torch.int32),
                torch.full((b, j), 5, dtype=torch.int32), torch.ones((b,), dtype=torch.float64))

    def reprojection_xe(kp3d, proj, hm, b, v, j, hh, wh, sigma, *, view_valid=None, view_joint_valid=None):
        calls.append(("reprojection_xe", float(kp3d.flatten()[0])) + which(view_valid, view_joint_valid))
        return torch.full((b,), 7.0, dtype=torch.float64)

    for f in (argmax_decode, refine_keypoints, triangulate_ransac, refine_points_3d, reprojection_xe):
        monkeypatch.setattr(_lib, f.__name__, f)


def test_triangulate_batch_reaches_the_refinement_only_when_asked(monkeypatch):
    from multi_view_active_learning_amd.utils import triangulation

    calls = []
    _fake_post_stage(monkeypatch, calls)
    hm, proj, valid = torch.zeros(2, 3, 5, 6, 8), torch.zeros(2, 3, 3, 4, dtype=torch.float64), torch.ones(2, 5)
    today = {"keypoints_3d", "keypoints_2d", "metric", "inlier_count", "joint_error", "joint_inliers"}
    for kw in ({}, dict(refine_3d="none"), dict(refine_3d="none", refine_3d_weights=None, refine_3d_epsilon=None)):
        del calls[:]
        r = triangulation.triangulate_batch(hm, proj, 4, valid, **kw)
        assert calls == [("argmax_decode",), ("triangulate_ransac", 5.0)] and set(r) == today
    del calls[:]
    r = triangulation.triangulate_batch(hm, proj, 4, valid, use_reprojection_xe=True, sigma=2.0)
    assert calls == [("argmax_decode",), ("triangulate_ransac", 5.0), ("reprojection_xe", 0.0)] and set(r) == today

    # "lm": exactly once, after the triangulation entry and before the XE entry, which reads the refined points
    del calls[:]
    r = triangulation.triangulate_batch(hm, proj, 4, valid, use_reprojection_xe=True, sigma=2.0, refine_3d="lm")
    assert calls == [("argmax_decode",), ("triangulate_ransac", 5.0), ("refine_points_3d", 5.0, torch.int64, None, None), ("reprojection_xe", 1.0)]
    assert set(r) == today | {"keypoints_3d_dlt", "joint_support", "joint_status"}
    assert r["keypoints_3d"].eq(1).all() and r["keypoints_3d_dlt"].eq(0).all() and r["joint_error"].eq(1).all() and r["metric"].eq(7).all()
    assert r["joint_inliers"].eq(2).all() and r["inlier_count"].eq(2).all()  # RANSAC's
    del calls[:]
    r = triangulation.triangulate_batch(hm, proj, 4, valid, reprojection_error_epsilon=3, refine_3d="lm", refine_3d_epsilon=1.5)
    assert calls == [("argmax_decode",), ("triangulate_ransac", 3.0), ("refine_points_3d", 1.5, torch.int64, None, None)] and r["metric"].eq(1).all()

    # masks go to the refinement as they go to the triangulation; weights: a tensor, or the confidences of a refined decode
    del calls[:]
    triangulation.triangulate_batch(hm, proj, 4, valid, refine_3d="lm", view_valid=torch.tensor([[1, 1, 0], [1, 1, 1]]))
    triangulation.triangulate_batch(hm, proj, 4, valid, refine_3d="lm", view_joint_valid=torch.ones(2, 3, 5), view_valid=torch.ones(2, 3),
                                    refine_3d_weights=torch.full((2, 3, 5), 2.0, dtype=torch.float64))
    assert calls == [("argmax_decode",), ("triangulate_ransac", 5.0, "views"), ("refine_points_3d", 5.0, torch.int64, "vv", None),
                     ("argmax_decode",), ("triangulate_ransac", 5.0, "view_joint"), ("refine_points_3d", 5.0, torch.int64, "vj", (torch.float32, (2, 3, 5), 2.0))]
    del calls[:]
    r = triangulation.triangulate_batch(hm, proj, 4, valid, refine="taylor", refine_3d="lm", refine_3d_weights="conf")
    assert calls == [("argmax_decode",), ("refine_keypoints", "taylor"), ("triangulate_ransac", 5.0),
                     ("refine_points_3d", 5.0, torch.float32, None, (torch.float32, (2, 3, 5), 0.5))]
    assert "keypoints_conf" in r and "joint_status" in r


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from multi_view_active_learning_amd.utils import triangulation

    calls = []
    _fake_post_stage(monkeypatch, calls)
    hm, proj, valid = torch.zeros(1, 2, 3, 4, 4), torch.zeros(1, 2, 3, 4, dtype=torch.float64), torch.ones(1, 3)
    for f, args in ((triangulation.triangulate_batch, (hm, proj, 4, valid)), (triangulation.triangulation, (hm[0], proj[0], 4, valid[0]))):
        with pytest.raises(ValueError, match="decode refinement"):  # "conf" without a decode refinement
            f(*args, refine_3d="lm", refine_3d_weights="conf")
        with pytest.raises(ValueError, match="without a 3-D refinement"):
            f(*args, refine_3d_weights=torch.ones(1, 2, 3)[0] if f is triangulation.triangulation else torch.ones(1, 2, 3))
        for bad in ("huber", "", 2):
            with pytest.raises(ValueError, match="'none', 'lm'"):
                f(*args, refine_3d=bad)
    with pytest.raises(NotImplementedError, match="direct_optimization"):  # raises exactly as before, refinement or not
        triangulation.triangulation(hm[0], proj[0], 4, valid[0], direct_optimization=True, refine_3d="lm")
    assert calls == []
    r = triangulation.triangulation(hm[0], proj[0], 4, valid[0], refine_3d="lm", refine_3d_weights=np.ones((2, 3)))
    assert [c[0] for c in calls] == ["argmax_decode", "triangulate_ransac", "refine_points_3d"] and calls[-1][-1] == (torch.float32, (1, 2, 3), 1.0)
    assert r["keypoints_3d"].shape == (3, 3) and r["keypoints_3d_dlt"].shape == (3, 3) and not r["keypoints_3d_dlt"].any()
    assert r["joint_error"].shape == r["joint_support"].shape == r["joint_status"].shape == (3,) and r["joint_status"].dtype == np.int32
    assert set(triangulation.triangulation(hm[0], proj[0], 4, valid[0])) == {"keypoints_3d", "keypoints_2d", "metric", "inlier_count"}


def _pass_kwargs(monkeypatch, cfg, which):
    """The keyword arguments ``_score_columns`` / ``evaluate_mkpe`` hand to ``triangulate_batch`` (replaced by a recorder)."""
    from collections import OrderedDict

    from multi_view_active_learning_amd import strategy
    from multi_view_active_learning_amd.utils import evaluation, triangulation

    b, v, j, hh, wh = 2, 3, 5, 6, 8
    seen = {}

    def score_heatmaps(configs, hm, joint_valid, stride=0, mirror_nonsquare_quirk=True, decode=False, view_valid=None, view_joint_valid=None):
        z = torch.zeros(b, v, j)
        return OrderedDict((k, (torch.zeros(b, dtype=torch.float64), z, z.to(torch.int32), torch.ones(b, j, dtype=torch.uint8),
                                torch.zeros(b, v, j, 2, dtype=torch.int64) if decode else None)) for k in configs)

    def triangulate_batch(hm, proj, stride, valid, *args, **kw):
        seen.update(kw)
        return {"keypoints_3d": torch.zeros(b, j, 3, dtype=torch.float64), "metric": torch.zeros(b, dtype=torch.float64),
                "inlier_count": torch.full((b,), 3, dtype=torch.int32)}

    monkeypatch.setattr(strategy, "_score_heatmaps", score_heatmaps)
    monkeypatch.setattr(triangulation, "triangulate_batch", triangulate_batch)
    monkeypatch.setattr(evaluation, "mkpe_per_sample", lambda pred, gt, valid: torch.zeros(b))
    dp = {"pose": torch.arange(b), "frame_id": torch.arange(b), "joint_valid": torch.ones(b, j), "proj_matrices": torch.zeros(b, v, 3, 4),
          "3d_keypoints": torch.zeros(b, 4, j)}
    st = strategy.ActiveLearningStrategy(cfg)
    st._pending_checks = []
    if which == "score":
        st._score_columns(torch.zeros(b * v, j, hh, wh), dp, ("HP", "TRIANGULATION", "CORESET"))
    else:
        def pool_loop(loader, model, body, inputs=None, stage=None):
            return [body(*inputs(torch.zeros(b * v, j, hh, wh), dp))]

        monkeypatch.setattr(st, "_pool_loop", pool_loop)
        monkeypatch.setattr(strategy._lib, "mkpe", lambda pred, gt, valid, n, jj, rows: (torch.zeros(()), None))
        monkeypatch.setattr("multi_view_active_learning_amd.parallel.all_gather_reference_order", lambda local, sizes: local)
        st.evaluate_mkpe(None, None)
    return seen


@pytest.mark.parametrize("which, node", [("score", "AL"), ("eval", "EVAL")])
def test_passes_read_the_config(monkeypatch, which, node):
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.config import get_default_configs

    monkeypatch.setattr(_lib, "refine_points_3d", lambda *a, **k: pytest.fail("the default configuration must not refine"))
    cfg = get_default_configs()
    seen = _pass_kwargs(monkeypatch, cfg, which)
    assert not any(k.startswith("refine") for k in seen), seen  # today's call, argument for argument
    getattr(cfg, node).REFINE_3D = "lm"
    seen = _pass_kwargs(monkeypatch, cfg, which)
    assert seen["refine_3d"] == "lm" and seen["refine_3d_weights"] is None and "refine" not in seen
    getattr(cfg, node).REFINE_3D_WEIGHTS = "conf"
    with pytest.raises(ValueError, match="decode refinement"):
        _pass_kwargs(monkeypatch, cfg, which)
    getattr(cfg, node).DECODE_REFINE = "taylor"
    seen = _pass_kwargs(monkeypatch, cfg, which)
    assert (seen["refine"], seen["refine_3d"], seen["refine_3d_weights"]) == ("taylor", "lm", "conf")
    getattr(cfg, node).REFINE_3D = "none"
    with pytest.raises(ValueError, match="without a 3-D refinement"):
        _pass_kwargs(monkeypatch, cfg, which)
    getattr(cfg, node).REFINE_3D_WEIGHTS = "none"
    getattr(cfg, node).REFINE_3D = "huber"
    with pytest.raises(ValueError, match="'none', 'lm'"):
        _pass_kwargs(monkeypatch, cfg, which)
    other = get_default_configs()  # the other node's fields do not leak into this pass
    getattr(other, "EVAL" if node == "AL" else "AL").REFINE_3D = "lm"
    assert not any(k.startswith("refine") for k in _pass_kwargs(monkeypatch, other, which))

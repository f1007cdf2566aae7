"""Host tests (no GPU) of the sub-pixel decode: the float64 oracle of tests/refine_oracle.py on exact Gaussians
and on one fixture per branch of the definition, the new entry in the header and the library, the two config fields and their
validator, and that the default configuration never reaches the refinement."""
import os
import re

import numpy as np
import pytest
import torch

import refine_oracle as ro

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1.0, 2.0, 3.0])
def test_oracle_recovers_exact_gaussians(sigma):
    """16 x 16 float32 maps of exp(-r^2 / 2 sigma^2), centres uniform in [2, 13]^2, 500 draws: the log of a Gaussian IS its
    second-order Taylor expansion, so taylor finds the centre up to the float32 rounding of the map's values -- within 1e-5
    heat-map px (the worst of these draws is 5.1e-7, 6.3e-7 and 9.6e-7 px for sigma 1, 2, 3, half of it the float32 rounding of the
    result itself, whose ulp between 8 and 16 is 9.5e-7: the bound is ten times that).
    quarter is within 0.25 px (+1e-6), the hard arg-max within 0.5 px."""
    rng = np.random.default_rng(int(sigma))
    ys, xs = np.mgrid[0:16, 0:16].astype(np.float64)
    worst = {"taylor": 0.0, "quarter": 0.0, "hard": 0.0}
    for _ in range(500):
        cx, cy = rng.uniform(2.0, 13.0, 2)
        h = np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2.0 * sigma ** 2)).astype(np.float32)
        for method in ro.METHODS:
            x, y, conf, status, margin = ro.refine_map(h, 1, method)
            assert status == "ok" and conf == h.max()
            worst[method] = max(worst[method], abs(float(x) - cx), abs(float(y) - cy))
        hard = ro.hard_decode(h[None, None, None], 1)[0, 0, 0]
        worst["hard"] = max(worst["hard"], abs(hard[0] - cx), abs(hard[1] - cy))
    print("sigma %g: worst |error| in px: %r" % (sigma, worst))
    assert worst["taylor"] <= 1e-5
    assert worst["quarter"] <= 0.25 + 1e-6
    assert worst["hard"] <= 0.5


def test_branch_fixture_ok():
    h = ro.block_map(ro.BLOCK_OK)
    x, y, conf, status, margin = ro.refine_map(h, 1, "taylor")
    assert status == "ok" and conf == np.float32(1.0) and margin >= 1e-6
    assert abs(float(x) - ro.OK_TAYLOR_PX[0]) < 1e-6 and abs(float(y) - ro.OK_TAYLOR_PX[1]) < 1e-6
    x4, y4 = ro.refine_map(h, 4, "taylor")[:2]
    assert abs(float(x4) - 4 * ro.OK_TAYLOR_PX[0]) < 4e-6 and abs(float(y4) - 4 * ro.OK_TAYLOR_PX[1]) < 4e-6
    # quarter: towards the higher neighbour on each axis (left .875 > right .125; below .875 > above .5)
    assert ro.refine_map(h, 1, "quarter")[:2] == (np.float32(1.75), np.float32(2.25))
    assert ro.refine_map(h, 4, "quarter")[:2] == (np.float32(7.0), np.float32(9.0))


@pytest.mark.parametrize("block, status", [(ro.BLOCK_FAR, "far"), (ro.BLOCK_NOTMAX, "notmax")])
def test_branch_fixtures_rejected(block, status):
    x, y, conf, got, margin = ro.refine_map(ro.block_map(block), 4, "taylor")
    assert got == status and (x, y, conf) == (np.float32(8.0), np.float32(8.0), np.float32(1.0))
    assert margin <= -1e-6
    assert ro.refine_map(ro.block_map(block), 4, "quarter")[3] == "ok"


def test_branch_fixture_plateau():
    """All nine equal: dxx == 0 exactly, ``dxx < 0`` is false.  Only a peak that is handed in sits in the middle of a plateau."""
    h = ro.block_map(ro.BLOCK_PLATEAU)
    x, y, conf, status, margin = ro.refine_map(h, 4, "taylor", peak=(2, 2))
    assert (status, x, y, conf) == ("notmax", np.float32(8.0), np.float32(8.0), np.float32(1.0)) and margin == -np.inf
    assert ro._taylor(np.ones((3, 3)))[2:] == ("notmax", -np.inf)
    assert ro.refine_map(h, 4, "quarter", peak=(2, 2))[:2] == (np.float32(8.0), np.float32(8.0))  # sgn(0) = 0
    # the map's own arg-max is the plateau's first element, whose neighbourhood is not flat
    assert ro.refine_map(h, 1, "taylor")[3] != "border" and ro.hard_decode(h[None, None, None], 1)[0, 0, 0].tolist() == [1, 1]


def test_branch_fixtures_nonpos_and_nonfinite():
    h = np.full((5, 5), -1.0, np.float32)
    h[2, 2] = 0.0
    assert ro.refine_map(h, 4, "taylor") == (np.float32(8.0), np.float32(8.0), np.float32(0.0), "nonpos", np.inf)
    assert ro.refine_map(h, 4, "quarter")[3] == "ok"  # (a flat surround: sgn 0 on both axes)
    assert ro.refine_map(h, 4, "quarter")[:2] == (np.float32(8.0), np.float32(8.0))
    h = ro.block_map(ro.BLOCK_OK)
    h[2, 2] = np.nan  # a NaN counts as the maximum
    for method in ro.METHODS:
        x, y, conf, status, _ = ro.refine_map(h, 4, method)
        assert (x, y, status) == (np.float32(8.0), np.float32(8.0), "nonfinite") and np.isnan(conf)
    h = ro.block_map(ro.BLOCK_OK)
    h[2, 2] = np.inf
    h[2, 3] = np.inf  # a +inf neighbour, later in the flat order than the peak
    for method in ro.METHODS:
        assert ro.refine_map(h, 4, method) == (np.float32(8.0), np.float32(8.0), np.float32(np.inf), "nonfinite", np.inf)
    h = ro.block_map(ro.BLOCK_OK)
    h[1, 1] = -np.inf
    for method in ro.METHODS:
        assert ro.refine_map(h, 4, method)[:4] == (np.float32(8.0), np.float32(8.0), np.float32(1.0), "nonfinite")


def test_branch_fixture_border_and_invalid():
    """Peaks at all four corners and on all four edges of a 6 x 5 map: offset (0, 0) whatever lies next to them."""
    hh, wh = 6, 5
    rng = np.random.default_rng(0)
    for px, py in [(0, 0), (wh - 1, 0), (0, hh - 1), (wh - 1, hh - 1), (2, 0), (2, hh - 1), (0, 3), (wh - 1, 3)]:
        h = rng.uniform(0.1, 0.5, (hh, wh)).astype(np.float32)
        h[py, px] = 1.0
        for method in ro.METHODS:
            assert ro.refine_map(h, 4, method) == (np.float32(4 * px), np.float32(4 * py), np.float32(1.0), "border", np.inf)
            assert ro.refine_map(h, 4, method, valid=False) == (np.float32(0), np.float32(0), np.float32(0), "invalid", np.inf)
    # the split is by the WIDTH: flat index 7 of a 6 x 5 map is (x, y) = (2, 1)
    h = np.zeros((hh, wh), np.float32)
    h[1, 2] = 1.0
    assert ro.refine_map(h, 1, "quarter")[:2] == (np.float32(2.0), np.float32(1.0))


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_and_exported():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    text = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+mval_refine_keypoints\s*\(([^)]*)\)", hdr)
    assert decl, "mval_refine_keypoints is not declared in include/mval_hip.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["int method", "const float* heatmaps", "const int64_t* kp2d", "const uint8_t* valid", "float* out", "float* conf",
                    "int B", "int V", "int J", "int hh", "int wh", "int stride", "void* stream"]
    assert hasattr(_lib.lib(), "mval_refine_keypoints"), "mval_refine_keypoints is not exported"
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))  # noqa: E731
    assert _lib.REFINE_IDS == {"quarter": define("MVAL_REFINE_QUARTER"), "taylor": define("MVAL_REFINE_TAYLOR")} == {"quarter": 1, "taylor": 2}


def test_entry_rejects_bad_arguments_without_a_launch():
    """method outside {1, 2}, stride <= 0 and bad dimensions are errors before anything touches a device; B = 0 returns 0."""
    import ctypes as C

    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    f = _lib.lib().mval_refine_keypoints
    null = C.c_void_p(0)

    def call(method=2, b=1, v=2, j=3, hh=8, wh=8, stride=4):
        return f(C.c_int(method), null, null, null, null, null, C.c_int(b), C.c_int(v), C.c_int(j), C.c_int(hh), C.c_int(wh), C.c_int(stride), null)

    assert call(b=0) == 0
    for bad in (dict(method=0), dict(method=3), dict(stride=0), dict(stride=-4), dict(b=-1), dict(v=0), dict(j=0), dict(hh=0), dict(wh=-1)):
        assert call(**bad) == -1, bad
        assert b"mval_refine_keypoints" in _lib.lib().mval_last_error()
    assert call() == -1  # (NULL heat-maps)


def test_check_decode_refine():
    from multi_view_active_learning_amd.config import check_decode_refine, get_default_configs

    cfg = get_default_configs()
    assert cfg.AL.DECODE_REFINE == "none" and cfg.EVAL.DECODE_REFINE == "none"
    from multi_view_active_learning_amd import _lib, config

    assert config.DECODE_REFINES == ("none",) + tuple(_lib.REFINE_IDS)
    for ok in ("none", "quarter", "taylor"):
        assert check_decode_refine(ok) == ok
    assert check_decode_refine("none", use_softargmax=True) == "none"
    for bad in ("", "dark", "TAYLOR", None, 1, True):
        with pytest.raises(ValueError, match="'none', 'quarter', 'taylor'"):
            check_decode_refine(bad)
    for m in ("quarter", "taylor"):
        with pytest.raises(ValueError, match="USE_SOFTARGMAX"):
            check_decode_refine(m, use_softargmax=True)


def _fake_post_stage(monkeypatch, calls):
    """triangulate_batch on host tensors: every ``_lib`` call it can make is recorded and answered with zeros."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils import triangulation

    monkeypatch.setattr(triangulation, "_device_of", lambda hm: hm.device)

    def argmax_decode(hm, valid, b, v, j, hh, wh, stride, split_width):
        calls.append(("argmax_decode", split_width))
        return torch.zeros((b, v, j, 2), dtype=torch.int64)

    def refine_keypoints(hm, kp2d, valid, b, v, j, hh, wh, stride, method):
        calls.append(("refine_keypoints", method, kp2d.dtype))
        return torch.zeros((b, v, j, 2), dtype=torch.float32), torch.ones((b, v, j), dtype=torch.float32)

    def triangulate_ransac(kp2d, proj, valid, b, v, j, eps, *, view_valid=None, view_joint_valid=None):
        mask = () if view_valid is None and view_joint_valid is None else ("views",) if view_joint_valid is None else ("view_joint",)
        calls.append(("triangulate_ransac", kp2d.dtype) + mask)
        return (torch.zeros((b, j, 3), dtype=torch.float64), torch.zeros((b, j), dtype=torch.float64), torch.zeros((b, j), dtype=torch.int32),
                torch.zeros((b,), dtype=torch.float64), torch.zeros((b,), dtype=torch.int32))

    monkeypatch.setattr(_lib, "argmax_decode", argmax_decode)
    monkeypatch.setattr(_lib, "refine_keypoints", refine_keypoints)
    monkeypatch.setattr(_lib, "triangulate_ransac", triangulate_ransac)
    monkeypatch.setattr(_lib, "soft_argmax", lambda hm, n, hh, wh, scale: calls.append(("soft_argmax",)) or torch.zeros((n, 2)))


def test_triangulate_batch_reaches_the_refinement_only_when_asked(monkeypatch):
    from multi_view_active_learning_amd.utils import triangulation

    calls = []
    _fake_post_stage(monkeypatch, calls)
    hm, proj, valid = torch.zeros(2, 3, 5, 6, 8), torch.zeros(2, 3, 3, 4, dtype=torch.float64), torch.ones(2, 5)
    r = triangulation.triangulate_batch(hm, proj, 4, valid)
    assert calls == [("argmax_decode", 6), ("triangulate_ransac", torch.int64)]  # the reference's split by the height, as ever
    assert "keypoints_conf" not in r and r["keypoints_2d"].dtype == torch.int64
    del calls[:]
    triangulation.triangulate_batch(hm, proj, 4, valid, mirror_nonsquare_quirk=False)
    triangulation.triangulate_batch(hm, proj, 4, valid, keypoints_2d=torch.zeros(2, 3, 5, 2, dtype=torch.int64))
    triangulation.triangulate_batch(hm, proj, 4, valid, use_soft_argmax=True)
    assert calls == [("argmax_decode", 8), ("triangulate_ransac", torch.int64), ("triangulate_ransac", torch.int64),
                     ("soft_argmax",), ("triangulate_ransac", torch.float32)]
    for method in ("quarter", "taylor"):
        for quirk in (True, False):  # no effect under a refinement: split by the width
            del calls[:]
            r = triangulation.triangulate_batch(hm, proj, 4, valid, mirror_nonsquare_quirk=quirk, refine=method)
            assert calls == [("argmax_decode", 8), ("refine_keypoints", method, torch.int64), ("triangulate_ransac", torch.float32)]
            assert r["keypoints_2d"].dtype == torch.float32 and r["keypoints_conf"].shape == (2, 3, 5)
        del calls[:]
        r = triangulation.triangulate_batch(hm, proj, 4, valid, keypoints_2d=torch.zeros(2, 3, 5, 2, dtype=torch.int64), refine=method,
                                            view_valid=torch.tensor([[1, 1, 0], [1, 1, 1]]))
        assert calls == [("refine_keypoints", method, torch.int64), ("triangulate_ransac", torch.float32, "views")]
        assert not r["keypoints_conf"][0, 2].any() and r["keypoints_conf"][0, :2].all() and r["keypoints_conf"][1].all()


def test_refine_with_soft_argmax_and_unknown_names_raise(monkeypatch):
    from multi_view_active_learning_amd.utils import triangulation

    calls = []
    _fake_post_stage(monkeypatch, calls)
    hm, proj, valid = torch.zeros(1, 2, 3, 4, 4), torch.zeros(1, 2, 3, 4, dtype=torch.float64), torch.ones(1, 3)
    for method in ("quarter", "taylor"):
        with pytest.raises(ValueError, match="use_soft_argmax"):
            triangulation.triangulate_batch(hm, proj, 4, valid, use_soft_argmax=True, refine=method)
        with pytest.raises(ValueError, match="use_soft_argmax"):
            triangulation.triangulation(hm[0], proj[0], 4, valid[0], use_soft_argmax=True, refine=method)
    for bad in ("dark", "", None, 2):
        with pytest.raises(ValueError, match="'quarter', 'taylor'"):
            triangulation.triangulate_batch(hm, proj, 4, valid, refine=bad)
        with pytest.raises(ValueError, match="'quarter', 'taylor'"):
            triangulation.decode_keypoints(hm, 4, refine=bad)
    assert calls == []
    kp, conf = triangulation.decode_keypoints(hm, 4)
    assert conf is None and kp.dtype == torch.int64
    kp, conf = triangulation.decode_keypoints(hm, 4, valid, refine="taylor")
    assert kp.dtype == torch.float32 and conf.shape == (1, 2, 3)
    assert calls == [("argmax_decode", 4), ("argmax_decode", 4), ("refine_keypoints", "taylor", torch.int64)]


def _score_columns_calls(monkeypatch, cfg, strategies):
    """What ``_score_columns`` hands to ``_score_heatmaps`` and ``triangulate_batch`` (both replaced by recorders)."""
    from collections import OrderedDict

    from multi_view_active_learning_amd import strategy
    from multi_view_active_learning_amd.utils import evaluation, triangulation

    b, v, j, hh, wh = 2, 3, 5, 6, 8
    seen = {}

    def score_heatmaps(configs, hm, joint_valid, stride=0, mirror_nonsquare_quirk=True, decode=False, view_valid=None, view_joint_valid=None):
        seen["score"] = dict(mirror_nonsquare_quirk=mirror_nonsquare_quirk, decode=decode)
        z = torch.zeros(b, v, j)
        return OrderedDict((k, (torch.zeros(b, dtype=torch.float64), z, z.to(torch.int32), torch.ones(b, j, dtype=torch.uint8),
                                torch.zeros(b, v, j, 2, dtype=torch.int64) if decode else None)) for k in configs)

    def triangulate_batch(hm, proj, stride, valid, *args, **kw):
        seen["triangulate"] = kw
        return {"keypoints_3d": torch.zeros(b, j, 3, dtype=torch.float64), "metric": torch.zeros(b, dtype=torch.float64),
                "inlier_count": torch.full((b,), 3, dtype=torch.int32)}

    monkeypatch.setattr(strategy, "_score_heatmaps", score_heatmaps)
    monkeypatch.setattr(triangulation, "triangulate_batch", triangulate_batch)
    monkeypatch.setattr(evaluation, "mkpe_per_sample", lambda pred, gt, valid: torch.zeros(b))
    dp = {"pose": torch.arange(b), "frame_id": torch.arange(b), "joint_valid": torch.ones(b, j), "proj_matrices": torch.zeros(b, v, 3, 4),
          "3d_keypoints": torch.zeros(b, 4, j)}
    st = strategy.ActiveLearningStrategy(cfg)
    st._pending_checks = []
    st._score_columns(torch.zeros(b * v, j, hh, wh), dp, strategies)
    return seen


def test_score_columns_default_path_is_todays(monkeypatch):
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.config import get_default_configs

    monkeypatch.setattr(_lib, "refine_keypoints", lambda *a, **k: pytest.fail("the default configuration must not refine"))
    cfg = get_default_configs()
    seen = _score_columns_calls(monkeypatch, cfg, ("HP", "TRIANGULATION"))
    assert seen["score"] == dict(mirror_nonsquare_quirk=True, decode=True)
    assert "refine" not in seen["triangulate"] and seen["triangulate"]["keypoints_2d"] is not None
    cfg.AL.USE_SOFTARGMAX = True
    seen = _score_columns_calls(monkeypatch, cfg, ("HP",))
    assert seen["score"] == dict(mirror_nonsquare_quirk=True, decode=False) and "refine" not in seen["triangulate"]


@pytest.mark.parametrize("method", ["quarter", "taylor"])
def test_score_columns_reads_the_config(monkeypatch, method):
    from multi_view_active_learning_amd.config import get_default_configs

    cfg = get_default_configs()
    cfg.AL.DECODE_REFINE = method
    seen = _score_columns_calls(monkeypatch, cfg, ("MPE", "TRIANGULATION"))
    assert seen["score"] == dict(mirror_nonsquare_quirk=False, decode=True)
    assert seen["triangulate"]["refine"] == method and seen["triangulate"]["keypoints_2d"].dtype == torch.int64
    seen = _score_columns_calls(monkeypatch, cfg, ("TRIANGULATION",))  # no heat-map statistic: triangulate_batch decodes itself
    assert "score" not in seen and seen["triangulate"]["refine"] == method and seen["triangulate"]["keypoints_2d"] is None
    cfg.AL.USE_SOFTARGMAX = True
    with pytest.raises(ValueError, match="USE_SOFTARGMAX"):
        _score_columns_calls(monkeypatch, cfg, ("TRIANGULATION",))
    cfg.AL.USE_SOFTARGMAX = False
    cfg.AL.DECODE_REFINE = "dark"
    with pytest.raises(ValueError, match="'none', 'quarter', 'taylor'"):
        _score_columns_calls(monkeypatch, cfg, ("TRIANGULATION",))

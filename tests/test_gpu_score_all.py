"""GPU: every uncertainty strategy from one pass -- mval_score_decode_maps_all (HP, MPE, BSB and the hard arg-max from ONE
staged read of each heat-map) against the single-kind entries, bit for bit, and ``_compute_sal_dicts`` against the
reference goldens and against ``_compute_sal_dict`` run once per strategy."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
ALL5 = ("HP", "MPE", "BSB", "TRIANGULATION", "CORESET")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


def _bits(t):
    """float32 tensor -> its bit patterns (NaNs compare by payload as well)."""
    return t.contiguous().view(torch.int32).cpu().numpy()


def _check_against_single_kind(dev, hm, valid, splits=None, decode_modes=(True, False)):
    """All outputs of the fused entry equal the single-kind entries' (mval_score_maps per kind, mval_argmax_decode)."""
    from multi_view_active_learning_amd import _lib

    b, v, j, hh, wh = hm.shape
    n = b * v * j
    t = torch.from_numpy(hm).to(dev)
    vd = None if valid is None else torch.from_numpy(valid).to(dev)
    want = [_lib.score_maps(kind, t, n, hh, wh) for kind in (_lib.SCORE_HP, _lib.SCORE_MPE, _lib.SCORE_BSB)]
    out = None
    for split in splits or (hh, wh):
        kp0 = _lib.argmax_decode(t, vd, b, v, j, hh, wh, 4, split)
        for decode in decode_modes:
            stat, cnt, kp = _lib.score_decode_maps_all(t, vd, b, v, j, hh, wh, 4, split, decode=decode)
            assert stat.shape == (3, n) and stat.dtype == torch.float32 and cnt.shape == (2, n) and cnt.dtype == torch.int32
            for k, name in enumerate(("HP", "MPE", "BSB")):
                np.testing.assert_array_equal(_bits(stat[k]), _bits(want[k][0]), err_msg="%s split %d decode %s" % (name, split, decode))
            assert torch.equal(cnt[0], want[1][1]) and torch.equal(cnt[1], want[2][1])
            if decode:
                assert torch.equal(kp, kp0)
            else:
                assert kp is None
            out = stat, cnt, kp0
    return out


# ---- (a) the kernel against the single-kind entries ----------------------------------------------------------------
SHAPES = [(2, 4, 19, 64, 64),   # float4 staging, 4 lanes per row
          (1, 8, 19, 96, 72),   # 2 lanes per row
          (3, 2, 5, 17, 23),    # scalar staging
          (1, 2, 2, 4, 9),      # no interior after the 2-px border
          (1, 1, 2, 8, 264)]    # interior wider than the workgroup


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_all_equals_single_kind_entries(dev, shape):
    """The inputs of test_fused_score_decode_equals_separate_passes (a constant map, a NaN pixel, a 2 x 2 plateau -- the
    map whose MPE spacing pass takes the tile's memory, so that it is staged again for HP and BSB --, one invalid joint), at
    both index splits, with and without the decode."""
    b, v, j, hh, wh = shape
    rng = np.random.default_rng(hh * 7 + wh)
    hm = rng.standard_normal(shape).astype(np.float32) * 0.3
    hm[0, 0, 0] = 0.25                                          # a constant map: all ties -> index 0, no peak above the minimum
    hm[0, 1 % v, 1, min(3, hh - 1), 4 if hh >= 9 else 7] = np.nan  # NaN is the arg-max (clear of the plateau on the small maps)
    y0, x0 = (5, 6) if hh >= 9 else (hh // 2 - 1, 3)
    hm[-1, -1, min(2, j - 1), y0:y0 + 2, x0:x0 + 2] = 9.0       # a 2 x 2 plateau (inside the interior where there is one)
    valid = np.ones((b, j), dtype=np.uint8)
    valid[0, min(3, j - 1)] = 0
    stat, cnt, kp = _check_against_single_kind(dev, hm, valid)
    assert kp[0, :, min(3, j - 1)].abs().sum().item() == 0      # invalid joint -> (0, 0)
    if hh >= 9:
        plateau = (b * v - 1) * j + min(2, j - 1)
        assert cnt[0, plateau].item() >= 1 and math.isfinite(stat[0, plateau].item())  # (HP of the re-staged map)
    _check_against_single_kind(dev, hm, None, splits=(hh,))     # valid NULL


# ---- (b) the rescue pass, statistic by statistic ----------------------------------------------------------------------
def test_rescue_pass_redoes_one_statistic_and_keeps_the_others(dev):
    """Two maps among noise: all ones with [0, 0] = 0 (3600 raw and 3540 row-softmax candidates: MPE and BSB overflow the
    first pass's SC_MAX_PEAKS = 512) and 0.1 * row with [0, 0] = -1 (0 raw, 3540 row-softmax candidates: BSB alone
    overflows, and its second pass must leave that map's MPE and HP as the first pass wrote them)."""
    from oracle import scoring

    shape = (1, 2, 3, 64, 64)
    hm = (np.random.default_rng(11).standard_normal(shape) * 0.3).astype(np.float32)
    both = np.ones((64, 64), dtype=np.float32)
    both[0, 0] = 0.0
    bsb_only = (0.1 * np.arange(64, dtype=np.float32))[:, None].repeat(64, axis=1)
    bsb_only[0, 0] = -1.0
    hm[0, 0, 1], hm[0, 1, 2] = both, bsb_only
    n_cand = lambda m: len(scoring.peak_candidates(m, 2))  # noqa: E731
    assert (n_cand(both), n_cand(scoring._row_softmax(both))) == (3600, 3540)
    assert (n_cand(bsb_only), n_cand(scoring._row_softmax(bsb_only))) == (0, 3540)
    stat, cnt, _ = _check_against_single_kind(dev, hm, np.ones((1, 3), dtype=np.uint8), splits=(64,))
    i_both, i_bsb = 1, 5
    assert cnt[:, i_both].min().item() > 512 // 4 and cnt[0, i_bsb].item() == 0 and cnt[1, i_bsb].item() > 512 // 4
    assert stat[1, i_bsb].item() == 0.0 and 0.0 < stat[0, i_bsb].item() < 1.0  # MPE without peaks: 0; HP of the map


# ---- (c) the pass against the reference goldens and the single-strategy pass -----------------------------------------------
def _sal_setup(c, dev):
    from multi_view_active_learning_amd.config import get_default_configs

    cfg = get_default_configs()
    cfg.AL.STRATEGY = c["strategy"]
    cfg.POSE_ESTIMATOR.STRIDE = c["stride"]
    cfg.AL.USE_REPROJECTION_XE = c.get("xe", False)
    cfg.AL.REPROJECTION_SIGMA = c.get("sigma", 1.0)
    loader, heatmaps = cases.build_sal_loader(c)
    tl = [{k: torch.from_numpy(v) for k, v in dp.items()} for dp in loader]

    def model():
        it = iter(heatmaps)
        return lambda images: torch.from_numpy(next(it)).to(dev)

    return cfg, tl, model


def _dicts_equal(a, b):
    """== on the five dicts, key order included; NaN mkpe aside (NaN != NaN)."""
    assert list(a) == list(b)
    for field in a:
        assert list(a[field]) == list(b[field]), field
        if field == "mkpe":
            for g in a[field]:
                assert a[field][g] == b[field][g] or (math.isnan(a[field][g]) and math.isnan(b[field][g])), (field, g)
        else:
            assert a[field] == b[field], field


@pytest.mark.parametrize("name", list(cases.sal_cases()))
def test_sal_dicts_vs_reference_golden_and_single_strategy_pass(dev, name):
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    with open(os.path.join(G, "sal_dict.json")) as f:
        want = json.load(f)[name]
    c = cases.sal_cases()[name]
    cfg, tl, model = _sal_setup(c, dev)
    dicts = ActiveLearningStrategy(cfg)._compute_sal_dicts(tl, model(), ALL5)
    assert list(dicts) == list(ALL5)
    # the case's own strategy: the comparisons of test_sal_dict_vs_reference_golden
    sal = dicts[c["strategy"]]
    for field in ("al_metric", "sal_metric", "inlier_count", "mkpe", "pred_3d_keypoints"):
        assert list(sal[field]) == list(want[field]), field  # key order = gather order
    for g in want["al_metric"]:
        tol = 0 if c["strategy"] == "CORESET" else 3e-6
        assert abs(sal["al_metric"][g] - want["al_metric"][g]) <= tol * abs(want["al_metric"][g]) + 1e-12, (g, sal["al_metric"][g], want["al_metric"][g])
        assert abs(sal["sal_metric"][g] - want["sal_metric"][g]) <= 1e-6 * abs(want["sal_metric"][g])
        assert sal["inlier_count"][g] == want["inlier_count"][g]
        a, b_ = sal["mkpe"][g], want["mkpe"][g]
        assert (np.isnan(a) and np.isnan(b_)) or abs(a - b_) <= 1e-5 * abs(b_)
        np.testing.assert_allclose(sal["pred_3d_keypoints"][g], want["pred_3d_keypoints"][g], rtol=0, atol=1e-3)
    st = ActiveLearningStrategy(cfg)
    if c["strategy"] != "CORESET":
        assert st.select_al_guids(sal, c["select"]) == want["nlargest"]
    # every strategy: exactly the single-strategy pass on the same inputs
    for s in ALL5:
        cfg.AL.STRATEGY = s
        _dicts_equal(dicts[s], ActiveLearningStrategy(cfg)._compute_sal_dict(tl, model()))


def test_sal_dicts_random_draws_and_soft_argmax(dev):
    """RANDOM draws one torch.rand(1) per frame in frame order, whatever else is asked for; with AL.USE_SOFTARGMAX the
    fused launch runs without its decode beside the soft-arg-max kernel; HP STD stays float64."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    c = cases.sal_cases()["hp"]
    cfg, tl, model = _sal_setup(c, dev)
    cfg.AL.USE_SOFTARGMAX = True
    cfg.AL.HP_CONFIG = "STD"
    names = ("RANDOM", "BSB", "HP", "MPE")
    torch.manual_seed(5)
    dicts = ActiveLearningStrategy(cfg)._compute_sal_dicts(tl, model(), names)
    assert list(dicts) == list(names)
    for s in names:
        cfg.AL.STRATEGY = s
        torch.manual_seed(5)
        _dicts_equal(dicts[s], ActiveLearningStrategy(cfg)._compute_sal_dict(tl, model()))
    hp = list(dicts["HP"]["al_metric"].values())
    assert any(float(np.float32(x)) != x for x in hp)  # float64 values, not float32-rounded ones


# ---- (c2) one table builder, one scorer: the single-strategy and the multi-strategy path side by side --------------------------
ALL6 = ("HP", "MPE", "BSB", "TRIANGULATION", "CORESET", "RANDOM")
# B = 2, V = 3, J = 3, maps 12 x 16, stride 4, two batches (cases.build_sal_loader: ring cameras, one invalid joint per batch)
SMALL = dict(strategy="HP", seed=60, nbatch=2, b=2, v=3, j=3, h=48, w=64, stride=4, noise=0.3, outliers=1)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "softargmax"])
def test_score_batch_equals_score_batch_all_column_for_column(dev, soft):
    """``score_batch`` under each of the six strategies against the columns of ONE ``score_batch_all`` over all six: the
    al_metric (column 2 against column 6 + 3J + e) and the base columns, torch.equal on the bit patterns (a frame's mkpe is
    NaN with these inputs, see ``_dicts_equal``, and NaN != NaN under torch.equal on the values).  torch's and python's generators are
    reseeded before each call (RANDOM draws one torch.rand(1) per frame; V = 3 draws no view pairs).
    Inputs: seed 60 with noise 0.3, checked on the CPU with oracle/scoring.py when this was written -- over the valid maps
    of both batches the fewest BSB peaks (peak_local_max of the row softmax, min_distance 2) are 2, the fewest MPE peaks 2,
    the most candidates 6; the 8 x 12 interior cannot overflow the candidate list of 128 at all."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy, _stage_batch

    cfg, tl, model = _sal_setup(SMALL, dev)
    cfg.AL.USE_SOFTARGMAX = soft
    dp, hm, j = _stage_batch(tl[0]), model()(None), SMALL["j"]
    st = ActiveLearningStrategy(cfg)
    st._pending_checks = []

    def seeded(fn, *args):
        torch.manual_seed(31)
        random.seed(31)
        return fn(hm, dp, *args)

    def same(a, b):  # torch.equal on the float64 bit patterns: what torch.equal asks, and a NaN equals itself
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))

    wide = seeded(st.score_batch_all, ALL6)
    assert wide.shape == (2, 6 + 3 * j + 6) and wide.dtype == torch.float64
    assert not wide[:, 2].any().item()
    for e, s in enumerate(ALL6):
        cfg.AL.STRATEGY = s
        one = seeded(st.score_batch)
        assert one.shape == (2, 6 + 3 * j) and one.dtype == torch.float64
        assert same(one[:, 2], wide[:, 6 + 3 * j + e]), s
        assert same(one[:, :2], wide[:, :2]) and same(one[:, 3:], wide[:, 3:6 + 3 * j]), s
    assert (wide[:, 6 + 3 * j + ALL6.index("RANDOM")] != 0).all().item()  # (the draws did arrive)
    st._raise_deferred_errors()  # no map overflowed, every valid map has its two BSB peaks


@pytest.mark.parametrize("names", [("MPE", "CORESET"), ("BSB", "RANDOM")], ids="-".join)
def test_pass_with_one_statistic_kind_equals_the_single_pass(dev, names):
    """A multi-strategy pass that names ONE of HP / MPE / BSB runs the one-kind kernel, like the single-strategy pass: its
    dict for that kind equals ``_compute_sal_dict``'s, all five dicts, values and key order (SMALL's inputs, two batches)."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    cfg, tl, model = _sal_setup(SMALL, dev)

    def seeded(fn, *args):
        torch.manual_seed(31)
        random.seed(31)
        return fn(tl, model(), *args)

    dicts = seeded(ActiveLearningStrategy(cfg)._compute_sal_dicts, names)
    assert list(dicts) == list(names) and len(dicts[names[0]]["al_metric"]) == 4
    cfg.AL.STRATEGY = names[0]
    _dicts_equal(dicts[names[0]], seeded(ActiveLearningStrategy(cfg)._compute_sal_dict))


# ---- (d) deferred errors only for what was asked for ------------------------------------------------------------------
def test_bsb_index_error_only_when_bsb_is_asked_for(dev):
    """One frame whose valid joint has a map with a single peak in its row softmax: -(x - 7)^2 / (1 + |y - 6|) -- every row
    peaks in column 7, the sharpest row (y = 6) highest.  ("HP", "BSB") raises the reference's IndexError, ("HP", "MPE")
    does not."""
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from oracle import scoring

    hh = wh = 16
    y, x = np.mgrid[0:hh, 0:wh].astype(np.float32)
    one_peak = (-((x - 7.0) ** 2) / (1.0 + np.abs(y - 6.0))).astype(np.float32)
    assert len(scoring.peak_local_max(scoring._row_softmax(one_peak), min_distance=2)) == 1
    v, j = 4, 2
    proj = cases.synth.ring_cameras(v, hh * 4, wh * 4, seed=3)[None]
    hm = (np.random.default_rng(2).standard_normal((v, j, hh, wh)) * 0.3).astype(np.float32)
    hm[:, 0] = one_peak
    dp = dict(images=torch.zeros((1, v, 3, 8, 8)), pose=torch.tensor([4]), frame_id=torch.tensor([9]),
              proj_matrices=torch.from_numpy(proj), joint_valid=torch.tensor([[1.0, 0.0]]),
              **{"3d_keypoints": torch.ones((1, 4, j))})
    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = 4
    model = lambda images: torch.from_numpy(hm).to(dev)  # noqa: E731
    st = ActiveLearningStrategy(cfg)
    with pytest.raises(IndexError):
        st._compute_sal_dicts([dp], model, ("HP", "BSB"))
    got = st._compute_sal_dicts([dp], model, ("HP", "MPE"))
    assert list(got) == ["HP", "MPE"] and list(got["MPE"]["al_metric"]) == ["4-9"]
    assert all(math.isfinite(d["al_metric"]["4-9"]) for d in got.values())


# ---- (e) capture and replay -------------------------------------------------------------------------------------------
def test_fused_launch_is_graph_capturable(dev):
    """One fused launch (both passes) captured into a graph and replayed on new inputs gives the eager bits: the entry
    neither allocates nor synchronises (either would fail the capture)."""
    from multi_view_active_learning_amd import _lib

    b, v, j, hh, wh = 1, 2, 3, 64, 64
    rng = np.random.default_rng(23)
    first = torch.from_numpy((rng.standard_normal((b, v, j, hh, wh)) * 0.3).astype(np.float32)).to(dev)
    second = (rng.standard_normal((b, v, j, hh, wh)) * 0.3).astype(np.float32)
    second[0, 1, 0] = 1.0
    second[0, 1, 0, 0, 0] = 0.0  # (a map for the second pass)
    second = torch.from_numpy(second).to(dev)
    valid = torch.ones((b, j), dtype=torch.uint8, device=dev)
    buf = first.clone()
    _lib.score_decode_maps_all(buf, valid, b, v, j, hh, wh, 4, hh)  # (first launch outside the capture: code objects loaded)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _lib.score_decode_maps_all(buf, valid, b, v, j, hh, wh, 4, hh)
    for src in (first, second):
        buf.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        eager = _lib.score_decode_maps_all(src, valid, b, v, j, hh, wh, 4, hh)
        np.testing.assert_array_equal(_bits(out[0]), _bits(eager[0]))
        assert torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2])
    assert (out[1] > 512).any().item()  # the second input did go through the second pass

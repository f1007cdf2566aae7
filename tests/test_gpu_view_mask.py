"""GPU tests of frames with missing views (``view_valid``, MVAL_MASK_VIEWS): the `_masked` triangulation entries,
mval_score_reduce_masked and mval_reprojection_xe_masked, and the calls that carry the mask (triangulate_batch, the heat-map scorers, the scoring and
evaluation passes).

Two oracles.  (1) The real reference handed each frame's present views alone (tests/golden/view_mask.npz and
sal_dict_view_mask.json, make_view_mask_golden.py), under the tolerances of the existing golden tests
(test_gpu_many_views.py): key-points, inlier counts and pair tables exact, 3-D points 1e-6 mm, errors and metric 1e-9
relative, HP 3e-6 relative (test_gpu_hotpath.py).  No problem is left out: every vote of every problem is decidable.
(2) Today's unmasked calls on the frame's present views alone, bit for bit -- which also pins MPE / BSB and the XE metric."""
import json
import os
import random

import numpy as np
import pytest
import torch

import cases
import many_view_cases as mv
import view_mask_cases as vm

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
NPZ = os.path.join(G, "view_mask.npz")
OUT = ("keypoints_3d", "joint_error", "joint_inliers", "metric", "inlier_count")
ALL6 = ("HP", "MPE", "BSB", "TRIANGULATION", "CORESET", "RANDOM")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


_INPUTS = {}


def _inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = vm.build(vm.view_mask_cases()[name])
    return _INPUTS[name]


def _same_bits(a, b):
    """torch.equal that takes NaN for what it is: the same bits."""
    if a.dtype.is_floating_point:
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                                                         b.contiguous().view(torch.int64 if b.dtype == torch.float64 else torch.int32))
    return torch.equal(a, b)


def _masked(dev, name, hm=None, proj=None, **kw):
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = vm.view_mask_cases()[name]
    hm0, proj0, valid, vv = _inputs(name)
    hm = hm0 if hm is None else hm
    proj = proj0 if proj is None else proj
    return triangulate_batch(torch.from_numpy(hm).to(dev), torch.from_numpy(proj), c["stride"], torch.from_numpy(valid),
                             n_iters=c["n_iters"], reprojection_error_epsilon=vm.EPS, pair_rng=random,
                             view_valid=torch.from_numpy(vv), **kw)


@pytest.mark.parametrize("name", list(vm.view_mask_cases()))
def test_triangulate_batch_vs_reference_golden(dev, name):
    """Every case of view_mask_cases.py against the reference on the present views: m4 (absent views with a consistent peak;
    two present views = one pair in an 8-lane group), m8_nonsquare (first and last bit absent), m11 (55-pair group), m12_mixed
    (ONE batch of a frame with 55 pairs, one that draws 64 of 66, one with 45: padded per-problem tables), m16_n100 (two lane
    trips), m32 (bit 31), degenerate (-2, -2, -1).  The RNG ends where the reference left it, untouched where nothing is
    drawn; the key-point rows of absent views are zero."""
    c = vm.view_mask_cases()[name]
    z = vm.load_golden(NPZ, name)
    _, _, valid, vv = _inputs(name)
    random.seed(int(z["rseed"]))
    before = random.getstate()
    r = _masked(dev, name)
    assert vm.state_digest(random.getstate()) == str(z["frame_digests"][-1])
    if not vm.draws(c).any():
        assert random.getstate() == before
    got = {k: t.cpu().numpy() for k, t in r.items()}
    assert not got["keypoints_2d"][~vv].any()
    ok = z["inlier_count"] >= 0  # (a frame the reference refused has no reference key-points)
    np.testing.assert_array_equal(got["keypoints_2d"][ok], z["keypoints_2d"][ok])
    np.testing.assert_array_equal(got["joint_inliers"], z["joint_inliers"])
    np.testing.assert_array_equal(got["inlier_count"], z["inlier_count"])
    print("max |kp3d - reference| = %.3e mm" % np.abs(got["keypoints_3d"] - z["keypoints_3d"]).max())
    np.testing.assert_allclose(got["keypoints_3d"], z["keypoints_3d"], rtol=0, atol=1e-6)
    assert not got["keypoints_3d"][~valid].any() and not got["keypoints_3d"][~ok].any()
    np.testing.assert_allclose(got["joint_error"], z["joint_error"], rtol=1e-9)
    np.testing.assert_allclose(got["metric"], z["metric"], rtol=1e-9)
    assert np.isnan(got["metric"][~ok]).all()


def test_degenerate_frames_raise_like_the_reference(dev):
    """One frame through ``triangulation``: one present view and none raise the reference's AssertionError (its
    ``assert len(points) >= 2``), no valid joint its ValueError (np.min([])) whatever the views."""
    from multi_view_active_learning_amd.utils.triangulation import triangulation

    c = vm.view_mask_cases()["degenerate"]
    hm, proj, valid, vv = _inputs("degenerate")
    for b, exc in ((0, AssertionError), (1, AssertionError), (2, ValueError)):
        with pytest.raises(exc, match="need at least two views" if exc is AssertionError else "zero-size array"):
            triangulation(torch.from_numpy(hm[b]).to(dev), torch.from_numpy(proj[b]), c["stride"], torch.from_numpy(valid[b]),
                          view_valid=torch.from_numpy(vv[b]))
    # and a frame that is fine comes back in the reference's types, rows of absent views zero
    c = vm.view_mask_cases()["m4"]
    z = vm.load_golden(NPZ, "m4")
    hm, proj, valid, vv = _inputs("m4")
    r = triangulation(torch.from_numpy(hm[2]).to(dev), torch.from_numpy(proj[2]), c["stride"], torch.from_numpy(valid[2]),
                      reprojection_error_epsilon=vm.EPS, view_valid=vv[2])
    assert isinstance(r["metric"], float) and r["inlier_count"] == z["inlier_count"][2] == 2
    np.testing.assert_array_equal(r["keypoints_2d"], z["keypoints_2d"][2])
    np.testing.assert_allclose(r["keypoints_3d"], z["keypoints_3d"][2], rtol=0, atol=1e-6)


@pytest.mark.parametrize("kp_dtype", [torch.int64, torch.float32], ids=["int64", "float32"])
@pytest.mark.parametrize("name", [n for n in vm.view_mask_cases() if n != "degenerate"])
def test_masked_batch_equals_the_unmasked_call_on_each_frames_present_views(dev, name, kp_dtype):
    """Bit for bit, every output, every frame -- with the reprojection error as metric and with the XE metric.  int64: both
    sides decode the heat-maps; float32: both get the same key-points handed in as float32.  The sliced calls run frame after
    frame from the same seed, so they draw what the batch drew."""
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = vm.view_mask_cases()[name]
    hm, proj, valid, vv = _inputs(name)
    seed = c["rseed"] + 100
    kp = None
    if kp_dtype is torch.float32:
        random.seed(seed)
        kp = _masked(dev, name)["keypoints_2d"].to(torch.float32)
    for xe in (dict(), dict(use_reprojection_xe=True, sigma=1.5)):
        random.seed(seed)
        got = _masked(dev, name, keypoints_2d=kp, **xe)
        assert got["keypoints_2d"].dtype == kp_dtype and not got["keypoints_2d"].cpu().numpy()[~vv].any()
        end = random.getstate()
        random.seed(seed)
        for b in range(c["b"]):
            p = np.flatnonzero(vv[b]).tolist()
            want = triangulate_batch(torch.from_numpy(hm[b : b + 1, p]).to(dev), torch.from_numpy(proj[b : b + 1, p]), c["stride"],
                                     torch.from_numpy(valid[b : b + 1]), n_iters=c["n_iters"], reprojection_error_epsilon=vm.EPS,
                                     pair_rng=random, keypoints_2d=None if kp is None else kp[b : b + 1, p].contiguous(), **xe)
            for k in OUT:
                assert _same_bits(got[k][b : b + 1], want[k]), (k, b, xe)
            assert torch.equal(got["keypoints_2d"][b, p], want["keypoints_2d"][0])
        assert random.getstate() == end


@pytest.mark.parametrize("name", list(vm.view_mask_cases()))
def test_scores_equal_the_unmasked_scorer_on_each_frames_present_views(dev, name):
    """score_heatmaps_batch under HP / MPE / BSB x AVG / STD: the masked value of a frame has the bits of the unmasked
    call on its present views (all four precision paths of mval_score_reduce); no present view or no valid joint: NaN.
    The fused all-kinds call with the mask gives the same values."""
    from multi_view_active_learning_amd.strategy import score_decode_heatmaps_all, score_heatmaps_batch

    c = vm.view_mask_cases()[name]
    hm, _, valid, vv = _inputs(name)
    t, tv, tvv = torch.from_numpy(hm).to(dev), torch.from_numpy(valid), torch.from_numpy(vv)
    for cfg in ("AVG", "STD"):
        fused = score_decode_heatmaps_all({k: cfg for k in ("HP", "MPE", "BSB")}, t, tv, c["stride"], view_valid=tvv)
        for kind in ("HP", "MPE", "BSB"):
            out, per_map, n_peaks, _ = score_heatmaps_batch(kind, cfg, t, tv, view_valid=tvv)
            assert _same_bits(fused[kind][0], out)
            plain = score_heatmaps_batch(kind, cfg, t, tv)
            assert _same_bits(per_map, plain[1]) and torch.equal(n_peaks, plain[2])  # the map kernels do not know the mask
            for b in range(c["b"]):
                p = np.flatnonzero(vv[b]).tolist()
                if len(p) == 0 or not valid[b].any():
                    assert torch.isnan(out[b]).item()
                    continue
                want = score_heatmaps_batch(kind, cfg, t[b : b + 1, p].contiguous(), tv[b : b + 1])[0]
                assert _same_bits(out[b : b + 1], want), (kind, cfg, b)
                if not vv[b].all() and not torch.isnan(out[b]).item():
                    assert not _same_bits(out[b : b + 1], plain[0][b : b + 1]), (kind, cfg, b)  # (the mask matters)


@pytest.mark.parametrize("name", list(vm.view_mask_cases()))
def test_masked_hp_vs_reference_golden(dev, name):
    """mval_score_reduce_masked (MVAL_MASK_VIEWS) against the reference's _compute_hp on the sliced heat-maps, AVG and STD (tolerance of
    test_scoring_vs_reference_golden)."""
    from multi_view_active_learning_amd.strategy import score_heatmaps_batch

    z = vm.load_golden(NPZ, name)
    hm, _, valid, vv = _inputs(name)
    t = torch.from_numpy(hm).to(dev)
    for cfg, key in (("AVG", "hp_avg"), ("STD", "hp_std")):
        got = score_heatmaps_batch("HP", cfg, t, torch.from_numpy(valid), view_valid=torch.from_numpy(vv))[0].cpu().numpy()
        print(name, cfg, got, z[key])
        np.testing.assert_allclose(got, z[key], rtol=3e-6, atol=1e-7, err_msg=cfg)


@pytest.mark.parametrize("name", ["m4", "m32"])
def test_absent_views_may_hold_nan(dev, name):
    """Heat-maps and matrices of the absent views set to NaN: every output, key-points included, and the scores have the
    bits of the run on the clean input -- nothing of an absent view enters arithmetic."""
    from multi_view_active_learning_amd.strategy import score_heatmaps_batch

    c = vm.view_mask_cases()[name]
    hm, proj, valid, vv = _inputs(name)
    bad_hm, bad_proj = hm.copy(), proj.copy()
    bad_hm[~vv] = np.nan
    bad_proj[~vv] = np.nan
    for xe in (dict(), dict(use_reprojection_xe=True, sigma=1.5)):
        random.seed(c["rseed"])
        clean = _masked(dev, name, **xe)
        random.seed(c["rseed"])
        poisoned = _masked(dev, name, hm=bad_hm, proj=bad_proj, **xe)
        for k in OUT + ("keypoints_2d",):
            assert _same_bits(clean[k], poisoned[k]), (k, xe)
            assert not torch.isnan(poisoned[k].to(torch.float64)).any().item(), k
    soft = []
    for h, p in ((hm, proj), (bad_hm, bad_proj)):
        random.seed(c["rseed"])
        soft.append(_masked(dev, name, hm=h, proj=p, use_soft_argmax=True))
    for k in OUT + ("keypoints_2d",):
        assert _same_bits(soft[0][k], soft[1][k]), ("soft arg-max", k)
    assert soft[1]["keypoints_2d"].dtype == torch.float32 and not soft[1]["keypoints_2d"].cpu().numpy()[~vv].any()
    tv, tvv = torch.from_numpy(valid), torch.from_numpy(vv)
    for kind, cfg in (("HP", "AVG"), ("HP", "STD"), ("MPE", "AVG"), ("BSB", "STD")):
        a = score_heatmaps_batch(kind, cfg, torch.from_numpy(hm).to(dev), tv, view_valid=tvv)[0]
        b = score_heatmaps_batch(kind, cfg, torch.from_numpy(bad_hm).to(dev), tv, view_valid=tvv)[0]
        assert _same_bits(a, b) and not torch.isnan(b).any().item(), (kind, cfg)


def test_all_ones_mask_equals_no_mask(dev):
    """Through the masked all-pairs entry (V = 4, 8), the masked table entry with drawn pairs (V = 12, 64 of 66) and with
    all pairs (V = 12, n_iters 128: per-problem tables here, the shared one without a mask): bit for bit, key-points and
    RNG state included.  The scorers and the XE metric likewise."""
    from multi_view_active_learning_amd.strategy import score_heatmaps_batch
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    todo = [(cases.triangulation_cases()["v4_outlier"], 64), (cases.triangulation_cases()["v8_nonsquare"], 64),
            (mv.many_view_cases()["v12_frames"], 64), (mv.many_view_cases()["v12_frames"], 128)]
    for c, n_iters in todo:
        hm, proj, valid = cases.build_triangulation_case(c)
        t, ones = torch.from_numpy(hm).to(dev), torch.ones((c["b"], c["v"]))
        for xe in (dict(), dict(use_reprojection_xe=True, sigma=1.5)):
            res = []
            for mask in (None, ones):
                random.seed(9)
                res.append((triangulate_batch(t, torch.from_numpy(proj), c["stride"], torch.from_numpy(valid), n_iters=n_iters,
                                              pair_rng=random, view_valid=mask, **xe), random.getstate()))
            assert res[0][1] == res[1][1]
            for k in OUT + ("keypoints_2d",):
                assert _same_bits(res[0][0][k], res[1][0][k]), (c["v"], n_iters, k, xe)
        for kind, cfg in (("HP", "AVG"), ("HP", "STD"), ("MPE", "STD"), ("BSB", "AVG")):
            assert _same_bits(score_heatmaps_batch(kind, cfg, t, torch.from_numpy(valid))[0],
                              score_heatmaps_batch(kind, cfg, t, torch.from_numpy(valid), view_valid=ones)[0])


@pytest.mark.parametrize("name", ["m4", "m11"])
def test_masked_all_pairs_entry_equals_the_masked_table_entry(dev, name):
    """V <= 11, MVAL_MASK_VIEWS: mval_triangulate_ransac_masked against mval_triangulate_ransac_pairs_masked with one shared lexicographic
    table of ALL C(V,2) pairs (the entries naming an absent view sit out) and against the padded per-problem tables of
    draw_view_pairs: bit for bit."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import draw_view_pairs

    c = vm.view_mask_cases()[name]
    z = vm.load_golden(NPZ, name)
    _, proj, valid, vv = _inputs(name)
    b, v, j = c["b"], c["v"], c["j"]
    kp, pt = torch.from_numpy(z["keypoints_2d"]).to(dev), torch.from_numpy(proj).to(dev)
    vt, vvt = torch.from_numpy(valid.astype(np.uint8)).to(dev), torch.from_numpy(vv.astype(np.uint8)).to(dev)
    lex = np.array([(a, k) for a in range(v) for k in range(a + 1, v)], np.uint8)
    want = _lib.triangulate_ransac(kp, pt, vt, b, v, j, vm.EPS, view_valid=vvt)
    shared = _lib.triangulate_ransac_pairs(kp, pt, vt, torch.from_numpy(lex[None]).to(dev), b, v, j, vm.EPS, view_valid=vvt)
    own = _lib.triangulate_ransac_pairs(kp, pt, vt, torch.from_numpy(draw_view_pairs(valid, v, 64, None, vv)).to(dev), b, v, j, vm.EPS, view_valid=vvt)
    np.testing.assert_array_equal(want[2].cpu().numpy(), z["joint_inliers"])
    for w, s, o in zip(want, shared, own):
        assert _same_bits(w, s) and _same_bits(w, o)


def _sal_setup(dev, mask=True):
    from multi_view_active_learning_amd.config import get_default_configs

    c = vm.sal_view_mask_case()
    cfg = get_default_configs()
    cfg.AL.STRATEGY = c["strategy"]
    cfg.POSE_ESTIMATOR.STRIDE = c["stride"]
    loader, heatmaps = cases.build_sal_loader(c)
    tl = [{k: torch.from_numpy(v) for k, v in dp.items()} for dp in loader]
    if mask:
        for dp, vv in zip(tl, vm.sal_view_valid(c)):
            dp["view_valid"] = torch.from_numpy(vv.astype(np.float32))

    def model():
        it = iter(heatmaps)
        return lambda images: torch.from_numpy(next(it)).to(dev)

    return c, cfg, tl, model, heatmaps


def _sliced_loader(c, tl, heatmaps, extra=()):
    """One frame per batch, present views only: what the reference would be handed."""
    hh, wh = c["h"] // c["stride"], c["w"] // c["stride"]
    out, maps = [], []
    for dp, hm, vv in zip(tl, heatmaps, vm.sal_view_valid(c)):
        hm = hm.reshape(c["b"], c["v"], c["j"], hh, wh)
        for k in range(c["b"]):
            p = np.flatnonzero(vv[k]).tolist()
            one = {key: val[k : k + 1] for key, val in dp.items() if key != "view_valid"}
            for key in ("images", "proj_matrices") + tuple(extra):
                one[key] = one[key][:, p]
            out.append(one)
            maps.append(np.ascontiguousarray(hm[k][p]))
    return out, maps


def test_sal_dict_on_a_masked_loader_vs_reference_golden(dev):
    """_compute_sal_dict over batches of two frames with different present views against the reference run on one sliced
    frame per batch (tolerances of test_sal_dict_twelve_views_vs_reference_golden), key order and picks; then
    _compute_sal_dicts over all six strategies against the six single-strategy passes, and those against the passes over
    the sliced loader."""
    import math

    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    with open(os.path.join(G, "sal_dict_view_mask.json")) as f:
        want = json.load(f)
    c, cfg, tl, model, heatmaps = _sal_setup(dev)
    random.seed(c["rseed"])
    st = ActiveLearningStrategy(cfg)
    sal = st._compute_sal_dict(tl, model())
    assert mv.state_digest(random.getstate()) == want["state_digest"]
    for field in ("al_metric", "sal_metric", "inlier_count", "mkpe", "pred_3d_keypoints"):
        assert list(sal[field]) == list(want[field]), field
    for g in want["al_metric"]:
        assert abs(sal["al_metric"][g] - want["al_metric"][g]) <= 1e-9 * abs(want["al_metric"][g])
        assert abs(sal["sal_metric"][g] - want["sal_metric"][g]) <= 1e-6 * abs(want["sal_metric"][g])
        assert sal["inlier_count"][g] == want["inlier_count"][g]
        assert np.isnan(sal["mkpe"][g]) and np.isnan(want["mkpe"][g])
        np.testing.assert_allclose(sal["pred_3d_keypoints"][g], want["pred_3d_keypoints"][g], rtol=0, atol=1e-3)
    assert st.select_al_guids(sal, c["select"]) == want["nlargest"]
    assert set(want["inlier_count"].values()) == {2.0, 3.0}  # (an absent view that voted would make one of them 4)

    def same(a, b):
        assert list(a) == list(b)
        for field in a:
            assert list(a[field]) == list(b[field]), field
            for g in a[field]:
                x, y = a[field][g], b[field][g]
                assert x == y or (field == "mkpe" and math.isnan(x) and math.isnan(y)), (field, g)

    torch.manual_seed(5)
    dicts = ActiveLearningStrategy(cfg)._compute_sal_dicts(tl, model(), ALL6)
    sliced, maps = _sliced_loader(c, tl, heatmaps)
    for s in ALL6:
        cfg.AL.STRATEGY = s
        torch.manual_seed(5)
        same(dicts[s], ActiveLearningStrategy(cfg)._compute_sal_dict(tl, model()))
        it = iter(maps)
        torch.manual_seed(5)
        same(dicts[s], ActiveLearningStrategy(cfg)._compute_sal_dict(sliced, lambda images: torch.from_numpy(next(it)).to(dev)))


def test_deferred_checks_know_the_mask(dev):
    """A frame with one present view makes the scoring pass raise the reference's AssertionError (after the pass, like the
    other per-sample errors); the BSB peak check ignores the maps of absent views (flat maps there have no two peaks)."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    c, cfg, tl, model, heatmaps = _sal_setup(dev)
    one = [dict(tl[0], view_valid=torch.tensor([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 1.0, 0.0]]))]
    with pytest.raises(AssertionError, match="need at least two views"):
        ActiveLearningStrategy(cfg)._compute_sal_dict(one, model())
    cfg.AL.STRATEGY = "BSB"
    flat = heatmaps[0].reshape(c["b"], c["v"], c["j"], *heatmaps[0].shape[2:]).copy()
    flat[1, 2] = 0.0  # frame 1, view 2 (absent in batch 0 of the case): no peaks at all
    hm = torch.from_numpy(flat.reshape(heatmaps[0].shape)).to(dev)
    got = ActiveLearningStrategy(cfg)._compute_sal_dict(tl[:1], lambda images: hm)
    assert len(got["al_metric"]) == 2 and not any(np.isnan(x) for x in got["al_metric"].values())
    with pytest.raises(IndexError):
        ActiveLearningStrategy(cfg)._compute_sal_dict([{k: v for k, v in tl[0].items() if k != "view_valid"}], lambda images: hm)


def test_evaluations_on_a_masked_loader_equal_the_sliced_loader(dev):
    """evaluate_mkpe / evaluate_all: the value and the gathered predictions over the masked loader are those over one sliced
    frame per batch.  evaluate_2d_pckh: the fractions over a loader rebuilt without the absent views, S = present images."""
    import pckh2d_cases as pc
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    c, cfg, tl, model, heatmaps = _sal_setup(dev)
    rng = np.random.default_rng(78)
    for dp, hm in zip(tl, heatmaps):  # the two keys the 2-D pass reads, as test_gpu_pckh2d._both_loader makes them
        b, v = dp["images"].shape[:2]
        lt = rng.integers(0, 40, (b, v, 2)).astype(np.float32)
        box = np.concatenate([lt, lt + np.float32(200.0)], axis=-1)
        place = pc.np_pred_coordinates(hm, box.reshape(-1, 4)).reshape(b, v, c["j"], 2)
        dp["square_box"] = torch.from_numpy(box)
        dp["2d_after_crop"] = torch.from_numpy((place + rng.standard_normal(place.shape) * 12.0).astype(np.float32))
    sliced, maps = _sliced_loader(c, tl, heatmaps, extra=("square_box", "2d_after_crop"))
    sliced_model = lambda: (lambda images, it=iter(maps): torch.from_numpy(next(it)).to(dev))  # noqa: E731
    st, ref = ActiveLearningStrategy(cfg), ActiveLearningStrategy(cfg)
    got, want = st.evaluate_mkpe(tl, model()), ref.evaluate_mkpe(sliced, sliced_model())
    assert _same_bits(got, want)
    for a, b_ in zip(st._eval_tables, ref._eval_tables):
        assert _same_bits(a, b_)
    unmasked = ActiveLearningStrategy(cfg)
    unmasked.evaluate_mkpe([{k: v for k, v in dp.items() if k != "view_valid"} for dp in tl], model())
    assert not torch.equal(unmasked._eval_tables[0], st._eval_tables[0])  # (the mask matters on this input)
    all_got, all_want = st.evaluate_all(tl, model()), ref.evaluate_all(sliced, sliced_model())
    assert list(all_got) == list(all_want)
    for k in all_got:
        assert all_got[k] == all_want[k] or (k == "mkpe" and np.isnan(all_got[k]) and np.isnan(all_want[k])), k
    thr, pcks = st.evaluate_2d_pckh(tl, model())
    thr2, pcks2 = ref.evaluate_2d_pckh(sliced, sliced_model())
    assert thr == thr2
    np.testing.assert_array_equal(np.asarray(pcks), np.asarray(pcks2))
    n_present = int(sum(vv.sum() for vv in vm.sal_view_valid(c)))
    assert st._eval2d_tables[0].shape[0] == n_present < c["nbatch"] * c["b"] * c["v"]
    for a, b_ in zip(st._eval2d_tables, ref._eval2d_tables):
        assert torch.equal(a, b_)


def test_draw_reads_the_host_masks_of_a_staged_batch(dev):
    """_stage_batch moves view_valid to the device and keeps the host tensor as view_valid_host (as joint_valid);
    triangulate_batch with the device masks plus the host copies draws and computes what it does with the host masks."""
    from multi_view_active_learning_amd.strategy import _stage_batch
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = vm.view_mask_cases()["m12_mixed"]
    hm, proj, valid, vv = _inputs("m12_mixed")
    host, host_vv = torch.from_numpy(valid.astype(np.float32)), torch.from_numpy(vv.astype(np.float32))
    dp = _stage_batch(dict(joint_valid=host, view_valid=host_vv, proj_matrices=torch.from_numpy(proj)))
    assert dp["view_valid"].is_cuda and dp["view_valid_host"] is host_vv and dp["joint_valid_host"] is host
    out = []
    for kw in (dict(valid_joints=dp["joint_valid"], valid_joints_host=dp["joint_valid_host"], view_valid=dp["view_valid"],
                    view_valid_host=dp["view_valid_host"]), dict(valid_joints=host, view_valid=host_vv)):
        random.seed(3)
        r = triangulate_batch(torch.from_numpy(hm).to(dev), dp["proj_matrices"], c["stride"], n_iters=c["n_iters"],
                              pair_rng=random, **kw)
        out.append((r, random.getstate()))
    assert out[0][1] == out[1][1]
    for k in OUT + ("keypoints_2d",):
        assert _same_bits(out[0][0][k], out[1][0][k])


def test_entries_refuse_bad_arguments_and_launch_nothing(dev):
    """V > 32 (V > 11 for the all-pairs entry), V < 2, a NULL mask and a mask_kind that is none or does not go with the mask
    pointer: the documented error, a message, and output buffers that keep their sentinel values.  The wrappers raise; triangulate_batch names the limit."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    b, v, j, p = 2, 33, 5, 64
    kp = torch.zeros((b, v, j, 2), dtype=torch.int64, device=dev)
    proj = torch.ones((b, v, 3, 4), dtype=torch.float64, device=dev)
    pairs = torch.zeros((b, j, p, 2), dtype=torch.uint8, device=dev)
    pairs[..., 1] = 1
    vvt = torch.ones((b, v), dtype=torch.uint8, device=dev)
    per_map = torch.zeros((b * v * j,), dtype=torch.float32, device=dev)
    hm = torch.zeros((b, v, j, 8, 8), dtype=torch.float32, device=dev)
    k3 = torch.full((b, j, 3), -7.0, dtype=torch.float64, device=dev)
    jerr = torch.full((b, j), -7.0, dtype=torch.float64, device=dev)
    jinl = torch.full((b, j), -7, dtype=torch.int32, device=dev)
    metric = torch.full((b,), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((b,), -7, dtype=torch.int32, device=dev)
    ws = torch.full((b * v * j,), -7.0, dtype=torch.float64, device=dev)
    P, N = _lib._p, _lib._p(None)
    outs = (P(k3), P(jerr), P(jinl), P(metric), P(cnt))
    K, NULL_MASK = _lib.MASK_VIEWS, "a mask goes with mask_kind 1 or 2, NULL with 0"
    views, table = _lib._views_entry("mval_triangulate_ransac_masked"), _lib._views_entry("mval_triangulate_ransac_pairs_masked")
    xe, red = _lib._views_entry("mval_reprojection_xe_masked"), _lib._views_entry("mval_score_reduce_masked")
    for vv_, mask, word in ((33, P(vvt), "32"), (1, P(vvt), "2 views"), (12, N, NULL_MASK)):
        assert table(P(kp), 0, P(proj), N, mask, K, P(pairs), p, 0, *outs, b, vv_, j, 5.0, _lib._stream()) != 0
        assert word in _lib.lib().mval_last_error().decode(), (vv_, word)
    for vv_, mask, word in ((33, P(vvt), "V > 11"), (12, P(vvt), "V > 11"), (1, P(vvt), "2 views"), (4, N, NULL_MASK)):
        assert views(P(kp), 0, P(proj), N, mask, K, *outs, b, vv_, j, 5.0, _lib._stream()) != 0
        assert word in _lib.lib().mval_last_error().decode(), (vv_, word)
    assert xe(P(k3), P(proj), P(hm), N, K, P(metric), P(ws), b, 4, j, 8, 8, 1.0, _lib._stream()) != 0
    assert NULL_MASK in _lib.lib().mval_last_error().decode()
    assert red(P(per_map), N, N, K, P(metric), b, 4, j, 0, _lib._stream()) != 0
    assert NULL_MASK in _lib.lib().mval_last_error().decode()
    # the mask_kind contract of every `_masked` entry: a kind outside 0..2, MVAL_MASK_NONE with a mask, a mask kind with NULL
    for mask, kind, word in ((P(vvt), 3, "mask_kind 3"), (P(vvt), _lib.MASK_NONE, NULL_MASK), (N, _lib.MASK_VIEWS, NULL_MASK),
                             (N, _lib.MASK_VIEW_JOINT, NULL_MASK)):
        for name, call in (("mval_triangulate_ransac_masked", lambda: views(P(kp), 0, P(proj), N, mask, kind, *outs, b, 4, j, 5.0, _lib._stream())),
                           ("mval_triangulate_ransac_pairs_masked", lambda: table(P(kp), 0, P(proj), N, mask, kind, P(pairs), p, 0, *outs, b, 12, j, 5.0, _lib._stream())),
                           ("mval_reprojection_xe_masked", lambda: xe(P(k3), P(proj), P(hm), mask, kind, P(metric), P(ws), b, 4, j, 8, 8, 1.0, _lib._stream())),
                           ("mval_score_reduce_masked", lambda: red(P(per_map), N, mask, kind, P(metric), b, 4, j, 0, _lib._stream()))):
            assert call() != 0, (name, kind)
            msg = _lib.lib().mval_last_error().decode()
            assert name in msg and word in msg, (name, kind, msg)
    torch.cuda.synchronize()
    for t in (k3, jerr, jinl, metric, cnt, ws):
        assert (t == -7).all().item()
    with pytest.raises(_lib.MvalError, match="32"):
        _lib.triangulate_ransac_pairs(kp, proj, None, pairs, b, v, j, 5.0, view_valid=vvt)
    with pytest.raises(_lib.MvalError, match="view_valid"):
        _lib.triangulate_ransac(kp[:, :4].contiguous(), proj[:, :4].contiguous(), None, b, 4, j, 5.0, view_valid=vvt)  # (B, 33) mask
    for rng in (None, random):
        with pytest.raises(NotImplementedError, match="32"):
            triangulate_batch(torch.zeros((b, v, j, 8, 8), device=dev), proj, 4, torch.ones((b, j)), pair_rng=rng, view_valid=vvt)

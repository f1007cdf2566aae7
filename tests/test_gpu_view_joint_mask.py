"""GPU tests of per-(view, joint) visibility (``view_joint_valid``, MVAL_MASK_VIEW_JOINT): the `_masked` triangulation entries,
mval_score_reduce_masked, mval_reprojection_xe_masked, mval_peak_mask, and the calls that carry the mask (triangulate_batch, triangulation, the heat-map
scorers, the scoring and evaluation passes, the two config fields).

Two oracles.  (1) The real reference's ``_triangulate_ransac`` handed each joint's present views (tests/golden/
view_joint_mask.npz, make_view_joint_mask_golden.py), under the tolerances test_gpu_view_mask.py holds the frame mask to:
key-points, inlier counts, pair tables and RNG digests exact, 3-D points 1e-6 mm, errors and metric 1e-9 relative, HP 3e-6
relative.  No problem is left out: every vote of every problem is decidable.  (2) Today's unmasked calls on a problem's own
slice (B = 1, J = 1, the joint's present views), bit for bit."""
import os
import random

import numpy as np
import pytest
import torch

import cases
import many_view_cases as mv
import view_joint_mask_cases as vjc
import view_mask_cases as vm

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
NPZ = os.path.join(G, "view_joint_mask.npz")
OUT = ("keypoints_3d", "joint_error", "joint_inliers", "metric", "inlier_count")
NAMES = list(vjc.view_joint_mask_cases())


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


_INPUTS = {}


def _inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = vjc.build(vjc.view_joint_mask_cases()[name])
    return _INPUTS[name]


def _same_bits(a, b):
    """torch.equal that takes NaN for what it is: the same bits."""
    if a.dtype.is_floating_point:
        as_int = torch.int64 if a.dtype == torch.float64 else torch.int32
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))
    return a.dtype == b.dtype and torch.equal(a, b)


def _masked(dev, name, hm=None, **kw):
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = vjc.view_joint_mask_cases()[name]
    hm0, proj, valid, mask = _inputs(name)
    return triangulate_batch(torch.from_numpy(hm0 if hm is None else hm).to(dev), torch.from_numpy(proj), c["stride"],
                             torch.from_numpy(valid), n_iters=c["n_iters"], reprojection_error_epsilon=vjc.EPS, pair_rng=random,
                             view_joint_valid=torch.from_numpy(mask), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_triangulate_batch_vs_reference_golden(dev, name):
    """Check 1.  j4 (4, 3, 2, 1 and 0 present views beside each other, an invalid joint, a frame without a used joint: -2,
    one without a valid joint: -1), j8_nonsquare (first and last bit), j11 (55-pair group), j12_mixed (ONE frame with joints
    that draw 64 of 66, that walk 55 and 45 lexicographic pairs: padded per-problem tables), j32 (bit 31).  The RNG ends where
    the reference's per-joint calls left it; absent key-point entries are zero; joint_used is the mask of the joints handed
    to the reference."""
    from multi_view_active_learning_amd.strategy import score_heatmaps_batch

    c = vjc.view_joint_mask_cases()[name]
    z = vjc.load_golden(NPZ, name)
    hm, _, valid, mask = _inputs(name)
    random.seed(int(z["rseed"]))
    before = random.getstate()
    r = _masked(dev, name)
    assert vjc.state_digest(random.getstate()) == str(z["frame_digests"][-1])
    if not vjc.draws(c).any():
        assert random.getstate() == before
    got = {k: t.cpu().numpy() for k, t in r.items()}
    assert not got["keypoints_2d"][~mask].any()
    np.testing.assert_array_equal(got["keypoints_2d"], z["keypoints_2d"])
    np.testing.assert_array_equal(got["joint_inliers"], z["joint_inliers"])
    np.testing.assert_array_equal(got["inlier_count"], z["inlier_count"])
    assert got["joint_used"].dtype == np.uint8
    np.testing.assert_array_equal(got["joint_used"].astype(bool), vjc.used(c))
    assert (got["joint_inliers"][vjc.used(c)] >= 2).all()
    print("max |kp3d - reference| = %.3e mm" % np.abs(got["keypoints_3d"] - z["keypoints_3d"]).max())
    np.testing.assert_allclose(got["keypoints_3d"], z["keypoints_3d"], rtol=0, atol=1e-6)
    assert not got["keypoints_3d"][~vjc.used(c)].any() and not got["joint_error"][~vjc.used(c)].any()
    np.testing.assert_allclose(got["joint_error"], z["joint_error"], rtol=1e-9)
    np.testing.assert_allclose(got["metric"], z["metric"], rtol=1e-9)
    assert np.isnan(got["metric"][z["inlier_count"] < 0]).all()
    t = torch.from_numpy(hm).to(dev)
    for cfg, key in (("AVG", "hp_avg"), ("STD", "hp_std")):
        out, per_map, _, _ = score_heatmaps_batch("HP", cfg, t, torch.from_numpy(valid), view_joint_valid=torch.from_numpy(mask))
        print(name, cfg, out.cpu().numpy(), z[key])
        np.testing.assert_allclose(out.cpu().numpy(), z[key], rtol=3e-6, atol=1e-7, err_msg=cfg)
        listed = ~np.isnan(z["hp_map"])
        np.testing.assert_array_equal(listed, mask & valid[:, None, :])
        np.testing.assert_allclose(per_map.cpu().numpy()[listed], z["hp_map"][listed], rtol=3e-6, atol=1e-7)


@pytest.mark.parametrize("name", NAMES)
def test_every_used_problem_equals_the_unmasked_call_on_its_slice(dev, name):
    """Check 2.  Bit for bit: keypoints_3d, joint_error, joint_inliers of every used problem against today's unmasked
    triangulate_batch on B = 1, J = 1 and the joint's present views.  The slices run in problem order from the batch's seed,
    so a slice that draws draws what the batch drew for it."""
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = vjc.view_joint_mask_cases()[name]
    hm, proj, valid, mask = _inputs(name)
    seed = c["rseed"] + 100
    random.seed(seed)
    got = _masked(dev, name)
    end = random.getstate()
    t, one = torch.from_numpy(hm).to(dev), torch.ones((1, 1))
    random.seed(seed)
    n = 0
    for b, j in zip(*np.nonzero(vjc.used(c))):
        p = np.flatnonzero(mask[b, :, j]).tolist()
        want = triangulate_batch(t[b : b + 1, p, j : j + 1].contiguous(), torch.from_numpy(proj[b : b + 1, p]), c["stride"], one,
                                 n_iters=c["n_iters"], reprojection_error_epsilon=vjc.EPS, pair_rng=random)
        for k in ("keypoints_3d", "joint_error", "joint_inliers"):
            assert _same_bits(got[k][b : b + 1, j : j + 1], want[k]), (k, b, j, p)
        assert torch.equal(got["keypoints_2d"][b, p, j], want["keypoints_2d"][0, :, 0])
        n += 1
    assert random.getstate() == end and n == int(vjc.used(c).sum()) > 0


@pytest.mark.parametrize("name", ["m4", "m12_mixed", "degenerate"])
def test_broadcast_mask_equals_the_view_valid_call(dev, name):
    """Check 3a.  view_joint_valid = view_valid[:, :, None].expand(B, V, J): every output and the RNG state of the
    ``view_valid`` call, at V = 4 (all-pairs entry; ``degenerate``: the -2 / -1 codes) and V = 12 (table entry, drawn pairs),
    with the reprojection error and with the XE metric; the scorers likewise.  Also with the frame mask beside an all-ones
    joint mask: the two are ANDed."""
    from multi_view_active_learning_amd.strategy import score_heatmaps_batch
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = vm.view_mask_cases()[name]
    hm, proj, valid, vv = vm.build(c)
    t, tv, tvv = torch.from_numpy(hm).to(dev), torch.from_numpy(valid), torch.from_numpy(vv)
    wide = tvv[:, :, None].expand(c["b"], c["v"], c["j"])
    for xe in (dict(), dict(use_reprojection_xe=True, sigma=1.5)):
        res = []
        for kw in (dict(view_valid=tvv), dict(view_joint_valid=wide), dict(view_valid=tvv, view_joint_valid=torch.ones_like(wide))):
            random.seed(9)
            r = triangulate_batch(t, torch.from_numpy(proj), c["stride"], tv, n_iters=c["n_iters"], reprojection_error_epsilon=vm.EPS,
                                  pair_rng=random, **kw, **xe)
            res.append((r, random.getstate()))
        for r, state in res[1:]:
            assert state == res[0][1]
            for k in OUT + ("keypoints_2d",):
                assert _same_bits(res[0][0][k], r[k]), (name, k, xe)
    for kind, cfg in (("HP", "AVG"), ("HP", "STD"), ("MPE", "STD"), ("BSB", "AVG")):
        assert _same_bits(score_heatmaps_batch(kind, cfg, t, tv, view_valid=tvv)[0],
                          score_heatmaps_batch(kind, cfg, t, tv, view_joint_valid=wide)[0]), (kind, cfg)


def test_all_ones_mask_equals_no_mask(dev):
    """Check 3b.  Through mval_triangulate_ransac_masked (V = 4) and mval_triangulate_ransac_pairs_masked with drawn pairs (V = 12, 64
    of 66) and with all pairs (V = 12, n_iters 128): bit for bit, key-points and RNG state included; the scorers and the XE
    metric likewise."""
    from multi_view_active_learning_amd.strategy import score_heatmaps_batch
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    todo = [(cases.triangulation_cases()["v4_outlier"], 64), (mv.many_view_cases()["v12_frames"], 64), (mv.many_view_cases()["v12_frames"], 128)]
    for c, n_iters in todo:
        hm, proj, valid = cases.build_triangulation_case(c)
        t, ones = torch.from_numpy(hm).to(dev), torch.ones((c["b"], c["v"], c["j"]))
        for xe in (dict(), dict(use_reprojection_xe=True, sigma=1.5)):
            res = []
            for mask in (None, ones):
                random.seed(9)
                res.append((triangulate_batch(t, torch.from_numpy(proj), c["stride"], torch.from_numpy(valid), n_iters=n_iters,
                                              pair_rng=random, view_joint_valid=mask, **xe), random.getstate()))
            assert res[0][1] == res[1][1]
            assert "joint_used" not in res[0][0] and res[1][0]["joint_used"].cpu().numpy().astype(bool).tolist() == valid.tolist()
            for k in OUT + ("keypoints_2d",):
                assert _same_bits(res[0][0][k], res[1][0][k]), (c["v"], n_iters, k, xe)
        for kind, cfg in (("HP", "AVG"), ("HP", "STD"), ("MPE", "STD"), ("BSB", "AVG")):
            assert _same_bits(score_heatmaps_batch(kind, cfg, t, torch.from_numpy(valid))[0],
                              score_heatmaps_batch(kind, cfg, t, torch.from_numpy(valid), view_joint_valid=ones)[0])


@pytest.mark.parametrize("name", ["j4", "j32"])
def test_absent_entries_may_hold_nan(dev, name):
    """Check 4.  NaN in every absent entry's heat-map: every output, key-points included, and the scores have the bits of the
    run on the clean input.  NaN in every absent entry's key-point row, handed straight to the entry (float32 key-points): the
    same outputs again -- nothing of an absent entry enters arithmetic."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import score_heatmaps_batch
    from multi_view_active_learning_amd.utils.triangulation import draw_view_pairs

    c = vjc.view_joint_mask_cases()[name]
    hm, proj, valid, mask = _inputs(name)
    assert not mask.all()
    bad = hm.copy()
    bad[~mask] = np.nan
    for xe in (dict(), dict(use_reprojection_xe=True, sigma=1.5)):
        random.seed(c["rseed"])
        clean = _masked(dev, name, **xe)
        random.seed(c["rseed"])
        poisoned = _masked(dev, name, hm=bad, **xe)
        for k in OUT + ("keypoints_2d", "joint_used"):
            assert _same_bits(clean[k], poisoned[k]), (k, xe)
        assert not torch.isnan(poisoned["keypoints_3d"]).any().item() and not torch.isnan(poisoned["joint_error"]).any().item()
    soft = []
    for h in (hm, bad):
        random.seed(c["rseed"])
        soft.append(_masked(dev, name, hm=h, use_soft_argmax=True))
    for k in OUT + ("keypoints_2d",):
        assert _same_bits(soft[0][k], soft[1][k]), ("soft arg-max", k)
    tv, tm = torch.from_numpy(valid), torch.from_numpy(mask)
    for kind, cfg in (("HP", "AVG"), ("HP", "STD"), ("MPE", "AVG"), ("BSB", "STD")):
        a = score_heatmaps_batch(kind, cfg, torch.from_numpy(hm).to(dev), tv, view_joint_valid=tm)[0]
        b = score_heatmaps_batch(kind, cfg, torch.from_numpy(bad).to(dev), tv, view_joint_valid=tm)[0]
        assert _same_bits(a, b), (kind, cfg)
    # the entries themselves, key-point rows poisoned
    b_, v, j = c["b"], c["v"], c["j"]
    random.seed(c["rseed"])
    kp = _masked(dev, name)["keypoints_2d"].to(torch.float32)
    kp_bad = torch.where(torch.from_numpy(mask).to(dev)[..., None], kp, torch.full_like(kp, float("nan")))
    pt = torch.from_numpy(proj).to(dev)
    vt, mt = torch.from_numpy(valid.astype(np.uint8)).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
    if v <= 11:
        call = lambda k: _lib.triangulate_ransac(k, pt, vt, b_, v, j, vjc.EPS, view_joint_valid=mt)  # noqa: E731
    else:
        pairs = torch.from_numpy(draw_view_pairs(valid, v, c["n_iters"], random.Random(1), view_joint_valid=mask)).to(dev)
        call = lambda k: _lib.triangulate_ransac_pairs(k, pt, vt, pairs, b_, v, j, vjc.EPS, view_joint_valid=mt)  # noqa: E731
    clean, poisoned = call(kp), call(kp_bad.contiguous())
    for x, y in zip(clean, poisoned):
        assert _same_bits(x, y)
    assert not torch.isnan(poisoned[0]).any().item() and not torch.isnan(poisoned[1]).any().item()


def test_score_reduce_vj_equals_score_reduce_on_the_compacted_list(dev):
    """Check 5.  All four modes (AVG / STD x float64 / float32): a frame's value has the bits of mval_score_reduce called
    with V = 1, J = n on its present entries of valid joints in view-major order; n = 0 gives NaN."""
    from multi_view_active_learning_amd import _lib

    b, v, j = 4, 5, 19
    rng = np.random.default_rng(12)
    per_map = torch.from_numpy(rng.standard_normal((b, v, j)).astype(np.float32) * np.float32(3.0)).to(dev)
    valid = np.ones((b, j), dtype=bool)
    valid[:, [2, 7]] = False
    mask = rng.random((b, v, j)) < 0.6
    mask[1] = True  # (a frame with every entry)
    mask[2][:, valid[2]] = False  # (none left: the entries of invalid joints do not count)
    mask[3] = False
    mask[3, 4, 18] = True  # (n = 1)
    vt, mt = torch.from_numpy(valid.astype(np.uint8)).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
    for mode in (_lib.REDUCE_AVG_F64, _lib.REDUCE_AVG_F32, _lib.REDUCE_STD_F64, _lib.REDUCE_STD_F32):
        got = _lib.score_reduce(per_map.reshape(-1), vt, b, v, j, mode, view_joint_valid=mt)
        for f in range(b):
            keep = torch.from_numpy(mask[f] & valid[f][None, :]).to(dev)
            vals = per_map[f][keep].contiguous()  # (row-major: views outer, joints inner)
            if vals.numel() == 0:
                assert f == 2 and torch.isnan(got[f]).item()
                continue
            want = _lib.score_reduce(vals, None, 1, 1, vals.numel(), mode)
            assert _same_bits(got[f : f + 1], want), (mode, f)
        plain = _lib.score_reduce(per_map.reshape(-1), vt, b, v, j, mode)
        assert _same_bits(got[1:2], plain[1:2]) and not _same_bits(got[:1], plain[:1])


def test_reprojection_xe_vj_equals_the_serial_sum_over_present_entries(dev):
    """Check 6.  Same bits as the float64 left-to-right host sum of single-map ``reprojection_xe`` calls over the present
    entries in view-major, joint-minor order (B = 3, V = 4, J = 19: case j4); through triangulate_batch a frame without a used
    joint keeps NaN."""
    from multi_view_active_learning_amd import _lib

    c = vjc.view_joint_mask_cases()["j4"]
    hm, proj, _, mask = _inputs("j4")
    b, v, j, hh, wh = hm.shape
    sigma = 1.5
    r = _masked(dev, "j4", use_reprojection_xe=True, sigma=sigma)
    plain = _masked(dev, "j4")
    assert r["inlier_count"].tolist() == [2, -2, -1]
    t, pt, mt = torch.from_numpy(hm).to(dev), torch.from_numpy(proj).to(dev), torch.from_numpy(mask.astype(np.uint8)).to(dev)
    kp3d = plain["keypoints_3d"]
    got = _lib.reprojection_xe(kp3d, pt, t, b, v, j, hh, wh, sigma, view_joint_valid=mt).cpu().numpy()
    for f in range(b):
        s = 0.0
        for vi in range(v):
            for ji in range(j):
                if mask[f, vi, ji]:
                    s += _lib.reprojection_xe(kp3d[f : f + 1, ji : ji + 1].contiguous(), pt[f : f + 1, vi : vi + 1].contiguous(),
                                              t[f : f + 1, vi : vi + 1, ji : ji + 1].contiguous(), 1, 1, 1, hh, wh, sigma).item()
        assert np.float64(s).tobytes() == got[f].tobytes(), (f, s, got[f])
    metric = r["metric"].cpu().numpy()
    assert metric[0].tobytes() == got[0].tobytes() and np.isnan(metric[1]) and metric[2].tobytes() == got[2].tobytes()
    assert got[0] != _lib.reprojection_xe(kp3d, pt, t, b, v, j, hh, wh, sigma)[0].item()  # (the mask matters)


@pytest.mark.parametrize("shape,offset", [((1, 3, 5, 64, 64), 0), ((2, 2, 3, 64, 48), 0), ((1, 1, 7, 7, 5), 0), ((1, 2, 3, 64, 64), 1)],
                         ids=["64x64", "64x48", "7x5_scalar", "64x64_unaligned"])
def test_peak_mask_equals_torch(dev, shape, offset):
    """Check 7.  Equal to ``(hm >= t).flatten(-2).any(-1)``: a threshold equal to one map's maximum (that map is in, lower maps
    are out), a map of NaNs (out), a map whose only hit is its first / its last element (the float4 body and the scalar tail),
    a map one ulp short everywhere (out), map counts that are no multiple of 4 (15, 7, 6) and one that is (12), and maps that
    start 4 bytes off a 16-byte boundary (scalar loads although 64 * 64 is a multiple of 4)."""
    from multi_view_active_learning_amd.utils.triangulation import peak_mask

    rng = np.random.default_rng(sum(shape))
    hm = rng.standard_normal(shape).astype(np.float32)
    flat = hm.reshape(-1, shape[3] * shape[4])
    thr = float(np.sort(flat.max(axis=1))[flat.shape[0] // 2])  # the maximum of the middle map, exactly
    flat[0] = np.nan
    flat[1] = -5.0
    flat[1, 0] = thr
    flat[2] = -5.0
    flat[2, -1] = thr
    flat[3] = np.float32(np.nextafter(np.float32(thr), np.float32(-np.inf)))  # one ulp short everywhere
    t = torch.from_numpy(hm).to(dev)
    if offset:
        buf = torch.empty((t.numel() + offset,), dtype=torch.float32, device=dev)
        buf[offset:] = t.reshape(-1)
        t = buf[offset:].view(shape)
        assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset
    for min_peak in (thr, 0.0, -np.inf, np.inf, 1e9):
        got = peak_mask(t, min_peak)
        want = (t >= min_peak).flatten(-2).any(-1)
        assert got.dtype == torch.uint8 and got.shape == shape[:3] and got.is_cuda
        assert torch.equal(got.bool(), want), min_peak
    got = peak_mask(t, thr).reshape(-1).tolist()
    assert got[:4] == [0, 1, 1, 0] and 0 < sum(got) < len(got)


def _sal_setup(dev):
    from multi_view_active_learning_amd.config import get_default_configs

    c = vm.sal_view_mask_case()
    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = c["stride"]
    loader, heatmaps = cases.build_sal_loader(c)
    tl = [{k: torch.from_numpy(v) for k, v in dp.items()} for dp in loader]
    rng = np.random.default_rng(5)
    masks = []
    for n in range(c["nbatch"]):
        m = rng.random((c["b"], c["v"], c["j"])) < 0.85
        m[:, :2, 0] = True  # (every frame keeps a used joint)
        masks.append(m)
    masks[0][0, :3, 2] = False  # batch 0, frame 0, joint 2: one view left -> not used
    masks[1][1, :, 5] = False  # batch 1, frame 1, joint 5: no view left

    def model():
        it = iter(heatmaps)
        return lambda images: torch.from_numpy(next(it)).to(dev)

    return c, cfg, tl, masks, model, heatmaps


@pytest.mark.parametrize("strategy", ["TRIANGULATION", "HP"])
def test_sal_dict_with_the_named_key(dev, strategy):
    """Check 8.  _compute_sal_dict with AL.VIEW_JOINT_VALID_KEY = "per_view_joint_valid" equals the per-batch score_batch tables
    (the mask handed over as the batch's own ``view_joint_valid``, default config) assembled by hand, whose columns are the
    masked triangulate_batch / scorer / MKPE over ``joint_valid & joint_used``; under the default config the sal_dict is
    bit-identical to the one of batches without the key."""
    import math

    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy, score_heatmaps_batch, tables_to_sal_dict
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c, cfg, tl, masks, model, heatmaps = _sal_setup(dev)
    cfg.AL.STRATEGY = strategy
    keyed = [dict(dp, per_view_joint_valid=torch.from_numpy(m.astype(np.float32))) for dp, m in zip(tl, masks)]
    own = [dict(dp, view_joint_valid=torch.from_numpy(m)) for dp, m in zip(tl, masks)]

    def same(a, b):
        assert list(a) == list(b)
        for field in a:
            assert list(a[field]) == list(b[field]), field
            for g in a[field]:
                x, y = a[field][g], b[field][g]
                assert x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y)), (field, g)

    plain = ActiveLearningStrategy(cfg)._compute_sal_dict(tl, model())
    same(plain, ActiveLearningStrategy(cfg)._compute_sal_dict(keyed, model()))  # default config: the key is not looked at
    st = ActiveLearningStrategy(cfg)
    st._pending_checks = []
    tables = []
    for dp, hm, m in zip(own, heatmaps, masks):
        t = torch.from_numpy(hm).to(dev)
        tab = st.score_batch(t, dp)
        tables.append(tab.cpu().numpy())
        b, j = c["b"], c["j"]
        hm5 = t.reshape(b, c["v"], j, *t.shape[2:])
        r = triangulate_batch(hm5, dp["proj_matrices"], c["stride"], dp["joint_valid"].reshape(b, j), view_joint_valid=torch.from_numpy(m))
        jv = (dp["joint_valid"].reshape(b, j) != 0).to(dev)
        used = jv & r["joint_used"].bool()
        assert torch.equal(used.cpu(), jv.cpu() & torch.from_numpy(m.sum(axis=1) >= 2))
        assert not torch.equal(used, jv) and (r["inlier_count"] >= 2).all().item()
        pred32 = r["keypoints_3d"].to(torch.float32)
        _, per = _lib.mkpe(pred32.contiguous(), dp["3d_keypoints"].to(dev, torch.float32).contiguous(), used.to(torch.float32).contiguous(),
                           b, j, dp["3d_keypoints"].shape[1])
        assert _same_bits(tab[:, 5], per.to(torch.float64)) and _same_bits(tab[:, 4], r["inlier_count"].to(torch.float64))
        assert _same_bits(tab[:, 6:], pred32.to(torch.float64).reshape(b, 3 * j))
        if strategy == "TRIANGULATION":
            assert _same_bits(tab[:, 2], r["metric"])
        else:
            al = score_heatmaps_batch("HP", cfg.AL.HP_CONFIG, hm5, dp["joint_valid"].reshape(b, j), view_joint_valid=torch.from_numpy(m))[0]
            assert _same_bits(tab[:, 2], al.to(torch.float32).to(torch.float64))
    want = tables_to_sal_dict([np.concatenate(tables)], [c["b"]] * c["nbatch"])
    cfg.AL.VIEW_JOINT_VALID_KEY = "per_view_joint_valid"
    got = ActiveLearningStrategy(cfg)._compute_sal_dict(keyed, model())
    same(got, want)
    assert any(got["al_metric"][g] != plain["al_metric"][g] for g in got["al_metric"])  # (the mask matters on this input)
    with pytest.raises(KeyError, match="per_view_joint_valid"):
        ActiveLearningStrategy(cfg)._compute_sal_dict(tl, model())


def test_evaluate_mkpe_leaves_unused_joints_out(dev):
    """Check 8, evaluation: the validity column evaluate_mkpe gathers is ``joint_valid & joint_used`` and its value is
    ``_lib.mkpe`` on that; a joint nobody triangulated is not scored as a prediction at the origin."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c, cfg, tl, masks, model, heatmaps = _sal_setup(dev)
    cfg.AL.VIEW_JOINT_VALID_KEY = "per_view_joint_valid"
    keyed = [dict(dp, per_view_joint_valid=torch.from_numpy(m.astype(np.float32))) for dp, m in zip(tl, masks)]
    st = ActiveLearningStrategy(cfg)
    got = st.evaluate_mkpe(keyed, model())
    pred, gt, valid = st._eval_tables
    b, j = c["b"], c["j"]
    used = []
    for dp, hm, m in zip(tl, heatmaps, masks):
        t = torch.from_numpy(hm).to(dev)
        r = triangulate_batch(t.reshape(b, c["v"], j, *t.shape[2:]), dp["proj_matrices"], c["stride"], dp["joint_valid"].reshape(b, j),
                              view_joint_valid=torch.from_numpy(m))
        used.append((dp["joint_valid"].reshape(b, j) != 0).to(dev) & r["joint_used"].bool())
    used = torch.cat(used).to(torch.float32)
    jv = torch.cat([dp["joint_valid"].reshape(b, j) for dp in tl]).to(dev, torch.float32)
    assert torch.equal(valid.to(dev), used) and int((used == 0).sum().item()) > int((jv == 0).sum().item())
    want, _ = _lib.mkpe(pred.to(dev).contiguous(), gt.to(dev).contiguous(), used.contiguous(), pred.shape[0], j, gt.shape[1])
    assert _same_bits(got.to(dev), want)
    off = ActiveLearningStrategy(cfg)
    cfg.AL.VIEW_JOINT_VALID_KEY = ""
    assert not _same_bits(off.evaluate_mkpe(keyed, model()).to(dev), want)  # (key off: every joint scored, as ever)
    assert torch.equal(off._eval_tables[2].to(dev), jv)


def test_triangulation_one_frame(dev):
    """Check 9.  ``triangulation`` on one frame of j4: a valid joint but no used one raises the reference's AssertionError, no
    valid joint its ValueError; a frame that is fine comes back in the reference's types, absent entries zero."""
    from multi_view_active_learning_amd.utils.triangulation import triangulation

    c = vjc.view_joint_mask_cases()["j4"]
    z = vjc.load_golden(NPZ, "j4")
    hm, proj, valid, mask = _inputs("j4")
    for b, exc in ((1, AssertionError), (2, ValueError)):
        with pytest.raises(exc, match="need at least two views" if exc is AssertionError else "zero-size array"):
            triangulation(torch.from_numpy(hm[b]).to(dev), torch.from_numpy(proj[b]), c["stride"], torch.from_numpy(valid[b]),
                          view_joint_valid=torch.from_numpy(mask[b]))
    r = triangulation(torch.from_numpy(hm[0]).to(dev), torch.from_numpy(proj[0]), c["stride"], torch.from_numpy(valid[0]),
                      reprojection_error_epsilon=vjc.EPS, view_joint_valid=mask[0])
    assert set(r) == {"keypoints_3d", "keypoints_2d", "metric", "inlier_count"}
    assert isinstance(r["metric"], float) and isinstance(r["inlier_count"], int) and r["inlier_count"] == z["inlier_count"][0] == 2
    assert isinstance(r["keypoints_3d"], np.ndarray) and r["keypoints_3d"].dtype == np.float64 and r["keypoints_2d"].dtype == np.int64
    np.testing.assert_array_equal(r["keypoints_2d"], z["keypoints_2d"][0])
    np.testing.assert_allclose(r["keypoints_3d"], z["keypoints_3d"][0], rtol=0, atol=1e-6)
    np.testing.assert_allclose(r["metric"], z["metric"][0], rtol=1e-9)


def test_staged_masks_and_the_peak_gate(dev):
    """_stage_batch moves view_joint_valid (and a named key) to the device and keeps the host tensor as ``<key>_host``;
    triangulate_batch at V = 12 with the device mask plus the host copy, with the device mask alone (copied back) and with
    the host mask draws and computes the same.  AL.MIN_PEAK: the resolved mask is the named key AND the peak gate, it has no
    host copy, and a scoring pass under it equals the pass handed that mask as ``view_joint_valid``."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy, _stage_batch
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = vjc.view_joint_mask_cases()["j12_mixed"]
    hm, proj, valid, mask = _inputs("j12_mixed")
    host_v, host_m = torch.from_numpy(valid.astype(np.float32)), torch.from_numpy(mask.astype(np.float32))
    dp = _stage_batch(dict(joint_valid=host_v, view_joint_valid=host_m, per_view_joint_valid=host_m, proj_matrices=torch.from_numpy(proj)),
                      ("per_view_joint_valid",))
    assert dp["view_joint_valid"].is_cuda and dp["view_joint_valid_host"] is host_m
    assert dp["per_view_joint_valid"].is_cuda and dp["per_view_joint_valid_host"] is host_m
    assert "per_view_joint_valid_host" not in _stage_batch(dict(per_view_joint_valid=host_m))
    out = []
    for kw in (dict(view_joint_valid=dp["view_joint_valid"], view_joint_valid_host=dp["view_joint_valid_host"]),
               dict(view_joint_valid=dp["view_joint_valid"]), dict(view_joint_valid=host_m)):
        random.seed(3)
        r = triangulate_batch(torch.from_numpy(hm).to(dev), dp["proj_matrices"], c["stride"], dp["joint_valid"], n_iters=c["n_iters"],
                              pair_rng=random, valid_joints_host=dp["joint_valid_host"], **kw)
        out.append((r, random.getstate()))
    for r, state in out[1:]:
        assert state == out[0][1]
        for k in OUT + ("keypoints_2d",):
            assert _same_bits(out[0][0][k], r[k])

    sc, cfg, tl, masks, model, heatmaps = _sal_setup(dev)
    cfg.AL.STRATEGY = "TRIANGULATION"
    cfg.AL.VIEW_JOINT_VALID_KEY, cfg.AL.MIN_PEAK = "per_view_joint_valid", 0.9
    st = ActiveLearningStrategy(cfg)
    keyed, gated = [], []
    for dp_, hm_, m in zip(tl, heatmaps, masks):
        t = torch.from_numpy(hm_).to(dev)
        hm5 = t.reshape(sc["b"], sc["v"], sc["j"], *t.shape[2:])
        gate = (hm5 >= 0.9).flatten(-2).any(-1).cpu()
        assert not gate.all().item()
        one = dict(dp_, per_view_joint_valid=torch.from_numpy(m.astype(np.float32)))
        got, host = st._view_joint_valid(hm5, st._stage_masked(one))
        assert host is None and got.is_cuda and torch.equal(got.cpu().bool(), gate & torch.from_numpy(m))
        keyed.append(one)
        gated.append(dict(dp_, view_joint_valid=gate & torch.from_numpy(m)))
    a = st._compute_sal_dict(keyed, model())
    cfg.AL.VIEW_JOINT_VALID_KEY, cfg.AL.MIN_PEAK = "", 0.0
    b = ActiveLearningStrategy(cfg)._compute_sal_dict(gated, model())
    assert list(a) == list(b)
    for field in a:
        assert list(a[field]) == list(b[field]) and all(a[field][g] == b[field][g] or a[field][g] != a[field][g] for g in a[field]), field


def test_entries_refuse_bad_arguments_and_launch_nothing(dev):
    """V > 32 (V > 11 for the all-pairs entry), V < 2 and a NULL mask: the documented error, a message, and output buffers that
    keep their sentinel values.  The wrappers raise on a mask of the wrong shape."""
    from multi_view_active_learning_amd import _lib

    b, v, j, p = 2, 33, 5, 64
    kp = torch.zeros((b, v, j, 2), dtype=torch.int64, device=dev)
    proj = torch.ones((b, v, 3, 4), dtype=torch.float64, device=dev)
    pairs = torch.zeros((b, j, p, 2), dtype=torch.uint8, device=dev)
    pairs[..., 1] = 1
    mt = torch.ones((b, v, j), dtype=torch.uint8, device=dev)
    per_map = torch.zeros((b * v * j,), dtype=torch.float32, device=dev)
    hm = torch.zeros((b, v, j, 8, 8), dtype=torch.float32, device=dev)
    k3 = torch.full((b, j, 3), -7.0, dtype=torch.float64, device=dev)
    jerr = torch.full((b, j), -7.0, dtype=torch.float64, device=dev)
    jinl = torch.full((b, j), -7, dtype=torch.int32, device=dev)
    metric = torch.full((b,), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((b,), -7, dtype=torch.int32, device=dev)
    ws = torch.full((b * v * j,), -7.0, dtype=torch.float64, device=dev)
    gate = torch.full((b * v * j,), 7, dtype=torch.uint8, device=dev)
    P, N = _lib._p, _lib._p(None)
    outs = (P(k3), P(jerr), P(jinl), P(metric), P(cnt))
    K, NULL_MASK = _lib.MASK_VIEW_JOINT, "a mask goes with mask_kind 1 or 2, NULL with 0"
    one, table = _lib._views_entry("mval_triangulate_ransac_masked"), _lib._views_entry("mval_triangulate_ransac_pairs_masked")
    xe, red, peak = (_lib._views_entry(n) for n in ("mval_reprojection_xe_masked", "mval_score_reduce_masked", "mval_peak_mask"))
    for v_, mask, word in ((33, P(mt), "32"), (1, P(mt), "2 views"), (12, N, NULL_MASK)):
        assert table(P(kp), 0, P(proj), N, mask, K, P(pairs), p, 0, *outs, b, v_, j, 5.0, _lib._stream()) != 0
        assert word in _lib.lib().mval_last_error().decode(), (v_, word)
    for v_, mask, word in ((33, P(mt), "V > 11"), (12, P(mt), "V > 11"), (1, P(mt), "2 views"), (4, N, NULL_MASK)):
        assert one(P(kp), 0, P(proj), N, mask, K, *outs, b, v_, j, 5.0, _lib._stream()) != 0
        assert word in _lib.lib().mval_last_error().decode(), (v_, word)
    assert xe(P(k3), P(proj), P(hm), N, K, P(metric), P(ws), b, 4, j, 8, 8, 1.0, _lib._stream()) != 0
    assert NULL_MASK in _lib.lib().mval_last_error().decode()
    assert red(P(per_map), N, N, K, P(metric), b, 4, j, 0, _lib._stream()) != 0
    assert NULL_MASK in _lib.lib().mval_last_error().decode()
    # (a mask_kind outside 0..2, or MVAL_MASK_NONE beside a mask: test_gpu_view_mask.py, for every entry and kind)
    assert peak(N, 0.5, P(gate), 4, 8, 8, _lib._stream()) != 0 and "NULL" in _lib.lib().mval_last_error().decode()
    assert peak(P(hm), 0.5, P(gate), 4, 0, 8, _lib._stream()) != 0 and "bad dims" in _lib.lib().mval_last_error().decode()
    torch.cuda.synchronize()
    for t in (k3, jerr, jinl, metric, cnt, ws):
        assert (t == -7).all().item()
    assert (gate == 7).all().item()
    with pytest.raises(_lib.MvalError, match="view_joint_valid"):
        _lib.triangulate_ransac(kp[:, :4].contiguous(), proj[:, :4].contiguous(), None, b, 4, j, 5.0, view_joint_valid=mt)  # (B, 33, J) mask
    with pytest.raises(_lib.MvalError, match="32"):
        _lib.triangulate_ransac_pairs(kp, proj, None, pairs, b, v, j, 5.0, view_joint_valid=mt)


# ---- one (mask, mask_kind) argument for every kind ---------------------------------------------------------------------------------
def _raw_triangulation(dev, entry, kp, pt, vt, mask_args, pairs, b, v, j):
    """One raw call of a triangulation entry (unmasked: converted by hand, it carries no argtypes; ``_masked``: through its
    argtypes) into sentinel-filled outputs; ``mask_args``: () or (mask pointer, mask_kind)."""
    import ctypes as C

    from multi_view_active_learning_amd import _lib

    outs = [torch.full((b, j, 3), -7.0, dtype=torch.float64, device=dev), torch.full((b, j), -7.0, dtype=torch.float64, device=dev),
            torch.full((b, j), -7, dtype=torch.int32, device=dev), torch.full((b,), -7.0, dtype=torch.float64, device=dev),
            torch.full((b,), -7, dtype=torch.int32, device=dev)]
    table = () if pairs is None else (_lib._p(pairs), C.c_int(pairs.shape[-2]), C.c_int(0))
    f = _lib._views_entry(entry) if mask_args else getattr(_lib.lib(), entry)
    rc = f(_lib._p(kp), C.c_int(int(kp.dtype == torch.float32)), _lib._p(pt), _lib._p(vt), *mask_args, *table, *(_lib._p(o) for o in outs),
           C.c_int(b), C.c_int(v), C.c_int(j), C.c_double(vm.EPS), _lib._stream())
    assert rc == 0, _lib.lib().mval_last_error().decode()
    return outs


@pytest.mark.parametrize("kp_dtype", [torch.int64, torch.float32], ids=["int64", "float32"])
@pytest.mark.parametrize("name", ["m4", "m12_mixed", "degenerate"])
def test_mask_kinds_agree(dev, name, kp_dtype):
    """The existing missing-view inputs at V = 4 (one lane per pair; B = 3, J = 19: 57 problems in 8-lane groups, so the last block
    has dead groups) and V = 12 (table kernel, one wave per problem), both key-point dtypes.
    (a) Every ``_masked`` entry with MVAL_MASK_NONE / NULL has the bits of its unmasked sibling -- raw calls, the python wrappers
    reach the ``_masked`` entries only.
    (b) MVAL_MASK_VIEWS with view_valid has the bits of MVAL_MASK_VIEW_JOINT with view_valid broadcast over the joints --
    triangulation, XE, score reduction in all four modes -- on every frame whose valid joints are all used.  On a frame with
    fewer than two present views (case ``degenerate``) both write what the header documents: inlier_count -2 with a valid joint,
    -1 without, metric NaN, no used joint (joint_inliers 0)."""
    import ctypes as C

    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import draw_view_pairs

    c = vm.view_mask_cases()[name]
    hm, proj, valid, vv = vm.build(c)
    b, v, j, hh, wh = hm.shape
    t, pt = torch.from_numpy(hm).to(dev), torch.from_numpy(proj).to(dev)
    vt, vvt = torch.from_numpy(valid.astype(np.uint8)).to(dev), torch.from_numpy(vv.astype(np.uint8)).to(dev)
    wide = vvt[:, :, None].expand(b, v, j).contiguous()
    kp = _lib.argmax_decode(t, vt, b, v, j, hh, wh, c["stride"], hh).to(kp_dtype)
    none = (_lib._p(None), _lib.MASK_NONE)
    per_map = torch.from_numpy(np.random.default_rng(5).standard_normal(b * v * j).astype(np.float32)).to(dev)
    sigma = 1.5

    # (a) MVAL_MASK_NONE == the unmasked entry
    drawn = torch.from_numpy(draw_view_pairs(valid, v, c["n_iters"], random.Random(1))).to(dev)  # (V = 12: 64 of 66 drawn per joint)
    todo = [("mval_triangulate_ransac_pairs", drawn)] + ([("mval_triangulate_ransac", None)] if v <= 11 else [])
    for entry, pairs in todo:
        want = _raw_triangulation(dev, entry, kp, pt, vt, (), pairs, b, v, j)
        got = _raw_triangulation(dev, entry + "_masked", kp, pt, vt, none, pairs, b, v, j)
        for w, g in zip(want, got):
            assert _same_bits(w, g), entry
    kp3d = want[0]
    xe = [torch.full((b,), -7.0, dtype=torch.float64, device=dev) for _ in range(2)]
    ws = torch.empty((b * v * j,), dtype=torch.float64, device=dev)
    assert _lib.lib().mval_reprojection_xe(_lib._p(kp3d), _lib._p(pt), _lib._p(t), _lib._p(xe[0]), _lib._p(ws), C.c_int(b), C.c_int(v), C.c_int(j),
                                           C.c_int(hh), C.c_int(wh), C.c_double(sigma), _lib._stream()) == 0
    assert _lib._views_entry("mval_reprojection_xe_masked")(_lib._p(kp3d), _lib._p(pt), _lib._p(t), *none, _lib._p(xe[1]), _lib._p(ws), b, v, j, hh, wh,
                                                            sigma, _lib._stream()) == 0
    assert _same_bits(xe[0], xe[1]) and not (xe[0] == -7).any().item()
    for mode in (_lib.REDUCE_AVG_F64, _lib.REDUCE_AVG_F32, _lib.REDUCE_STD_F64, _lib.REDUCE_STD_F32):
        red = [torch.full((b,), -7.0, dtype=torch.float64, device=dev) for _ in range(2)]
        assert _lib.lib().mval_score_reduce(_lib._p(per_map), _lib._p(vt), _lib._p(red[0]), C.c_int(b), C.c_int(v), C.c_int(j), C.c_int(mode),
                                            _lib._stream()) == 0
        assert _lib._views_entry("mval_score_reduce_masked")(_lib._p(per_map), _lib._p(vt), *none, _lib._p(red[1]), b, v, j, mode, _lib._stream()) == 0
        assert _same_bits(red[0], red[1]) and not (red[0] == -7).any().item(), mode

    # (b) MVAL_MASK_VIEWS == MVAL_MASK_VIEW_JOINT with the mask broadcast over the joints
    full = torch.from_numpy(vv.sum(axis=1) >= 2).to(dev)  # the frames whose valid joints are all used
    by_frame, by_entry = dict(view_valid=vvt), dict(view_joint_valid=wide)
    if v <= 11:
        tri = [_lib.triangulate_ransac(kp, pt, vt, b, v, j, vm.EPS, **kw) for kw in (by_frame, by_entry)]
    else:
        tabs = [torch.from_numpy(draw_view_pairs(valid, v, c["n_iters"], random.Random(2), **kw)).to(dev)
                for kw in (dict(view_valid=vv), dict(view_joint_valid=wide.cpu().numpy()))]
        assert torch.equal(tabs[0], tabs[1])
        tri = [_lib.triangulate_ransac_pairs(kp, pt, vt, tabs[0], b, v, j, vm.EPS, **kw) for kw in (by_frame, by_entry)]
    for x, y in zip(*tri):
        assert _same_bits(x[full], y[full])
    any_valid = torch.from_numpy(valid.any(axis=1)).to(dev)
    for kp3d_, jerr, jinl, metric, inl in tri:
        assert not (jinl[~full] > 0).any().item() and torch.isnan(metric[~full]).all().item()  # no used joint
        assert torch.equal(inl[~full], torch.where(any_valid[~full], -2, -1).to(torch.int32))
    assert name != "degenerate" or (~full).sum().item() == 3
    xes = [_lib.reprojection_xe(tri[0][0], pt, t, b, v, j, hh, wh, sigma, **kw) for kw in (by_frame, by_entry)]
    assert _same_bits(xes[0][full], xes[1][full])
    for mode in (_lib.REDUCE_AVG_F64, _lib.REDUCE_AVG_F32, _lib.REDUCE_STD_F64, _lib.REDUCE_STD_F32):
        reds = [_lib.score_reduce(per_map, vt, b, v, j, mode, **kw) for kw in (by_frame, by_entry)]
        assert _same_bits(reds[0][full], reds[1][full]), mode

"""GPU tests of the 3-D refinement: ``mval_refine_points_3d`` against the goldens of tests/golden/refine3d.npz --
the long-double minimum of every problem and the float64 oracle of tests/refine3d_oracle.py, within four times the oracle's own
recorded gap --, descent, independence from the rest of the batch, absent entries, exact data, and the calls that carry the
refinement: triangulate_batch, the scoring pass and the evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import cases  # noqa: E402
import refine3d_cases as rc  # noqa: E402
import refine3d_oracle as ro  # noqa: E402
from multi_view_active_learning_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = rc.refine3d_cases()
KINDS = ("i64", "f32")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return rc.load_golden()


def _same_bits(a, b):
    """torch.equal that takes NaN for what it is: the same bits."""
    if a.dtype.is_floating_point:
        as_int = torch.int64 if a.dtype == torch.float64 else torch.int32
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _run(dev, d, kp, x0, err0, inl0, sl=None, eps=rc.EPS):
    """The entry on a case's inputs (``sl`` = (b, j): that problem alone, as B = 1, J = 1 with its own mask row) -> numpy
    (points, joint_error, joint_support, joint_status, metric)."""
    from multi_view_active_learning_amd import _lib

    pick = (lambda a, axes: a) if sl is None else (lambda a, axes: a[tuple(slice(sl[0], sl[0] + 1) if ax == "b" else slice(sl[1], sl[1] + 1) if ax == "j"
                                                                           else slice(None) for ax in axes)])
    t = lambda a, axes: None if a is None else torch.from_numpy(np.ascontiguousarray(pick(a, axes))).to(dev)  # noqa: E731
    kp, proj, x0, err0, inl0 = t(kp, "bvj"), t(d["proj"], "bv"), t(x0, "bj"), t(err0, "bj"), t(inl0.astype(np.int32), "bj")
    b, v, j = kp.shape[:3]
    valid = t(d["valid"].astype(np.uint8), "bj")
    vv = None if d["view_valid"] is None else t(d["view_valid"].astype(np.uint8), "bv")
    vj = None if d["view_joint_valid"] is None else t(d["view_joint_valid"].astype(np.uint8), "bvj")
    out = _lib.refine_points_3d(kp, proj, valid, x0, err0, inl0, b, v, j, eps, view_valid=vv, view_joint_valid=vj, weights=t(d["weights"], "bvj"))
    return tuple(o.cpu().numpy() for o in out)


def _case(golden, name, kind):
    d = rc.build(CASES[name])
    g = lambda key: golden[f"{name}/{kind}/{key}"]  # noqa: E731
    return d, g


def _cost(d, g, bi, ji, X):
    S = np.flatnonzero(g("support")[bi, :, ji])
    w = np.ones(len(S)) if d["weights"] is None else d["weights"][bi, S, ji]
    return ro.cost(d["proj"][bi, S], g("kp")[bi, S, ji], w, X)


# ---- the kernel against the goldens ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_goldens(dev, golden, name, kind):
    """Every case, both key-point types, from the stored DLT points: the refined points are within the V group's tolerance
    (4 x the largest recorded gap_oracle) of the long-double minimum AND of the oracle's point; joint_support = |S| exactly;
    status 0 exactly where the oracle's is and positive wherever the oracle's is; unrefined problems hand X0 and its error
    through bit for bit; the joint error is the mean half-distance over S at the returned point (1e-9 relative, recomputed on
    the host); the cost did not rise (descent); the metric is the mean of the new joint errors over the used joints."""
    c = CASES[name]
    d, g = _case(golden, name, kind)
    x, jerr, support, status, metric = _run(dev, d, g("kp"), g("x0"), g("err0"), g("inliers0"))
    np.testing.assert_array_equal(support, g("support").sum(axis=1))
    assert support.dtype == status.dtype == np.int32
    refined = g("status") != 0
    np.testing.assert_array_equal(status == 0, ~refined)
    assert (status[g("status") > 0] > 0).all(), status
    assert x[~refined].tobytes() == g("x0")[~refined].tobytes() and jerr[~refined].tobytes() == g("err0")[~refined].tobytes()
    if refined.any():
        tol = rc.tolerances(golden)[c["v"]]
        to_min = np.linalg.norm(x - g("xmin"), axis=-1)[refined]
        to_oracle = np.linalg.norm(x - g("x"), axis=-1)[refined]
        print(f"{name}/{kind}: {refined.sum()} refined, device iterations {status[refined].min()}..{status[refined].max()} (oracle "
              f"{g('status')[refined].min()}..{g('status')[refined].max()}), |device - minimum| max {to_min.max():.2e} mm, |device - oracle| max "
              f"{to_oracle.max():.2e} mm, tolerance {tol:.2e} mm")
        assert to_min.max() <= tol and to_oracle.max() <= tol
        assert (status[refined] <= ro.MAX_ITERS).all()
        for bi, ji in zip(*np.nonzero(refined)):
            S = np.flatnonzero(g("support")[bi, :, ji])
            want = np.mean([ro.half_distance(d["proj"][bi, v], x[bi, ji], g("kp")[bi, v, ji].astype(np.float64)) for v in S])
            assert jerr[bi, ji] == pytest.approx(want, rel=1e-9)
            assert _cost(d, g, bi, ji, x[bi, ji]) <= _cost(d, g, bi, ji, g("x0")[bi, ji]) * (1 + 1e-12)
    used = d["valid"] & (g("inliers0") > 0)
    for bi in range(c["b"]):
        if used[bi].any():
            assert metric[bi] == pytest.approx(np.mean(jerr[bi][used[bi]]), rel=1e-14)
        else:
            assert np.isnan(metric[bi])


@pytest.mark.parametrize("name", ["v4", "v32", "v4_views", "v8_view_joint", "v4_weighted"])
def test_a_problem_does_not_depend_on_its_batch(dev, golden, name):
    """Each problem alone (B = 1, J = 1, its own mask row and weights) gives the bits it gives inside the batch: without a mask,
    under view_valid and under view_joint_valid."""
    c = CASES[name]
    for kind in KINDS:
        d, g = _case(golden, name, kind)
        x, jerr, support, status, _ = _run(dev, d, g("kp"), g("x0"), g("err0"), g("inliers0"))
        for bi in range(c["b"]):
            for ji in range(c["j"]):
                x1, jerr1, support1, status1, _ = _run(dev, d, g("kp"), g("x0"), g("err0"), g("inliers0"), sl=(bi, ji))
                assert x1.tobytes() == x[bi, ji].tobytes() and jerr1.tobytes() == jerr[bi, ji].tobytes(), (kind, bi, ji)
                assert support1[0, 0] == support[bi, ji] and status1[0, 0] == status[bi, ji], (kind, bi, ji)


@pytest.mark.parametrize("name", ["v4_views", "v8_view_joint"])
def test_absent_entries_are_not_read(dev, golden, name):
    """The cases hold NaN in the matrices of absent views and in the float32 key-points of absent entries (a far-away value in
    the int64 ones); plausible finite values in their place -- the frame's first present view, the joint's true projection --
    change no bit of any output."""
    for kind in KINDS:
        d, g = _case(golden, name, kind)
        got = _run(dev, d, g("kp"), g("x0"), g("err0"), g("inliers0"))
        filled, kp = dict(d, proj=d["proj"].copy()), g("kp").copy()
        for bi in range(kp.shape[0]):
            for vi in range(kp.shape[1]):
                if d["view_valid"] is not None and not d["view_valid"][bi, vi]:
                    filled["proj"][bi, vi] = d["proj"][bi, np.flatnonzero(d["view_valid"][bi])[0]]
        truth = rc.project(filled["proj"], d["joints"])
        absent = ~(np.broadcast_to(d["view_valid"][:, :, None], kp.shape[:3]) if d["view_joint_valid"] is None else d["view_joint_valid"])
        assert absent.any() and (kind == "i64" or np.isnan(kp[absent]).all())
        kp[absent] = truth[absent].astype(kp.dtype)
        assert np.isfinite(filled["proj"]).all() and np.isfinite(kp.astype(np.float64)).all()
        want = _run(dev, filled, kp, g("x0"), g("err0"), g("inliers0"))
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()


def _exact_rig(n=12, seed=5):
    """Noise-free data whose float32 key-points are EXACT: per frame one joint with integer coordinates and four axis-aligned
    cameras (f = 256 px) placed so that the joint's depths are 2048, 4096, 1024 and 8192 mm -- every projection is an integer
    over a power of two.  -> proj (N, 4, 3, 4), joints (N, 1, 3), kp (N, 4, 1, 2) float32."""
    rng = np.random.default_rng(seed)
    k = np.array([[256.0, 0, 128.0], [0, 256.0, 128.0], [0, 0, 1]])
    joints = rng.integers(-300, 301, (n, 1, 3)).astype(np.float64)
    proj = np.zeros((n, 4, 3, 4))
    rots = [np.array([[0.0, 1, 0], [0, 0, -1], [-1, 0, 0]]), np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]]),
            np.array([[-1.0, 0, 0], [0, 0, -1], [0, -1, 0]]), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])]
    for bi in range(n):
        for vi, (r, depth) in enumerate(zip(rots, (2048.0, 4096.0, 1024.0, 8192.0))):
            t = np.array([0.0, 0.0, depth - r[2] @ joints[bi, 0]])  # the camera sits on its axis, `depth` in front of the joint
            proj[bi, vi] = k @ np.concatenate([r, t[:, None]], axis=1)
    kp = rc.project(proj, joints)
    assert (kp.astype(np.float32).astype(np.float64) == kp).all()
    return proj, joints, kp.astype(np.float32)


def test_exact_data_stays_where_it_is(dev, golden):
    """Noise-free float32 key-points handed in through ``keypoints_2d=``: the DLT point already is the minimum, and the refined
    point is within the V = 4 tolerance of it and of the true joint."""
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    proj, joints, kp = _exact_rig()
    n = len(kp)
    r = triangulate_batch(torch.zeros(n, 4, 1, 2, 2, device=dev), torch.from_numpy(proj), 4, torch.ones(n, 1), keypoints_2d=torch.from_numpy(kp).to(dev),
                          refine_3d="lm")
    tol = rc.tolerances(golden)[4]
    x, x0 = r["keypoints_3d"].cpu().numpy(), r["keypoints_3d_dlt"].cpu().numpy()
    print("exact data: |lm - dlt| max %.2e mm, |lm - truth| max %.2e mm, |dlt - truth| max %.2e mm, status %r" % (
        np.linalg.norm(x - x0, axis=-1).max(), np.linalg.norm(x - joints, axis=-1).max(), np.linalg.norm(x0 - joints, axis=-1).max(),
        r["joint_status"].flatten().tolist()))
    assert (r["joint_support"] == 4).all() and (r["joint_status"] > 0).all()
    assert np.linalg.norm(x - x0, axis=-1).max() <= tol and np.linalg.norm(x - joints, axis=-1).max() <= tol


# ---- plumbing: triangulate_batch -----------------------------------------------------------------------------------------------
def _rig(noise=0.02, n=3, v=4, j=5, hh=32, wh=32, stride=4, seed=2):  # (square maps: the default decode splits by the height)
    proj = np.stack([synth.ring_cameras(v, hh * stride, wh * stride, radius=1500.0 * (1 + k), seed=k) for k in range(n)])
    kp3d = synth.joints_3d(1, n, j, sigma_mm=150)
    return synth.gaussian_heatmaps(seed, proj, kp3d, hh, wh, stride, noise=noise), proj, kp3d


TODAY = {"keypoints_3d", "keypoints_2d", "metric", "inlier_count", "joint_error", "joint_inliers"}


@pytest.mark.parametrize("mask", [None, "view_valid", "view_joint_valid"])
def test_triangulate_batch_under_lm(dev, mask):
    """"lm" returns the kernel's outputs on the triangulation's own results plus ``keypoints_3d_dlt``; "none" is today's result,
    key for key and bit for bit, with and without the argument; the metric is the mean of the new joint errors over the joints it
    ran over before; inlier counts stay RANSAC's."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch, triangulation

    hm, proj, _ = _rig()
    b, v, j, hh, wh = hm.shape
    valid = torch.ones(b, j, dtype=torch.uint8)
    valid[1, 3] = 0
    kw, vv, vj = {}, None, None
    if mask == "view_valid":
        vv = torch.tensor([[1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]], dtype=torch.uint8)
        kw = {"view_valid": vv}
    elif mask == "view_joint_valid":
        vj = torch.ones(b, v, j, dtype=torch.uint8)
        vj[0, 1, 2] = vj[1, 0, 4] = vj[2, 2, 0] = 0
        vj[0, :3, 3] = 0  # one view left: not used
        kw = {"view_joint_valid": vj}
    t_hm, t_proj = torch.from_numpy(hm).to(dev), torch.from_numpy(proj)
    plain = triangulate_batch(t_hm, t_proj, 4, valid, **kw)
    again = triangulate_batch(t_hm, t_proj, 4, valid, refine_3d="none", refine_3d_weights=None, refine_3d_epsilon=None, **kw)
    assert set(plain) == set(again) == TODAY | ({"joint_used"} if vj is not None else set())
    for k in plain:
        assert _same_bits(plain[k], again[k]), k
    got = triangulate_batch(t_hm, t_proj, 4, valid, refine_3d="lm", **kw)
    assert set(got) == set(plain) | {"keypoints_3d_dlt", "joint_support", "joint_status"}
    x, jerr, support, status, metric = _lib.refine_points_3d(
        plain["keypoints_2d"], t_proj.to(dev), valid.to(dev), plain["keypoints_3d"], plain["joint_error"], plain["joint_inliers"], b, v, j, 5.0,
        view_valid=None if vv is None else vv.to(dev), view_joint_valid=None if vj is None else vj.to(dev))
    for k, want in (("keypoints_3d", x), ("joint_error", jerr), ("joint_support", support), ("joint_status", status), ("metric", metric),
                    ("keypoints_3d_dlt", plain["keypoints_3d"]), ("keypoints_2d", plain["keypoints_2d"]), ("joint_inliers", plain["joint_inliers"]),
                    ("inlier_count", plain["inlier_count"])):
        assert _same_bits(got[k], want), k
    used = (valid.bool() & (plain["joint_inliers"].cpu() > 0)).numpy()
    assert (got["joint_status"].cpu().numpy()[used] > 0).all() and not got["joint_status"].cpu().numpy()[~used].any()
    assert not _same_bits(got["keypoints_3d"], plain["keypoints_3d"])
    for bi in range(b):
        assert got["metric"][bi].item() == pytest.approx(np.mean(got["joint_error"][bi].cpu().numpy()[used[bi]]), rel=1e-14)
        assert got["metric"][bi].item() != plain["metric"][bi].item()
    # a tighter support threshold than the vote's: fewer views in S, never more
    tight = triangulate_batch(t_hm, t_proj, 4, valid, refine_3d="lm", refine_3d_epsilon=0.75, **kw)
    assert (tight["joint_support"] <= got["joint_support"]).all() and (tight["joint_support"] < got["joint_support"]).any()
    assert _same_bits(tight["keypoints_3d_dlt"], plain["keypoints_3d"])
    one = triangulation(t_hm[1], proj[1], 4, valid[1], refine_3d="lm", **{k: m[1] for k, m in kw.items()})
    for k in ("keypoints_3d", "keypoints_3d_dlt", "joint_error", "joint_support", "joint_status"):
        assert one[k].tobytes() == got[k][1].cpu().numpy().tobytes(), k
    assert one["metric"] == got["metric"][1].item() and set(one) == {"keypoints_3d", "keypoints_2d", "metric", "inlier_count", "keypoints_3d_dlt",
                                                                      "joint_error", "joint_support", "joint_status"}


def test_xe_decode_refinement_and_weights_under_lm(dev):
    """XE under "lm" is ``_lib.reprojection_xe`` on the refined points; "lm" works on a refined decode, and
    ``refine_3d_weights="conf"`` weights it by the peak heights -- the entry called with ``keypoints_conf``."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    # stride 1: the reference lays input-pixel reprojections on the heat-map-sized grid, and only there do they fall inside it
    hm, proj, _ = _rig(stride=1)
    b, v, j, hh, wh = hm.shape
    valid = torch.ones(b, j)
    t_hm, t_proj = torch.from_numpy(hm).to(dev), torch.from_numpy(proj)
    got = triangulate_batch(t_hm, t_proj, 1, valid, use_reprojection_xe=True, sigma=1.5, refine_3d="lm")
    assert (got["joint_status"] > 0).all()
    assert _same_bits(got["metric"], _lib.reprojection_xe(got["keypoints_3d"], t_proj.to(dev), t_hm, b, v, j, hh, wh, 1.5))
    assert not _same_bits(got["metric"], _lib.reprojection_xe(got["keypoints_3d_dlt"], t_proj.to(dev), t_hm, b, v, j, hh, wh, 1.5))

    hm, proj, _ = _rig()
    t_hm, t_proj = torch.from_numpy(hm).to(dev), torch.from_numpy(proj)
    dec = triangulate_batch(t_hm, t_proj, 4, valid, refine="taylor")
    for weights in (None, "conf"):
        got = triangulate_batch(t_hm, t_proj, 4, valid, refine="taylor", refine_3d="lm", refine_3d_weights=weights)
        assert got["keypoints_2d"].dtype == torch.float32 and _same_bits(got["keypoints_3d_dlt"], dec["keypoints_3d"])
        x, jerr, support, status, metric = _lib.refine_points_3d(dec["keypoints_2d"], t_proj.to(dev), valid.to(dev, torch.uint8), dec["keypoints_3d"],
                                                                 dec["joint_error"], dec["joint_inliers"], b, v, j, 5.0,
                                                                 weights=None if weights is None else dec["keypoints_conf"])
        assert _same_bits(got["keypoints_3d"], x) and _same_bits(got["joint_error"], jerr) and _same_bits(got["metric"], metric)
        assert _same_bits(got["joint_status"], status) and (status > 0).all()
        if weights is None:
            unweighted = x
    assert not _same_bits(unweighted, x)  # (the weights matter)
    tensor = triangulate_batch(t_hm, t_proj, 4, valid, refine="taylor", refine_3d="lm", refine_3d_weights=dec["keypoints_conf"].cpu().numpy())
    assert _same_bits(tensor["keypoints_3d"], x)


# ---- accuracy ------------------------------------------------------------------------------------------------------------------
def test_accuracy_on_the_unequal_radius_rig(dev):
    """Cameras at 1500 / 3000 / 4500 / 6000 mm, 300 problems (B = 15, J = 20, V = 4), grid-snapped points: the mean distance to the
    true joints under "lm" is below the DLT's of the same run.  The float64 oracle gives 17.05 mm (DLT) and 12.05 mm (lm) on the
    host for this seed."""
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    proj, joints, kp = rc.accuracy_rig()
    b, v, j = kp.shape[:3]
    r = triangulate_batch(torch.zeros(b, v, j, 2, 2, device=dev), torch.from_numpy(proj), 4, torch.ones(b, j), keypoints_2d=torch.from_numpy(kp).to(dev),
                          refine_3d="lm")
    dlt = np.linalg.norm(r["keypoints_3d_dlt"].cpu().numpy() - joints, axis=-1)
    lm = np.linalg.norm(r["keypoints_3d"].cpu().numpy() - joints, axis=-1)
    status = r["joint_status"].cpu().numpy()
    print("unequal-radius rig: mean error DLT %.3f mm, lm %.3f mm (%.0f %% of the problems better), iterations %d..%d" % (
        dlt.mean(), lm.mean(), 100 * (lm < dlt).mean(), status.min(), status.max()))
    assert (status > 0).all()
    assert lm.mean() < dlt.mean()


# ---- strategy ------------------------------------------------------------------------------------------------------------------
def _sal_setup(dev):
    from multi_view_active_learning_amd.config import get_default_configs

    c = cases.sal_cases()["hp"]
    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = c["stride"]
    loader, heatmaps = cases.build_sal_loader(c)
    tl = [{k: torch.from_numpy(a) for k, a in dp.items()} for dp in loader]
    return c, cfg, tl, heatmaps


@pytest.mark.parametrize("strategy", ["TRIANGULATION", "CORESET"])
def test_score_batch_under_refine_3d(dev, strategy):
    """score_batch under AL.REFINE_3D = "lm" is the table built by hand from triangulate_batch(refine_3d="lm"); under "none" it is
    the table built from today's triangulate_batch.  EVAL.REFINE_3D has no say in it."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c, cfg, tl, heatmaps = _sal_setup(dev)
    cfg.AL.STRATEGY = strategy
    cfg.EVAL.REFINE_3D = "lm"
    b, v, j = c["b"], c["v"], c["j"]
    tables = {}
    for mode in ("none", "lm"):
        cfg.AL.REFINE_3D = mode
        for dp, hm in zip(tl, heatmaps):
            t = torch.from_numpy(hm).to(dev)
            st = ActiveLearningStrategy(cfg)
            st._pending_checks = []
            tab = st.score_batch(t, dp)
            hm5 = t.reshape(b, v, j, *t.shape[2:])
            jv = dp["joint_valid"].reshape(b, j)
            r = triangulate_batch(hm5, dp["proj_matrices"], c["stride"], jv, **({} if mode == "none" else {"refine_3d": "lm"}))
            assert ("joint_status" in r) == (mode == "lm")
            pred32 = r["keypoints_3d"].to(torch.float32)
            _, per = _lib.mkpe(pred32.contiguous(), dp["3d_keypoints"].to(dev, torch.float32).contiguous(), jv.to(dev, torch.float32).contiguous(),
                               b, j, dp["3d_keypoints"].shape[1])
            assert _same_bits(tab[:, 3], r["metric"].to(torch.float32).to(torch.float64))
            assert _same_bits(tab[:, 4], r["inlier_count"].to(torch.float64)) and _same_bits(tab[:, 5], per.to(torch.float64))
            assert _same_bits(tab[:, 6:], pred32.to(torch.float64).reshape(b, 3 * j))
            assert _same_bits(tab[:, 2], r["metric"] if strategy == "TRIANGULATION" else torch.zeros_like(r["metric"]))
            tables.setdefault(mode, []).append(tab)
    assert not any(_same_bits(a[:, 6:], b_) for a, b_ in zip(tables["none"], tables["lm"]))  # (the refinement matters on this input)


def test_evaluate_mkpe_under_refine_3d(dev):
    """evaluate_mkpe under EVAL.REFINE_3D = "lm" is the MKPE of triangulate_batch(refine_3d="lm") on the same heat-maps; under
    "none" today's; AL.REFINE_3D has no say in it; the table evaluate_all reads its 3-D PCK from holds the refined points."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    hm, proj, kp3d = _rig()
    b, v, j, hh, wh = hm.shape
    loader = [{"images": torch.zeros(b, v, 3, 8, 8), "pose": torch.arange(b), "frame_id": torch.arange(b), "proj_matrices": torch.from_numpy(proj),
               "joint_valid": torch.ones(b, j), "3d_keypoints": torch.from_numpy(kp3d)}]
    model = lambda images: torch.from_numpy(hm.reshape(b * v, j, hh, wh)).to(dev)  # noqa: E731
    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = 4
    cfg.AL.REFINE_3D = "lm"
    value = {}
    for mode in ("none", "lm"):
        cfg.EVAL.REFINE_3D = mode
        st = ActiveLearningStrategy(cfg)
        value[mode] = st.evaluate_mkpe(loader, model)
        r = triangulate_batch(torch.from_numpy(hm).to(dev), torch.from_numpy(proj), 4, torch.ones(b, j), **({} if mode == "none" else {"refine_3d": "lm"}))
        want, _ = _lib.mkpe(r["keypoints_3d"].to(torch.float32).contiguous(), torch.from_numpy(kp3d).to(dev, torch.float32).contiguous(),
                            torch.ones(b, j, device=dev), b, j, 3)
        assert _same_bits(value[mode], want)
        assert _same_bits(st._eval_tables[0], r["keypoints_3d"].to(torch.float32))
    print("evaluate_mkpe on the rig in mm: %r" % ({k: float(x.item()) for k, x in value.items()},))
    assert not _same_bits(value["none"], value["lm"])

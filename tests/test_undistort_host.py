"""Host tests (no GPU) of the key-point undistortion: the new entry in the header and the library and its
argument checks, the two config fields and their validator, the float64 oracle of tests/undistort_oracle.py against the reference's
own projections (tests/golden/undistort.npz), and where ``triangulate_batch``, ``undistort_keypoints``, ``prepare_views`` and the
scoring and evaluation passes reach the stage -- never under the default configuration."""
import os
import re
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import undistort_cases as uc  # noqa: E402
import undistort_oracle as uo  # noqa: E402

CASES = uc.undistort_cases()


@pytest.fixture(scope="module")
def golden():
    return uc.load_golden()


# ---- the entry -------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_and_exported():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    text = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+mval_undistort_keypoints\s*\(([^)]*)\)", hdr)
    assert decl, "mval_undistort_keypoints is not declared in include/mval_hip.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["const void* kp2d", "int kp_is_f32", "const double* K", "const double* dist", "const uint8_t* valid", "const uint8_t* mask",
                    "int mask_kind", "float* out", "int32_t* status", "int B", "int V", "int J", "void* stream"]
    assert hasattr(_lib.lib(), "mval_undistort_keypoints"), "mval_undistort_keypoints is not exported"
    assert len(_lib._VIEWS_ARGTYPES["mval_undistort_keypoints"]) == len(args)
    define = lambda name: int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, text).group(1))  # noqa: E731
    assert _lib.UNDISTORT_MAX_ITERS == define("MVAL_UNDISTORT_MAX_ITERS") == uo.MAX_ITERS == 16
    assert _lib.UNDISTORT_FOLD == define("MVAL_UNDISTORT_FOLD") == uo.FOLD == -1
    assert _lib.UNDISTORT_NOCONV == define("MVAL_UNDISTORT_NOCONV") == uo.NOCONV == -2


def test_entry_rejects_bad_arguments_without_a_launch():
    """V outside 1..32, bad dimensions, a mask kind outside 0..2 or not matching the mask pointer, NULL and misaligned arrays are
    errors before anything touches a device; B = 0 returns 0."""
    import ctypes as C

    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    f = _lib._views_entry("mval_undistort_keypoints")
    p = lambda a: C.c_void_p(a)  # noqa: E731  (never dereferenced: every call below fails its checks or is the B = 0 no-op)

    def call(b=1, v=4, j=5, mask=0, kind=0, kp=0x1000, f32=0, K=0x2000, dist=0x3000, out=0x4000, status=0x5000):
        return f(p(kp), f32, p(K), p(dist), p(0), p(mask), kind, p(out), p(status), b, v, j, p(0))

    assert call(b=0) == 0
    bad = (dict(v=0), dict(v=33), dict(v=-1), dict(j=0), dict(b=-1), dict(kind=3), dict(kind=-1), dict(kind=1), dict(kind=2), dict(mask=0x6000),
           dict(kp=0), dict(K=0), dict(dist=0), dict(out=0), dict(status=0), dict(K=0x2004), dict(dist=0x3004), dict(out=0x4004),
           dict(kp=0x1004), dict(kp=0x1002, f32=1), dict(status=0x5002))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"mval_undistort_keypoints" in _lib.lib().mval_last_error()


def test_check_undistort():
    from multi_view_active_learning_amd.config import UNDISTORTS, check_undistort, get_default_configs

    cfg = get_default_configs()
    assert cfg.AL.UNDISTORT == cfg.EVAL.UNDISTORT == "none"
    assert UNDISTORTS == ("none", "brown")
    assert check_undistort("none") == "none" == check_undistort("none", True)  # (XE alone is today's path)
    assert check_undistort("brown") == "brown" == check_undistort("brown", False)
    for bad in ("", "BROWN", "opencv", "fisheye", None, 1, True):
        with pytest.raises(ValueError, match="'none', 'brown'"):
            check_undistort(bad)
    with pytest.raises(ValueError, match="XE metric"):
        check_undistort("brown", True)


# ---- the oracle against the reference's projections ------------------------------------------------------------------------------
def test_golden_holds_the_cases(golden):
    assert str(golden["meta/numpy_version"])
    shapes = {(c["b"], c["v"], c["j"]) for c in CASES.values()}
    assert shapes == {(1, 2, 1), (3, 4, 5), (2, 32, 3), (3, 5, 19)}
    for name, c in CASES.items():
        d = uc.case_arrays(golden, name)
        assert d["K"].shape == (c["b"], c["v"], 3, 3) and d["dist"].shape == (c["b"], c["v"], 5)
        assert d["p_dist"].shape == (c["b"], c["v"], c["j"], 2) and d["kp_f32"].dtype == np.float32 and d["kp_i64"].dtype == np.int64
        assert np.abs(d["p_dist"]).max() < 512 and 550 < d["K"][:, :, 0, 0].min() and d["K"][:, :, 1, 1].max() < 1600
        for vi in range(c["v"]):  # the lens of the case list is the stored one
            want = np.zeros(5) if uc.lens_of(c, vi) is None else np.array(uc.lens_of(c, vi))
            assert (d["dist"][:, vi] == want).all()
        np.testing.assert_array_equal(d["proj"], d["K"] @ np.concatenate([d["R"], d["t"][..., None]], axis=-1))  # Camera.projection
        assert d["fold_entry"].any() == bool(c["fold"])
    assert (golden["mixed/dist"] == 0).all(-1).any() and (golden["mixed/dist"] != 0).any(-1).any()  # distorted and dist-free views


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_inverts_the_reference_projection(golden, name):
    """The oracle on the float64 distorted points (the reference's project_3d_points_with_camera) is within 1e-9 px of the
    reference's pinhole projection for every admitted entry: the Newton residual is about 1e-15 in normalised units, the
    conditioning at most 1 / 0.25 and f at most 1500 px -- about 1e-11 px, so 1e-9 leaves a 100x margin.  The measured maximum is
    stored as gap_reference (1.7e-13 px over all cases)."""
    d = uc.case_arrays(golden, name)
    b, v, j = d["p_dist"].shape[:3]
    worst, n = 0.0, 0
    for bi in range(b):
        for vi in range(v):
            for ji in range(j):
                if d["fold_entry"][bi, vi, ji]:
                    continue
                p = d["p_dist"][bi, vi, ji]
                x, y, st, dets = uo.undistort_point(p[0], p[1], d["K"][bi, vi], d["dist"][bi, vi])
                if (d["dist"][bi, vi] == 0).all():
                    assert st == 0 and x is None and not dets
                    got = p  # handed through: a dist-free camera is projected without distortion
                else:
                    assert 1 <= st <= 6 and min(dets) >= uc.MIN_DET
                    got = np.array([x, y])
                worst, n = max(worst, float(np.abs(got - d["p_pin"][bi, vi, ji]).max())), n + 1
    print(f"{name}: {n} entries, |oracle - pinhole| max {worst:.2e} px (stored gap_reference max {d['gap_reference'].max():.2e} px)")
    assert worst <= 1e-9
    assert worst == pytest.approx(float(d["gap_reference"].max()), abs=1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reproduces_the_stored_results(golden, name):
    """The stored oracle outputs are what the oracle gives today on the stored inputs, masks included: converged where an entry is
    present, valid and distorted; 0 and handed through on dist-free views; 0 and (0, 0) on absent entries and invalid joints."""
    d = uc.case_arrays(golden, name)
    b, v, j = d["p_dist"].shape[:3]
    processed = uo.present(b, v, j, d["valid"], d["view_valid"], d["view_joint_valid"])
    for kind in ("f32", "i64"):
        r = uo.undistort_batch(d["kp_" + kind], d["K"], d["dist"], d["valid"], d["view_valid"], d["view_joint_valid"])
        assert r["out64"].tobytes() == d[kind + "/out64"].tobytes() and (r["status"] == d[kind + "/status"]).all()
        assert not r["status"][~processed].any() and not r["out64"][~processed].any()
        free = processed & (d["dist"] == 0).all(-1)[:, :, None]
        assert not r["status"][free].any() and r["out"][free].tobytes() == d["kp_" + kind][free].astype(np.float32).tobytes()
        ran = processed & ~free
        assert (r["status"][ran & ~d["fold_entry"]] > 0).all() and (r["status"][ran & d["fold_entry"]] == uo.FOLD).all()


def test_fold_entries_are_decided_with_a_margin(golden):
    """Every fold entry stops at a det J below -1e-3 after iterates whose det J were all above 1e-3, for both key-point types: an
    implementation one ulp away takes the same decision.  Their output is the input as float32."""
    d = uc.case_arrays(golden, "fold")
    assert d["fold_entry"].sum() == 3 * 4 * 2
    for kind in ("f32", "i64"):
        r = uo.undistort_batch(d["kp_" + kind], d["K"], d["dist"], d["valid"])
        later = 0
        for e in zip(*np.nonzero(d["fold_entry"])):
            dets = r["dets"][tuple(int(i) for i in e)]
            assert r["status"][e] == uo.FOLD and dets[-1] < -uc.FOLD_MARGIN and all(x > uc.FOLD_MARGIN for x in dets[:-1])
            later += len(dets) > 1
            assert r["out"][e].tobytes() == d["kp_" + kind][e].astype(np.float32).tobytes()
        print(f"fold/{kind}: {later} of {int(d['fold_entry'].sum())} entries fold after the first iterate")


def test_oracle_hands_through_what_is_no_point():
    """NaN and inf input and a singular K2 end in FOLD; zero coefficients never read K."""
    K = np.array([[800.0, 0.5, 190.0], [0.0, 790.0, 185.0], [0.0, 0.0, 1.0]])
    for px, py in ((np.nan, 10.0), (10.0, np.inf), (-np.inf, np.nan)):
        assert uo.undistort_point(px, py, K, uc.BARREL)[2] == uo.FOLD
    assert uo.undistort_point(100.0, 120.0, np.zeros((3, 3)), uc.BARREL)[2] == uo.FOLD
    assert uo.undistort_point(100.0, 120.0, np.full((3, 3), np.nan), np.zeros(5))[2] == 0
    assert uo.undistort_point(100.0, 120.0, K, [np.nan, 0, 0, 0, 0])[2] == uo.FOLD


# ---- the calls that carry the stage -----------------------------------------------------------------------------------------------
def test_triangulate_batch_refuses_before_device_work():
    """"brown" without both tensors, an unknown name and "brown" together with XE are ValueErrors raised before the heat-maps are
    looked at: a host tensor gets that far only under "none"."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch, triangulation

    hm, proj, valid = torch.zeros(1, 2, 3, 4, 4), torch.zeros(1, 2, 3, 4), torch.ones(1, 3)
    K, dist = torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 5)
    for kw in (dict(), dict(intrinsics=K), dict(distortion=dist)):
        with pytest.raises(ValueError, match="intrinsics .* and distortion"):
            triangulate_batch(hm, proj, 4, valid, undistort="brown", **kw)
        with pytest.raises(ValueError, match="intrinsics .* and distortion"):
            triangulation(hm[0], proj[0], 4, valid[0], undistort="brown", **{k: t[0] for k, t in kw.items()})
    with pytest.raises(ValueError, match="'none', 'brown'"):
        triangulate_batch(hm, proj, 4, valid, undistort="opencv", intrinsics=K, distortion=dist)
    with pytest.raises(ValueError, match="XE metric"):
        triangulate_batch(hm, proj, 4, valid, use_reprojection_xe=True, sigma=1.0, undistort="brown", intrinsics=K, distortion=dist)
    with pytest.raises(_lib.MvalError, match="HIP tensor"):  # (the default goes on to the device check, as it always did)
        triangulate_batch(hm, proj, 4, valid)


def test_shape_refusals():
    """``undistort_keypoints`` refuses intrinsics that are not (B, V, 3, 3), a distortion that is not (B, V, 5), key-points that are
    not (B, V, J, 2) int64 | float32 -- all on host tensors, before any device work; lists and arrays are accepted as tensors are."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import undistort_keypoints

    kp = torch.zeros(2, 3, 4, 2)
    K, dist = np.zeros((2, 3, 3, 3)), np.zeros((2, 3, 5))
    for bad_k, bad_d in ((K[:1], dist), (K, dist[:, :2]), (K.reshape(2, 3, 9), dist), (K, dist[..., :4]), (K[0], dist[0]), (K.tolist(), dist[..., :4].tolist())):
        with pytest.raises(ValueError, match=r"intrinsics must be \(2, 3, 3, 3\) and distortion \(2, 3, 5\)"):
            undistort_keypoints(kp, bad_k, bad_d)
    for bad_kp in (torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, 3), np.zeros((2, 3, 4, 2), np.float32)):
        with pytest.raises(ValueError, match=r"\(B, V, J, 2\)"):
            undistort_keypoints(bad_kp, K, dist)
    with pytest.raises(ValueError, match="int64 .* or float32"):
        undistort_keypoints(kp.double(), K, dist)
    with pytest.raises(_lib.MvalError, match="HIP tensor"):  # well-formed host input: refused at the device check, not before
        undistort_keypoints(kp, K.tolist(), torch.from_numpy(dist).float())


def test_batch_without_the_camera_keys():
    """Under UNDISTORT "brown" a batch without ``intrinsics`` and ``distortion`` raises a KeyError naming both, for the scoring pass
    and the evaluation alike, before anything is triangulated; "brown" together with AL.USE_REPROJECTION_XE is check_undistort's
    ValueError; the staging adds the two keys only under "brown"."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    b, v, j = 2, 3, 4
    dp = {"pose": torch.arange(b), "frame_id": torch.arange(b), "proj_matrices": torch.zeros(b, v, 3, 4, dtype=torch.float64),
          "joint_valid": torch.ones(b, j), "3d_keypoints": torch.zeros(b, 3, j), "images": torch.zeros(b, v, 3, 8, 8)}
    hm = torch.zeros(b * v, j, 4, 4)
    cfg = get_default_configs()
    cfg.AL.STRATEGY = "TRIANGULATION"
    cfg.AL.UNDISTORT = "brown"
    st = ActiveLearningStrategy(cfg)
    st._pending_checks = []
    for lacking in (dp, dict(dp, intrinsics=torch.zeros(b, v, 3, 3)), dict(dp, distortion=torch.zeros(b, v, 5))):
        with pytest.raises(KeyError, match="'intrinsics' and 'distortion'"):
            st.score_batch(hm, lacking)
    cams = ActiveLearningStrategy._batch_cameras(dict(dp, intrinsics=np.zeros((b * v, 3, 3)), distortion=np.zeros((b, v, 5))), b)
    assert tuple(cams["intrinsics"].shape) == (b, v, 3, 3) and tuple(cams["distortion"].shape) == (b, v, 5)
    cfg.AL.USE_REPROJECTION_XE = True
    with pytest.raises(ValueError, match="XE metric"):
        st.score_batch(hm, dp)
    cfg.AL.USE_REPROJECTION_XE = False
    cfg.AL.UNDISTORT = "none"
    cfg.EVAL.UNDISTORT = "brown"

    def evaluate(cfg):  # (the network is replaced by its output: the host has no device to upload the images to)
        st = ActiveLearningStrategy(cfg)
        st._compute_batch_heatmap = lambda pose_estimator, data: hm
        return st.evaluate_mkpe([dp], None)

    with pytest.raises(KeyError, match="'intrinsics' and 'distortion'"):
        evaluate(cfg)
    cfg.EVAL.UNDISTORT = "fisheye"
    with pytest.raises(ValueError, match="'none', 'brown'"):
        evaluate(cfg)
    # older config nodes without the fields are "none": past the undistortion checks, the host heat-maps are refused further down
    del cfg.AL["UNDISTORT"], cfg.EVAL["UNDISTORT"]
    with pytest.raises(_lib.MvalError, match="HIP tensor"):
        evaluate(cfg)
    with pytest.raises(_lib.MvalError, match="HIP tensor"):
        st.score_batch(hm, dp)


def test_prepare_views_signature():
    import inspect

    from multi_view_active_learning_amd.utils.preprocess import prepare_views

    assert inspect.signature(prepare_views).parameters["with_cameras"].default is False

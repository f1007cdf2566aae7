"""2-D PCKh without a GPU: the NumPy float32 restatement of the reference's ``get_pred_coordinates`` (hard arg-max branch) and
``compute_pckh`` (tests/golden/pckh2d_cases.py) equals what the real reference returned (tests/golden/pckh2d.npz, written by
make_pckh2d_golden.py) on every case -- exact equality --, and the C ABI, the ctypes bindings, the EVAL.METRIC check and the
no-CPU-path rule of the new entry points are in place.  The GPU tests (test_gpu_pckh2d.py) compare the kernels with both."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pckh2d_cases as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mval_pred_coordinates", "mval_pred_coordinates_from_keys", "mval_pckh2d")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "pckh2d.npz"))


@pytest.fixture(scope="module")
def lib():
    from multi_view_active_learning_amd import _lib

    return _lib.lib()


def test_golden_file_holds_data_only_and_names_its_versions(golden):
    import json

    v = json.loads(str(golden["versions"]))
    assert set(v) == {"numpy", "torch", "python"}
    for k in golden.files:
        if k != "versions":
            assert golden[k].dtype in (np.float32, np.float64), k
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "pckh2d.npz")) < 100 * 1024


@pytest.mark.parametrize("name", ["noisy", "ties", "degenerate"])
def test_restated_pckh_equals_the_reference(golden, name):
    c = pc.metric_cases()[name]
    k = c["num_keypoints"]
    fig = pc.np_pckh(c["pred"], c["gt"], pc.THRESHOLDS, k)
    assert fig.shape == (10, k) == golden[name + "/figure"].shape
    np.testing.assert_array_equal(fig, golden[name + "/figure"])
    np.testing.assert_array_equal(pc.np_pckh(c["pred"], c["gt"], (0.5,), k)[0], golden[name + "/pckh_0_5"])
    np.testing.assert_array_equal(golden[name + "/figure"][4], golden[name + "/pckh_0_5"])
    if name == "degenerate":
        np.testing.assert_array_equal(pc.np_pckh(c["pred"], c["gt"], pc.THRESHOLDS, k, c["kp0"], c["kp1"]), golden[name + "/pckh_kp"])


def test_the_cases_can_tell_the_roundings_apart(golden):
    """What each case is there for, read off the reference's own numbers: in ``ties`` the product head * float32(t) left
    unrounded in double, or ``<=`` for ``<``, each change the counts (a product formed entirely in double does not: on integer
    distances it rounds to the same integers); in ``degenerate`` a zero head hits
    nothing, the NaN / +inf joints of image 1 miss at every threshold and the dis = 0 joint under a positive head hits at every one."""
    c = pc.metric_cases()["ties"]
    pred, gt = c["pred"].astype(np.float64), c["gt"].astype(np.float64)
    head = np.sqrt(((gt[:, 0] - gt[:, 1]) ** 2).sum(-1))
    dis = np.sqrt(((pred - gt) ** 2).sum(-1))
    want = golden["ties/figure"] * pred.shape[0]  # (every coordinate is a small integer: head and dis are exact in either precision)
    others = {
        "float32(t), product left in double": lambda t: dis < (head * np.float64(np.float32(t)))[:, None],
        "<= for <": lambda t: dis <= (head.astype(np.float32) * np.float32(t)).astype(np.float64)[:, None],
    }
    for what, hit in others.items():
        assert (np.stack([hit(t).sum(0) for t in pc.THRESHOLDS]) != want).any(), what
    assert (golden["ties/figure"][-1, 1] == 0.0) and golden["ties/figure"][0, 0] == 1.0  # dis == head at t = 1; dis == 0
    d = pc.metric_cases()["degenerate"]
    only0 = pc.np_pckh_hits(d["pred"][:1], d["gt"][:1], pc.THRESHOLDS, 5, 2, 5)
    assert (only0 == 0).all() and (pc.np_pckh_hits(d["pred"][:1], d["gt"][:1], pc.THRESHOLDS, 5) == 0).all()
    only1 = pc.np_pckh_hits(d["pred"][1:2], d["gt"][1:2], pc.THRESHOLDS, 5, 2, 5)
    assert (only1[:, :2] == 0).all() and (only1[:, 3] == 1).all()


@pytest.mark.parametrize("hh, wh", pc.DECODE_SIZES)
def test_restated_decode_equals_the_reference(golden, hh, wh):
    hm, boxes = pc.decode_case(hh, wh)
    want = golden[pc.decode_name(hh, wh) + "/xy"]
    got = pc.np_pred_coordinates(hm, boxes)
    assert want.dtype == np.float32 and got.dtype == np.float32 and got.shape == (3, 5, 2)
    np.testing.assert_array_equal(got, want)
    flat = hm.reshape(3, 5, -1).argmax(-1)
    assert (flat[:, 2] == hh * wh - 1).all() and (flat[:, 2] >= hh * (wh - 1)).all() and (flat[:, 3] == 0).all()
    assert ((hm[:, 1].reshape(3, -1) == 1.0).sum(1) == 2).all()  # the two-way tie
    if (hh, wh) == (8, 6):  # row 5, column 4 under the non-square box (10, 20, 110, 180)
        assert want[2, 0].tolist() == [np.float32(53.333332), 50.0]


def test_restated_pass_equals_the_reference(golden):
    loader, maps = pc.pass_case()
    assert [dp["square_box"].shape[:2] for dp in loader] == list(pc.PASS_BATCHES)
    pred = np.concatenate([pc.np_pred_coordinates(hm, dp["square_box"].reshape(-1, 4)) for dp, hm in zip(loader, maps)])
    gt = np.concatenate([dp["2d_after_crop"].reshape(-1, pc.J, 2) for dp in loader])
    np.testing.assert_array_equal(pc.np_pckh(pred, gt, pc.THRESHOLDS, pc.J), golden["pass/figure"])
    np.testing.assert_array_equal(pc.np_pckh(pred, gt, (0.5,), pc.J)[0], golden["pass/pckh_0_5"])
    assert 0.0 < golden["pass/figure"].min() and golden["pass/figure"][0].max() < 1.0 == golden["pass/figure"][-1].max()


def test_entries_are_declared_exported_and_bound(lib):
    from multi_view_active_learning_amd import _lib

    hdr = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int mval_pred_coordinates(const float* heatmaps, const float* boxes, float* xy, int64_t N, int J, int hh, int wh, "
            "void* stream);") in hdr
    assert ("int mval_pred_coordinates_from_keys(const uint64_t* keys, const float* boxes, float* xy, int64_t N, int J, int hh, "
            "int wh, void* stream);") in hdr
    assert ("int mval_pckh2d(const float* pred, const float* gt, const double* thresholds, int T, int kp0, int kp1, "
            "long long* hits, int64_t S, int J, int n_keypoints, void* stream);") in hdr
    for n in ENTRIES:
        assert hasattr(lib, n), f"{n} declared in include/mval_hip.h but not exported"
        assert callable(getattr(_lib, n[len("mval_"):]))
    import inspect

    assert list(inspect.signature(_lib.pred_coordinates).parameters) == ["hm", "boxes", "keys"]
    assert inspect.signature(_lib.pred_coordinates).parameters["keys"].default is None


def _pckh2d(lib, s=4, j=19, t=10, kp0=0, kp1=1, nk=19, ptr=1):
    """(The pointers are never dereferenced: every call here fails a check that comes before any launch.)"""
    p = ctypes.c_void_p(0x1000 * ptr)
    return lib.mval_pckh2d(p, p, p, ctypes.c_int(t), ctypes.c_int(kp0), ctypes.c_int(kp1), p, ctypes.c_longlong(s), ctypes.c_int(j),
                           ctypes.c_int(nk), ctypes.c_void_p(0))


@pytest.mark.parametrize("bad", [dict(j=1, nk=1), dict(kp1=19), dict(kp0=-1), dict(nk=20), dict(nk=0), dict(t=0), dict(s=-1), dict(ptr=0)],
                         ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_pckh2d_argument_checks_leave_a_message_and_launch_nothing(lib, bad):
    assert _pckh2d(lib, **bad) == -1
    assert b"mval_pckh2d" in lib.mval_last_error()


def test_pred_coordinates_argument_checks_launch_nothing(lib):
    p, z = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
    for entry in (lib.mval_pred_coordinates, lib.mval_pred_coordinates_from_keys):
        call = lambda a=p, n=2, j=3, hh=8, wh=6: entry(a, p, p, ctypes.c_longlong(n), ctypes.c_int(j), ctypes.c_int(hh), ctypes.c_int(wh), z)  # noqa: E731
        for bad in (dict(n=-1), dict(j=0), dict(hh=0), dict(wh=-2), dict(hh=4096, wh=4096), dict(a=z)):
            assert call(**bad) == -1 and b"mval_pred_coordinates" in lib.mval_last_error(), bad
        assert call(n=0) == 0  # nothing to do, nothing launched


def test_check_eval_metric():
    from multi_view_active_learning_amd import config

    assert config.EVAL_METRICS == ("2DPCKH", "3DPCK", "3DPCKH", "MKPE")
    for m in config.EVAL_METRICS:
        assert config.check_eval_metric(m) == m
    assert config.check_eval_metric(config.get_default_configs().EVAL.METRIC) == "3DPCK"
    with pytest.raises(NotImplementedError) as e:
        config.check_eval_metric("PCK")
    for m in config.EVAL_METRICS:
        assert repr(m) in str(e.value)


def test_strategy_has_the_pass_and_rejects_an_unknown_metric_before_any_work():
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    st = ActiveLearningStrategy(get_default_configs())
    for n in ("_compute_pred_labels", "evaluate_2d_pckh", "evaluate"):
        assert callable(getattr(st, n))
    with pytest.raises(NotImplementedError):
        st.evaluate(iter(()), None, metric="PCK")  # (an exhausted loader: the check comes first)


def test_no_cpu_path():
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils import evaluation

    c = pc.metric_cases()["noisy"]
    pred, gt = torch.from_numpy(c["pred"]), torch.from_numpy(c["gt"])
    for args in ((pred, gt), ([pred[:16], pred[16:]], [gt[:16], gt[16:]]), (pred.reshape(1, 37, 19, 2), gt.reshape(1, 37, 19, 2))):
        with pytest.raises(_lib.MvalError):
            evaluation.compute_pckh(*args, 0.5, 19)
        with pytest.raises(_lib.MvalError):
            evaluation.compute_pckh_0_5(*args, 19)
        with pytest.raises(_lib.MvalError):
            evaluation.compute_pckh_figure(*args, 19)
    hm, boxes = pc.decode_case(8, 6)
    with pytest.raises(_lib.MvalError):
        evaluation.pred_coordinates_batch(torch.from_numpy(hm), torch.from_numpy(boxes))
    with pytest.raises(_lib.MvalError):
        _lib.pred_coordinates(torch.from_numpy(hm), torch.from_numpy(boxes))
    with pytest.raises(_lib.MvalError):
        _lib.pckh2d(pred, gt, (0.5,), 19)


def test_no_image_divides_by_zero_like_the_reference():
    from multi_view_active_learning_amd.utils import evaluation

    with pytest.raises(ZeroDivisionError):
        evaluation.compute_pckh([], [], 0.5, 19)
    with pytest.raises(ZeroDivisionError):
        evaluation.compute_pckh_figure([], [], 19)

"""Host tests (no GPU) of the weighted training loss: the five entries in the header and the library and their
argument checks, the ctypes calls of the _lib wrappers against the header, TRAIN.LOSS and its validator, compose_joint_weights,
which loss entries train_step reaches, and the properties of the oracle (tests/weighted_loss_oracle.py) the GPU tests rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import weighted_loss_oracle as wo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mval_weighted_mse_workspace_bytes", "mval_weighted_mse_fwd", "mval_weighted_mse_points_fwd", "mval_weighted_mse_bwd",
           "mval_weighted_mse_points_bwd")


def _header_args():
    """entry -> the parameter types of its declaration in include/mval_hip.h"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mval_hip.h")).read(), flags=re.S)
    out = {}
    for n in ENTRIES:
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)" % n, hdr)
        assert decl, n + " is not declared in include/mval_hip.h"
        out[n] = [" ".join(a.split()).rsplit(" ", 1)[0] for a in decl.group(1).split(",")]
    return out


def _lib_built():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


# ---- plumbing --------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported():
    _lib = _lib_built()
    args = _header_args()
    for n in ENTRIES:
        assert hasattr(_lib.lib(), n), n + " is not exported"
    assert _lib.lib().mval_weighted_mse_workspace_bytes.restype is C.c_size_t
    assert args["mval_weighted_mse_workspace_bytes"] == ["int64_t", "int"]
    # both forwards end in the three outputs, the workspace and the sizes; the points forms put (pt, sigma, sigma_per_map) for g
    tail = ["int64_t", "int", "int", "int", "void*"]
    assert args["mval_weighted_mse_fwd"] == ["const float*", "const float*", "const float*", "int", "float*", "double*", "float*", "void*"] + tail
    assert args["mval_weighted_mse_points_fwd"] == ["const float*", "const double*", "double", "const double*", "const float*", "int", "float*",
                                                    "double*", "float*", "void*"] + tail
    assert args["mval_weighted_mse_bwd"] == ["const float*", "const float*", "const float*", "const float*", "float*"] + tail
    assert args["mval_weighted_mse_points_bwd"] == ["const float*", "const double*", "double", "const double*", "const float*", "const float*",
                                                    "float*"] + tail
    assert _lib.weighted_mse_workspace_bytes(128, 19) >= 128 * 19 * 8 and _lib.weighted_mse_workspace_bytes(0, 19) == 0


def test_ctypes_calls_match_the_header(monkeypatch):
    """Every wrapper hands its entry one ctypes value per declared parameter, of the declared kind."""
    from multi_view_active_learning_amd import _lib

    seen = {}

    class FakeLib:
        def __getattr__(self, name):
            def entry(*a):
                seen[name] = [type(x) for x in a]
                return 0
            return entry

    monkeypatch.setattr(_lib, "lib", lambda: FakeLib())
    monkeypatch.setattr(_lib, "_p", lambda t: C.c_void_p(0))
    monkeypatch.setattr(_lib, "_stream", lambda: C.c_void_p(0))
    monkeypatch.setattr(_lib, "_points_args", lambda *a: None)
    n, j, hh, wh = 2, 3, 4, 5
    h = torch.zeros(n * j * hh * wh)
    pt = torch.zeros((n * j, 2), dtype=torch.float64)
    w = torch.ones(n * j)
    go = torch.ones(())
    _lib.weighted_mse_fwd(h, h, w, 2, n, j, hh, wh)
    _lib.weighted_mse_points_fwd(h, pt, 1.0, w, 2, n, j, hh, wh)
    _lib.weighted_mse_bwd(h, h, w, go, n, j, hh, wh)
    _lib.weighted_mse_points_bwd(h, pt, np.ones(n * j), w, go, n, j, hh, wh)
    kind = {"int": C.c_int, "int64_t": C.c_longlong, "double": C.c_double}
    for name, types in _header_args().items():
        assert seen[name] == [kind.get(t, C.c_void_p) for t in types], name


def test_entries_refuse_bad_arguments_without_a_launch():
    """topk outside [0, J], a null out, a scalar sigma <= 0 and bad sizes return -1 with the entry's name in mval_last_error()."""
    _lib = _lib_built()
    lib = _lib.lib()
    null, some = C.c_void_p(0), C.c_void_p(64)  # (never dereferenced: every call below is refused before a launch)

    def fwd(points, topk=2, out=some, sigma=1.0, n=2, j=3, hh=4, wh=5, h=some):
        tail = (C.c_int(topk), out, some, some, some, C.c_longlong(n), C.c_int(j), C.c_int(hh), C.c_int(wh), null)
        if points:
            return lib.mval_weighted_mse_points_fwd(h, some, C.c_double(sigma), null, some, *tail)
        return lib.mval_weighted_mse_fwd(h, some, some, *tail)

    def bwd(points, sigma=1.0, n=2, j=3, hh=4, wh=5, gh=some):
        tail = (some, some, gh, C.c_longlong(n), C.c_int(j), C.c_int(hh), C.c_int(wh), null)
        if points:
            return lib.mval_weighted_mse_points_bwd(some, some, C.c_double(sigma), null, *tail)
        return lib.mval_weighted_mse_bwd(some, some, *tail)

    both = [dict(n=-1), dict(j=0), dict(hh=0), dict(wh=-1), dict(hh=65536, wh=65536), dict(hh=46341, wh=46341), dict(n=2 ** 31, j=3)]
    for points, name in ((False, b"mval_weighted_mse_fwd"), (True, b"mval_weighted_mse_points_fwd")):
        for bad in both + [dict(topk=4), dict(topk=-1), dict(out=null), dict(h=null)] + ([dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan"))] if points else []):
            assert fwd(points, **bad) == -1, (name, bad)
            assert name in lib.mval_last_error(), (name, bad, lib.mval_last_error())
    for points, name in ((False, b"mval_weighted_mse_bwd"), (True, b"mval_weighted_mse_points_bwd")):
        for bad in both + [dict(gh=null)] + ([dict(sigma=0.0), dict(sigma=float("nan"))] if points else []):
            assert bwd(points, **bad) == -1, (name, bad)
            assert name in lib.mval_last_error(), (name, bad, lib.mval_last_error())
    assert bwd(False, n=0) == 0 and bwd(True, n=0) == 0  # no maps: nothing to launch


def test_wrappers_check_host_weights():
    """Weights that arrive on the host are checked there; the count must be the maps'."""
    from multi_view_active_learning_amd import _lib

    cpu = torch.device("cpu")
    for bad in ([1.0, -0.5, 1.0], [1.0, float("nan"), 1.0], [float("inf"), 1.0, 1.0]):
        with pytest.raises(_lib.MvalError, match="weights must be finite and >= 0"):
            _lib.loss_weights(torch.tensor(bad), 3, cpu, "mval_weighted_mse_fwd")
    with pytest.raises(_lib.MvalError, match="2 weights for 3 maps"):
        _lib.loss_weights(torch.ones(2), 3, cpu, "mval_weighted_mse_fwd")
    w = _lib.loss_weights(np.array([0.0, 2.0, 0.5]), 3, cpu, "mval_weighted_mse_fwd")
    assert w.dtype == torch.float32 and w.tolist() == [0.0, 2.0, 0.5]


# ---- configuration ---------------------------------------------------------------------------------------------------------
def test_defaults_and_check_train_loss():
    from multi_view_active_learning_amd.config import check_train_loss, get_default_configs

    cfg = get_default_configs()
    node = cfg.TRAIN.LOSS
    assert (node.JOINT_WEIGHTS, node.OHKM_TOPK, node.PSEUDO_LABEL_WEIGHT, node.WEIGHT_KEY) == ([], 0, 1.0, "")
    assert type(node.OHKM_TOPK) is int and type(node.PSEUDO_LABEL_WEIGHT) is float
    j = 19
    assert check_train_loss(node, j) == ((), 0, 1.0, "")
    node.JOINT_WEIGHTS, node.OHKM_TOPK, node.PSEUDO_LABEL_WEIGHT, node.WEIGHT_KEY = [1.0] * 18 + [2], j, 0, "joint_weight"
    assert check_train_loss(node, j) == ((1.0,) * 18 + (2.0,), j, 0.0, "joint_weight")

    def refused(match, **fields):
        n = get_default_configs().TRAIN.LOSS
        for k, v in fields.items():
            setattr(n, k, v)
        with pytest.raises(ValueError, match=match):
            check_train_loss(n, j)

    refused("JOINT_WEIGHTS.*19 finite numbers >= 0", JOINT_WEIGHTS=[1.0] * 18)
    refused("JOINT_WEIGHTS", JOINT_WEIGHTS=[1.0] * 20)
    refused("JOINT_WEIGHTS", JOINT_WEIGHTS=[1.0] * 18 + [-0.5])
    refused("JOINT_WEIGHTS", JOINT_WEIGHTS=[1.0] * 18 + [float("nan")])
    refused("JOINT_WEIGHTS", JOINT_WEIGHTS=[1.0] * 18 + [float("inf")])
    refused("JOINT_WEIGHTS", JOINT_WEIGHTS=[1.0] * 18 + [True])
    refused("JOINT_WEIGHTS", JOINT_WEIGHTS="1.0")
    refused(r"OHKM_TOPK.*integer in \[0, 19\]", OHKM_TOPK=j + 1)
    refused("OHKM_TOPK", OHKM_TOPK=-1)
    refused("OHKM_TOPK", OHKM_TOPK=True)
    refused("OHKM_TOPK", OHKM_TOPK=8.0)
    refused("PSEUDO_LABEL_WEIGHT.*finite number >= 0", PSEUDO_LABEL_WEIGHT=-1.0)
    refused("PSEUDO_LABEL_WEIGHT", PSEUDO_LABEL_WEIGHT=float("nan"))
    refused("PSEUDO_LABEL_WEIGHT", PSEUDO_LABEL_WEIGHT=False)
    refused("WEIGHT_KEY.*string", WEIGHT_KEY=3)


def test_compose_joint_weights():
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import compose_joint_weights

    rng = np.random.default_rng(11)
    b, v, j = 3, 2, 19
    valid = (rng.uniform(size=(b, v, j)) > 0.3).astype(np.float32) * 2.0  # (nonzero means valid, whatever the value)
    node = get_default_configs().TRAIN.LOSS
    data = {"per_view_joint_valid": torch.from_numpy(valid)}
    assert compose_joint_weights(data["per_view_joint_valid"], node, data) is None
    assert compose_joint_weights(data["per_view_joint_valid"], None, data) is None
    assert compose_joint_weights(data["per_view_joint_valid"], node, dict(data, joint_weight=torch.ones(b, v, j))) is None  # not the named key

    jw = rng.uniform(0, 2, j).astype(np.float32)
    extra = rng.uniform(0, 2, (b, v, j)).astype(np.float32)
    pseudo = np.array([1, 0, 3])
    node.JOINT_WEIGHTS, node.PSEUDO_LABEL_WEIGHT, node.WEIGHT_KEY = [float(x) for x in jw], 0.3, "joint_weight"
    data.update(pseudo_label=torch.from_numpy(pseudo), joint_weight=torch.from_numpy(extra))
    got = compose_joint_weights(data["per_view_joint_valid"], node, data)
    one = np.float32(1.0)
    want = (valid != 0).astype(np.float32) * jw.reshape(1, 1, j)
    want = want * np.where(pseudo != 0, np.float32(0.3), one).reshape(b, 1, 1)
    want = want * extra
    assert got.dtype == torch.float32 and got.shape == (b, v, j) and want.dtype == np.float32
    np.testing.assert_array_equal(got.numpy().view(np.int32), want.view(np.int32))

    # each single cause switches the weights on, and a missing factor is 1
    ones = (valid != 0).astype(np.float32)
    base = {"per_view_joint_valid": torch.from_numpy(valid)}
    for field, value in (("OHKM_TOPK", 8), ("PSEUDO_LABEL_WEIGHT", 0.5), ("WEIGHT_KEY", "joint_weight")):
        n2 = get_default_configs().TRAIN.LOSS
        setattr(n2, field, value)
        np.testing.assert_array_equal(compose_joint_weights(base["per_view_joint_valid"], n2, base).numpy(), ones)
    n2 = get_default_configs().TRAIN.LOSS
    got = compose_joint_weights(base["per_view_joint_valid"], n2, dict(base, pseudo_label=np.array([0, 1, 0])))
    np.testing.assert_array_equal(got.numpy(), ones)  # PSEUDO_LABEL_WEIGHT 1.0
    for bad in (dict(pseudo_label=np.zeros(b + 1)), dict(joint_weight=np.ones((b, v, j + 1)))):
        with pytest.raises(ValueError, match="compose_joint_weights"):
            compose_joint_weights(base["per_view_joint_valid"], node, dict(base, **bad))
    node.JOINT_WEIGHTS = [1.0] * (j - 1)
    with pytest.raises(ValueError, match="JOINT_WEIGHTS"):
        compose_joint_weights(base["per_view_joint_valid"], node, base)


# ---- train_step ------------------------------------------------------------------------------------------------------------
LOSS_ENTRIES = ("masked_mse_fwd", "masked_mse_bwd", "masked_mse_points_fwd", "masked_mse_points_bwd", "weighted_mse_fwd", "weighted_mse_bwd",
                "weighted_mse_points_fwd", "weighted_mse_points_bwd")


def _train_step_calls(monkeypatch, kind, fields=None, extra=None, drop_node=False):
    """One train_step on the host with the eight loss entries of _lib replaced by recorders: [(entry, topk or None), ...]."""
    from multi_view_active_learning_amd import _lib, strategy
    from multi_view_active_learning_amd.config import get_default_configs

    calls = []

    def recorder(name):
        def f(*a):
            h = a[0]
            calls.append((name, a[4 if "points" in name else 3] if name.startswith("weighted") and name.endswith("fwd") else None))
            if name.endswith("bwd"):
                return torch.zeros_like(h)
            out = torch.tensor(0.25)
            if name.startswith("weighted"):
                lead = h.shape[0] * h.shape[1]
                return out, torch.zeros(lead, dtype=torch.float64), torch.zeros(lead)
            return out
        return f

    for name in LOSS_ENTRIES:
        monkeypatch.setattr(_lib, name, recorder(name))
    monkeypatch.setattr(strategy, "_stage_small", lambda t: t)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    cfg = get_default_configs()
    for k, v in (fields or {}).items():
        setattr(cfg.TRAIN.LOSS, k, v)
    if drop_node:
        del cfg.TRAIN["LOSS"]
    b, v, j, hh, wh = 2, 2, cfg.DATA.NUM_JOINTS, 4, 4
    torch.manual_seed(0)
    net = torch.nn.Conv2d(3, j, 1)
    data = {"images": torch.randn(b, v, 3, hh, wh), "per_view_joint_valid": torch.ones(b, v, j)}
    if kind == "gt_heatmap":
        data["gt_heatmap"] = torch.zeros(b, v, j, hh, wh)
    else:
        data["gt_points"] = torch.ones(b, v, j, 2, dtype=torch.float64)
    data.update(extra or {})
    value, stepped = strategy.ActiveLearningStrategy(cfg).train_step(net, torch.optim.SGD(net.parameters(), lr=0.1), data)
    assert (value, stepped) == (0.25, True)
    return calls


@pytest.mark.parametrize("kind", ["gt_heatmap", "points"])
def test_train_step_reaches_the_weighted_loss_only_when_asked(monkeypatch, kind):
    p = "points_" if kind == "points" else ""
    today = [("masked_mse_%sfwd" % p, None), ("masked_mse_%sbwd" % p, None)]
    assert _train_step_calls(monkeypatch, kind) == today
    assert _train_step_calls(monkeypatch, kind, drop_node=True) == today  # a config from before TRAIN.LOSS
    assert _train_step_calls(monkeypatch, kind, dict(OHKM_TOPK=8)) == [("weighted_mse_%sfwd" % p, 8), ("weighted_mse_%sbwd" % p, None)]
    assert _train_step_calls(monkeypatch, kind, extra=dict(pseudo_label=torch.tensor([1, 0]))) == [("weighted_mse_%sfwd" % p, 0), ("weighted_mse_%sbwd" % p, None)]
    with pytest.raises(ValueError, match="finite and >= 0"):
        _train_step_calls(monkeypatch, kind, dict(WEIGHT_KEY="jw"), extra=dict(jw=torch.full((2, 2, 19), -1.0)))


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_topk_all_is_no_mining():
    rng = np.random.default_rng(3)
    n, j = 4, 19
    S = rng.uniform(0, 50, (n, j))
    w = rng.uniform(0, 2, (n, j)).astype(np.float32)
    w[rng.uniform(size=(n, j)) < 0.3] = 0
    a, b = wo.forward(w, S, 0, 64.0), wo.forward(w, S, j, 64.0)
    assert a[0].view(np.int32) == b[0].view(np.int32)
    np.testing.assert_array_equal(a[2].view(np.int32), b[2].view(np.int32))
    np.testing.assert_array_equal(a[2], w)
    np.testing.assert_array_equal(a[1], w.astype(np.float64) * S)
    # fewer joints only remove terms: the loss falls (weakly) with topk, and topk = 1 keeps each image's largest term
    losses = [float(wo.forward(w, S, k, 64.0)[0]) for k in range(1, j + 1)]
    assert all(x <= y for x, y in zip(losses, losses[1:]))
    assert wo.forward(w, S, 1, 64.0)[0] == np.float32(sum(a[1][i].max() for i in range(n)) / 64.0)
    assert wo.forward(np.zeros((0, j), np.float32), np.zeros((0, j)), 0, 1.0)[0] == 0


def test_oracle_ties_and_nan_ranking():
    w = np.ones((1, 6), np.float32)
    S = np.array([[1.0, 5.0, 3.0, 5.0, 0.0, 5.0]])
    for k, want in ((1, [1]), (2, [1, 3]), (3, [1, 3, 5]), (4, [1, 2, 3, 5])):  # the lower index wins a tie
        assert np.flatnonzero(wo.select(wo.per_map_loss(w, S), w, k)[0][0]).tolist() == want
    S[0, 4] = np.nan
    loss, l, wsel = wo.forward(w, S, 1, 6.0)  # NaN is the maximum
    assert np.isnan(loss) and np.flatnonzero(wsel[0]).tolist() == [4]
    S[0, 0] = np.nan
    assert np.flatnonzero(wo.forward(w, S, 1, 6.0)[2][0]).tolist() == [0]  # and two NaNs tie to the lower index
    assert np.flatnonzero(wo.forward(w, S, 3, 6.0)[2][0]).tolist() == [0, 1, 4]
    w[0, [0, 4]] = 0  # a map of weight 0 has S = +0.0 on the device, never a NaN: l = 0 ranks last among non-negative values
    S[0, [0, 4]] = 0.0
    loss, l, wsel = wo.forward(w, S, 6, 6.0)
    assert loss == np.float32(18.0 / 6.0) and wsel[0].tolist() == [0, 1, 1, 1, 0, 1]
    g = wo.gradient(np.full((1, 6, 4), np.nan, np.float32), np.zeros((1, 6, 4), np.float32), np.zeros((1, 6), np.float32), 1.0, 4.0)
    assert not g.view(np.int32).any()  # +0.0 whatever the map holds

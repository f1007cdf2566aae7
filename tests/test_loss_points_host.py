"""CPU (no GPU): the points form of the training loss is declared and exported, and train_step's target selection
(strategy.select_train_target) picks what it should."""
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mval_masked_mse_points_fwd", "mval_masked_mse_points_bwd")


@pytest.fixture(scope="module")
def lib():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_points_entries_are_declared_and_exported(lib):
    from multi_view_active_learning_amd import _lib

    hdr = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(mval_[a-z0-9_]+)\s*\(", hdr))
    for n in ENTRIES:
        assert n in names, f"{n} is not declared in include/mval_hip.h"
        assert hasattr(lib, n), f"{n} declared in include/mval_hip.h but not exported"
        assert callable(getattr(_lib, n[len("mval_"):]))


def _cfg():
    from multi_view_active_learning_amd.config import get_default_configs

    cfg = get_default_configs()
    cfg.DATA.SIGMA = 1.5
    cfg.POSE_ESTIMATOR.STRIDE = 4
    return cfg


def _batch():
    rng = np.random.default_rng(0)
    return {
        "gt_heatmap": torch.from_numpy(rng.standard_normal((2, 2, 3, 4, 4)).astype(np.float32)),
        "gt_points": torch.from_numpy(rng.uniform(0, 4, (2, 2, 3, 2))),
        "2d_keypoints": torch.from_numpy(rng.uniform(0, 16, (2, 2, 3, 2)).astype(np.float32)),
        "gt_sigma": torch.tensor([1.0, 2.0], dtype=torch.float64),
    }


def test_target_order():
    from multi_view_active_learning_amd.strategy import select_train_target

    cfg, full = _cfg(), _batch()
    kind, target, sigma = select_train_target(full, cfg)
    assert kind == "gt_heatmap" and target is full["gt_heatmap"] and sigma is None
    data = {k: v for k, v in full.items() if k != "gt_heatmap"}
    kind, target, sigma = select_train_target(data, cfg)
    assert kind == "points" and target.dtype == torch.float64 and torch.equal(target, full["gt_points"])
    data.pop("gt_points")
    kind, target, sigma = select_train_target(data, cfg)
    assert kind == "points" and target.dtype == torch.float64
    assert torch.equal(target, full["2d_keypoints"].to(torch.float64) / 4)  # the division is float64's, after the cast
    # numpy batches are taken too
    kind, target, _ = select_train_target({"2d_keypoints": full["2d_keypoints"].numpy()}, cfg)
    assert kind == "points" and torch.equal(target, full["2d_keypoints"].to(torch.float64) / 4)


def test_sigma_order():
    from multi_view_active_learning_amd.strategy import select_train_target

    cfg, full = _cfg(), _batch()
    data = {"gt_points": full["gt_points"], "gt_sigma": full["gt_sigma"]}
    assert select_train_target(data, cfg)[2] is full["gt_sigma"]
    data.pop("gt_sigma")
    assert select_train_target(data, cfg)[2] == 1.5
    assert select_train_target({"2d_keypoints": full["2d_keypoints"]}, cfg)[2] == 1.5


def test_no_target_raises():
    from multi_view_active_learning_amd.strategy import select_train_target

    with pytest.raises(KeyError) as e:
        select_train_target({"images": torch.zeros(1), "gt_sigma": torch.ones(1)}, _cfg())
    for k in ("gt_heatmap", "gt_points", "2d_keypoints"):
        assert k in str(e.value)


def test_heatmap_batch_is_left_alone():
    from multi_view_active_learning_amd.strategy import select_train_target

    full = _batch()
    keys, ids = list(full), {k: id(v) for k, v in full.items()}
    copies = {k: v.clone() for k, v in full.items()}
    select_train_target(full, _cfg())
    assert list(full) == keys and {k: id(v) for k, v in full.items()} == ids
    assert all(torch.equal(full[k], copies[k]) for k in full)

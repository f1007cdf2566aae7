"""Inputs of the CLUSTER-pass goldens (tests/golden/cluster.json), regenerated from seeds on both sides: the generator
(make_cluster_golden.py, the real reference's ``cluster()``) and the tests (tests/test_cluster_host.py,
tests/test_gpu_cluster.py).  Nothing but numpy here."""
from collections import OrderedDict

import numpy as np


def cluster_cases():
    """``ids``: how ``pose`` / ``frame_id`` reach OUR pass -- "B" as (B,), "B1" as (B, 1); the generator turns either into
    the layouts the reference's indexing runs on (make_cluster_golden.reference_batch)."""
    return OrderedDict(
        loss_v4_64x64=dict(type="LOSS", seed=71, sizes=(3, 2), v=4, j=19, hh=64, wh=64, ids="B"),
        loss_v2_64x48=dict(type="LOSS", seed=72, sizes=(3, 2), v=2, j=19, hh=64, wh=48, ids="B1"),
        pose_j19=dict(type="POSE", seed=73, sizes=(3, 2), j=19, rows=4, ids="B1"),
        pose_j42=dict(type="POSE", seed=74, sizes=(3, 2), j=42, rows=4, ids="B"),
    )


def _ids(c, i, b):
    pose = (np.arange(b, dtype=np.int64) % 2) * 11 + 3 + i
    frame = np.arange(b, dtype=np.int64) * 3 + 100 * i + 1
    if c["ids"] == "B1":
        pose, frame = pose[:, None], frame[:, None]
    return pose, frame


def gaussian_maps(pt, sigma, hh, wh):
    """dataset.py:198-207 in numpy: pt (..., 2) float64 heat-map pixels -> (..., hh, wh) float32."""
    y, x = np.mgrid[0:hh, 0:wh].astype(np.float64)
    d2 = (x - pt[..., 0, None, None]) ** 2 + (y - pt[..., 1, None, None]) ** 2
    return np.exp(-d2 / (2.0 * sigma ** 2)).astype(np.float32)


def build_cluster_loader(c):
    """-> (list of batch dicts with numpy values, list of heat-map batches (B*V, J, hh, wh) float32; empty for POSE).
    LOSS batches carry ``gt_heatmap`` (B, V, J, hh, wh) float32, the reference loader's field: Gaussians at random joints;
    the heat-maps are those plus noise, a shift and two dead views -- losses of different sizes."""
    loader, hms = [], []
    for i, b in enumerate(c["sizes"]):
        rng = np.random.default_rng(c["seed"] * 10 + i)
        pose, frame = _ids(c, i, b)
        dp = dict(pose=pose, frame_id=frame)
        if c["type"] == "POSE":
            kp = (rng.standard_normal((b, c["rows"], c["j"])) * 250.0).astype(np.float32)
            kp[:, 3:] = 1.0  # (the confidence row)
            dp["3d_keypoints"] = kp
        else:
            v, j, hh, wh = c["v"], c["j"], c["hh"], c["wh"]
            pt = rng.random((b, v, j, 2)) * np.array([wh + 8.0, hh + 8.0]) - 4.0
            gt = gaussian_maps(pt, 1.0, hh, wh)
            hm = gt * rng.uniform(0.5, 1.1, (b, v, j, 1, 1)).astype(np.float32) + (rng.standard_normal(gt.shape) * 0.05).astype(np.float32)
            hm[0, 0] = 0.0
            hm[-1, -1] = rng.standard_normal((j, hh, wh)).astype(np.float32)
            dp["images"] = np.zeros((b, v, 3, 8, 8), dtype=np.float32)
            dp["gt_heatmap"] = gt
            hms.append(np.ascontiguousarray(hm.reshape(b * v, j, hh, wh).astype(np.float32)))
        loader.append(dp)
    return loader, hms


def frame_loss_f64(hm, gt):
    """The float64 reference value of a frame's loss: float32(h - g), squared in float32, summed and divided by
    hh * wh in float64.  hm, gt (..., V, J, hh, wh) float32 -> (...,) float64."""
    d = hm.astype(np.float32) - gt.astype(np.float32)
    sq = (d * d).astype(np.float32)
    return sq.astype(np.float64).sum(axis=(-1, -2, -3, -4)) / float(hm.shape[-1] * hm.shape[-2])


def ulp32(x):
    """One float32 unit in the last place at |x| (float64)."""
    return float(np.spacing(np.float32(abs(x))))

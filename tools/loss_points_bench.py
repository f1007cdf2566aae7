#!/usr/bin/env python3
"""What a compact training batch (key-point targets, uint8 views) costs and saves on the device, at the C3 size (128 images x 19 x 64 x 64,
views 256 x 256) and at 64 x 19 x 96 x 72 (views 384 x 288).  Six ways alternated over --rounds rounds of at least --window seconds each,
median of the rounds:

  loss_read      (a) mval_masked_mse_fwd + _bwd on device-resident ground-truth maps
  loss_points    (b) mval_masked_mse_points_fwd + _bwd: the maps rendered per pixel, twice
  gt_copy        (c) the ground-truth maps from pinned host memory to the device: the copy the points form removes
  points_copy        the copy it adds: the points (lead x 2 float64) from pinned host memory
  views_f32      (d) the normalised float32 views from pinned host memory
  views_u8       (d) the uint8 views from pinned host memory + mval_normalize_views_u8

Every time is device events around back-to-back calls on one stream (python wrappers and output allocation included, no synchronisation
inside).  The comparisons are (b) + points_copy against (a) + (c), and views_u8 against views_f32.  The loss kernels' results are compared in
bits before anything is timed.
GPU box: python tools/loss_points_bench.py [--rounds 3] [--window 0.5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multi_view_active_learning_amd import _lib
from multi_view_active_learning_amd.utils.preprocess import gt_heatmaps, normalize_views_u8

# images, joints, heat-map (hh, wh), view (H, W)
SHAPES = {"c3": (128, 19, 64, 64, 256, 256), "c4": (64, 19, 96, 72, 384, 288)}


def device_time(fn, window):
    """Seconds per call of fn: device events around n back-to-back calls, n doubled until the window is filled."""
    n = 8
    while True:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        t = start.elapsed_time(stop) * 1e-3
        if t >= window:
            return t / n
        n *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path to time)"
    dev = torch.device("cuda:0")
    for name, (n, j, hh, wh, vh, vw) in SHAPES.items():
        rng = np.random.default_rng(n)
        lead, hw, denom = n * j, hh * wh, float(n * hh * wh)
        pt_host = torch.from_numpy(rng.random((lead, 2)) * np.array([wh, hh], dtype=np.float64)).pin_memory()
        pt = pt_host.to(dev)
        gt = gt_heatmaps(pt, 1.0, hh, wh).reshape(-1)
        hm = gt + 0.05 * torch.randn(gt.shape, device=dev)
        valid = torch.from_numpy((rng.random(lead) > 0.2).astype(np.uint8)).to(dev)
        go = torch.ones((), dtype=torch.float32, device=dev)
        gt_host = gt.cpu().pin_memory()
        u8_host = torch.from_numpy(rng.integers(0, 256, size=(n, vh, vw, 3), dtype=np.uint8)).pin_memory()
        f32_host = normalize_views_u8(u8_host.to(dev)).cpu().pin_memory()

        def loss_read():
            _lib.masked_mse_fwd(hm, gt, valid, lead, hw, denom)
            return _lib.masked_mse_bwd(hm, gt, valid, go, lead, hw, denom)

        def loss_points():
            _lib.masked_mse_points_fwd(hm, pt, 1.0, valid, lead, hh, wh, denom)
            return _lib.masked_mse_points_bwd(hm, pt, 1.0, valid, go, lead, hh, wh, denom)

        ways = {
            "loss_read": loss_read,
            "loss_points": loss_points,
            "gt_copy": lambda: gt_host.to(dev, non_blocking=True),
            "points_copy": lambda: pt_host.to(dev, non_blocking=True),
            "views_f32": lambda: f32_host.to(dev, non_blocking=True),
            "views_u8": lambda: normalize_views_u8(u8_host.to(dev, non_blocking=True)),
        }
        # the same bits, and a warm-up of every way
        assert torch.equal(_lib.masked_mse_fwd(hm, gt, valid, lead, hw, denom).view(torch.int32),
                           _lib.masked_mse_points_fwd(hm, pt, 1.0, valid, lead, hh, wh, denom).view(torch.int32))
        assert torch.equal(loss_read().view(torch.int32), loss_points().view(torch.int32))
        assert torch.equal(ways["views_f32"]().view(torch.int32), ways["views_u8"]().view(torch.int32))
        ways["gt_copy"](), ways["points_copy"]()
        torch.cuda.synchronize()
        times = {k: [] for k in ways}
        for _ in range(args.rounds):
            for k, fn in ways.items():
                times[k].append(device_time(fn, args.window))
        out = dict(shape=name, images=n, joints=j, hh=hh, wh=wh, view_h=vh, view_w=vw, rounds=args.rounds, window_s=args.window,
                   gt_bytes=lead * hw * 4, points_bytes=lead * 16, views_f32_bytes=n * 3 * vh * vw * 4, views_u8_bytes=n * 3 * vh * vw)
        med = {}
        for k in ways:
            med[k] = float(np.median(times[k]))
            out[k + "_us"] = round(med[k] * 1e6, 2)
            out[k + "_spread_us"] = [round(min(times[k]) * 1e6, 2), round(max(times[k]) * 1e6, 2)]
        out["read_plus_gt_copy_us"] = round((med["loss_read"] + med["gt_copy"]) * 1e6, 2)
        out["points_plus_points_copy_us"] = round((med["loss_points"] + med["points_copy"]) * 1e6, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

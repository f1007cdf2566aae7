#!/usr/bin/env python3
"""Per-frame heat-map loss of a batch (csrc/frame_loss.hip) at the C2 and C4 batch sizes, three ways of getting the same
B numbers, alternated over --rounds rounds of at least --window seconds each, median of the rounds:

  fused_gt      Pose2DMeanSquaredError.pose_2d_mse_per_frame (mval_frame_loss: reads heat-maps and ground truth)
  fused_points  pose_2d_mse_per_frame_from_points (mval_frame_loss_points: renders the ground truth per pixel)
  per_frame     the loop this replaces: B calls of pose_2d_mse_single_batch, each followed by .item()

The fused times are device events around back-to-back CALLS (python wrapper, output allocation and both launches
included, no synchronisation inside); per_frame is the host clock around the loop, which synchronises at every .item().
"bytes/time" is the algorithm's bytes (2 * n * hw * 4 for the ground-truth forms, half that for the points form) over that
call time -- a call-level rate, not a kernel's share of peak.
GPU box: python tools/frame_loss_bench.py [--rounds 3] [--window 0.5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError
from multi_view_active_learning_amd.utils.preprocess import gt_heatmaps

SHAPES = {"c2": (32, 4, 19, 64, 64), "c4": (8, 8, 19, 96, 72)}


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


def host_time(fn, window):
    """Seconds per call of a fn that ends synchronised: host clock, calls repeated until the window is filled."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        t = time.perf_counter() - t0
        if t >= window:
            return t / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (there is no CPU path to time)"
    dev = torch.device("cuda:0")
    loss = Pose2DMeanSquaredError()
    for name, (b, v, j, hh, wh) in SHAPES.items():
        rng = np.random.default_rng(b)
        pt = torch.from_numpy(rng.random((b, v, j, 2)) * np.array([wh, hh], dtype=np.float64)).to(dev)
        gt = gt_heatmaps(pt, 1.0, hh, wh)
        hm = gt + 0.05 * torch.randn(gt.shape, device=dev)
        ways = {
            "fused_gt": (device_time, lambda: loss.pose_2d_mse_per_frame(hm, gt)),
            "fused_points": (device_time, lambda: loss.pose_2d_mse_per_frame_from_points(hm, pt, 1.0)),
            "per_frame": (host_time, lambda: [loss.pose_2d_mse_single_batch(hm[i], gt[i]).item() for i in range(b)]),
        }
        fused = loss.pose_2d_mse_per_frame(hm, gt)
        assert torch.equal(fused, loss.pose_2d_mse_per_frame_from_points(hm, pt, 1.0))
        looped = torch.tensor(ways["per_frame"][1](), dtype=torch.float32)  # (warm-up of every way, and the same numbers)
        assert (fused.cpu() - looped).abs().max().item() <= 1.2e-7 * looped.abs().max().item()
        times = {k: [] for k in ways}
        for _ in range(args.rounds):
            for k, (timer, fn) in ways.items():
                times[k].append(timer(fn, args.window))
        n_bytes = 2 * b * v * j * hh * wh * 4
        out = dict(shape=name, frames=b, views=v, joints=j, hh=hh, wh=wh, bytes_gt_form=n_bytes, rounds=args.rounds, window_s=args.window)
        for k in ways:
            t = float(np.median(times[k]))
            out[k + "_us_per_batch"] = round(t * 1e6, 2)
            out[k + "_spread_us"] = [round(min(times[k]) * 1e6, 2), round(max(times[k]) * 1e6, 2)]
            out[k + "_bytes_over_time_GBps"] = round((n_bytes // 2 if k == "fused_points" else n_bytes) / t * 1e-9, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

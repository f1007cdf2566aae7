"""Device time of the key-point undistortion at the benchmark's C2 post-stage shape (B=32 frames, V=4 views, J=19
joints: 2432 entries; 64x64 maps, stride 4, synth Gaussians with noise 0.02 around projected joints), next to the sub-pixel
refinement ``mval_refine_keypoints`` at the same shape: torch events around 100 back-to-back launches after 10 warm-up launches,
the two entries alternated over the repeats.  The window bounds a launch from above: it includes the host's enqueue where the host
is the slower side.  Every view carries the barrel lens of the design note's probe, on the hard decode (int64) and on the refined one
(float32).  One JSON line; [--repeats 5]."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_view_active_learning_amd import _lib, synth  # noqa: E402

BARREL = (-0.25, 0.15, 3e-4, 8e-4, -0.04)


def window(fn, calls=100, warmup=10):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def main():
    if not torch.cuda.is_available():
        raise SystemExit("undistort_bench: no HIP device -- a time measured anywhere else says nothing (NOT MEASURED)")
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    dev = torch.device("cuda:0")
    b, v, j, hh, wh, stride = 32, 4, 19, 64, 64, 4
    proj = np.stack([synth.ring_cameras(v, hh * stride, wh * stride, seed=s) for s in range(b)])
    hm = torch.from_numpy(synth.gaussian_heatmaps(7, proj, synth.joints_3d(7, b, j), hh, wh, stride, noise=0.02)).to(dev)
    f = 300.0 * (hh * stride / 256.0)  # synth.ring_cameras' intrinsics
    K = torch.tensor([[f, 0.0, wh * stride / 2.0], [0.0, f, hh * stride / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=dev).repeat(b, v, 1, 1).contiguous()
    dist = torch.tensor(BARREL, dtype=torch.float64, device=dev).repeat(b, v, 1).contiguous()
    valid = torch.ones(b, j, dtype=torch.uint8, device=dev)
    kp = _lib.argmax_decode(hm, valid, b, v, j, hh, wh, stride, wh)
    kp_f32, _ = _lib.refine_keypoints(hm, kp, valid, b, v, j, hh, wh, stride, "taylor")
    variants = {
        "refine_keypoints_taylor": lambda: _lib.refine_keypoints(hm, kp, valid, b, v, j, hh, wh, stride, "taylor"),
        "undistort_keypoints_i64": lambda: _lib.undistort_keypoints(kp, K, dist, valid, b, v, j),
        "undistort_keypoints_f32": lambda: _lib.undistort_keypoints(kp_f32, K, dist, valid, b, v, j),
    }
    status = variants["undistort_keypoints_f32"]()[1].cpu().numpy()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(window(fn))
    us = lambda t: {"median": round(float(np.median(t)) * 1e6, 2), "min": round(min(t) * 1e6, 2), "max": round(max(t) * 1e6, 2)}  # noqa: E731
    print(json.dumps({"shape": f"B={b} V={v} J={j}", "entries": b * v * j, "launches_per_window": 100, "warmup": 10, "repeats": repeats,
                      "iterations": {"min": int(status.min()), "max": int(status.max()), "mean": round(float(status.mean()), 2)},
                      "us_per_launch": {k: us(t) for k, t in times.items()},
                      "note": "back-to-back launches, no sync inside a window: host-enqueue bound where the host is slower than the device"}))


if __name__ == "__main__":
    main()

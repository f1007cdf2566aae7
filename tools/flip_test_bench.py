"""Cost of the flip test at the benchmark's C2 shape: HRNet-W32, B=32 frames x V=4 views of 256x256, J=19, 64x64
maps, synthetic weights and images (times only: synthetic weights say nothing about accuracy).

  step    one evaluation step -- ``evaluate_mkpe`` over a one-batch loader whose images are already on the device: the network (twice
          and the two launches of the flip test under "mirror_shift"), decode, triangulation, MKPE -- under EVAL.FLIP_TEST "none" and
          "mirror_shift", alternated; a host clock around ``--steps`` steps that end in a device synchronise, ``--repeats`` windows each.
  launch  ``mval_flip_merge_heatmaps`` (shift, keys) and ``mval_mirror_images`` alone at the step's shapes: device events around 100
          back-to-back launches after 10 warm-up launches.  The window bounds a launch from above (it includes the host's enqueue
          where the host is the slower side); GB/s = the bytes the launch must move over that time -- 3 x N*J*hh*wh*4 for the merge
          (two reads, one write; its keys add N*128*J*8), 2 x N*3*H*W*4 for the mirror.  The kernels' own times come from
          ``rocprofv3 --kernel-trace --stats -- python tools/flip_test_bench.py`` in a run of its own (flip_merge_kernel, mirror_images_kernel).

One JSON line; [--steps 10] [--repeats 5] [--frames 32]."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_view_active_learning_amd import _lib, synth  # noqa: E402


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


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
        raise SystemExit("flip_test_bench: no HIP device -- a time measured anywhere else says nothing (NOT MEASURED)")
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.pose_estimators import PoseHighResolutionNet
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils import flip_test

    steps, repeats, b = _arg("--steps", 10), _arg("--repeats", 5), _arg("--frames", 32)
    dev = torch.device("cuda:0")
    v, j, h, w, stride = 4, 19, 256, 256, 4
    hh, wh = h // stride, w // stride
    model = PoseHighResolutionNet(j)
    sd = synth.synthetic_state_dict(model._graph.param_shapes(), 0)
    model.load_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, strict=True)
    model = model.to(dev).eval()
    dp = dict(images=torch.from_numpy(synth.images(77, b, v, h, w)).to(dev), pose=torch.arange(b), frame_id=torch.arange(b),
              proj_matrices=torch.from_numpy(np.stack([synth.ring_cameras(v, h, w, seed=s) for s in range(b)])),
              joint_valid=torch.ones(b, j), **{"3d_keypoints": torch.from_numpy(np.concatenate([synth.joints_3d(3, b, j), np.ones((b, 1, j), np.float32)], axis=1))})
    strategies = {}
    for mode in ("none", "mirror_shift"):
        cfg = get_default_configs()
        cfg.EVAL.FLIP_TEST = mode
        strategies[mode] = ActiveLearningStrategy(cfg)

    def run(mode, k):
        for _ in range(k):
            strategies[mode].evaluate_mkpe([dp], model)
        torch.cuda.synchronize()

    step_s = {mode: [] for mode in strategies}
    for mode in strategies:  # warm-up: plans, graph capture, code objects
        run(mode, 3)
    for _ in range(repeats):
        for mode in strategies:
            t0 = time.perf_counter()
            run(mode, steps)
            step_s[mode].append((time.perf_counter() - t0) / steps)

    n = b * v
    rng = np.random.default_rng(5)
    hm, hmm = (torch.from_numpy(rng.standard_normal((n, j, hh, wh)).astype(np.float32)).to(dev) for _ in range(2))
    out, x = torch.empty_like(hm), dp["images"].reshape(n, 3, h, w)
    x_out = torch.empty_like(x)
    pairs = flip_test.pairs_on_device(flip_test.flip_pairs(get_default_configs().DATA), dev)
    launches = {
        "flip_merge_heatmaps_shift_keys": (lambda: _lib.flip_merge_heatmaps(hm, hmm, pairs, 1, out=out), 3 * hm.numel() * 4),
        "flip_merge_heatmaps_shift_nokeys": (lambda: _lib.flip_merge_heatmaps(hm, hmm, pairs, 1, keep_keys=False, out=out), 3 * hm.numel() * 4),
        "mirror_images": (lambda: _lib.mirror_images(x, out=x_out), 2 * x.numel() * 4),
    }
    launch_s = {k: [] for k in launches}
    for _ in range(repeats):
        for k, (fn, _bytes) in launches.items():
            launch_s[k].append(window(fn))
    stat = lambda t, scale: {"median": round(float(np.median(t)) * scale, 3), "min": round(min(t) * scale, 3), "max": round(max(t) * scale, 3)}  # noqa: E731
    print(json.dumps({
        "shape": f"HRNet-W32 B={b} V={v} J={j} {h}x{w} -> {hh}x{wh}", "steps_per_window": steps, "repeats": repeats,
        "ms_per_step": {mode: stat(t, 1e3) for mode, t in step_s.items()},
        "step_ratio_median": round(float(np.median(step_s["mirror_shift"]) / np.median(step_s["none"])), 3),
        "us_per_launch": {k: stat(t, 1e6) for k, t in launch_s.items()},
        "bytes_per_launch": {k: nbytes for k, (_fn, nbytes) in launches.items()},
        "gb_per_s_at_median": {k: round(launches[k][1] / float(np.median(t)) * 1e-9, 1) for k, t in launch_s.items()},
        "note": "launch windows: back-to-back launches, no sync inside a window -- host-enqueue bound where the host is slower than the device",
    }))


if __name__ == "__main__":
    main()

"""Device times of the confidence-weighted triangulation entry beside the entries it extends, B = 32 frames,
J = 19 joints, float32 key-points (exact projections + 0.5 px noise, one outlier view per joint):
  * V = 4 and V = 11: mval_triangulate_ransac_masked (the parent's launch, unchanged) against mval_triangulate_ransac_weighted with
    the winning set alone (weights NULL) and with weights;
  * V = 16: mval_triangulate_ransac_pairs_masked on 64 drawn pairs per problem against the same two forms of the new entry.
Every call is one triangulation launch plus the frame reduction.  Two figures per variant, the variants of a shape alternating
inside every repeat so that a drift of the clocks or a neighbour on the machine hits all alike:
  * us_per_call: a device event before and after each SINGLE call on an idle queue, synchronised; median [min, max] of the repeats.
    It holds the host's enqueue of the call (the output allocations, the ctypes call, two launches) as well as the kernels;
  * us_per_call_window: device events around windows of back-to-back calls, as the other tools here time; it bounds a call from
    above by the slower of host and device.
Neither is the kernels' own time: that comes from a kernel trace of this tool (`rocprofv3 --kernel-trace --stats -- python
tools/weighted_tri_bench.py --repeats 50`), in a run of its own, where the instantiations show as `ransac_*_kernel<MASK, EXT, KP>`.
One JSON line; [--repeats 200] [--warmup 20] [--windows 9] [--calls 200]."""
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_view_active_learning_amd import _lib, synth  # noqa: E402
from multi_view_active_learning_amd.utils.triangulation import draw_view_pairs  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn):  # one call between two device events -> seconds
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def window(fn, calls):  # device events around `calls` back-to-back calls -> seconds per call
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def shape_variants(v, dev, b=32, j=19, size=1024, eps=5.0):
    rng = np.random.default_rng(v)
    proj = np.stack([synth.ring_cameras(v, size, size, seed=s) for s in range(b)])
    x = synth.joints_3d(3, b, j).astype(np.float64)
    kp = np.stack([synth.project(proj[i], x[i].T) for i in range(b)]) + rng.standard_normal((b, v, j, 2)) * 0.5
    bad = rng.integers(0, v, (b, j))
    for bi in range(b):
        kp[bi, bad[bi], np.arange(j)] += 60.0
    kp = torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float32)).to(dev)
    proj = torch.from_numpy(proj).to(dev)
    valid = torch.ones(b, j, dtype=torch.uint8, device=dev)
    w = torch.from_numpy(rng.uniform(0.05, 1.0, (b, v, j)).astype(np.float32)).to(dev)
    ones = torch.ones_like(w)
    pairs = None
    if v > 11:
        pairs = torch.from_numpy(draw_view_pairs(np.ones((b, j)), v, 64, random.Random(v))).to(dev)
        old = lambda: _lib.triangulate_ransac_pairs(kp, proj, valid, pairs, b, v, j, eps)  # noqa: E731
    else:
        old = lambda: _lib.triangulate_ransac(kp, proj, valid, b, v, j, eps)  # noqa: E731
    new = lambda weights: _lib.triangulate_ransac_weighted(kp, proj, valid, b, v, j, eps, pairs=pairs, weights=weights, want_inlier_mask=True)  # noqa: E731
    name = "V%d" % v
    variants = {name + "/masked_entry": old, name + "/weighted_entry_set_only": lambda: new(None), name + "/weighted_entry": lambda: new(w)}
    # faster and different is not faster: the set alone and all-ones weights give the old entry's bits
    want = old()
    for got in (new(None), new(ones)):
        assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, c.view(torch.int64) if c.dtype == torch.float64 else c)
                   for a, c in zip(want, got[:5]))
    moved = (new(w)[0] - want[0]).norm(dim=-1)
    return variants, {"problems": b * j, "pairs": 64 if pairs is not None else v * (v - 1) // 2,
                      "mean_shift_mm_under_weights": round(float(moved.mean().item()), 4)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("weighted_tri_bench: no HIP device -- a time measured anywhere else says nothing (NOT MEASURED)")
    repeats, warmup, windows, calls = arg("--repeats", 200), arg("--warmup", 20), arg("--windows", 9), arg("--calls", 200)
    dev = torch.device("cuda:0")
    variants, shapes = {}, {}
    for v in (4, 11, 16):
        var, shapes["V%d" % v] = shape_variants(v, dev)
        variants.update(var)
    for fn in variants.values():  # warm-up: code objects, the allocator's blocks
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    in_window = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            in_window[k].append(window(fn, calls))
    us = lambda t: {"median": round(float(np.median(t)) * 1e6, 2), "min": round(min(t) * 1e6, 2), "max": round(max(t) * 1e6, 2)}  # noqa: E731
    print(json.dumps({"shapes": shapes, "repeats": repeats, "warmup": warmup, "us_per_call": {k: us(t) for k, t in times.items()},
                      "windows": windows, "calls_per_window": calls, "us_per_call_window": {k: us(t) for k, t in in_window.items()},
                      "note": "B=32 J=19; us_per_call: one call between two device events on an idle queue (host enqueue included); "
                              "us_per_call_window: back-to-back calls, host-enqueue bound where the host is slower than the device"}))


if __name__ == "__main__":
    main()

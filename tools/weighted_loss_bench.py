"""Device times of the weighted training loss at the C3 shape: 128 images x 19 joints x 64 x 64 maps, points form (the
ground truth rendered in both directions), every weight positive and every map valid, so that all variants move the same bytes:
  * weighted_top0 / weighted_top8: mval_weighted_mse_points_fwd then _bwd at topk = 0 and topk = 8 (the backward of topk = 8 skips the maps
    that were not selected and only writes zeros there);
  * masked: mval_masked_mse_points_fwd then _bwd, today's loss, in the same process;
  * the forwards and backwards of weighted_top0 and masked alone, to see where a difference sits.
Device events around windows of back-to-back calls after a warm-up; the variants alternate inside every repeat, so a drift of the clocks or
a neighbour on the machine hits all of them alike.  One JSON line; [--windows 9] [--calls 100] [--warmup 10]."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_view_active_learning_amd import _lib  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def window(fn, calls):  # device events around `calls` back-to-back calls -> seconds per call
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def main():
    if not torch.cuda.is_available():
        raise SystemExit("weighted_loss_bench: no HIP device -- a time measured anywhere else says nothing (NOT MEASURED)")
    windows, calls, warmup = arg("--windows", 9), arg("--calls", 100), arg("--warmup", 10)
    n, j, hh, wh = 128, 19, 64, 64
    lead = n * j
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    h = torch.from_numpy(rng.standard_normal(lead * hh * wh).astype(np.float32) * 0.5).to(dev)
    pt = torch.from_numpy(np.stack([rng.uniform(0, wh - 1, lead), rng.uniform(0, hh - 1, lead)], 1)).to(dev)
    w = torch.from_numpy(rng.uniform(0.5, 2.0, lead).astype(np.float32)).to(dev)
    valid = torch.ones(lead, dtype=torch.uint8, device=dev)
    go = torch.ones((), dtype=torch.float32, device=dev)
    denom = float(n * hh * wh)
    wsel = {k: _lib.weighted_mse_points_fwd(h, pt, 1.0, w, k, n, j, hh, wh)[2] for k in (0, 8)}

    def weighted_fwd(k):
        return _lib.weighted_mse_points_fwd(h, pt, 1.0, w, k, n, j, hh, wh)

    def weighted_bwd(k):
        return _lib.weighted_mse_points_bwd(h, pt, 1.0, wsel[k], go, n, j, hh, wh)

    def masked_fwd():
        return _lib.masked_mse_points_fwd(h, pt, 1.0, valid, lead, hh, wh, denom)

    def masked_bwd():
        return _lib.masked_mse_points_bwd(h, pt, 1.0, valid, go, lead, hh, wh, denom)

    variants = {
        "weighted_top0": lambda: (weighted_fwd(0), weighted_bwd(0)),
        "weighted_top8": lambda: (weighted_fwd(8), weighted_bwd(8)),
        "masked": lambda: (masked_fwd(), masked_bwd()),
        "weighted_top0_fwd": lambda: weighted_fwd(0),
        "masked_fwd": masked_fwd,
        "weighted_top0_bwd": lambda: weighted_bwd(0),
        "masked_bwd": masked_bwd,
    }
    # the variants compute the same thing where they should: all-ones weights give today's gradient bits and its loss within 1 ulp
    ones = torch.ones(lead, dtype=torch.float32, device=dev)
    a = _lib.weighted_mse_points_fwd(h, pt, 1.0, ones, 0, n, j, hh, wh)
    assert abs(int(a[0].view(torch.int32).item()) - int(masked_fwd().view(torch.int32).item())) <= 1
    assert torch.equal(_lib.weighted_mse_points_bwd(h, pt, 1.0, a[2], go, n, j, hh, wh).view(torch.int32), masked_bwd().view(torch.int32))
    for fn in variants.values():  # warm-up: code objects, the allocator's blocks
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for k, fn in variants.items():
            times[k].append(window(fn, calls))
    us = lambda t: {"median": round(float(np.median(t)) * 1e6, 2), "min": round(min(t) * 1e6, 2), "max": round(max(t) * 1e6, 2)}  # noqa: E731
    med = {k: float(np.median(t)) for k, t in times.items()}
    print(json.dumps({"shape": f"{n} images x {j} joints x {hh}x{wh}, points form", "maps": lead, "windows": windows, "calls_per_window": calls,
                      "us_per_call": {k: us(t) for k, t in times.items()},
                      "weighted_top0_over_masked": round(med["weighted_top0"] / med["masked"], 3),
                      "bytes": {"forward_read": lead * hh * wh * 4, "backward_read": lead * hh * wh * 4, "backward_written": lead * hh * wh * 4},
                      "note": "calls are back to back with no sync inside a window; each allocates its outputs from torch's caching allocator"}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/small_graph_inputs.npz: the input batch of every case of tests/test_train_small_graphs.py.

The small-graph tests compare against float64 autograd far below the level at which a flipped ReLU mask shows, so their inputs must keep every
ReLU's pre-activation away from zero: min |pre-activation| (float64) > 64 x the largest float32 - float64 difference of that tensor (~3e-6
on these graphs).  With 1e5 pre-activations per case no seed of a Gaussian input does that (expected: one seed in 1e5), so the input is
MADE to: start from the seeded Gaussian batch and, while any pre-activation lies within TAU of zero, move x along that pre-activation's own
gradient (float64, CPU) until it sits 1.5 x TAU away; the other pre-activations move an order of magnitude less, so a few rounds clear all
of them.  Only the reference model is used (tests/tiny_graphs.py graph_forward); the parameters stay as the case's seed gives them.

    python tests/golden/make_small_graph_inputs.py [case ...]

Only the cases named are made again (all of them without arguments); every other array of the file is written back as it was read, which the
script asserts at its end.  The `linear` cases of the test have no ReLU and draw their inputs when they run: nothing of them is stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import tiny_graphs as tg  # noqa: E402
from test_train_small_graphs import CASES, INPUTS  # noqa: E402

TAU = 1.2e-3  # ~400 x the float32 - float64 differences: the margin holds on hosts whose float32 convs sum in another order
ROUNDS, PER_ROUND = 60, 256


def widen(case):
    m = tg.TinyNet(tg.BUILDERS[case["graph"]], case["args"], case["seed"])
    sd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in m.state_dict().items()}
    x = tg.seeded_input(case).double()
    for rnd in range(ROUNDS):
        x.requires_grad_(True)
        fresh = {k: v.clone() for k, v in sd.items()}  # (the running statistics are not part of the question)
        _, pre = tg.graph_forward(m._graph, fresh, x, torch.float64)
        flat = torch.cat([p.reshape(-1) for p in pre.values()])
        idx = torch.nonzero(flat.abs() < TAU).reshape(-1)
        print(f"  round {rnd}: {idx.numel()} of {flat.numel()} pre-activations within {TAU:g} of zero; min {float(flat.abs().min()):.2e}", flush=True)
        if idx.numel() == 0:
            return x.detach().float()
        idx = idx[torch.argsort(flat[idx].abs())][:PER_ROUND]
        step = torch.zeros_like(x)
        for j in idx.tolist():
            (gr,) = torch.autograd.grad(flat[j], x, retain_graph=True)
            v = float(flat[j])
            target = 1.5 * TAU * (1.0 if v >= 0 else -1.0)
            step += (target - v) * gr / float((gr * gr).sum())
        x = (x + step).detach()
    raise RuntimeError("no margin after %d rounds" % ROUNDS)


def main():
    todo = sys.argv[1:] or list(CASES)
    have = dict(np.load(INPUTS)) if os.path.exists(INPUTS) else {}
    kept = {k: v.copy() for k, v in have.items() if k not in todo}
    for cid in todo:
        print(cid, flush=True)
        xf = widen(CASES[cid])
        have[cid] = xf.numpy()
        np.savez_compressed(INPUTS, **have)
    # the arrays of the cases that were not asked for come out of the rewritten file as they went in, bit for bit
    back = np.load(INPUTS)
    assert set(back.files) == set(have) and all(back[k].dtype == v.dtype and np.array_equal(back[k], v) for k, v in kept.items())
    print(f"{len(todo)} written, {len(kept)} unchanged")


if __name__ == "__main__":
    main()

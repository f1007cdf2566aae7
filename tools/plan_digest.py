#!/usr/bin/env python3
"""Digest of every decision a plan builder makes, for a fixed set of models, sizes and switch settings: one line per case with a few
readable aggregates and a SHA-256 over the whole plan.  Two trees build the same plans exactly when their outputs are equal (`diff`);
when a change is MEANT to move a plan, the aggregates show which decision moved.

    plan_digest.py [train|infer|all] > digest.txt        (timings go to stderr)

Needs no GPU: the builders call only host-side predicates of libmval_hip.so and allocate with torch.empty, so the plans are built on
torch.device("cpu").  One predicate (mval_conv_p2_inz_supported) dry-runs a launch and reads the compute-unit count (256 without a
device), so a digest is comparable only with one taken on the same kind of machine."""
import ctypes as C
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multi_view_active_learning_amd import engine, engine_train
from multi_view_active_learning_amd.pose_estimators import PoseHighResolutionNet, PoseResNet, hrnet_w48

# filled per step, not by the plan
PTR = {"gamma", "beta", "running_mean", "running_var", "mean", "invstd", "dweight", "dgamma", "dbeta"}
TRAIN_ATTRS = ("arena_floats", "param_floats", "n_lanes", "segments", "zero_slots", "p2_rows", "jobs", "stat_off", "gz_lane", "wsf_lane",
               "ws_lane", "sums_lane", "grad_floats", "ones_off", "zeros_off", "gz_amax_off", "out_hw", "maxc")
INFER_ATTRS = ("param_jobs", "arena_floats", "param_floats", "amax_base", "_p2_rows", "p2")
SIZES = (("hrnet_w32", (128, 256, 256)), ("hrnet_w32", (32, 256, 256)), ("hrnet_w32", (2, 64, 64)), ("hrnet_w48", (8, 384, 288)),
         ("resnet50", (32, 256, 192)), ("resnet50", (8, 256, 192)))
# inference plans only: a non-square size whose 1/32-resolution map is 6 columns wide, a one-image batch, and PoseResNet at 64 images
# (from 32 images on its transposed convs are P2-eligible: the stem + max-pool + MVAL_OP_TO_P2 form)
INFER_SIZES = (("hrnet_w32", (8, 256, 192)), ("hrnet_w32", (1, 256, 256)), ("resnet50", (64, 256, 192)))
TRAIN_OTHER = {"MVAL_CONV": ("h2", "bf3", "fp32"), "MVAL_FORCE_DIRECT": ("1",), "MVAL_TRAIN_LANES": ("0", "1", "2")}  # every other switch: ("0",)
INFER_OTHER = {"MVAL_CONV": ("h2", "bf3", "fp32"), "MVAL_FORCE_DIRECT": ("1",), "MVAL_STREAMS": ("1",), "MVAL_P2": ("0", "force")}


def model(arch):
    return {"hrnet_w32": lambda: PoseHighResolutionNet(19), "hrnet_w48": lambda: PoseHighResolutionNet(19, hrnet_cfg=hrnet_w48()),
            "resnet50": lambda: PoseResNet(19, 50)}[arch]()


def variants(table, other):
    """The default switches, then every switch moved alone to each of its other values."""
    yield {}
    for key in table:
        for v in other.get(key, ("0",)):
            yield {key: v}


def train_digest(plan):
    h = hashlib.sha256()
    for t in plan.ops:
        for name, _ in engine_train.MvalTrainOp._fields_:
            if name not in PTR:
                v = getattr(t, name)
                h.update(name.encode() + (bytes(v) if name == "op" else repr(int(v)).encode()))
    for a in TRAIN_ATTRS:
        h.update(a.encode() + repr(getattr(plan, a)).encode())
    h.update(repr([sorted(s.items()) for s in plan.grad_slots]).encode())
    h.update(repr([tuple(p.shape) for p in plan.param_list]).encode())
    h.update(repr([[tuple(p.shape) for p in ps] for ps in plan.seg_params]).encode())
    bits = ",".join(str(sum(int(t.p2_flags >> b & 1) for t in plan.ops)) for b in range(14))
    return (f"lanes={plan.n_lanes} uses_p2={int(plan.uses_p2)} arena={plan.arena_floats} params={plan.param_floats} grads={plan.grad_floats} "
            f"fwd_p2={sum(int(t.fwd_p2 != 0) for t in plan.ops)} flag_bits={bits} bn_in_conv={plan.n_bn_in_conv} "
            f"bn_bwd_in_dgrad={plan.n_bn_bwd_in_dgrad} segments={len(plan.segments)} sha256={h.hexdigest()}")


def infer_digest(plan):
    h = hashlib.sha256()
    for ops in (plan.graph_ops, plan.ops):
        h.update(repr(len(ops)).encode())
        for m in ops:
            h.update(bytes(m))
    for a in INFER_ATTRS:
        h.update(a.encode() + repr(getattr(plan, a)).encode())
    return (f"p2={int(bool(plan.p2))} graph_ops={len(plan.graph_ops)} launches={len(plan.ops)} arena={plan.arena_floats} "
            f"params={plan.param_floats} sha256={h.hexdigest()}")


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    cpu = torch.device("cpu")
    models = {}
    cases, t_all = 0, time.time()
    for arch, (n, hh, ww) in SIZES + INFER_SIZES:
        m = models.get(arch) or models.setdefault(arch, model(arch))
        todo = []
        if what in ("train", "all") and (arch, (n, hh, ww)) in SIZES:
            base = engine._switches(engine_train._SWITCHES)
            todo += [("train", dict(base, **v), v, p2) for v in variants(base, TRAIN_OTHER) for p2 in (True, False)]
        if what in ("infer", "all"):
            base = engine._switches(engine._SWITCHES)
            todo += [("infer", dict(base, **v), v, None) for v in variants(base, INFER_OTHER)]
        for kind, sw, v, p2 in todo:
            name = f"{kind} {arch} {n}x{hh}x{ww} {','.join(f'{k}={x}' for k, x in v.items()) or 'default'}" + ("" if p2 is None else f" p2={int(p2)}")
            t0 = time.time()
            try:
                if kind == "train":
                    line = train_digest(engine_train.TrainPlan(m.train(), n, hh, ww, cpu, p2=p2, sw=sw))
                else:
                    line = infer_digest(engine.InferencePlan(m.eval(), n, hh, ww, cpu, sw=sw))
            except Exception as e:  # noqa: BLE001  (a case whose builder raises is part of the record)
                line = f"{type(e).__name__}: {e}"
            print(f"{name}: {line}")
            print(f"{name}: {time.time() - t0:.3f} s", file=sys.stderr)
            cases += 1
    print(f"{cases} cases in {time.time() - t_all:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()

"""One training batch through the device RandAugment (csrc/augment.hip) against the same ops on the host with Pillow, one CPU thread.

    python tools/augment_bench.py [--views 128] [--size 256] [--num-aug 2] [--magnitude 20] [--reps 20] [--reference-augmentation FILE] [--cpu-only]

Device: RandAugment.apply on (views, size, size, 3) uint8, device events around `reps` calls after a warm-up, a fresh plan per call (drawn before
the clock starts); also the same with 1/4 of the views, to show that the launches per batch do not grow with the number of views.
Host: the same plans view by view on Pillow images -- through the reference's own RandAugment when --reference-augmentation names its
dataset/augmentation.py (that one also rotates the heat-maps it then throws away: 19 maps of size / 4), else through the Pillow calls its
ops make.  Prints one JSON line.

    python tools/augment_bench.py --targets [--views 128] [--maps 19] [--map-size 64] [--reps 20]

The target side instead (rotate_targets="maps"): RandAugment.rotate_maps in place on (views, maps, map-size, map-size) float32 with every view
rotating once, beside gt_heatmaps at the same shape as the yardstick for a pass that writes the same bytes; the two alternate, each call
between device events of its own."""
import argparse
import importlib.util
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from multi_view_active_learning_amd.utils import augmentation as aug  # noqa: E402

STATS = (1 << aug.AUG_AUTOCONTRAST) | (1 << aug.AUG_EQUALIZE) | (1 << aug.AUG_CONTRAST)
TABLE = STATS | (1 << aug.AUG_INVERT) | (1 << aug.AUG_POSTERIZE) | (1 << aug.AUG_SOLARIZE) | (1 << aug.AUG_BRIGHTNESS)
SPATIAL = (1 << aug.AUG_SHARPNESS) | (1 << aug.AUG_ROTATE)


def launches(masks):
    """Kernel launches (and the one memset) mval_augment_views issues for these per-step kind masks."""
    return sum(2 * bool(m & STATS) + 2 * bool(m & TABLE) + bool(m & (1 << aug.AUG_COLOR)) + 2 * bool(m & SPATIAL) for m in masks)


def images(n, size, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    base = np.stack([127 + 120 * np.sin(xx / 9.0), 127 + 120 * np.cos(yy / 7.0), (3 * xx + 5 * yy) % 256], -1)
    return np.clip(base[None] + rng.normal(0, 12, (n,) + base.shape), 0, 255).astype(np.uint8)


def pillow_op(im, name, val):
    from PIL import Image, ImageEnhance, ImageOps

    if name == "Rotate":
        return im.rotate(val, resample=Image.BICUBIC)
    if name in ("AutoContrast", "Invert", "Equalize"):
        return getattr(ImageOps, name.lower())(im)
    if name == "Solarize":
        return ImageOps.solarize(im, val)
    if name == "Posterize":
        return ImageOps.posterize(im, max(1, int(val)))
    return getattr(ImageEnhance, name)(im).enhance(val)


def host_time(args, imgs):
    import torch
    from PIL import Image

    torch.set_num_threads(1)
    pil = [Image.fromarray(i) for i in imgs]
    random.seed(1)
    np.random.seed(1)
    if args.reference_augmentation:
        spec = importlib.util.spec_from_file_location("_ref_augmentation", args.reference_augmentation)
        mod = importlib.util.module_from_spec(spec)
        sys.dont_write_bytecode = True
        spec.loader.exec_module(mod)
        ra = mod.RandAugment(args.num_aug, args.magnitude, True, True, False)
        hm = torch.zeros(19, args.size // 4, args.size // 4)
        t0 = time.perf_counter()
        for im in pil:
            np.asarray(ra(im, hm)[0])
        return time.perf_counter() - t0, "reference RandAugment"
    plan = aug.RandAugment(args.num_aug, args.magnitude, True, True, False).draw(len(pil))
    t0 = time.perf_counter()
    for im, ops in zip(pil, plan):
        for name, val in ops:
            im = pillow_op(im, name, val)
        np.asarray(im)
    return time.perf_counter() - t0, "Pillow calls"


def device_time(args, imgs, n_views):
    import torch

    x = torch.from_numpy(imgs[:n_views]).cuda()
    ra = aug.RandAugment(args.num_aug, args.magnitude, True, True, False)
    random.seed(1)
    np.random.seed(1)
    plans = [ra.draw(n_views) for _ in range(args.reps + 3)]
    n_launch = [launches(aug.plan_descriptors(p, args.size, args.size)[1]) for p in plans[3:]]
    for p in plans[:3]:
        ra.apply(x, p)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for p in plans[3:]:
        ra.apply(x, p)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps, sum(n_launch) / len(n_launch), max(n_launch)


def targets_time(args):
    import torch

    from multi_view_active_learning_amd.utils import preprocess

    v, j, n = args.views, args.maps, args.map_size
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(rng.uniform(0, n - 1, (v, j, 2))).cuda()
    plans = [[[("Rotate", float(a))] for a in rng.uniform(1.0, 30.0, v) * rng.choice([-1.0, 1.0], v)] for _ in range(args.reps + 3)]
    hm = preprocess.gt_heatmaps(pts, 1.0, n, n)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in plans]
    for p, (e0, e1, e2) in zip(plans, ev):
        e0.record()
        aug.RandAugment.rotate_maps(hm, p, inplace=True)
        e1.record()
        hm = preprocess.gt_heatmaps(pts, 1.0, n, n)
        e2.record()
    torch.cuda.synchronize()
    rot = sorted(e0.elapsed_time(e1) for e0, e1, _ in ev[3:])
    gt = sorted(e1.elapsed_time(e2) for _, e1, e2 in ev[3:])
    return rot[len(rot) // 2], gt[len(gt) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", action="store_true")
    ap.add_argument("--maps", type=int, default=19)
    ap.add_argument("--map-size", type=int, default=64)
    ap.add_argument("--views", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--num-aug", type=int, default=2)
    ap.add_argument("--magnitude", type=float, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reference-augmentation", default=None)
    ap.add_argument("--cpu-only", action="store_true")
    args = ap.parse_args()
    if args.targets:
        rot, gt = targets_time(args)
        print(json.dumps(dict(views=args.views, maps=args.maps, map_size=args.map_size, reps=args.reps, rotate_maps_ms=round(rot, 4),
                              gt_heatmaps_ms=round(gt, 4), ratio=round(rot / gt, 2))))
        return
    imgs = images(args.views, args.size)
    res = dict(views=args.views, size=args.size, num_aug=args.num_aug, magnitude=args.magnitude)
    if not args.cpu_only:
        ms, mean_l, max_l = device_time(args, imgs, args.views)
        ms4, mean_l4, max_l4 = device_time(args, imgs, max(1, args.views // 4))
        res.update(device_ms_per_batch=round(ms, 4), device_launches_mean=mean_l, device_launches_max=max_l,
                   quarter_batch_ms=round(ms4, 4), quarter_batch_launches_mean=mean_l4, quarter_batch_launches_max=max_l4)
    s, how = host_time(args, imgs)
    res.update(host_ms_per_batch=round(s * 1e3, 2), host_path=how)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

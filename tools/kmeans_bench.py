#!/usr/bin/env python3
"""SAL pose-cluster KMeans fit timing (utils/kmeans.py, csrc/kmeans.hip): 50 000 rows x D = 57 (Panoptic, J = 19)
and D = 126 (InterHand, J = 42), K = 10, structured (pose modes plus noise) and unstructured (Gaussian) rows.
Device time is the whole KMeans(10, random_state=0).fit from host array to numpy attributes (upload included),
median of the repetitions; sklearn's CPU time on the same host is printed when sklearn imports.
GPU box: python tools/kmeans_bench.py [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multi_view_active_learning_amd.utils.kmeans import KMeans


def data(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "structured":
        modes = rng.normal(0, 300, (10, d))
        return modes[rng.integers(0, 10, n)] + rng.normal(0, 40, (n, d))
    return rng.normal(0, 100, (n, d))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=50000)
    args = ap.parse_args()
    try:
        from sklearn.cluster import KMeans as SkKMeans
    except ImportError:
        SkKMeans = None
    for d in (57, 126):
        for kind in ("structured", "unstructured"):
            x = data(kind, args.n, d, d)
            KMeans(10, random_state=0).fit(x)  # warm-up (library load, allocator)
            t, km = timed(lambda: KMeans(10, random_state=0).fit(x), args.reps)
            out = dict(n=args.n, D=d, K=10, kind=kind, n_iter=km.n_iter_, device_fit_ms=round(t * 1e3, 3),
                       device_ms_per_iter=round(t * 1e3 / km.n_iter_, 4), inertia=km.inertia_)
            if SkKMeans is not None:
                ts = []
                for _ in range(max(1, min(3, args.reps))):
                    t0 = time.perf_counter()
                    sk = SkKMeans(10, random_state=0).fit(x)
                    ts.append(time.perf_counter() - t0)
                out.update(sklearn_cpu_ms=round(float(np.median(ts)) * 1e3, 3), sklearn_n_iter=int(sk.n_iter_),
                           sklearn_inertia=float(sk.inertia_), cpu_threads=torch.get_num_threads())
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

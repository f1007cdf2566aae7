"""Generate the many-view triangulation goldens by running the REAL reference (build container only):

    python tests/golden/make_many_view_golden.py            # check the committed case seeds, write the fixtures
    python tests/golden/make_many_view_golden.py --search   # print, per case, the first seed >= the committed one that passes

  triangulation_many_views.npz  per case of many_view_cases.many_view_cases(): the ``random.seed`` value, the pair tables
                                the reference drew (B, J, P, 2; zero rows for invalid joints; none where all pairs fit),
                                a digest of ``random.getstate()`` after the last frame (and after each frame), the
                                reference's keypoints_2d / keypoints_3d / metric / inlier_count (``triangulation``) and
                                per-joint mean error / inlier count (``_triangulate_ransac``)
  sal_dict_many_views.json      ``_compute_sal_dict`` at V = 12, strategy TRIANGULATION, like sal_dict.json

The draws are CAPTURED from the reference: its ``random.shuffle`` call (utils/triangulation.py:281) goes through a
recording stand-in for the ``random`` name of that module, which forwards to python's global generator.

Every case must meet three conditions (the search moves the case seed on until they hold):
  (a) vote margin: min |err - eps| over the drawn pairs and all views of every valid problem >= 1e-6 px, so that the strict
      ``err < eps`` vote is decidable between two float64 implementations -- no problem is left out of any comparison;
  (b) pair dependence (heavy-outlier cases): under ``random.seed(rseed + 1)`` at least a quarter of the valid problems give
      a different 3-D point;
  (c) conditioning: the final DLT system ``A`` of every problem is no worse conditioned than the worst final DLT of the
      existing golden case ``v11_outliers`` (triangulation_edges.npz), measured as sigma_1 / (sigma_3 - sigma_4) of the
      reference's ``A``: the null vector's sensitivity to a perturbation of A relative to its norm.  This is what
      makes the tolerances of the existing golden tests apply here.
      The heavy-outlier cases CANNOT meet (c) by this measure: their final DLT runs over the three views that see the
      joint (plus at most two accidental ones) where v11_outliers has eight, and a thousand case seeds of v12_sampled
      all gave 1.36e3 .. 9.7e3 against the bound 1.06e3.  (b) and (c) conflict: pair dependence needs inlier sets that
      tie in size, which needs few views that see the joint.  The heavy-outlier cases and the sal_dict input are
      therefore admitted on (a) and (b) alone -- the asserts below say so -- and their ratio is printed and stored
      (``<case>/sigma_ratio``) so that a tolerance missed on them can be read against it.  The test tolerances stay.
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import geometry, ref_harness  # noqa: E402

import cases  # noqa: E402
import many_view_cases as mv  # noqa: E402

MARGIN = 1e-6


class _RecordingRandom:
    """Stands in for the name ``random`` inside the reference's utils/triangulation.py: forwards to python's global
    generator and keeps every shuffled list."""

    def __init__(self):
        self.shuffled = []

    def shuffle(self, x):
        random.shuffle(x)
        self.shuffled.append(list(x))

    def __getattr__(self, k):
        return getattr(random, k)


class Spy:
    """Records, per ``_triangulate_ransac`` call of the reference: its result, the pairs it drew (None without a draw)
    and the arguments of its last ``_triangulate_dlt`` call (the final DLT)."""

    def __init__(self, ns):
        self.tri = ns.triangulation
        self.calls = []

    def __enter__(self):
        t = self.tri
        self._saved = (t.random, t._triangulate_ransac, t._triangulate_dlt)
        rec = _RecordingRandom()
        ransac, dlt = t._triangulate_ransac, t._triangulate_dlt
        last = {}

        def dlt_spy(pm, pts):
            last["dlt"] = (np.array(pm), np.array(pts))
            return dlt(pm, pts)

        def ransac_spy(pm, pts, n_iters, eps, direct):
            n0 = len(rec.shuffled)
            x, e, n = ransac(pm, pts, n_iters, eps, direct)
            drawn = rec.shuffled[n0][:n_iters] if len(rec.shuffled) > n0 else None
            self.calls.append(dict(x=np.array(x), err=float(e), n=int(n), pairs=drawn, dlt=last["dlt"],
                                   pm=np.array(pm), pts=np.array(pts), eps=eps))
            return x, e, n

        t.random, t._triangulate_ransac, t._triangulate_dlt = rec, ransac_spy, dlt_spy
        return self

    def __exit__(self, *a):
        self.tri.random, self.tri._triangulate_ransac, self.tri._triangulate_dlt = self._saved


def sigma_ratio(pm, pts):
    a = np.zeros((2 * len(pm), 4))
    for j in range(len(pm)):
        a[2 * j] = pts[j][0] * pm[j][2, :] - pm[j][0, :]
        a[2 * j + 1] = pts[j][1] * pm[j][2, :] - pm[j][1, :]
    s = np.linalg.svd(a, compute_uv=False)
    return s[0] / (s[2] - s[3])


def vote_margin(call, v):
    pairs = call["pairs"] if call["pairs"] is not None else [(a, c) for a in range(v) for c in range(a + 1, v)]
    m = np.inf
    for pr in pairs:
        pr = list(pr)
        x = geometry.triangulate_dlt(call["pm"][pr], call["pts"][pr])
        m = min(m, float(np.min(np.abs(geometry.reprojection_errors(x, call["pts"], call["pm"]) - call["eps"]))))
    return m


def run_case(ns, c, rseed):
    """The reference's ``triangulation`` frame after frame from ``random.seed(rseed)`` -> (results, spy calls, digests)."""
    hm, proj, valid = mv.build(c)
    random.seed(rseed)
    res, digests = [], []
    with Spy(ns) as spy:
        for b in range(hm.shape[0]):
            res.append(ns.triangulation.triangulation(torch.from_numpy(hm[b]), torch.from_numpy(proj[b]), c["stride"],
                                                      torch.from_numpy(valid[b]), n_iters=c["n_iters"],
                                                      reprojection_error_epsilon=mv.EPS))
            digests.append(mv.state_digest(random.getstate()))
    return res, spy.calls, digests, valid


def worst_existing_ratio(ns):
    c = cases.triangulation_edge_cases()["v11_outliers"]
    hm, proj, valid = cases.build_triangulation_case(c)
    with Spy(ns) as spy:
        for b in range(hm.shape[0]):
            ns.triangulation.triangulation(torch.from_numpy(hm[b]), torch.from_numpy(proj[b]), c["stride"], torch.from_numpy(valid[b]))
    return max(sigma_ratio(*k["dlt"]) for k in spy.calls)


def check(ns, c, worst, say=print):
    """-> (ok, record or None): conditions (a)-(c) for case ``c``."""
    res, calls, digests, valid = run_case(ns, c, c["rseed"])
    margin = min(vote_margin(k, c["v"]) for k in calls)
    ratio = max(sigma_ratio(*k["dlt"]) for k in calls)
    changed = None
    if c["heavy"]:
        _, calls2, _, _ = run_case(ns, c, c["rseed"] + 1)
        changed = sum(not np.array_equal(k["x"], k2["x"]) for k, k2 in zip(calls, calls2))
    ok = margin >= MARGIN and (c["heavy"] or ratio <= worst) and (changed is None or 4 * changed >= len(calls))
    say(f"  seed {c['seed']}: margin {margin:.3e}, sigma ratio {ratio:.4e} (bound {worst:.4e}), "
        f"changed under rseed+1: {changed} of {len(calls)}, inliers {sorted(set(k['n'] for k in calls))} -> {'ok' if ok else 'NO'}")
    return ok, (res, calls, digests, valid, ratio)


def pair_table(c, calls, valid):
    b, j = valid.shape
    tab = np.zeros((b, j, mv.n_pairs(c), 2), np.uint8)
    it = iter(calls)
    for bi in range(b):
        for ji in range(j):
            if valid[bi, ji]:
                tab[bi, ji] = np.array(next(it)["pairs"], np.uint8)
    return tab


def per_joint(calls, valid, key, dtype):
    out = np.zeros(valid.shape, dtype)
    it = iter(calls)
    for bi, ji in zip(*np.nonzero(valid)):
        out[bi, ji] = next(it)[key]
    return out


def gen_sal(ns, worst):
    c = mv.sal_many_view_case()
    loader, heatmaps = cases.build_sal_loader(c)
    it = iter(heatmaps)
    st = ref_harness.make_strategy(c["strategy"], **{"POSE_ESTIMATOR.STRIDE": c["stride"]})
    tl = [{k: torch.from_numpy(v) for k, v in dp.items()} for dp in loader]

    def run(rseed):
        nonlocal it
        it = iter(heatmaps)
        random.seed(rseed)
        with Spy(ns) as spy:
            sal = st._compute_sal_dict(tl, lambda images: torch.from_numpy(next(it)))
        return sal, spy.calls, mv.state_digest(random.getstate())

    sal, calls, digest = run(c["rseed"])
    _, calls2, _ = run(c["rseed"] + 1)
    margin = min(vote_margin(k, c["v"]) for k in calls)
    ratio = max(sigma_ratio(*k["dlt"]) for k in calls)
    changed = sum(not np.array_equal(k["x"], k2["x"]) for k, k2 in zip(calls, calls2))
    print(f"sal_dict V=12: margin {margin:.3e}, sigma ratio {ratio:.4e} (bound {worst:.4e}), changed {changed} of {len(calls)}")
    assert margin >= MARGIN and 4 * changed >= len(calls), "sal_dict V=12: (a) vote margin or (b) pair dependence not met"
    # (c) cannot hold on a heavy-outlier input (final DLT over the three views that see the joint: module docstring);
    # should it ever hold, enforce it
    assert ratio > worst, f"sal_dict V=12 meets (c) after all ({ratio:.4e} <= {worst:.4e}): enforce it"
    import math
    from heapq import nlargest

    entry = {k: dict(d) for k, d in sal.items()}
    alm = {g: m for g, m in sal["al_metric"].items() if not math.isnan(m)}
    entry["nlargest"] = nlargest(c["select"], alm, key=alm.get)
    entry["state_digest"] = digest
    entry["sigma_ratio"] = float(ratio)
    with open(os.path.join(HERE, "sal_dict_many_views.json"), "w") as f:
        json.dump(entry, f)


def main():
    ns = ref_harness.load()
    worst = worst_existing_ratio(ns)
    print(f"worst final-DLT sigma ratio of v11_outliers: {worst:.4e}")
    search = "--search" in sys.argv
    out = {}
    for name, c in mv.many_view_cases().items():
        print(name)
        if search:
            c = dict(c)
            while not check(ns, c, worst)[0]:
                c["seed"] += 1
            print(f"  -> {name}: seed={c['seed']}")
            continue
        ok, (res, calls, digests, valid, ratio) = check(ns, c, worst)
        assert ok, (f"{name}: the committed seed does not meet (a) margin >= {MARGIN}, (b) a quarter of the problems pair-dependent "
                    f"(heavy-outlier cases) and (c) sigma ratio <= {worst:.4e} (all other cases: a final DLT over the three views "
                    "that see the joint cannot meet (c), see the module docstring); run with --search")
        if c["heavy"]:
            assert ratio > worst, f"{name}: meets (c) after all ({ratio:.4e} <= {worst:.4e}): enforce it for this case"
        out[name + "/rseed"] = np.int64(c["rseed"])
        out[name + "/sigma_ratio"] = np.float64(ratio)
        if mv.is_sampled(c):
            out[name + "/pairs"] = pair_table(c, calls, valid)
        else:
            assert all(k["pairs"] is None for k in calls)
        out[name + "/state_digest"] = digests[-1]
        out[name + "/frame_digests"] = np.array(digests)
        out[name + "/keypoints_2d"] = np.stack([r["keypoints_2d"] for r in res])
        out[name + "/keypoints_3d"] = np.stack([r["keypoints_3d"] for r in res])
        out[name + "/metric"] = np.asarray([r["metric"] for r in res], np.float64)
        out[name + "/inlier_count"] = np.asarray([r["inlier_count"] for r in res], np.int64)
        out[name + "/joint_error"] = per_joint(calls, valid, "err", np.float64)
        out[name + "/joint_inliers"] = per_joint(calls, valid, "n", np.int64)
    if search:
        return
    versions = json.dumps(dict(numpy=np.__version__, torch=torch.__version__, python=sys.version.split()[0]))
    np.savez_compressed(os.path.join(HERE, "triangulation_many_views.npz"), versions=versions, **out)
    gen_sal(ns, worst)


if __name__ == "__main__":
    main()

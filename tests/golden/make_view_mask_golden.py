"""Generate the missing-view goldens by running the REAL reference (build container only):

    python tests/golden/make_view_mask_golden.py            # check the committed case seeds, write the fixtures
    python tests/golden/make_view_mask_golden.py --search   # print, per case, the first seed >= the committed one that passes

  view_mask.npz            per case of view_mask_cases.view_mask_cases(): after ``random.seed(rseed)`` once per case, the
                           reference's ``triangulation`` frame after frame on ``heatmaps[b][present]``, ``proj[b][present]``
                           -- keypoints_2d scattered back to (B, V, J, 2) with the rows of absent views zero, keypoints_3d,
                           metric, inlier_count, per-joint mean error / inlier count (``_triangulate_ransac``), the pair
                           table in ORIGINAL view indices laid out as utils.triangulation.draw_view_pairs lays it out
                           (drawn rows as the reference drew them; padding 255), a digest of ``random.getstate()`` after
                           every frame, and ``_compute_hp`` (AVG, STD) on the sliced heat-maps.  A frame the reference
                           refuses is recorded by the exception it raised: AssertionError -> inlier_count -2,
                           ValueError (np.min([])) -> -1; its other outputs are zero / NaN.
                           ONE entry is not a reference output: a frame with NO present view (``degenerate``, frame 1) is not
                           handed to the reference, whose key-point decode fails on an empty tensor (IndexError) before either
                           error is reached.  Its -2 (with a valid joint; -1 without) is this project's convention, written
                           by this generator: the frame is counted as the frames with one present view are.
  sal_dict_view_mask.json  ``_compute_sal_dict`` (strategy TRIANGULATION) over one sliced frame per batch, like
                           sal_dict_many_views.json

The draws are captured from the reference with the recording stand-in of make_many_view_golden.py (``Spy``).

Every case must meet three conditions (the search moves the case seed on until they hold):
  (a) vote margin: min |err - eps| over the pairs walked and all present views of every valid problem >= 1e-6 px, so that
      the strict ``err < eps`` vote is decidable between two float64 implementations -- no problem is left out;
  (b) sensitive cases: in every frame with an absent view, the reference run on ALL views of the frame differs from the
      sliced run in joint_inliers for at least one joint -- an implementation that ignores the mask cannot pass;
  (c) sampled cases: under ``random.seed(rseed + 1)`` at least a quarter of the valid problems of the frames that draw
      give a different 3-D point -- the result depends on the draw.
"""
from __future__ import annotations

import itertools
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

from oracle import ref_harness  # noqa: E402

import cases  # noqa: E402
import make_many_view_golden as mm  # noqa: E402
import view_mask_cases as vm  # noqa: E402

MARGIN = mm.MARGIN
CODES = {"AssertionError": -2, "ValueError": -1}


def run_case(ns, c, rseed, full=False):
    """The reference frame after frame on the present views (``full``: on all views) -> one dict per frame."""
    hm, proj, valid, vv = vm.build(c)
    random.seed(rseed)
    frames = []
    with mm.Spy(ns) as spy:
        for b in range(c["b"]):
            present = np.arange(c["v"]) if full else np.flatnonzero(vv[b])
            n0, res, err = len(spy.calls), None, None
            if len(present) == 0:
                # not handed to the reference: its key-point decode fails on an empty tensor (IndexError) before it reaches
                # either error.  Counted as the frames with one view are: the assert with a valid joint, np.min([]) without
                frames.append(dict(res=None, err="AssertionError" if valid[b].any() else "ValueError", calls=[],
                                   present=present, digest=vm.state_digest(random.getstate())))
                continue
            try:
                res = ns.triangulation.triangulation(torch.from_numpy(hm[b][present]), torch.from_numpy(proj[b][present]),
                                                     c["stride"], torch.from_numpy(valid[b]), n_iters=c["n_iters"],
                                                     reprojection_error_epsilon=vm.EPS)
            except (AssertionError, ValueError) as e:
                err = type(e).__name__
            frames.append(dict(res=res, err=err, calls=spy.calls[n0:], present=present,
                               digest=vm.state_digest(random.getstate())))
    return frames, valid, vv


def per_joint(frame, valid_b, key, dtype):
    out = np.zeros(valid_b.shape, dtype)
    if frame["err"] is None:
        out[np.flatnonzero(valid_b)] = [k[key] for k in frame["calls"]]
    return out


def pair_table(c, frames, valid):
    tab = np.full((c["b"], c["j"], vm.n_pairs(c), 2), vm.PAD, np.uint8)
    for b, f in enumerate(frames):
        present = f["present"]
        lex = np.array(list(itertools.combinations(present.tolist(), 2)), np.uint8).reshape(-1, 2)
        if len(lex) == 0:
            continue
        if len(lex) <= c["n_iters"]:
            assert all(k["pairs"] is None for k in f["calls"])
            tab[b, :, : len(lex)] = lex
            continue
        tab[b] = 0
        for ji, k in zip(np.flatnonzero(valid[b]), f["calls"]):
            tab[b, ji] = present[np.array(k["pairs"])]
    return tab


def check(ns, c, say=print):
    frames, valid, vv = run_case(ns, c, c["rseed"])
    calls = [(k, len(f["present"])) for f in frames for k in f["calls"] if f["err"] is None]
    margin = min([mm.vote_margin(k, n) for k, n in calls] or [np.inf])
    ok, notes = margin >= MARGIN, ["margin %.3e" % margin]
    if c["sensitive"]:
        full, _, _ = run_case(ns, c, c["rseed"], full=True)
        for b, (f, g) in enumerate(zip(frames, full)):
            if vv[b].all():
                continue
            differ = int((per_joint(f, valid[b], "n", np.int64) != per_joint(g, valid[b], "n", np.int64)).sum())
            notes.append("frame %d: %d joints differ from the all-view run" % (b, differ))
            ok = ok and differ >= 1
    if c["sampled"]:
        other, _, _ = run_case(ns, c, c["rseed"] + 1)
        drawing = vm.draws(c)
        assert drawing.any()
        pairs = [(k, k2) for b in np.flatnonzero(drawing) for k, k2 in zip(frames[b]["calls"], other[b]["calls"])]
        assert all(k["pairs"] is not None for k, _ in pairs)
        changed = sum(not np.array_equal(k["x"], k2["x"]) for k, k2 in pairs)
        notes.append("changed under rseed+1: %d of %d" % (changed, len(pairs)))
        ok = ok and 4 * changed >= len(pairs)
    say("  seed %d: %s -> %s" % (c["seed"], "; ".join(notes), "ok" if ok else "NO"))
    return ok, (frames, valid, vv)


def hp_values(c, valid, vv):
    hm = vm.build(c)[0]
    out = {}
    for cfgk in ("AVG", "STD"):
        st = ref_harness.make_strategy("HP", **{"AL.HP_CONFIG": cfgk})
        vals = []
        for b in range(c["b"]):
            present = np.flatnonzero(vv[b])
            try:
                with np.errstate(all="ignore"):
                    import warnings

                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        vals.append(float(torch.tensor(st._compute_hp(torch.from_numpy(hm[b][present]), torch.from_numpy(valid[b]))).item()))
            except ZeroDivisionError:  # no valid (view, joint) map: sum([]) / 0
                vals.append(float("nan"))
        out[cfgk] = np.asarray(vals, np.float64)
    return out


def gen_sal(ns):
    c = vm.sal_view_mask_case()
    loader, heatmaps = cases.build_sal_loader(c)
    hh, wh = c["h"] // c["stride"], c["w"] // c["stride"]
    tl, hms = [], []
    for i, (dp, hm, vv) in enumerate(zip(loader, heatmaps, vm.sal_view_valid(c))):
        hm = hm.reshape(c["b"], c["v"], c["j"], hh, wh)
        for k in range(c["b"]):
            present = np.flatnonzero(vv[k])
            one = {key: torch.from_numpy(val[k : k + 1]) for key, val in dp.items()}
            one["images"] = one["images"][:, present]
            one["proj_matrices"] = one["proj_matrices"][:, present]
            tl.append(one)
            hms.append(np.ascontiguousarray(hm[k][present]))
    st = ref_harness.make_strategy(c["strategy"], **{"POSE_ESTIMATOR.STRIDE": c["stride"]})
    it = iter(hms)
    random.seed(c["rseed"])
    with mm.Spy(ns) as spy:
        sal = st._compute_sal_dict(tl, lambda images: torch.from_numpy(next(it)))
    margin = min(mm.vote_margin(k, len(k["pts"])) for k in spy.calls)
    print("sal_dict view mask: margin %.3e, inlier counts %s" % (margin, sorted(set(sal["inlier_count"].values()))))
    assert margin >= MARGIN, "sal_dict view mask: (a) vote margin not met"
    import math
    from heapq import nlargest

    entry = {k: dict(d) for k, d in sal.items()}
    alm = {g: m for g, m in sal["al_metric"].items() if not math.isnan(m)}
    entry["nlargest"] = nlargest(c["select"], alm, key=alm.get)
    entry["state_digest"] = vm.state_digest(random.getstate())
    with open(os.path.join(HERE, "sal_dict_view_mask.json"), "w") as f:
        json.dump(entry, f)


def main():
    ns = ref_harness.load()
    search = "--search" in sys.argv
    out = {}
    for name, c in vm.view_mask_cases().items():
        print(name)
        if search:
            c = dict(c)
            while not check(ns, c)[0]:
                c["seed"] += 1
            print("  -> %s: seed=%d" % (name, c["seed"]))
            continue
        ok, (frames, valid, vv) = check(ns, c)
        assert ok, name + ": the committed seed does not meet (a) vote margin, (b) mask sensitivity or (c) pair dependence; run with --search"
        b, v, j = c["b"], c["v"], c["j"]
        kp2d = np.zeros((b, v, j, 2), np.int64)
        kp3d, metric, inl = np.zeros((b, j, 3)), np.full((b,), np.nan), np.zeros((b,), np.int64)
        for bi, f in enumerate(frames):
            if f["err"] is not None:
                inl[bi] = CODES[f["err"]]
                continue
            kp2d[bi, f["present"]] = f["res"]["keypoints_2d"]
            kp3d[bi], metric[bi], inl[bi] = f["res"]["keypoints_3d"], f["res"]["metric"], f["res"]["inlier_count"]
        print("  inlier_count", inl.tolist(), "errors", [f["err"] for f in frames])
        hp = hp_values(c, valid, vv)
        out[name + "/rseed"] = np.int64(c["rseed"])
        out[name + "/pairs"] = pair_table(c, frames, valid)
        out[name + "/frame_digests"] = np.array([f["digest"] for f in frames])
        out[name + "/keypoints_2d"] = kp2d
        out[name + "/keypoints_3d"] = kp3d
        out[name + "/metric"] = metric
        out[name + "/inlier_count"] = inl
        out[name + "/joint_error"] = np.stack([per_joint(f, valid[bi], "err", np.float64) for bi, f in enumerate(frames)])
        out[name + "/joint_inliers"] = np.stack([per_joint(f, valid[bi], "n", np.int64) for bi, f in enumerate(frames)])
        out[name + "/hp_avg"], out[name + "/hp_std"] = hp["AVG"], hp["STD"]
    if search:
        return
    versions = json.dumps(dict(numpy=np.__version__, torch=torch.__version__, python=sys.version.split()[0]))
    np.savez_compressed(os.path.join(HERE, "view_mask.npz"), versions=versions, **out)
    gen_sal(ns)


if __name__ == "__main__":
    main()

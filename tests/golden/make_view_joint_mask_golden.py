"""Generate the per-(view, joint) visibility goldens by running the REAL reference (build container only):

    python tests/golden/make_view_joint_mask_golden.py            # check the committed case seeds, write the fixture
    python tests/golden/make_view_joint_mask_golden.py --search   # print, per case, the first seed >= the committed one that passes

  view_joint_mask.npz  per case of view_joint_mask_cases.view_joint_mask_cases(): after ``random.seed(rseed)`` once per case,
                       frame after frame: the reference's own key-point decode (``get_scaled_pred_corrdinates``) of the
                       whole frame, then its ``_triangulate_ransac`` joint after joint (valid joints ascending) on
                       ``proj[b][views_j]``, ``keypoints_2d[views_j, j]`` -- views_j the views that have the joint; a joint
                       with fewer than two of them is not handed over (the reference would assert) and is written like an
                       invalid joint.  Stored: keypoints_2d dense (B, V, J, 2) with absent entries zero, keypoints_3d, per-joint
                       mean error / inlier count, the frame's metric = ``np.mean`` and inlier_count = ``np.min`` over the
                       joints handed over (no valid joint: -1; a valid joint but none handed over: -2; metric NaN in both --
                       this project's codes, view_mask.npz has the same), the pair table in ORIGINAL view indices laid out as
                       utils.triangulation.draw_view_pairs lays it out (drawn rows as the reference drew them; padding 255),
                       a digest of ``random.getstate()`` after every frame, the per-map HP values of ``_compute_hp`` (AVG
                       config: the value of a one-map list is the map's value) on (1, 1, h, w) slices of every present
                       entry of a valid joint (hp_map, NaN elsewhere), and the frame values the reference's arithmetic
                       gives on that list in view-major order: ``sum(list) / len(list)`` (hp_avg) and ``np.std`` (hp_std),
                       NaN for an empty list.

The draws are captured from the reference with the recording stand-in of make_many_view_golden.py (``Spy``).

Every case must meet three conditions (the search moves the case seed on until they hold):
  (a) vote margin: min |err - eps| over the pairs walked and all present views of every problem handed over >= 1e-6 px, so
      that the strict ``err < eps`` vote is decidable between two float64 implementations -- no problem is left out;
  (b) sensitivity: in every frame with an absent entry, the same per-joint run on ALL views differs from the masked run in
      joint_inliers for at least one joint -- an implementation that ignores the mask cannot pass;
  (c) sampled cases: under ``random.seed(rseed + 1)`` at least a quarter of the problems that draw give a different 3-D
      point -- the result depends on the draw.
"""
from __future__ import annotations

import itertools
import json
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import ref_harness  # noqa: E402

import make_many_view_golden as mm  # noqa: E402
import view_joint_mask_cases as vj  # noqa: E402

MARGIN = mm.MARGIN


def run_case(ns, c, rseed, full=False):
    """The reference joint after joint on the views that have the joint (``full``: on all views) -> one dict per frame:
    kp (V, J, 2) the reference's decode, calls {joint: spy record}, digest."""
    hm, proj, valid, mask = vj.build(c)
    if full:
        mask = np.ones_like(mask)
    tri = ns.triangulation
    random.seed(rseed)
    frames = []
    with mm.Spy(ns) as spy:
        for b in range(c["b"]):
            kp = np.asarray(tri.get_scaled_pred_corrdinates(torch.from_numpy(hm[b]), c["stride"], c["j"], torch.from_numpy(valid[b])))
            calls = {}
            for j in np.flatnonzero(valid[b]):
                views = np.flatnonzero(mask[b, :, j])
                if len(views) < 2:
                    continue
                tri._triangulate_ransac(proj[b][views], kp[views, j], c["n_iters"], vj.EPS, False)
                calls[int(j)] = dict(spy.calls[-1], views=views)
            frames.append(dict(kp=kp, calls=calls, digest=vj.state_digest(random.getstate())))
    return frames, valid, mask


def per_joint(frame, j_count, key, dtype):
    out = np.zeros((j_count,), dtype)
    for j, k in frame["calls"].items():
        out[j] = k[key]
    return out


def pair_table(c, frames, valid, mask):
    tab = np.full((c["b"], c["j"], vj.n_pairs(c), 2), vj.PAD, np.uint8)
    for b, f in enumerate(frames):
        for j in range(c["j"]):
            views = np.flatnonzero(mask[b, :, j])
            lex = np.array(list(itertools.combinations(views.tolist(), 2)), np.uint8).reshape(-1, 2)
            if len(lex) == 0:
                continue
            if len(lex) <= c["n_iters"]:
                assert j not in f["calls"] or f["calls"][j]["pairs"] is None
                tab[b, j, : len(lex)] = lex
                continue
            tab[b, j] = 0
            if valid[b, j]:
                tab[b, j] = views[np.array(f["calls"][j]["pairs"])]
    return tab


def check(ns, c, say=print):
    frames, valid, mask = run_case(ns, c, c["rseed"])
    calls = [k for f in frames for k in f["calls"].values()]
    margin = min([mm.vote_margin(k, len(k["views"])) for k in calls] or [np.inf])
    ok, notes = margin >= MARGIN, ["margin %.3e" % margin]
    full, _, _ = run_case(ns, c, c["rseed"], full=True)
    for b, (f, g) in enumerate(zip(frames, full)):
        if mask[b].all():
            continue
        differ = int((per_joint(f, c["j"], "n", np.int64) != per_joint(g, c["j"], "n", np.int64)).sum())
        notes.append("frame %d: %d joints differ from the all-view run" % (b, differ))
        ok = ok and differ >= 1
    if c["sampled"]:
        other, _, _ = run_case(ns, c, c["rseed"] + 1)
        drawing = vj.draws(c)
        assert drawing.any()
        pairs = [(frames[b]["calls"][j], other[b]["calls"][j]) for b, j in zip(*np.nonzero(drawing))]
        assert all(k["pairs"] is not None for k, _ in pairs)
        changed = sum(not np.array_equal(k["x"], k2["x"]) for k, k2 in pairs)
        notes.append("changed under rseed+1: %d of %d" % (changed, len(pairs)))
        ok = ok and 4 * changed >= len(pairs)
    say("  seed %d: %s -> %s" % (c["seed"], "; ".join(notes), "ok" if ok else "NO"))
    return ok, (frames, valid, mask)


def hp_values(c, valid, mask):
    """-> hp_map (B, V, J) float64 (NaN where the entry is absent or the joint invalid), hp_avg, hp_std (B,)."""
    hm = vj.build(c)[0]
    st = ref_harness.make_strategy("HP", **{"AL.HP_CONFIG": "AVG"})
    per_map = np.full((c["b"], c["v"], c["j"]), np.nan)
    avg, std = np.full((c["b"],), np.nan), np.full((c["b"],), np.nan)
    one = torch.ones((1,), dtype=torch.bool)
    for b in range(c["b"]):
        hps = []
        for v in range(c["v"]):
            for j in range(c["j"]):
                if not (valid[b, j] and mask[b, v, j]):
                    continue
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    per_map[b, v, j] = st._compute_hp(torch.from_numpy(hm[b, v : v + 1, j : j + 1]), one)
                hps.append(per_map[b, v, j])
        if hps:  # strategy.py:1188-1193 on the list
            avg[b] = sum(hps) / len(hps)
            std[b] = np.std(np.array(hps))
    return per_map, avg, std


def main():
    ns = ref_harness.load()
    search = "--search" in sys.argv
    out = {}
    for name, c in vj.view_joint_mask_cases().items():
        print(name)
        if search:
            c = dict(c)
            while not check(ns, c)[0]:
                c["seed"] += 1
            print("  -> %s: seed=%d" % (name, c["seed"]))
            continue
        ok, (frames, valid, mask) = check(ns, c)
        assert ok, name + ": the committed seed does not meet (a) vote margin, (b) mask sensitivity or (c) pair dependence; run with --search"
        b, v, j = c["b"], c["v"], c["j"]
        kp2d = np.zeros((b, v, j, 2), np.int64)
        kp3d, metric, inl = np.zeros((b, j, 3)), np.full((b,), np.nan), np.zeros((b,), np.int64)
        for bi, f in enumerate(frames):
            kp2d[bi] = np.where(mask[bi][:, :, None], f["kp"], 0)
            for ji, k in f["calls"].items():
                kp3d[bi, ji] = k["x"]
            if f["calls"]:
                order = sorted(f["calls"])
                metric[bi] = np.mean([f["calls"][ji]["err"] for ji in order])  # utils/triangulation.py:226
                inl[bi] = np.min([f["calls"][ji]["n"] for ji in order])  # :231
            else:
                inl[bi] = -2 if valid[bi].any() else -1
        print("  inlier_count", inl.tolist(), "used joints per frame", [len(f["calls"]) for f in frames])
        assert (np.array([[ji in f["calls"] for ji in range(j)] for f in frames]) == vj.used(c)).all()
        out[name + "/rseed"] = np.int64(c["rseed"])
        out[name + "/pairs"] = pair_table(c, frames, valid, mask)
        out[name + "/frame_digests"] = np.array([f["digest"] for f in frames])
        out[name + "/keypoints_2d"] = kp2d
        out[name + "/keypoints_3d"] = kp3d
        out[name + "/metric"] = metric
        out[name + "/inlier_count"] = inl
        out[name + "/joint_error"] = np.stack([per_joint(f, j, "err", np.float64) for f in frames])
        out[name + "/joint_inliers"] = np.stack([per_joint(f, j, "n", np.int64) for f in frames])
        out[name + "/hp_map"], out[name + "/hp_avg"], out[name + "/hp_std"] = hp_values(c, valid, mask)
    if search:
        return
    versions = json.dumps(dict(numpy=np.__version__, torch=torch.__version__, python=sys.version.split()[0]))
    np.savez_compressed(os.path.join(HERE, "view_joint_mask.npz"), versions=versions, **out)


if __name__ == "__main__":
    main()

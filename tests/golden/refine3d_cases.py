"""Cases of the 3-D refinement goldens (tests/golden/refine3d.npz, written by make_refine3d_golden.py): seeded ring rigs whose
cameras stand at unequal distances (radii drawn from 1500 .. 6000 mm, f = 300 px, all looking at the origin), joints
~N(0, 300 mm), B = 3 frames of J = 5 joints.  The 2-D key-points are the projections snapped to the stride-4 grid plus
N(0, 1.5 px) noise, once rounded to int64 and once as float32: the two key-point types of the triangulation entries.

A case may add: ``outlier`` (one view per frame, b % V, whose points are moved by 60 px: it must fall out of the support set),
``invalid`` ((frame, joint) pairs whose joint is invalid), ``absent`` ((frame, view) pairs: a ``view_valid`` case),
``absent_vj`` ((frame, view, joint) triples: a ``view_joint_valid`` case) -- the matrices of an absent view and the float32
key-points of an absent entry are NaN, the int64 ones a value far outside every image --, ``weighted`` (float32 weights
(B, V, J) from U(0.2, 1), some 0, negative or NaN: those views leave the support set), ``split`` (both views of a two-view
rig are moved apart, so that fewer than two views are within eps of the DLT point).

Nothing here needs the device; the tests import ``refine3d_cases()``, ``build`` and ``load_golden``.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np

EPS = 5.0  # reprojection_error_epsilon, the reference's default
N_ITERS = 496  # every pair of up to 32 views, lexicographic: nothing is drawn from an RNG
FAR = 1 << 20  # the int64 key-point of an absent entry


def refine3d_cases():
    base = dict(b=3, j=5, outlier=False, invalid=(), absent=(), absent_vj=(), weighted=False, split=False)
    return OrderedDict(
        v2=dict(base, seed=7102, v=2, invalid=((1, 3),)),
        v3=dict(base, seed=7103, v=3),  # (two good views and a moved one: RANSAC cannot tell which pair is right)
        v4=dict(base, seed=7104, v=4, outlier=True, invalid=((0, 0), (2, 4))),
        v8=dict(base, seed=7108, v=8, outlier=True),
        v12=dict(base, seed=7112, v=12, outlier=True, invalid=((1, 1),)),
        v32=dict(base, seed=7132, v=32, outlier=True),
        v4_views=dict(base, seed=7204, v=4, absent=((0, 3), (2, 0))),
        v8_view_joint=dict(base, seed=7208, v=8, outlier=True,
                           absent_vj=((0, 0, 1), (0, 7, 1), (0, 3, 2), (1, 2, 0), (1, 4, 4), (2, 1, 3), (2, 5, 3), (2, 6, 3)) +
                           tuple((1, v, 2) for v in range(7))),  # (frame 1, joint 2: one view left, an unused joint)
        v4_weighted=dict(base, seed=7304, v=4, weighted=True, invalid=((1, 2),)),
        v2_split=dict(base, seed=7402, v=2, split=True),
    )


def rig(rng, v):
    """-> proj (V, 3, 4): cameras on a ring around the origin at radii from 1500 .. 6000 mm, looking at it."""
    out = np.zeros((v, 3, 4))
    k = np.array([[300.0, 0, 128.0], [0, 300.0, 128.0], [0, 0, 1]])
    for i in range(v):
        a = 2 * np.pi * (i + rng.uniform(-0.2, 0.2)) / max(v, 3) + 0.3
        c = rng.uniform(1500.0, 6000.0) * np.array([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.3)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        r = np.stack([x, np.cross(z, x), z])
        out[i] = k @ np.concatenate([r, (-r @ c)[:, None]], axis=1)
    return out


def project(proj, X):
    h = np.einsum("...vik,...jk->...vji", proj[..., :3], X) + proj[..., None, :, 3]
    return h[..., :2] / h[..., 2:]


def build(c):
    """-> dict: proj (B, V, 3, 4) f64, joints (B, J, 3), kp_i64 / kp_f32 (B, V, J, 2), valid (B, J) bool, view_valid (B, V) bool
    or None, view_joint_valid (B, V, J) bool or None, weights (B, V, J) f32 or None."""
    rng = np.random.default_rng(c["seed"])
    b, v, j = c["b"], c["v"], c["j"]
    proj = np.stack([rig(rng, v) for _ in range(b)])
    joints = rng.normal(0.0, 300.0, (b, j, 3))
    kp = np.round(project(proj, joints) / 4.0) * 4.0 + rng.normal(0.0, 1.5, (b, v, j, 2))
    if c["outlier"]:
        for bi in range(b):
            kp[bi, bi % v] += 60.0
    if c["split"]:
        kp[:, 0, :, 1] += 40.0
        kp[:, 1, :, 1] -= 40.0
    valid = np.ones((b, j), bool)
    for bi, ji in c["invalid"]:
        valid[bi, ji] = False
    kp_i64, kp_f32 = np.round(kp).astype(np.int64), kp.astype(np.float32)
    view_valid = view_joint_valid = weights = None
    if c["absent"]:
        view_valid = np.ones((b, v), bool)
        for bi, vi in c["absent"]:
            view_valid[bi, vi] = False
        proj[~view_valid] = np.nan
        kp_i64[~view_valid], kp_f32[~view_valid] = FAR, np.nan
    if c["absent_vj"]:
        view_joint_valid = np.ones((b, v, j), bool)
        for bi, vi, ji in c["absent_vj"]:
            view_joint_valid[bi, vi, ji] = False
        kp_i64[~view_joint_valid], kp_f32[~view_joint_valid] = FAR, np.nan
    if c["weighted"]:
        weights = rng.uniform(0.2, 1.0, (b, v, j)).astype(np.float32)
        weights[0, 1, 0], weights[1, 2, 1], weights[2, 0, 3], weights[2, 3, 4] = 0.0, -1.0, np.nan, np.inf
        weights[0, :3, 4] = 0.0  # one view left in S: not refined
    return dict(proj=proj, joints=joints, kp_i64=kp_i64, kp_f32=kp_f32, valid=valid, view_valid=view_valid,
                view_joint_valid=view_joint_valid, weights=weights)


def present_views(d, bi, ji):
    """-> (V,) bool: the views problem (bi, ji) is triangulated from."""
    if d["view_joint_valid"] is not None:
        return d["view_joint_valid"][bi, :, ji]
    if d["view_valid"] is not None:
        return d["view_valid"][bi]
    return np.ones(d["proj"].shape[1], bool)


def accuracy_rig(seed=7500, b=15, j=20):
    """The unequal-radius rig of DESIGN.md 6.5: four ring cameras at 1500 / 3000 / 4500 / 6000 mm (f = 300 px), joints
    ~N(0, 300 mm), 300 problems as B = 15 frames of J = 20 joints, the 2-D points snapped to the stride-4 grid (what the hard
    arg-max of a stride-4 heat-map gives).  -> proj (B, 4, 3, 4), joints (B, J, 3), kp (B, 4, J, 2) int64."""
    rng = np.random.default_rng(seed)
    k = np.array([[300.0, 0, 128.0], [0, 300.0, 128.0], [0, 0, 1]])
    one = np.zeros((4, 3, 4))
    for i, radius in enumerate((1500.0, 3000.0, 4500.0, 6000.0)):
        a = 2 * np.pi * (i + rng.uniform(-0.25, 0.25)) / 4
        c = np.array([radius * np.cos(a), radius * np.sin(a), 400.0 * rng.uniform(-1, 1)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        r = np.stack([x, np.cross(z, x), z])
        one[i] = k @ np.concatenate([r, (-r @ c)[:, None]], axis=1)
    proj = np.stack([one] * b)
    joints = rng.normal(0.0, 300.0, (b, j, 3))
    kp = (np.round(project(proj, joints) / 4.0) * 4.0).astype(np.int64)
    return proj, joints, kp


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refine3d.npz")


def load_golden():
    return np.load(GOLDEN)


def tolerances(g):
    """-> {V: tolerance in mm}: four times the largest recorded ``gap_oracle`` among the refined problems of the cases with
    that many views (DESIGN.md 6.5 lists them)."""
    gaps = {}
    for name, c in refine3d_cases().items():
        for kind in ("i64", "f32"):
            refined = g[f"{name}/{kind}/status"] != 0
            if refined.any():
                gaps[c["v"]] = max(gaps.get(c["v"], 0.0), float(g[f"{name}/{kind}/gap_oracle"][refined].max()))
    return {v: 4.0 * gap for v, gap in gaps.items()}

"""Cases of the per-(view, joint) visibility goldens (tests/golden/view_joint_mask.npz): batches in which single joints are
missing from single views.  The oracle is exact: for every joint, the result under the mask is the reference's
``_triangulate_ransac`` handed the views that have the joint (``proj[b][views_j]``, ``keypoints_2d[views_j, j]``), which is
how make_view_joint_mask_golden.py calls it; the frame values are the reference's ``np.mean`` / ``np.min`` over the joints
that could be triangulated.

Inputs come from ``view_mask_cases.build`` (seeded, nothing stored); a case adds ``absent_vj``: per frame a tuple of rules
``(joints, views)`` -- those views lack those joints; ``joints`` None means every joint of the frame.  The heat-maps of an
absent entry are built like every other map: they carry a consistent peak (outlier views apart), so an implementation that
lets an absent entry vote counts it as an inlier and differs from the golden in ``joint_inliers`` (the generator asserts
this for every frame with an absent entry).  The sampled cases put heavy outliers among the views so that the result
depends on the drawn pairs.  Maps are 64 x 64, 64 x 48 for the non-square case (view_mask_cases.py says why).
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import view_mask_cases as vm
from view_mask_cases import EPS, PAD, load_golden, state_digest  # noqa: F401  (shared with the tests)


def view_joint_mask_cases():
    base = dict(h=256, w=256, stride=4, noise=0.05, j=19, invalid=(), n_iters=64, sampled=False, no_valid_joint=(), outliers=0)
    return OrderedDict(
        # frame 0: joints with 4 (most), 3, 2 (one pair in an 8-lane group), 1 and 0 present views beside each other, one
        # invalid joint; frame 1: every joint in one view only -> no used joint, -2; frame 2: no valid joint -> -1
        j4=dict(base, seed=601, rseed=31, v=4, b=3, invalid=(4,), no_valid_joint=(2,),
                absent_vj=((((1, 9), (0,)), ((2,), (0, 3)), ((3, 18), (0, 1, 2)), ((5,), (0, 1, 2, 3)), ((6,), (1, 2))),
                           ((None, (0, 1, 2)),),
                           ())),
        # first and last mask bit absent for some joints only; the shape[2] quirk of the decode; one outlier view
        j8_nonsquare=dict(base, seed=602, rseed=32, v=8, b=2, w=192, outliers=1,
                          absent_vj=((((0, 7, 12), (0,)), ((3, 7), (7,)), ((18,), (0, 7))),
                                     (((1,), (7,)), ((2, 3), (0, 3, 4)), ((10,), (1, 2, 3, 4, 5, 6))))),
        # the 55-pair group (PG = 64) with per-joint holes
        j11=dict(base, seed=603, rseed=33, v=11, b=2, outliers=3,
                 absent_vj=((((0, 5), (10,)), ((6,), (0, 5)), ((17,), (1, 2, 3, 4, 6, 7, 8, 9, 10))),
                            (((2, 8), (3, 9)), ((18,), (0,))))),
        # ONE frame: most joints see all 12 views (draw 64 of 66), some 11 (55 pairs, lexicographic), some 10 (45): padded
        # per-problem tables inside one frame, and only the drawing joints move the RNG
        j12_mixed=dict(base, seed=604, rseed=34, v=12, b=1, outliers=9, invalid=(3,), sampled=True,
                       absent_vj=((((1, 7, 13), (4,)), ((2, 8, 14), (0, 11)), ((5,), (6,))),)),
        # mask bit 31 absent for joint 6 and present for its neighbours; 64 of 465 / 496 pairs drawn
        j32=dict(base, seed=605, rseed=35, v=32, b=1, outliers=27, sampled=True,
                 absent_vj=((((6,), (31,)), ((11,), (0, 31)), ((12,), (0,))),)),
    )


def view_joint_valid(c):
    """-> (B, V, J) bool, True = the joint is usable in that view."""
    vj = np.ones((c["b"], c["v"], c["j"]), dtype=bool)
    for b, rules in enumerate(c["absent_vj"]):
        for joints, views in rules:
            for v in views:
                vj[b, v, slice(None) if joints is None else list(joints)] = False
    return vj


def build(c):
    """-> heatmaps (B,V,J,Hh,Wh) f32, proj (B,V,3,4) f64, valid (B,J) bool, view_joint_valid (B,V,J) bool."""
    hm, proj, valid, _ = vm.build(dict(c, absent=((),) * c["b"]))
    return hm, proj, valid, view_joint_valid(c)


def valid_joints(c):
    """-> (B, J) bool, without building the heat-maps."""
    valid = np.ones((c["b"], c["j"]), dtype=bool)
    valid[:, list(c["invalid"])] = False
    valid[list(c["no_valid_joint"])] = False
    return valid


def n_present_pairs(c):
    """-> (B, J): C(n_bj, 2) of every problem."""
    n = view_joint_valid(c).sum(axis=1)
    return n * (n - 1) // 2


def n_pairs(c):
    """P of the case's pair table: max over problems of min(C(n_bj, 2), n_iters), at least 1."""
    return max(1, int(np.minimum(n_present_pairs(c), c["n_iters"]).max()))


def draws(c):
    """-> (B, J) bool: the problems that draw -- valid joints whose C(n_bj, 2) present pairs exceed n_iters."""
    return (n_present_pairs(c) > c["n_iters"]) & valid_joints(c)


def used(c):
    """-> (B, J) bool: valid joints with two or more present views."""
    return (view_joint_valid(c).sum(axis=1) >= 2) & valid_joints(c)

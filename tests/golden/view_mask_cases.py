"""Cases of the missing-view goldens (tests/golden/view_mask.npz, sal_dict_view_mask.json): batches whose frames lack
some of the rig's views.  The oracle is exact: for every frame, the result under a view mask is the reference run on that
frame's present views alone (``heatmaps[b][present]``, ``proj[b][present]``), which is how make_view_mask_golden.py calls it.

Like many_view_cases.py, both sides build their INPUTS from these seeded definitions (``cases.build_triangulation_case``
/ ``cases.build_sal_loader``) plus one ``absent`` tuple per frame, and the fixture holds outputs only: the reference's
results scattered back to the dense (B, V, ...) layout (rows of absent views zero), the pairs it drew mapped to ORIGINAL
view indices, a digest of the RNG state after every frame, and its ``_compute_hp`` (AVG and STD) on the sliced heat-maps.

The heat-maps and matrices of an absent view are built like every other view's: in the *sensitive* cases they carry a
consistent peak and a correct matrix, so an implementation that lets an absent view vote counts it as an inlier and
differs from the golden in ``joint_inliers`` (the generator asserts this, condition b).  The *sampled* cases put heavy
outliers among the views (``outliers`` counts views of the whole rig, see many_view_cases.py) so that the result depends
on the drawn pairs (condition c).  Maps are 64 x 64 (256 x 256 images at stride 4; many_view_cases.py says why smaller maps
make every vote an inlier), 64 x 48 for the non-square case.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import cases
from many_view_cases import EPS, load_golden, state_digest  # noqa: F401  (shared with the tests)

PAD = 255  # utils.triangulation.PAIR_PAD


def view_mask_cases():
    base = dict(h=256, w=256, stride=4, noise=0.05, j=19, invalid=(), n_iters=64, sensitive=False, sampled=False,
                no_valid_joint=())
    return OrderedDict(
        # absent views with a consistent peak; frame 2 has exactly two present views = one pair in an 8-lane group
        m4=dict(base, seed=501, rseed=21, v=4, b=3, outliers=0, invalid=(4, 11), absent=((), (0,), (1, 3)), sensitive=True),
        # first and last mask bit absent, the shape[2] quirk of the decode, one outlier view
        m8_nonsquare=dict(base, seed=502, rseed=22, v=8, b=2, w=192, outliers=1, absent=((0, 7), (2, 3, 4)), sensitive=True),
        # 55-pair group, PG = 64
        m11=dict(base, seed=503, rseed=23, v=11, b=2, outliers=3, absent=((10,), (0, 5))),
        # ONE batch: frame 0 has 55 pairs (nothing drawn), frame 1 draws 64 of 66, frame 2 has 45: padded per-problem
        # tables, and frame 1 alone moves the RNG
        m12_mixed=dict(base, seed=504, rseed=24, v=12, b=3, outliers=9, invalid=(3,), absent=((3,), (), (0, 11)), sampled=True),
        # 15 present: 100 of 105 drawn; 14 present: all 91; two lane trips
        m16_n100=dict(base, seed=506, rseed=25, v=16, b=2, n_iters=100, outliers=12, absent=((5,), (2, 9)), sampled=True),
        # mask bit 31 clear in frame 0, set in frame 1; 64 of 465 pairs drawn in both
        m32=dict(base, seed=506, rseed=26, v=32, b=2, outliers=27, absent=((31,), (0,)), sampled=True),
        # one present view; none; one present view and no valid joint: -2, -2, -1
        degenerate=dict(base, seed=507, rseed=27, v=4, b=3, outliers=0, absent=((0, 1, 2), (0, 1, 2, 3), (1, 2, 3)),
                        no_valid_joint=(2,)),
    )


def sal_view_mask_case():
    """_compute_sal_dict on a masked loader: V = 4, B = 2 per batch, built like cases.sal_cases(); ``absent`` per batch,
    per frame.  The reference gets one sliced frame per batch (one rank: the key order is the frame order)."""
    return dict(seed=48, rseed=28, nbatch=2, b=2, v=4, j=19, h=256, w=256, stride=4, noise=0.05, outliers=1, select=2,
                strategy="TRIANGULATION", absent=(((), (2,)), ((0, 3), (1,))))


def view_valid(c):
    """-> (B, V) bool, True = present."""
    vv = np.ones((c["b"], c["v"]), dtype=bool)
    for b, absent in enumerate(c["absent"]):
        vv[b, list(absent)] = False
    return vv


def sal_view_valid(c):
    """-> list (one per batch) of (B, V) bool."""
    return [view_valid(dict(b=c["b"], v=c["v"], absent=a)) for a in c["absent"]]


def build(c):
    """-> heatmaps (B,V,J,Hh,Wh) f32, proj (B,V,3,4) f64, valid (B,J) bool, view_valid (B,V) bool."""
    hm, proj, valid = cases.build_triangulation_case(c)
    for b in c["no_valid_joint"]:
        valid[b] = False
    return hm, proj, valid, view_valid(c)


def n_pairs(c):
    """P of the case's pair table: max over frames of min(C(n_b, 2), n_iters), at least 1."""
    n = view_valid(c).sum(axis=1)
    return max(1, int(np.minimum(n * (n - 1) // 2, c["n_iters"]).max()))


def draws(c):
    """-> (B,) bool: the frames whose C(n_b, 2) present pairs exceed n_iters."""
    n = view_valid(c).sum(axis=1)
    return n * (n - 1) // 2 > c["n_iters"]

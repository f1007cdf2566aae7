"""Cases of the undistortion goldens (tests/golden/undistort.npz, written by make_undistort_golden.py): seeded ring rigs of
full-frame cameras (f = 1400 px, 1920 x 1080, 3000 mm from the origin, aimed up to 800 mm beside it so that the joints sit off
the optical axis), each cropped to a square box around its joints and resized to at most 384 px through the reference's
``Camera.update_after_crop`` / ``update_after_resize``: f comes out at about 600 .. 1500 px and every coordinate below 512.
Joints are drawn within +-350 mm; the make script admits a joint only if det J >= 0.25 at its true point in every present view
and redraws it otherwise.

A case names its lens per view (``lens``: a tuple cycled over the views; None = a camera without ``dist``), and may add
``invalid`` ((frame, joint) pairs), ``absent`` ((frame, view) pairs: a ``view_valid`` case whose absent views hold NaN in K and
dist), ``absent_vj`` ((frame, view, joint) triples: a ``view_joint_valid`` case), ``skew`` (K01 of the full-frame camera) and
``fold`` (joints whose key-points, in every view, are no projections but pixels beyond the lens's monotone radius: the solver
must stop there with MVAL_UNDISTORT_FOLD).

Nothing here needs the device or the reference; the tests import ``undistort_cases()``, ``load_golden`` and ``case_arrays``.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import numpy as np

EPS = 5.0  # reprojection_error_epsilon, the reference's default
N_ITERS = 496  # every pair of up to 32 views, lexicographic: nothing is drawn from an RNG
MIN_DET = 0.25  # a joint is admitted when det J at its true point is at least this in every present view
FOLD_MARGIN = 1e-3  # a fold entry is admitted when its failing det J is below -this and every earlier one above +this
FULL_W, FULL_H, FULL_F, RING = 1920, 1080, 1400.0, 3000.0

BARREL = (-0.25, 0.15, 3e-4, 8e-4, -0.04)
MILD_BARREL = (-0.10, 0.0, 0.0, 0.0, 0.0)
STRONG_BARREL = (-0.35, 0.0, 0.0, 0.0, 0.0)
PINCUSHION = (0.20, 0.05, 0.0, 0.0, 0.01)
TANGENTIAL = (0.0, 0.0, 2e-3, -1.5e-3, 0.0)
FOLDING = (-0.5, 0.0, 0.0, 0.0, 0.0)  # monotone up to r = sqrt(2/3): no pixel beyond 0.544 f of the centre is an image of anything


def undistort_cases():
    base = dict(invalid=(), absent=(), absent_vj=(), skew=0.0, fold=(), in_w=384, in_h=384, e2e=True)
    return OrderedDict(
        pincushion=dict(base, seed=8101, b=1, v=2, j=1, lens=(PINCUSHION,)),
        barrel=dict(base, seed=8102, b=3, v=4, j=5, lens=(BARREL, STRONG_BARREL, MILD_BARREL, BARREL), invalid=((1, 3),)),
        tangential=dict(base, seed=8103, b=3, v=4, j=5, lens=(TANGENTIAL,), skew=0.75, in_w=384, in_h=320),
        mixed=dict(base, seed=8104, b=3, v=5, j=19, lens=(BARREL, None, STRONG_BARREL, None, PINCUSHION), invalid=((0, 7), (2, 18))),
        many_views=dict(base, seed=8105, b=2, v=32, j=3, lens=(MILD_BARREL, BARREL, None, PINCUSHION)),
        views_masked=dict(base, seed=8106, b=3, v=4, j=5, lens=(BARREL, PINCUSHION), absent=((0, 3), (2, 0))),
        view_joint_masked=dict(base, seed=8107, b=3, v=5, j=19, lens=(STRONG_BARREL, BARREL, None, MILD_BARREL, TANGENTIAL),
                               absent_vj=((0, 0, 1), (0, 4, 1), (0, 3, 2), (1, 2, 0), (1, 4, 18), (2, 1, 3), (2, 3, 3), (2, 1, 17)),
                               invalid=((1, 5),)),
        # (joints 1 and 3 are fold entries in every view: nothing to triangulate them from, so no end-to-end figure)
        fold=dict(base, seed=8108, b=3, v=4, j=5, lens=(FOLDING,), fold=(1, 3), e2e=False),
    )


def lens_of(c, vi):
    return c["lens"][vi % len(c["lens"])]


def draw_camera(rng, i, v, skew):
    """-> K (3, 3), R (3, 3), t (3,): a full-frame camera on the ring, aimed beside the origin."""
    a = 2 * np.pi * (i + rng.uniform(-0.2, 0.2)) / max(v, 3) + 0.3
    centre = RING * np.array([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.3)])
    z = rng.uniform(-800.0, 800.0, 3) - centre
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    r = np.stack([x, np.cross(z, x), z])
    k = np.array([[FULL_F * rng.uniform(0.95, 1.05), skew, FULL_W / 2 + rng.uniform(-20, 20)],
                  [0.0, FULL_F * rng.uniform(0.95, 1.05), FULL_H / 2 + rng.uniform(-20, 20)], [0.0, 0.0, 1.0]])
    return k, r, -r @ centre


def draw_joint(rng):
    return rng.uniform(-350.0, 350.0, 3)


def square_box(k, r, t):
    """The crop of a view: the square around the pinhole image of the +-350 mm cube, scaled by 1.1, integer corners."""
    corners = np.array([[sx, sy, sz] for sx in (-350.0, 350.0) for sy in (-350.0, 350.0) for sz in (-350.0, 350.0)])
    h = (k @ (r @ corners.T + t[:, None])).T
    p = h[:, :2] / h[:, 2:]
    cx, cy = (p.min(0) + p.max(0)) / 2
    half = 1.1 * max(p.max(0) - p.min(0)) / 2
    return tuple(int(round(q)) for q in (cx - half, cy - half, cx + half, cy + half))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "undistort.npz")


def load_golden():
    return np.load(GOLDEN)


def masks(c):
    """-> valid (B, J) bool, view_valid (B, V) bool or None, view_joint_valid (B, V, J) bool or None."""
    b, v, j = c["b"], c["v"], c["j"]
    valid = np.ones((b, j), bool)
    for bi, ji in c["invalid"]:
        valid[bi, ji] = False
    view_valid = view_joint_valid = None
    if c["absent"]:
        view_valid = np.ones((b, v), bool)
        for bi, vi in c["absent"]:
            view_valid[bi, vi] = False
    if c["absent_vj"]:
        view_joint_valid = np.ones((b, v, j), bool)
        for bi, vi, ji in c["absent_vj"]:
            view_joint_valid[bi, vi, ji] = False
    return valid, view_valid, view_joint_valid


def case_arrays(g, name):
    """The golden's arrays of one case as a dict (key without the ``<case>/`` prefix), with ``valid``, ``view_valid`` and
    ``view_joint_valid`` from the case list (None where the case has none)."""
    d = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    d["valid"], d["view_valid"], d["view_joint_valid"] = masks(undistort_cases()[name])
    return d

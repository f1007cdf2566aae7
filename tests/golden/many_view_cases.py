"""Cases of the many-view triangulation goldens (tests/golden/triangulation_many_views.npz, sal_dict_many_views.json):
rigs whose C(V,2) view pairs exceed ``n_iters``, where the reference shuffles the pair list of every valid joint with
python's global ``random`` and keeps the first ``n_iters`` (utils/triangulation.py:279-282).

Like cases.py, both sides build their INPUTS from these seeded definitions (``cases.build_triangulation_case`` /
``cases.build_sal_loader``), so the fixtures hold the reference's outputs, the pair tables it drew and a digest of the
RNG state it left behind.  ``rseed`` is what ``random.seed`` gets before the first frame of a case.

The heavy-outlier cases (``outliers = V - 3``) are the ones whose result DEPENDS on the drawn pairs: only three views
see the joint, the pairs among them gather different accidental inliers, and among sets of equal size the first in the
table wins -- so a wrong table, or a right table walked in another order, gives another point.  With few outliers every
sample leads to the same set and such inputs could not show a wrong table.  make_many_view_golden.py asserts this
(condition b) and two more for every case, and moves ``seed`` on until they hold; the seeds below are its result.

Map size: 256 x 256 images at stride 4, i.e. 64 x 64 maps, as in cases.triangulation_edge_cases().  The inlier vote is
``err < 5`` on half the pixel distance, a radius of 10 px: in a 64 x 64 image (16 x 16 maps) the ring cameras (f = 75 px)
put every joint within about 8 px of the centre and nearly every random outlier position inside that radius too, so
almost every view votes inlier whatever the pair and no input depends on the draw.  The inputs are rebuilt from the seeds
(about 0.1 s for the largest, V = 32 x J = 19 maps) and the fixture holds outputs only, 37 KB.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import cases

EPS = 5.0


def many_view_cases():
    base = dict(h=256, w=256, stride=4, noise=0.05, b=1, j=19, invalid=(), heavy=False)
    return OrderedDict(
        # P = 3, PG = 4: 16 problems per wave, each with its own table; 38 problems leave the last wave partial
        v4_n3=dict(base, seed=369, rseed=11, v=4, n_iters=3, b=2, outliers=1, invalid=(5,)),
        # the first sampled size at the default n_iters: 64 of 66 pairs, one problem per wave
        v12_sampled=dict(base, seed=101, rseed=12, v=12, n_iters=64, outliers=9, invalid=(3,), heavy=True),
        # all 66 pairs fit: nothing is drawn, shared lexicographic table, second lane trip of 2 lanes
        v12_all=dict(base, seed=302, rseed=13, v=12, n_iters=128, outliers=3),
        # 100 of 120 pairs: two lane trips, the second of 36 lanes
        v16_n100=dict(base, seed=303, rseed=14, v=16, n_iters=100, outliers=13, heavy=True),
        # inlier-mask bit 31 and the 32-entry error array
        v32_sampled=dict(base, seed=139, rseed=15, v=32, n_iters=64, outliers=27, heavy=True),
        # P = 496: eight lane trips (the last of 48 lanes), the largest reduction key
        v32_all=dict(base, seed=304, rseed=16, v=32, n_iters=496, j=5, outliers=4),
        # two frames in a row: the second starts from the RNG state the first left
        v12_frames=dict(base, seed=305, rseed=17, v=12, n_iters=64, b=2, outliers=9, invalid=(0, 18), heavy=True),
    )


def sal_many_view_case():
    """_compute_sal_dict at V = 12 with strategy TRIANGULATION, built like cases.sal_cases() / build_sal_loader."""
    return dict(seed=47, rseed=18, nbatch=2, b=2, v=12, j=19, h=256, w=256, stride=4, noise=0.05, outliers=9, select=2,
                strategy="TRIANGULATION", n_iters=64)


def n_pairs(c):
    return min(c["n_iters"], c["v"] * (c["v"] - 1) // 2)


def is_sampled(c):
    return c["v"] * (c["v"] - 1) // 2 > c["n_iters"]


def build(c):
    """-> heatmaps (B,V,J,Hh,Wh) f32, proj (B,V,3,4) f64, valid (B,J) bool."""
    return cases.build_triangulation_case(c)


def state_digest(state):
    """A short digest of ``random.getstate()``."""
    import hashlib

    return hashlib.sha256(repr(state).encode()).hexdigest()


def load_golden(path, name):
    z = np.load(path)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}

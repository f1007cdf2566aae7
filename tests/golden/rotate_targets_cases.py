"""Case definitions of the rotated-target fixtures (tests/golden/rotate_targets.npz, rotate_targets.json): shared by the generator
(make_rotate_targets_golden.py), the GPU tests (tests/test_gpu_rotate_targets.py) and the host tests (tests/test_rotate_targets_host.py).
Inputs are regenerated from seeds on both sides; the fixtures hold expected outputs, angles and the Pillow version only."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

# (h, w) of a heat-map: square; more rows than columns, several workgroups; the map of a 256 x 192 input; odd on both axes; smaller than the
# filter's four taps on one axis; a single row
SIZES = [(64, 64), (96, 72), (64, 48), (17, 23), (5, 4), (1, 7)]
# one view per angle: the reference's extremes, a small one of either sign, one with many digits, a nearly-zero one (d close to 0 and 1),
# and three that Pillow answers with a copy (0 mod 360), so that every launch mixes rotating and resting views
ANGLES = (30.0, -30.0, 7.0, -7.0, 12.345678, 0.001, 0.0, -0.0, 360.0)
MAPS = 3  # maps per view


def rests(angle):
    return angle % 360.0 == 0


def gaussian(h, w, cx, cy, sigma=1.0):
    """The ground-truth map of dataset.py:198-207 for a point (cx, cy), float64 arithmetic and one float32 rounding."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * sigma * sigma)).astype(np.float32)


def noise(rng, h, w):
    """Normal noise: full-mantissa taps of either sign, what separates float32 coefficient sums from float64 ones."""
    return rng.normal(0.0, 1.0, (h, w)).astype(np.float32)


def noisy_view(h, w, i):
    """Whether map 1 of view i is noise (else a Gaussian): every view of the small sizes; at the large ones two rotating views and a
    resting one, so that the expected outputs (noise does not compress) stay small."""
    return h * w <= 1024 or i in (0, 4, 6)


def size_seed(h, w):
    return 7000 + h * 128 + w


def single_maps(h, w, centres=False):
    """(len(ANGLES), MAPS, h, w) float32: per view a Gaussian somewhere inside, noise or a second Gaussian, and a Gaussian on the border.
    centres=True: also the (x, y) of map 0's Gaussian per view."""
    rng = np.random.default_rng(size_seed(h, w))
    out = np.empty((len(ANGLES), MAPS, h, w), dtype=np.float32)
    at = []
    for i in range(len(ANGLES)):
        at.append((rng.uniform(0, w - 1), rng.uniform(0, h - 1)))
        out[i, 0] = gaussian(h, w, *at[-1])
        second = (noise(rng, h, w), gaussian(h, w, rng.uniform(0, w - 1), rng.uniform(0, h - 1)))
        out[i, 1] = second[0] if noisy_view(h, w, i) else second[1]
        out[i, 2] = gaussian(h, w, rng.uniform(-1.5, 0.5) % w, rng.uniform(0, h - 1))  # (within 1.5 px of the left or the right edge)
    return (out, at) if centres else out


# ---- chains: K = 3, views with 0, 1, 2 and 3 rotations and other kinds between them -----------------------------------------------------
CHAIN_SIZE = (33, 29)  # odd on both axes, four workgroups per map
CHAIN_PLAN = [
    [("Invert", 0.0), ("Color", 0.52), ("Equalize", 0.0)],
    [("Rotate", 30.0), ("Invert", 0.0), ("Sharpness", 1.3)],
    [("Rotate", 30.0), ("Solarize", 100.0), ("Rotate", -30.0)],
    [("Rotate", 7.5), ("Rotate", -12.345678), ("Rotate", 29.999)],
    [("Posterize", 2.0), ("Rotate", -0.001), ("Rotate", 0.0)],
    [("Rotate", 360.0), ("Rotate", -0.0), ("Brightness", 1.0)],
]


def plan_angles(ops):
    """The angles of a view's effective rotations, in order."""
    return [float(val) for name, val in ops if name == "Rotate" and not rests(float(val))]


def chain_maps(centres=False):
    """(len(CHAIN_PLAN), MAPS, h, w) float32: a Gaussian at least 8 px inside, noise, and the sum of two Gaussians anywhere.
    centres=True: also the (x, y) of map 0's Gaussian per view."""
    h, w = CHAIN_SIZE
    rng = np.random.default_rng(7501)
    out = np.empty((len(CHAIN_PLAN), MAPS, h, w), dtype=np.float32)
    at = []
    for i in range(len(CHAIN_PLAN)):
        at.append((rng.uniform(8, w - 9), rng.uniform(8, h - 9)))
        out[i, 0] = gaussian(h, w, *at[-1])
        out[i, 1] = noise(rng, h, w)
        out[i, 2] = gaussian(h, w, rng.uniform(0, w - 1), rng.uniform(0, h - 1)) + gaussian(h, w, rng.uniform(0, w - 1), rng.uniform(0, h - 1))
    return (out, at) if centres else out


# ---- NaN and inf ------------------------------------------------------------------------------------------------------------------------
NAN_SIZE = (17, 23)
NAN_ANGLE = 30.0


def nan_map():
    h, w = NAN_SIZE
    m = noise(np.random.default_rng(7601), h, w)
    m[6, 9] = np.nan
    m[11, 15] = np.inf
    return m


# ---- whole RandAugment calls (K = 3) with the maps kept -----------------------------------------------------------------------------------
def call_cases():
    """RandAugment(3, magnitude, True, True, const)(image, heat-maps) per view under one seed: `views` images of h x w (augment_cases.image)
    and per view 2 maps of mh x mw.  Seeds under which views draw no, one and two rotations."""
    return OrderedDict(
        const_v8=dict(seed=123, const=True, magnitude=20, h=32, w=24, mh=16, mw=12, views=8),
        random_v8=dict(seed=146, const=False, magnitude=25, h=32, w=24, mh=16, mw=12, views=8),
    )


def call_images(c):
    import augment_cases

    return [augment_cases.image(c["h"], c["w"], c["seed"] * 10 + v) for v in range(c["views"])]


def call_maps(c):
    """(views, 2, mh, mw) float32: a Gaussian and noise per view."""
    rng = np.random.default_rng(c["seed"] + 5000)
    out = np.empty((c["views"], 2, c["mh"], c["mw"]), dtype=np.float32)
    for v in range(c["views"]):
        out[v, 0] = gaussian(c["mh"], c["mw"], rng.uniform(0, c["mw"] - 1), rng.uniform(0, c["mh"] - 1))
        out[v, 1] = noise(rng, c["mh"], c["mw"])
    return out


# ---- prepare_single_view(split="train") with the corrected Rotate ---------------------------------------------------------------------------
TRAIN_SEEDS = (303, 316)  # one rotation (by 22 degrees) in the first view's plan, two (24.9 and -21.1 degrees) in the second's


def train_cases():
    """A preprocess case (cases.preprocess_cases) plus the augmentation's settings; the seeds are ones under which the view's plan holds at
    least one effective rotation (rotate_targets.json records the count)."""
    return OrderedDict(
        inside=dict(seed=TRAIN_SEEDS[0], const=True, num_aug=2, magnitude=22),
        outside=dict(seed=TRAIN_SEEDS[1], const=False, num_aug=3, magnitude=30),
    )


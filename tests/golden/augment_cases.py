"""Case definitions of the RandAugment fixtures (tests/golden/augment.npz, augment.json): shared by the generator
(make_augment_golden.py), the GPU tests (tests/test_gpu_augment.py) and the host tests (tests/test_augment_host.py).
Inputs are regenerated from seeds on both sides; the fixtures hold expected outputs, op names and values only."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

# (H, W): odd tails; a plain size; 192 pixels (Equalize: step == 0); 384 pixels (Equalize: step == 1); nearly all border for Sharpness
SIZES = [(37, 50), (64, 48), (12, 16), (16, 24), (5, 4)]
CONST_VALUE = 77  # the constant channel of the "const" cases


def image(h, w, seed, const_channel=None):
    """Smooth-plus-noise (h, w, 3) uint8 image, built the way cases.preprocess_inputs builds its images (position 0 is what
    Pillow is handed as "R": the reference's image is BGR at that point, the ops only see positions)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 120 * np.sin(xx / 9.0 + seed), 127 + 120 * np.cos(yy / 7.0), (3 * xx + 5 * yy) % 256], -1)
    img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    if const_channel is not None:
        img[..., const_channel] = CONST_VALUE
    return np.ascontiguousarray(img)


def size_seed(h, w):
    return 1000 + h * 64 + w


def single_op_cases():
    """name -> (op name, value handed to the reference's op function, constant channel or None).  Rotate's value is the
    signed angle (the generator pins the reference's coin to "no flip")."""
    c = OrderedDict()
    c["invert"] = ("Invert", 0.0, None)
    c["autocontrast"] = ("AutoContrast", 0.0, None)
    c["equalize"] = ("Equalize", 0.0, None)
    for t in (0.0, 128.5, 256.0):
        c["solarize_%g" % t] = ("Solarize", t, None)
    for v in (0.0, 1.9, 4.0):
        c["posterize_%g" % v] = ("Posterize", v, None)
    for op in ("Brightness", "Contrast", "Color", "Sharpness"):
        for f in (0.1, 0.52, 1.0, 1.3, 1.9):
            c["%s_%g" % (op.lower(), f)] = (op, f, None)
    for i, a in enumerate((0.0, -0.0, 7.0, -7.0, 30.0, -30.0)):
        c["rotate_%d" % i] = ("Rotate", a, None)
    c["autocontrast_const"] = ("AutoContrast", 0.0, 1)
    c["equalize_const"] = ("Equalize", 0.0, 1)
    c["contrast_const_0.52"] = ("Contrast", 0.52, 1)
    c["contrast_const_1.3"] = ("Contrast", 1.3, 1)
    return c


def sequence_cases():
    """Whole RandAugment calls: K = 3, V views drawn one after the other under one seed."""
    return OrderedDict(
        const_v8=dict(seed=101, const=True, magnitude=20, h=64, w=48, views=8),
        random_v8=dict(seed=102, const=False, magnitude=25, h=64, w=48, views=8),
        const_256=dict(seed=103, const=True, magnitude=12, h=256, w=256, views=1),
        random_256=dict(seed=104, const=False, magnitude=30, h=256, w=256, views=1),
    )


def sequence_images(c):
    return [image(c["h"], c["w"], c["seed"] * 10 + v) for v in range(c["views"])]


def draw_cases():
    """RandAugment.draw against the reference's random streams: both magnitude modes, with and without rotation / image ops."""
    c = OrderedDict()
    for const in (True, False):
        for rot, aug in ((True, True), (True, False), (False, True)):
            name = "%s_%s%s" % ("const" if const else "random", "r" if rot else "", "i" if aug else "")
            c[name] = dict(seed=200 + len(c), const=const, rotation=rot, image_aug=aug, num_aug=3, magnitude=17, views=6)
    return c


def train_cases():
    """prepare_single_view with split == "train": a preprocess case (cases.preprocess_cases) plus the augmentation's settings."""
    return OrderedDict(
        inside=dict(seed=301, const=True, num_aug=2, magnitude=22),
        outside=dict(seed=302, const=False, num_aug=3, magnitude=30),
    )

"""Host half of the device RandAugment (utils/augmentation.py), no GPU: ``draw`` picks what the reference's RandAugment picks under the
same seeds and leaves both random streams where the reference leaves them (tests/golden/augment.json, recorded from the real reference);
bad arguments raise; the fixtures regenerate from the installed Pillow."""
import json
import os
import random

import numpy as np
import pytest

import augment_cases

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(G, "augment.json")) as f:
        return json.load(f)


def _same_plan(plan, want):
    assert len(plan) == len(want)
    for got_view, want_view in zip(plan, want):
        assert [n for n, _ in got_view] == [n for n, _ in want_view]
        for (name, val), (_, wval) in zip(got_view, want_view):
            # the very float64, sign of a zero angle included
            assert np.float64(val).tobytes() == np.float64(wval).tobytes(), (name, val, wval)


@pytest.mark.parametrize("name", list(augment_cases.draw_cases()))
def test_draw_picks_what_the_reference_picks(meta, name):
    from multi_view_active_learning_amd.utils.augmentation import RandAugment

    c = augment_cases.draw_cases()[name]
    want = meta["draws"][name]
    ra = RandAugment(c["num_aug"], c["magnitude"], c["rotation"], c["image_aug"], c["const"])
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    plan = ra.draw(c["views"])
    _same_plan(plan, want["ops"])
    assert random.random() == want["next_random"]
    assert float(np.random.rand()) == want["next_np"]
    names = {n for view in plan for n, _ in view}
    assert c["rotation"] or "Rotate" not in names
    assert c["image_aug"] or names <= {"Rotate"}


@pytest.mark.parametrize("name", list(augment_cases.sequence_cases()))
def test_draw_reproduces_the_sequence_fixtures(meta, name):
    """The plans the GPU tests replay from augment.json are what draw() gives under the fixture's seed."""
    from multi_view_active_learning_amd.utils.augmentation import RandAugment

    c = augment_cases.sequence_cases()[name]
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    _same_plan(RandAugment(3, c["magnitude"], True, True, c["const"]).draw(c["views"]), meta["sequences"][name])


def test_draw_view_by_view_equals_one_call():
    from multi_view_active_learning_amd.utils.augmentation import RandAugment

    ra = RandAugment(2, 21, True, True, False)
    random.seed(5)
    np.random.seed(5)
    whole = ra.draw(7)
    random.seed(5)
    np.random.seed(5)
    assert [ra.draw(1)[0] for _ in range(7)] == whole


def test_num_aug_zero_draws_nothing():
    from multi_view_active_learning_amd.utils.augmentation import RandAugment

    random.seed(1)
    want = random.random()
    random.seed(1)
    assert RandAugment(0, 0, True, True).draw(3) == [[], [], []]  # (config.py's defaults: NUM_AUG = 0)
    assert random.random() == want


def test_bad_arguments_raise():
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils import augmentation as aug

    for args in ((-1, 10, True, True), (1.5, 10, True, True), (True, 10, True, True), (2, 31, True, True), (2, -1, True, True),
                 (2, 10, False, False)):
        with pytest.raises(ValueError):
            aug.RandAugment(*args)
    ra = aug.RandAugment(2, 10, True, True)
    for n in (0, -3, 2.0, True):
        with pytest.raises(ValueError):
            ra.draw(n)
    for plan in ([], [[("Invert", 0.0)], []], [[("Flip", 0.0)]], [[("Rotate", 31.0)]], [[("Solarize", 257.0)]], [[("Color", 0.0)]],
                 [[("Sharpness", float("nan"))]]):
        with pytest.raises(ValueError):
            aug.plan_descriptors(plan, 8, 8)
    import torch

    with pytest.raises(_lib.MvalError):  # no CPU path
        aug.RandAugment.apply(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), [[("Invert", 0.0)]])


def test_plan_descriptors_layout_and_rotation_matrix():
    """[V][K] descriptors of 56 bytes (include/mval_hip.h: mval_aug_op); a zero angle of either sign becomes NONE; the matrix is Pillow's."""
    import ctypes
    import math

    from multi_view_active_learning_amd.utils import augmentation as aug

    assert ctypes.sizeof(aug._AugOp) == 56
    descs, masks = aug.plan_descriptors([[("Rotate", -0.0), ("Color", 0.52)], [("Rotate", -7.0), ("Equalize", 0.0)]], 12, 16)
    assert [d.kind for d in descs] == [aug.AUG_NONE, aug.AUG_COLOR, aug.AUG_ROTATE, aug.AUG_EQUALIZE]
    assert masks == [(1 << aug.AUG_NONE) | (1 << aug.AUG_ROTATE), (1 << aug.AUG_COLOR) | (1 << aug.AUG_EQUALIZE)]
    assert descs[1].p[0] == 0.52
    a = -math.radians(353.0)
    m = list(descs[2].p)
    assert m[0] == round(math.cos(a), 15) and m[1] == round(math.sin(a), 15) and m[3] == -m[1] and m[4] == m[0]
    assert m[2] == m[0] * -8.0 + m[1] * -6.0 + 0.0 + 8.0 and m[5] == m[3] * -8.0 + m[4] * -6.0 + 0.0 + 6.0


def test_header_kinds_match_the_python_mirror():
    import re

    from multi_view_active_learning_amd.utils import augmentation as aug

    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "mval_hip.h")).read()
    for name in ("NONE", "AUTOCONTRAST", "EQUALIZE", "INVERT", "POSTERIZE", "SOLARIZE", "COLOR", "CONTRAST", "BRIGHTNESS", "SHARPNESS", "ROTATE"):
        assert int(re.search(r"\bMVAL_AUG_%s\s*=\s*(\d+)" % name, text).group(1)) == getattr(aug, "AUG_" + name), name


# ---- the fixtures themselves ---------------------------------------------------------------------------------------------------
def _pillow_op(img, op, val):
    """The Pillow call behind each of the reference's op functions (dataset/augmentation.py), angle sign as given."""
    from PIL import Image, ImageEnhance, ImageOps

    im = Image.fromarray(img)
    if op == "Rotate":
        return im.rotate(val, resample=Image.BICUBIC)
    if op in ("AutoContrast", "Invert", "Equalize"):
        return getattr(ImageOps, op.lower())(im)
    if op == "Solarize":
        return ImageOps.solarize(im, val)
    if op == "Posterize":
        return ImageOps.posterize(im, max(1, int(val)))
    return getattr(ImageEnhance, op)(im).enhance(val)


def test_single_op_fixtures_regenerate_from_the_installed_pillow(meta):
    import PIL

    assert PIL.__version__ == meta["pillow"], "tests/golden/augment.npz was recorded with Pillow %s" % meta["pillow"]
    z = np.load(os.path.join(G, "augment.npz"))
    for (h, w) in augment_cases.SIZES:
        for name, (op, val, const) in augment_cases.single_op_cases().items():
            img = augment_cases.image(h, w, augment_cases.size_seed(h, w), const)
            np.testing.assert_array_equal(np.asarray(_pillow_op(img, op, val)), z["%dx%d/%s" % (h, w, name)], err_msg="%dx%d/%s" % (h, w, name))


def test_fixture_is_no_larger_than_the_largest_other_fixture():
    sizes = {f: os.path.getsize(os.path.join(G, f)) for f in os.listdir(G) if f.endswith(".npz")}
    assert sizes["augment.npz"] <= max(v for f, v in sizes.items() if f != "augment.npz")
    assert sizes["augment.npz"] <= 1 << 20


def test_equalize_fixtures_reach_the_branches_they_are_sized_for():
    """12 x 16: step == 0 on every channel; 16 x 24: step == 1; the larger sizes: step > 1; the constant channel: one bin."""
    def steps(img):
        out = []
        for c in range(3):
            h = np.bincount(img[..., c].ravel(), minlength=256)
            nz = h[h > 0]
            out.append(None if len(nz) <= 1 else int((nz.sum() - nz[-1]) // 255))
        return out

    assert steps(augment_cases.image(12, 16, augment_cases.size_seed(12, 16))) == [0, 0, 0]
    assert steps(augment_cases.image(16, 24, augment_cases.size_seed(16, 24))) == [1, 1, 1]
    assert min(steps(augment_cases.image(37, 50, augment_cases.size_seed(37, 50)))) > 1
    assert steps(augment_cases.image(64, 48, augment_cases.size_seed(64, 48), 1))[1] is None


@pytest.mark.reference
def test_fixtures_regenerate_from_the_reference(meta):
    """Everything in augment.npz / augment.json again from the real reference and the installed Pillow: identical."""
    import make_augment_golden as mk

    out, got_meta = mk.build()
    assert mk.meta_text(got_meta) == open(os.path.join(G, "augment.json")).read()
    z = np.load(os.path.join(G, "augment.npz"))
    assert sorted(z.files) == sorted(out)
    for k, a in out.items():
        assert z[k].dtype == a.dtype and z[k].shape == a.shape, k
        np.testing.assert_array_equal(z[k], a, err_msg=k)

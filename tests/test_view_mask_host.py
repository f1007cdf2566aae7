"""Host tests (no GPU) of the missing-view support: the pair tables ``draw_view_pairs(..., view_valid=)`` builds per frame
from its present views -- against the tables and RNG digests the real reference left when it was handed each frame's
present views alone (tests/golden/view_mask.npz, make_view_mask_golden.py) --, the padding and width rules, the unchanged
unmasked draw, and the new entries in the header and the library."""
import ctypes
import itertools
import os
import random
import re

import numpy as np
import pytest
import torch

import many_view_cases as mv
import view_mask_cases as vm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
NPZ = os.path.join(G, "view_mask.npz")
NEW_ENTRIES = ("mval_triangulate_ransac_masked", "mval_triangulate_ransac_pairs_masked", "mval_reprojection_xe_masked",
               "mval_score_reduce_masked", "mval_peak_mask")


def _valid(c):
    valid = np.ones((c["b"], c["j"]), dtype=bool)
    valid[:, list(c["invalid"])] = False
    valid[list(c["no_valid_joint"])] = False
    return valid


@pytest.mark.parametrize("name", list(vm.view_mask_cases()))
def test_masked_draw_reproduces_the_reference_tables(name):
    """Frame by frame (the digest after EVERY frame is the reference's) and for the whole batch at once: the same table,
    the same final RNG state.  A frame that draws nothing leaves the state alone."""
    from multi_view_active_learning_amd.utils.triangulation import PAIR_PAD, draw_view_pairs

    c = vm.view_mask_cases()[name]
    z = vm.load_golden(NPZ, name)
    valid, vv = _valid(c), vm.view_valid(c)
    assert PAIR_PAD == vm.PAD == 255
    random.seed(int(z["rseed"]))
    tab = draw_view_pairs(valid, c["v"], c["n_iters"], random, view_valid=vv)
    assert tab.dtype == np.uint8 and tab.shape == z["pairs"].shape == (c["b"], c["j"], vm.n_pairs(c), 2)
    np.testing.assert_array_equal(tab, z["pairs"])
    assert vm.state_digest(random.getstate()) == str(z["frame_digests"][-1])
    random.seed(int(z["rseed"]))
    for b in range(c["b"]):
        before = random.getstate()
        one = draw_view_pairs(valid[b : b + 1], c["v"], c["n_iters"], random, view_valid=vv[b : b + 1])
        assert vm.state_digest(random.getstate()) == str(z["frame_digests"][b])
        if not vm.draws(c)[b]:
            assert random.getstate() == before
        np.testing.assert_array_equal(one[0], z["pairs"][b, :, : one.shape[2]])
        assert (z["pairs"][b, :, one.shape[2] :] == 255).all()


def test_padding_and_width_rules():
    """P = max over frames of min(C(n_b, 2), n_iters), at least 1; a row shorter than P ends in entries naming view 255;
    a frame with fewer than two present views draws nothing and is all padding; torch masks and 0/1 numbers work."""
    from multi_view_active_learning_amd.utils.triangulation import draw_view_pairs

    vv = np.array([[1, 1, 1, 1, 1], [0, 1, 0, 1, 1], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]], dtype=np.float32)
    valid = np.ones((4, 3), dtype=bool)
    valid[0, 1] = False

    class NoDraw:
        def shuffle(self, x):
            raise AssertionError("nothing is drawn when all pairs fit")

    tab = draw_view_pairs(torch.from_numpy(valid), 5, 64, NoDraw(), view_valid=torch.from_numpy(vv))
    assert tab.shape == (4, 3, 10, 2)
    lex5 = np.array(list(itertools.combinations(range(5), 2)), np.uint8)
    for j in range(3):  # (all pairs fit: every joint's row is the list, valid or not, as without a mask)
        np.testing.assert_array_equal(tab[0, j], lex5)
        np.testing.assert_array_equal(tab[1, j, :3], [(1, 3), (1, 4), (3, 4)])
    assert (tab[1, :, 3:] == 255).all() and (tab[2:] == 255).all()
    # n_iters below every frame's pair count: P = n_iters, every valid row drawn, invalid rows zero
    rng = random.Random(5)
    tab = draw_view_pairs(valid[:2], 5, 2, rng, view_valid=vv[:2])
    assert tab.shape == (2, 3, 2, 2) and not tab[0, 1].any()
    ref = random.Random(5)
    for b, n, present in ((0, 10, [0, 1, 2, 3, 4]), (1, 3, [1, 3, 4])):
        lex = list(itertools.combinations(present, 2))
        for j in np.flatnonzero(valid[b]):
            order = list(range(n))
            ref.shuffle(order)
            np.testing.assert_array_equal(tab[b, j], [lex[k] for k in order[:2]])
    assert rng.getstate() == ref.getstate()
    # no frame with two present views: P is still 1
    assert draw_view_pairs(valid[2:], 5, 64, NoDraw(), view_valid=vv[2:]).shape == (2, 3, 1, 2)


def test_unmasked_draw_is_unchanged():
    """view_valid=None: the tables and the RNG state of the many-view goldens (the reference's own draws), the shared
    lexicographic list when all pairs fit, zero rows for invalid joints -- no padding, P = min(n_iters, C(V,2))."""
    from multi_view_active_learning_amd.utils.triangulation import draw_view_pairs

    many = os.path.join(G, "triangulation_many_views.npz")
    for name in ("v4_n3", "v12_frames", "v16_n100"):
        c = mv.many_view_cases()[name]
        z = mv.load_golden(many, name)
        valid = np.ones((c["b"], c["j"]), dtype=bool)
        valid[:, list(c["invalid"])] = False
        random.seed(int(z["rseed"]))
        tab = draw_view_pairs(valid, c["v"], c["n_iters"], random, view_valid=None)
        np.testing.assert_array_equal(tab, z["pairs"])
        assert mv.state_digest(random.getstate()) == str(z["state_digest"])
        random.seed(int(z["rseed"]))
        np.testing.assert_array_equal(draw_view_pairs(valid, c["v"], c["n_iters"], random), tab)
    state = random.getstate()
    tab = draw_view_pairs(np.ones((2, 3)), 12, 128, random, None)
    assert random.getstate() == state and tab.shape == (2, 3, 66, 2)
    np.testing.assert_array_equal(tab[1, 2], list(itertools.combinations(range(12), 2)))


def test_new_entries_are_declared_and_exported():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    hdr = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(mval_[a-z0-9_]+)\s*\(", hdr))
    for n in NEW_ENTRIES:
        assert n in names, n + " is not declared in include/mval_hip.h"
        assert hasattr(_lib.lib(), n), n + " is not exported"
        f = _lib._views_entry(n)
        assert f.restype is ctypes.c_int and len(f.argtypes) == len(_lib._VIEWS_ARGTYPES[n])
        # the declaration's parameter count is the mirror's
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1)
        assert len(decl.split(",")) == len(f.argtypes), n


def test_stage_batch_and_wrappers_know_the_mask():
    """_stage_batch treats view_valid as it treats joint_valid; the public calls take the keyword."""
    import inspect

    from multi_view_active_learning_amd import strategy
    from multi_view_active_learning_amd.utils import triangulation

    assert "view_valid" in strategy._SMALL_KEYS
    for fn, kws in ((triangulation.triangulate_batch, ("view_valid", "view_valid_host")), (triangulation.triangulation, ("view_valid",)),
                    (triangulation.draw_view_pairs, ("view_valid",)), (strategy.score_heatmaps_batch, ("view_valid",)),
                    (strategy.score_decode_heatmaps_batch, ("view_valid",)), (strategy.score_decode_heatmaps_all, ("view_valid",))):
        params = inspect.signature(fn).parameters
        for kw in kws:
            assert kw in params and params[kw].default is None, (fn.__name__, kw)

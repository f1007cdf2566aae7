"""Host tests (no GPU) of the flip test: the config fields and their validator, the pair tables, the numpy oracle's
own identity, the two entries in the header and the library with their argument checks, and that the passes hand the mode on --
never under the default configuration."""
import os
import re

import numpy as np
import pytest
import torch

import flip_oracle as fo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- config --------------------------------------------------------------------------------------------------------------------
def test_config_fields_and_check():
    from multi_view_active_learning_amd.config import FLIP_TESTS, check_flip_test, get_default_configs
    from multi_view_active_learning_amd.utils import flip_test

    cfg = get_default_configs()
    assert cfg.AL.FLIP_TEST == "none" and cfg.EVAL.FLIP_TEST == "none" and list(cfg.DATA.FLIP_PAIRS) == []
    assert FLIP_TESTS == flip_test.FLIP_TESTS == ("none", "mirror", "mirror_shift")
    for mode in FLIP_TESTS:
        assert check_flip_test(mode) == mode
    for bad in ("MIRROR", "flip", "", None, True, 1, ["mirror"]):
        with pytest.raises(ValueError, match="'none', 'mirror', 'mirror_shift'"):
            check_flip_test(bad)


def _data(kind="panoptic", j=19, pairs=()):
    from multi_view_active_learning_amd.config import get_default_configs

    d = get_default_configs().DATA
    d.TYPE, d.NUM_JOINTS, d.FLIP_PAIRS = kind, j, [list(p) for p in pairs]
    return d


def _is_involution(table, j):
    return len(table) == j and sorted(table) == list(range(j)) and all(table[table[i]] == i for i in range(j))


def test_default_pairs_are_involutions():
    from multi_view_active_learning_amd.utils.flip_test import flip_pairs

    pan = flip_pairs(_data())
    assert _is_involution(pan, 19)
    assert [i for i in range(19) if pan[i] == i] == [0, 1, 2]  # neck, nose, body centre (joint_root_index 2)
    assert (pan[3], pan[8], pan[14], pan[15], pan[18]) == (9, 14, 8, 17, 16)
    ih = flip_pairs(_data("ih26m", 42))
    assert _is_involution(ih, 42) and ih == list(range(21, 42)) + list(range(21))


def test_given_pairs_accept_and_reject():
    from multi_view_active_learning_amd.utils.flip_test import check_pairs, flip_pairs

    assert flip_pairs(_data("other", 5, [(0, 3), (4, 1)])) == [3, 4, 2, 0, 1]  # (joints not named map to themselves)
    assert flip_pairs(_data("panoptic", 4, [(1, 2)])) == [0, 2, 1, 3]  # (given pairs: the default of TYPE is not consulted)
    assert flip_pairs(_data("other", 3, [(1, 1)])) == [0, 1, 2]
    with pytest.raises(ValueError, match="outside 0..4"):  # out of range
        flip_pairs(_data("other", 5, [(0, 5)]))
    with pytest.raises(ValueError, match="outside 0..4"):
        flip_pairs(_data("other", 5, [(-1, 2)]))
    with pytest.raises(ValueError, match="another pair"):  # overlap
        flip_pairs(_data("other", 5, [(0, 1), (1, 2)]))
    with pytest.raises(ValueError, match="not a pair"):
        flip_pairs(_data("other", 5, [(0, 1, 2)]))
    with pytest.raises(ValueError, match="19 joints"):  # wrong length: the default table against another NUM_JOINTS
        flip_pairs(_data("panoptic", 17))
    with pytest.raises(ValueError, match="no default"):
        flip_pairs(_data("other", 5))
    assert check_pairs([1, 0, 2], 3) == [1, 0, 2]
    with pytest.raises(ValueError, match="own inverse"):  # a permutation, but a 3-cycle
        check_pairs([1, 2, 0], 3)
    with pytest.raises(ValueError, match="own inverse"):  # not a permutation
        check_pairs([1, 1, 2], 3)
    with pytest.raises(ValueError, match="outside 0..2"):
        check_pairs([0, 1, 3], 3)
    with pytest.raises(ValueError, match="2 entries for 3 joints"):
        check_pairs([1, 0], 3)


def test_merge_rejects_none_and_unknown_modes():
    from multi_view_active_learning_amd.utils.flip_test import flip_test_heatmaps, merge_flipped

    hm = torch.zeros(1, 2, 3, 4)
    for f in (lambda m: merge_flipped(hm, hm, [0, 1], m), lambda m: flip_test_heatmaps(None, hm, [0, 1], m)):
        with pytest.raises(ValueError, match="merges nothing"):
            f("none")
        with pytest.raises(ValueError, match="accepted are"):
            f("shift")


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def test_oracle_known_answers():
    x = np.arange(12, dtype=np.float32).reshape(1, 2, 2, 3)
    np.testing.assert_array_equal(fo.mirror(x)[0, 0], [[2, 1, 0], [5, 4, 3]])
    a = np.zeros((1, 2, 1, 4), np.float32)
    b = np.array([[[[1, 2, 3, 4]], [[10, 20, 30, 40]]]], np.float32)
    np.testing.assert_array_equal(fo.merge(a, b, [1, 0], 0)[0, :, 0], [[20, 15, 10, 5], [2, 1.5, 1, 0.5]])
    np.testing.assert_array_equal(fo.merge(a, b, [0, 1], 1)[0, :, 0], [[2, 2, 1.5, 1], [20, 20, 15, 10]])  # column 0 keeps its own value
    one = np.array([[[[3.0], [5.0]]]], np.float32)  # a one-column map: the shift changes nothing
    np.testing.assert_array_equal(fo.merge(one, one, [0], 1), one)
    assert fo.first_argmax(np.array([[1.0, 7.0], [7.0, 2.0]], np.float32)) == 1
    assert fo.first_argmax(np.array([1.0, np.inf, np.nan, np.nan], np.float32)) == 2
    assert fo.first_argmax(np.array([0.0, -0.0, 0.0], np.float32)) == 0 and fo.first_argmax(np.full(5, -np.inf, np.float32)) == 0


def test_oracle_identity_mirrored_batch():
    """For shift == 0, merge(B, A)[j] == mirror(merge(A, B)[pairs[j]]) bit for bit (float32 addition commutes): the merged maps of
    the mirrored batch are the mirrored, pair-swapped merged maps of the batch."""
    rng = np.random.default_rng(5)
    pairs = [2, 1, 0, 4, 3]
    a, b = (rng.standard_normal((3, 5, 6, 7)).astype(np.float32) for _ in range(2))
    a[0, 1, 2, 3] = np.nan
    fwd, back = fo.merge(a, b, pairs, 0), fo.merge(b, a, pairs, 0)
    np.testing.assert_array_equal(back.view(np.int32), fo.mirror(fwd[:, pairs]).view(np.int32))
    assert not np.array_equal(fo.merge(b, a, pairs, 1).view(np.int32), fo.mirror(fo.merge(a, b, pairs, 1)[:, pairs]).view(np.int32))


# ---- the entries ---------------------------------------------------------------------------------------------------------------
def _lib_built():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib


def test_entries_are_declared_and_exported():
    _lib = _lib_built()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mval_hip.h")).read(), flags=re.S)
    want = {
        "mval_mirror_images": ["const float* in", "float* out", "int64_t n_rows", "int W", "void* stream"],
        "mval_flip_merge_heatmaps": ["const float* hm", "const float* hm_mirrored", "const int32_t* pairs", "int shift", "float* merged",
                                     "uint64_t* argmax_keys", "int64_t N", "int J", "int hh", "int wh", "void* stream"],
    }
    for name, args in want.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert decl, name + " is not declared in include/mval_hip.h"
        assert [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")] == args
        assert hasattr(_lib.lib(), name), name + " is not exported"
        assert len(_lib._VIEWS_ARGTYPES[name]) == len(args)


def test_entries_reject_bad_arguments_without_a_launch():
    """Aliased outputs, NULL arrays and bad dimensions are errors before anything touches a device; N = 0 / n_rows = 0 return 0
    before any pointer check."""
    _lib = _lib_built()
    mirror, merge = _lib._views_entry("mval_mirror_images"), _lib._views_entry("mval_flip_merge_heatmaps")
    err = lambda: _lib.lib().mval_last_error().decode()  # noqa: E731
    # (the addresses are never dereferenced: every call below fails its checks or is the empty no-op)
    assert mirror(0, 0, 0, 5, None) == 0
    assert mirror(0x1000, 0x9000, 4, 0, None) == -1 and "bad dims" in err()
    assert mirror(0x1000, 0x9000, -1, 4, None) == -1 and "bad dims" in err()
    assert mirror(0, 0x9000, 4, 4, None) == -1 and "NULL" in err()
    assert mirror(0x1000, 0x1000, 4, 4, None) == -1 and "alias" in err()
    assert mirror(0x1000, 0x1000 + 4 * 15, 4, 4, None) == -1 and "alias" in err()  # (the last element overlaps)
    assert mirror(0x1000 + 4 * 15, 0x1000, 4, 4, None) == -1 and "alias" in err()

    def call(hm=0x10000, hmm=0x20000, pairs=0x30000, merged=0x40000, keys=0x50000, n=2, j=3, hh=4, wh=5):
        return merge(hm, hmm, pairs, 0, merged, keys, n, j, hh, wh, None)

    assert call(hm=0, hmm=0, pairs=0, merged=0, keys=0, n=0) == 0
    assert call(n=0, j=0) == -1 and "bad dims" in err()  # (J >= 1 holds for an empty batch too)
    for bad in (dict(j=0), dict(hh=0), dict(wh=0), dict(n=-1), dict(hh=4096, wh=4096)):
        assert call(**bad) == -1 and "bad dims" in err(), bad
    for null in ("hm", "hmm", "pairs", "merged"):
        assert call(**{null: 0}) == -1 and "NULL" in err(), null
    size = 2 * 3 * 4 * 5 * 4
    assert call(merged=0x10000) == -1 and "alias" in err()
    assert call(merged=0x20000) == -1 and "alias" in err()
    assert call(merged=0x10000 + size - 4) == -1 and "alias" in err()
    assert call(merged=0x20000 - size + 4) == -1 and "alias" in err()
    assert call(keys=0x50004) == -1 and "aligned" in err()
    assert call(n=1 << 30, j=4, hmm=0x10000) == -1 and "too many maps" in err()


def test_wrappers_need_device_tensors():
    _lib = _lib_built()
    with pytest.raises(_lib.MvalError, match="HIP device"):
        _lib.mirror_images(torch.zeros(2, 3))
    with pytest.raises(_lib.MvalError, match="one shape"):
        _lib.flip_merge_heatmaps(torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3, 5), torch.zeros(2, dtype=torch.int32), 0)
    with pytest.raises(_lib.MvalError, match=r"pairs must be \(2,\)"):
        _lib.flip_merge_heatmaps(torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3, 4), torch.zeros(3, dtype=torch.int32), 0)


# ---- the passes ----------------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, loader, model, body, inputs=None, stage=None, **kw):
        self.calls.append(kw)
        return []


@pytest.mark.parametrize("node", ["AL", "EVAL"])
def test_passes_hand_the_mode_on(monkeypatch, node):
    """The scoring passes read AL.FLIP_TEST, the evaluation passes EVAL.FLIP_TEST, once per pass; under "none" (or a config without
    the field) the pool loop is called exactly as before, and the CLUSTER pass never flips."""
    from multi_view_active_learning_amd import strategy
    from multi_view_active_learning_amd.config import get_default_configs

    cfg = get_default_configs()
    monkeypatch.setattr("multi_view_active_learning_amd.parallel.all_gather_reference_order", lambda local, sizes: local)
    monkeypatch.setattr(strategy._lib, "mkpe", lambda pred, gt, valid, n, jj, rows: (torch.zeros(()), None))
    for figure in ("compute_pckh_figure", "compute_3d_pck_figure", "compute_3d_pckh_figure"):
        monkeypatch.setattr(strategy.evaluation, figure, lambda *a: (None, None))

    def passes(st):
        rec = _Recorder()
        monkeypatch.setattr(st, "_pool_loop", rec)
        st._compute_sal_dict([], None)
        st._compute_sal_dicts([], None, ("HP", "MPE"))
        n_al = len(rec.calls)
        st.evaluate_mkpe([], None)
        st.evaluate_2d_pckh([], None)
        st.evaluate([], None, metric="MKPE")
        st.evaluate_all([], None)
        return rec.calls[:n_al], rec.calls[n_al:]

    al, ev = passes(strategy.ActiveLearningStrategy(cfg))
    assert len(al) == 2 and len(ev) == 4 and all(kw == {} for kw in al + ev)
    getattr(cfg, node).FLIP_TEST = "mirror_shift"
    al, ev = passes(strategy.ActiveLearningStrategy(cfg))
    flipped, plain = (al, ev) if node == "AL" else (ev, al)
    assert all(kw == {"flip": "mirror_shift"} for kw in flipped) and all(kw == {} for kw in plain)
    del getattr(cfg, node)["FLIP_TEST"]  # (a config from before the field)
    al, ev = passes(strategy.ActiveLearningStrategy(cfg))
    assert all(kw == {} for kw in al + ev)
    getattr(cfg, node).FLIP_TEST = "both"
    st = strategy.ActiveLearningStrategy(cfg)
    with pytest.raises(ValueError, match="accepted are"):
        (st._compute_sal_dict if node == "AL" else st.evaluate_mkpe)([], None)
    getattr(cfg, node).FLIP_TEST = "mirror"
    cfg.DATA.FLIP_PAIRS = [[0, 1], [1, 2]]
    st = strategy.ActiveLearningStrategy(cfg)
    with pytest.raises(ValueError, match="another pair"):  # (before the pass starts)
        (st._compute_sal_dict if node == "AL" else st.evaluate_mkpe)([], None)


def test_pool_loop_picks_the_forward_once(monkeypatch):
    """``_pool_loop`` under "none" calls ``_compute_batch_heatmap`` and never ``_compute_batch_heatmap_flip``; under a mode it is
    the other way round, with the mode handed on."""
    from multi_view_active_learning_amd import strategy
    from multi_view_active_learning_amd.config import get_default_configs

    st = strategy.ActiveLearningStrategy(get_default_configs())
    seen = []
    monkeypatch.setattr(st, "_compute_batch_heatmap", lambda pe, dp: seen.append(("plain",)) or "hm")
    monkeypatch.setattr(st, "_compute_batch_heatmap_flip", lambda pe, dp, mode: seen.append(("flip", mode)) or "hm")
    loader = [{"k": 1}, {"k": 2}]
    ident = lambda dp: dp  # noqa: E731
    assert st._pool_loop(loader, None, lambda hm, dp: (hm, dp["k"]), inputs=lambda hm, dp: (hm, dp), stage=ident) == [("hm", 1), ("hm", 2)]
    assert seen == [("plain",)] * 2
    del seen[:]
    st._pool_loop(loader, None, lambda hm, dp: 0, inputs=lambda hm, dp: (hm, dp), stage=ident, flip="mirror")
    assert seen == [("flip", "mirror")] * 2

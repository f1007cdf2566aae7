"""CPU (no GPU): the host side of the multi-strategy scoring pass -- the C entry's symbol, declaration and argument
checks (mval_score_decode_maps_all), the slicing of the widened per-rank tables into one ``tables_to_sal_dict`` table
per strategy, and the validation of the strategy list."""
import ctypes
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_symbol_is_exported_and_declared(lib):
    assert hasattr(lib, "mval_score_decode_maps_all")
    with open(os.path.join(REPO, "include", "mval_hip.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert ("int mval_score_decode_maps_all(const float* heatmaps, const uint8_t* valid, float* stat, int32_t* n_peaks, "
            "int64_t* kp2d, int B, int V, int J, int hh, int wh, int stride, int split_width, void* stream);") in header
    from multi_view_active_learning_amd import _lib

    assert callable(_lib.score_decode_maps_all)


def _call(lib, hm=1, stat=1, cnt=1, kp=1, b=1, v=2, j=3, hh=8, wh=8, stride=4, split=8):
    """(The pointers are never dereferenced: every call here fails a check that comes before any launch.)"""
    p = lambda x: ctypes.c_void_p(0x1000 * x)  # noqa: E731
    return lib.mval_score_decode_maps_all(p(hm), ctypes.c_void_p(0), p(stat), p(cnt), p(kp), ctypes.c_int(b), ctypes.c_int(v),
                                          ctypes.c_int(j), ctypes.c_int(hh), ctypes.c_int(wh), ctypes.c_int(stride),
                                          ctypes.c_int(split), ctypes.c_void_p(0))


@pytest.mark.parametrize("bad, word", [
    (dict(b=-1), "bad dims"), (dict(v=0), "bad dims"), (dict(j=0), "bad dims"), (dict(hh=0), "bad dims"), (dict(wh=-3), "bad dims"),
    (dict(split=0), "split_width"), (dict(stat=0), "must not be NULL"), (dict(cnt=0), "must not be NULL"),
    (dict(hm=0), "must not be NULL"),
    (dict(hh=300, wh=300), "heat-map 300x300 does not fit LDS"),  # (the size check precedes the launch as well)
], ids=lambda x: "-".join("%s=%s" % kv for kv in x.items()) if isinstance(x, dict) else None)
def test_argument_checks_leave_a_message_and_launch_nothing(lib, bad, word):
    lib.mval_last_error.restype = ctypes.c_char_p
    assert _call(lib, **bad) == -1
    msg = lib.mval_last_error().decode()
    assert "mval_score_decode_maps_all" in msg and word in msg, msg


def test_split_width_is_ignored_without_decode_and_an_empty_batch_is_a_no_op(lib):
    assert _call(lib, b=0) == 0             # no map: nothing to launch
    assert _call(lib, b=0, kp=0, split=0) == 0  # kp2d NULL: split_width is not looked at


# ---- table slicing --------------------------------------------------------------------------------------------------
def _rank_tables(strategies, sizes_per_rank, j, seed):
    """Hand-made widened per-rank tables (6 + 3J + E columns) and, per strategy, the 6 + 3J tables a single-strategy pass
    would have gathered: the same base columns with that strategy's al_metric in column 2."""
    rng = np.random.default_rng(seed)
    wide, single = [], {s: [] for s in strategies}
    for r, sizes in enumerate(sizes_per_rank):
        n = sum(sizes)
        base = rng.standard_normal((n, 6 + 3 * j))
        base[:, 0] = r            # pose
        base[:, 1] = np.arange(n)  # frame_id: guids "<rank>-<row>" are unique
        if n:
            base[0, 5] = np.nan   # a NaN mkpe travels through
        al = rng.standard_normal((n, len(strategies)))
        w = base.copy()
        w[:, 2] = 0.0
        wide.append(np.concatenate([w, al], axis=1))
        for e, s in enumerate(strategies):
            t = base.copy()
            t[:, 2] = al[:, e]
            single[s].append(t)
    return wide, single


def _same(a, b):
    assert list(a) == list(b)
    for field in a:
        assert list(a[field]) == list(b[field]), field  # key order
        for g in a[field]:
            np.testing.assert_array_equal(np.asarray(a[field][g]), np.asarray(b[field][g]))  # (NaN == NaN here)


@pytest.mark.parametrize("sizes_per_rank", [
    [[2, 2, 1]],                        # one rank, a short last batch
    [[2, 2], [2, 1]],                   # a short last batch on rank 1
    [[3, 3, 2], [3, 3], [3, 1], []],    # ragged shards, one of them empty
], ids=["1rank", "2ranks", "4ranks_ragged"])
def test_each_slice_gives_the_single_strategy_sal_dict(sizes_per_rank):
    from multi_view_active_learning_amd.strategy import split_strategy_tables, tables_to_sal_dict

    strategies = ("HP", "MPE", "BSB", "TRIANGULATION", "CORESET", "RANDOM")
    j = 5
    wide, single = _rank_tables(strategies, sizes_per_rank, j, seed=len(sizes_per_rank))
    keep = [w.copy() for w in wide]
    split = split_strategy_tables(wide, len(strategies))
    assert len(split) == len(strategies)
    for w, k in zip(wide, keep):
        np.testing.assert_array_equal(w, k)  # the gathered tables are left as they were
    for s, tabs in zip(strategies, split):
        assert [t.shape for t in tabs] == [(sum(b), 6 + 3 * j) for b in sizes_per_rank]
        _same(tables_to_sal_dict(tabs, sizes_per_rank), tables_to_sal_dict(single[s], sizes_per_rank))
    # one strategy: the extra column simply moves into column 2
    one = split_strategy_tables([np.concatenate([w[:, : 6 + 3 * j], w[:, 6 + 3 * j + 2 : 6 + 3 * j + 3]], axis=1) for w in wide], 1)
    _same(tables_to_sal_dict(one[0], sizes_per_rank), tables_to_sal_dict(single["BSB"], sizes_per_rank))


def test_slicing_refuses_a_table_of_the_wrong_width():
    from multi_view_active_learning_amd.strategy import split_strategy_tables

    with pytest.raises(ValueError):
        split_strategy_tables([np.zeros((2, 6 + 3 * 5 + 2))], 3)  # 6 + 3J + E with E = 2, asked for 3
    with pytest.raises(ValueError):
        split_strategy_tables([np.zeros((2, 7))], 3)


# ---- strategy names -------------------------------------------------------------------------------------------------
def test_strategy_list_validation():
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import AL_STRATEGIES, ActiveLearningStrategy, check_strategies

    assert AL_STRATEGIES == ("HP", "MPE", "BSB", "TRIANGULATION", "CORESET", "RANDOM")
    assert check_strategies(["BSB", "HP"]) == ("BSB", "HP")  # the order given is kept
    assert check_strategies(iter(AL_STRATEGIES)) == AL_STRATEGIES
    st = ActiveLearningStrategy(get_default_configs())
    for bad, err in ((("HP", "ENTROPY"), NotImplementedError), (("hp",), NotImplementedError), (("HP", "MPE", "HP"), ValueError),
                     ((), ValueError), ([], ValueError)):
        with pytest.raises(err):
            check_strategies(bad)
        with pytest.raises(err):  # the pass checks its list before it touches the loader or the model
            st._compute_sal_dicts(None, None, bad)


def test_an_empty_loader_gives_empty_dicts_per_strategy():
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    st = ActiveLearningStrategy(get_default_configs())
    got = st._compute_sal_dicts([], None, ("MPE", "RANDOM"))
    assert isinstance(got, OrderedDict) and list(got) == ["MPE", "RANDOM"]
    assert got["MPE"] == st._compute_sal_dict([], None)
    assert got["MPE"] is not got["RANDOM"]

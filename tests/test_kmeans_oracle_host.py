"""CPU (no GPU): the KMeans restatement tests/kmeans_oracle.py against the real scikit-learn on every case of
tests/golden/kmeans_edge_cases.py, the conditions the cases must meet so that an exact comparison is fair, and that
each case reaches the branch it is named for.  tests/test_gpu_kmeans_edges.py then holds csrc/kmeans.hip against the
same oracle.  Nothing is stored: inputs come from seeds, expectations from the oracle, so there is nothing to regenerate.

Path of csrc/kmeans.hip -> case(s) -> the assertion here that proves the case gets there:

  more than 256 workgroups (km_pp_search, km_finish, block search)  seed_n65541_*   test_seeding_case_reaches_its_branch:
                                                    blocks > 256 and a pick in block 256
  K tail of 3 / K = 1, 2, 65, 256                    shape_k3_*, shape_k7_*, limit_k15_*, shape_k1/k2/k65/k256   the table's K
  D = 1, 2, 257, 512 (second trip of the D loops)    shape_*_d1/d2/d257/d512, reloc_two_empty_n200_d300          the table's D
  K*D in (3774, 3840]                                limit_*          test_shape_case_reaches_its_branch: LDS > 64 KiB
  target 0 / on a prefix sum / one ulp above / flat run / clip; first or last row of a workgroup; blocks 63, 64
                                                     seed_*           test_seeding_case_reaches_its_branch: the oracle's picks
                                                    and candidates are the rows seeding_uniforms aimed at
  two candidates tie in potential, the first wins    seed_dup_candidates_first_wins   same test: pot_gap == 0, pick == row 20
  n = K, 255, 256, 257, 256 k + 1; first_idx 0, n-1  shape_n_equals_k, seed_n*_first0 / _firstlast   same test
  relocation: two empty / far rows beyond 256 / tie / same old cluster / only member -> fallback
                                                     reloc_*          test_relocation_case_reaches_its_branch
  max_iter 1, 15, 16, 17, 32, 33; natural end at 15, 16, 17, 33; tol = 0; end by tol with labels changing
                                                     end_*            test_ending_case_reaches_its_branch
  C-ABI refusals, workspace + 8 bytes, side stream, reused workspace, the KMeans class: tests/test_gpu_kmeans_edges.py only
"""
import warnings

import numpy as np
import pytest

import kmeans_edge_cases as ec

NAMES = list(ec.cases())
SEEDED = [n for n in NAMES if ec.cases()[n]["kind"] in ("seeding", "shape")]
MIN_GAP = 1e-9  # a reordered float64 sum moves the compared values by about 1e-13


class _Replay:
    """A RandomState stand-in that hands _kmeans_plusplus the first index and the uniforms of a case."""

    def __init__(self, first, rand_u, trials):
        self.first, self.u, self.trials, self.at = first, np.asarray(rand_u, dtype=np.float64), trials, 0

    def choice(self, n, p=None):
        return self.first

    def uniform(self, size=None):
        assert size == self.trials
        out = self.u[self.at:self.at + size]
        self.at += size
        return out


def _inertia_close(got, want, x, rel=1e-10):
    floor = 1e-20 * x.shape[0] * float(np.abs(x).max()) ** 2
    return abs(got - want) <= rel * max(abs(want), floor)


@pytest.mark.parametrize("name", SEEDED)
def test_plusplus_matches_sklearn(name):
    pytest.importorskip("sklearn")
    from sklearn.cluster._kmeans import _kmeans_plusplus

    a = ec.inputs(name)
    pp, _ = ec.expected(name)
    xc = a["x"] - a["x"].mean(axis=0)
    _, want = _kmeans_plusplus(xc, a["k"], (xc * xc).sum(axis=1), np.ones(len(xc)),
                               _Replay(a["first"], a["rand_u"], a["trials"]), n_local_trials=a["trials"])
    np.testing.assert_array_equal(pp.picks, want)


@pytest.mark.parametrize("name", NAMES)
def test_lloyd_matches_sklearn(name):
    pytest.importorskip("sklearn")
    from sklearn.cluster import KMeans

    a = ec.inputs(name)
    pp, ll = ec.expected(name)
    init = a["init"] if "init" in a else a["x"][pp.picks]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(a["k"], init=init.copy(), n_init=1, max_iter=a["max_iter"], tol=a["tol"]).fit(a["x"].copy())
    np.testing.assert_array_equal(ll.labels, km.labels_)
    assert ll.n_iter == km.n_iter_
    np.testing.assert_allclose(ll.centers, km.cluster_centers_, rtol=0, atol=1e-9 * np.abs(a["x"]).max())
    assert _inertia_close(ll.inertia, km.inertia_, a["x"]), (ll.inertia, km.inertia_)


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_away_from_every_rounding_decision(name):
    """What lets the device suite compare picks, labels and n_iter exactly.  No case is exempt."""
    c, a = ec.cases()[name], ec.inputs(name)
    pp, ll = ec.expected(name)
    assert ll.gap >= MIN_GAP, "a row lies between two centres"
    assert ll.info["reloc_gap"] >= MIN_GAP, "two farthest rows at (nearly) one distance"
    assert ll.info["tol_margin"] >= 1e-6, "a centre shift lands on the tolerance"
    if c["kind"] == "seeding":
        # an exact lattice: integers, zero column sums, and sums that do not depend on their order
        x = a["x"]
        assert np.array_equal(x, np.round(x)) and not x.sum(axis=0).any() and not x[::-1].sum(axis=0).any()
        xn = (x * x).sum(axis=1)
        closest = np.full(len(x), np.inf)
        for p in pp.picks[:-1]:
            closest = np.minimum(closest, np.maximum((-2.0 * (x @ x[p]) + xn[p]) + xn, 0.0))
            assert np.array_equal(closest, np.round(closest))
            fwd, bwd = np.cumsum(closest), np.cumsum(closest[::-1])
            assert fwd[-1] == bwd[-1] and fwd[-1] < 2.0 ** 53
            assert np.array_equal(fwd[-1] - fwd[:-1], bwd[::-1][1:])  # every suffix sum, both ways round
    elif pp is not None:
        assert pp.pot_gap >= MIN_GAP, "two candidate rows with (nearly) one potential"
        assert pp.search_gap >= MIN_GAP, "a target (nearly) on a prefix sum"


def _in_set(spec, row, n):
    rows = spec[1]
    return row in (ec._row_sets(n)[rows] if isinstance(rows, str) else rows)


@pytest.mark.parametrize("name", [n for n in NAMES if ec.cases()[n]["kind"] == "seeding"])
def test_seeding_case_reaches_its_branch(name):
    c, a = ec.cases()[name], ec.inputs(name)
    pp, _ = ec.expected(name)
    n = c["n"]
    assert pp.picks.tolist() == a["expect_picks"] and len(set(a["expect_picks"])) == c["k"]
    assert pp.picks[0] == c["first"] and c["first"] in (0, n - 1)
    for specs, got, cand in zip(c["steps"], a["trace"], pp.candidates):
        assert [r for _, r in got] == cand
        for spec, (kind, row) in zip(specs, got):
            if kind == "zero":
                assert row == 0
            elif kind == "clip":
                assert row == n - 1
            elif kind == "on" and not isinstance(spec, str):
                assert _in_set(spec, row, n)
    blocks = -(-n // ec.WG)
    if "n65541" in name:
        assert blocks > 256  # second trip of the one-workgroup loops over workgroups
        assert any(p // ec.WG >= 256 for p in pp.picks[1:]) or "firstlast" in name
    if name == "seed_n16385_first0":
        assert {63, 64} <= {int(p) // ec.WG for p in pp.picks}
        assert {0, ec.WG - 1} <= {int(p) % ec.WG for p in pp.picks[1:]}
    if n % ec.WG == 1:
        assert blocks * ec.WG - n == ec.WG - 1  # the last workgroup holds one row
    if name == "seed_dup_candidates_first_wins":
        x = a["x"]
        assert np.array_equal(x[10], x[20]) and pp.candidates[0][:2] == [20, 10] and pp.picks[1] == 20 and pp.pot_gap == 0.0


@pytest.mark.parametrize("name", [n for n in NAMES if ec.cases()[n]["kind"] == "shape"])
def test_shape_case_reaches_its_branch(name):
    c = ec.cases()[name]
    _, ll = ec.expected(name)
    kd = c["k"] * c["d"]
    assert kd <= 3840 and c["n"] >= c["k"]
    if name.startswith("limit"):
        assert 3774 < kd <= 3840 and 2 * kd * 8 + 5152 > 65536
    if name == "shape_n_equals_k":
        # every row its own centre: the centres do not move, so sklearn stops on the shift (0 <= tol) in iteration 1,
        # before the labels can repeat
        assert ll.inertia == 0.0 and ll.n_iter == 1 and ll.info["ended"] == "tol" and ll.info["shift_tot"] == [0.0]
        assert sorted(ll.labels.tolist()) == list(range(c["k"]))


@pytest.mark.parametrize("name", [n for n in NAMES if ec.cases()[n]["kind"] == "reloc"])
def test_relocation_case_reaches_its_branch(name):
    c, a = ec.cases()[name], ec.inputs(name)
    _, ll = ec.expected(name)
    info, sit = ll.info, c["sit"]
    moved = info["relocated"][0]
    assert info["n_empty"][0] == (1 if sit in ("one_empty", "only_member") else 2) == len(moved)
    if "d300" in name:
        assert c["d"] > 256  # second trip of the relocation's loop over the columns
    if c["n"] > 256:
        assert all(far > 256 for far, _, _ in moved) and any(far > 512 for far, _, _ in moved)
    else:
        assert c["n"] < 256
    if sit == "one_empty" and c["n"] > 256:
        assert moved[0][0] == c["n"] - 1
    if sit == "tie":
        x = a["x"]
        far = moved[1][0]
        twin = [i for i in range(len(x)) if i != far and np.array_equal(x[i], x[far])]
        assert len(twin) == 1 and twin[0] > far  # equal rows, equal distances: the lower index was taken
    if sit == "same_old":
        assert moved[0][1] == moved[1][1]
    if sit == "only_member":
        far, old, new = moved[0]
        assert (old, new) == (0, 2) and info["fallback"][0] == [0]


@pytest.mark.parametrize("name", [n for n in NAMES if ec.cases()[n]["kind"] == "ending"])
def test_ending_case_reaches_its_branch(name):
    c = ec.cases()[name]
    _, ll = ec.expected(name)
    info = ll.info
    if name.startswith("end_max_iter"):
        assert ll.n_iter == c["max_iter"] and info["ended"] == "max_iter" and info["changed"][-1] > 0
    if "ends_at" in c:
        assert ll.n_iter == c["ends_at"] and info["ended"] in ("strict", "tol")
    if name == "end_tol0_strict":
        assert info["tol_abs"] == 0.0 and info["ended"] == "strict"
    if name == "end_by_tol_labels_still_changing":
        assert info["ended"] == "tol" and info["changed"][-1] > 0
        assert (ll.labels != info["labels_last_iter"]).any()  # the final E-step moves rows


def test_every_listed_path_has_a_case():
    names = " ".join(NAMES)
    for word in ("n255", "n256", "n257", "n16385", "n65541", "first0", "firstlast", "dup_candidates", "k1_", "k2_", "k3_",
                 "k7_", "k65_", "k256_", "d1", "d2", "d257", "d512", "n_equals_k", "kd3840", "kd3825", "one_empty",
                 "two_empty", "tie", "same_old", "only_member", "far_rows_beyond_256", "two_empty_n200_d300", "max_iter_1 ", "max_iter_15",
                 "max_iter_16", "max_iter_17", "max_iter_32", "max_iter_33", "iteration_15", "iteration_16",
                 "iteration_17", "iteration_33", "tol0", "by_tol"):
        assert word in names + " ", word

"""Case table of the KMeans edge suites (tests/test_kmeans_oracle_host.py on the CPU, tests/test_gpu_kmeans_edges.py on
the device).  Every input is regenerated from ``default_rng`` seeds; nothing is stored, so there is nothing to
regenerate: the expected results come from tests/kmeans_oracle.py at test time, and the host suite holds that oracle
against the real scikit-learn.

Two kinds of input:

* exact lattices (``lattice_rows``): small-integer rows in +/- pairs (row i and row n-1-i), so every column mean is
  exactly 0 and every squared distance, potential and prefix sum is an integer far below 2^53.  Every summation order
  gives the same bits, so k-means++ picks must equal the oracle's exactly for ANY uniforms -- also for uniforms placed on
  purpose on a prefix sum, one ulp above one, at 0 and above 1 (``seeding_uniforms``).
* separated modes plus noise (``mode_rows``, as kmeans_cases.py "modes", scaled down) and plain Gaussian rows
  (``gauss_rows``, slow to converge) for the Lloyd paths.

``cases()`` maps a name to its description; ``inputs(name)`` builds (and caches) the arguments of one fit.
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np

WG = 256  # rows per workgroup in csrc/kmeans.hip (KM_THREADS): only used to NAME rows (first / last row of a workgroup)


# ---- inputs ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_rows(seed, n, d, k_modes=10, spread=300, noise=3, flat=(40, 5), dups=()):
    """(x (n, d) float64 of small integers, mode id per row).  Row n-1-i is minus row i (an odd n has three rows a, b,
    -(a + b) in the middle, the third with mode -1), so the column sums are exactly 0.  ``flat`` = (a, m): rows a .. a+m-1 are copies of row 0 (so rows
    n-a-m .. n-1-a are copies of row n-1): once row 0 (row n-1) is a centre they form a run of zero distances.  The rows
    on both sides of the run are the only members of the two last modes.  ``dups``: (src, dst) rows made equal."""
    rng = np.random.default_rng(seed)
    half = n // 2 - (n % 2)
    modes = rng.integers(-spread, spread + 1, (k_modes, d))
    mode = rng.integers(0, k_modes - 2, half)
    p = modes[mode] + rng.integers(-noise, noise + 1, (half, d))
    if flat is not None:
        a, m = flat
        assert 1 <= a and a + m < half
        p[a:a + m] = p[0]
        mode[a:a + m] = mode[0]
        for row, q in ((a - 1, k_modes - 2), (a + m, k_modes - 1)):
            p[row] = modes[q] + rng.integers(-noise, noise + 1, d)
            mode[row] = q
    for src, dst in dups:
        p[dst] = p[src]
        mode[dst] = mode[src]
    mid, mid_ids = np.zeros((0, d), dtype=p.dtype), np.zeros(0, dtype=mode.dtype)
    if n % 2:
        mid_ids = rng.integers(0, k_modes - 2, 2)
        ab = modes[mid_ids] + rng.integers(-noise, noise + 1, (2, d))
        mid, mid_ids = np.concatenate([ab, -ab.sum(axis=0, keepdims=True)]), np.concatenate([mid_ids, [-1]])
    x = np.concatenate([p, mid, -p[::-1]]).astype(np.float64)
    ids = np.concatenate([mode, mid_ids, mode[::-1] + k_modes])
    x.setflags(write=False)
    return x, ids


@functools.lru_cache(maxsize=None)
def mode_rows(seed, n, d, k):
    rng = np.random.default_rng(seed)
    modes = rng.normal(0, 300, (k, d))
    which = rng.integers(0, k, n) if n > k else rng.permutation(k)  # n == k: one row per mode
    x = np.ascontiguousarray(modes[which] + rng.normal(0, 40, (n, d)))
    x.setflags(write=False)
    return x, which, modes


@functools.lru_cache(maxsize=None)
def gauss_rows(seed, n, d):
    x = np.ascontiguousarray(np.random.default_rng(seed).normal(0, 100, (n, d)))
    x.setflags(write=False)
    return x


def n_local_trials(k):
    return 2 + int(np.log(k))


def drawn_uniforms(seed, n, k):
    """first index and uniforms as utils/kmeans.py draw_plusplus takes them from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    first = int(rs.choice(n, p=np.full(n, 1.0 / n)))
    u = [rs.uniform(size=n_local_trials(k)) for _ in range(k - 1)]
    return first, (np.concatenate(u) if u else np.zeros(0))


# ---- uniforms placed on purpose (lattices only: every number below is an exact integer) ---------------------------------
def _row_sets(n):
    return dict(
        any=range(1, n - 1),
        wg_first=range(WG, n, WG),
        wg_last=range(WG - 1, n, WG),
        blk63=range(63 * WG, min(n, 64 * WG)),
        blk64=range(64 * WG, min(n, 65 * WG)),
        blk256=range(256 * WG, n),
    )


def _uniform_for(target, pot):
    """A double u with u * pot == target exactly, or None."""
    u = target / pot
    for step in range(0, 17):
        for v in ((u,) if step == 0 else (_ulps(u, step), _ulps(u, -step))):
            if v >= 0 and v * pot == target:
                return float(v)
    return None


def _ulps(u, k):
    for _ in range(abs(k)):
        u = np.nextafter(u, np.inf if k > 0 else -np.inf)
    return u


def seeding_uniforms(x, ids, first_idx, steps):
    """Uniforms that make k-means++ take the named paths.  ``steps``: per further centre a list of trials, each one of

    "zero"            u = 0: target 0 -> row 0
    "clip"            u = the double after 1: target above the last prefix sum -> searchsorted gives n, clipped to n - 1
    ("on", rows)      target exactly ON the prefix sum of a row r of ``rows`` (a name of _row_sets or a list) whose own
                      distance is > 0 -> r (searchsorted left)
    ("above", rows)   target one ulp ABOVE the prefix sum of r -> the next row with a distance > 0
    "flat_on" / "flat_above"   the same two with r the row before a run of >= 2 zero distances: the first gives r (the
                      first of the equal prefix sums), the second the first row after the run

    A row is taken only if the pick lands in a mode that holds no centre yet (no two centres in one mode: the Lloyd run
    that follows then has no near-tie).  Returns (rand_u, expected picks, per step the list of (kind, candidate row))."""
    n = len(x)
    xn = (x * x).sum(axis=1)
    sets = _row_sets(n)

    def dist(r):
        return np.maximum((-2.0 * (x @ x[r]) + xn[r]) + xn, 0.0)

    closest = dist(first_idx)
    used = {int(ids[first_idx])}
    picks, us, trace = [int(first_idx)], [], []
    for trials in steps:
        pot = closest.sum()
        prefix = np.cumsum(closest)
        nonzero = np.flatnonzero(closest > 0)
        cands = []
        for spec in trials:
            kind, rows = (spec, None) if isinstance(spec, str) else spec
            if kind == "zero":
                u, r = 0.0, 0
            elif kind == "clip":
                u, r = float(np.nextafter(1.0, 2.0)), n - 1
                assert u * pot > prefix[-1]
            else:
                if kind.startswith("flat"):
                    z = closest == 0
                    rows = [r for r in range(0, n - 2) if not z[r] and z[r + 1] and z[r + 2]]
                    kind = kind[5:]
                elif isinstance(rows, str):
                    rows = sets[rows]
                u = r = None
                for r0 in rows:
                    if closest[r0] <= 0:
                        continue
                    if kind == "on":
                        t, hit = prefix[r0], r0
                    else:
                        t = np.nextafter(prefix[r0], np.inf)
                        after = nonzero[nonzero > r0]
                        if not len(after):
                            continue
                        hit = int(after[0])
                    if int(ids[hit]) in used or ids[hit] < 0:
                        continue
                    u = _uniform_for(t, pot)
                    if u is not None:
                        r = hit
                        break
                assert r is not None, (spec, "no reachable row")
            us.append(u)
            cands.append((spec if isinstance(spec, str) else spec[0], int(r)))
        pots = [np.minimum(closest, dist(r)).sum() for _, r in cands]
        best = int(np.argmin(pots))
        closest = np.minimum(closest, dist(cands[best][1]))
        picks.append(cands[best][1])
        used.add(int(ids[cands[best][1]]))
        trace.append(cands)
    return np.asarray(us, dtype=np.float64), picks, trace


# ---- the table -----------------------------------------------------------------------------------------------------------
def _seed_case(n, d, seed, first, steps, **kw):
    return dict(kind="seeding", n=n, d=d, seed=seed, first=first, steps=steps, k=len(steps) + 1, max_iter=3, tol=1e-4, **kw)


def _shape_case(n, d, k, seed, **kw):
    return dict(kind="shape", n=n, d=d, k=k, seed=seed, max_iter=kw.pop("max_iter", 300), tol=1e-4, **kw)


def _reloc_case(sit, n, seed, d=6):
    return dict(kind="reloc", sit=sit, n=n, d=d, seed=seed, max_iter=300, tol=1e-4)


def _end_case(data, max_iter, tol, **kw):
    return dict(kind="ending", data=data, max_iter=max_iter, tol=tol, **kw)


# slow-converging inputs of the "ending" cases: (rows, n, d, k, seed) -- Gaussian rows, centres from the first k rows
SLOW = ("gauss", 1500, 2, 8, 4115)
CUTS = (1, 15, 16, 17, 32, 33)
# inputs whose uncut fit ends after exactly this many iterations (found by running the oracle over seeds; the host suite
# asserts the count)
ENDS_AT = {15: ("gauss", 400, 2, 5, 5002), 16: ("gauss", 400, 2, 5, 5007), 17: ("gauss", 400, 2, 5, 5018),
           33: ("gauss", 400, 2, 5, 5133)}
TOL_CASE = ("gauss", 3000, 2, 6, 6000)


@functools.lru_cache(maxsize=None)
def cases():
    c = OrderedDict()
    # -- seeding on lattices, one trial per step (L = 1) so that every placed uniform is a pick -----------------------
    c["seed_n255_first0"] = _seed_case(255, 3, 201, 0, [["flat_above"], ["flat_on"], [("on", "any")], [("above", "any")], ["clip"]])
    c["seed_n255_firstlast"] = _seed_case(255, 3, 201, 254, [["zero"], ["flat_above"], ["flat_on"], [("above", "any")]])
    c["seed_n256_first0"] = _seed_case(256, 3, 202, 0, [[("on", [255])], [("above", "any")], ["flat_on"]])
    c["seed_n256_firstlast"] = _seed_case(256, 3, 202, 255, [["zero"], [("on", "any")], ["flat_above"]])
    c["seed_n257_first0"] = _seed_case(257, 3, 203, 0, [[("on", [256])], [("on", [255])], ["flat_above"]])
    c["seed_n257_firstlast"] = _seed_case(257, 3, 203, 256, [["zero"], [("on", "wg_last")], ["flat_on"]])
    c["seed_n16385_first0"] = _seed_case(16385, 2, 204, 0, [[("on", "blk63")], [("on", "blk64")], [("on", "wg_first")],
                                                           [("on", "wg_last")], [("above", "wg_last")], ["flat_above"]])
    c["seed_n16385_firstlast"] = _seed_case(16385, 2, 204, 16384, [["zero"], [("above", "blk63")], [("on", "wg_first")], ["flat_on"]])
    c["seed_n65541_first0"] = _seed_case(65541, 2, 205, 0, [[("on", "blk256")], [("on", "blk64")], ["clip"]])
    c["seed_n65541_firstlast"] = _seed_case(65541, 2, 205, 65540, [["zero"], [("above", "blk63")]])
    # three trials per step; rows 10 and 20 are equal, the trial that names row 20 comes first and must win the tie
    c["seed_dup_candidates_first_wins"] = _seed_case(
        300, 3, 206, 0, [[("on", [20]), ("on", [10]), "zero"], ["zero", ("on", "any"), ("above", "any")]], dups=((20, 10),))
    # -- K and D shapes: modes + noise, k-means++ from RandomState draws, then Lloyd -----------------------------------
    c["shape_k1_d3"] = _shape_case(300, 3, 1, 301)
    c["shape_k2_d1"] = _shape_case(257, 1, 2, 302)
    c["shape_k3_d2_n513"] = _shape_case(513, 2, 3, 303)
    c["shape_k7_d257"] = _shape_case(300, 257, 7, 304)
    c["shape_k7_d512"] = _shape_case(260, 512, 7, 305)
    c["shape_k65_d5"] = _shape_case(700, 5, 65, 306)
    c["shape_k256_d2"] = _shape_case(1000, 2, 256, 307)
    c["shape_n_equals_k"] = _shape_case(7, 4, 7, 308)
    c["shape_k3_d512_class"] = _shape_case(300, 512, 3, 309)  # also fitted through the KMeans class
    # -- the limit band: K*D above 3774 (dynamic + static LDS of km_assign above 64 KiB), up to KM_MAX_KD = 3840 ----------
    c["limit_k10_d384_kd3840"] = _shape_case(300, 384, 10, 311)
    c["limit_k15_d255_kd3825"] = _shape_case(300, 255, 15, 312)
    c["limit_k256_d15_kd3840"] = _shape_case(2000, 15, 256, 313)
    # -- relocation with an array init ---------------------------------------------------------------------------------------
    for sit in ("one_empty", "two_empty", "tie", "same_old", "only_member"):
        c["reloc_%s_n200" % sit] = _reloc_case(sit, 200, 400 + len(c))
        c["reloc_%s_n600_far_rows_beyond_256" % sit] = _reloc_case(sit, 600, 400 + len(c))
    c["reloc_two_empty_n200_d300"] = _reloc_case("two_empty", 200, 431, d=300)  # second trip of the relocation's D loop
    # -- endings --------------------------------------------------------------------------------------------------------------
    for m in CUTS:
        c["end_max_iter_%d" % m] = _end_case(SLOW, m, 1e-4)
    for it, data in ENDS_AT.items():
        c["end_at_iteration_%d" % it] = _end_case(data, 300, 1e-4, ends_at=it)
    c["end_tol0_strict"] = _end_case(ENDS_AT[17], 300, 0.0)
    c["end_by_tol_labels_still_changing"] = _end_case(TOL_CASE, 300, 1e-2)
    return c


def _reloc_inputs(c):
    """Three modes of rows; K = 5 (4 for "one_empty") centres of which some start far from all rows, so their clusters
    are empty after the first assignment.  Outlier rows are placed by hand, below row 256 for n = 200 and above row
    256 (and 512) for n = 600:

    one_empty    one far centre, one outlier (the last row of the larger table)
    two_empty    two far centres (clusters 0 and 2), outliers in two different modes at distinct distances
    tie          two far centres; the farthest row is alone, the second farthest distance is shared by two exactly equal
                 rows, of which the lower one is taken.  (sklearn's argpartition may take either; they are equal rows
                 with equal labels, so sums, counts and centres are the same whichever it takes.  Two empty clusters
                 that BOTH take tied rows would get equal centres, and every later assignment would tie exactly.)
    same_old     two far centres, both outliers in the same mode (and cluster)
    only_member  cluster 0 starts beyond an outlier so that it holds this row alone, and the row is still the
                 farthest of all from its centre: it goes to the empty cluster 2, cluster 0 is left with no row and
                 takes the row of the largest cluster in _average_centers (0 < that cluster: the row is not yet averaged)"""
    n, d, sit = c["n"], c["d"], c["sit"]
    x, which, modes = mode_rows(c["seed"], n, d, 3)
    x = x.copy()
    rng = np.random.default_rng(c["seed"] + 1)
    big = n > 256
    r1, r2, r3 = (300, 520, 580) if big else (17, 130, 170)
    e0 = np.zeros(d)
    e0[0] = 1.0
    e1 = np.zeros(d)
    e1[1] = 1.0
    rep = [int(np.flatnonzero(which == m)[-5]) for m in range(3)]  # one ordinary row per mode, for the init
    far1, far2 = np.full(d, 1e4), np.full(d, -1e4)
    if sit == "one_empty":
        r = n - 1 if big else 0
        x[r] = modes[which[r]] + 2000 * e0
        init = np.stack([x[rep[0]], far1, x[rep[1]], x[rep[2]]])
    elif sit == "two_empty":
        x[r1] = modes[0] + 2000 * e0
        x[r2] = modes[1] + 1500 * e1
        init = np.stack([far1, x[rep[0]], far2, x[rep[1]], x[rep[2]]])
    elif sit == "tie":
        x[r1] = modes[0] + 2500 * e0
        x[r2] = x[r3] = modes[1] + 2000 * e1
        init = np.stack([far1, x[rep[0]], far2, x[rep[1]], x[rep[2]]])
    elif sit == "same_old":
        x[r1] = modes[0] + 1500 * e1
        x[r2] = modes[0] + 2000 * e0
        init = np.stack([far1, x[rep[0]], far2, x[rep[1]], x[rep[2]]])
    elif sit == "only_member":
        x[r2] = modes[0] + 5000 * e0
        init = np.stack([x[r2] + 3000 * e0, x[rep[0]], far2, x[rep[1]], x[rep[2]]])
    else:
        raise ValueError(sit)
    del rng
    return dict(x=np.ascontiguousarray(x), k=len(init), init=init, max_iter=c["max_iter"], tol=c["tol"])


def _rows_of(data):
    kind, n, d, k, seed = data
    x = gauss_rows(seed, n, d) if kind == "gauss" else mode_rows(seed, n, d, k)[0]
    return x, k


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(x, k, max_iter, tol) plus either ``init`` (K, D) or ``first``, ``rand_u``, ``trials`` (k-means++); seeding
    cases add ``expect_picks`` and ``trace`` (what seeding_uniforms aimed at)."""
    c = cases()[name]
    if c["kind"] == "seeding":
        x, ids = lattice_rows(c["seed"], c["n"], c["d"], dups=c.get("dups", ()))
        u, picks, trace = seeding_uniforms(x, ids, c["first"], c["steps"])
        return dict(x=x, k=c["k"], first=c["first"], rand_u=u, trials=len(c["steps"][0]), max_iter=c["max_iter"],
                    tol=c["tol"], expect_picks=picks, trace=trace)
    if c["kind"] == "shape":
        x = mode_rows(c["seed"], c["n"], c["d"], c["k"])[0]
        first, u = drawn_uniforms(c["seed"], c["n"], c["k"])
        return dict(x=x, k=c["k"], first=first, rand_u=u, trials=n_local_trials(c["k"]), max_iter=c["max_iter"], tol=c["tol"])
    if c["kind"] == "reloc":
        return _reloc_inputs(c)
    if c["kind"] == "ending":
        x, k = _rows_of(c["data"])
        return dict(x=x, k=k, init=x[:k].copy(), max_iter=c["max_iter"], tol=c["tol"])
    raise ValueError(c["kind"])


LATTICE_KINDS = ("seeding",)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(PlusPlus or None, Lloyd) of tests/kmeans_oracle.py for a case, computed once per process."""
    import kmeans_oracle

    a = inputs(name)
    if "init" in a:
        return None, kmeans_oracle.lloyd(a["x"], a["init"], a["max_iter"], a["tol"])
    return kmeans_oracle.fit(a["x"], a["k"], a["first"], a["rand_u"], a["trials"], a["max_iter"], a["tol"])

"""GPU: core-set selection under the l1, cosine and Chebyshev metrics (csrc/kcenter_metric.hip, mval_kcenter_select_metric,
``CoreSet(..., metric=)``) against the REAL reference's goldens (golden/coreset_metric.npz) and, at the smallest shapes at
which the kernels can still go wrong, against the numpy restatement (coreset_metric_oracle.py).

Bounds, as in test_coreset_metric_host.py: picks equal; ``min_distances`` bit-equal for l1 / Chebyshev (no products, one
accumulator in feature order on both sides); within 1e-13 absolute for cosine (distances in [0, 2]; a dot product of unit
rows of D <= 512 terms differs between two summation orders by at most ~512 * 1.1e-16 = 5.7e-14, 1.4e-14 at the goldens'
D <= 126, plus a few ulp from the two normalisations).  A randomly drawn case is admissible only if the restatement's own
top two ``min_distances`` differ by more than 1e-9 (relative) at every step, or are exactly equal (a constructed tie)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import coreset_metric_cases as cmc
import coreset_metric_oracle as cmo

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
METRICS = ("manhattan", "cosine", "chebyshev")
COSINE_ATOL = 1e-13
MIN_GAP = cmc.MIN_GAP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "coreset_metric.npz"))


def _say(capsys, text):
    with capsys.disabled():
        print("\n[coreset_metric] " + text)


def _device(dev, feat, labeled, n_select, metric, min_dist=None):
    from multi_view_active_learning_amd import _lib

    ft = feat if torch.is_tensor(feat) else torch.from_numpy(np.ascontiguousarray(feat)).to(dev)
    lab = torch.as_tensor(list(labeled), dtype=torch.int64, device=dev) if len(labeled) else None
    picks, md = _lib.kcenter_select(ft, lab, n_select, min_dist, metric)
    return picks.cpu().tolist(), md


def _same_min_distances(metric, got, want):
    """The bound of the module docstring; NaNs must sit at the same rows."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    if cmo.ALIASES[metric] != "cosine":
        np.testing.assert_array_equal(got, want)
        return 0.0
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    worst = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    assert worst <= COSINE_ATOL, worst
    return worst


def _against_restatement(dev, feat, labeled, n_select, metric, capsys=None, what=""):
    picks, md, gaps = cmo.kcenter_greedy(feat, labeled, n_select, metric)
    assert all(g == 0.0 or g > MIN_GAP for g in gaps), gaps
    got, mdt = _device(dev, feat, labeled, n_select, metric)
    if capsys is not None:
        finite = [g for g in gaps if np.isfinite(g)]
        _say(capsys, f"{what} {metric}: restatement's smallest relative gap {min(finite) if finite else float('inf'):.3e}")
    assert got == picks, (metric, got, picks)
    if md is None:  # no labelled row and no pick: every distance is still +inf
        assert torch.isposinf(mdt).all().item()
    else:
        worst = _same_min_distances(metric, mdt, md)
        if capsys is not None and cmo.ALIASES[metric] == "cosine":
            _say(capsys, f"{what} cosine: max |min_distances - restatement| = {worst:.3e}")
    return picks, mdt


# ---------------------------------------------------------------------------------------------------------------------
# the reference's goldens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cmc.coreset_metric_cases()))
def test_coreset_metric_vs_reference_golden(dev, golden, name, capsys):
    """CoreSet(sal, al, root, metric=m).select_batch(N): the reference's picks, and its final min_distances where the
    golden stores them.  (NotImplementedError before csrc/kcenter_metric.hip existed.)"""
    from multi_view_active_learning_amd.utils.coreset import CoreSet

    c = cmc.coreset_metric_cases()[name]
    assert golden[name + "/gaps"].min() >= MIN_GAP
    sal, al = cmc.build(c)
    cs = CoreSet(sal, al, c["root"], metric=c["metric"])
    assert cs.metric == c["metric"]  # the name as given, alias or not
    got = cs.select_batch(c["select"])
    keys = list(sal.keys())
    assert got == [keys[i] for i in golden[name + "/picks"].tolist()]
    if c["shape"] in cmc.STORES_MIN_DISTANCES:
        worst = _same_min_distances(c["metric"], cs.min_distances, golden[name + "/min_distances"])
        if c["metric"] == "cosine":
            _say(capsys, f"{name}: max |min_distances - reference| = {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------------
# smallest shapes at which the kernels can go wrong, against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_rows_around_one_workgroup(dev, metric, n, capsys):
    """n_obs = 1 (no labelled row: +inf everywhere, the pick is row 0), 255, 256, 257: one short of a workgroup, exactly
    one, and one row in the second."""
    feat = np.random.default_rng(100 + n).standard_normal((n, 57)) * 300.0
    labeled = [n - 1] if n > 1 else []
    _against_restatement(dev, feat, labeled, min(4, n - len(labeled)), metric, capsys, f"n={n}")


@pytest.mark.parametrize("metric", METRICS)
def test_grid_stride_second_trip_and_continuation(dev, metric, capsys):
    """262 145 rows = KC_MAX_BLOCKS * KC_THREADS + 1: workgroup 0 makes a second trip through the init and the step loop
    for one row (D = 3 keeps it small: 6.3 MB).  That last row is made the farthest one, so the second trip decides the
    first pick.  Then a continuation: 4 picks followed by 2 more on the returned min_dist (have_min_dist = 1, no new
    centres) equal one call of 6 -- picks and bits."""
    n, d = 1024 * 256 + 1, 3
    feat = np.random.default_rng(7).standard_normal((n, d)) * 300.0
    feat[0] = [250.0, 10.0, -40.0]
    feat[1] = feat[0] * 2.0  # both labelled rows in one direction ...
    feat[n - 1] = feat[0] * -20.0  # ... and the last row opposite to it and far out: the farthest under every metric
    labeled = [0, 1]
    picks, mdt = _against_restatement(dev, feat, labeled, 6, metric, capsys, f"n={n}")
    assert picks[0] == n - 1
    ft = torch.from_numpy(feat).to(dev)
    first, md4 = _device(dev, ft, labeled, 4, metric)
    more, md6 = _device(dev, ft, [], 2, metric, md4)
    assert first + more == picks
    assert torch.equal(md6, mdt)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [1, 3, 57, 126, 512])
def test_feature_widths(dev, metric, d, capsys):
    """D = 1 and 512 are the ends of the accepted range, 57 and 126 the two data sets' widths.  Under cosine D = 1
    normalises every row to +-1: all distances are exactly 0 or 2 and every step is an exact tie (lowest index wins)."""
    n = 300
    feat = np.random.default_rng(200 + d).standard_normal((n, d)) * 300.0
    _against_restatement(dev, feat, [n - 2, n - 1], 4, metric, capsys, f"D={d}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("l", [0, 1, 4, 5, 9])
def test_labelled_counts_around_the_centre_groups(dev, metric, l, capsys):
    """The init pass stages four centres per trip over a row: none, one, one full group, a group + 1, two groups + 1."""
    n = 300
    feat = np.random.default_rng(300 + l).standard_normal((n, 57)) * 300.0
    _against_restatement(dev, feat, list(range(n - l, n)), 4, metric, capsys, f"L={l}")


def _raw(dev, metric_id, ft, labeled, n_select, entry="mval_kcenter_select_metric"):
    """The C entry itself, with sentinels in picks and min_dist."""
    from multi_view_active_learning_amd import _lib

    n, d = ft.shape
    picks = torch.full((max(n_select, 1) + 2,), -7, dtype=torch.int64, device=dev)
    md = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    norms = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    ws = torch.empty((_lib.kcenter_workspace_bytes(n, d) // 8 + 1,), dtype=torch.float64, device=dev)
    lab = torch.as_tensor(labeled, dtype=torch.int64, device=dev) if labeled else None
    args = (_lib._p(ft), C.c_longlong(n), C.c_int(d), _lib._p(lab), C.c_longlong(len(labeled)), C.c_int(n_select), C.c_int(0),
            _lib._p(norms), _lib._p(md), _lib._p(picks), _lib._p(ws), _lib._stream())
    if entry == "mval_kcenter_select":
        rc = _lib.lib().mval_kcenter_select(*args)
    else:
        rc = _lib.lib().mval_kcenter_select_metric(C.c_int(metric_id), *args)
    assert rc == 0
    return picks.cpu().tolist(), md, norms


@pytest.mark.parametrize("metric", METRICS)
def test_no_picks_leaves_picks_untouched_and_min_dist_initialised(dev, metric):
    from multi_view_active_learning_amd import _lib

    n, d = 257, 57
    feat = np.random.default_rng(77).standard_normal((n, d)) * 300.0
    ft = torch.from_numpy(feat).to(dev)
    mid = _lib.KC_METRIC_IDS[metric]
    p, md, norms = _raw(dev, mid, ft, [], 0)
    assert p == [-7] * 3 and torch.isposinf(md).all().item()
    p, md, norms = _raw(dev, mid, ft, [3, 200], 0)
    assert p == [-7] * 3
    _same_min_distances(metric, md, np.min(cmo.distances(cmo.prepare(feat, metric), [3, 200], metric), axis=1))
    if metric == "cosine":  # row_norms receives the divisors; the other forms leave it alone
        np.testing.assert_allclose(norms.cpu().numpy(), np.sqrt((feat * feat).sum(axis=1)), rtol=1e-14)
    else:
        assert (norms == -7.0).all().item()
    p, md, _ = _raw(dev, mid, ft, [], 1)
    assert p == [0, -7, -7]


@pytest.mark.parametrize("metric", METRICS)
def test_identical_poses_tie_at_row_zero(dev, metric):
    """Every pose the same (300 pool rows in two workgroups, 2 labelled): every distance is the same number -- under
    cosine whatever 1 - xh.xh rounds to -- so every step is a tie and the picks are [0, 0, 0, 0, 0]."""
    from multi_view_active_learning_amd.utils.coreset import CoreSet

    pose = (np.random.default_rng(3).standard_normal((19, 3)) * 300.0).astype(np.float32)
    sal = {i: pose.tolist() for i in range(300)}
    al = {i: np.concatenate([pose.astype(np.float64), np.ones((19, 1))], axis=1) for i in range(2)}
    cs = CoreSet(sal, al, 2, metric=metric)
    assert cs.select_batch(5) == [0, 0, 0, 0, 0]
    md = cs.min_distances.cpu().numpy()
    assert (md == md[0]).all() and abs(md[0]) <= COSINE_ATOL
    # the reference's own degenerate case (its tests/test_coreset.py): every joint of every pose at one point, so every
    # feature row is zero -- cosine distance exactly 1 everywhere, 0 under the other two
    sal = {i: [[0, 1, 2] for _ in range(19)] for i in range(20)}
    al = {i: [[0, 1, 2] for _ in range(19)] for i in range(5)}
    cs = CoreSet(sal, al, 2, metric=metric)
    assert cs.select_batch(5) == [0, 0, 0, 0, 0]
    assert (cs.min_distances == (1.0 if metric == "cosine" else 0.0)).all().item()


def test_cosine_zero_row_is_at_distance_one_and_pickable(dev):
    """A pose whose joints all equal the root has a zero feature row: its norm counts as 1, it stays zero, and its cosine
    distance to every row -- itself included, nothing is zeroed -- is exactly 1.0.  With the other pool rows close to the
    labelled direction it is the farthest row, is picked, and (still at distance 1 from itself) is picked again."""
    from multi_view_active_learning_amd.utils.coreset import CoreSet

    rng = np.random.default_rng(11)
    n, j, root, z = 300, 19, 2, 270
    base = rng.standard_normal((j, 3)) * 300.0
    pool = base[None] + rng.standard_normal((n, j, 3)) * 30.0
    pool[z] = pool[z, root]  # every joint at the root
    lab = base[None] + rng.standard_normal((2, j, 3)) * 30.0
    cs = CoreSet.from_tensors(torch.from_numpy(pool).to(dev), torch.from_numpy(lab).to(dev), root, metric="cosine")
    feat = cs.features.cpu().numpy()
    assert (feat[z] == 0.0).all()
    _, md = _device(dev, cs.features, [z], 0, "cosine")
    assert (md == 1.0).all().item()
    want, wmd, _ = cmo.kcenter_greedy(feat, cs.al_indices, 3, "cosine")
    assert want == [z, z, z]
    assert cs.select_batch(3) == want
    assert cs.min_distances[z].item() == 1.0
    _same_min_distances("cosine", cs.min_distances, wmd)


def test_cosine_power_of_two_multiples_are_one_row(dev):
    """Rows a, 4a and a/8 are bit-identical after normalisation (scaling by a power of two commutes with every rounding
    on the way): their distances to any centre are the same bits, their mutual distance equals each row's self-distance,
    and either of them as the centre gives the same min_dist vector."""
    n = 300
    feat = np.random.default_rng(13).standard_normal((n, 57)) * 300.0
    feat[40] = feat[7] * 4.0
    feat[299] = feat[7] * 0.125
    ft = torch.from_numpy(feat).to(dev)
    mds = [_device(dev, ft, [r], 0, "cosine")[1] for r in (7, 40, 299)]
    assert torch.equal(mds[0], mds[1]) and torch.equal(mds[0], mds[2])
    m = mds[0].cpu().numpy()
    assert m[7] == m[40] == m[299] and m[7] <= COSINE_ATOL
    _, md = _device(dev, ft, [5], 0, "cosine")
    m = md.cpu().numpy()
    assert m[7] == m[40] == m[299]


@pytest.mark.parametrize("metric", METRICS)
def test_exact_ties_across_workgroups_and_trips(dev, metric):
    """The farthest row A three times -- index 10 (workgroup 0), 300 (workgroup 1) and 262 144 + 5 (workgroup 0 again,
    second trip of the grid-stride loop) -- and the second-farthest row B at 262 144 + 6 and at the last index: the lowest
    index must win each time, so the picks start 10, 262 150.  Copies of a row are bit-identical, so these ties are exact
    under every metric; for l1 / Chebyshev the features are integers and every distance is exact as well.  The small pool
    (1000 rows, 4 workgroups) does the same without the second trip."""
    for n, dup in ((300_000, (10, 300, 262_144 + 5)), (1000, (10, 300, 777))):
        rng = np.random.default_rng(n)
        b_rows = (262_144 + 6, n - 1) if n > 262_144 else (600, n - 1)
        if metric == "cosine":
            u = rng.standard_normal(8)
            u /= np.linalg.norm(u)
            w = rng.standard_normal(8)
            w -= u * (w @ u)  # orthogonal to u: cosine distance ~1 from +-u
            feat = (u[None] + rng.standard_normal((n, 8)) * 0.05) * rng.uniform(50.0, 500.0, size=(n, 1))
            feat[list(dup)] = -300.0 * u  # distance ~2 from the labelled direction
            feat[list(b_rows)] = 200.0 * w
        else:
            feat = rng.integers(-50, 51, size=(n, 8)).astype(np.float64)
            feat[list(dup)] = 2000.0
            feat[list(b_rows)] = -1000.0
        labeled = [0, 1]
        picks, md, gaps = cmo.kcenter_greedy(feat, labeled, 4, metric)
        assert picks[:2] == [dup[0], b_rows[0]] and gaps[0] == 0.0 and gaps[1] == 0.0
        assert all(g == 0.0 or g > MIN_GAP for g in gaps), gaps
        got, mdt = _device(dev, feat, labeled, 4, metric)
        assert got == picks, (n, got, picks)
        _same_min_distances(metric, mdt, md)


@pytest.mark.parametrize("metric", METRICS)
def test_nan_row(dev, metric):
    """The rules of the Euclidean kernels: a NaN row is the maximum (np.argmax) and is picked first; its distances are
    NaN and spread through ``minimum``, so every later pick is row 0.  Against the restatement only -- sklearn refuses
    non-finite input."""
    n, d = 1000, 57
    feat = np.random.default_rng(5).standard_normal((n, d)) * 300.0
    feat[417, 3] = np.nan
    labeled = [998, 999]
    picks, md, _ = cmo.kcenter_greedy(feat, labeled, 3, metric)
    assert picks == [417, 0, 0] and np.isnan(md).all()
    got, mdt = _device(dev, feat, labeled, 3, metric)
    assert got == picks and torch.isnan(mdt).all().item()
    got1, md1 = _device(dev, feat, labeled, 1, metric)
    assert got1 == [417] and torch.isnan(md1).all().item()
    _, md0 = _device(dev, feat, labeled, 0, metric)  # before any pick only the NaN row itself is NaN
    m0 = md0.cpu().numpy()
    assert np.isnan(m0[417]) and np.isfinite(np.delete(m0, 417)).all()


# ---------------------------------------------------------------------------------------------------------------------
# the Euclidean entry is what it was; the public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_euclidean_entry_unchanged_and_forwarded(dev):
    """mval_kcenter_select called directly gives the reference's picks of golden/coreset.npz as before, and
    mval_kcenter_select_metric(MVAL_KC_EUCLIDEAN) and kcenter_select(metric="euclidean" / "l2") give its picks and its
    min_dist bits (they forward to it)."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.coreset import CoreSet

    c = cases.coreset_cases()["n1000_l200_j42"]
    pool, lab = cases.coreset_arrays(c)
    z = np.load(os.path.join(G, "coreset.npz"))
    cs = CoreSet.from_tensors(torch.from_numpy(pool).to(dev), torch.from_numpy(lab).to(dev), c["root"])
    ft, labeled, k = cs.features, cs.al_indices, c["select"]
    p0, md0, _ = _raw(dev, None, ft, labeled, k, entry="mval_kcenter_select")
    assert p0[:k] == z["n1000_l200_j42/picks"].tolist() and p0[k:] == [-7, -7]
    p1, md1, _ = _raw(dev, _lib.KC_EUCLIDEAN, ft, labeled, k)
    assert p1 == p0 and torch.equal(md1, md0)
    for name in ("euclidean", "l2"):
        p2, md2 = _device(dev, ft, labeled, k, name)
        assert p2 == p0[:k] and torch.equal(md2, md0)
    p3, md3 = _lib.kcenter_select(ft, torch.as_tensor(labeled, dtype=torch.int64, device=dev), k)  # the default
    assert p3.cpu().tolist() == p0[:k] and torch.equal(md3, md0)


@pytest.mark.parametrize("metric", METRICS + ("l1", "cityblock"))
def test_from_tensors_with_metric_and_empty_labelled_set(dev, metric):
    """CoreSet.from_tensors(..., metric=): the dict-free path, with a labelled set and without one (L = 0 has no reference
    golden -- its constructor raises IndexError -- so the restatement is the yardstick: first pick row 0)."""
    from multi_view_active_learning_amd.utils.coreset import CoreSet

    c = dict(seed=71, n=300, l=3, j=19)
    pool, lab = cases.coreset_arrays(c)
    for l in (3, 0):
        cs = CoreSet.from_tensors(torch.from_numpy(pool).to(dev), torch.from_numpy(lab[:l]).to(dev), 2, metric=metric)
        assert cs.metric == metric
        feat = cmo.stacked_features(pool, lab[:l], 2)
        np.testing.assert_array_equal(cs.features.cpu().numpy(), feat)
        want, wmd, gaps = cmo.kcenter_greedy(feat, range(300, 300 + l), 5, metric)
        assert all(g > MIN_GAP for g in gaps)
        assert cs.select_batch(5) == want and (l > 0 or want[0] == 0)
        _same_min_distances(metric, cs.min_distances, wmd)
        # update_distances / a second select_batch continue on top, as under the Euclidean metric
        more, wmd2, _ = cmo.kcenter_greedy(feat, [], 2, metric, min_d=wmd)
        assert cs.select_batch(2) == more
        _same_min_distances(metric, cs.min_distances, wmd2)


def _strategy(metric_in_config=None):
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    cfg = get_default_configs()
    cfg.AL.STRATEGY = "CORESET"
    if metric_in_config is not None:
        cfg.AL.CORESET_METRIC = metric_in_config
    return ActiveLearningStrategy(cfg)


def test_select_al_guids_passes_the_metric(dev):
    """select_al_guids(..., metric="cosine") == CoreSet(..., metric="cosine").select_batch; metric=None reads
    AL.CORESET_METRIC, whose default "euclidean" is the behaviour before the argument existed."""
    from multi_view_active_learning_amd.utils.coreset import CoreSet

    c = cmc.coreset_metric_cases()["cosine/n64_l5_j19"]
    sal, al = cmc.build(c)
    sal_dict = {"pred_3d_keypoints": sal, "al_metric": {g: 0.0 for g in sal}}
    st = _strategy()
    root = st.joint_root_index
    by_metric = {m: CoreSet(sal, al, root, metric=m).select_batch(6) for m in ("cosine", "euclidean", "chebyshev")}
    assert by_metric["cosine"] != by_metric["euclidean"]
    assert st.select_al_guids(sal_dict, 6, al, metric="cosine") == by_metric["cosine"]
    assert st.select_al_guids(sal_dict, 6, al) == by_metric["euclidean"]
    assert _strategy("chebyshev").select_al_guids(sal_dict, 6, al) == by_metric["chebyshev"]
    assert _strategy("chebyshev").select_al_guids(sal_dict, 6, al, metric="cosine") == by_metric["cosine"]
    with pytest.raises(NotImplementedError):
        st.select_al_guids(sal_dict, 6, al, metric="minkowski")


def _two_rank_worker(rank, world, path, out, c):
    import sys

    import torch.distributed as dist

    for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method="file://" + path)
    res = _core_set_pass(c, _frames_of(c)[rank::world])  # DistributedSampler: indices[rank::world]
    torch.save(res, out + ".%d" % rank)
    dist.barrier()
    dist.destroy_process_group()


def _frames_of(c):
    """The case's loader as per-frame records (dict of arrays without the batch axis, heat-maps (V, J, h, w))."""
    loader, hms = cases.build_sal_loader(c)
    out = []
    for dp, hm in zip(loader, hms):
        b = dp["pose"].shape[0]
        hm = hm.reshape((b, -1) + hm.shape[1:])
        out += [({k: v[i] for k, v in dp.items()}, hm[i]) for i in range(b)]
    return out


def _core_set_pass(c, frames):
    """Pool scoring of one rank's frames (the gather inside when torch.distributed is up), then the replicated greedy
    loop under the metric: once from the argument, once from AL.CORESET_METRIC."""
    dev = torch.device("cuda:0")
    st = _strategy()
    st.al_cfg.POSE_ESTIMATOR.STRIDE = c["stride"]
    loader, hms = [], []
    for i in range(0, len(frames), c["b"]):
        chunk = frames[i:i + c["b"]]
        loader.append({k: torch.from_numpy(np.stack([f[0][k] for f in chunk])) for k in chunk[0][0]})
        hms.append(np.concatenate([f[1] for f in chunk]))
    it = iter(hms)
    sal = st._compute_sal_dict(loader, lambda images: torch.from_numpy(next(it)).to(dev))
    rng = np.random.default_rng(9)
    labeled = {"L-%d" % i: (rng.standard_normal((c["j"], 3)) * 250.0).tolist() for i in range(5)}
    picks = st.select_al_guids(sal, c["select"], labeled, metric=c["metric"])
    st.al_cfg.AL.CORESET_METRIC = c["metric"]
    return {"guids": list(sal["pred_3d_keypoints"]), "picks": picks, "picks_cfg": st.select_al_guids(sal, c["select"], labeled),
            "euclidean": st.select_al_guids(sal, c["select"], labeled, metric="euclidean")}


def test_two_ranks_one_gpu_core_set_pass_under_manhattan(dev, tmp_path):
    """World size 2 (two processes on cuda:0 over gloo, as tests/test_gpu_distributed.py): the predictions are gathered
    once, every rank runs the greedy loop under metric="manhattan" and gets the one-rank picks."""
    import torch.multiprocessing as mp

    c = dict(cases.sal_cases()["mpe"], strategy="CORESET", nbatch=4, select=3, metric="manhattan")
    sync, out = str(tmp_path / "sync"), str(tmp_path / "out")
    mp.spawn(_two_rank_worker, args=(2, sync, out, c), nprocs=2, join=True)
    got = [torch.load(out + ".%d" % r, weights_only=False) for r in range(2)]
    want = _core_set_pass(c, _frames_of(c))
    assert len(want["guids"]) == 8 and len(want["picks"]) == 3
    for g in got:
        assert g["guids"] == want["guids"]
        assert g["picks"] == want["picks"] and g["picks_cfg"] == want["picks"] and g["euclidean"] == want["euclidean"]

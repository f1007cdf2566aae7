"""Device KMeans (csrc/kmeans.hip through _lib.kmeans_fit, and utils/kmeans.py where noted) at the branches, sizes and
limits the stored sklearn fits of test_gpu_kmeans.py do not reach: every case of tests/golden/kmeans_edge_cases.py against
the plain numpy restatement tests/kmeans_oracle.py (which tests/test_kmeans_oracle_host.py holds against the real
scikit-learn, together with the conditions that make an exact comparison fair and the branch each case is named for).

Contract: k-means++ picks, labels and n_iter exactly; centres to 1e-9 * max|X| absolute; inertia to
1e-10 relative.  Each test prints the oracle's gaps and the errors it saw; the last test prints the worst of the run.
Nothing is stored: inputs come from seeds, expectations from the oracle, so there is nothing to regenerate.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import kmeans_edge_cases as ec

pytestmark = pytest.mark.gpu
NAMES = list(ec.cases())
WORST = dict(centre=0.0, centre_case="", inertia=0.0, inertia_case="", fits=0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _say(capsys, text):
    with capsys.disabled():
        print("\n    " + text, end="")


def _up(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dev)  # (a copy: the table's arrays are read-only)


def _host(res):
    centers, labels, inertia, n_iter, idx = res
    return (centers.cpu().numpy(), labels.cpu().numpy(), float(inertia.item()), int(n_iter.item()), idx.cpu().numpy())


def _fit(dev, name, x_dev=None, **over):
    from multi_view_active_learning_amd import _lib

    a = dict(ec.inputs(name), **over)
    x = _up(a["x"], dev) if x_dev is None else x_dev
    if "init" in a:
        res = _lib.kmeans_fit(x, a["k"], _up(a["init"], dev), 0, None, 1, a["max_iter"], a["tol"])
    else:
        u = _up(a["rand_u"], dev) if a["k"] > 1 else None
        res = _lib.kmeans_fit(x, a["k"], None, a["first"], u, a["trials"], a["max_iter"], a["tol"])
    return _host(res)


def _fit_raw(dev, name, ws):
    """mval_kmeans_fit through the C ABI with a caller-chosen workspace tensor (any slice of a float64 tensor)."""
    from multi_view_active_learning_amd import _lib

    a = ec.inputs(name)
    x = _up(a["x"], dev)
    n, d = x.shape
    k = a["k"]
    init = _up(a["init"], dev) if "init" in a else None
    u = _up(a["rand_u"], dev) if "init" not in a and k > 1 else None
    trials = 1 if init is not None else a["trials"]
    assert ws.numel() * 8 >= _lib.kmeans_workspace_bytes(n, d, k, trials)
    centers = torch.empty((k, d), dtype=torch.float64, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    inertia = torch.empty((1,), dtype=torch.float64, device=dev)
    n_iter = torch.empty((1,), dtype=torch.int32, device=dev)
    idx = torch.empty((k,), dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    rc = _lib.lib().mval_kmeans_fit(p(x), C.c_longlong(n), C.c_int(d), C.c_int(k), p(init), C.c_longlong(a.get("first", 0)),
                                    p(u), C.c_int(trials), C.c_int(a["max_iter"]), C.c_double(a["tol"]), p(centers),
                                    p(labels), p(inertia), p(n_iter), p(idx), p(ws),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.lib().mval_last_error()
    return _host((centers, labels, inertia, n_iter, idx))


def _against_oracle(name, got, capsys, what=""):
    centers, labels, inertia, n_iter, idx = got
    a = ec.inputs(name)
    pp, ll = ec.expected(name)
    x = a["x"]
    gaps = "Lloyd gap %.2e" % ll.gap
    if pp is not None:
        gaps += ", potential gap %.2e, search gap %.2e" % (pp.pot_gap, pp.search_gap)
        np.testing.assert_array_equal(idx, pp.picks)
    else:
        np.testing.assert_array_equal(idx, np.full(a["k"], -1))
    assert labels.dtype == np.int32 and centers.dtype == np.float64
    bound = 1e-9 * float(np.abs(x).max())
    cerr = float(np.abs(centers - ll.centers).max())
    floor = 1e-20 * x.shape[0] * float(np.abs(x).max()) ** 2
    ierr = abs(inertia - ll.inertia) / max(abs(ll.inertia), floor)
    _say(capsys, f"{what or name}: {gaps}; n_iter {n_iter} (oracle {ll.n_iter}, ended by {ll.info['ended']}); centres off by "
                 f"{cerr:.2e} (bound {bound:.2e}); inertia off by {ierr:.2e} relative (bound 1e-10)")
    np.testing.assert_array_equal(labels, ll.labels)
    assert n_iter == ll.n_iter
    assert cerr <= bound
    assert ierr <= 1e-10
    WORST["fits"] += 1
    if cerr / bound > WORST["centre"]:
        WORST.update(centre=cerr / bound, centre_case=name)
    if ierr > WORST["inertia"]:
        WORST.update(inertia=ierr, inertia_case=name)


def _same_bits(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2] and a[3] == b[3]
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[4], b[4])


# ---- every case of the table: seeding on lattices, K and D shapes, the limit band, relocation, endings ---------------
@pytest.mark.parametrize("name", NAMES)
def test_case_matches_oracle(dev, name, capsys):
    _against_oracle(name, _fit(dev, name), capsys)


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------
GOOD = "reloc_two_empty_n200"
REFUSALS = {
    "kd_3841": (dict(n=30, d=167, k=23), "bad dims"),
    "d_513": (dict(n=10, d=513, k=1), "bad dims"),
    "k_257": (dict(n=300, d=1, k=257), "bad dims"),
    "n_below_k": (dict(n=5, d=3, k=7), "bad dims"),
    "l_17": (dict(n=50, d=3, k=4, trials=17), r"k-means\+\+ needs"),
    "first_idx_n": (dict(n=50, d=3, k=4, first=50), r"k-means\+\+ needs"),
    "max_iter_0": (dict(n=50, d=3, k=4, max_iter=0), "bad max_iter"),
    "tol_negative": (dict(n=50, d=3, k=4, tol=-1e-4), "bad max_iter"),
}


@pytest.mark.parametrize("which", list(REFUSALS))
def test_refusal_then_a_good_fit(dev, which, capsys):
    from multi_view_active_learning_amd import _lib

    r, text = REFUSALS[which]
    assert r["d"] * r["k"] == 3841 or which != "kd_3841"
    x = torch.zeros((r["n"], r["d"]), dtype=torch.float64, device=dev)
    trials = r.get("trials", ec.n_local_trials(r["k"]))
    u = torch.full((max(1, (r["k"] - 1) * trials),), 0.5, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.MvalError, match="mval_kmeans_fit: " + text):
        _lib.kmeans_fit(x, r["k"], None, r.get("first", 0), u, trials, r.get("max_iter", 10), r.get("tol", 1e-4))
    _against_oracle(GOOD, _fit(dev, GOOD), capsys, "after the refusal " + which)


# ---- plumbing --------------------------------------------------------------------------------------------------------------
PLUMB = "reloc_only_member_n600_far_rows_beyond_256"


def test_workspace_pointer_off_by_8_bytes(dev, capsys):
    from multi_view_active_learning_amd import _lib

    a = ec.inputs(PLUMB)
    words = _lib.kmeans_workspace_bytes(a["x"].shape[0], a["x"].shape[1], a["k"], 1) // 8 + 1
    base = torch.empty((words + 64,), dtype=torch.float64, device=dev)
    at0 = (-base.data_ptr() % 256) // 8  # first 256-byte-aligned element
    odd, even = base[at0 + 1:at0 + 1 + words], base[at0:at0 + words]
    assert odd.data_ptr() % 256 == 8 and even.data_ptr() % 256 == 0
    got = _fit_raw(dev, PLUMB, odd)
    _same_bits(got, _fit_raw(dev, PLUMB, even))
    _against_oracle(PLUMB, got, capsys, "workspace + 8 bytes")


def test_side_stream_gives_the_same_bits(dev, capsys):
    want = _fit(dev, PLUMB)
    side = torch.cuda.Stream(device=dev)
    x = _up(ec.inputs(PLUMB)["x"], dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        got = _fit(dev, PLUMB, x_dev=x)
    side.synchronize()
    _same_bits(got, want)
    _against_oracle(PLUMB, got, capsys, "side stream")


def test_small_fit_after_a_large_one_on_the_same_memory(dev, capsys):
    from multi_view_active_learning_amd import _lib

    large, small = "seed_n16385_first0", "reloc_tie_n200"
    a = ec.inputs(large)
    words = _lib.kmeans_workspace_bytes(a["x"].shape[0], a["x"].shape[1], a["k"], a["trials"]) // 8 + 1
    ws = torch.empty((words,), dtype=torch.float64, device=dev)
    fresh = _fit_raw(dev, small, torch.zeros((words,), dtype=torch.float64, device=dev))
    _against_oracle(large, _fit_raw(dev, large, ws), capsys, "large fit")
    got = _fit_raw(dev, small, ws)
    _same_bits(got, fresh)
    _against_oracle(small, got, capsys, "small fit on the large fit's workspace")


@pytest.mark.parametrize("name", ["shape_k1_d3", "shape_k3_d512_class"])
def test_kmeans_class(dev, name, capsys):
    """KMeans(K, random_state=seed) draws what the case's drawn_uniforms(seed) draws."""
    from multi_view_active_learning_amd.utils.kmeans import KMeans

    c, a = ec.cases()[name], ec.inputs(name)
    km = KMeans(c["k"], random_state=c["seed"], max_iter=a["max_iter"], tol=a["tol"]).fit(np.array(a["x"]))
    assert km.init_indices_.shape == (1, c["k"])
    _against_oracle(name, (km.cluster_centers_, km.labels_, km.inertia_, km.n_iter_, km.init_indices_[0]), capsys,
                    "KMeans(%d) on %s" % (c["k"], name))


def test_zz_report_worst_errors(dev, capsys):
    """Runs last in this file: the measured slack of the whole run beside the contract's bounds."""
    assert WORST["fits"] > 0
    _say(capsys, "%d fits against the oracle: worst centre error %.3g of its bound 1e-9 * max|X| (%s); worst inertia error "
                 "%.3g relative, bound 1e-10 (%s)\n" % (WORST["fits"], WORST["centre"], WORST["centre_case"], WORST["inertia"],
                                                        WORST["inertia_case"]))

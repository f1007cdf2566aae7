"""2-D PCKh on the device against the real reference's numbers (tests/golden/pckh2d.npz) and their NumPy float32 restatement
(tests/golden/pckh2d_cases.py): the box-scaled decode (``mval_pred_coordinates`` / ``_from_keys``), the counters
(``mval_pckh2d``), the reference-shaped functions of utils/evaluation.py, the pass ``evaluate_2d_pckh`` and the EVAL.METRIC
switch ``evaluate``.  Every comparison is exact equality."""
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases
import pckh2d_cases as pc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "pckh2d.npz"))


def _strategy(**over):
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = 4
    for k, v in over.items():
        node = cfg
        for p in k.split(".")[:-1]:
            node = node[p]
        node[k.split(".")[-1]] = v
    return ActiveLearningStrategy(cfg)


# ---- the reference-shaped functions against the golden ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noisy", "ties", "degenerate"])
def test_pckh_functions_equal_the_reference(dev, golden, name):
    """List-of-tensors input with ragged batches, one 3-D tensor, one 4-D tensor: the fractions are the reference's floats."""
    from multi_view_active_learning_amd.utils import evaluation

    c = pc.metric_cases()[name]
    k = c["num_keypoints"]
    pred, gt = torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(c["gt"]).to(dev)
    ragged = ([t for t in torch.split(pred, list(c["batches"]))], [t for t in torch.split(gt, list(c["batches"]))])
    assert len({t.shape[0] for t in ragged[0]}) > 1
    forms = [ragged, (pred, gt), (pred[None], gt[None])]
    if pred.shape[0] % 2 == 0:
        forms.append((pred.reshape(2, -1, pc.J, 2), gt.reshape(2, -1, pc.J, 2)))
    want, want05 = golden[name + "/figure"], golden[name + "/pckh_0_5"]
    for p, g in forms:
        thresholds, pcks = evaluation.compute_pckh_figure(p, g, k)
        assert thresholds == pc.THRESHOLDS and isinstance(pcks, list) and all(type(v) is float for row in pcks for v in row)
        np.testing.assert_array_equal(np.asarray(pcks), want)
        np.testing.assert_array_equal(np.asarray(evaluation.compute_pckh_0_5(p, g, k)), want05)
        for t in (0.1, 0.3, 0.7, 1.0):
            np.testing.assert_array_equal(np.asarray(evaluation.compute_pckh(p, g, t, k)), want[pc.THRESHOLDS.index(t)])
    if name == "degenerate":
        got = [evaluation.compute_pckh(*ragged, t, k, kp0=c["kp0"], kp1=c["kp1"]) for t in pc.THRESHOLDS]
        np.testing.assert_array_equal(np.asarray(got), golden[name + "/pckh_kp"])
    # float64 input is converted to float32 (the dtype of the reference's only call site)
    np.testing.assert_array_equal(np.asarray(evaluation.compute_pckh_figure(pred.double(), gt.double(), k)[1]), want)
    # a thresholds argument of the caller's comes back as it was given
    th, one = evaluation.compute_pckh_figure(pred, gt, k, thresholds=[0.5])
    assert th == [0.5]
    np.testing.assert_array_equal(np.asarray(one), want05[None])


@pytest.mark.parametrize("s", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("j", [2, 19, 42])
def test_pckh2d_counters_equal_the_restatement(dev, s, j):
    """pckh2d_kernel is laid out as pck3d_kernel: one workgroup per (joint, threshold), ``for (s = threadIdx.x; s < S; s += 256)``.
    S = 1: one thread works; 255 / 256: the last thread idle / busy on the first trip; 257: thread 0 alone takes a second trip;
    1025: a fifth trip.  J = 2 is the smallest the entry accepts (kp0 = 0, kp1 = 1), 42 the hand data set's.  T in {1, 10} and
    n_keypoints in {1, J} change the grid and the row stride of ``hits``; a second head (kp0 = J - 1, kp1 = 0) moves the table reads."""
    from multi_view_active_learning_amd import _lib

    rng = np.random.default_rng(1000 * s + j)
    gt = rng.uniform(10.0, 240.0, (s, j, 2)).astype(np.float32)
    pred = (gt + rng.standard_normal((s, j, 2)) * 25.0).astype(np.float32)
    pt, gt_t = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    for thr in ((0.5,), pc.THRESHOLDS):
        for nk in (1, j):
            for kp0, kp1 in ((0, 1), (j - 1, 0)):
                hits = _lib.pckh2d(pt, gt_t, thr, nk, kp0, kp1)
                assert hits.dtype == torch.int64 and tuple(hits.shape) == (len(thr), nk)
                want = pc.np_pckh_hits(pred, gt, thr, nk, kp0, kp1)
                np.testing.assert_array_equal(hits.cpu().numpy(), want)
    assert 0 < want.sum() < want.size * s  # (the data decide something)


def test_no_image_and_bad_arguments(dev):
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils import evaluation

    e = torch.zeros((0, 19, 2), device=dev)
    for call in (lambda: evaluation.compute_pckh(e, e, 0.5, 19), lambda: evaluation.compute_pckh_0_5([e], [e], 19),
                 lambda: evaluation.compute_pckh_figure(e[None], e[None], 19), lambda: evaluation.compute_pckh_figure([], [], 19)):
        with pytest.raises(ZeroDivisionError):
            call()
    assert _lib.pckh2d(e, e, (0.5, 1.0), 19).tolist() == [[0] * 19] * 2  # (the entry itself counts nothing)
    p = torch.zeros((4, 19, 2), device=dev)
    one = torch.zeros((4, 1, 2), device=dev)
    for bad in (lambda: _lib.pckh2d(one, one, (0.5,), 1), lambda: _lib.pckh2d(p, p, (0.5,), 19, 0, 19), lambda: _lib.pckh2d(p, p, (0.5,), 20),
                lambda: _lib.pckh2d(p, p, (0.5,), 0), lambda: _lib.pckh2d(p, p, (0.5,), 19, -1, 1), lambda: _lib.pckh2d(p, p[:3], (0.5,), 19),
                lambda: evaluation.compute_pckh(p, p[:3], 0.5, 19), lambda: evaluation.compute_pckh(p, p.cpu(), 0.5, 19)):
        with pytest.raises(_lib.MvalError):
            bad()
    torch.cuda.synchronize()


# ---- the decode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hh, wh", pc.DECODE_SIZES)
def test_pred_coordinates_equal_the_reference(dev, golden, hh, wh):
    from multi_view_active_learning_amd.utils import evaluation

    hm, boxes = pc.decode_case(hh, wh)
    got = evaluation.pred_coordinates_batch(torch.from_numpy(hm).to(dev), torch.from_numpy(boxes).to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 5, 2) and got.is_cuda
    want = golden[pc.decode_name(hh, wh) + "/xy"]
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # boxes from the host, a float64 copy of the maps: converted, same result
    again = evaluation.pred_coordinates_batch(torch.from_numpy(hm).to(dev).double(), boxes)
    assert torch.equal(again, got)


def test_pred_coordinates_nan_and_all_minus_inf_maps(dev):
    """NaN counts as the maximum (first NaN wins), an all -inf map decodes to index 0: the existing reduction's rules."""
    from multi_view_active_learning_amd.utils import evaluation

    hm, boxes = pc.decode_case(8, 6)
    hm[0, 0, 2, 3] = np.nan
    hm[0, 0, 6, 1] = np.nan
    hm[1, 2] = -np.inf
    got = evaluation.pred_coordinates_batch(torch.from_numpy(hm).to(dev), torch.from_numpy(boxes).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, pc.np_pred_coordinates(hm, boxes))
    assert got[1, 2].tolist() == [0.0, 0.0] and got[0, 0].tolist() == [np.float32(256.0 / 6.0) * 7.0, 32.0]  # flat 15 -> (15 % 8, 15 // 8)


@pytest.mark.parametrize("hh, wh", [(64, 64), (32, 16), (16, 16)])
def test_pred_coordinates_equal_the_stacked_get_pred_coordinates(dev, hh, wh):
    """``get_pred_coordinates`` is unchanged: N x J pairs of 0-d device tensors; stacked, they are the new function's output
    element for element.  The sizes are powers of two, square and not, for a reason that lies in torch and not in either
    function: ``get_pred_coordinates`` divides the box extent by the Python float ``1.0 * wh`` ON THE DEVICE, where torch
    multiplies by the scalar's reciprocal (exact only for a power of two), while the reference's numbers -- and the goldens of
    test_pred_coordinates_equal_the_reference, at 8 x 6, 64 x 48 and 96 x 72 too -- are a true float32 division."""
    from multi_view_active_learning_amd.utils import evaluation

    hm, boxes = pc.decode_case(hh, wh)
    hm_t, box_t = torch.from_numpy(hm).to(dev), torch.from_numpy(boxes).to(dev)
    old = evaluation.get_pred_coordinates(hm_t, box_t, hm.shape[1])
    assert isinstance(old, list) and len(old) == 3 and len(old[0]) == 5 and old[0][0][0].dim() == 0
    stacked = torch.stack([torch.stack([torch.stack(pair) for pair in img]) for img in old])
    got = evaluation.pred_coordinates_batch(hm_t, box_t)
    assert torch.equal(stacked, got)
    np.testing.assert_array_equal(got.cpu().numpy(), pc.np_pred_coordinates(hm, boxes))
    fewer = evaluation.get_pred_coordinates(hm_t, box_t, 2)  # num_keypoints below J: the first joints
    assert torch.equal(torch.stack([torch.stack([torch.stack(pair) for pair in img]) for img in fewer]), got[:, :2])


def test_keys_path_equals_the_maps_path_on_a_real_forward(dev, monkeypatch):
    """One forward of the smallest network case of the GPU tests (HRNet-W32, 3 images of 64 x 96, 5 joints: 16 x 24 maps, not
    square), whose plan keeps arg-max keys: decoding from the keys reads no map and gives the bits of the decode from the maps,
    and ``_compute_pred_labels`` takes the keys when the network kept them."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils import evaluation

    c = cases.model_cases()["w32_small"]
    m = cases.product_model(c)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.model_state_dict(c).items()}, strict=True)
    m = m.to(dev).eval()
    x = torch.from_numpy(cases.model_input(c)).to(dev)
    boxes = torch.tensor([[0.0, 0.0, 96.0, 96.0], [10.0, 20.0, 110.0, 180.0], [3.5, 7.25, 260.0, 263.75]])
    with torch.no_grad():
        hm = m(x)
    n, j, hh, wh = hm.shape
    assert (n, j, hh, wh) == (3, 5, 16, 24)
    keys = _lib.argmax_keys_of(hm)
    assert keys is not None and tuple(keys.shape) == (n, _lib.ARGMAX_SLOTS, j)
    from_maps = evaluation.pred_coordinates_batch(hm, boxes.to(dev))
    from_keys = evaluation.pred_coordinates_batch(hm, boxes.to(dev), keys=keys)
    assert torch.equal(from_keys, from_maps)
    np.testing.assert_array_equal(from_maps.cpu().numpy(), pc.np_pred_coordinates(hm.cpu().numpy(), boxes.numpy()))
    assert len(np.unique(from_maps.cpu().numpy().reshape(-1, 2), axis=0)) > 1  # (the forward's peaks are not all in one place)

    used = []
    real = _lib.pred_coordinates
    monkeypatch.setattr(_lib, "pred_coordinates", lambda h, b, k=None: (used.append(k is not None), real(h, b, k))[1])
    st = _strategy(**{"DATA.NUM_JOINTS": j})
    data = {"square_box": boxes.reshape(1, 3, 4)}
    assert torch.equal(st._compute_pred_labels(m, data, hm), from_maps) and used == [True]
    assert torch.equal(st._compute_pred_labels(m, data, hm.clone()), from_maps) and used == [True, False]  # a copy has no keys
    with pytest.raises(_lib.MvalError):
        _lib.pred_coordinates(hm, boxes.to(dev), keys[:2])


# ---- the pass and the metric switch ---------------------------------------------------------------------------------------------
def _pass_loader(dev):
    loader, maps = pc.pass_case()
    return [{k: torch.from_numpy(v) for k, v in dp.items()} for dp in loader], [torch.from_numpy(hm).to(dev) for hm in maps]


def test_evaluate_2d_pckh_equals_the_reference(dev, golden):
    """The fake model returns a plain HIP tensor (no keys): decode from the maps, one packed table, one counter launch."""
    st = _strategy()
    loader, maps = _pass_loader(dev)
    it = iter(maps)
    thresholds, pcks = st.evaluate_2d_pckh(loader, lambda images: next(it))
    assert thresholds == pc.THRESHOLDS
    np.testing.assert_array_equal(np.asarray(pcks), golden["pass/figure"])
    pred, gt = st._eval2d_tables
    assert tuple(pred.shape) == tuple(gt.shape) == (20, pc.J, 2) and pred.dtype == gt.dtype == torch.float32 and pred.is_cuda
    np.testing.assert_array_equal(gt.cpu().numpy(), np.concatenate([dp["2d_after_crop"].reshape(-1, pc.J, 2).numpy() for dp in loader]))
    it = iter(maps)
    thresholds, pcks = st.evaluate_2d_pckh(loader, lambda images: next(it), thresholds=(0.5,))
    assert thresholds == (0.5,)
    np.testing.assert_array_equal(np.asarray(pcks), golden["pass/pckh_0_5"][None])
    with pytest.raises(ZeroDivisionError):  # the reference's k / count over an empty loader
        st.evaluate_2d_pckh([], lambda images: next(it))


def _both_loader(dev):
    """The 3-D evaluation loader of the SAL cases (2 batches of 2 frames x 4 views, 64 x 64 maps) with the two keys the 2-D pass reads."""
    c = cases.sal_cases()["mpe"]
    loader, hms = cases.build_sal_loader(c)
    rng = np.random.default_rng(77)
    out = []
    for dp, hm in zip(loader, hms):
        b, v = dp["images"].shape[:2]
        lt = rng.integers(0, 40, (b, v, 2)).astype(np.float32)
        box = np.concatenate([lt, lt + np.float32(200.0)], axis=-1)
        place = pc.np_pred_coordinates(hm, box.reshape(-1, 4)).reshape(b, v, pc.J, 2)
        gt = (place + rng.standard_normal(place.shape) * 12.0).astype(np.float32)
        out.append({**{k: torch.from_numpy(a) for k, a in dp.items()}, "square_box": torch.from_numpy(box), "2d_after_crop": torch.from_numpy(gt)})
    return out, [torch.from_numpy(hm).to(dev) for hm in hms]


def test_evaluate_follows_eval_metric(dev):
    st = _strategy()
    loader, maps = _both_loader(dev)
    model = lambda: (lambda images, it=iter(maps): next(it))  # noqa: E731
    want2d = st.evaluate_2d_pckh(loader, model())
    assert 0.0 < np.asarray(want2d[1]).mean() < 1.0
    want_all = st.evaluate_all(loader, model())
    want_mkpe = st.evaluate_mkpe(loader, model()).item()
    assert want_all["mkpe"] == want_mkpe and "pckh_pcks" in want_all  # (DATA.TYPE panoptic)
    assert st.evaluate(loader, model(), metric="2DPCKH") == {"metric": "2DPCKH", "thresholds": want2d[0], "pcks": want2d[1]}
    assert st.evaluate(loader, model(), metric="3DPCK") == {"metric": "3DPCK", "thresholds": want_all["thresholds"], "pcks": want_all["pcks"],
                                                            "mkpe": want_mkpe}
    assert st.evaluate(loader, model(), metric="3DPCKH") == {"metric": "3DPCKH", "thresholds": want_all["pckh_thresholds"],
                                                             "pcks": want_all["pckh_pcks"], "mkpe": want_mkpe}
    assert st.evaluate(loader, model(), metric="MKPE") == {"metric": "MKPE", "thresholds": None, "pcks": None, "mkpe": want_mkpe}
    assert st.al_cfg.EVAL.METRIC == "3DPCK" and st.evaluate(loader, model())["metric"] == "3DPCK"  # metric=None reads EVAL.METRIC
    st.al_cfg.EVAL.METRIC = "2DPCKH"
    assert st.evaluate(loader, model()) == st.evaluate(loader, model(), metric="2DPCKH")
    st.al_cfg.EVAL.METRIC = "PCK"
    with pytest.raises(NotImplementedError):
        st.evaluate(loader, model())
    # evaluate_all is what it was: same dict again after the new passes ran on the same strategy object
    assert st.evaluate_all(loader, model()) == want_all


def test_pass_stages_its_inputs_before_the_network(dev, monkeypatch):
    """Inside a batch's side-stream body nothing goes host -> device or device -> host: ``square_box`` and ``2d_after_crop`` were
    staged with the small tensors before the network launch (a blocking copy there would hold up the next batch's network)."""
    from multi_view_active_learning_amd import parallel

    st = _strategy()
    loader, maps = _pass_loader(dev)
    it = iter(maps)
    inside, events = {"depth": 0}, []
    real_enter, real_exit = parallel.PostStream._Ctx.__enter__, parallel.PostStream._Ctx.__exit__
    monkeypatch.setattr(parallel.PostStream._Ctx, "__enter__", lambda self: (inside.__setitem__("depth", inside["depth"] + 1), real_enter(self))[1])
    monkeypatch.setattr(parallel.PostStream._Ctx, "__exit__", lambda self, *e: (inside.__setitem__("depth", inside["depth"] - 1), real_exit(self, *e))[1])
    for name in ("cpu", "item", "tolist", "numpy", "to", "cuda"):
        real = getattr(torch.Tensor, name)

        def f(self, *a, _real=real, _name=name, **k):
            if inside["depth"] > 0 and (self.is_cuda if _name in ("cpu", "item", "tolist", "numpy") else not self.is_cuda):
                events.append((_name, tuple(self.shape)))
            return _real(self, *a, **k)

        monkeypatch.setattr(torch.Tensor, name, f)
    st.evaluate_2d_pckh(loader, lambda images: next(it))
    assert events == [] and inside["depth"] == 0


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _frames():
    loader, maps = pc.pass_case()
    out = []
    for dp, hm in zip(loader, maps):
        b = dp["images"].shape[0]
        hm = hm.reshape((b, -1) + hm.shape[1:])
        out.extend(({k: v[i] for k, v in dp.items()}, hm[i]) for i in range(b))
    return out


def _rank_pass(frames, dev):
    loader = [{k: torch.from_numpy(np.stack([f[0][k] for f in frames[i:i + 2]])) for k in frames[0][0]} for i in range(0, len(frames), 2)]
    maps = iter([torch.from_numpy(np.concatenate([f[1] for f in frames[i:i + 2]])).to(dev) for i in range(0, len(frames), 2)])
    return _strategy().evaluate_2d_pckh(loader, lambda images: next(maps))


def _worker(rank, world, path, out):
    import sys

    for p in (REPO, os.path.join(REPO, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method="file://" + path)
    res = _rank_pass(_frames()[rank::world], torch.device("cuda:0"))  # DistributedSampler: indices[rank::world]
    torch.save(res, out + ".%d" % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_equal_one_rank(tmp_path, dev, golden):
    """Two processes share cuda:0 over gloo (as tests/test_gpu_distributed.py), strided shards of the pass case's five frames
    (3 + 2, so the last batches differ in size): one packed gather, and both ranks hold the one-rank (thresholds, pcks)."""
    sync, out = str(tmp_path / "sync"), str(tmp_path / "out")
    ctx = mp.spawn(_worker, args=(2, sync, out), nprocs=2, join=False)
    deadline = time.monotonic() + 240.0  # (each of the two processes ends by then, or is ended)
    try:
        while not ctx.join(timeout=5.0):
            assert time.monotonic() < deadline, "a rank did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    want = _rank_pass(_frames(), dev)
    np.testing.assert_array_equal(np.asarray(want[1]), golden["pass/figure"])
    for r in range(2):
        assert torch.load(out + ".%d" % r, weights_only=False) == want

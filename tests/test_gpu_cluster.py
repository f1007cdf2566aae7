"""GPU: the per-frame heat-map loss (csrc/frame_loss.hip: mval_frame_loss, mval_frame_loss_points) against float64
arithmetic, against itself under other batches, against the materialised ground truth and against the existing
single-frame entry; then the CLUSTER pass on the real reference's goldens (tests/golden/cluster.json), the POSE file
feeding the SAL clusters, and two ranks on one GPU.

Bound of the synthetic cases (derived, not measured): the float32 squares are torch's bit for bit, at most 2^20 float64
additions leave a relative error near 1e-10, one rounding to float32 follows -- so every value is the float64 reference
value rounded to float32, or its neighbour: at most 1 float32 ulp."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cluster_cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _ulps(a, b):
    """Distance in float32 steps between non-negative float32 arrays."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _maps(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.random(shape).astype(np.float32)
    h = (g + rng.standard_normal(shape).astype(np.float32) * rng.uniform(0.01, 1.0, shape[:2] + (1, 1)).astype(np.float32)).astype(np.float32)
    return h, g


def _reference(h, g, valid=None):
    """-> (per-map SSE (B, M) float64, per-frame value (B,) float64): float32(h - g), squared in float32, summed and
    divided in float64."""
    d = h - g
    sq = (d * d).astype(np.float32)
    per_map = sq.astype(np.float64).sum(axis=(2, 3))
    if valid is not None:
        per_map = per_map * (valid.reshape(per_map.shape) != 0)
    return per_map, per_map.sum(axis=1) / float(h.shape[2] * h.shape[3])


def _offset_by_one_float(t, dev):
    """The array on the device with its base one float past a 16-byte boundary."""
    buf = torch.empty(t.size + 1, dtype=torch.float32, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(torch.from_numpy(t))
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# ---- (a) against float64 ------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 5, 13),     # 65 pixels: a scalar tail, one map
          (3, 3, 7, 9),      # 63 pixels: less than a wave of groups, odd map bases
          (2, 5, 8, 8),
          (5, 7, 64, 48),
          (2, 38, 96, 72)]   # 6912 pixels: several trips of the workgroup


# a base one float past a 16-byte boundary (no float4 loads): of the heat-maps only, of both tensors
CASES = [(s, "aligned") for s in SHAPES] + [((2, 5, 8, 8), "h+1"), ((2, 5, 8, 8), "both+1"), ((3, 3, 7, 9), "both+1")]


@pytest.mark.parametrize("shape,offset", CASES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_frame_loss_within_one_ulp_of_float64(dev, shape, offset):
    from multi_view_active_learning_amd import _lib

    b, m, hh, wh = shape
    h, g = _maps(shape, hh * 31 + wh)
    th = _offset_by_one_float(h, dev) if offset != "aligned" else torch.from_numpy(h).to(dev)
    tg = _offset_by_one_float(g, dev) if offset == "both+1" else torch.from_numpy(g).to(dev)
    valid = (np.random.default_rng(5).random((b, m)) < 0.7).astype(np.uint8)
    valid[-1] = 0  # a fully masked frame
    for v in (None, valid):
        out, per_map = _lib.frame_loss(th, tg, None if v is None else torch.from_numpy(v).to(dev).reshape(-1), b, m, hh, wh)
        want_map, want = _reference(h, g, v)
        assert out.dtype == torch.float32 and out.shape == (b,) and per_map.dtype == torch.float64 and per_map.shape == (b * m,)
        assert _ulps(out.cpu().numpy(), want.astype(np.float32)).max() <= 1, (out.cpu().numpy(), want)
        np.testing.assert_allclose(per_map.cpu().numpy().reshape(b, m), want_map, rtol=1e-12, atol=0)
        if v is not None:
            assert out[-1].item() == 0.0 and _bits(out)[-1] == 0
            assert (per_map.cpu().numpy().reshape(b, m)[valid == 0] == 0.0).all()


def test_unaligned_and_aligned_bases_give_the_same_bits(dev):
    """The pixel -> lane assignment does not depend on whether float4 loads are possible."""
    from multi_view_active_learning_amd import _lib

    shape = (2, 5, 8, 8)
    h, g = _maps(shape, 77)
    a = _lib.frame_loss(torch.from_numpy(h).to(dev), torch.from_numpy(g).to(dev), None, 2, 5, 8, 8)
    u = _lib.frame_loss(_offset_by_one_float(h, dev), _offset_by_one_float(g, dev), None, 2, 5, 8, 8)
    np.testing.assert_array_equal(_bits(a[0]), _bits(u[0]))
    assert torch.equal(a[1], u[1])


def test_bad_arguments_are_refused(dev):
    from multi_view_active_learning_amd import _lib

    h = torch.zeros((1, 1, 4, 4), device=dev)
    assert _lib.frame_loss_workspace_bytes(3, 7) == 3 * 7 * 8 and _lib.frame_loss_workspace_bytes(0, 7) == 0
    with pytest.raises(_lib.MvalError):
        _lib.frame_loss(h, h, None, 1, 0, 4, 4)
    with pytest.raises(_lib.MvalError):
        _lib.frame_loss_points(h, torch.zeros((1, 2), dtype=torch.float64, device=dev), 0.0, None, 1, 1, 4, 4)
    out, _ = _lib.frame_loss(h, h, None, 0, 1, 4, 4)  # no frames: nothing launched
    assert out.shape == (0,)


# ---- (b) batch invariance -------------------------------------------------------------------------------------------------
def test_a_frame_scores_the_same_alone_and_in_any_batch(dev):
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError

    loss = Pose2DMeanSquaredError()
    h, g = _maps((5, 7, 64, 48), 11)
    th, tg = torch.from_numpy(h).to(dev).reshape(5, 1, 7, 64, 48), torch.from_numpy(g).to(dev).reshape(5, 1, 7, 64, 48)
    full = loss.pose_2d_mse_per_frame(th, tg)
    again = loss.pose_2d_mse_per_frame(th, tg)
    np.testing.assert_array_equal(_bits(full), _bits(again))
    alone = loss.pose_2d_mse_per_frame(th[2:3], tg[2:3])
    three = loss.pose_2d_mse_per_frame(th[1:4], tg[1:4])
    last = loss.pose_2d_mse_per_frame(th[0:3], tg[0:3])
    assert _bits(alone)[0] == _bits(three)[1] == _bits(last)[2] == _bits(full)[2]


# ---- (c) points form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1.0, 2.5])
@pytest.mark.parametrize("size", [(16, 12), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_points_form_equals_the_materialised_form_bit_for_bit(dev, size, sigma):
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError
    from multi_view_active_learning_amd.utils.preprocess import gt_heatmaps

    hh, wh = size
    b, v, j = 2, 2, 5
    rng = np.random.default_rng(hh + int(sigma * 10))
    pt = rng.random((b, v, j, 2)) * np.array([wh, hh], dtype=np.float64)
    pt[0, 0, 0] = (-3.25, hh + 7.5)        # outside the map
    pt[0, 0, 1] = (wh - 1.0, 0.0)          # on its border, an exact pixel centre
    pt[0, 0, 2] = (3.0, 5.0)               # an exact pixel centre
    pt[0, 0, 3] = (-0.5, hh - 0.5)         # half a pixel outside / on the last row's edge
    pt[1, 1, 4] = (1e4, -1e4)              # far outside: the map underflows to 0
    h = (rng.standard_normal((b, v, j, hh, wh)) * 0.4).astype(np.float32)
    th, tp = torch.from_numpy(h).to(dev), torch.from_numpy(pt).to(dev)
    loss = Pose2DMeanSquaredError()
    gt = gt_heatmaps(tp, sigma, hh, wh)
    assert gt.shape == (b, v, j, hh, wh)
    valid = torch.ones((b, 1, j), dtype=torch.uint8, device=dev)
    valid[1, 0, 2] = 0
    for jv in (valid, None):
        want = loss.pose_2d_mse_per_frame(th, gt, jv)
        got = loss.pose_2d_mse_per_frame_from_points(th, tp, sigma, jv)
        assert got.dtype == torch.float32 and got.shape == (b,)
        np.testing.assert_array_equal(_bits(got), _bits(want))
    # and the (unmasked) materialised form is what float64 arithmetic gives
    _, ref = _reference(h.reshape(b, v * j, hh, wh), gt.cpu().numpy().reshape(b, v * j, hh, wh))
    assert _ulps(want.cpu().numpy(), ref.astype(np.float32)).max() <= 1


def test_pass_on_batches_with_key_points_only(dev):
    """A batch without ``gt_heatmap`` (what prepare_views returns per frame, stacked): the loss against the maps of
    ``2d_keypoints / STRIDE`` with DATA.SIGMA, exactly the value against those maps materialised."""
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils.preprocess import gt_heatmaps

    b, v, j, hh, wh = 3, 2, 19, 16, 12
    rng = np.random.default_rng(3)
    kp = (rng.random((b, v, j, 2)) * np.array([wh * 4, hh * 4])).astype(np.float32)
    hm = (rng.standard_normal((b * v, j, hh, wh)) * 0.3).astype(np.float32)
    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = 4
    cfg.DATA.SIGMA = 1.5
    dp = {"images": torch.zeros(b, v, 3, 8, 8), "pose": torch.tensor([1, 1, 2]), "frame_id": torch.tensor([[4], [5], [6]]),
          "2d_keypoints": torch.from_numpy(kp)}
    st = ActiveLearningStrategy(cfg)
    got = st.cluster_dict([dp], lambda images: torch.from_numpy(hm).to(dev), "LOSS")
    gt = gt_heatmaps(torch.from_numpy(kp).to(dev).to(torch.float64) / 4, 1.5, hh, wh)
    want = st.loss.pose_2d_mse_per_frame(torch.from_numpy(hm).to(dev).reshape(b, v, j, hh, wh), gt).cpu().tolist()
    assert list(got.items()) == list(zip(["1-4", "1-5", "2-6"], want))


# ---- (d) the existing single-frame entry ------------------------------------------------------------------------------
def test_per_frame_agrees_with_pose_2d_mse_single_batch(dev):
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError

    loss = Pose2DMeanSquaredError()
    h, g = _maps((4, 6, 24, 20), 19)
    th, tg = torch.from_numpy(h).to(dev).reshape(4, 2, 3, 24, 20), torch.from_numpy(g).to(dev).reshape(4, 2, 3, 24, 20)
    got = loss.pose_2d_mse_per_frame(th, tg).cpu().numpy()
    single = np.array([loss.pose_2d_mse_single_batch(th[i], tg[i]).item() for i in range(4)], dtype=np.float32)
    assert _ulps(got, single).max() <= 1, (got, single)


# ---- (e) the reference's files --------------------------------------------------------------------------------------------
def _loss_pass(c, dev, loader=None, hms=None):
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    if loader is None:
        loader, hms = cluster_cases.build_cluster_loader(c)
    tl = [{k: torch.from_numpy(np.asarray(v)) for k, v in dp.items()} for dp in loader]
    it = iter(hms)
    cfg = get_default_configs()
    return ActiveLearningStrategy(cfg), tl, lambda images: torch.from_numpy(next(it)).to(dev)


@pytest.mark.parametrize("name", ["loss_v4_64x64", "loss_v2_64x48"])
def test_loss_file_vs_reference_golden(dev, name, tmp_path):
    """Keys and order are the reference's; each value is within (the reference's own recorded deviation from the float64
    value) + 1 float32 ulp of the reference's -- its float32 torch sum cannot be bit-equal to a float64 one."""
    from multi_view_active_learning_amd.utils import experiment_io

    with open(os.path.join(G, "cluster.json")) as f:
        gold = json.load(f)[name]
    want = json.loads(gold["text"])
    assert gold["deviation"] <= 2e-6
    st, tl, model = _loss_pass(cluster_cases.cluster_cases()[name], dev)
    st.al_cfg.AL.CLUSTER.SAVE_PATH = str(tmp_path / "loss.json")
    got = st.cluster(model, tl)
    assert list(got) == list(want)
    for g in want:
        value = gold["f64"][g]
        tol = gold["deviation"] * abs(value) + cluster_cases.ulp32(value)
        print(name, g, "ours %.9g reference %.9g float64 %.17g tolerance %.3g" % (got[g], want[g], value, tol))
        assert abs(got[g] - want[g]) <= tol, (g, got[g], want[g], tol)
        assert _ulps([got[g]], [np.float32(value)]).max() <= 1  # and the derived bound against the float64 value
        assert isinstance(got[g], float) and float(np.float32(got[g])) == got[g]
    assert list(experiment_io.read_cluster_losses(st.al_cfg.AL.CLUSTER.SAVE_PATH).items()) == list(got.items())


def test_pose_file_fits_the_sal_clusters(dev, tmp_path):
    """cluster() (POSE) -> file -> ``ActiveLearningStrategy.kmeans`` under SAL.CLUSTER_FILE_PATH: the centres of KMeans
    on the root-relative poses computed directly."""
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils.kmeans import KMeans

    c = cluster_cases.cluster_cases()["pose_j19"]
    loader, _ = cluster_cases.build_cluster_loader(c)
    cfg = get_default_configs()
    cfg.AL.CLUSTER.TYPE = "POSE"
    cfg.AL.CLUSTER.SAVE_PATH = str(tmp_path / "poses.json")
    ActiveLearningStrategy(cfg).cluster(None, [{k: torch.from_numpy(v) for k, v in dp.items()} for dp in loader])
    cfg.EXPR_TYPE = "SAL"
    cfg.SAL.CLUSTER_FILE_PATH = cfg.AL.CLUSTER.SAVE_PATH
    cfg.SAL.NUM_CLUSTERS = 3
    st = ActiveLearningStrategy(cfg)
    kp = np.concatenate([dp["3d_keypoints"] for dp in loader]).astype(np.float64)
    feats = (kp[:, 0:3] - kp[:, 0:3, 2:3]).reshape(len(kp), -1)
    direct = KMeans(3, random_state=cfg.RANDOM_SEED).fit(feats)
    assert st.kmeans.cluster_centers_.shape == (3, 57)
    assert np.array_equal(st.kmeans.cluster_centers_, direct.cluster_centers_)
    assert np.array_equal(st.kmeans.labels_, direct.labels_)


# ---- (f) two ranks on one GPU ----------------------------------------------------------------------------------------
def _frames(c):
    loader, hms = cluster_cases.build_cluster_loader(c)
    out = []
    for dp, hm in zip(loader, hms):
        b = dp["pose"].shape[0]
        hm = hm.reshape((b, -1) + hm.shape[1:])
        out.extend(({k: v[i] for k, v in dp.items()}, hm[i]) for i in range(b))
    return out


def _batches(frames, b):
    loader, hms = [], []
    for i in range(0, len(frames), b):
        chunk = frames[i:i + b]
        loader.append({k: np.stack([f[0][k] for f in chunk]) for k in chunk[0][0]})
        hms.append(np.concatenate([f[1] for f in chunk]))
    return loader, hms


def _rank_pass(c, frames):
    dev = torch.device("cuda:0")
    loader, hms = _batches(frames, 2)
    st, tl, model = _loss_pass(c, dev, loader, hms)
    return st.cluster_dict(tl, model, "LOSS")


def _worker(rank, world, path, out, c):
    import sys

    for p in (REPO, G):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method="file://" + path)
    torch.save(_rank_pass(c, _frames(c)[rank::world]), out + ".%d" % rank)  # DistributedSampler: indices[rank::world]
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_gpu_equal_one_rank(tmp_path):
    """Two processes share cuda:0 and talk over gloo (as tests/test_gpu_distributed.py): strided shards in batches of 2
    give exactly the one-rank dict -- a frame's loss does not depend on its batch, the gather restores dataset order."""
    c = cluster_cases.cluster_cases()["loss_v2_64x48"]
    sync, out = str(tmp_path / "sync"), str(tmp_path / "out")
    mp.spawn(_worker, args=(2, sync, out, c), nprocs=2, join=True)
    want = _rank_pass(c, _frames(c))
    assert len(want) == 5
    for r in range(2):
        got = torch.load(out + ".%d" % r, weights_only=False)
        assert list(got.items()) == list(want.items())

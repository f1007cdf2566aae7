"""CPU (no device): the CLUSTER pass (reference strategy.py:137-191) -- config fields, the POSE file against the real
reference's (tests/golden/cluster.json, byte for byte), the LOSS pass with its device stage stood in for by NumPy, the
two collectives of a pass under world 2 over gloo, and ``cluster()``'s restore and write.  The device stage itself and
the LOSS goldens run in tests/test_gpu_cluster.py."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cluster_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
J = 5


def _golden():
    with open(os.path.join(G, "cluster.json")) as f:
        return json.load(f)


def _cfg(**cluster):
    from multi_view_active_learning_amd.config import get_default_configs

    cfg = get_default_configs()
    for k, v in cluster.items():
        cfg.AL.CLUSTER[k] = v
    return cfg


def _torch_loader(loader):
    return [{k: torch.from_numpy(np.asarray(v)) for k, v in dp.items()} for dp in loader]


def _numpy_stages(cfg, loss_of_batch):
    """A strategy whose two device stages are stand-ins: the 'network' hands the batch's images on, the per-frame loss
    is ``loss_of_batch(dp)`` (float32 values)."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    class NumpyStages(ActiveLearningStrategy):
        @staticmethod
        def _compute_batch_heatmap(pose_estimator, data):
            return data["images"]

        def _frame_losses(self, heatmaps, dp):
            return torch.from_numpy(np.asarray(loss_of_batch(dp), dtype=np.float32))

    return NumpyStages(cfg)


# ---- config --------------------------------------------------------------------------------------------------------
def test_cluster_config_defaults_merge_and_unknown_type(tmp_path):
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    cfg = _cfg()
    assert (cfg.AL.CLUSTER.TYPE, cfg.AL.CLUSTER.SAVE_PATH, cfg.AL.CLUSTER.RESTORE_FROM) == ("LOSS", "", "")
    cfg.merge_from_list(["AL.CLUSTER.TYPE", "POSE", "AL.CLUSTER.SAVE_PATH", "/tmp/x.json", "AL.CLUSTER.RESTORE_FROM", "c.pth"])
    assert (cfg.AL.CLUSTER.TYPE, cfg.AL.CLUSTER.SAVE_PATH, cfg.AL.CLUSTER.RESTORE_FROM) == ("POSE", "/tmp/x.json", "c.pth")
    cfg._merge({"EXPR_TYPE": "CLUSTER", "AL": {"CLUSTER": {"TYPE": "LOSS"}}})
    assert cfg.EXPR_TYPE == "CLUSTER" and cfg.AL.CLUSTER.TYPE == "LOSS"
    with pytest.raises(KeyError):
        cfg.merge_from_list(["AL.CLUSTER.KIND", "POSE"])
    st = ActiveLearningStrategy(_cfg(TYPE="CLUSETER", SAVE_PATH=str(tmp_path / "never-written.json")))
    for call in (lambda: st.cluster_dict([]), lambda: st.cluster(None, []), lambda: st.cluster_dict([], cluster_type="HP")):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "'LOSS'" in str(e.value) and "'POSE'" in str(e.value)
    assert not os.path.exists(str(tmp_path / "never-written.json"))
    with pytest.raises(ValueError):
        ActiveLearningStrategy(_cfg(TYPE="POSE")).cluster(None, [])  # nowhere to write


# ---- POSE ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pose_j19", "pose_j42"])
def test_pose_file_equals_the_reference_file(name, tmp_path):
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils import experiment_io

    c = cluster_cases.cluster_cases()[name]
    text = _golden()[name]["text"]
    loader, _ = cluster_cases.build_cluster_loader(c)
    cfg = _cfg(TYPE="POSE", SAVE_PATH=str(tmp_path / "sub" / "poses.json"))
    cfg.DATA.NUM_JOINTS = c["j"]
    cfg.DATA.TYPE = "panoptic" if c["j"] == 19 else "ih26m"
    st = ActiveLearningStrategy(cfg)
    got = st.cluster_dict(_torch_loader(loader))
    want = json.loads(text)
    assert list(got) == list(want) and got == want
    assert st.cluster_dict(_torch_loader(loader), cluster_type="POSE") == got
    assert st.cluster(None, _torch_loader(loader)) == got  # (no estimator needed)
    with open(cfg.AL.CLUSTER.SAVE_PATH) as f:
        assert f.read() == text  # byte for byte
    kp = np.concatenate([dp["3d_keypoints"] for dp in loader]).astype(np.float64)
    root = st.joint_root_index
    rows = (kp[:, 0:3] - kp[:, 0:3, root:root + 1]).reshape(len(kp), -1)
    feats = experiment_io.read_cluster_features(cfg.AL.CLUSTER.SAVE_PATH, root)
    assert feats.shape == (5, 3 * c["j"]) and np.array_equal(feats, rows)


# ---- LOSS, device stage stood in for ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["loss_v4_64x64", "loss_v2_64x48"])
def test_loss_pass_keys_order_and_file_round_trip(name, tmp_path):
    from multi_view_active_learning_amd.utils import experiment_io

    c = cluster_cases.cluster_cases()[name]
    gold = _golden()[name]
    want = json.loads(gold["text"])
    loader, hms = cluster_cases.build_cluster_loader(c)
    it = iter(hms)
    st = _numpy_stages(_cfg(SAVE_PATH=str(tmp_path / "loss.json")),
                       lambda dp: cluster_cases.frame_loss_f64(next(it).reshape(dp["gt_heatmap"].shape), dp["gt_heatmap"].cpu().numpy()))  # (the pool loop stages the batch on the device where there is one)
    got = st.cluster(None, _torch_loader(loader))
    assert list(got) == list(want) == list(gold["f64"])
    for g, v in got.items():
        assert isinstance(v, float) and float(np.float32(v)) == v == float(np.float32(gold["f64"][g]))
    back = experiment_io.read_cluster_losses(str(tmp_path / "loss.json"))
    assert list(back.items()) == list(got.items())
    with open(str(tmp_path / "loss.json")) as f:
        assert f.read() == json.dumps(got)


def test_pass_rejects_ids_it_cannot_key():
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    st = ActiveLearningStrategy(_cfg(TYPE="POSE"))
    kp = torch.zeros(2, 4, 19)
    with pytest.raises(ValueError):
        st.cluster_dict([{"pose": torch.zeros(2, 2), "frame_id": torch.zeros(2), "3d_keypoints": kp}])
    with pytest.raises(ValueError):
        st.cluster_dict([{"pose": torch.zeros(3), "frame_id": torch.zeros(2), "3d_keypoints": kp}])


# ---- restore and write ------------------------------------------------------------------------------------------------
def test_cluster_restores_only_when_asked(tmp_path, monkeypatch):
    from multi_view_active_learning_amd.utils import experiment_io

    calls = []
    monkeypatch.setattr(experiment_io, "restore_checkpoint", lambda path, model, optimizer=None: calls.append((path, model)))

    class Model:
        evals = 0

        def eval(self):
            self.evals += 1

    loader = _host_loader(ALL[:3], 2, "B")
    for restore, kind, n in (("", "LOSS", 0), ("ckpt.pth", "LOSS", 1), ("ckpt.pth", "POSE", 0)):
        del calls[:]
        m = Model()
        st = _numpy_stages(_cfg(TYPE=kind, RESTORE_FROM=restore, SAVE_PATH=str(tmp_path / "out.json")), _host_losses)
        d = st.cluster(m, loader)
        assert len(calls) == n and m.evals == 1 and len(d) == 3
        if n:
            assert calls[0] == ("ckpt.pth", m)
    os.remove(str(tmp_path / "out.json"))
    st.cluster(m, loader, rank=1)  # only rank 0 writes
    assert not os.path.exists(str(tmp_path / "out.json"))


# ---- world 2 over gloo ------------------------------------------------------------------------------------------------
ALL = [(1, f) for f in range(7)] + [(2, f) for f in range(4)]  # 11 frames of two poses


def _host_pose(p, f):
    return (np.random.default_rng(1000 * p + f).standard_normal((4, J)) * 200.0).astype(np.float32)


def _host_loss(p, f):
    return np.float32(np.random.default_rng(7000 * p + f).random())


def _host_losses(dp):
    return [_host_loss(int(p), int(f)) for p, f in zip(dp["pose"].reshape(-1).tolist(), dp["frame_id"].reshape(-1).tolist())]


def _host_loader(frames, batch, ids):
    out = []
    for i in range(0, len(frames), batch):
        chunk = frames[i:i + batch]
        shape = (-1,) if ids == "B" else (-1, 1)
        out.append({"pose": torch.tensor([p for p, _ in chunk]).reshape(shape), "frame_id": torch.tensor([f for _, f in chunk]).reshape(shape),
                    "images": torch.zeros(len(chunk), 1, 3, 4, 4),
                    "3d_keypoints": torch.from_numpy(np.stack([_host_pose(p, f) for p, f in chunk]))})
    return out


def _host_pass(frames, kind, ids, save, rank=0):
    cfg = _cfg(TYPE=kind, SAVE_PATH=save)
    cfg.DATA.NUM_JOINTS = J
    return _numpy_stages(cfg, _host_losses).cluster(None, _host_loader(frames, 2, ids), rank=rank)


def _shard(mode, rank, world):
    from multi_view_active_learning_amd import parallel

    if mode == "strided":   # DistributedSampler
        return ALL[rank::world]
    if mode == "blocks":    # contiguous blocks, a short last rank with a short last batch
        lo, hi = parallel.shard_range(len(ALL), rank, world)
        return ALL[lo:hi]
    return ALL if rank == 0 else []  # "empty": rank 1 has nothing and still takes part


def _worker(rank, world, path, out):
    import sys

    for p in (REPO, G):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method="file://" + path)
    calls = []
    real, real_list = dist.all_gather_into_tensor, dist.all_gather
    dist.all_gather_into_tensor = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    dist.all_gather = lambda *a, **k: (calls.append(1), real_list(*a, **k))[1]
    res = {}
    for mode in ("strided", "blocks", "empty"):
        for kind in ("LOSS", "POSE"):
            n0 = len(calls)
            save = "%s.%s.%s.r%d" % (out, mode, kind, rank)
            d = _host_pass(_shard(mode, rank, world), kind, "B1" if kind == "POSE" else "B", save, rank=rank)
            res[mode, kind] = {"dict": d, "collectives": len(calls) - n0, "wrote": os.path.exists(save)}
    dist.all_gather_into_tensor, dist.all_gather = real, real_list
    torch.save(res, out + ".%d" % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_build_the_one_rank_dict_with_two_collectives(tmp_path):
    sync, out = str(tmp_path / "sync"), str(tmp_path / "out")
    mp.spawn(_worker, args=(2, sync, out), nprocs=2, join=True)
    got = [torch.load(out + ".%d" % r, weights_only=False) for r in range(2)]
    a, b = ALL[:6], ALL[6:]
    blocks_order = ["%d-%d" % blk[i + s] for i in range(0, 6, 2) for s in range(2) for blk in (a, b) if i + s < len(blk)]
    for kind in ("LOSS", "POSE"):
        want = _host_pass(ALL, kind, "B", str(tmp_path / "one"))
        assert list(want) == ["%d-%d" % x for x in ALL]
        first = want["1-0"]
        assert first == (float(_host_loss(1, 0)) if kind == "LOSS" else _host_pose(1, 0).tolist())
        for mode in ("strided", "blocks", "empty"):
            for r in range(2):
                g = got[r][mode, kind]
                assert g["collectives"] == 2, (mode, kind, r)
                assert g["wrote"] == (r == 0)
                assert dict(g["dict"]) == dict(want), (mode, kind, r)  # every frame once, every value exact
                assert list(g["dict"]) == (blocks_order if mode == "blocks" else list(want)), (mode, kind, r)
        with open("%s.strided.%s.r0" % (out, kind)) as f:
            assert f.read() == json.dumps(want)

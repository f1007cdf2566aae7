"""Generate the golden vectors under tests/golden/ by running the REAL reference.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden.py

Inputs are regenerated from seeds by ``multi_view_active_learning_amd.synth`` on both
sides, so the fixtures hold (almost) only *expected outputs* plus the library versions
they were produced with.  Nothing of the reference's source is stored.

What is pinned:
  triangulation_reftest.npz  the reference's own test input (tests/test_triangulation.py:15-69)
  triangulation_synth.npz    ring cameras, V in {2,4,8}, square / non-square maps, invalid joints, outlier views
  triangulation_xe.npz       use_reprojection_xe=True (utils/triangulation.py:236-257)
  triangulation_edges.npz    V in {5,6,7,9,10,11} (every lane-group size of the device kernel), J = 130 and 512 at V = 2
  scoring.npz                _compute_hp/_compute_mpe/_compute_bsb AVG+STD (strategy.py:1149-1215)
  sal_dict.json              _compute_sal_dict over a 2-batch loader for HP/TRIANGULATION/CORESET/MPE + nlargest picks
  coreset.npz                CoreSet.select_batch picks (+ boundary gaps from the restatement)
  models.npz                 eval heat-maps of HRNet-W32 / W48 / PoseResNet-50 with synthetic weights
  train_step.npz             train-mode loss, gradient norms, BN running stats after one step
  pck.npz                    compute_3d_pck_figure / compute_3d_pckh_figure (utils/evaluation.py:121-195)
  sal_filter.json            _sal_pseudo_labeling (strategy.py:915-1001): AL picks + pseudo-label filter (clusters / random.sample)
  preprocess.npz             prepare_single_view (dataset/dataset.py:158-220): crop / LANCZOS resize / normalise / GT heat-maps
  formats.json               the files sample_next_batch / restore_dataset / _save_checkpoints write and read
                             (strategy.py:54-135,314-337,681-743): exact JSON texts + checkpoint structure
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

import torch  # noqa: E402

from multi_view_active_learning_amd import synth  # noqa: E402
from oracle import coreset as ocoreset  # noqa: E402
from oracle import ref_harness  # noqa: E402

import cases  # noqa: E402  (tests/golden/cases.py: shared case definitions)


def versions():
    import scipy
    import sklearn

    return json.dumps(
        dict(numpy=np.__version__, torch=torch.__version__, sklearn=sklearn.__version__, scipy=scipy.__version__)
    )


def capture_reference_test_input(ns):
    """Run the reference's own tests/test_triangulation.py with ``triangulation`` patched
    to record its arguments: the projection matrices / heat-maps that test holds are
    captured as DATA into reftest_input.npz (no source text is stored)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "_ref_test_triangulation", os.path.join(ref_harness.REFERENCE_ROOT, "tests", "test_triangulation.py")
    )
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = {}

    def spy(heatmaps, proj, stride, valid, *a, **k):
        got.update(heatmaps=heatmaps.numpy().copy(), proj=proj.numpy().copy(), stride=stride, valid=valid.numpy().copy())
        return ns.triangulation.triangulation(heatmaps, proj, stride, valid, *a, **k)

    mod.triangulation = spy
    import contextlib
    import io

    with contextlib.redirect_stdout(io.StringIO()):
        mod.TestTriangulation("test_triangulation").test_triangulation()
    np.savez_compressed(
        os.path.join(HERE, "reftest_input.npz"),
        heatmaps=got["heatmaps"], proj=got["proj"], stride=np.int64(got["stride"]), valid=got["valid"],
    )


def gen_triangulation(ns):
    tri = ns.triangulation.triangulation
    capture_reference_test_input(ns)
    # (1) the reference's own test input
    proj, hm, valid, stride = cases.reference_test_input()
    r = tri(torch.from_numpy(hm), torch.from_numpy(proj), stride, torch.from_numpy(valid))
    np.savez(
        os.path.join(HERE, "triangulation_reftest.npz"),
        keypoints_2d=r["keypoints_2d"], keypoints_3d=r["keypoints_3d"], metric=np.float64(r["metric"]),
        inlier_count=np.int64(r["inlier_count"]), versions=versions(),
    )
    print("reftest kp3d[0]", r["keypoints_3d"][0], "metric", r["metric"], "inliers", r["inlier_count"])
    # (2) synthetic cases
    out = {}
    for name, c in cases.triangulation_cases().items():
        hm, proj, valid = cases.build_triangulation_case(c)
        k2, k3, me, ic = [], [], [], []
        for b in range(hm.shape[0]):
            r = tri(torch.from_numpy(hm[b]), torch.from_numpy(proj[b]), c["stride"], torch.from_numpy(valid[b]))
            k2.append(r["keypoints_2d"]); k3.append(r["keypoints_3d"]); me.append(r["metric"]); ic.append(r["inlier_count"])
        out[name + "/keypoints_2d"] = np.stack(k2)
        out[name + "/keypoints_3d"] = np.stack(k3)
        out[name + "/metric"] = np.asarray(me, dtype=np.float64)
        out[name + "/inlier_count"] = np.asarray(ic, dtype=np.int64)
        print(name, "inliers", ic, "metric", np.round(me, 4))
    np.savez(os.path.join(HERE, "triangulation_synth.npz"), versions=versions(), **out)
    # (3) XE metric
    out = {}
    for name, c in cases.xe_cases().items():
        hm, proj, valid = cases.build_triangulation_case(c)
        me = []
        for b in range(hm.shape[0]):
            r = tri(torch.from_numpy(hm[b]), torch.from_numpy(proj[b]), c["stride"], torch.from_numpy(valid[b]),
                    False, True, c["sigma"])
            me.append(float(r["metric"]))
        out[name + "/metric"] = np.asarray(me, dtype=np.float64)
        print(name, "xe", me)
    np.savez(os.path.join(HERE, "triangulation_xe.npz"), versions=versions(), **out)


def gen_triangulation_edges(ns):
    """cases.triangulation_edge_cases() -> triangulation_edges.npz (outputs only, like triangulation_synth.npz)."""
    tri = ns.triangulation.triangulation
    out = {}
    for name, c in cases.triangulation_edge_cases().items():
        hm, proj, valid = cases.build_triangulation_case(c)
        k2, k3, me, ic = [], [], [], []
        for b in range(hm.shape[0]):
            r = tri(torch.from_numpy(hm[b]), torch.from_numpy(proj[b]), c["stride"], torch.from_numpy(valid[b]))
            k2.append(r["keypoints_2d"]); k3.append(r["keypoints_3d"]); me.append(r["metric"]); ic.append(r["inlier_count"])
        out[name + "/keypoints_2d"] = np.stack(k2)
        out[name + "/keypoints_3d"] = np.stack(k3)
        out[name + "/metric"] = np.asarray(me, dtype=np.float64)
        out[name + "/inlier_count"] = np.asarray(ic, dtype=np.int64)
        print(name, "inliers", ic, "metric", np.round(me, 4))
    np.savez_compressed(os.path.join(HERE, "triangulation_edges.npz"), versions=versions(), **out)


def gen_scoring(ns):
    out = {}
    for name, c in cases.scoring_cases().items():
        hm, valid = cases.build_scoring_case(c)
        for kind in ("HP", "MPE", "BSB"):
            for cfgk in ("AVG", "STD"):
                st = ref_harness.make_strategy(kind, **{f"AL.{kind}_CONFIG": cfgk})
                fn = {"HP": st._compute_hp, "MPE": st._compute_mpe, "BSB": st._compute_bsb}[kind]
                vals = []
                for b in range(hm.shape[0]):
                    v = fn(torch.from_numpy(hm[b]), torch.from_numpy(valid[b]))
                    # what the reference then does: torch.tensor(v) (strategy.py:1077-1090)
                    t = torch.tensor(v)
                    vals.append((float(t.item()), str(t.dtype)))
                out[f"{name}/{kind}_{cfgk}"] = np.asarray([v[0] for v in vals], dtype=np.float64)
                out[f"{name}/{kind}_{cfgk}_dtype"] = vals[0][1]
        print(name, {k: out[k] for k in out if k.startswith(name) and not k.endswith("dtype")})
    np.savez(os.path.join(HERE, "scoring.npz"), versions=versions(), **out)


def gen_sal_dict(ns):
    res = {"versions": versions()}
    for name, c in cases.sal_cases().items():
        loader, heatmaps = cases.build_sal_loader(c)
        it = iter(heatmaps)

        def fake_model(images):
            return torch.from_numpy(next(it))

        st = ref_harness.make_strategy(
            c["strategy"],
            **{"POSE_ESTIMATOR.STRIDE": c["stride"], "AL.USE_SOFTARGMAX": c.get("soft", False),
               "AL.USE_REPROJECTION_XE": c.get("xe", False), "AL.REPROJECTION_SIGMA": c.get("sigma", 1.0)},
        )
        torch_loader = [{k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in dp.items()} for dp in loader]
        sal = st._compute_sal_dict(torch_loader, fake_model)
        entry = {k: {g: v for g, v in d.items()} for k, d in sal.items()}
        import math
        from heapq import nlargest

        alm = {g: m for g, m in sal["al_metric"].items() if not math.isnan(m)}
        entry["nlargest"] = nlargest(c["select"], alm, key=alm.get)
        res[name] = entry
        print(name, "keys", list(sal["al_metric"].keys())[:3], "al", list(sal["al_metric"].values())[:3], "pick", entry["nlargest"])
    with open(os.path.join(HERE, "sal_dict.json"), "w") as f:
        json.dump(res, f)


def gen_coreset(ns):
    out = {}
    import contextlib
    import io

    for name, c in cases.coreset_cases().items():
        sal, al = cases.build_coreset_case(c)
        with contextlib.redirect_stdout(io.StringIO()):
            cs = ns.coreset.CoreSet(sal, al, c["root"])
            picks = cs.select_batch(c["select"])
        o = ocoreset.CoreSet(sal, al, c["root"])
        opicks = o.select_batch(c["select"])
        assert picks == opicks, (name, picks[:5], opicks[:5])
        key_index = {k: i for i, k in enumerate(sal.keys())}
        picks = [key_index[k] for k in picks]  # stored as pool row indices
        out[name + "/picks"] = np.asarray(picks, dtype=np.int64)
        out[name + "/gaps"] = np.asarray(o.gaps, dtype=np.float64)
        out[name + "/final_min_distances"] = np.asarray(cs.min_distances, dtype=np.float64).ravel()[:: max(1, cs.n_obs // 64)]
        print(name, picks[:8], "min gap", min(o.gaps))
    # the reference's own degenerate test (tests/test_coreset.py:15-18): duplicates allowed
    sal = {i: [[0, 1, 2] for _ in range(19)] for i in range(20)}
    al = {i: [[0, 1, 2] for _ in range(19)] for i in range(5)}
    with contextlib.redirect_stdout(io.StringIO()):
        picks = ns.coreset.CoreSet(sal, al, 2).select_batch(5)
    out["reftest/picks"] = np.asarray(picks, dtype=np.int64)
    print("reftest picks", picks)
    np.savez(os.path.join(HERE, "coreset.npz"), versions=versions(), **out)


def gen_models(ns):
    out = {}
    for name, c in cases.model_cases().items():
        model = cases.build_reference_model(ns, c)
        x = cases.model_input(c)
        with torch.no_grad():
            y = model.eval()(torch.from_numpy(x)).numpy()
        out[name + "/heatmaps0"] = y[0]  # first image in full
        flat = y.reshape(y.shape[0], y.shape[1], -1)
        out[name + "/argmax"] = flat.argmax(-1).astype(np.int64)
        top2 = np.sort(flat, axis=-1)[..., -2:]
        out[name + "/margin"] = (top2[..., 1] - top2[..., 0]).astype(np.float32)
        out[name + "/mean"] = flat.mean(-1).astype(np.float32)
        out[name + "/max"] = flat.max(-1).astype(np.float32)
        print(name, y.shape, "std", y.std(), "min margin", out[name + "/margin"].min())
    np.savez(os.path.join(HERE, "models.npz"), versions=versions(), **out)


def gen_train(ns):
    out = {}
    for name, c in cases.train_cases().items():
        model = cases.build_reference_model(ns, c).train()
        x, gt, valid = cases.train_input(c)
        loss_fn = ns.loss.Pose2DMeanSquaredError()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        opt.zero_grad()
        hm = model(torch.from_numpy(x))
        loss = loss_fn.pose_2d_mse(hm, torch.from_numpy(gt), torch.from_numpy(valid).reshape(hm.shape[0], -1, 1, 1).bool())
        loss.backward()
        out[name + "/loss"] = np.float32(loss.item())
        named = dict(model.named_parameters())
        for k in c["grad_keys"]:
            out[name + "/grad_norm/" + k] = np.float64(named[k].grad.double().norm().item())
            out[name + "/grad_head/" + k] = named[k].grad.reshape(-1)[:16].numpy().copy()
        sd = model.state_dict()
        for k in c["bn_keys"]:
            out[name + "/running_mean/" + k] = sd[k + ".running_mean"].numpy().copy()
            out[name + "/running_var/" + k] = sd[k + ".running_var"].numpy().copy()
        opt.step()
        named = dict(model.named_parameters())
        for k in c["grad_keys"]:
            out[name + "/after_step_head/" + k] = named[k].detach().reshape(-1)[:16].numpy().copy()
        out[name + "/heatmaps_head"] = hm.detach().reshape(-1)[:64].numpy().copy()
        print(name, "loss", loss.item())
    np.savez(os.path.join(HERE, "train_step.npz"), versions=versions(), **out)


def gen_pck(ns):
    """compute_3d_pck_figure / compute_3d_pckh_figure (utils/evaluation.py:121-195) with their default
    thresholds, plus the mm thresholds 10..150 the panoptic-scale noise needs."""
    out = {}
    ev = ns.evaluation
    for name, c in cases.pck_cases().items():
        pred, gt, valid = cases.pck_arrays(c)
        pl, gl, vl = [torch.from_numpy(p) for p in pred], [torch.from_numpy(g) for g in gt], [torch.from_numpy(v) for v in valid]
        for tag, thr in (("pck", (1, 2, 3, 4, 5)), ("pck_wide", (10, 25, 50, 100, 150))):
            t, pcks = ev.compute_3d_pck_figure(pl, gl, vl, c["j"], thresholds=thr)
            out[f"{name}/{tag}"] = np.asarray(pcks, dtype=np.float64)
        t, pcks = ev.compute_3d_pckh_figure(pl, gl, c["j"])
        out[f"{name}/pckh"] = np.asarray(pcks, dtype=np.float64)
        out[f"{name}/pckh_thresholds"] = np.asarray(t, dtype=np.float64)
    np.savez(os.path.join(HERE, "pck.npz"), versions=versions(), **out)


def gen_preprocess(ns):
    """The reference's own ``ActiveLearningDataset.prepare_single_view`` (dataset/dataset.py:158-220) run
    unbound on an in-memory PNG per case: normalised image, projection matrix, 2-D key points and the
    Gaussian ground-truth heat-maps."""
    import io
    import types

    from dataset import dataset as ref_ds  # type: ignore  (reference module, harness path)
    from PIL import Image

    out = {}
    for name, c in cases.preprocess_cases().items():
        img, kp3d, cam = cases.preprocess_inputs(c)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        fake = types.SimpleNamespace(
            _pathmgr=types.SimpleNamespace(open=lambda path, mode: io.BytesIO(buf.getvalue())),
            _logger=types.SimpleNamespace(debug=lambda *a, **k: None),
            data_cfg=types.SimpleNamespace(SCALE_BBOX=c["scale"], INPUT_WIDTH=c["in_w"], INPUT_HEIGHT=c["in_h"]),
            gt_stride=c["stride"], split="val", augmentation=None)
        view = {"path": "mem.png", "box": list(c["box"]), "camera": cam, "camera_name": "cam0"}
        v = ref_ds.ActiveLearningDataset.prepare_single_view(fake, view, kp3d, c["sigma"])
        out[f"{name}/images"] = v["images"].numpy()
        out[f"{name}/gt_heatmap"] = v["gt_heatmap"].numpy()
        out[f"{name}/proj_matrices"] = v["proj_matrices"].numpy()
        out[f"{name}/2d_keypoints"] = v["2d_keypoints"].numpy()
        out[f"{name}/2d_after_crop"] = v["2d_after_crop"].numpy()
        out[f"{name}/square_box"] = v["square_box"].numpy()
    import PIL

    np.savez_compressed(os.path.join(HERE, "preprocess.npz"), versions=versions(), pillow=PIL.__version__, **out)


def gen_sal_filter(ns):
    """The reference's ``_sal_pseudo_labeling`` (strategy.py:915-1001) run unbound on a fake strategy /
    dataset around a prepared sal_dict: AL picks, then the pseudo-label filter with KMeans cluster balancing
    (centres fitted here and stored) or ``random.sample`` (python's RNG seeded with the case seed)."""
    import random
    import types

    from sklearn.cluster import KMeans

    out = {"versions": versions()}
    for name, c in cases.sal_filter_cases().items():
        sal, done = cases.sal_filter_inputs(c)
        cfg = ns.config.get_cfg_defaults() if hasattr(ns.config, "get_cfg_defaults") else ns.config._C.clone()
        cfg.AL.STRATEGY = "HP"
        cfg.EXPR_TYPE = "SAL"
        cfg.SAL.INLIER_THRESHOLD = c["thr"]
        cfg.SAL.NUM_CLUSTERS = c["clusters"]
        cfg.SAL.CLUSTER_FILE_PATH = "fitted-in-the-generator" if c["use_clusters"] else ""
        root = 2
        feats = []
        for g in sal["pred_3d_keypoints"]:
            kp = np.array(sal["pred_3d_keypoints"][g]).T
            feats.append((kp[0:3, :] - kp[0:3, root : root + 1]).flatten())
        km = KMeans(n_clusters=c["clusters"], n_init=3, random_state=c["seed"]).fit(np.asarray(feats))
        labelled = {}

        class FakeDataset:
            pseudo_label_guids = list(done)

            def resample_unlabeled_data(self):
                pass

            def get_al_dict_for_coreset(self):
                return {}

            def label_by_frame_guids(self, guids):
                labelled["al"] = list(guids)

            def pseudo_label_by_frame_guids(self, guids, preds):
                labelled["sal"] = list(guids)

        fake = types.SimpleNamespace(
            al_cfg=cfg, joint_root_index=root, kmeans=km,
            _logger=types.SimpleNamespace(info=lambda *a, **k: None),
            _get_dataloader=lambda *a, **k: None, _compute_sal_dict=lambda *a, **k: sal)
        random.seed(c["seed"])
        _, al_guids, sal_guids, _ = ns.strategy.ActiveLearningStrategy._sal_pseudo_labeling(
            fake, FakeDataset(), c["al_num"], c["pseudo_num"], None)
        out[name] = dict(al_guids=list(al_guids), sal_guids=list(sal_guids), centers=km.cluster_centers_.tolist())
    with open(os.path.join(HERE, "sal_filter.json"), "w") as f:
        json.dump(out, f)


def _structure(state_dict):
    return [[k, list(v.shape), str(v.dtype)] for k, v in state_dict.items()]


def gen_formats(ns):
    """The on-disk side of an experiment, produced by the reference's own writers (strategy.py:54-135 rank-0 branch
    of ``sample_next_batch``; ``restore_dataset`` :314-337; ``_save_checkpoints`` / ``_load_weights`` :681-743) into
    a temporary directory.  Stored: the exact texts of the three JSON files for a real ``_compute_sal_dict`` result,
    what ``restore_dataset`` hands to the dataset, and the STRUCTURE (names / shapes / dtypes / hyper-parameters) of
    a checkpoint -- plus whether the reference's loader accepts a checkpoint written by this repo's writer and the
    other way round (both checked live here, where both implementations can be imported)."""
    import hashlib
    import shutil
    import tempfile
    import types

    from multi_view_active_learning_amd.pose_estimators import PoseHighResolutionNet, PoseResNet
    from multi_view_active_learning_amd.utils import experiment_io as eio

    tmp = tempfile.mkdtemp(prefix="mval_formats_")
    out = {"versions": versions()}
    try:
        c = cases.sal_cases()["hp"]
        loader, heatmaps = cases.build_sal_loader(c)
        it = iter(heatmaps)
        st = ref_harness.make_strategy("HP", **{"POSE_ESTIMATOR.STRIDE": c["stride"], "LOG_DIR": tmp, "EXPR_NAME": "expr",
                                                "EXPR_TYPE": "SAL"})
        st._pathmgr = types.SimpleNamespace(open=open, isfile=os.path.isfile, rm=os.remove, isdir=os.path.isdir,
                                            mkdirs=os.makedirs)
        st.al_writer = types.SimpleNamespace(add_histogram=lambda *a, **k: None, add_scalar=lambda *a, **k: None)
        os.makedirs(os.path.join(tmp, "expr"))
        torch_loader = [{k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in dp.items()} for dp in loader]
        sal = st._compute_sal_dict(torch_loader, lambda images: torch.from_numpy(next(it)))
        guids = list(sal["al_metric"].keys())
        seed_guids = ["900-1", "901-4"]  # iteration 0: the random seed batch
        al_guids, sal_guids = guids[1:3], guids[3:4]
        st._random_sample_frames = lambda ds, n: (ds, seed_guids)
        st._sal_pseudo_labeling = lambda ds, a, s, pe: (ds, al_guids, sal_guids, sal)
        st.sample_next_batch(None, 2, 0, None, 0, rank=0)
        st.sample_next_batch(None, 2, 1, None, 1, rank=0)
        files = {}
        for name in sorted(os.listdir(os.path.join(tmp, "expr"))):
            with open(os.path.join(tmp, "expr", name)) as f:
                files[name] = f.read()
        out["files"] = files
        out["seed_guids"], out["al_guids"], out["sal_guids"] = seed_guids, al_guids, sal_guids

        calls = []

        class FakeDataset:
            labeled_data = {}
            pseudo_label_guids = None

            def label_by_frame_guids(self, g):
                calls.append(list(g))

        ds = st.restore_dataset(FakeDataset(), 2)
        out["restore"] = dict(labeled=calls, pseudo=ds.pseudo_label_guids)

        # ---- checkpoints: structure of what the reference writes, and cross-loading ---------------------------
        ck = {}
        for kind, ref_model, our_model in (
            ("POSE_RESNET", ns.pose_resnet.PoseResNet(19, 50), PoseResNet(19, 50)),
            ("HRNET", ns.hrnet.PoseHighResolutionNet(19), PoseHighResolutionNet(19)),
        ):
            def stepped_adam(model):
                opt = torch.optim.Adam(model.parameters(), lr=1e-3)  # strategy.py:405
                for p in model.parameters():
                    p.grad = torch.zeros_like(p)
                opt.step()
                return opt

            os.makedirs(os.path.join(tmp, "ck"), exist_ok=True)
            ref_path = st._save_checkpoints(os.path.join(tmp, "ck"), 3, 17, ref_model, stepped_adam(ref_model))
            blob = torch.load(ref_path)
            opt_sd = blob["optimizer"]
            lines = "".join("%s:%s:%s\n" % (k, list(v.shape), v.dtype) for k, v in blob["state_dict"].items())
            entry = dict(
                file=os.path.basename(ref_path),
                top_keys=list(blob.keys()), epoch=blob["epoch"], global_step=blob["global_step"],
                state_dict_sha256=hashlib.sha256(lines.encode()).hexdigest(), n_entries=len(blob["state_dict"]),
                param_group_keys=sorted(opt_sd["param_groups"][0].keys()),
                optimizer_state_keys=sorted(opt_sd["state"][0].keys()),
                n_optimizer_params=len(opt_sd["param_groups"][0]["params"]),
            )
            if kind == "POSE_RESNET":
                entry["state_dict"] = _structure(blob["state_dict"])
            # ours -> reference loader (strict), reference -> our loader (strict)
            our_path = eio.save_checkpoint(os.path.join(tmp, "ck_ours"), 3, 17, our_model, stepped_adam(our_model))
            cfg = st.al_cfg.clone()
            cfg.TRAIN.RESTORE_FROM = our_path
            st._load_weights(cfg, ref_model)
            def same(a, b):
                a, b = a.state_dict(), b.state_dict()
                return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)

            entry["reference_loads_ours"] = same(ref_model, our_model)
            fresh = type(our_model)(19) if kind == "HRNET" else type(our_model)(19, 50)
            entry["ours_loads_reference"] = eio.load_weights(fresh, restore_from=ref_path) == "restored" and all(
                torch.equal(v, blob["state_dict"][k]) for k, v in fresh.state_dict().items())
            ck[kind] = entry
            print(kind, entry["file"], entry["n_entries"], "ref<-ours", entry["reference_loads_ours"], "ours<-ref",
                  entry["ours_loads_reference"])
        out["checkpoint"] = ck
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(HERE, "formats.json"), "w") as f:
        json.dump(out, f)


def main():
    ns = ref_harness.load()
    which = sys.argv[1:] or ["tri", "tri_edges", "scoring", "sal", "coreset", "models", "train", "pck", "preprocess", "sal_filter", "formats"]
    if "formats" in which:
        gen_formats(ns)
    if "pck" in which:
        gen_pck(ns)
    if "preprocess" in which:
        gen_preprocess(ns)
    if "sal_filter" in which:
        gen_sal_filter(ns)
    if "tri" in which:
        gen_triangulation(ns)
    if "tri_edges" in which:
        gen_triangulation_edges(ns)
    if "scoring" in which:
        gen_scoring(ns)
    if "sal" in which:
        gen_sal_dict(ns)
    if "coreset" in which:
        gen_coreset(ns)
    if "models" in which:
        gen_models(ns)
    if "train" in which:
        gen_train(ns)


if __name__ == "__main__":
    main()

"""Generate tests/golden/cluster.json: the files the REAL reference's ``ActiveLearningStrategy.cluster()``
(strategy.py:137-191) writes for the cases of cluster_cases.py.

Run in the build container only (needs the reference tree):

    python tests/golden/make_cluster_golden.py

The reference's function is run as it is; what it needs around it is stubbed: ``_get_dataloader`` returns the case's
batches, the dataset only has ``label_all`` / ``resample_frames``, AL.CLUSTER.RESTORE_FROM (which the reference's
config.py does not define) is set on the config, the estimator replays the case's heat-maps and accepts the one-key
checkpoint.  ``pose`` / ``frame_id`` are fed in the only layouts the reference's indexing (strategy.py:165-169,177-186)
runs on: after its ``np.array(...).transpose()`` both must be (B, 1) -- ``pose`` (B,) for POSE.

Per case the file's text; per LOSS case also each frame's float64 value (cluster_cases.frame_loss_f64) and the largest
relative deviation of the reference's float32 sum from it, which the GPU test adds to its 1-ulp bound.  Inputs are not
stored: cluster_cases.py regenerates them.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import cluster_cases  # noqa: E402

DEVIATION_CAP = 2e-6  # the project's loss tolerance (test_masked_mse_and_mkpe_vs_oracle): a case beyond it needs another seed


def reference_batch(c, dp):
    """One of our batches in the layouts the reference's cluster() indexes."""
    out = {k: torch.from_numpy(np.asarray(v)) for k, v in dp.items()}
    out["frame_id"] = out["frame_id"].reshape(1, -1)  # .transpose() -> (B, 1): frame_ids[idx][0]
    out["pose"] = out["pose"].reshape(-1) if c["type"] == "POSE" else out["pose"].reshape(1, -1)  # poses[idx] / poses[idx][0]
    return out


class _Dataset:
    def label_all(self):
        pass

    def resample_frames(self, n):
        assert n == -1


class _Replay:
    """Estimator stand-in: the case's heat-map batches in order."""

    def __init__(self, hms):
        self.it = iter(hms)
        self.loaded = 0

    def eval(self):
        return self

    def load_state_dict(self, state_dict, strict=True):
        assert strict and list(state_dict) == ["w"]
        self.loaded += 1

    def __call__(self, images):
        return torch.from_numpy(next(self.it))


def run_case(name, c, tmp):
    from oracle import ref_harness

    loader, hms = cluster_cases.build_cluster_loader(c)
    save = os.path.join(tmp, name + ".json")
    ckpt = os.path.join(tmp, name + ".pth")
    torch.save({"state_dict": {"w": torch.zeros(1)}}, ckpt)
    st = ref_harness.make_strategy("HP", **{"AL.CLUSTER.TYPE": c["type"], "AL.CLUSTER.SAVE_PATH": save,
                                            "AL.CLUSTER.RESTORE_FROM": ckpt, "DATA.NUM_JOINTS": c["j"]})
    st._pathmgr.open = open
    st._get_dataloader = lambda dataset, batch_size, num_workers: [reference_batch(c, dp) for dp in loader]
    model = _Replay(hms)
    st.cluster(model, _Dataset(), 0)
    assert model.loaded == (1 if c["type"] == "LOSS" else 0)
    with open(save) as f:
        text = f.read()
    rec = {"text": text}
    if c["type"] == "LOSS":
        got = json.loads(text)
        f64, dev = {}, 0.0
        k = 0
        keys = list(got)
        for dp, hm in zip(loader, hms):
            b = dp["gt_heatmap"].shape[0]
            vals = cluster_cases.frame_loss_f64(hm.reshape(dp["gt_heatmap"].shape), dp["gt_heatmap"])
            for i in range(b):
                f64[keys[k]] = float(vals[i])
                dev = max(dev, abs(got[keys[k]] - float(vals[i])) / float(vals[i]))
                k += 1
        assert k == len(keys)
        assert dev <= DEVIATION_CAP, "%s: the reference deviates by %.3g from the float64 value: pick another seed" % (name, dev)
        rec["f64"] = f64
        rec["deviation"] = dev
        print("%s: %d frames, values %.4g .. %.4g, reference deviation %.3g" % (name, k, min(f64.values()), max(f64.values()), dev))
    else:
        print("%s: %d frames, %d bytes" % (name, len(json.loads(text)), len(text)))
    return rec


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in cluster_cases.cluster_cases().items():
            out[name] = run_case(name, c, tmp)
    with open(os.path.join(HERE, "cluster.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

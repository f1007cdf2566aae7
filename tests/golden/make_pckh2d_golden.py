"""Generate the 2-D PCKh goldens by running the REAL reference's utils/evaluation.py on the CPU (build container only):

    python tests/golden/make_pckh2d_golden.py [path of the reference tree]

  pckh2d.npz   per case of pckh2d_cases.py, data only --
    <noisy|ties|degenerate>/figure     compute_pckh_figure(pred batches, gt batches, num_keypoints)[1]          (10, K) f64
    <...>/pckh_0_5                     compute_pckh_0_5(...)                                                     (K,) f64
    degenerate/pckh_kp                 compute_pckh(..., t, 5, kp0=2, kp1=5) for each of the ten thresholds      (10, 5) f64
    decode_<hh>x<wh>/xy                torch.Tensor(get_pred_coordinates(hm, boxes, J))                          (N, J, 2) f32
    pass/figure, pass/pckh_0_5         compute_pckh_figure / compute_pckh_0_5 over the per-batch
                                       torch.Tensor(get_pred_coordinates(...)) and the reshaped 2d_after_crop:
                                       the arithmetic of _evaluate_2d_pckh (strategy.py:548-582) at world size 1
    versions                           the library versions the reference ran under

The inputs are rebuilt from the seeds of pckh2d_cases.py.  The reference module is loaded from its file with a stand-in for
``kornia`` (absent here; only the soft-arg-max branch, which is not captured, calls it) and without writing bytecode into the
reference tree.  The NumPy restatement of pckh2d_cases.py is checked against every captured array before the file is written.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle.ref_harness import REFERENCE_ROOT  # noqa: E402  (the path only: the module is loaded from its file below)

import pckh2d_cases as pc  # noqa: E402


def load_reference_evaluation(root):
    if "kornia" not in sys.modules:
        sys.modules["kornia"] = types.ModuleType("kornia")
    spec = importlib.util.spec_from_file_location("reference_utils_evaluation", os.path.join(root, "utils", "evaluation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ev = load_reference_evaluation(sys.argv[1] if len(sys.argv) > 1 else REFERENCE_ROOT)
    out = {}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    for name, c in pc.metric_cases().items():
        pred, gt = [t(a) for a in pc.split(c["pred"], c["batches"])], [t(a) for a in pc.split(c["gt"], c["batches"])]
        k = c["num_keypoints"]
        thresholds, pcks = ev.compute_pckh_figure(pred, gt, k)
        assert tuple(thresholds) == pc.THRESHOLDS
        out[name + "/figure"] = np.asarray(pcks, np.float64)
        out[name + "/pckh_0_5"] = np.asarray(ev.compute_pckh_0_5(pred, gt, k), np.float64)
        np.testing.assert_array_equal(out[name + "/figure"], pc.np_pckh(c["pred"], c["gt"], pc.THRESHOLDS, k))
        if (c["kp0"], c["kp1"]) != (0, 1):
            out[name + "/pckh_kp"] = np.asarray([ev.compute_pckh(pred, gt, th, k, kp0=c["kp0"], kp1=c["kp1"]) for th in pc.THRESHOLDS], np.float64)
            np.testing.assert_array_equal(out[name + "/pckh_kp"], pc.np_pckh(c["pred"], c["gt"], pc.THRESHOLDS, k, c["kp0"], c["kp1"]))
        print(name, out[name + "/pckh_0_5"])

    for hh, wh in pc.DECODE_SIZES:
        hm, boxes = pc.decode_case(hh, wh)
        xy = torch.Tensor(ev.get_pred_coordinates(t(hm), t(boxes), hm.shape[1]))
        assert xy.dtype == torch.float32
        out[pc.decode_name(hh, wh) + "/xy"] = xy.numpy()
        np.testing.assert_array_equal(xy.numpy(), pc.np_pred_coordinates(hm, boxes))
    # (the probe the case was designed around: row 5, column 4 of the 8 x 6 map under the non-square box)
    assert out["decode_8x6/xy"][2, 0].tolist() == [np.float32(160.0) / np.float32(6.0) * np.float32(2.0), 50.0], out["decode_8x6/xy"][2, 0]
    print("decode 8x6, non-square box, joint 0:", out["decode_8x6/xy"][2, 0])

    loader, maps = pc.pass_case()
    preds, gts = [], []
    for dp, hm in zip(loader, maps):
        preds.append(torch.Tensor(ev.get_pred_coordinates(t(hm), t(dp["square_box"]).reshape([-1, 4]), pc.J)))
        gts.append(t(dp["2d_after_crop"]).reshape([-1, pc.J, 2]))
    out["pass/figure"] = np.asarray(ev.compute_pckh_figure(preds, gts, pc.J)[1], np.float64)
    out["pass/pckh_0_5"] = np.asarray(ev.compute_pckh_0_5(preds, gts, pc.J), np.float64)
    np.testing.assert_array_equal(out["pass/figure"], pc.np_pckh(np.concatenate([p.numpy() for p in preds]),
                                                                 np.concatenate([g.numpy() for g in gts]), pc.THRESHOLDS, pc.J))
    print("pass", out["pass/pckh_0_5"])

    versions = json.dumps(dict(numpy=np.__version__, torch=torch.__version__, python=sys.version.split()[0]))
    np.savez_compressed(os.path.join(HERE, "pckh2d.npz"), versions=versions, **out)


if __name__ == "__main__":
    main()

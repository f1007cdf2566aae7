"""Generate tests/golden/rotate_targets.npz and rotate_targets.json: heat-maps rotated by the real Pillow, and the REAL reference's
RandAugment / ``prepare_single_view(split="train")`` with its Rotate corrected to keep the maps it rotates.

Run in the build container only (needs /root/reference):

    python tests/golden/make_rotate_targets_golden.py

The reference's dataset/augmentation.py:22 reads ``h.rotate(v, resample=Image.BICUBIC)`` and drops the result.  ``corrected_rotate`` below is
that function with the result kept: the same coin toss, the same image rotate, the rotated maps returned.  It is put into the freshly
loaded module before ``RandAugment.__init__`` reads the op functions into its list; the reference's own ``__call__`` and
``prepare_single_view`` then produce the expected values.  Only arrays, op names, angles and counts are stored (plus the Pillow version);
inputs are regenerated from seeds by rotate_targets_cases.py.
  single/<h>x<w>            the rotating views of rotate_targets_cases.single_maps(h, w), in order: (views, MAPS, h, w) float32
  chain                     the rotating views of chain_maps() through their plan's rotations one after the other
  nan                       nan_map() rotated by NAN_ANGLE
  call/<case>               the heat-maps of whole RandAugment calls (K = 3): (views, 2, mh, mw) float32; ops in rotate_targets.json
  train/<case>/<field>      images and gt_heatmap of prepare_single_view(split="train")
"""
from __future__ import annotations

import io
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
sys.dont_write_bytecode = True

import cases  # noqa: E402
import make_augment_golden  # noqa: E402
import rotate_targets_cases as rc  # noqa: E402


def corrected_rotate(img, heatmap, v):
    """dataset/augmentation.py's Rotate as its code evidently meant it: heatmap (h, w, J) comes back rotated with the image."""
    from PIL import Image

    assert -30 <= v <= 30
    if random.random() > 0.5:
        v = -v
    rotated = [np.asarray(Image.fromarray(heatmap[:, :, kp]).rotate(v, resample=Image.BICUBIC)) for kp in range(heatmap.shape[2])]
    return img.rotate(v, resample=Image.BICUBIC), np.stack(rotated, axis=-1)


def load_corrected_reference(log):
    """A fresh instance of the reference's augmentation module with Rotate replaced; every op call is appended to log as [name, value]
    (for Rotate the signed angle, read off the coin the op is about to toss)."""
    mod = make_augment_golden.load_reference_augmentation()
    mod.Rotate = corrected_rotate
    for name in make_augment_golden.OPS:
        def rec(img, hm, v, _orig=getattr(mod, name), _name=name):
            val = float(v)
            if _name == "Rotate":
                st = random.getstate()
                val = -val if random.random() > 0.5 else val
                random.setstate(st)
            log.append([_name, val])
            return _orig(img, hm, v)

        setattr(mod, name, rec)
    return mod


def pillow_rotate(m, angles):
    from PIL import Image

    for a in angles:
        m = np.asarray(Image.fromarray(np.ascontiguousarray(m, dtype=np.float32)).rotate(a, resample=Image.BICUBIC)).copy()
    return m


def gen_pillow(out, meta):
    for (h, w) in rc.SIZES:
        maps = rc.single_maps(h, w)
        out["single/%dx%d" % (h, w)] = np.stack([np.stack([pillow_rotate(m, [a]) for m in maps[i]])
                                                 for i, a in enumerate(rc.ANGLES) if not rc.rests(a)])
    maps = rc.chain_maps()
    out["chain"] = np.stack([np.stack([pillow_rotate(m, rc.plan_angles(ops)) for m in maps[i]])
                             for i, ops in enumerate(rc.CHAIN_PLAN) if rc.plan_angles(ops)])
    out["nan"] = pillow_rotate(rc.nan_map(), [rc.NAN_ANGLE])
    meta["angles"] = [float(a) for a in rc.ANGLES]
    meta["chain_angles"] = [rc.plan_angles(ops) for ops in rc.CHAIN_PLAN]


def gen_calls(out, meta):
    import torch
    from PIL import Image

    meta["calls"] = {}
    for name, c in rc.call_cases().items():
        log = []
        mod = load_corrected_reference(log)
        ra = mod.RandAugment(3, c["magnitude"], True, True, c["const"])
        random.seed(c["seed"])
        np.random.seed(c["seed"])
        res = []
        for img, hm in zip(rc.call_images(c), rc.call_maps(c)):
            _, r = ra(Image.fromarray(img), torch.from_numpy(hm.copy()))
            assert r.dtype == torch.float32
            res.append(r.numpy().copy())
        out["call/" + name] = np.stack(res)
        meta["calls"][name] = [log[i * 3:(i + 1) * 3] for i in range(c["views"])]


def gen_train(out, meta):
    """As make_augment_golden.gen_train, with the corrected Rotate."""
    from oracle import ref_harness
    from PIL import Image

    ref_harness.load()
    from dataset import dataset as ref_ds  # type: ignore  (reference module, harness path)

    meta["train"] = {}
    for name, a in rc.train_cases().items():
        c = cases.preprocess_cases()[name]
        img, kp3d, cam = cases.preprocess_inputs(c)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        log = []
        mod = load_corrected_reference(log)
        fake = types.SimpleNamespace(
            _pathmgr=types.SimpleNamespace(open=lambda path, mode: io.BytesIO(buf.getvalue())),
            _logger=types.SimpleNamespace(debug=lambda *a, **k: None),
            data_cfg=types.SimpleNamespace(SCALE_BBOX=c["scale"], INPUT_WIDTH=c["in_w"], INPUT_HEIGHT=c["in_h"]),
            gt_stride=c["stride"], split="train", augmentation=mod.RandAugment(a["num_aug"], a["magnitude"], True, True, a["const"]))
        view = {"path": "mem.png", "box": list(c["box"]), "camera": cam, "camera_name": "cam0"}
        random.seed(a["seed"])
        np.random.seed(a["seed"])
        v = ref_ds.ActiveLearningDataset.prepare_single_view(fake, view, kp3d, c["sigma"])
        for k in ("images", "gt_heatmap"):
            out["train/%s/%s" % (name, k)] = v[k].numpy()
        meta["train"][name] = dict(ops=log, rotations=len(rc.plan_angles(log)))
        assert meta["train"][name]["rotations"] >= 1, "%s: seed %d draws no rotation" % (name, a["seed"])


def build():
    """(arrays, meta): everything the two fixture files hold."""
    import PIL

    out, meta = {}, {"pillow": PIL.__version__}
    gen_pillow(out, meta)
    gen_calls(out, meta)
    gen_train(out, meta)
    return out, meta


def meta_text(meta):
    return json.dumps(meta, indent=1, sort_keys=True) + "\n"


def main():
    out, meta = build()
    np.savez_compressed(os.path.join(HERE, "rotate_targets.npz"), **out)
    with open(os.path.join(HERE, "rotate_targets.json"), "w") as f:
        f.write(meta_text(meta))
    print("rotate_targets.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "rotate_targets.npz"))))


if __name__ == "__main__":
    main()

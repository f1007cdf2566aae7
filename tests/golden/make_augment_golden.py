"""Generate tests/golden/augment.npz and augment.json: the REAL reference's RandAugment (dataset/augmentation.py) on the
real Pillow, and its ``prepare_single_view`` with ``split == "train"``.

Run in the build container only (needs /root/reference):

    python tests/golden/make_augment_golden.py

The reference's augmentation module is loaded by file path; its op functions are wrapped so that every call is recorded as
(op name, value) -- for Rotate the signed angle, read off the coin the op is about to toss.  Only arrays, op names and values
are stored (plus the Pillow version); inputs are regenerated from seeds by augment_cases.py.
  <H>x<W>/<case>           one op alone on augment_cases.image(H, W, ...): (H, W, 3) uint8
  seq/<case>               whole RandAugment calls (K = 3) on the views of a case: (V, H, W, 3) uint8; ops in augment.json
  train/<case>/<field>     prepare_single_view(split="train") on a cases.preprocess_cases() input
augment.json: Pillow version, the recorded op lists, and for the draw cases the next value of both random streams.
"""
from __future__ import annotations

import importlib.util
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

import augment_cases  # noqa: E402
import cases  # noqa: E402

OPS = ("Rotate", "AutoContrast", "Invert", "Equalize", "Solarize", "Posterize", "Contrast", "Color", "Brightness", "Sharpness")


def load_reference_augmentation(log=None):
    """A fresh instance of the reference's dataset/augmentation.py, loaded by file path.  With a list, every op call is
    appended to it as [name, value]."""
    from oracle import ref_harness

    spec = importlib.util.spec_from_file_location("_ref_augmentation", os.path.join(ref_harness.REFERENCE_ROOT, "dataset", "augmentation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if log is not None:
        for name in OPS:
            def rec(img, hm, v, _orig=getattr(mod, name), _name=name):
                val = float(v)
                if _name == "Rotate":  # the sign is tossed inside the op: look at the coin, then put it back
                    st = random.getstate()
                    val = -val if random.random() > 0.5 else val
                    random.setstate(st)
                log.append([_name, val])
                return _orig(img, hm, v)

            setattr(mod, name, rec)  # before RandAugment.__init__ reads the functions into its list
    return mod


def gen_single(out):
    from PIL import Image

    mod = load_reference_augmentation()
    mod.random = types.SimpleNamespace(random=lambda: 0.0)  # Rotate's coin: never flips, the case's angle is the angle
    hm = np.zeros((4, 4, 1), dtype=np.float32)
    for (h, w) in augment_cases.SIZES:
        for name, (op, val, const) in augment_cases.single_op_cases().items():
            img = augment_cases.image(h, w, augment_cases.size_seed(h, w), const)
            res, _ = getattr(mod, op)(Image.fromarray(img), hm, val)
            out["%dx%d/%s" % (h, w, name)] = np.asarray(res).copy()


def gen_sequences(out, meta):
    import torch
    from PIL import Image

    meta["sequences"] = {}
    for name, c in augment_cases.sequence_cases().items():
        log = []
        mod = load_reference_augmentation(log)
        ra = mod.RandAugment(3, c["magnitude"], True, True, c["const"])
        random.seed(c["seed"])
        np.random.seed(c["seed"])
        res = []
        for img in augment_cases.sequence_images(c):
            r, _ = ra(Image.fromarray(img), torch.zeros(1, 4, 4))
            res.append(np.asarray(r).copy())
        out["seq/" + name] = np.stack(res)
        meta["sequences"][name] = [log[i * 3:(i + 1) * 3] for i in range(c["views"])]


def gen_draws(meta):
    import torch
    from PIL import Image

    meta["draws"] = {}
    img = Image.fromarray(augment_cases.image(8, 8, 1))
    for name, c in augment_cases.draw_cases().items():
        log = []
        mod = load_reference_augmentation(log)
        ra = mod.RandAugment(c["num_aug"], c["magnitude"], c["rotation"], c["image_aug"], c["const"])
        random.seed(c["seed"])
        np.random.seed(c["seed"])
        for _ in range(c["views"]):
            ra(img, torch.zeros(1, 4, 4))
        meta["draws"][name] = dict(ops=[log[i * c["num_aug"]:(i + 1) * c["num_aug"]] for i in range(c["views"])],
                                   next_random=random.random(), next_np=float(np.random.rand()))


def gen_train(out, meta):
    """As make_golden.gen_preprocess drives prepare_single_view for the validation split, with split="train"."""
    from oracle import ref_harness
    from PIL import Image

    ref_harness.load()
    from dataset import dataset as ref_ds  # type: ignore  (reference module, harness path)

    meta["train"] = {}
    for name, a in augment_cases.train_cases().items():
        c = cases.preprocess_cases()[name]
        img, kp3d, cam = cases.preprocess_inputs(c)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        log = []
        mod = load_reference_augmentation(log)
        fake = types.SimpleNamespace(
            _pathmgr=types.SimpleNamespace(open=lambda path, mode: io.BytesIO(buf.getvalue())),
            _logger=types.SimpleNamespace(debug=lambda *a, **k: None),
            data_cfg=types.SimpleNamespace(SCALE_BBOX=c["scale"], INPUT_WIDTH=c["in_w"], INPUT_HEIGHT=c["in_h"]),
            gt_stride=c["stride"], split="train", augmentation=mod.RandAugment(a["num_aug"], a["magnitude"], True, True, a["const"]))
        view = {"path": "mem.png", "box": list(c["box"]), "camera": cam, "camera_name": "cam0"}
        random.seed(a["seed"])
        np.random.seed(a["seed"])
        v = ref_ds.ActiveLearningDataset.prepare_single_view(fake, view, kp3d, c["sigma"])
        for k in ("images", "gt_heatmap", "proj_matrices", "2d_keypoints", "2d_after_crop", "square_box"):
            out["train/%s/%s" % (name, k)] = v[k].numpy()
        meta["train"][name] = dict(ops=log)


def build():
    """(arrays, meta): everything the two fixture files hold."""
    import PIL

    out, meta = {}, {"pillow": PIL.__version__}
    gen_single(out)
    gen_sequences(out, meta)
    gen_draws(meta)
    gen_train(out, meta)
    return out, meta


def meta_text(meta):
    return json.dumps(meta, indent=1, sort_keys=True) + "\n"


def main():
    out, meta = build()
    np.savez_compressed(os.path.join(HERE, "augment.npz"), **out)
    with open(os.path.join(HERE, "augment.json"), "w") as f:
        f.write(meta_text(meta))
    print("augment.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "augment.npz"))))


if __name__ == "__main__":
    main()

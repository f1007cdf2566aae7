"""The training split's RandAugment (the reference's dataset/augmentation.py) on the device, bit-exact with Pillow.

``RandAugment.draw`` picks the ops on the host from the process-global ``random`` / ``numpy.random`` streams in the
reference's order, so a seeded run picks what the reference picks; ``RandAugment.apply`` runs a plan on a batch of uint8
views (csrc/augment.hip: per step one pass per KIND of op present, whatever the number of views).  The image is in the
reference's channel order at that point (BGR handed to Pillow as "RGB"): the ops see channel positions only.

The reference's Rotate turns the image and drops the heat-maps it rotated.  That is the default; ``rotate_targets`` offers the two ways of
turning the targets along: ``RandAugment.rotate_maps`` (Pillow's mode-"F" bicubic rotate of every map, on the device, bit for bit) and
``rotate_points`` (the key-points through the image's affine map, on the host).
"""
from __future__ import annotations

import ctypes as C
import math
import random

import numpy as np
import torch

from .. import _lib

# include/mval_hip.h: MVAL_AUG_*
AUG_NONE, AUG_AUTOCONTRAST, AUG_EQUALIZE, AUG_INVERT, AUG_POSTERIZE, AUG_SOLARIZE = 0, 1, 2, 3, 4, 5
AUG_COLOR, AUG_CONTRAST, AUG_BRIGHTNESS, AUG_SHARPNESS, AUG_ROTATE = 6, 7, 8, 9, 10
KINDS = {"AutoContrast": AUG_AUTOCONTRAST, "Equalize": AUG_EQUALIZE, "Invert": AUG_INVERT, "Posterize": AUG_POSTERIZE,
         "Solarize": AUG_SOLARIZE, "Color": AUG_COLOR, "Contrast": AUG_CONTRAST, "Brightness": AUG_BRIGHTNESS,
         "Sharpness": AUG_SHARPNESS, "Rotate": AUG_ROTATE}
# the values the reference's op functions assert or that Pillow accepts
_RANGES = {"Rotate": (-30.0, 30.0), "Solarize": (0.0, 256.0), "Posterize": (0.0, 8.0), "Color": (0.1, 1.9), "Contrast": (0.1, 1.9),
           "Brightness": (0.1, 1.9), "Sharpness": (0.1, 1.9)}


class _AugOp(C.Structure):
    """include/mval_hip.h: struct mval_aug_op."""

    _fields_ = [("kind", C.c_int32), ("pad", C.c_int32), ("p", C.c_double * 6)]


def rotate_coefficients(angle, w, h):
    """PIL.Image.Image.rotate's affine matrix (output pixel -> input position) for the default centre, or None where
    Pillow returns a copy (angle mod 360 == 0).  The reference only produces |angle| <= 30, so Pillow's transpose
    short cuts at 90 / 180 / 270 degrees are out of reach (and rejected by apply)."""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def plan_descriptors(plan, h, w, full_turns=False):
    """plan (per view a list of (op name, value)) -> (ctypes array [V][K] of mval_aug_op, per-step bit masks of the kinds present).
    full_turns=True also takes a Rotate by a multiple of 360 degrees from outside the reference's range: NONE, as every angle that is
    0 mod 360 (Pillow answers it with a copy)."""
    v = len(plan)
    k = len(plan[0]) if v else 0
    if v == 0 or any(len(ops) != k for ops in plan):
        raise ValueError("augment: every view needs an op list of the same length")
    descs = (_AugOp * (v * max(k, 1)))()
    masks = [0] * k
    for i, ops in enumerate(plan):
        for s, (name, val) in enumerate(ops):
            if name not in KINDS:
                raise ValueError("augment: unknown op %r" % (name,))
            val = float(val)
            lo, hi = _RANGES.get(name, (-math.inf, math.inf))
            if not lo <= val <= hi and not (full_turns and name == "Rotate" and val % 360.0 == 0):  # (the range test is also False for a NaN)
                raise ValueError("augment: %s value %r outside [%g, %g]" % (name, val, lo, hi))
            d = descs[i * k + s]
            d.kind = KINDS[name]
            if name == "Rotate":
                m = rotate_coefficients(val, w, h)
                if m is None:
                    d.kind = AUG_NONE
                else:
                    d.p[:] = m
            else:
                d.p[0] = val
            masks[s] |= 1 << d.kind
    return descs, masks


ROTATE_TARGETS = ("none", "maps", "points")


def rotate_points(points, plan, w, h):
    """Carry key-points along with the image through a plan's Rotate steps: points (V, J, 2) float64 (x, y) in pixels of the w x h image
    the plan was applied to -> the positions the same image content has afterwards.  Per Rotate step, with Pillow's coefficients
    m = rotate_coefficients(angle, w, h) (output pixel centre -> input position), the inverse of that map:
        u = x + 0.5 - m2, v = y + 0.5 - m5, det = m0 m4 - m1 m3, x' = (m4 u - m1 v) / det - 0.5, y' = (-m3 u + m0 v) / det - 0.5
    in float64, steps in plan order; other ops and angles that are 0 mod 360 leave the points alone.  Host arithmetic, returns a new array."""
    pts = np.array(points, dtype=np.float64)
    if pts.ndim != 3 or pts.shape[2] != 2:
        raise ValueError("rotate_points: points must be (V, J, 2), got %r" % (pts.shape,))
    if len(plan) != pts.shape[0]:
        raise ValueError("rotate_points: %d op lists for %d views" % (len(plan), pts.shape[0]))
    for i, ops in enumerate(plan):
        for name, val in ops:
            m = rotate_coefficients(float(val), w, h) if name == "Rotate" else None
            if m is None:
                continue
            u, v = pts[i, :, 0] + 0.5 - m[2], pts[i, :, 1] + 0.5 - m[5]
            det = m[0] * m[4] - m[1] * m[3]
            pts[i, :, 0], pts[i, :, 1] = (m[4] * u - m[1] * v) / det - 0.5, (-m[3] * u + m[0] * v) / det - 0.5
    return pts


class RandAugment:
    """The reference's RandAugment(num_aug, magnitude, rotation, image_aug, const_magnitude=True) for batches of device views.
    rotate_targets (not in the reference) says what Rotate does to the training targets: "none" -- nothing, the reference as published
    (its Rotate drops the rotated heat-maps); "maps" -- every heat-map of a view is rotated as the image was, by Pillow's
    Image.rotate(angle, BICUBIC) on the map itself, what the reference's code evidently meant (``rotate_maps``); "points" -- the projected
    key-points go through the inverse of the image's own affine map before the targets are rendered (``rotate_points``, through
    ``utils.preprocess.prepare_views``).  ``draw`` and the random streams are the same in every mode."""

    def __init__(self, num_aug, magnitude, rotation: bool, image_aug: bool, const_magnitude: bool = True, *, rotate_targets="none"):
        if rotate_targets not in ROTATE_TARGETS:
            raise ValueError("RandAugment: rotate_targets %r: accepted are %s" % (rotate_targets, ", ".join(repr(t) for t in ROTATE_TARGETS)))
        self.rotate_targets = rotate_targets
        if isinstance(num_aug, bool) or not isinstance(num_aug, (int, np.integer)) or num_aug < 0:
            raise ValueError("RandAugment: num_aug must be a non-negative integer, got %r" % (num_aug,))
        if not 0 <= float(magnitude) <= 30:  # beyond 30 the reference's ops assert on their value
            raise ValueError("RandAugment: magnitude must lie in [0, 30], got %r" % (magnitude,))
        self.num_aug = int(num_aug)
        self.magnitude = magnitude
        self.const_magnitude = bool(const_magnitude)
        self.augment_list = []
        if rotation:
            self.augment_list.append(("Rotate", 0, 30))
        if image_aug:
            self.augment_list += [("AutoContrast", 0, 1), ("Equalize", 0, 1), ("Invert", 0, 1), ("Posterize", 0, 4), ("Solarize", 0, 256),
                                  ("Color", 0.1, 1.9), ("Contrast", 0.1, 1.9), ("Brightness", 0.1, 1.9), ("Sharpness", 0.1, 1.9)]
        if self.num_aug and not self.augment_list:
            raise ValueError("RandAugment: num_aug > 0 needs rotation or image_aug")

    def draw(self, n_views):
        """The op plan of n_views views, one after the other: per view a list of num_aug (op name, value); Rotate's value
        is the signed angle.  Consumes ``random`` and ``numpy.random`` exactly as the reference's __call__ (and its Rotate) does."""
        if isinstance(n_views, bool) or not isinstance(n_views, (int, np.integer)) or n_views <= 0:
            raise ValueError("RandAugment.draw: n_views must be a positive integer, got %r" % (n_views,))
        plan = []
        for _ in range(n_views):
            ops = random.choices(self.augment_list, k=self.num_aug) if self.num_aug else []
            view = []
            for name, minval, maxval in ops:
                if self.const_magnitude:
                    val = (float(self.magnitude) / 30) * float(maxval - minval) + minval
                else:
                    val = np.random.rand() * float(self.magnitude) / 30
                    val = val * float(maxval - minval) + minval
                if name == "Rotate" and random.random() > 0.5:
                    val = -val
                view.append((name, float(val)))
            plan.append(view)
        return plan

    @staticmethod
    def apply(images_u8, plan, inplace=False):
        """Run a plan on images_u8 (V, H, W, 3) uint8 (HIP tensor, the reference's channel order).  No host synchronisation;
        all work goes to the current stream."""
        if (not torch.is_tensor(images_u8)) or (not images_u8.is_cuda) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 \
                or images_u8.shape[3] != 3:
            raise _lib.MvalError("augment: images must be a uint8 HIP tensor (V, H, W, 3)")
        v, h, w, _ = images_u8.shape
        if len(plan) != v:
            raise ValueError("augment: %d op lists for %d views" % (len(plan), v))
        descs, masks = plan_descriptors(plan, h, w)
        out = images_u8.contiguous() if inplace else images_u8.clone(memory_format=torch.contiguous_format)
        if not masks or not any(m & ~1 for m in masks):
            return out
        from .preprocess import _upload_descs

        lib = _lib.lib()
        lib.mval_augment_views_workspace_bytes.restype = C.c_size_t
        ws = torch.empty(int(lib.mval_augment_views_workspace_bytes(C.c_int(v), C.c_int(h), C.c_int(w))), dtype=torch.uint8, device=out.device)
        dd = _upload_descs(bytes(descs), out.device)
        step_kinds = (C.c_uint32 * len(masks))(*masks)
        _lib._check(lib.mval_augment_views(_lib._p(out), _lib._p(dd), step_kinds, C.c_int(v), C.c_int(len(masks)), C.c_int(h), C.c_int(w),
                                           _lib._p(ws), _lib._stream()), "mval_augment_views")
        return out

    @classmethod
    def from_config(cls, data_cfg):
        """The augmentation of a DATA config node: the five knobs the reference's ActiveLearningDataset hands its RandAugment
        (dataset/dataset.py:30-36) and DATA.ROTATE_TARGETS ("none" where the node has no such field, as a reference YAML)."""
        from ..config import check_rotate_targets

        mode = check_rotate_targets(data_cfg.ROTATE_TARGETS if "ROTATE_TARGETS" in data_cfg else "none")
        return cls(data_cfg.NUM_AUG, data_cfg.AUG_MAGNITUDE, data_cfg.USE_ROTATION, data_cfg.USE_IMAGE_AUG, data_cfg.USE_CONST_AUG_MAGNITUDE,
                   rotate_targets=mode)

    @staticmethod
    def rotate_maps(heatmaps, plan, inplace=False):
        """The target side of a plan's Rotate steps: heatmaps (V, J, h, w) float32 (HIP tensor) with every map of view v rotated by Pillow's
        Image.rotate(angle, BICUBIC) on a mode-"F" image of h x w, bit for bit, for each Rotate of plan[v] in order (about the map's own
        centre, as the corrected reference would).  Other ops, and angles that are 0 mod 360, leave a view's maps alone; a plan without an
        effective rotation returns the input (inplace) or its clone and launches nothing.  No host synchronisation."""
        if (not torch.is_tensor(heatmaps)) or (not heatmaps.is_cuda) or heatmaps.dtype != torch.float32 or heatmaps.dim() != 4:
            raise _lib.MvalError("rotate_maps: heat-maps must be a float32 HIP tensor (V, J, h, w)")
        v, j, h, w = heatmaps.shape
        if len(plan) != v:
            raise ValueError("rotate_maps: %d op lists for %d views" % (len(plan), v))
        descs, masks = plan_descriptors(plan, h, w, full_turns=True)
        out = heatmaps.contiguous() if inplace else heatmaps.clone(memory_format=torch.contiguous_format)
        if j == 0 or not any(m & (1 << AUG_ROTATE) for m in masks):
            return out
        from .preprocess import _upload_descs

        lib = _lib.lib()
        lib.mval_rotate_maps_workspace_bytes.restype = C.c_size_t
        ws = torch.empty(int(lib.mval_rotate_maps_workspace_bytes(C.c_int(v), C.c_int(j), C.c_int(h), C.c_int(w))), dtype=torch.uint8,
                         device=out.device)
        dd = _upload_descs(bytes(descs), out.device)
        step_kinds = (C.c_uint32 * len(masks))(*masks)
        _lib._check(lib.mval_rotate_maps(_lib._p(out), _lib._p(dd), step_kinds, C.c_int(v), C.c_int(len(masks)), C.c_int(j), C.c_int(h), C.c_int(w),
                                         _lib._p(ws), _lib._stream()), "mval_rotate_maps")
        return out

    def __call__(self, images_u8, heatmaps):
        """(augmented copy of images_u8, heatmaps).  rotate_targets "none": the reference's Rotate throws its rotated heat-maps away
        (dataset/augmentation.py:19-25), so the heat-maps come out as they went in.  "maps": one plan is drawn and used for both, the
        heat-maps (V, J, h, w) come back as their rotated copy.  "points" has no points to work on here and raises."""
        if self.rotate_targets == "points":
            raise ValueError("RandAugment: rotate_targets='points' works on key-points, not on heat-maps: use utils.preprocess.prepare_views("
                             "..., augmentation=ra), or draw() a plan and hand it to apply() and rotate_points()")
        plan = self.draw(int(images_u8.shape[0]))
        out = self.apply(images_u8, plan)
        return out, (self.rotate_maps(heatmaps, plan) if self.rotate_targets == "maps" else heatmaps)

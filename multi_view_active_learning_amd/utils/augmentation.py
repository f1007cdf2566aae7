"""The training split's RandAugment (the reference's dataset/augmentation.py) on the device, bit-exact with Pillow.

``RandAugment.draw`` picks the ops on the host from the process-global ``random`` / ``numpy.random`` streams in the
reference's order, so a seeded run picks what the reference picks; ``RandAugment.apply`` runs a plan on a batch of uint8
views (csrc/augment.hip: per step one pass per KIND of op present, whatever the number of views).  The image is in the
reference's channel order at that point (BGR handed to Pillow as "RGB"): the ops see channel positions only.
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


def plan_descriptors(plan, h, w):
    """plan (per view a list of (op name, value)) -> (ctypes array [V][K] of mval_aug_op, per-step bit masks of the kinds present)."""
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
            if not lo <= val <= hi:  # (also False for a NaN)
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


class RandAugment:
    """The reference's RandAugment(num_aug, magnitude, rotation, image_aug, const_magnitude=True) for batches of device views."""

    def __init__(self, num_aug, magnitude, rotation: bool, image_aug: bool, const_magnitude: bool = True):
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

    def __call__(self, images_u8, heatmaps):
        """(augmented copy of images_u8, heatmaps): the reference's Rotate throws its rotated heat-maps away
        (dataset/augmentation.py:19-25), so the heat-maps come out as they went in."""
        return self.apply(images_u8, self.draw(int(images_u8.shape[0]))), heatmaps

"""The exact-fp32 MFMA conv (csrc/conv_mfma.hip: conv_mfma_kernel on v_mfma_f32_16x16x4_f32 -- the whole MVAL_CONV=fp32 plan, every transposed
conv and its data gradient, every zero-dilated data gradient the parity form does not take, and the "exact" side of every accuracy assertion
of the suite) at every kernel form its dispatch can pick.

Which form a launch runs on is read from the library's own dispatch (mval_conv_mfma_form: the launcher's dry run, host arithmetic, no GPU;
tests/mfma_forms.py names the forms and holds the sweep).  The host tests hold every row of the case tables to the form it is in the table
for and the tables to every form a fixed sweep of shapes finds, per use of the kernel.  The GPU tests run each row against float64 and repeat
the form assertion on the shape they ran.

Rows were chosen from the sweep as the cheapest shape (device tensors + float64 reference) that reaches the form with, where the form's tile
allows it, at least two images, a batch the images-per-tile count does not divide (more than one image group, the last partly filled), a
ragged last tile in columns and rows, a cout that leaves the last cout sub-tile partly empty or a wave idle (20, 40, 80; a multiple of 4, so
that the kept max |x| rows are checked) and at least two channel chunks (cin 48 on 16-channel chunks, 64 on 32-channel chunks: the buffer
swap of the double-buffered forms, the re-stage of the single-buffered one)."""
import ctypes as C
import functools
import os
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mfma_forms as mf
import tiny_graphs as tg

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]

# ---- the case tables ----
# ("conv" | "deconv" (ConvTranspose2d k4 s2 p1), (n, cin, cout, h, w, k, stride) of the FORWARD conv on an h x w input, [epilogue options,]
# the form the row is in the table for).  Options: relu, res1, res2, up1 .. up3 (nearest up-sampling, on 1x1 rows), nchw (NCHW output).
# FWD_EXTRA: the cases that belong to no single form -- 3x3 with cout 19 / 20 (NHWC: the scalar store path for 19, the float4 path with a
# ragged quad range for 20; NCHW: the scalar path, also with several images per tile), cin 16 (ONE 16-channel chunk: a single LDS buffer) and
# cin 48 at 64- and 128-pixel tiles, the stride-2 1x1 conv on odd input sizes, the transposed conv on a one-row map and on 5 x 7.
FWD_CASES = [
    ("conv", (2, 48, 40, 6, 10, 1, 1), "up1", "k1s1_kc16_w1x4_nt3_ms2_ne4"),
    ("conv", (5, 48, 40, 3, 5, 1, 1), "relu+up1", "k1s1_kc16_w1x4_nt3_ms2_ne4_tn"),
    ("conv", (2, 48, 16, 5, 7, 1, 1), "res1+up2", "k1s1_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 48, 16, 3, 5, 1, 1), "relu+res1+up2", "k1s1_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (32, 48, 20, 130, 127, 1, 1), "res1+res2", "k1s1_kc16_w2x2_nt1_ms4_ne4"),
    ("conv", (2, 48, 80, 5, 7, 1, 1), "relu+res1+res2+up3", "k1s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 48, 80, 3, 5, 1, 1), "", "k1s1_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (19, 48, 80, 130, 127, 1, 1), "relu", "k1s1_kc16_w4x1_nt1_ms8_ne4"),
    ("conv", (2, 64, 40, 6, 10, 1, 1), "res1", "k1s1_kc32_w1x4_nt3_ms2_ne4"),
    ("conv", (5, 64, 40, 3, 5, 1, 1), "relu+res1", "k1s1_kc32_w1x4_nt3_ms2_ne4_tn"),
    ("conv", (2, 64, 16, 5, 7, 1, 1), "res1+res2+up1", "k1s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 64, 16, 3, 5, 1, 1), "relu+res1+res2+up1", "k1s1_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (32, 64, 20, 130, 127, 1, 1), "", "k1s1_kc32_w2x2_nt1_ms4_ne4"),
    ("conv", (2, 64, 80, 5, 7, 1, 1), "relu+up2", "k1s1_kc32_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 64, 80, 3, 5, 1, 1), "res1+up3", "k1s1_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (19, 64, 80, 130, 127, 1, 1), "relu+res1", "k1s1_kc32_w4x1_nt1_ms8_ne4"),
    ("conv", (2, 48, 40, 9, 7, 1, 2), "res1+res2", "k1s2_kc16_w1x4_nt3_ms1_ne4"),
    ("conv", (3, 48, 40, 5, 7, 1, 2), "relu+res1+res2", "k1s2_kc16_w1x4_nt3_ms1_ne4_tn"),
    ("conv", (2, 48, 16, 9, 7, 1, 2), "", "k1s2_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 48, 16, 5, 7, 1, 2), "relu", "k1s2_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (2, 48, 80, 9, 7, 1, 2), "res1+up1", "k1s2_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 48, 80, 5, 7, 1, 2), "relu+res1+up1", "k1s2_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (2, 64, 40, 9, 7, 1, 2), "res1+res2+up2", "k1s2_kc32_w1x4_nt3_ms1_ne10"),
    ("conv", (3, 64, 40, 5, 7, 1, 2), "relu+res1+res2+up2", "k1s2_kc32_w1x4_nt3_ms1_ne10_tn"),
    ("conv", (11, 64, 40, 1, 5, 1, 2), "up3", "k1s2_kc32_w1x4_nt3_ms1_ne4_tn"),
    ("conv", (5, 64, 40, 4, 4, 1, 2), "relu+up3", "k1s2_kc32_w1x4_nt3_ms1_ne6_tn"),
    ("conv", (2, 64, 16, 9, 7, 1, 2), "res1", "k1s2_kc32_w2x2_nt1_ms2_ne10"),
    ("conv", (3, 64, 16, 5, 7, 1, 2), "relu+res1", "k1s2_kc32_w2x2_nt1_ms2_ne10_tn"),
    ("conv", (11, 64, 16, 1, 5, 1, 2), "res1+res2", "k1s2_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (5, 64, 16, 3, 5, 1, 2), "relu+res1+res2", "k1s2_kc32_w2x2_nt1_ms2_ne6_tn"),
    ("conv", (2, 64, 80, 9, 7, 1, 2), "up1", "k1s2_kc32_w4x1_nt1_ms4_ne10"),
    ("conv", (3, 64, 80, 5, 7, 1, 2), "relu+up1", "k1s2_kc32_w4x1_nt1_ms4_ne10_tn"),
    ("conv", (11, 64, 80, 1, 5, 1, 2), "res1+up2", "k1s2_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (5, 64, 80, 4, 4, 1, 2), "relu+res1+up2", "k1s2_kc32_w4x1_nt1_ms4_ne6_tn"),
    ("conv", (19, 48, 40, 1, 5, 3, 1), "res1+res2", "k3s1_kc16_w1x4_nt3_ms2_ne10_tn"),
    ("conv", (2, 48, 40, 6, 10, 3, 1), "relu+res1+res2", "k3s1_kc16_w1x4_nt3_ms2_ne4"),
    ("conv", (5, 48, 40, 3, 5, 3, 1), "", "k3s1_kc16_w1x4_nt3_ms2_ne4_tn"),
    ("conv", (5, 48, 40, 2, 9, 3, 1), "relu", "k3s1_kc16_w1x4_nt3_ms2_ne6_tn"),
    ("conv", (2, 48, 16, 5, 7, 3, 1), "res1", "k3s1_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 48, 16, 3, 5, 3, 1), "relu+res1", "k3s1_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (32, 48, 20, 130, 127, 3, 1), "res1+res2", "k3s1_kc16_w2x2_nt1_ms4_ne4"),
    ("conv", (2, 48, 80, 5, 7, 3, 1), "relu+res1+res2", "k3s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 48, 80, 3, 5, 3, 1), "", "k3s1_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (19, 48, 80, 130, 127, 3, 1), "relu", "k3s1_kc16_w4x1_nt1_ms8_ne4"),
    ("conv", (19, 64, 40, 1, 5, 3, 1), "res1", "k3s1_kc32_w1x4_nt3_ms2_ne0_tn"),
    ("conv", (5, 64, 40, 3, 5, 3, 1), "relu+res1", "k3s1_kc32_w1x4_nt3_ms2_ne10_tn"),
    ("conv", (2, 64, 40, 6, 10, 3, 1), "res1+res2", "k3s1_kc32_w1x4_nt3_ms2_ne6"),
    ("conv", (11, 64, 16, 1, 5, 3, 1), "relu+res1+res2", "k3s1_kc32_w2x2_nt1_ms2_ne10_tn"),
    ("conv", (2, 64, 16, 5, 7, 3, 1), "", "k3s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 64, 16, 3, 5, 3, 1), "relu", "k3s1_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (3, 64, 16, 2, 9, 3, 1), "res1", "k3s1_kc32_w2x2_nt1_ms2_ne6_tn"),
    ("conv", (32, 64, 20, 130, 127, 3, 1), "relu+res1", "k3s1_kc32_w2x2_nt1_ms4_ne6"),
    ("conv", (11, 64, 80, 1, 5, 3, 1), "res1+res2", "k3s1_kc32_w4x1_nt1_ms4_ne10_tn"),
    ("conv", (2, 64, 80, 5, 7, 3, 1), "relu+res1+res2", "k3s1_kc32_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 64, 80, 3, 5, 3, 1), "", "k3s1_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (3, 64, 80, 2, 9, 3, 1), "relu", "k3s1_kc32_w4x1_nt1_ms4_ne6_tn"),
    ("conv", (19, 64, 80, 130, 127, 3, 1), "res1", "k3s1_kc32_w4x1_nt1_ms8_ne6"),
    ("conv", (11, 32, 40, 1, 5, 3, 2), "relu+res1", "k3s2_kc16_w1x4_nt3_ms1_ne10_tn"),
    ("conv", (2, 32, 40, 9, 7, 3, 2), "res1+res2", "k3s2_kc16_w1x4_nt3_ms1_ne6"),
    ("conv", (3, 32, 40, 5, 7, 3, 2), "relu+res1+res2", "k3s2_kc16_w1x4_nt3_ms1_ne6_tn"),
    ("conv", (11, 32, 16, 1, 5, 3, 2), "", "k3s2_kc16_w2x2_nt1_ms2_ne10_tn"),
    ("conv", (2, 32, 16, 9, 7, 3, 2), "relu", "k3s2_kc16_w2x2_nt1_ms2_ne6"),
    ("conv", (3, 32, 16, 5, 7, 3, 2), "res1", "k3s2_kc16_w2x2_nt1_ms2_ne6_tn"),
    ("conv", (11, 32, 80, 1, 5, 3, 2), "relu+res1", "k3s2_kc16_w4x1_nt1_ms4_ne10_tn"),
    ("conv", (2, 32, 80, 9, 7, 3, 2), "res1+res2", "k3s2_kc16_w4x1_nt1_ms4_ne6"),
    ("conv", (3, 32, 80, 5, 7, 3, 2), "relu+res1+res2", "k3s2_kc16_w4x1_nt1_ms4_ne6_tn"),
    ("deconv", (2, 32, 16, 3, 5, 4, 2), "", "k4s1_kc16_w4x1_nt1_ms4_ne4_dil2"),
    ("deconv", (3, 32, 16, 1, 5, 4, 2), "relu", "k4s1_kc16_w4x1_nt1_ms4_ne4_tn_dil2"),
]
FWD_EXTRA = [
    ("conv", (2, 32, 19, 20, 24, 3, 1), "relu+res1", "k3s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 32, 20, 20, 24, 3, 1), "res1+res2", "k3s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 32, 19, 20, 24, 3, 1), "relu+nchw", "k3s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 32, 20, 9, 7, 3, 2), "nchw", "k3s2_kc16_w2x2_nt1_ms2_ne6"),
    ("conv", (3, 64, 19, 3, 5, 1, 1), "nchw", "k1s1_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (2, 16, 64, 9, 7, 3, 1), "relu", "k3s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (2, 16, 48, 9, 7, 3, 1), "res1", "k3s1_kc16_w1x4_nt3_ms2_ne4"),
    ("conv", (2, 48, 64, 9, 7, 3, 1), "relu+res1", "k3s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (2, 48, 96, 9, 7, 3, 1), "", "k3s1_kc16_w1x4_nt3_ms2_ne4"),
    ("conv", (3, 16, 16, 3, 5, 1, 1), "up2", "k1s1_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (2, 64, 144, 17, 23, 1, 2), "relu+res1", "k1s2_kc32_w1x4_nt3_ms1_ne10"),
    ("conv", (3, 16, 40, 9, 7, 1, 2), "up1", "k1s2_kc16_w1x4_nt3_ms1_ne4"),
    ("deconv", (3, 32, 48, 1, 5, 4, 2), "relu", "k4s1_kc16_w4x1_nt1_ms4_ne4_tn_dil2"),
    ("deconv", (2, 32, 48, 5, 7, 4, 2), "relu+res1", "k4s1_kc16_w4x1_nt1_ms4_ne4_dil2"),
]
# the data gradient of the FORWARD conv (n, cin, cout, h, w, k, stride): the kernel's own cin is the conv's cout.  Stride 2 = the zero-dilated
# form (`_dil2`); "deconv": the k4 stride-2 conv that is the data gradient of a transposed conv, run inside a training step.  DGRAD_EXTRA: the
# zero-dilated forms on the input sizes of the other parity than their row's (even x even, odd x odd, even x odd), and a cin of 19 / 20 (dx
# through the scalar store path / a ragged quad range).
DGRAD_CASES = [
    ("conv", (2, 40, 48, 6, 10, 1, 1), "k1s1_kc16_w1x4_nt3_ms2_ne4"),
    ("conv", (2, 40, 48, 6, 10, 1, 2), "k1s1_kc16_w1x4_nt3_ms2_ne4_dil2"),
    ("conv", (5, 40, 48, 3, 5, 1, 1), "k1s1_kc16_w1x4_nt3_ms2_ne4_tn"),
    ("conv", (5, 40, 48, 3, 5, 1, 2), "k1s1_kc16_w1x4_nt3_ms2_ne4_tn_dil2"),
    ("conv", (2, 16, 48, 5, 7, 1, 1), "k1s1_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 16, 48, 5, 7, 1, 2), "k1s1_kc16_w2x2_nt1_ms2_ne4_dil2"),
    ("conv", (3, 16, 48, 3, 5, 1, 1), "k1s1_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (3, 16, 48, 3, 5, 1, 2), "k1s1_kc16_w2x2_nt1_ms2_ne4_tn_dil2"),
    ("conv", (32, 20, 48, 130, 127, 1, 1), "k1s1_kc16_w2x2_nt1_ms4_ne4"),
    ("conv", (32, 20, 48, 130, 127, 1, 2), "k1s1_kc16_w2x2_nt1_ms4_ne4_dil2"),
    ("conv", (2, 80, 48, 5, 7, 1, 1), "k1s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (2, 80, 48, 5, 7, 1, 2), "k1s1_kc16_w4x1_nt1_ms4_ne4_dil2"),
    ("conv", (3, 80, 48, 3, 5, 1, 1), "k1s1_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (3, 80, 48, 3, 5, 1, 2), "k1s1_kc16_w4x1_nt1_ms4_ne4_tn_dil2"),
    ("conv", (19, 80, 48, 130, 127, 1, 1), "k1s1_kc16_w4x1_nt1_ms8_ne4"),
    ("conv", (19, 80, 48, 130, 127, 1, 2), "k1s1_kc16_w4x1_nt1_ms8_ne4_dil2"),
    ("conv", (2, 40, 64, 6, 10, 1, 1), "k1s1_kc32_w1x4_nt3_ms2_ne4"),
    ("conv", (2, 40, 64, 6, 10, 1, 2), "k1s1_kc32_w1x4_nt3_ms2_ne4_dil2"),
    ("conv", (5, 40, 64, 3, 5, 1, 1), "k1s1_kc32_w1x4_nt3_ms2_ne4_tn"),
    ("conv", (5, 40, 64, 3, 5, 1, 2), "k1s1_kc32_w1x4_nt3_ms2_ne4_tn_dil2"),
    ("conv", (2, 16, 64, 5, 7, 1, 1), "k1s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 16, 64, 5, 7, 1, 2), "k1s1_kc32_w2x2_nt1_ms2_ne4_dil2"),
    ("conv", (3, 16, 64, 3, 5, 1, 1), "k1s1_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (3, 16, 64, 3, 5, 1, 2), "k1s1_kc32_w2x2_nt1_ms2_ne4_tn_dil2"),
    ("conv", (32, 20, 64, 130, 127, 1, 1), "k1s1_kc32_w2x2_nt1_ms4_ne4"),
    ("conv", (32, 20, 64, 130, 127, 1, 2), "k1s1_kc32_w2x2_nt1_ms4_ne4_dil2"),
    ("conv", (2, 80, 64, 5, 7, 1, 1), "k1s1_kc32_w4x1_nt1_ms4_ne4"),
    ("conv", (2, 80, 64, 5, 7, 1, 2), "k1s1_kc32_w4x1_nt1_ms4_ne4_dil2"),
    ("conv", (3, 80, 64, 3, 5, 1, 1), "k1s1_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (3, 80, 64, 3, 5, 1, 2), "k1s1_kc32_w4x1_nt1_ms4_ne4_tn_dil2"),
    ("conv", (19, 80, 64, 130, 127, 1, 1), "k1s1_kc32_w4x1_nt1_ms8_ne4"),
    ("conv", (19, 80, 64, 130, 127, 1, 2), "k1s1_kc32_w4x1_nt1_ms8_ne4_dil2"),
    ("conv", (19, 40, 48, 1, 5, 3, 1), "k3s1_kc16_w1x4_nt3_ms2_ne10_tn"),
    ("conv", (19, 40, 48, 1, 5, 3, 2), "k3s1_kc16_w1x4_nt3_ms2_ne10_tn_dil2"),
    ("conv", (2, 40, 48, 6, 10, 3, 1), "k3s1_kc16_w1x4_nt3_ms2_ne4"),
    ("conv", (2, 40, 48, 6, 10, 3, 2), "k3s1_kc16_w1x4_nt3_ms2_ne4_dil2"),
    ("conv", (5, 40, 48, 3, 5, 3, 1), "k3s1_kc16_w1x4_nt3_ms2_ne4_tn"),
    ("conv", (5, 40, 48, 3, 5, 3, 2), "k3s1_kc16_w1x4_nt3_ms2_ne4_tn_dil2"),
    ("conv", (5, 40, 48, 2, 9, 3, 1), "k3s1_kc16_w1x4_nt3_ms2_ne6_tn"),
    ("conv", (5, 40, 48, 2, 9, 3, 2), "k3s1_kc16_w1x4_nt3_ms2_ne6_tn_dil2"),
    ("conv", (2, 16, 48, 5, 7, 3, 1), "k3s1_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 16, 48, 5, 7, 3, 2), "k3s1_kc16_w2x2_nt1_ms2_ne4_dil2"),
    ("conv", (3, 16, 48, 3, 5, 3, 1), "k3s1_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (3, 16, 48, 3, 5, 3, 2), "k3s1_kc16_w2x2_nt1_ms2_ne4_tn_dil2"),
    ("conv", (32, 20, 48, 130, 127, 3, 1), "k3s1_kc16_w2x2_nt1_ms4_ne4"),
    ("conv", (32, 20, 48, 130, 127, 3, 2), "k3s1_kc16_w2x2_nt1_ms4_ne4_dil2"),
    ("conv", (2, 80, 48, 5, 7, 3, 1), "k3s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (2, 80, 48, 5, 7, 3, 2), "k3s1_kc16_w4x1_nt1_ms4_ne4_dil2"),
    ("conv", (3, 80, 48, 3, 5, 3, 1), "k3s1_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (3, 80, 48, 3, 5, 3, 2), "k3s1_kc16_w4x1_nt1_ms4_ne4_tn_dil2"),
    ("conv", (19, 80, 48, 130, 127, 3, 1), "k3s1_kc16_w4x1_nt1_ms8_ne4"),
    ("conv", (19, 80, 48, 130, 127, 3, 2), "k3s1_kc16_w4x1_nt1_ms8_ne4_dil2"),
    ("conv", (19, 40, 64, 1, 5, 3, 1), "k3s1_kc32_w1x4_nt3_ms2_ne0_tn"),
    ("conv", (19, 40, 64, 1, 5, 3, 2), "k3s1_kc32_w1x4_nt3_ms2_ne0_tn_dil2"),
    ("conv", (5, 40, 64, 3, 5, 3, 1), "k3s1_kc32_w1x4_nt3_ms2_ne10_tn"),
    ("conv", (5, 40, 64, 3, 5, 3, 2), "k3s1_kc32_w1x4_nt3_ms2_ne10_tn_dil2"),
    ("conv", (2, 40, 64, 6, 10, 3, 1), "k3s1_kc32_w1x4_nt3_ms2_ne6"),
    ("conv", (2, 40, 64, 6, 10, 3, 2), "k3s1_kc32_w1x4_nt3_ms2_ne6_dil2"),
    ("conv", (11, 16, 64, 1, 5, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne10_tn"),
    ("conv", (11, 16, 64, 1, 5, 3, 2), "k3s1_kc32_w2x2_nt1_ms2_ne10_tn_dil2"),
    ("conv", (2, 16, 64, 5, 7, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 16, 64, 5, 7, 3, 2), "k3s1_kc32_w2x2_nt1_ms2_ne4_dil2"),
    ("conv", (3, 16, 64, 3, 5, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (3, 16, 64, 3, 5, 3, 2), "k3s1_kc32_w2x2_nt1_ms2_ne4_tn_dil2"),
    ("conv", (3, 16, 64, 2, 9, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne6_tn"),
    ("conv", (3, 16, 64, 2, 9, 3, 2), "k3s1_kc32_w2x2_nt1_ms2_ne6_tn_dil2"),
    ("conv", (32, 20, 64, 130, 127, 3, 1), "k3s1_kc32_w2x2_nt1_ms4_ne6"),
    ("conv", (32, 20, 64, 130, 127, 3, 2), "k3s1_kc32_w2x2_nt1_ms4_ne6_dil2"),
    ("conv", (11, 80, 64, 1, 5, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne10_tn"),
    ("conv", (11, 80, 64, 1, 5, 3, 2), "k3s1_kc32_w4x1_nt1_ms4_ne10_tn_dil2"),
    ("conv", (2, 80, 64, 5, 7, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne4"),
    ("conv", (2, 80, 64, 5, 7, 3, 2), "k3s1_kc32_w4x1_nt1_ms4_ne4_dil2"),
    ("conv", (3, 80, 64, 3, 5, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (3, 80, 64, 3, 5, 3, 2), "k3s1_kc32_w4x1_nt1_ms4_ne4_tn_dil2"),
    ("conv", (3, 80, 64, 2, 9, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne6_tn"),
    ("conv", (3, 80, 64, 2, 9, 3, 2), "k3s1_kc32_w4x1_nt1_ms4_ne6_tn_dil2"),
    ("conv", (19, 80, 64, 130, 127, 3, 1), "k3s1_kc32_w4x1_nt1_ms8_ne6"),
    ("conv", (19, 80, 64, 130, 127, 3, 2), "k3s1_kc32_w4x1_nt1_ms8_ne6_dil2"),
    ("deconv", (3, 16, 32, 2, 9, 4, 2), "k4s2_kc16_w4x1_nt1_ms4_ne10_tn"),
    ("deconv", (2, 16, 32, 5, 7, 4, 2), "k4s2_kc16_w4x1_nt1_ms4_ne6"),
    ("deconv", (3, 16, 32, 3, 5, 4, 2), "k4s2_kc16_w4x1_nt1_ms4_ne6_tn"),
]
DGRAD_EXTRA = [
    ("conv", (2, 16, 48, 8, 6, 3, 2), "k3s1_kc16_w2x2_nt1_ms2_ne4_dil2"),
    ("conv", (2, 40, 64, 7, 10, 3, 2), "k3s1_kc32_w1x4_nt3_ms2_ne6_dil2"),
    ("conv", (3, 16, 64, 4, 6, 3, 2), "k3s1_kc32_w2x2_nt1_ms2_ne4_tn_dil2"),
    ("conv", (2, 80, 64, 8, 8, 1, 2), "k1s1_kc32_w4x1_nt1_ms4_ne4_dil2"),
    ("conv", (2, 16, 16, 9, 7, 1, 2), "k1s1_kc16_w2x2_nt1_ms2_ne4_dil2"),
    ("conv", (2, 19, 32, 9, 7, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (2, 20, 16, 10, 14, 3, 2), "k3s1_kc16_w2x2_nt1_ms2_ne4_dil2"),
]
# the training forward: one row per form that keeps the batch-statistics partials (tiny_graphs.single: the conv "c" behind a stride-2 head),
# and the two forms of the transposed conv (tiny_graphs.deconv: "up", which never keeps them)
TRAIN_CASES = [
    ("conv", (2, 48, 16, 5, 7, 1, 1), "k1s1_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 48, 16, 3, 5, 1, 1), "k1s1_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (32, 48, 20, 130, 127, 1, 1), "k1s1_kc16_w2x2_nt1_ms4_ne4"),
    ("conv", (2, 48, 80, 5, 7, 1, 1), "k1s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 48, 80, 3, 5, 1, 1), "k1s1_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (19, 48, 80, 130, 127, 1, 1), "k1s1_kc16_w4x1_nt1_ms8_ne4"),
    ("conv", (2, 64, 16, 5, 7, 1, 1), "k1s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 64, 16, 3, 5, 1, 1), "k1s1_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (32, 64, 20, 130, 127, 1, 1), "k1s1_kc32_w2x2_nt1_ms4_ne4"),
    ("conv", (2, 64, 80, 5, 7, 1, 1), "k1s1_kc32_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 64, 80, 3, 5, 1, 1), "k1s1_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (19, 64, 80, 130, 127, 1, 1), "k1s1_kc32_w4x1_nt1_ms8_ne4"),
    ("conv", (2, 48, 16, 9, 7, 1, 2), "k1s2_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 48, 16, 5, 7, 1, 2), "k1s2_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (2, 48, 80, 9, 7, 1, 2), "k1s2_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 48, 80, 5, 7, 1, 2), "k1s2_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (2, 64, 16, 9, 7, 1, 2), "k1s2_kc32_w2x2_nt1_ms2_ne10"),
    ("conv", (3, 64, 16, 5, 7, 1, 2), "k1s2_kc32_w2x2_nt1_ms2_ne10_tn"),
    ("conv", (11, 64, 16, 1, 5, 1, 2), "k1s2_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (5, 64, 16, 3, 5, 1, 2), "k1s2_kc32_w2x2_nt1_ms2_ne6_tn"),
    ("conv", (2, 64, 80, 9, 7, 1, 2), "k1s2_kc32_w4x1_nt1_ms4_ne10"),
    ("conv", (3, 64, 80, 5, 7, 1, 2), "k1s2_kc32_w4x1_nt1_ms4_ne10_tn"),
    ("conv", (11, 64, 80, 1, 5, 1, 2), "k1s2_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (5, 64, 80, 4, 4, 1, 2), "k1s2_kc32_w4x1_nt1_ms4_ne6_tn"),
    ("conv", (2, 48, 16, 5, 7, 3, 1), "k3s1_kc16_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 48, 16, 3, 5, 3, 1), "k3s1_kc16_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (32, 48, 20, 130, 127, 3, 1), "k3s1_kc16_w2x2_nt1_ms4_ne4"),
    ("conv", (2, 48, 80, 5, 7, 3, 1), "k3s1_kc16_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 48, 80, 3, 5, 3, 1), "k3s1_kc16_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (19, 48, 80, 130, 127, 3, 1), "k3s1_kc16_w4x1_nt1_ms8_ne4"),
    ("conv", (11, 64, 16, 1, 5, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne10_tn"),
    ("conv", (2, 64, 16, 5, 7, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne4"),
    ("conv", (3, 64, 16, 3, 5, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne4_tn"),
    ("conv", (3, 64, 16, 2, 9, 3, 1), "k3s1_kc32_w2x2_nt1_ms2_ne6_tn"),
    ("conv", (32, 64, 20, 130, 127, 3, 1), "k3s1_kc32_w2x2_nt1_ms4_ne6"),
    ("conv", (11, 64, 80, 1, 5, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne10_tn"),
    ("conv", (2, 64, 80, 5, 7, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne4"),
    ("conv", (3, 64, 80, 3, 5, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne4_tn"),
    ("conv", (3, 64, 80, 2, 9, 3, 1), "k3s1_kc32_w4x1_nt1_ms4_ne6_tn"),
    ("conv", (19, 64, 80, 130, 127, 3, 1), "k3s1_kc32_w4x1_nt1_ms8_ne6"),
    ("conv", (11, 32, 16, 1, 5, 3, 2), "k3s2_kc16_w2x2_nt1_ms2_ne10_tn"),
    ("conv", (2, 32, 16, 9, 7, 3, 2), "k3s2_kc16_w2x2_nt1_ms2_ne6"),
    ("conv", (3, 32, 16, 5, 7, 3, 2), "k3s2_kc16_w2x2_nt1_ms2_ne6_tn"),
    ("conv", (11, 32, 80, 1, 5, 3, 2), "k3s2_kc16_w4x1_nt1_ms4_ne10_tn"),
    ("conv", (2, 32, 80, 9, 7, 3, 2), "k3s2_kc16_w4x1_nt1_ms4_ne6"),
    ("conv", (3, 32, 80, 5, 7, 3, 2), "k3s2_kc16_w4x1_nt1_ms4_ne6_tn"),
    ("deconv", (2, 32, 16, 3, 5, 4, 2), "k4s1_kc16_w4x1_nt1_ms4_ne4_dil2"),
    ("deconv", (3, 32, 16, 1, 5, 4, 2), "k4s1_kc16_w4x1_nt1_ms4_ne4_tn_dil2"),
]
# no form needs an exemption: the largest rows (32 images of 130 x 127 with 64 channels; 19 with 80) have 135 MB / 100 MB tensors
EXEMPT = {use: {} for use in mf.USES}  # use -> {form: (shape, why its smallest reaching shape is too large)}
FP32_PLAN = {"MVAL_CONV": "fp32"}
HEAD_CHANNELS = 32  # of the transposed-conv graphs (tiny_graphs.deconv(c, cmid, cup): the rows give cmid -> cup)
U = 2.0 ** -24  # unit roundoff of float32


def _opts(text):
    t = set(text.split("+")) - {""}
    up = [int(x[2:]) for x in t if x.startswith("up")]
    assert t <= {"relu", "res1", "res2", "nchw", "up1", "up2", "up3"}, text
    return dict(relu="relu" in t, res1="res1" in t, res2="res2" in t, nchw="nchw" in t, up=up[0] if up else 0)


def _fwd_id(row):
    kind, (n, cin, cout, h, w, k, s), opts, form = row
    return f"{form}-{kind}_n{n}_c{cin}-{cout}_{h}x{w}" + ("-" + opts if opts else "")


def _shape_id(row):
    kind, (n, cin, cout, h, w, k, s), form = row
    return f"{form}-{kind}_n{n}_c{cin}-{cout}_{h}x{w}"


def _fwd_form(row, n=None):
    kind, shape, opts, _ = row
    return mf.query("op", n or shape[0], *shape[1:], kind, **_opts(opts))


def _graph_of(row):
    """(builder name, its arguments, images, map size behind the stride-2 head, name of the conv under test) of a training row."""
    kind, (n, cin, cout, h, w, k, s), _ = row
    if kind == "deconv":  # head, max-pool to h x w, a 3x3 conv to cin channels, the transposed conv cin -> cout on h x w
        return "deconv", (HEAD_CHANNELS, cin, cout), n, (2 * h, 2 * w), "up"
    return "single", (cin, cout, k, s), n, (h, w), "c"


def _host_plan(row):
    from multi_view_active_learning_amd import engine_train as et

    graph, args, n, hw, _ = _graph_of(row)
    model = tg.TinyNet(tg.BUILDERS[graph], args, 1).train()
    return et.TrainPlan(model, n, 2 * hw[0], 2 * hw[1], torch.device("cpu"), sw=dict(et._SWITCHES, **FP32_PLAN))


def _plan_form(plan, conv, use, n):
    """(index, MfmaForm, algo) of the op named `conv` of a training plan under `use`, from the plan's own geometry."""
    i = next(j for j, op in enumerate(plan.graph.ops) if op.conv == conv)
    op, t = plan.graph.ops[i], plan.ops[i]
    hin, win = plan.geo[i][:2]
    f = mf.query(use, n, op.cin, op.cout, hin, win, op.k, op.stride, "deconv" if op.kind == "deconv" else "conv")
    return i, f, (t.dgrad_algo if use == "dgrad" else t.op.algo)


# ---- host tests (no GPU) ----
def test_mfma_form_mirror_matches_the_header():
    """_lib.MfmaForm restates struct mval_mfma_form of include/mval_hip.h, and the uses are the MVAL_SPLIT_USE_* of the split query."""
    from multi_view_active_learning_amd import _lib

    text = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    body = re.search(r"typedef struct mval_mfma_form \{(.*?)\} mval_mfma_form;", text, flags=re.S).group(1)
    fields = [name for line in body.split(";") if line.strip() for name in re.sub(r"^\s*int32_t", "", line).replace(" ", "").split(",")]
    assert fields == [name for name, _ in _lib.MfmaForm._fields_] and C.sizeof(_lib.MfmaForm) == 4 * len(fields)
    assert fields == ["ks", "s", "kc", "wn", "wm", "nt", "ms", "ne", "th", "tw", "tn", "dil", "nbuf", "grid_x", "grid_y", "bn_part_ok", "bn_part"]
    enum = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))
    assert [enum("MVAL_SPLIT_USE_" + n) for n in ("OP", "TRAIN_FWD", "DGRAD")] == [mf.USES.index(u) for u in mf.USES] == [0, 1, 2]
    assert re.search(r"int mval_conv_mfma_form\(int use, const mval_op\* op, int n_images, mval_mfma_form\* form\);", text)


def test_the_query_answers_like_the_support_predicate():
    """mval_conv_mfma_form returns "unsupported" exactly where mval_op_mfma_supported does (mval_launch_conv_mfma returns 1): a cin that is no
    multiple of 16, NCHW input, a pad other than (k - 1) / 2; the parity use has no exact-fp32 form; a transposed conv answers the stride-1 k4
    conv over the zero-dilated input (op, training forward) or the k4 stride-2 conv (data gradient); and it needs no GPU."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    lib = _lib.lib()
    seen = set()
    for cin, in_nchw, k, pad in [(32, 0, 3, 1), (24, 0, 3, 1), (40, 0, 1, 0), (16, 0, 1, 0), (32, 1, 3, 1), (32, 0, 3, 0), (32, 0, 1, 1), (48, 0, 3, 1), (3, 1, 3, 1)]:
        for n, h, w, cout in [(2, 16, 16, 32), (3, 3, 5, 19), (1, 64, 48, 144)]:
            ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
            op = _query_op(mf.OP_CONV, k, 1, pad, cin, cout, h, w, ho, wo, in_nchw=in_nchw, res1_off=-1, res2_off=-1, algo=mf.ALGO_MFMA)
            ok = bool(lib.mval_op_mfma_supported(C.byref(op), C.c_int(n)))
            assert ok == (cin % 16 == 0 and not in_nchw and pad == (k - 1) // 2), (cin, in_nchw, k, pad)
            for use in range(2):
                assert (_lib.conv_mfma_form(use, op, n) is not None) == ok, (use, cin, in_nchw, k, pad)
            # (the data gradient's conv reads dz: its cin is the conv's cout, its input NHWC whatever the conv's input is)
            assert (_lib.conv_mfma_form(2, op, n) is not None) == (cout % 16 == 0 and pad == (k - 1) // 2), (cin, cout, k, pad)
            assert _lib.conv_mfma_form(_lib.SPLIT_USE_DGRAD_PARITY, op, n) is None and _lib.conv_mfma_form(7, op, n) is None
            seen.add(ok)
    assert seen == {True, False}
    assert mf.query("op", 2, 24, 32, 16, 16, 3, 1) is None and mf.query("op", 2, 32, 32, 16, 16, 3, 1, in_nchw=True) is None
    assert mf.query("op", 2, 32, 32, 16, 16, 3, 1, pad=0) is None and mf.query("dgrad", 2, 32, 24, 16, 16, 3, 1) is None  # (the gradient's cin is cout)
    assert mf.query("dgrad", 2, 24, 32, 16, 16, 3, 1) is not None
    d = [mf.query(use, 2, 32, 48, 8, 6, 4, 2, "deconv") for use in mf.USES]
    assert [(f.ks, f.s, f.dil, f.kc) for f in d] == [(4, 1, 2, 16), (4, 1, 2, 16), (4, 2, 1, 16)] and not any(f.bn_part for f in d)
    assert (d[0].grid_x, d[2].grid_x) == (2 * 4 * 1, 2 * 1 * 1) and (d[0].grid_y, d[2].grid_y) == (1, 1)  # (16 x 12 output in 4 x 16 tiles; 8 x 6 in 8 x 8)
    f = mf.query("train", 3, 64, 256, 33, 31, 3, 1)  # (what the struct holds, on one launch)
    assert f.as_dict() == dict(ks=3, s=1, kc=32, wn=4, wm=1, nt=1, ms=4, ne=4, th=4, tw=16, tn=1, dil=1, nbuf=2, grid_x=3 * 9 * 2, grid_y=4,
                               bn_part_ok=1, bn_part=1)
    g = mf.query("op", 19, 32, 40, 1, 5, 3, 1)  # (the issue's example of the generic staging: one 32-channel chunk, 16 images per tile)
    assert (mf.name(g), g.tn, g.nbuf, g.grid_x) == ("k3s1_kc32_w1x4_nt3_ms2_ne0_tn", 16, 1, 2)


def test_every_row_takes_the_form_it_is_in_the_table_for():
    bad = []
    for row in FWD_CASES + FWD_EXTRA:
        f = _fwd_form(row)
        if f is None or mf.name(f) != row[3]:
            bad.append((_fwd_id(row), f and mf.name(f)))
    for kind, shape, form in DGRAD_CASES + DGRAD_EXTRA:
        for acc in (False, True):
            f = mf.query("dgrad", *shape, kind, res1=acc)
            if f is None or mf.name(f) != form:
                bad.append(("dgrad", kind, shape, f and mf.name(f)))
    for use, table, conv in (("train", TRAIN_CASES, None), ("dgrad", [r for r in DGRAD_CASES if r[0] == "deconv"], "up")):
        for row in table:
            plan = _host_plan(row)
            name = conv or _graph_of(row)[4]
            i, f, algo = _plan_form(plan, name, use, row[1][0])
            if f is None or mf.name(f) != row[2] or algo != mf.ALGO_MFMA:
                bad.append((use, _shape_id(row), f and mf.name(f), algo))
            elif use == "train":
                cout = plan.graph.ops[i].cout
                if bool(f.bn_part) != (row[0] == "conv") or (f.bn_part and not cout * f.grid_x * 2 <= plan.ws_lane):
                    bad.append((_shape_id(row), "partials", f.bn_part, cout * f.grid_x * 2, plan.ws_lane))
    assert not bad, bad
    ids = [_fwd_id(r) for r in FWD_CASES + FWD_EXTRA] + [_shape_id(r) for r in DGRAD_CASES + DGRAD_EXTRA]
    assert len(set(ids)) == len(ids)


def _train_forms(found):
    """The training-forward forms that want a row: those some shape of the sweep reaches with the partials kept, and the transposed conv's."""
    return {form for form, cases in found.items() if any(c[3] or c[0] == "deconv" for c in cases)}


@pytest.mark.parametrize("use", mf.USES)
def test_the_tables_name_every_form_the_sweep_finds(use):
    """Coverage and drift: the sweep's forms for this use (tests/mfma_forms.py: the documented domain, one pass of host arithmetic) are
    exactly the forms the use's table names (+ the exemptions, none at present).  A threshold change that creates a form without a row, or
    takes the last shape away from a row's form, fails here.  Found on this dispatch: 68 forms for mval_op_launch (66 convs + 2 of the
    transposed conv), 68 for the training forward -- 48 of them with a row: the 46 that keep the batch-statistics partials (the 20 forms of
    the three-cout-blocks-per-wave layout never do) and the transposed conv's 2 --, 81 for the data gradient (39 stride-1 forms, their 39
    zero-dilated twins, 3 k4 stride-2 forms): 110 distinct kernel forms in all (66 + 39 twins + 5 k4)."""
    found = mf.sweep(use)
    table = {"op": [r[3] for r in FWD_CASES], "train": [r[2] for r in TRAIN_CASES], "dgrad": [r[2] for r in DGRAD_CASES]}[use]
    want = _train_forms(found) if use == "train" else set(found)
    print(f"[mfma forms] {use}: {len(found)} forms ({sum('_dil2' in k for k in found)} zero-dilated, {sum(k.startswith('k4') for k in found)} k4, "
          f"{sum('_tn' in k for k in found)} with several images per tile, {sum('_ne0' in k for k in found)} generic staging); {len(want)} want a row")
    assert len(found) == {"op": 68, "train": 68, "dgrad": 81}[use] and len(want) == {"op": 68, "train": 48, "dgrad": 81}[use]
    missing = want - set(table) - set(EXEMPT[use])
    assert not missing, f"forms without a row: {sorted(missing)}"
    stale = set(table) - want
    assert not stale, f"rows whose form the sweep no longer finds: {sorted(stale)}"
    assert len(table) == len(set(table)) and not set(EXEMPT[use]) & set(table) and len(EXEMPT[use]) * 10 <= len(found)
    if use == "op":
        assert {r[3] for r in FWD_EXTRA} <= set(found)
    if use == "dgrad":
        assert {r[2] for r in DGRAD_EXTRA} <= set(found)
        distinct = set(mf.sweep("op")) | set(found)
        assert len(distinct) == 110 and set(mf.sweep("train")) == set(mf.sweep("op"))


@pytest.mark.parametrize("use", mf.USES)
def test_dispatch_facts_over_the_sweep(use):
    """What the launcher and the kernel rely on, stated from the query on every launch of the sweep: the tile fills the MT pixel slots exactly
    with powers of two (abase's shift decode); several images per tile only where the map's rows, rounded up to a power of two, are fewer
    than the tile's; the patch inside conv_div20's range; the generic staging exactly when the patch needs more than ten float4 per thread,
    and then one LDS buffer; two buffers exactly with more than one chunk on the register-staged forms; the cout groups cover cout; the grid
    covers the map and the batch; the partials possible exactly under mfma_forms.partials_rule, and kept exactly where they are possible and
    asked for (the training forward of a conv)."""
    bad = []
    pow2 = lambda v: v > 0 and v & (v - 1) == 0
    for form, cases in mf.sweep(use).items():
        for kind, shape, tile, part in cases:
            f = mf.query(use, *shape, kind)
            assert tile == (f.th, f.tw, f.tn) and part == f.bn_part
            n = shape[0]
            ci, co = mf.kernel_channels(use, shape)
            ho, wo = mf.grid_hw(use, kind, shape)
            ph, pw = (f.th - 1) * f.s + f.ks, (f.tw - 1) * f.s + f.ks
            per_thread = -(-(f.tn * ph * pw * (f.kc // 4)) // mf.NTH)
            hh = 1 << (ho - 1).bit_length()  # rows rounded up to a power of two
            ok = (f.th * f.tw * f.tn == 16 * f.ms * f.wm and pow2(f.th) and pow2(f.tw) and pow2(f.tn) and f.wn * f.wm == 4 and
                  (f.tn > 1) == (hh < 16 * f.ms * f.wm // f.tw) and (f.tn == 1 or f.th == hh) and f.tw == (16 if wo > 8 else 8) and
                  f.tn * ph * pw < 4096 and pw < 256 and ph < 256 and
                  f.ne == (4 if per_thread <= 4 else 6 if per_thread <= 6 else 10 if per_thread <= 10 else 0) and
                  (f.ne != 0 or f.nbuf == 1) and (f.nbuf == 2) == (ci // f.kc > 1 and f.ne != 0) and f.nbuf in (1, 2) and
                  ci % f.kc == 0 and f.kc == (32 if ci % 32 == 0 and not (f.ks == 3 and f.s == 2) and f.ks != 4 else 16) and
                  f.grid_y * f.wn * f.nt * 16 >= co and (f.grid_y - 1) * f.wn * f.nt * 16 < co and
                  f.grid_x == -(-ho // f.th) * -(-wo // f.tw) * -(-n // f.tn) and
                  f.dil == (2 if (kind == "deconv") != (use == "dgrad") and shape[6] == 2 else 1) and
                  bool(f.bn_part_ok) == mf.partials_rule(f, cout=co) and f.bn_part == (f.bn_part_ok if use == "train" and kind == "conv" else 0))
            if not ok:
                bad.append((form, kind, shape, f.as_dict()))
    assert not bad, bad[:5]


def test_partials_rule_with_the_epilogue_options():
    """The partials under the forward rows' epilogue options (residuals, ReLU, up-sampling, NCHW output, a cout that is no multiple of 4):
    possible exactly when mfma_forms.partials_rule says so, and mval_op_launch never asks for them; nor could a data gradient that accumulates."""
    seen = set()
    for row in FWD_CASES + FWD_EXTRA:
        o = _opts(row[2])
        for opts in (o, dict(relu=False, res1=False, res2=False, nchw=False, up=0)):
            f = mf.query("op", *row[1], row[0], **opts)
            assert bool(f.bn_part_ok) == mf.partials_rule(f, cout=row[1][2], **opts) and not f.bn_part, (_fwd_id(row), opts)
            seen.add((bool(f.bn_part_ok), any(opts.values())))
    assert seen == {(True, False), (False, False), (False, True)}
    assert not any(mf.query("dgrad", *shape, kind, res1=True).bn_part_ok for kind, shape, _ in DGRAD_CASES)


def _tables():
    return (("op", [(r[0], r[1], r[3]) for r in FWD_CASES]), ("train", TRAIN_CASES), ("dgrad", DGRAD_CASES))


def test_rows_carry_the_edges_they_were_chosen_for():
    """Every row: at least two images; with several images per tile a batch that is larger than, and no multiple of, the images per tile
    (two image groups or more, the last partly filled); a ragged last tile in columns, and in rows unless no shape of the sweep that reaches
    the form has both (the forms that hold all rows of a low map in one tile); a partly empty last cout group with a cout that is a multiple
    of 4; at least two channel chunks.  Over the forward table: both residuals with and without ReLU, up 1 .. 3 on 1x1 rows -- also with
    several images per tile --, NCHW output with one and with several images per tile, cout 19 and 20 on 3x3, one-chunk rows (cin 16) at 64-
    and 128-pixel tiles, the stride-2 1x1 conv on odd sizes, the transposed conv on a one-row map; the zero-dilated data gradient on even
    and on odd sizes in both directions."""
    bad = []
    for use, table in _tables():
        found = mf.sweep(use)
        for kind, shape, form in table:
            f = mf.query(use, *shape, kind)
            ci, co = mf.kernel_channels(use, shape)
            rows, cols = mf.ragged(use, kind, shape, (f.th, f.tw, f.tn))
            both = any(all(mf.ragged(use, c[0], c[1], c[2])) for c in found[form])
            ok = (shape[0] >= 2 and (f.tn == 1 or (shape[0] % f.tn and shape[0] > f.tn)) and cols and (rows or not both) and
                  (both or (f.tn > 1 and f.th >= mf.grid_hw(use, kind, shape)[0])) and co % (16 * f.nt * f.wn) and co % 4 == 0 and ci // f.kc >= 2)
            if not ok:
                bad.append((use, form, shape, f.as_dict()))
    assert not bad, bad
    fwd = FWD_CASES + FWD_EXTRA
    seen = {tuple(sorted(k_ for k_, v in _opts(r[2]).items() if v and k_ != "up")) for r in fwd}
    assert {(), ("relu",), ("res1",), ("relu", "res1"), ("res1", "res2"), ("relu", "res1", "res2"), ("nchw",), ("nchw", "relu")} <= seen, seen
    assert {_opts(r[2])["up"] for r in fwd if r[1][5] == 1} == {0, 1, 2, 3} and not any(_opts(r[2])["up"] for r in fwd if r[1][5] != 1)
    assert {_opts(r[2])["up"] for r in fwd if _fwd_form(r).tn > 1} == {0, 1, 2, 3}
    assert {_fwd_form(r).tn > 1 for r in fwd if _opts(r[2])["nchw"]} == {True, False}
    assert {19, 20} <= {r[1][2] for r in FWD_EXTRA if r[1][5] == 3}
    assert {16 * _fwd_form(r).ms * _fwd_form(r).wm for r in FWD_EXTRA if r[1][1] == 16 and r[1][5] == 3} == {64, 128}
    assert {16 * _fwd_form(r).ms * _fwd_form(r).wm for r in fwd if r[1][1] == 48 and r[1][5] == 3} >= {64, 128}
    assert any(r[1][5:] == (1, 2) and r[1][3] % 2 and r[1][4] % 2 for r in FWD_EXTRA) and any(r[0] == "deconv" and r[1][3] == 1 for r in fwd)
    assert any(r[0] == "deconv" and r[1][3:5] == (5, 7) for r in FWD_EXTRA)
    parities = {(r[1][3] % 2, r[1][4] % 2) for r in DGRAD_CASES + DGRAD_EXTRA if r[0] == "conv" and r[1][6] == 2}
    assert parities == {(0, 0), (0, 1), (1, 0), (1, 1)}, parities
    for k in (1, 3):  # every zero-dilated kernel size on an even and on an odd size
        assert {r[1][3] % 2 for r in DGRAD_CASES + DGRAD_EXTRA if r[0] == "conv" and r[1][5:] == (k, 2)} == {0, 1}


def test_forms_the_older_case_tables_reach():
    """The per-operator cases that predate this suite, held to the query: CONV_CASES and the transposed-conv shapes (test_gpu_models.py) reach
    13 of the 66 forward conv forms and 1 of the 2 transposed-conv forms -- none with several images per tile, the generic staging or ten
    staging slots on 3x3 stride 1 --, WG_CASES (test_gpu_train.py) 14 of the 81 data-gradient forms, without the generic staging and the k4
    stride-2 conv."""
    import test_gpu_models as tm
    import test_gpu_train as tt

    reached = set()
    for n, cin, cout, h, w, k, s, relu, r1, r2, up, nchw in tm.CONV_CASES:
        if cin % 16 == 0:
            reached.add(mf.name(mf.query("op", n, cin, cout, h, w, k, s, relu=relu, res1=r1, res2=r2, up=up, nchw=nchw)))
    deconv = {mf.name(mf.query("op", n, cin, cout, h, w, 4, 2, "deconv", relu=True)) for n, cin, cout, h, w in
              [(2, 64, 32, 8, 6), (3, 256, 256, 16, 12), (1, 2048, 256, 8, 6), (2, 32, 48, 5, 7)]}
    dgrad = {mf.name(mf.query("dgrad", *c)) for c in tt.WG_CASES if c[2] % 16 == 0}  # (the condition of test_conv_wgrad_and_dgrad_vs_torch)
    print(f"[mfma forms] the older tables reach {len(reached)} conv forms, {len(deconv)} transposed-conv form and {len(dgrad)} data-gradient forms: "
          f"{sorted(reached | deconv)} {sorted(dgrad)}")
    assert reached | deconv <= set(mf.sweep("op")) and dgrad <= set(mf.sweep("dgrad"))
    assert not any("_tn" in k or "_ne0" in k or k.startswith("k3s1") and "_ne10" in k for k in reached | deconv)
    assert not any("_ne0" in k or k.startswith("k4") for k in dgrad)
    assert (len(reached), len(deconv), len(dgrad)) == (13, 1, 14)


# ---- GPU ----
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _ref_conv(x, w, scale, shift, stride, relu, res1, res2, up, transposed):
    y = F.conv_transpose2d(x, w, None, stride=stride, padding=1) if transposed else F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2)
    y = y * scale[None, :, None, None] + shift[None, :, None, None]
    if up:
        y = F.interpolate(y, scale_factor=2 ** up, mode="nearest")
    for r in (res1, res2):
        if r is not None:
            y = y + r
    return F.relu(y) if relu else y


def _within(tag, got, want64, bound):
    """|got - want64| <= bound elementwise; returns the largest ratio (the figure the test prints)."""
    err = (got.double() - want64).abs()
    over = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max())
    assert not bool(over.any()), (tag, int(over.sum()), ratio, float(err.max()))
    return ratio


@functools.lru_cache(maxsize=2)
def _op_case(row):
    """Inputs as test_fused_conv_vs_torch_cpu makes them (+ a random sign on the scale), the float64 and the torch-CPU float32 result of the
    fused operator, and the a-priori bound  (K + 4) u (|scale| conv(|x|, |w|) + |shift| + |res1| + |res2|),  K = k k cin, u = 2^-24: K
    sequential float32 accumulations in any order and the epilogue's operations.  Computed once per row and never modified."""
    kind, (n, cin, cout, h, w, k, stride), opts, _ = row
    o = _opts(opts)
    transposed = kind == "deconv"
    rng = np.random.default_rng(zlib.crc32(_fwd_id(row).encode()))
    x = _f32(rng.standard_normal((n, cin, h, w)))
    taps = 4 if transposed else k * k  # (taps that meet one output pixel)
    wt = _f32(rng.standard_normal((cin, cout, k, k) if transposed else (cout, cin, k, k)) * np.sqrt(2.0 / (cin * taps)))
    scale = _f32(rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.5, -1.0, 1.0))
    shift = _f32(rng.standard_normal(cout) * 0.1)
    ho, wo = ((2 * h, 2 * w) if transposed else ((h - 1) // stride + 1, (w - 1) // stride + 1))
    ho, wo = ho << o["up"], wo << o["up"]
    res1 = _f32(rng.standard_normal((n, cout, ho, wo))) if o["res1"] else None
    res2 = _f32(rng.standard_normal((n, cout, ho, wo))) if o["res2"] else None
    return (x, wt, scale, shift, res1, res2) + _op_reference((x, wt, scale, shift, res1, res2), stride, o["relu"], o["up"], transposed)


def _op_reference(t, stride, relu, up, transposed):
    x, wt, scale, shift, res1, res2 = t
    d64 = lambda v: None if v is None else v.double()
    want64 = _ref_conv(x.double(), wt.double(), scale.double(), shift.double(), stride, relu, d64(res1), d64(res2), up, transposed)
    want32 = _ref_conv(x, wt, scale, shift, stride, relu, res1, res2, up, transposed)
    a64 = lambda v: None if v is None else v.double().abs()
    mag = _ref_conv(x.double().abs(), wt.double().abs(), scale.double().abs(), shift.double().abs(), stride, False, a64(res1), a64(res2), up, transposed)
    k, cin = wt.shape[-1], x.shape[1]
    return want64, want32, (k * k * cin + 4) * U * mag


def _poison(x):
    """Image 1 with a NaN in its first and +Inf in its last element (channel, row, column)."""
    y = x.clone()
    y[1, 0, 0, 0] = float("nan")
    y[1, -1, -1, -1] = float("inf")
    return y


@gpu
@pytest.mark.parametrize("row", FWD_CASES + FWD_EXTRA, ids=_fwd_id)
def test_mfma_forward_form_vs_float64(dev, row):
    """ops.fused_conv(algo=ALGO_MFMA) (mval_op_launch) on the row's form.  (1) the project's bound against torch-CPU float32: rtol 1e-4 /
    atol 2e-5 (3e-5 for the transposed conv); (2) the a-priori elementwise bound of _op_case against float64, which torch-CPU float32 must
    meet as well (so it cannot be vacuous; float32 sits at a few hundredths of it, a dropped or doubled product or a tap read from the wrong
    pixel hundreds of times above it); (3) NHWC with cout % 4 == 0: the kept per-image max |x| rows equal amax of the stored output, with
    several images per tile too (the per-image scratch path); (4) batch independence, bit for bit: the images in reversed order, and image 0
    alone (whatever form a batch of one takes); (5) with several images per tile and without ReLU: a NaN and a +Inf in image 1 leave every
    other image's bits alone, and image 1 is NaN exactly where float64 is."""
    from multi_view_active_learning_amd import ops

    kind, (n, cin, cout, h, w, k, stride), opts, form = row
    o = _opts(opts)
    f = _fwd_form(row)
    assert f is not None and mf.name(f) == form, "the case must run on the form it is in the table for"
    transposed = kind == "deconv"
    x, wt, scale, shift, res1, res2, want64, want32, bound = _op_case(row)
    nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, sd, bd = wt.to(dev), scale.to(dev), shift.to(dev)

    def run(xs, r1, r2, relu=o["relu"]):
        y = ops.fused_conv(nhwc(xs), wd, sd, bd, stride=stride, pad=1 if transposed else None, relu=relu, res1=nhwc(r1), res2=nhwc(r2), up=o["up"],
                           algo=mf.ALGO_MFMA, out_nchw=o["nchw"], kind=ops.OP_DECONV if transposed else ops.OP_CONV)
        kept = ops.fused_conv.last_out_amax.cpu().view(torch.float32)
        return (y.cpu() if o["nchw"] else y.permute(0, 3, 1, 2).cpu()), kept

    got, kept = run(x, res1, res2)
    r32, rgpu = _within("torch-CPU float32", want32, want64, bound), None
    try:
        rgpu = _within("the kernel", got, want64, bound)
    finally:
        print(f"[mfma forms] {_fwd_id(row)}: tile {f.th}x{f.tw}x{f.tn} grid {f.grid_x}x{f.grid_y} nbuf {f.nbuf}; max |err| / bound: kernel {rgpu}, "
              f"torch-CPU float32 {r32:.4f}")
    np.testing.assert_allclose(got.numpy(), want32.numpy(), rtol=1e-4, atol=3e-5 if transposed else 2e-5)
    if not o["nchw"] and cout % 4 == 0:  # (where the kernel keeps them: the float4 store path)
        assert torch.equal(kept, got.abs().amax(dim=(1, 2, 3))), "per-image max |x| rows"
    flip = lambda t: None if t is None else t.flip(0)
    rev, kept_rev = run(flip(x), flip(res1), flip(res2))
    assert _bits_equal(rev.flip(0), got), "every image has the same bits with the batch in reversed order"
    if not o["nchw"] and cout % 4 == 0:
        assert torch.equal(kept_rev.flip(0), kept)
    sub = lambda t: None if t is None else t[:1]
    alone, _ = run(x[:1], sub(res1), sub(res2))
    f1 = _fwd_form(row, n=1)
    assert _bits_equal(alone[0], got[0]), ("image 0 alone has the same bits", mf.name(f1), (f1.th, f1.tw, f1.tn))
    if f.tn > 1:
        clean, _ = run(x, res1, res2, relu=False)
        x2 = _poison(x)
        dirty, _ = run(x2, res1, res2, relu=False)
        keep = [i for i in range(n) if i != 1]
        assert _bits_equal(dirty[keep], clean[keep]), "a NaN / Inf in image 1 reaches no other image of its tile"
        w64, _, _ = _op_reference((x2[1:2], wt, scale, shift, None if res1 is None else res1[1:2], None if res2 is None else res2[1:2]), stride, False,
                                  o["up"], transposed)
        assert torch.equal(torch.isnan(dirty[1]), torch.isnan(w64[0])) and bool(torch.isnan(w64).any()) and not bool(torch.isnan(w64).all())


def _dgrad_reference(t, shape):
    dz, wt, base = t
    n, cin, cout, h, w, k, s = shape
    ho, wo = dz.shape[2:]
    pad = k // 2
    opad = (h - ((ho - 1) * s - 2 * pad + k), w - ((wo - 1) * s - 2 * pad + k))
    dx = lambda a, b: F.conv_transpose2d(a, b, None, stride=s, padding=pad, output_padding=opad)
    want64 = {False: dx(dz.double(), wt.double())}
    want64[True] = want64[False] + base.double()
    want32 = {False: dx(dz, wt)}
    want32[True] = want32[False] + base
    mag = dx(dz.double().abs(), wt.double().abs())
    bound = {False: (k * k * cout + 4) * U * mag, True: (k * k * cout + 4) * U * (mag + base.double().abs())}
    return want64, want32, bound


@functools.lru_cache(maxsize=2)
def _dgrad_case(row):
    """dz, the weight and a base to accumulate into; the float64 and torch-CPU float32 data gradient (stored, and added to the base); the
    a-priori bound (K + 4) u (conv^T(|dz|, |w|) + |base|), K = k k cout.  Computed once per row and never modified."""
    kind, shape, _ = row
    n, cin, cout, h, w, k, s = shape
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    rng = np.random.default_rng(zlib.crc32(_shape_id(row).encode()))
    dz = _f32(rng.standard_normal((n, cout, ho, wo)))
    wt = _f32(rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cout * k * k)))
    base = _f32(rng.standard_normal((n, cin, h, w)))
    return (dz, wt, base) + _dgrad_reference((dz, wt, base), shape)


@gpu
@pytest.mark.parametrize("row", [r for r in DGRAD_CASES + DGRAD_EXTRA if r[0] == "conv"], ids=_shape_id)
def test_mfma_dgrad_form_vs_float64(dev, row):
    """ops.conv_dgrad(algo=ALGO_MFMA) (mval_conv_dgrad) on the row's form, stride 1 and the zero-dilated stride 2, stored over stale contents
    and accumulated into a base: assertions (1), (2), (4) and (5) of the forward test (the kernel keeps no max |x| rows here)."""
    from multi_view_active_learning_amd import ops

    kind, shape, form = row
    n, cin, cout, h, w, k, s = shape
    dz, wt, base, want64, want32, bound = _dgrad_case(row)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = wt.to(dev)

    def run(dzs, bs, acc):
        into = nhwc(bs) if acc else None
        out = ops.conv_dgrad(nhwc(dzs), wd, (h, w), stride=s, algo=mf.ALGO_MFMA, accumulate_into=into)
        return out.permute(0, 3, 1, 2).cpu()

    for acc in (False, True):
        f = mf.query("dgrad", *shape, kind, res1=acc)
        assert f is not None and mf.name(f) == form, "the case must run on the form it is in the table for"
        got = run(dz, base, acc)
        r32, rgpu = _within("torch-CPU float32", want32[acc], want64[acc], bound[acc]), None
        try:
            rgpu = _within("the kernel", got, want64[acc], bound[acc])
        finally:
            print(f"[mfma forms] {_shape_id(row)} accumulate={int(acc)}: tile {f.th}x{f.tw}x{f.tn} grid {f.grid_x}x{f.grid_y} nbuf {f.nbuf}; "
                  f"max |err| / bound: kernel {rgpu}, torch-CPU float32 {r32:.4f}")
        np.testing.assert_allclose(got.numpy(), want32[acc].numpy(), rtol=1e-4, atol=2e-5)
        assert _bits_equal(run(dz.flip(0), base.flip(0), acc).flip(0), got), "every image has the same bits with the batch in reversed order"
        assert _bits_equal(run(dz[:1], base[:1], acc)[0], got[0]), "image 0 alone has the same bits"
        if f.tn > 1:
            dz2 = _poison(dz)
            dirty = run(dz2, base, acc)
            keep = [i for i in range(n) if i != 1]
            assert _bits_equal(dirty[keep], got[keep]), "a NaN / Inf in image 1 reaches no other image of its tile"
            w64 = _dgrad_reference((dz2[1:2], wt, base[1:2]), (1,) + shape[1:])[0][acc]
            assert torch.equal(torch.isnan(dirty[1]), torch.isnan(w64[0])) and bool(torch.isnan(w64).any()) and not bool(torch.isnan(w64).all())


# (n, cin, cout, h, w, k, stride, pad) of a conv x [n, cin, h, w] -> [n, cout, ho, wo] on maps whose output has one row (the last: two rows,
# which always fitted); k4 s2 p1 is the weight gradient of a transposed conv with the activations' roles swapped
WGRAD_LOW_MAPS = [(11, 64, 16, 1, 5, 3, 1, 1), (19, 32, 16, 1, 13, 3, 1, 1), (11, 32, 80, 1, 5, 3, 2, 1), (3, 16, 32, 2, 10, 4, 2, 1), (5, 48, 16, 2, 9, 3, 1, 1)]


@gpu
@pytest.mark.parametrize("case", WGRAD_LOW_MAPS, ids=lambda c: "n%d_c%d-%d_%dx%d_k%ds%dp%d" % c)
def test_fp32_weight_gradient_on_one_row_maps(dev, case):
    """mval_conv_wgrad (the weight gradient of the MVAL_CONV=fp32 plan, which the training rows below run) where the halos of the 8 (4 on 16-wide
    tiles) images that a 64-pixel tile of one-row maps would hold exceed the kernel's staging registers: the launcher takes a taller tile
    with fewer images -- it used to refuse the launch, and the training step with it.  Relative L2 < 2e-5 against float64 autograd, the
    bound of test_conv_wgrad_and_dgrad_vs_torch."""
    from multi_view_active_learning_amd import _lib

    n, cin, cout, h, w, k, s, pad = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    x = _f32(rng.standard_normal((n, cin, h, w)))
    wt = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double(), wt, None, stride=s, padding=pad)
    dz = _f32(rng.standard_normal(tuple(y.shape)))
    (want,) = torch.autograd.grad(y, wt, dz.double())
    ho, wo = y.shape[2:]
    assert ho <= 2
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev)
    xd, dzd = nhwc(x), nhwc(dz)
    lib, p = _lib.lib(), _lib._p
    lib.mval_conv_wgrad_workspace_floats.restype = C.c_size_t
    ws = torch.empty(int(lib.mval_conv_wgrad_workspace_floats(C.c_int(cin), C.c_int(cout), C.c_int(k))) + 64, device=dev)
    dw = torch.full((cout, cin, k, k), float("nan"), device=dev)
    _lib._check(lib.mval_conv_wgrad(p(xd), p(dzd), p(dw), p(ws), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(cin), C.c_int(ho), C.c_int(wo), C.c_int(cout),
                                    C.c_int(k), C.c_int(s), C.c_int(pad), C.c_int(0), _lib._stream()), "wgrad")
    e = tg.rel_l2(dw.cpu().numpy(), want.numpy())
    print(f"[mfma forms] weight gradient {case}: rel L2 {e:.2e}")
    assert e < 2e-5, e


# ---- the training step (MVAL_CONV=fp32) on one-conv graphs ----
TAU = 1.2e-3  # as tests/golden/make_small_graph_inputs.py: ~400 x the float32 - float64 differences of a pre-activation
WIDEN_LIMIT = 200000  # pre-activations of a graph up to which its input is moved off the ReLUs' zeros (and its gradients are compared)


def _widened_input(model, x):
    """The procedure of tests/golden/make_small_graph_inputs.py on the float64 reference alone: while a ReLU pre-activation lies within TAU of
    zero, move x along that pre-activation's own gradient until it sits 1.5 TAU away.  None for graphs above WIDEN_LIMIT pre-activations."""
    sd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in model.state_dict().items()}
    x = x.double()
    for _ in range(60):
        x.requires_grad_(True)
        _, pre = tg.graph_forward(model._graph, {k: v.clone() for k, v in sd.items()}, x, torch.float64)
        flat = torch.cat([p.reshape(-1) for p in pre.values()])
        if flat.numel() > WIDEN_LIMIT:
            return None
        idx = torch.nonzero(flat.abs() < TAU).reshape(-1)
        if idx.numel() == 0:
            return x.detach().float()
        idx = idx[torch.argsort(flat[idx].abs())][:256]
        step = torch.zeros_like(x)
        for j in idx.tolist():
            (gr,) = torch.autograd.grad(flat[j], x, retain_graph=True)
            v = float(flat[j].detach())
            step += (1.5 * TAU * (1.0 if v >= 0 else -1.0) - v) * gr / float((gr * gr).sum())
        x = (x + step).detach()
    raise RuntimeError("no ReLU margin after 60 rounds")


@functools.lru_cache(maxsize=1)
def _train_case(graph, args, n, hw, conv):
    """One training graph on the CPU, computed once: the input (moved off the ReLUs' zeros where the graph is small enough), the output
    gradient, and in float64 and float32 the output, the raw output z of the conv under test with its batch mean and 1 / sqrt(var + eps), the
    running statistics after the step, every parameter gradient and the gradient of that conv's input."""
    model = tg.TinyNet(tg.BUILDERS[graph], args, 1)
    g_ = model._graph
    seeded = tg.seeded_input(dict(n=n, hw=hw, seed=1))
    x = _widened_input(model, seeded)
    widened = x is not None
    x = x if widened else seeded
    keys = [k for k, _ in model.named_parameters()]
    op = next(o for o in g_.ops if o.conv == conv)
    res = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: (v.detach().clone().to(dt) if v.dtype.is_floating_point else v.detach().clone()) for k, v in model.state_dict().items()}
        leaves = [sd[k].requires_grad_(True) for k in keys]
        acts = {}
        out, pre = tg.graph_forward(g_, sd, x, dt, acts)
        if dt == torch.float64:
            gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1001))
        src = acts[op.src]
        grads = torch.autograd.grad((out * gout.to(dt)).sum(), leaves + [src]) if widened else None
        with torch.no_grad():
            wgt = sd[op.conv + ".weight"]
            z = F.conv_transpose2d(src, wgt, None, stride=op.stride, padding=op.pad) if op.kind == "deconv" else F.conv2d(src, wgt, None, stride=op.stride, padding=op.pad)
            mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        res[dt] = dict(out=out.detach(), z=z, mean=mean, invstd=1.0 / torch.sqrt(var + tg.BN_EPS), pre={i: v.detach() for i, v in pre.items()},
                       stats={k: v.detach().double().numpy() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))},
                       grads=None if grads is None else {k: v.double().numpy() for k, v in zip(keys, grads[:-1])},
                       dsrc=None if grads is None else grads[-1].detach())
    if widened:  # the condition of test_small_graph_training_step_vs_float64: no ReLU mask flips within float32's own error
        f64, f32 = res[torch.float64]["pre"], res[torch.float32]["pre"]
        margins = [float(f64[i].abs().min()) / max(float((f32[i].double() - f64[i]).abs().max()), 1e-300) for i in f64]
        assert min(margins) > 64.0, margins
    return x, gout, widened, res


def _train_step(dev, monkeypatch, row, epi, backward):
    """One forward (+ backward) of the row's graph under MVAL_CONV=fp32 with MVAL_TRAIN_EPI_STATS=epi -> (model, plan, output)."""
    from multi_view_active_learning_amd import engine_train as et

    graph, args, n, hw, conv = _graph_of(row)
    x, gout, widened, _ = _train_case(graph, args, n, hw, conv)
    for k_ in et._SWITCHES:
        monkeypatch.delenv(k_, raising=False)
    for k_, v in dict(FP32_PLAN, MVAL_TRAIN_EPI_STATS=epi).items():
        monkeypatch.setenv(k_, v)
    model = tg.TinyNet(tg.BUILDERS[graph], args, 1).to(dev).train()
    if backward:
        out = model(x.to(dev))
        out.backward(gout.to(dev))
    else:
        with torch.no_grad():
            out = model(x.to(dev))
    plan = next(iter(model._train_plans.values()))
    assert all(bool(t.p2_flags & et.TRAIN_STATS_PASS) == (epi == "0") for t in plan.ops) and not plan.uses_p2
    return model, plan, out.detach()


@gpu
@pytest.mark.parametrize("row", TRAIN_CASES, ids=_shape_id)
def test_mfma_training_form_vs_float64(dev, row, monkeypatch):
    """One training step of a one-conv graph (tiny_graphs.single; tiny_graphs.deconv for the transposed conv) under MVAL_CONV=fp32, with the
    batch statistics from the conv epilogue's partials and, under MVAL_TRAIN_EPI_STATS=0, from the separate pass: the conv under test runs on
    the row's form; its raw output z and the network's output within rtol 2e-5 / atol 2e-5 x max of float64, its batch mean and
    1 / sqrt(var + eps) and every running statistic within rtol 2e-4 / atol 2e-5, every parameter gradient within e <= 2 floor + 2e-5 (the
    bounds of test_small_graph_training_step_vs_float64).  The gradient bound needs an input on which no ReLU mask flips within float32's
    own error; it is made at run time (_widened_input) for graphs of up to WIDEN_LIMIT pre-activations -- all rows but the eight of the
    128-pixel-tile forms that need a million output elements, whose step runs forward only."""
    from multi_view_active_learning_amd.engine import _align
    from test_train_small_graphs import _gradient_check

    kind, (n, cin, cout, h, w, k, s), form = row
    graph, args, _, hw, conv = _graph_of(row)
    x, gout, widened, ref = _train_case(graph, args, n, hw, conv)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert widened or n * h * w * cout > 1 << 20
    for epi in ("1", "0"):
        model, plan, out = _train_step(dev, monkeypatch, row, epi, widened)
        i, f, algo = _plan_form(plan, conv, "train", n)
        assert f is not None and mf.name(f) == form and algo == mf.ALGO_MFMA and bool(f.bn_part) == (kind == "conv"), (f and mf.name(f), algo)
        t = plan.ops[i]
        zs = r64["z"].shape
        z = plan.arena[t.z_off : t.z_off + r64["z"].numel()].reshape(zs[0], zs[2], zs[3], zs[1]).permute(0, 3, 1, 2).cpu()
        so = plan.stat_off[i]
        mean, invstd = plan.stats[so : so + cout].cpu(), plan.stats[so + _align(cout) : so + _align(cout) + cout].cpu()
        tag = f"{_shape_id(row)} EPI_STATS={epi}"
        print(f"[mfma forms] {tag}: max |dz| {float((z.double() - r64['z']).abs().max()):.2e}, max |d mean| {float((mean.double() - r64['mean']).abs().max()):.2e}, "
              f"max rel d invstd {float(((invstd.double() - r64['invstd']) / r64['invstd']).abs().max()):.2e}; gradients compared: {widened}")
        np.testing.assert_allclose(z.numpy(), r64["z"].numpy(), rtol=2e-5, atol=2e-5 * float(r64["z"].abs().max()), err_msg=tag + " z")
        np.testing.assert_allclose(mean.numpy(), r64["mean"].numpy(), rtol=2e-4, atol=2e-5, err_msg=tag + " mean")
        np.testing.assert_allclose(invstd.numpy(), r64["invstd"].numpy(), rtol=2e-4, atol=2e-5, err_msg=tag + " invstd")
        want_out = r64["out"].numpy()
        np.testing.assert_allclose(out.cpu().numpy(), want_out, rtol=2e-5, atol=2e-5 * float(np.abs(want_out).max()), err_msg=tag)
        stats = {k_: v.cpu().numpy() for k_, v in model.state_dict().items() if k_.endswith(("running_mean", "running_var"))}
        assert set(stats) == set(r64["stats"])
        for k_, v in stats.items():
            np.testing.assert_allclose(v, r64["stats"][k_], rtol=2e-4, atol=2e-5, err_msg=f"{k_} {tag}")
        if widened:
            _gradient_check(tag, model, r64["grads"], r32["grads"], 2.0)


@gpu
@pytest.mark.parametrize("row", [r for r in DGRAD_CASES if r[0] == "deconv"], ids=_shape_id)
def test_mfma_transposed_conv_dgrad_form_vs_float64(dev, row, monkeypatch):
    """The k4 stride-2 conv that mval_train_backward runs as the data gradient of a transposed conv, inside a training step of
    tiny_graphs.deconv under MVAL_CONV=fp32: it runs on the row's form, and the gradient of the transposed conv's input (read from the
    plan's gradient arena) is within e <= 2 floor + 2e-5 of float64 autograd (e: relative L2; floor: torch-CPU float32's), as every
    parameter gradient is."""
    from test_train_small_graphs import _gradient_check

    kind, (n, cin, cout, h, w, k, s), form = row
    graph, args, _, hw, conv = _graph_of(row)
    x, gout, widened, ref = _train_case(graph, args, n, hw, conv)
    assert widened
    model, plan, out = _train_step(dev, monkeypatch, row, "1", True)
    i, f, algo = _plan_form(plan, conv, "dgrad", n)
    assert f is not None and mf.name(f) == form and algo == mf.ALGO_MFMA and (f.ks, f.s) == (4, 2), (f and mf.name(f), algo)
    t = plan.ops[i]
    assert t.gin_off >= 0 and t.first_touch & 1  # (stored, not accumulated: the transposed conv is the only reader of its input)
    got = plan.garena[t.gin_off : t.gin_off + n * h * w * cin].reshape(n, h, w, cin).permute(0, 3, 1, 2).cpu().numpy()
    want, floor_of = ref[torch.float64]["dsrc"].numpy(), ref[torch.float32]["dsrc"].double().numpy()
    e, floor = tg.rel_l2(got, want), tg.rel_l2(floor_of, want)
    print(f"[mfma forms] {_shape_id(row)}: tile {f.th}x{f.tw}x{f.tn} grid {f.grid_x}x{f.grid_y}; gradient of the transposed conv's input: e {e:.2e}, floor {floor:.2e}")
    assert e <= 2.0 * floor + 2e-5, (e, floor)
    _gradient_check(_shape_id(row), model, ref[torch.float64]["grads"], ref[torch.float32]["grads"], 2.0)

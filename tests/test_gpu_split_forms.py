"""The split-MFMA conv (csrc/conv_mfma_split.hip: the bf16x3 and fp16x2 kernels behind the h2 / bf3 inference plans, the training forward of
every non-P2 plan, every stride-1 and zero-dilated data gradient and the four-parity 2x2 form) at every kernel form its dispatch can pick.

Which form a launch runs on is read from the library's own dispatch (mval_conv_split_form: the launcher's dry run, host arithmetic, no GPU;
tests/split_forms.py names the forms and holds the sweep).  The host tests hold every row of the case tables to the form it is in the table
for and the tables to every form a fixed sweep of shapes finds, per use of the kernel -- so a re-tuned threshold that moves a case to another
form, or creates a form without a row, fails here and not silently.  The GPU tests run each row against float64 under the bounds the
per-operator tests already use (test_gpu_models.py::test_fused_conv_vs_torch_cpu, test_gpu_train_entries.py::
test_conv_dgrad_scaled_h2_vs_float64, test_train_small_graphs.py::test_small_graph_training_step_vs_float64) and repeat the form assertion
on the shape they ran.

Rows were chosen from the sweep as the cheapest shape (device tensors + float64 reference) that reaches the form with, where the form's
tile allows it, a ragged last tile in rows and columns, a batch the images-per-tile count does not divide, a cout that leaves the last cout
sub-tile or wave partly or wholly empty, and at least two images."""
import ctypes as C
import functools
import os
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_forms as sf
import tiny_graphs as tg

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the case tables ----
# FWD_CASES / FWD_EXTRA: (split, "conv" | "deconv" (ConvTranspose2d k4 s2 p1), (n, cin, cout, h, w, k, stride) of the conv on an h x w input,
# epilogue options, the form the row is in the table for).  Options: relu, res1, res2, up1 .. up3 (nearest up-sampling, 1x1 only), nchw
# (NCHW output), mag (fp16x2: the images differ in magnitude by 2^10 -- every image but the last is scaled by 2^-10, so that a per-image
# scale read from another image's row either overflows fp16 or loses ten bits).  FWD_EXTRA: the cases that belong to no single form -- 3x3
# with cout 19 / 20 (NHWC: the scalar store path for 19, the float4 path with a ragged quad range for 20; NCHW: the scalar path), cin 48
# (a half-empty second chunk) at 64- and 32-pixel tiles, the stride-2 1x1 conv on odd input sizes.
FWD_CASES = [
    ("bf3", "conv", (2, 32, 16, 5, 41, 1, 1), "", "bf3_k1s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (3, 32, 16, 5, 41, 1, 2), "relu+up1", "bf3_k1s1_w2x2_nt1_ms2_ne6_tn"),
    ("bf3", "conv", (8, 32, 16, 130, 127, 1, 1), "res1", "bf3_k1s1_w2x2_nt1_ms4_ne6_pow2"),
    ("bf3", "conv", (2, 32, 48, 3, 5, 1, 1), "relu+res1+up3", "bf3_k1s1_w3x1_nt1_ms1_ne6_pow2"),
    ("bf3", "conv", (3, 32, 48, 1, 5, 1, 2), "res1+res2", "bf3_k1s1_w3x1_nt1_ms1_ne6_tn"),
    ("bf3", "conv", (32, 32, 96, 5, 41, 1, 1), "relu+res1+res2", "bf3_k1s1_w3x1_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (8, 32, 144, 33, 31, 1, 1), "", "bf3_k1s1_w3x1_nt1_ms4_ne6_pow2"),
    ("bf3", "conv", (2, 48, 64, 3, 5, 1, 1), "relu+up3", "bf3_k1s1_w4x1_nt1_ms1_g2_pow2"),
    ("bf3", "conv", (3, 48, 64, 1, 5, 1, 2), "res1", "bf3_k1s1_w4x1_nt1_ms1_g2_tn"),
    ("bf3", "conv", (2, 32, 80, 3, 5, 1, 1), "relu+res1+up1", "bf3_k1s1_w4x1_nt1_ms1_ne6_pow2"),
    ("bf3", "conv", (3, 32, 80, 1, 5, 1, 2), "res1+res2+up2", "bf3_k1s1_w4x1_nt1_ms1_ne6_tn"),
    ("bf3", "conv", (3, 48, 256, 33, 31, 1, 1), "relu+res1+res2", "bf3_k1s1_w4x1_nt1_ms2_g2_pow2"),
    ("bf3", "conv", (32, 32, 80, 5, 41, 1, 1), "", "bf3_k1s1_w4x1_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (8, 48, 192, 33, 31, 1, 1), "relu", "bf3_k1s1_w4x1_nt1_ms4_g2_pow2"),
    ("bf3", "conv", (8, 32, 80, 47, 37, 1, 1), "res1", "bf3_k1s1_w4x1_nt1_ms4_ne6_pow2"),
    ("bf3", "conv", (32, 48, 256, 33, 31, 1, 1), "relu+res1", "bf3_k1s1_w4x1_nt2_ms4_g2_pow2"),
    ("bf3", "deconv", (2, 32, 16, 5, 41, 4, 2), "res1+res2", "bf3_k2s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", "deconv", (3, 32, 16, 3, 5, 4, 2), "relu+res1+res2", "bf3_k2s1_w2x2_nt1_ms2_ne6_tn"),
    ("bf3", "deconv", (8, 32, 16, 130, 127, 4, 2), "", "bf3_k2s1_w2x2_nt1_ms4_ne6_pow2"),
    ("bf3", "deconv", (2, 32, 40, 3, 5, 4, 2), "relu", "bf3_k2s1_w3x1_nt1_ms1_ne6_pow2"),
    ("bf3", "deconv", (3, 32, 40, 1, 5, 4, 2), "res1", "bf3_k2s1_w3x1_nt1_ms1_ne6_tn"),
    ("bf3", "deconv", (3, 32, 40, 33, 31, 4, 2), "relu+res1", "bf3_k2s1_w3x1_nt1_ms2_ne6_pow2"),
    ("bf3", "deconv", (32, 32, 40, 5, 41, 4, 2), "res1+res2", "bf3_k2s1_w3x1_nt1_ms4_ne6_pow2"),
    ("bf3", "deconv", (2, 32, 80, 3, 5, 4, 2), "relu+res1+res2", "bf3_k2s1_w4x1_nt1_ms1_ne6_pow2"),
    ("bf3", "deconv", (3, 32, 80, 1, 5, 4, 2), "", "bf3_k2s1_w4x1_nt1_ms1_ne6_tn"),
    ("bf3", "deconv", (8, 32, 80, 5, 41, 4, 2), "relu", "bf3_k2s1_w4x1_nt1_ms2_ne6_pow2"),
    ("bf3", "deconv", (3, 32, 80, 33, 31, 4, 2), "res1", "bf3_k2s1_w4x1_nt1_ms4_ne6_pow2"),
    ("bf3", "conv", (5, 32, 16, 1, 13, 3, 1), "relu+res1", "bf3_k3s1_w2x2_nt1_ms2_ne10_tn"),
    ("bf3", "conv", (2, 32, 16, 9, 37, 3, 1), "res1+res2", "bf3_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (3, 32, 16, 3, 5, 3, 1), "relu+res1+res2", "bf3_k3s1_w2x2_nt1_ms2_ne6_tn"),
    ("bf3", "conv", (2, 32, 16, 5, 41, 3, 1), "", "bf3_k3s1_w2x2_nt1_ms2_rows_pow2"),
    ("bf3", "conv", (8, 32, 16, 129, 129, 3, 1), "relu", "bf3_k3s1_w2x2_nt1_ms4_ne6_pow2"),
    ("bf3", "conv", (8, 32, 16, 130, 127, 3, 1), "res1", "bf3_k3s1_w2x2_nt1_ms4_rows_pow2"),
    ("bf3", "conv", (2, 32, 40, 3, 5, 3, 1), "relu+res1", "bf3_k3s1_w3x1_nt1_ms1_ne6_pow2"),
    ("bf3", "conv", (3, 32, 40, 1, 5, 3, 1), "res1+res2", "bf3_k3s1_w3x1_nt1_ms1_ne6_tn"),
    ("bf3", "conv", (2, 32, 40, 5, 41, 3, 1), "relu+res1+res2", "bf3_k3s1_w3x1_nt1_ms1_rows_pow2"),
    ("bf3", "conv", (32, 32, 40, 5, 41, 3, 1), "", "bf3_k3s1_w3x1_nt1_ms4_ne6_odd"),
    ("bf3", "conv", (3, 32, 40, 47, 37, 3, 1), "relu", "bf3_k3s1_w3x1_nt1_ms4_ne6_pow2"),
    ("bf3", "conv", (5, 32, 40, 33, 31, 3, 1), "res1", "bf3_k3s1_w3x1_nt1_ms4_rows_pow2"),
    ("bf3", "conv", (2, 32, 80, 3, 5, 3, 1), "relu+res1", "bf3_k3s1_w4x1_nt1_ms1_ne6_pow2"),
    ("bf3", "conv", (3, 32, 80, 1, 5, 3, 1), "res1+res2", "bf3_k3s1_w4x1_nt1_ms1_ne6_tn"),
    ("bf3", "conv", (2, 32, 80, 5, 41, 3, 1), "relu+res1+res2", "bf3_k3s1_w4x1_nt1_ms1_rows_pow2"),
    ("bf3", "conv", (32, 32, 80, 5, 41, 3, 1), "", "bf3_k3s1_w4x1_nt1_ms4_ne6_odd"),
    ("bf3", "conv", (2, 32, 80, 47, 37, 3, 1), "relu", "bf3_k3s1_w4x1_nt1_ms4_ne6_pow2"),
    ("bf3", "conv", (3, 32, 80, 33, 31, 3, 1), "res1", "bf3_k3s1_w4x1_nt1_ms4_rows_pow2"),
    ("bf3", "conv", (5, 32, 16, 1, 5, 3, 2), "relu+res1", "bf3_k3s2_w2x2_nt1_ms1_ne10_tn"),
    ("bf3", "conv", (2, 32, 16, 9, 37, 3, 2), "res1+res2", "bf3_k3s2_w2x2_nt1_ms1_ne6_pow2"),
    ("bf3", "conv", (3, 32, 16, 4, 4, 3, 2), "relu+res1+res2", "bf3_k3s2_w2x2_nt1_ms1_ne6_tn"),
    ("bf3", "conv", (2, 32, 40, 9, 37, 3, 2), "", "bf3_k3s2_w3x1_nt1_ms2_ne10_odd"),
    ("bf3", "conv", (2, 32, 40, 34, 42, 3, 2), "relu", "bf3_k3s2_w3x1_nt1_ms2_ne10_pow2"),
    ("bf3", "conv", (5, 32, 40, 1, 5, 3, 2), "res1", "bf3_k3s2_w3x1_nt1_ms2_ne10_tn"),
    ("bf3", "conv", (2, 32, 40, 17, 21, 3, 2), "relu+res1", "bf3_k3s2_w3x1_nt1_ms2_ne6_odd"),
    ("bf3", "conv", (5, 32, 80, 1, 5, 3, 2), "res1+res2", "bf3_k3s2_w4x1_nt1_ms2_ne10_tn"),
    ("bf3", "conv", (2, 32, 80, 9, 37, 3, 2), "relu+res1+res2", "bf3_k3s2_w4x1_nt1_ms2_ne6_odd"),
    ("bf3", "conv", (2, 32, 80, 34, 42, 3, 2), "", "bf3_k3s2_w4x1_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (3, 32, 80, 4, 4, 3, 2), "relu", "bf3_k3s2_w4x1_nt1_ms2_ne6_tn"),
    ("h2", "conv", (2, 32, 16, 5, 41, 1, 1), "res1+mag", "h2_k1s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", "conv", (8, 32, 16, 130, 127, 1, 1), "relu+res1+mag", "h2_k1s1_w2x2_nt1_ms4_ne6_pow2"),
    ("h2", "conv", (2, 32, 48, 3, 5, 1, 1), "res1+res2+up2+mag", "h2_k1s1_w3x1_nt1_ms1_ne6_pow2"),
    ("h2", "conv", (32, 32, 96, 5, 41, 1, 1), "relu+res1+res2+mag", "h2_k1s1_w3x1_nt1_ms2_ne6_pow2"),
    ("h2", "conv", (8, 32, 144, 33, 31, 1, 1), "mag", "h2_k1s1_w3x1_nt1_ms4_ne6_pow2"),
    ("h2", "conv", (2, 48, 64, 3, 5, 1, 1), "relu+up1+mag", "h2_k1s1_w4x1_nt1_ms1_g2_pow2"),
    ("h2", "conv", (2, 32, 80, 3, 5, 1, 1), "res1+up2+mag", "h2_k1s1_w4x1_nt1_ms1_ne6_pow2"),
    ("h2", "conv", (3, 48, 256, 33, 31, 1, 1), "relu+res1+mag", "h2_k1s1_w4x1_nt1_ms2_g2_pow2"),
    ("h2", "conv", (32, 32, 80, 5, 41, 1, 1), "res1+res2+mag", "h2_k1s1_w4x1_nt1_ms2_ne6_pow2"),
    ("h2", "conv", (8, 48, 192, 33, 31, 1, 1), "relu+res1+res2+mag", "h2_k1s1_w4x1_nt1_ms4_g2_pow2"),
    ("h2", "conv", (8, 32, 80, 47, 37, 1, 1), "mag", "h2_k1s1_w4x1_nt1_ms4_ne6_pow2"),
    ("h2", "conv", (32, 48, 256, 33, 31, 1, 1), "relu+mag", "h2_k1s1_w4x1_nt2_ms4_g2_pow2"),
    ("h2", "deconv", (2, 32, 16, 5, 41, 4, 2), "res1+mag", "h2_k2s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", "deconv", (8, 32, 16, 130, 127, 4, 2), "relu+res1+mag", "h2_k2s1_w2x2_nt1_ms4_ne6_pow2"),
    ("h2", "deconv", (2, 32, 40, 3, 5, 4, 2), "res1+res2+mag", "h2_k2s1_w3x1_nt1_ms1_ne6_pow2"),
    ("h2", "deconv", (3, 32, 40, 33, 31, 4, 2), "relu+res1+res2+mag", "h2_k2s1_w3x1_nt1_ms2_ne6_pow2"),
    ("h2", "deconv", (32, 32, 40, 5, 41, 4, 2), "mag", "h2_k2s1_w3x1_nt1_ms4_ne6_pow2"),
    ("h2", "deconv", (2, 32, 80, 3, 5, 4, 2), "relu+mag", "h2_k2s1_w4x1_nt1_ms1_ne6_pow2"),
    ("h2", "deconv", (8, 32, 80, 5, 41, 4, 2), "res1+mag", "h2_k2s1_w4x1_nt1_ms2_ne6_pow2"),
    ("h2", "deconv", (3, 32, 80, 33, 31, 4, 2), "relu+res1+mag", "h2_k2s1_w4x1_nt1_ms4_ne6_pow2"),
    ("h2", "conv", (2, 32, 16, 9, 37, 3, 1), "res1+res2+mag", "h2_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", "conv", (2, 32, 16, 5, 41, 3, 1), "relu+res1+res2+mag", "h2_k3s1_w2x2_nt1_ms2_rows_pow2"),
    ("h2", "conv", (8, 32, 16, 129, 129, 3, 1), "mag", "h2_k3s1_w2x2_nt1_ms4_ne6_pow2"),
    ("h2", "conv", (8, 32, 16, 130, 127, 3, 1), "relu+mag", "h2_k3s1_w2x2_nt1_ms4_rows_pow2"),
    ("h2", "conv", (2, 32, 40, 3, 5, 3, 1), "res1+mag", "h2_k3s1_w3x1_nt1_ms1_ne6_pow2"),
    ("h2", "conv", (2, 32, 40, 5, 41, 3, 1), "relu+res1+mag", "h2_k3s1_w3x1_nt1_ms1_rows_pow2"),
    ("h2", "conv", (32, 32, 40, 5, 41, 3, 1), "res1+res2+mag", "h2_k3s1_w3x1_nt1_ms4_ne6_odd"),
    ("h2", "conv", (3, 32, 40, 47, 37, 3, 1), "relu+res1+res2+mag", "h2_k3s1_w3x1_nt1_ms4_ne6_pow2"),
    ("h2", "conv", (5, 32, 40, 33, 31, 3, 1), "mag", "h2_k3s1_w3x1_nt1_ms4_rows_pow2"),
    ("h2", "conv", (2, 32, 80, 3, 5, 3, 1), "relu+mag", "h2_k3s1_w4x1_nt1_ms1_ne6_pow2"),
    ("h2", "conv", (2, 32, 80, 5, 41, 3, 1), "res1+mag", "h2_k3s1_w4x1_nt1_ms1_rows_pow2"),
    ("h2", "conv", (32, 32, 80, 5, 41, 3, 1), "relu+res1+mag", "h2_k3s1_w4x1_nt1_ms4_ne6_odd"),
    ("h2", "conv", (2, 32, 80, 47, 37, 3, 1), "res1+res2+mag", "h2_k3s1_w4x1_nt1_ms4_ne6_pow2"),
    ("h2", "conv", (3, 32, 80, 33, 31, 3, 1), "relu+res1+res2+mag", "h2_k3s1_w4x1_nt1_ms4_rows_pow2"),
    ("h2", "conv", (2, 32, 16, 9, 37, 3, 2), "mag", "h2_k3s2_w2x2_nt1_ms1_ne6_pow2"),
    ("h2", "conv", (2, 32, 40, 9, 37, 3, 2), "relu+mag", "h2_k3s2_w3x1_nt1_ms2_ne10_odd"),
    ("h2", "conv", (2, 32, 40, 34, 42, 3, 2), "res1+mag", "h2_k3s2_w3x1_nt1_ms2_ne10_pow2"),
    ("h2", "conv", (2, 32, 40, 17, 21, 3, 2), "relu+res1+mag", "h2_k3s2_w3x1_nt1_ms2_ne6_odd"),
    ("h2", "conv", (2, 32, 80, 9, 37, 3, 2), "res1+res2+mag", "h2_k3s2_w4x1_nt1_ms2_ne6_odd"),
    ("h2", "conv", (2, 32, 80, 34, 42, 3, 2), "relu+res1+res2+mag", "h2_k3s2_w4x1_nt1_ms2_ne6_pow2"),
]
FWD_EXTRA = [
    ("bf3", "conv", (2, 32, 19, 20, 24, 3, 1), "relu+res1", "bf3_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (2, 32, 20, 20, 24, 3, 1), "res1+res2", "bf3_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (2, 32, 19, 20, 24, 3, 1), "relu+nchw", "bf3_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", "conv", (2, 32, 19, 9, 7, 3, 2), "nchw", "bf3_k3s2_w2x2_nt1_ms1_ne6_pow2"),
    ("bf3", "conv", (8, 48, 64, 33, 31, 3, 1), "relu", "bf3_k3s1_w4x1_nt1_ms4_rows_pow2"),
    ("bf3", "conv", (8, 48, 64, 47, 37, 1, 1), "res1+up1", "bf3_k1s1_w4x1_nt1_ms2_g2_pow2"),
    ("bf3", "conv", (2, 64, 128, 17, 24, 1, 2), "relu+res1", "bf3_k1s1_w4x1_nt1_ms1_g2_pow2"),
    ("bf3", "conv", (3, 256, 512, 9, 7, 1, 2), "up1", "bf3_k1s1_w4x1_nt1_ms1_g2_pow2"),
    ("h2", "conv", (2, 32, 19, 20, 24, 3, 1), "relu+res1+mag", "h2_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", "conv", (2, 32, 20, 20, 24, 3, 1), "res1+res2+mag", "h2_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", "conv", (2, 32, 19, 20, 24, 3, 1), "relu+nchw+mag", "h2_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", "conv", (2, 32, 19, 9, 7, 3, 2), "nchw+mag", "h2_k3s2_w2x2_nt1_ms1_ne6_pow2"),
    ("h2", "conv", (8, 48, 64, 33, 31, 3, 1), "relu+mag", "h2_k3s1_w4x1_nt1_ms4_rows_pow2"),
    ("h2", "conv", (8, 48, 64, 47, 37, 1, 1), "res1+up1+mag", "h2_k1s1_w4x1_nt1_ms2_g2_pow2"),
    ("h2", "conv", (2, 64, 128, 17, 24, 1, 2), "relu+res1+mag", "h2_k1s1_w4x1_nt1_ms1_g2_pow2"),
    ("h2", "conv", (3, 256, 512, 9, 7, 1, 2), "up1+mag", "h2_k1s1_w4x1_nt1_ms1_g2_pow2"),
]
DGRAD_CASES = [
    ("bf3", (2, 16, 32, 5, 41, 1, 1), "bf3_k1s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", (3, 16, 32, 3, 5, 1, 1), "bf3_k1s1_w2x2_nt1_ms2_ne6_tn"),
    ("bf3", (8, 16, 32, 130, 127, 1, 1), "bf3_k1s1_w2x2_nt1_ms4_ne6_pow2"),
    ("bf3", (2, 48, 32, 3, 5, 1, 1), "bf3_k1s1_w3x1_nt1_ms1_ne6_pow2"),
    ("bf3", (3, 48, 32, 1, 5, 1, 1), "bf3_k1s1_w3x1_nt1_ms1_ne6_tn"),
    ("bf3", (32, 96, 32, 5, 41, 1, 1), "bf3_k1s1_w3x1_nt1_ms2_ne6_pow2"),
    ("bf3", (8, 144, 32, 33, 31, 1, 1), "bf3_k1s1_w3x1_nt1_ms4_ne6_pow2"),
    ("bf3", (2, 64, 48, 3, 5, 1, 1), "bf3_k1s1_w4x1_nt1_ms1_g2_pow2"),
    ("bf3", (3, 64, 48, 1, 5, 1, 1), "bf3_k1s1_w4x1_nt1_ms1_g2_tn"),
    ("bf3", (2, 80, 32, 3, 5, 1, 1), "bf3_k1s1_w4x1_nt1_ms1_ne6_pow2"),
    ("bf3", (3, 80, 32, 1, 5, 1, 1), "bf3_k1s1_w4x1_nt1_ms1_ne6_tn"),
    ("bf3", (3, 256, 48, 33, 31, 1, 1), "bf3_k1s1_w4x1_nt1_ms2_g2_pow2"),
    ("bf3", (32, 80, 32, 5, 41, 1, 1), "bf3_k1s1_w4x1_nt1_ms2_ne6_pow2"),
    ("bf3", (8, 192, 48, 33, 31, 1, 1), "bf3_k1s1_w4x1_nt1_ms4_g2_pow2"),
    ("bf3", (8, 80, 32, 47, 37, 1, 1), "bf3_k1s1_w4x1_nt1_ms4_ne6_pow2"),
    ("bf3", (32, 256, 48, 33, 31, 1, 1), "bf3_k1s1_w4x1_nt2_ms4_g2_pow2"),
    ("bf3", (5, 16, 32, 1, 13, 3, 1), "bf3_k3s1_w2x2_nt1_ms2_ne10_tn"),
    ("bf3", (5, 16, 32, 1, 13, 3, 2), "bf3_k3s1_w2x2_nt1_ms2_ne10_tn_dil2"),
    ("bf3", (2, 16, 32, 9, 37, 3, 1), "bf3_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", (2, 16, 32, 9, 37, 3, 2), "bf3_k3s1_w2x2_nt1_ms2_ne6_pow2_dil2"),
    ("bf3", (3, 16, 32, 3, 5, 3, 1), "bf3_k3s1_w2x2_nt1_ms2_ne6_tn"),
    ("bf3", (3, 16, 32, 3, 5, 3, 2), "bf3_k3s1_w2x2_nt1_ms2_ne6_tn_dil2"),
    ("bf3", (2, 16, 32, 5, 41, 3, 1), "bf3_k3s1_w2x2_nt1_ms2_rows_pow2"),
    ("bf3", (2, 16, 32, 5, 41, 3, 2), "bf3_k3s1_w2x2_nt1_ms2_rows_pow2_dil2"),
    ("bf3", (8, 16, 32, 129, 129, 3, 1), "bf3_k3s1_w2x2_nt1_ms4_ne6_pow2"),
    ("bf3", (2, 16, 32, 258, 258, 3, 2), "bf3_k3s1_w2x2_nt1_ms4_ne6_pow2_dil2"),
    ("bf3", (8, 16, 32, 130, 127, 3, 1), "bf3_k3s1_w2x2_nt1_ms4_rows_pow2"),
    ("bf3", (8, 16, 32, 130, 127, 3, 2), "bf3_k3s1_w2x2_nt1_ms4_rows_pow2_dil2"),
    ("bf3", (2, 40, 32, 3, 5, 3, 1), "bf3_k3s1_w3x1_nt1_ms1_ne6_pow2"),
    ("bf3", (2, 40, 32, 3, 5, 3, 2), "bf3_k3s1_w3x1_nt1_ms1_ne6_pow2_dil2"),
    ("bf3", (3, 40, 32, 1, 5, 3, 1), "bf3_k3s1_w3x1_nt1_ms1_ne6_tn"),
    ("bf3", (3, 40, 32, 1, 5, 3, 2), "bf3_k3s1_w3x1_nt1_ms1_ne6_tn_dil2"),
    ("bf3", (2, 40, 32, 5, 41, 3, 1), "bf3_k3s1_w3x1_nt1_ms1_rows_pow2"),
    ("bf3", (2, 40, 32, 5, 41, 3, 2), "bf3_k3s1_w3x1_nt1_ms1_rows_pow2_dil2"),
    ("bf3", (32, 40, 32, 5, 41, 3, 1), "bf3_k3s1_w3x1_nt1_ms4_ne6_odd"),
    ("bf3", (32, 40, 32, 5, 41, 3, 2), "bf3_k3s1_w3x1_nt1_ms4_ne6_odd_dil2"),
    ("bf3", (3, 40, 32, 47, 37, 3, 1), "bf3_k3s1_w3x1_nt1_ms4_ne6_pow2"),
    ("bf3", (3, 40, 32, 47, 37, 3, 2), "bf3_k3s1_w3x1_nt1_ms4_ne6_pow2_dil2"),
    ("bf3", (5, 40, 32, 33, 31, 3, 1), "bf3_k3s1_w3x1_nt1_ms4_rows_pow2"),
    ("bf3", (5, 40, 32, 33, 31, 3, 2), "bf3_k3s1_w3x1_nt1_ms4_rows_pow2_dil2"),
    ("bf3", (2, 80, 32, 3, 5, 3, 1), "bf3_k3s1_w4x1_nt1_ms1_ne6_pow2"),
    ("bf3", (2, 80, 32, 3, 5, 3, 2), "bf3_k3s1_w4x1_nt1_ms1_ne6_pow2_dil2"),
    ("bf3", (3, 80, 32, 1, 5, 3, 1), "bf3_k3s1_w4x1_nt1_ms1_ne6_tn"),
    ("bf3", (3, 80, 32, 1, 5, 3, 2), "bf3_k3s1_w4x1_nt1_ms1_ne6_tn_dil2"),
    ("bf3", (2, 80, 32, 5, 41, 3, 1), "bf3_k3s1_w4x1_nt1_ms1_rows_pow2"),
    ("bf3", (2, 80, 32, 5, 41, 3, 2), "bf3_k3s1_w4x1_nt1_ms1_rows_pow2_dil2"),
    ("bf3", (32, 80, 32, 5, 41, 3, 1), "bf3_k3s1_w4x1_nt1_ms4_ne6_odd"),
    ("bf3", (32, 80, 32, 5, 41, 3, 2), "bf3_k3s1_w4x1_nt1_ms4_ne6_odd_dil2"),
    ("bf3", (2, 80, 32, 47, 37, 3, 1), "bf3_k3s1_w4x1_nt1_ms4_ne6_pow2"),
    ("bf3", (2, 80, 32, 47, 37, 3, 2), "bf3_k3s1_w4x1_nt1_ms4_ne6_pow2_dil2"),
    ("bf3", (3, 80, 32, 33, 31, 3, 1), "bf3_k3s1_w4x1_nt1_ms4_rows_pow2"),
    ("bf3", (3, 80, 32, 33, 31, 3, 2), "bf3_k3s1_w4x1_nt1_ms4_rows_pow2_dil2"),
    ("h2", (2, 16, 32, 5, 41, 1, 1), "h2_k1s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", (8, 16, 32, 130, 127, 1, 1), "h2_k1s1_w2x2_nt1_ms4_ne6_pow2"),
    ("h2", (2, 48, 32, 3, 5, 1, 1), "h2_k1s1_w3x1_nt1_ms1_ne6_pow2"),
    ("h2", (32, 96, 32, 5, 41, 1, 1), "h2_k1s1_w3x1_nt1_ms2_ne6_pow2"),
    ("h2", (8, 144, 32, 33, 31, 1, 1), "h2_k1s1_w3x1_nt1_ms4_ne6_pow2"),
    ("h2", (2, 64, 48, 3, 5, 1, 1), "h2_k1s1_w4x1_nt1_ms1_g2_pow2"),
    ("h2", (2, 80, 32, 3, 5, 1, 1), "h2_k1s1_w4x1_nt1_ms1_ne6_pow2"),
    ("h2", (3, 256, 48, 33, 31, 1, 1), "h2_k1s1_w4x1_nt1_ms2_g2_pow2"),
    ("h2", (32, 80, 32, 5, 41, 1, 1), "h2_k1s1_w4x1_nt1_ms2_ne6_pow2"),
    ("h2", (8, 192, 48, 33, 31, 1, 1), "h2_k1s1_w4x1_nt1_ms4_g2_pow2"),
    ("h2", (8, 80, 32, 47, 37, 1, 1), "h2_k1s1_w4x1_nt1_ms4_ne6_pow2"),
    ("h2", (32, 256, 48, 33, 31, 1, 1), "h2_k1s1_w4x1_nt2_ms4_g2_pow2"),
    ("h2", (2, 16, 32, 9, 37, 3, 1), "h2_k3s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", (2, 16, 32, 5, 41, 3, 1), "h2_k3s1_w2x2_nt1_ms2_rows_pow2"),
    ("h2", (8, 16, 32, 129, 129, 3, 1), "h2_k3s1_w2x2_nt1_ms4_ne6_pow2"),
    ("h2", (8, 16, 32, 130, 127, 3, 1), "h2_k3s1_w2x2_nt1_ms4_rows_pow2"),
    ("h2", (2, 40, 32, 3, 5, 3, 1), "h2_k3s1_w3x1_nt1_ms1_ne6_pow2"),
    ("h2", (2, 40, 32, 5, 41, 3, 1), "h2_k3s1_w3x1_nt1_ms1_rows_pow2"),
    ("h2", (32, 40, 32, 5, 41, 3, 1), "h2_k3s1_w3x1_nt1_ms4_ne6_odd"),
    ("h2", (3, 40, 32, 47, 37, 3, 1), "h2_k3s1_w3x1_nt1_ms4_ne6_pow2"),
    ("h2", (5, 40, 32, 33, 31, 3, 1), "h2_k3s1_w3x1_nt1_ms4_rows_pow2"),
    ("h2", (2, 80, 32, 3, 5, 3, 1), "h2_k3s1_w4x1_nt1_ms1_ne6_pow2"),
    ("h2", (2, 80, 32, 5, 41, 3, 1), "h2_k3s1_w4x1_nt1_ms1_rows_pow2"),
    ("h2", (32, 80, 32, 5, 41, 3, 1), "h2_k3s1_w4x1_nt1_ms4_ne6_odd"),
    ("h2", (2, 80, 32, 47, 37, 3, 1), "h2_k3s1_w4x1_nt1_ms4_ne6_pow2"),
    ("h2", (3, 80, 32, 33, 31, 3, 1), "h2_k3s1_w4x1_nt1_ms4_rows_pow2"),
]
PARITY_CASES = [
    ("bf3", (2, 20, 32, 34, 42, 3, 2), "bf3_k2s1_w2x2_nt1_ms2_ne6_pow2"),
    ("bf3", (3, 20, 32, 6, 10, 3, 2), "bf3_k2s1_w2x2_nt1_ms2_ne6_tn"),
    ("bf3", (8, 20, 32, 258, 258, 3, 2), "bf3_k2s1_w2x2_nt1_ms4_ne6_pow2"),
    ("bf3", (2, 40, 32, 6, 10, 3, 2), "bf3_k2s1_w3x1_nt1_ms1_ne6_pow2"),
    ("bf3", (3, 40, 32, 66, 74, 3, 2), "bf3_k2s1_w3x1_nt1_ms2_ne6_pow2"),
    ("bf3", (5, 40, 32, 66, 74, 3, 2), "bf3_k2s1_w3x1_nt1_ms4_ne6_pow2"),
    ("bf3", (2, 80, 32, 6, 10, 3, 2), "bf3_k2s1_w4x1_nt1_ms1_ne6_pow2"),
    ("bf3", (5, 80, 32, 34, 42, 3, 2), "bf3_k2s1_w4x1_nt1_ms2_ne6_pow2"),
    ("bf3", (3, 80, 32, 66, 74, 3, 2), "bf3_k2s1_w4x1_nt1_ms4_ne6_pow2"),
    ("h2", (2, 20, 32, 34, 42, 3, 2), "h2_k2s1_w2x2_nt1_ms2_ne6_pow2"),
    ("h2", (8, 20, 32, 258, 258, 3, 2), "h2_k2s1_w2x2_nt1_ms4_ne6_pow2"),
    ("h2", (2, 40, 32, 6, 10, 3, 2), "h2_k2s1_w3x1_nt1_ms1_ne6_pow2"),
    ("h2", (3, 40, 32, 66, 74, 3, 2), "h2_k2s1_w3x1_nt1_ms2_ne6_pow2"),
    ("h2", (5, 40, 32, 66, 74, 3, 2), "h2_k2s1_w3x1_nt1_ms4_ne6_pow2"),
    ("h2", (2, 80, 32, 6, 10, 3, 2), "h2_k2s1_w4x1_nt1_ms1_ne6_pow2"),
    ("h2", (5, 80, 32, 34, 42, 3, 2), "h2_k2s1_w4x1_nt1_ms2_ne6_pow2"),
    ("h2", (3, 80, 32, 66, 74, 3, 2), "h2_k2s1_w4x1_nt1_ms4_ne6_pow2"),
]
TRAIN_CASES = [
    ("bf3", "single", (32, 16, 1, 1), 2, (5, 41), "c", "bf3_k1s1_w2x2_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "single", (32, 16, 1, 2), 3, (5, 41), "c", "bf3_k1s1_w2x2_nt1_ms2_ne6_tn_precise"),
    ("bf3", "single", (32, 16, 1, 1), 8, (130, 127), "c", "bf3_k1s1_w2x2_nt1_ms4_ne6_pow2_precise"),
    ("bf3", "single", (32, 48, 1, 1), 2, (3, 5), "c", "bf3_k1s1_w3x1_nt1_ms1_ne6_pow2_precise"),
    ("bf3", "single", (32, 48, 1, 2), 3, (1, 5), "c", "bf3_k1s1_w3x1_nt1_ms1_ne6_tn_precise"),
    ("bf3", "single", (32, 96, 1, 1), 32, (5, 41), "c", "bf3_k1s1_w3x1_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "single", (32, 144, 1, 1), 8, (33, 31), "c", "bf3_k1s1_w3x1_nt1_ms4_ne6_pow2_precise"),
    ("bf3", "single", (48, 64, 1, 1), 2, (3, 5), "c", "bf3_k1s1_w4x1_nt1_ms1_g2_pow2_precise"),
    ("bf3", "single", (48, 64, 1, 2), 3, (1, 5), "c", "bf3_k1s1_w4x1_nt1_ms1_g2_tn_precise"),
    ("bf3", "single", (32, 80, 1, 1), 2, (3, 5), "c", "bf3_k1s1_w4x1_nt1_ms1_ne6_pow2_precise"),
    ("bf3", "single", (32, 80, 1, 2), 3, (1, 5), "c", "bf3_k1s1_w4x1_nt1_ms1_ne6_tn_precise"),
    ("bf3", "single", (48, 256, 1, 1), 3, (33, 31), "c", "bf3_k1s1_w4x1_nt1_ms2_g2_pow2_precise"),
    ("bf3", "single", (32, 80, 1, 1), 32, (5, 41), "c", "bf3_k1s1_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "single", (48, 192, 1, 1), 8, (33, 31), "c", "bf3_k1s1_w4x1_nt1_ms4_g2_pow2_precise"),
    ("bf3", "single", (32, 80, 1, 1), 8, (47, 37), "c", "bf3_k1s1_w4x1_nt1_ms4_ne6_pow2_precise"),
    ("bf3", "single", (48, 256, 1, 1), 32, (33, 31), "c", "bf3_k1s1_w4x1_nt2_ms4_g2_pow2_precise"),
    ("bf3", "single", (32, 16, 3, 1), 5, (1, 13), "c", "bf3_k3s1_w2x2_nt1_ms2_ne10_tn_precise"),
    ("bf3", "single", (32, 16, 3, 1), 2, (9, 37), "c", "bf3_k3s1_w2x2_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "single", (32, 16, 3, 1), 3, (3, 5), "c", "bf3_k3s1_w2x2_nt1_ms2_ne6_tn_precise"),
    ("bf3", "single", (32, 16, 3, 1), 2, (5, 41), "c", "bf3_k3s1_w2x2_nt1_ms2_rows_pow2_precise"),
    ("bf3", "single", (32, 16, 3, 1), 8, (129, 129), "c", "bf3_k3s1_w2x2_nt1_ms4_ne6_pow2_precise"),
    ("bf3", "single", (32, 16, 3, 1), 8, (130, 127), "c", "bf3_k3s1_w2x2_nt1_ms4_rows_pow2_precise"),
    ("bf3", "single", (32, 40, 3, 1), 2, (3, 5), "c", "bf3_k3s1_w3x1_nt1_ms1_ne6_pow2_precise"),
    ("bf3", "single", (32, 40, 3, 1), 3, (1, 5), "c", "bf3_k3s1_w3x1_nt1_ms1_ne6_tn_precise"),
    ("bf3", "single", (32, 40, 3, 1), 2, (5, 41), "c", "bf3_k3s1_w3x1_nt1_ms1_rows_pow2_precise"),
    ("bf3", "single", (32, 40, 3, 1), 32, (5, 41), "c", "bf3_k3s1_w3x1_nt1_ms4_ne6_odd_precise"),
    ("bf3", "single", (32, 40, 3, 1), 3, (47, 37), "c", "bf3_k3s1_w3x1_nt1_ms4_ne6_pow2_precise"),
    ("bf3", "single", (32, 40, 3, 1), 5, (33, 31), "c", "bf3_k3s1_w3x1_nt1_ms4_rows_pow2_precise"),
    ("bf3", "single", (32, 80, 3, 1), 2, (3, 5), "c", "bf3_k3s1_w4x1_nt1_ms1_ne6_pow2_precise"),
    ("bf3", "single", (32, 80, 3, 1), 3, (1, 5), "c", "bf3_k3s1_w4x1_nt1_ms1_ne6_tn_precise"),
    ("bf3", "single", (32, 80, 3, 1), 2, (5, 41), "c", "bf3_k3s1_w4x1_nt1_ms1_rows_pow2_precise"),
    ("bf3", "single", (32, 80, 3, 1), 32, (5, 41), "c", "bf3_k3s1_w4x1_nt1_ms4_ne6_odd_precise"),
    ("bf3", "single", (32, 80, 3, 1), 2, (47, 37), "c", "bf3_k3s1_w4x1_nt1_ms4_ne6_pow2_precise"),
    ("bf3", "single", (32, 80, 3, 1), 3, (33, 31), "c", "bf3_k3s1_w4x1_nt1_ms4_rows_pow2_precise"),
    ("bf3", "single", (32, 16, 3, 2), 5, (1, 5), "c", "bf3_k3s2_w2x2_nt1_ms1_ne10_tn_precise"),
    ("bf3", "single", (32, 16, 3, 2), 2, (9, 37), "c", "bf3_k3s2_w2x2_nt1_ms1_ne6_pow2_precise"),
    ("bf3", "single", (32, 16, 3, 2), 3, (4, 4), "c", "bf3_k3s2_w2x2_nt1_ms1_ne6_tn_precise"),
    ("bf3", "single", (32, 40, 3, 2), 2, (9, 37), "c", "bf3_k3s2_w3x1_nt1_ms2_ne10_odd_precise"),
    ("bf3", "single", (32, 40, 3, 2), 2, (34, 42), "c", "bf3_k3s2_w3x1_nt1_ms2_ne10_pow2_precise"),
    ("bf3", "single", (32, 40, 3, 2), 5, (1, 5), "c", "bf3_k3s2_w3x1_nt1_ms2_ne10_tn_precise"),
    ("bf3", "single", (32, 40, 3, 2), 2, (17, 21), "c", "bf3_k3s2_w3x1_nt1_ms2_ne6_odd_precise"),
    ("bf3", "single", (32, 80, 3, 2), 5, (1, 5), "c", "bf3_k3s2_w4x1_nt1_ms2_ne10_tn_precise"),
    ("bf3", "single", (32, 80, 3, 2), 2, (9, 37), "c", "bf3_k3s2_w4x1_nt1_ms2_ne6_odd_precise"),
    ("bf3", "single", (32, 80, 3, 2), 2, (34, 42), "c", "bf3_k3s2_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "single", (32, 80, 3, 2), 3, (4, 4), "c", "bf3_k3s2_w4x1_nt1_ms2_ne6_tn_precise"),
    ("h2", "single", (32, 16, 1, 1), 2, (5, 41), "c", "h2_k1s1_w2x2_nt1_ms2_ne6_pow2_precise"),
    ("h2", "single", (32, 16, 1, 1), 8, (130, 127), "c", "h2_k1s1_w2x2_nt1_ms4_ne6_pow2_precise"),
    ("h2", "single", (32, 48, 1, 1), 2, (3, 5), "c", "h2_k1s1_w3x1_nt1_ms1_ne6_pow2_precise"),
    ("h2", "single", (32, 96, 1, 1), 32, (5, 41), "c", "h2_k1s1_w3x1_nt1_ms2_ne6_pow2_precise"),
    ("h2", "single", (32, 144, 1, 1), 8, (33, 31), "c", "h2_k1s1_w3x1_nt1_ms4_ne6_pow2_precise"),
    ("h2", "single", (48, 64, 1, 1), 2, (3, 5), "c", "h2_k1s1_w4x1_nt1_ms1_g2_pow2_precise"),
    ("h2", "single", (32, 80, 1, 1), 2, (3, 5), "c", "h2_k1s1_w4x1_nt1_ms1_ne6_pow2_precise"),
    ("h2", "single", (48, 256, 1, 1), 3, (33, 31), "c", "h2_k1s1_w4x1_nt1_ms2_g2_pow2_precise"),
    ("h2", "single", (32, 80, 1, 1), 32, (5, 41), "c", "h2_k1s1_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("h2", "single", (48, 192, 1, 1), 8, (33, 31), "c", "h2_k1s1_w4x1_nt1_ms4_g2_pow2_precise"),
    ("h2", "single", (32, 80, 1, 1), 8, (47, 37), "c", "h2_k1s1_w4x1_nt1_ms4_ne6_pow2_precise"),
    ("h2", "single", (48, 256, 1, 1), 32, (33, 31), "c", "h2_k1s1_w4x1_nt2_ms4_g2_pow2_precise"),
    ("h2", "single", (32, 16, 3, 1), 2, (9, 37), "c", "h2_k3s1_w2x2_nt1_ms2_ne6_pow2_precise"),
    ("h2", "single", (32, 16, 3, 1), 2, (5, 41), "c", "h2_k3s1_w2x2_nt1_ms2_rows_pow2_precise"),
    ("h2", "single", (32, 16, 3, 1), 8, (129, 129), "c", "h2_k3s1_w2x2_nt1_ms4_ne6_pow2_precise"),
    ("h2", "single", (32, 16, 3, 1), 8, (130, 127), "c", "h2_k3s1_w2x2_nt1_ms4_rows_pow2_precise"),
    ("h2", "single", (32, 40, 3, 1), 2, (3, 5), "c", "h2_k3s1_w3x1_nt1_ms1_ne6_pow2_precise"),
    ("h2", "single", (32, 40, 3, 1), 2, (5, 41), "c", "h2_k3s1_w3x1_nt1_ms1_rows_pow2_precise"),
    ("h2", "single", (32, 40, 3, 1), 32, (5, 41), "c", "h2_k3s1_w3x1_nt1_ms4_ne6_odd_precise"),
    ("h2", "single", (32, 40, 3, 1), 3, (47, 37), "c", "h2_k3s1_w3x1_nt1_ms4_ne6_pow2_precise"),
    ("h2", "single", (32, 40, 3, 1), 5, (33, 31), "c", "h2_k3s1_w3x1_nt1_ms4_rows_pow2_precise"),
    ("h2", "single", (32, 80, 3, 1), 2, (3, 5), "c", "h2_k3s1_w4x1_nt1_ms1_ne6_pow2_precise"),
    ("h2", "single", (32, 80, 3, 1), 2, (5, 41), "c", "h2_k3s1_w4x1_nt1_ms1_rows_pow2_precise"),
    ("h2", "single", (32, 80, 3, 1), 32, (5, 41), "c", "h2_k3s1_w4x1_nt1_ms4_ne6_odd_precise"),
    ("h2", "single", (32, 80, 3, 1), 2, (47, 37), "c", "h2_k3s1_w4x1_nt1_ms4_ne6_pow2_precise"),
    ("h2", "single", (32, 80, 3, 1), 3, (33, 31), "c", "h2_k3s1_w4x1_nt1_ms4_rows_pow2_precise"),
    ("h2", "single", (32, 16, 3, 2), 2, (9, 37), "c", "h2_k3s2_w2x2_nt1_ms1_ne6_pow2_precise"),
    ("h2", "single", (32, 40, 3, 2), 2, (9, 37), "c", "h2_k3s2_w3x1_nt1_ms2_ne10_odd_precise"),
    ("h2", "single", (32, 40, 3, 2), 2, (34, 42), "c", "h2_k3s2_w3x1_nt1_ms2_ne10_pow2_precise"),
    ("h2", "single", (32, 40, 3, 2), 2, (17, 21), "c", "h2_k3s2_w3x1_nt1_ms2_ne6_odd_precise"),
    ("h2", "single", (32, 80, 3, 2), 2, (9, 37), "c", "h2_k3s2_w4x1_nt1_ms2_ne6_odd_precise"),
    ("h2", "single", (32, 80, 3, 2), 2, (34, 42), "c", "h2_k3s2_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "blocks", (64,), 3, (33, 31), "b0.conv1", "bf3_k3s1_w4x1_nt1_ms1_rows_pow2_precise"),
    ("h2", "blocks", (64,), 3, (33, 31), "b0.conv1", "h2_k3s1_w4x1_nt1_ms1_rows_pow2_precise"),
    ("bf3", "bneck", (64, 64, 1), 3, (33, 31), "bn0.conv1", "bf3_k1s1_w4x1_nt1_ms1_g2_pow2_precise"),
    ("bf3", "bneck", (64, 64, 1), 3, (33, 31), "bn0.conv3", "bf3_k1s1_w4x1_nt1_ms2_g2_pow2_precise"),
    ("h2", "bneck", (64, 64, 1), 3, (33, 31), "bn0.conv1", "h2_k1s1_w4x1_nt1_ms1_g2_pow2_precise"),
    ("h2", "bneck", (64, 64, 1), 3, (33, 31), "bn0.conv3", "h2_k1s1_w4x1_nt1_ms2_g2_pow2_precise"),
    ("bf3", "bneck", (64, 64, 2), 3, (33, 31), "bn0.conv2", "bf3_k3s2_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "bneck", (64, 64, 2), 3, (33, 31), "bn0.downsample.0", "bf3_k1s1_w4x1_nt1_ms1_g2_pow2_precise"),
    ("h2", "bneck", (64, 64, 2), 3, (33, 31), "bn0.conv2", "h2_k3s2_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("h2", "bneck", (64, 64, 2), 3, (33, 31), "bn0.downsample.0", "h2_k1s1_w4x1_nt1_ms1_g2_pow2_precise"),
    ("bf3", "fuse", (48, 96, 64), 8, (32, 24), "t1", "bf3_k3s2_w3x1_nt1_ms2_ne10_pow2_precise"),
    ("bf3", "fuse", (48, 96, 64), 8, (32, 24), "t2", "bf3_k3s2_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("bf3", "fuse", (48, 96, 64), 8, (32, 24), "f02", "bf3_k1s1_w3x1_nt1_ms1_ne6_pow2_precise"),
    ("h2", "fuse", (48, 96, 64), 8, (32, 24), "t1", "h2_k3s2_w3x1_nt1_ms2_ne10_pow2_precise"),
    ("h2", "fuse", (48, 96, 64), 8, (32, 24), "t2", "h2_k3s2_w4x1_nt1_ms2_ne6_pow2_precise"),
    ("h2", "fuse", (48, 96, 64), 8, (32, 24), "f02", "h2_k1s1_w3x1_nt1_ms1_ne6_pow2_precise"),
    ("bf3", "deconv", (64, 96, 48), 2, (24, 18), "c1", "bf3_k3s1_w3x1_nt1_ms1_rows_pow2_precise"),
    ("h2", "deconv", (64, 96, 48), 2, (24, 18), "c1", "h2_k3s1_w3x1_nt1_ms1_rows_pow2_precise"),
]
# no form needs an exemption: the largest row (8 images of 130 x 127, 32 channels) has 17 MB tensors
EXEMPT = {use: {} for use in sf.USES}  # use -> {form: (shape, why its smallest reaching shape is too large)}
PLANS = {"h2": {"MVAL_TRAIN_P2": "0"}, "bf3": {"MVAL_CONV": "bf3"}}


def _opts(text):
    t = set(text.split("+")) - {""}
    up = [int(x[2:]) for x in t if x.startswith("up")]
    assert t <= {"relu", "res1", "res2", "nchw", "mag", "up1", "up2", "up3"}, text
    return dict(relu="relu" in t, res1="res1" in t, res2="res2" in t, nchw="nchw" in t, up=up[0] if up else 0), "mag" in t


def _fwd_id(row):
    split, kind, (n, cin, cout, h, w, k, s), opts, form = row
    return f"{form}-{kind}_n{n}_c{cin}-{cout}_{h}x{w}" + ("-" + opts if opts else "")


def _shape_id(row):
    split, (n, cin, cout, h, w, k, s), form = row
    return f"{form}-n{n}_c{cin}-{cout}_{h}x{w}"


def _fwd_form(row, n=None):
    split, kind, shape, opts, _ = row
    o, _ = _opts(opts)
    return sf.query("fwd", split, n or shape[0], *shape[1:], kind, **o)


def _train_runs():
    """The training graphs to run: {(split, graph, args, n, hw): [(conv, form), ...]}."""
    runs = {}
    for split, graph, args, n, hw, conv, form in TRAIN_CASES:
        runs.setdefault((split, graph, args, n, hw), []).append((conv, form))
    return runs


def _train_id(key):
    split, graph, args, n, hw = key
    return f"{split}-{graph}_{'_'.join(str(a) for a in args)}-n{n}_{hw[0]}x{hw[1]}"


def _train_forms(plan, split, n):
    """{conv name: (form name, SplitForm)} of the BatchNorm'd convs of a training plan that run on the split kernels, from the plan's own ops."""
    out = {}
    for i, (op, t) in enumerate(zip(plan.graph.ops, plan.ops)):
        if op.kind == "conv" and op.bn and t.op.algo in (sf.ALGO_MFMA_BF3, sf.ALGO_MFMA_H2):
            hin, win = plan.geo[i][:2]
            f = sf.query("train", "h2" if t.op.algo == sf.ALGO_MFMA_H2 else "bf3", n, op.cin, op.cout, hin, win, op.k, op.stride)
            assert f is not None, (op.conv, "the plan runs a conv on a split algo the launcher has no kernel for")
            out[op.conv] = (sf.name(f), f, t.op.algo)
    return out


def _host_plan(key):
    from multi_view_active_learning_amd import engine_train as et

    split, graph, args, n, hw = key
    model = tg.TinyNet(tg.BUILDERS[graph], args, 1).train()
    return et.TrainPlan(model, n, 2 * hw[0], 2 * hw[1], torch.device("cpu"), sw=dict(et._SWITCHES, **PLANS[split]))


# ---- host tests (no GPU) ----
def test_split_form_mirror_matches_the_header():
    """_lib.SplitForm and the SPLIT_* constants restate struct mval_split_form and two enums of include/mval_hip.h."""
    from multi_view_active_learning_amd import _lib

    text = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    body = re.search(r"typedef struct mval_split_form \{(.*?)\} mval_split_form;", text, flags=re.S).group(1)
    fields = [name for line in body.split(";") if line.strip() for name in re.sub(r"^\s*int32_t", "", line).replace(" ", "").split(",")]
    assert fields == [name for name, _ in _lib.SplitForm._fields_] and C.sizeof(_lib.SplitForm) == 4 * len(fields)
    enum = lambda name: int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))
    assert [enum("MVAL_SPLIT_" + n) for n in ("NE6", "NE10", "ROW_SHARING", "TWO_CHUNK")] == [_lib.SPLIT_NE6, _lib.SPLIT_NE10, _lib.SPLIT_ROW_SHARING, _lib.SPLIT_TWO_CHUNK]
    assert [enum("MVAL_SPLIT_USE_" + n) for n in ("OP", "TRAIN_FWD", "DGRAD", "DGRAD_PARITY")] == list(range(4)) == [sf.USES.index(u) for u in sf.USES]
    assert sorted(sf.VARIANT) == [_lib.SPLIT_NE6, _lib.SPLIT_NE10, _lib.SPLIT_ROW_SHARING, _lib.SPLIT_TWO_CHUNK]


def test_the_query_answers_like_the_support_predicates():
    """mval_conv_split_form returns "unsupported" where the launcher returns 1 (and where the entry itself refuses): channel counts the kernels
    do not cover, a 1x1 with NCHW output, the fp16 split on maps under 8 rows that would share a tile, the fp16 zero-dilated data gradient,
    a transposed conv in the training forward (it runs on the exact-fp32 kernels), the parity form on odd sizes; and it needs no GPU."""
    assert sf.query("fwd", "bf3", 2, 40, 64, 16, 16, 3, 1) is None and sf.query("fwd", "bf3", 2, 48, 64, 16, 16, 3, 1) is not None
    assert sf.query("fwd", "bf3", 2, 32, 19, 16, 16, 1, 1) is None and sf.query("fwd", "bf3", 2, 32, 16, 16, 16, 1, 1, nchw=True) is None
    assert sf.query("fwd", "bf3", 2, 32, 19, 16, 16, 3, 1, nchw=True) is not None
    assert sf.query("fwd", "h2", 2, 32, 16, 3, 5, 3, 1) is None and sf.query("fwd", "bf3", 2, 32, 16, 3, 5, 3, 1).tn == 2
    assert sf.query("dgrad", "h2", 2, 32, 32, 16, 16, 3, 2) is None and sf.name(sf.query("dgrad", "bf3", 2, 32, 32, 16, 16, 3, 2), 2).endswith("_dil2")
    assert sf.query("train", "bf3", 2, 32, 32, 8, 8, 4, 2, "deconv") is None and sf.query("fwd", "bf3", 2, 32, 32, 8, 8, 4, 2, "deconv").grid_z == 4
    assert sf.query("parity", "bf3", 2, 32, 32, 17, 16, 3, 2) is None and sf.query("parity", "bf3", 2, 32, 32, 16, 16, 3, 2).grid_z == 4
    assert sf.query("parity", "bf3", 2, 18, 32, 16, 16, 3, 2) is None and sf.query("parity", "bf3", 2, 20, 32, 16, 16, 3, 2) is not None
    f = sf.query("train", "h2", 3, 64, 256, 33, 31, 1, 1)  # (what the struct holds, on one launch)
    assert f.as_dict() == dict(pl=2, ks=1, s=1, wn=4, wm=1, nt=1, ms=2, g=2, variant=3, th=2, tw=16, tn=1, odd=0, precise=1, grid_x=3 * 17 * 2, grid_y=4,
                               grid_z=1, bn_part_ok=1, bn_part=1)


def test_every_row_takes_the_form_it_is_in_the_table_for():
    bad = []
    for row in FWD_CASES + FWD_EXTRA:
        f = _fwd_form(row)
        if f is None or sf.name(f) != row[4]:
            bad.append((_fwd_id(row), f and sf.name(f)))
    for use, table in (("dgrad", DGRAD_CASES), ("parity", PARITY_CASES)):
        for split, shape, form in table:
            for acc in (False, True):
                f = sf.query(use, split, *shape, res1=acc)
                if f is None or sf.name(f, shape[6] if use == "dgrad" else 1) != form:
                    bad.append((use, split, shape, f and sf.name(f)))
    for key, rows in _train_runs().items():
        plan = _host_plan(key)
        forms = _train_forms(plan, key[0], key[3])
        for conv, (_, f, _) in forms.items():  # the plan's workspace has room for the partials of every conv whose form keeps them
            cout = next(op.cout for op in plan.graph.ops if op.conv == conv)
            if f.bn_part and not cout * f.grid_x * 2 <= plan.ws_lane:
                bad.append((_train_id(key), conv, "partials do not fit", cout * f.grid_x * 2, plan.ws_lane))
        for conv, form in rows:
            if conv not in forms or forms[conv][0] != form or forms[conv][2] != sf.ALGO_OF[key[0]]:
                bad.append((_train_id(key), conv, forms.get(conv)))
    assert not bad, bad
    ids = [_fwd_id(r) for r in FWD_CASES + FWD_EXTRA]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("use", sf.USES)
def test_the_tables_name_every_form_the_sweep_finds(use):
    """Coverage and drift: the sweep's forms for this use (tests/split_forms.py: the documented domain, one pass of host arithmetic) are
    exactly the forms the use's table names (+ the exemptions, none at present).  A threshold change that creates a form without a row, or
    takes the last shape away from a row's form, fails here.  Found on this dispatch: 96 forms for the forward (56 bf16x3 + 40 fp16x2), 77
    for the training forward, 78 for the data gradient, 17 for the parity form."""
    found = sf.sweep(use)
    table = {"fwd": [r[4] for r in FWD_CASES], "train": [r[6] for r in TRAIN_CASES], "dgrad": [r[2] for r in DGRAD_CASES],
             "parity": [r[2] for r in PARITY_CASES]}[use]
    print(f"[split forms] {use}: {len(found)} forms ({sum(k.startswith('bf3') for k in found)} bf16x3 + {sum(k.startswith('h2') for k in found)} fp16x2)")
    assert len(found) >= 15
    missing = set(found) - set(table) - set(EXEMPT[use])
    assert not missing, f"forms without a row: {sorted(missing)}"
    stale = set(table) - set(found)
    assert not stale, f"rows whose form the sweep no longer finds: {sorted(stale)}"
    assert not set(EXEMPT[use]) & set(table)
    if use == "fwd":
        assert {r[4] for r in FWD_EXTRA} <= set(found)


@pytest.mark.parametrize("use", sf.USES)
def test_dispatch_facts_over_the_sweep(use):
    """What the launcher promises, stated from the query on every launch of the sweep: several images per tile never with the fp16 split
    (it scales per image; the launcher refuses), an odd tile never with several images per tile or the two-chunk stage, row sharing only for
    3x3 stride 1 on 16-wide one-image tiles, 10 staging slots only on 64-pixel or stride-2 tiles; `precise` exactly in the training
    forward; the parity grid exactly for the 2x2 kernel; the partials possible exactly under the rule of split_forms.partials_rule, and
    kept exactly where they are possible and asked for (the training forward)."""
    bad = []
    for form, cases in sf.sweep(use).items():
        for split, kind, shape, tile in cases:
            f = sf.query(use, split, *shape, kind)
            assert tile == (f.th, f.tw, f.tn)
            n, cin, cout = shape[:3]
            co = cin if use in ("dgrad", "parity") else cout
            ho, wo = sf.grid_hw(use, kind, shape)
            ok = ((f.pl == 2) == (split == "h2") and not (f.pl == 2 and f.tn > 1) and not (f.odd and (f.tn > 1 or f.g > 1)) and
                  (f.variant == 3) == (f.g == 2) and (f.g == 1 or f.ks == 1) and
                  (f.variant != 2 or (f.ks == 3 and f.s == 1 and f.tw == 16 and f.tn == 1)) and
                  (f.variant != 1 or 16 * f.ms * f.wm >= 64 or f.s == 2) and
                  f.precise == (use == "train") and (f.grid_z == 4) == (f.ks == 2) and f.th * f.tw * f.tn <= 16 * f.ms * f.wm and
                  (f.odd or f.th * f.tw * f.tn == 16 * f.ms * f.wm) and
                  f.grid_x == -(-ho // f.th) * -(-wo // f.tw) * -(-n // f.tn) and f.grid_y == -(-(-(-co // 16)) // (f.wn * f.nt)) and
                  bool(f.bn_part_ok) == sf.partials_rule(f, cout=co) and f.bn_part == (f.bn_part_ok if use == "train" else 0))
            if not ok:
                bad.append((form, split, kind, shape, f.as_dict()))
    assert not bad, bad[:5]


def test_partials_rule_with_the_epilogue_options():
    """The partials under the forward rows' epilogue options (residuals, ReLU, up-sampling, NCHW output, the parity grid): possible exactly
    when split_forms.partials_rule says so, and mval_op_launch never asks for them."""
    seen = set()
    for row in FWD_CASES + FWD_EXTRA:
        o, _ = _opts(row[3])
        for opts in (o, dict(relu=False, res1=False, res2=False, nchw=False, up=0)):
            f = sf.query("fwd", row[0], *row[2], row[1], **opts)
            assert bool(f.bn_part_ok) == sf.partials_rule(f, cout=row[2][2], **opts) and not f.bn_part, (_fwd_id(row), opts)
            seen.add((bool(f.bn_part_ok), any(opts.values()), f.grid_z))
    assert {(True, False, 1), (False, False, 1), (False, True, 1), (False, False, 4)} <= seen
    # accumulate is a residual: no data gradient could keep them
    assert not any(sf.query("dgrad", s, *shape, res1=True).bn_part_ok for s, shape, _ in DGRAD_CASES)


# forms that no shape of the sweep reaches with a partly filled last tile in BOTH directions (every other form's row must have both), per use: their
# tiles have ONE row (the 16-pixel row-sharing tiles, 1 x 16) or hold several images of a map of one or two rows, all of its rows in the tile -- only
# their columns can be ragged
NOT_RAGGED = {
    "fwd": {"bf3_k1s1_w3x1_nt1_ms1_ne6_tn", "bf3_k1s1_w4x1_nt1_ms1_g2_tn", "bf3_k1s1_w4x1_nt1_ms1_ne6_tn", "bf3_k2s1_w3x1_nt1_ms1_ne6_tn",
            "bf3_k2s1_w4x1_nt1_ms1_ne6_tn", "bf3_k3s1_w2x2_nt1_ms2_ne10_tn", "bf3_k3s1_w3x1_nt1_ms1_ne6_tn", "bf3_k3s1_w3x1_nt1_ms1_rows_pow2",
            "bf3_k3s1_w4x1_nt1_ms1_ne6_tn", "bf3_k3s1_w4x1_nt1_ms1_rows_pow2", "bf3_k3s2_w2x2_nt1_ms1_ne10_tn", "bf3_k3s2_w2x2_nt1_ms1_ne6_tn",
            "bf3_k3s2_w3x1_nt1_ms2_ne10_tn", "bf3_k3s2_w4x1_nt1_ms2_ne10_tn", "bf3_k3s2_w4x1_nt1_ms2_ne6_tn", "h2_k3s1_w3x1_nt1_ms1_rows_pow2",
            "h2_k3s1_w4x1_nt1_ms1_rows_pow2"},
    "train": {"bf3_k1s1_w3x1_nt1_ms1_ne6_tn_precise", "bf3_k1s1_w4x1_nt1_ms1_g2_tn_precise", "bf3_k1s1_w4x1_nt1_ms1_ne6_tn_precise",
              "bf3_k3s1_w2x2_nt1_ms2_ne10_tn_precise", "bf3_k3s1_w3x1_nt1_ms1_ne6_tn_precise", "bf3_k3s1_w3x1_nt1_ms1_rows_pow2_precise",
              "bf3_k3s1_w4x1_nt1_ms1_ne6_tn_precise", "bf3_k3s1_w4x1_nt1_ms1_rows_pow2_precise", "bf3_k3s2_w2x2_nt1_ms1_ne10_tn_precise",
              "bf3_k3s2_w2x2_nt1_ms1_ne6_tn_precise", "bf3_k3s2_w3x1_nt1_ms2_ne10_tn_precise", "bf3_k3s2_w4x1_nt1_ms2_ne10_tn_precise",
              "bf3_k3s2_w4x1_nt1_ms2_ne6_tn_precise", "h2_k3s1_w3x1_nt1_ms1_rows_pow2_precise", "h2_k3s1_w4x1_nt1_ms1_rows_pow2_precise"},
    "dgrad": {"bf3_k1s1_w3x1_nt1_ms1_ne6_tn", "bf3_k1s1_w4x1_nt1_ms1_g2_tn", "bf3_k1s1_w4x1_nt1_ms1_ne6_tn", "bf3_k3s1_w2x2_nt1_ms2_ne10_tn",
              "bf3_k3s1_w2x2_nt1_ms2_ne10_tn_dil2", "bf3_k3s1_w3x1_nt1_ms1_ne6_tn", "bf3_k3s1_w3x1_nt1_ms1_ne6_tn_dil2",
              "bf3_k3s1_w3x1_nt1_ms1_rows_pow2", "bf3_k3s1_w3x1_nt1_ms1_rows_pow2_dil2", "bf3_k3s1_w4x1_nt1_ms1_ne6_tn",
              "bf3_k3s1_w4x1_nt1_ms1_ne6_tn_dil2", "bf3_k3s1_w4x1_nt1_ms1_rows_pow2", "bf3_k3s1_w4x1_nt1_ms1_rows_pow2_dil2",
              "h2_k3s1_w3x1_nt1_ms1_rows_pow2", "h2_k3s1_w4x1_nt1_ms1_rows_pow2"},
    "parity": set(),
}


def _rows_of(use):
    """[(form, split, kind, shape)] of a use's table (the training table: its one-conv graphs)."""
    if use == "fwd":
        return [(r[4], r[0], r[1], r[2]) for r in FWD_CASES]
    if use == "train":
        return [(form, split, "conv", (n, args[0], args[1], hw[0], hw[1], args[2], args[3])) for split, graph, args, n, hw, conv, form in TRAIN_CASES
                if graph == "single"]
    return [(form, split, "conv", shape) for split, shape, form in (DGRAD_CASES if use == "dgrad" else PARITY_CASES)]


@pytest.mark.parametrize("use", sf.USES)
def test_every_form_sees_a_ragged_last_tile_in_rows_and_columns(use):
    """Per form: the row's map leaves a partly filled last tile in rows AND in columns (where the odd-tile decode, the tile walk and the
    store's bounds can go wrong), unless no shape of the sweep that reaches the form does -- those forms are listed by name in NOT_RAGGED."""
    found = sf.sweep(use)
    cannot = {form for form, cases in found.items() if not any(all(sf.ragged(use, kind, shape, tile)) for _, kind, shape, tile in cases)}
    assert cannot == NOT_RAGGED[use], (sorted(cannot - NOT_RAGGED[use]), sorted(NOT_RAGGED[use] - cannot))
    assert all(tile[0] in (1, sf.grid_hw(use, kind, shape)[0]) for form in cannot for _, kind, shape, tile in found[form]), "one row, or all the map's rows"
    bad = []
    for form, split, kind, shape in _rows_of(use):
        f = sf.query(use, split, *shape, kind)
        rows, cols = sf.ragged(use, kind, shape, (f.th, f.tw, f.tn))
        if not cols or not (rows or form in cannot):  # (every form has shapes with ragged columns)
            bad.append((form, shape, (f.th, f.tw, f.tn)))
    assert not bad, bad


def test_forms_the_older_case_tables_reach():
    """The per-operator tables that predate this suite, held to the query: CONV_CASES and the transposed-conv shapes (test_gpu_models.py)
    reach 40 of the forward forms, DG_CASES (test_gpu_train_entries.py) and WG_CASES (test_gpu_train.py) 17 of the data-gradient and 6 of the
    parity forms -- the figures DESIGN.md quotes.  A re-tuned threshold that moves one of their cases shows here."""
    import test_gpu_models as tm
    import test_gpu_train as tt
    import test_gpu_train_entries as te

    reached = {use: set() for use in sf.USES}
    for n, cin, cout, h, w, k, s, relu, r1, r2, up, nchw in tm.CONV_CASES:
        for split in ("bf3", "h2"):
            if (cin % 32 and cin != 48) or (k == 1 and (cout % 16 or nchw)):  # (the cases test_fused_conv_vs_torch_cpu skips)
                continue
            reached["fwd"].add(sf.name(sf.query("fwd", split, n, cin, cout, h, w, k, s, relu=relu, res1=r1, res2=r2, up=up, nchw=nchw)))
    for n, cin, cout, h, w in [(2, 64, 32, 8, 6), (3, 256, 256, 16, 12), (1, 2048, 256, 8, 6), (2, 32, 48, 5, 7)]:  # test_deconv_mfma_vs_torch_cpu
        for split in ("bf3", "h2"):
            reached["fwd"].add(sf.name(sf.query("fwd", split, n, cin, cout, h, w, 4, 2, "deconv", relu=True)))
    for n, cin, cout, h, w, k in te.DG_CASES:
        reached["dgrad"].add(sf.name(sf.query("dgrad", "h2", n, cin, cout, h, w, k, 1)))
    for n, cin, cout, h, w, k, s in tt.WG_CASES:  # (the conditions of test_conv_wgrad_and_dgrad_vs_torch)
        if (cout % 32 == 0 or cout == 48) and (k == 3 or s == 1):
            reached["dgrad"].add(sf.name(sf.query("dgrad", "bf3", n, cin, cout, h, w, k, s), s))
        if k == 3 and s == 2 and h % 2 == 0 and w % 2 == 0 and cin % 4 == 0 and (cout % 32 == 0 or cout == 48):
            for split in ("bf3", "h2"):
                reached["parity"].add(sf.name(sf.query("parity", split, n, cin, cout, h, w, k, s)))
    for use in ("fwd", "dgrad", "parity"):
        assert reached[use] <= set(sf.sweep(use)), (use, sorted(reached[use] - set(sf.sweep(use))))
    assert [len(reached[use]) for use in ("fwd", "dgrad", "parity")] == [40, 17, 6]


def test_support_predicate_sees_the_launch_of_a_transposed_conv():
    """mval_op_algo_supported builds the launch as mval_op_launch does (the four parities in one launch enter the tile choice): 64 images of
    1 x 16 with 256 output channels take 32-pixel tiles of two images, which the fp16 split refuses -- the predicate says so (it used to
    evaluate the one-parity tile and accept), and bf16x3 takes it."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    op = _query_op(sf.OP_DECONV, 4, 2, 1, 32, 256, 1, 16, 2, 32)
    ok = lambda algo: bool(_lib.lib().mval_op_algo_supported(C.byref(op), C.c_int(64), C.c_int(algo)))
    assert not ok(sf.ALGO_MFMA_H2) and ok(sf.ALGO_MFMA_BF3)
    assert sf.query("fwd", "h2", 64, 32, 256, 1, 16, 4, 2, "deconv") is None
    f = sf.query("fwd", "bf3", 64, 32, 256, 1, 16, 4, 2, "deconv")
    assert f.tn == 2 and f.grid_z == 4


def test_forward_rows_carry_the_edges_and_options():
    """What the rows were chosen for, held: at least two images on every one-image-per-tile form (image 0's independence of the batch), a
    batch the images-per-tile count does not divide; ragged last tiles in rows and columns, a partly empty last cout group and a ragged cout
    sub-tile on most forms; over the table both residuals with and without ReLU, up 1 .. 3 on 1x1, NCHW output, and different magnitudes
    in every fp16x2 batch."""
    ragged_rows = ragged_cols = ragged_cout = 0
    for row in FWD_CASES + FWD_EXTRA:
        split, kind, (n, cin, cout, h, w, k, s), opts, form = row
        o, mag = _opts(opts)
        f = _fwd_form(row)
        ho, wo = (h, w) if kind == "deconv" else ((h - 1) // s + 1, (w - 1) // s + 1)
        assert n >= 2 and (f.tn == 1 or (n % f.tn and n > f.tn)), _fwd_id(row)
        assert mag == (split == "h2") and (not o["up"] or k == 1), _fwd_id(row)
        ragged_rows += bool(ho % f.th)  # (a last tile that the map fills only partly)
        ragged_cols += bool(wo % f.tw)
        ragged_cout += bool(cout % (16 * f.nt * f.wn))
    n_rows = len(FWD_CASES + FWD_EXTRA)
    assert ragged_rows >= n_rows // 2 and ragged_cols >= n_rows // 2 and ragged_cout >= n_rows // 2, (ragged_rows, ragged_cols, ragged_cout, n_rows)
    seen = {tuple(sorted(k_ for k_, v in _opts(r[3])[0].items() if v and k_ != "up")) for r in FWD_CASES + FWD_EXTRA}
    assert {(), ("relu",), ("res1",), ("relu", "res1"), ("res1", "res2"), ("relu", "res1", "res2"), ("nchw",), ("nchw", "relu")} <= seen, seen
    assert {_opts(r[3])[0]["up"] for r in FWD_CASES + FWD_EXTRA if r[2][5] == 1} == {0, 1, 2, 3}
    assert {19, 20} <= {r[2][2] for r in FWD_EXTRA if r[2][5] == 3} and any(r[2][1] == 48 and _fwd_form(r).ms == 4 for r in FWD_EXTRA)
    assert any(r[2][5:] == (1, 2) and r[2][3] % 2 for r in FWD_EXTRA)  # the stride-2 1x1 conv on an odd input size


def test_training_rows_include_the_named_forms():
    """The training-forward table reaches, with the partials kept: row sharing with MS = 4, an odd tile, WN = 3, stride 2 with MS = 2 and 10
    staging slots, the two-chunk 1x1 forms including NT = 2, ragged tiles in both directions; and 16-pixel forms where they are off."""
    kept, off = set(), set()
    ragged = False
    for split, graph, args, n, hw, conv, form in TRAIN_CASES:
        if graph != "single":
            continue
        cin, cout, k, s = args
        f = sf.query("train", split, n, cin, cout, hw[0], hw[1], k, s)
        assert sf.name(f) == form
        (kept if f.bn_part else off).add(form)
        ho, wo = (hw[0] - 1) // s + 1, (hw[1] - 1) // s + 1
        ragged |= bool(f.bn_part and ho % f.th and wo % f.tw and ho > f.th and wo > f.tw)
    for split in ("bf3", "h2"):
        for want in ("k3s1_w4x1_nt1_ms4_rows_pow2", "k3s1_w4x1_nt1_ms4_ne6_odd", "k3s1_w3x1_nt1_ms4_rows_pow2", "k3s2_w3x1_nt1_ms2_ne10_pow2",
                     "k1s1_w4x1_nt1_ms2_g2_pow2", "k1s1_w4x1_nt1_ms4_g2_pow2", "k1s1_w4x1_nt2_ms4_g2_pow2"):
            assert f"{split}_{want}_precise" in kept, (split, want)
        assert f"{split}_k3s1_w4x1_nt1_ms1_rows_pow2_precise" in off and f"{split}_k1s1_w4x1_nt1_ms1_g2_pow2_precise" in off
    assert ragged


# ---- GPU ----
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _ref_conv(x, w, scale, shift, stride, relu, res1, res2, up, transposed):
    y = F.conv_transpose2d(x, w, None, stride=stride, padding=1) if transposed else F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2)
    y = y * scale[None, :, None, None] + shift[None, :, None, None]
    if up:
        y = F.interpolate(y, scale_factor=2 ** up, mode="nearest")
    for r in (res1, res2):
        if r is not None:
            y = y + r
    return F.relu(y) if relu else y


@gpu
@pytest.mark.parametrize("row", FWD_CASES + FWD_EXTRA, ids=_fwd_id)
def test_split_forward_form_vs_float64(dev, row):
    """ops.fused_conv (mval_op_launch) on the row's form, the bounds of test_fused_conv_vs_torch_cpu: elementwise rtol 1e-4 / atol 2e-5 (3e-5
    for the transposed conv) against the float64 reference rounded to float32; rms error <= 1.25 x and max error <= 2.5 x the exact-fp32
    MFMA kernel's on the same problem (+ 1e-8 / 1e-7), over the batch and, where the images differ in magnitude, per image; the kept per-image
    max |x| rows equal to amax of the stored output; image 0 alone (or, where one image takes another kernel form, image 0 next to other
    images than before) gives image 0's bits on every one-image-per-tile form."""
    from multi_view_active_learning_amd import ops

    split, kind, (n, cin, cout, h, w, k, stride), opts, form = row
    o, mag = _opts(opts)
    f = _fwd_form(row)
    assert f is not None and sf.name(f) == form, "the case must run on the form it is in the table for"
    transposed = kind == "deconv"
    rng = np.random.default_rng(zlib.crc32(_fwd_id(row).encode()))
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    x = f32(rng.standard_normal((n, cin, h, w)))
    if mag:
        assert n >= 2
        x[:-1] *= 2.0 ** -10
    taps = 4 if transposed else k * k  # (taps that meet one output pixel)
    wt = f32(rng.standard_normal((cin, cout, k, k) if transposed else (cout, cin, k, k)) * np.sqrt(2.0 / (cin * taps)))
    scale = f32(rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.5, -1.0, 1.0))
    shift = f32(rng.standard_normal(cout) * 0.1)
    ho, wo = ((2 * h, 2 * w) if transposed else ((h - 1) // stride + 1, (w - 1) // stride + 1))
    ho, wo = ho << o["up"], wo << o["up"]
    res1 = f32(rng.standard_normal((n, cout, ho, wo))) if o["res1"] else None
    res2 = f32(rng.standard_normal((n, cout, ho, wo))) if o["res2"] else None
    d64 = lambda t: None if t is None else t.double()
    want64 = _ref_conv(x.double(), wt.double(), scale.double(), shift.double(), stride, o["relu"], d64(res1), d64(res2), o["up"], transposed)
    nhwc = lambda t: None if t is None else t.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, sd, bd = wt.to(dev), scale.to(dev), shift.to(dev)

    def run(algo, xs, r1, r2):
        y = ops.fused_conv(nhwc(xs), wd, sd, bd, stride=stride, pad=1 if transposed else None, relu=o["relu"], res1=nhwc(r1), res2=nhwc(r2), up=o["up"],
                           algo=algo, out_nchw=o["nchw"], kind=ops.OP_DECONV if transposed else ops.OP_CONV)
        kept = ops.fused_conv.last_out_amax.cpu().view(torch.float32)
        return (y.cpu() if o["nchw"] else y.permute(0, 3, 1, 2).cpu()), kept

    got, kept = run(sf.ALGO_OF[split], x, res1, res2)
    if not o["nchw"] and cout % 4 == 0:  # (where the kernel keeps them: the float4 store path)
        assert torch.equal(kept, got.abs().amax(dim=(1, 2, 3))), "per-image max |x| rows"
    exact, _ = run(sf.ALGO_MFMA, x, res1, res2)
    err = lambda y, i=slice(None): ((y.double() - want64)[i].abs().max().item(), (y.double() - want64)[i].pow(2).mean().sqrt().item())
    (max_gpu, rms_gpu), (max_f32, rms_f32) = err(got), err(exact)
    print(f"[split forms] {_fwd_id(row)}: tile {f.th}x{f.tw}x{f.tn} grid {f.grid_x}x{f.grid_y}x{f.grid_z}; rms {rms_gpu:.3e} (exact fp32 {rms_f32:.3e}), "
          f"max {max_gpu:.3e} ({max_f32:.3e})")
    np.testing.assert_allclose(got.numpy(), want64.float().numpy(), rtol=1e-4, atol=3e-5 if transposed else 2e-5)
    assert rms_gpu <= 1.25 * rms_f32 + 1e-8 and max_gpu <= 2.5 * max_f32 + 1e-7, (split, max_gpu, max_f32, rms_gpu, rms_f32)
    if mag:
        for i in range(n):
            (mi, ri), (mf, rf) = err(got, i), err(exact, i)
            assert ri <= 1.25 * rf + 1e-8 and mi <= 2.5 * mf + 1e-7, ("image", i, mi, mf, ri, rf)
    if f.tn == 1:
        sub = lambda t: None if t is None else t[:1]
        f1 = _fwd_form(row, n=1)
        if f1 is not None and (sf.name(f1), f1.th, f1.tw) == (form, f.th, f.tw):
            alone, _ = run(sf.ALGO_OF[split], x[:1], sub(res1), sub(res2))
        else:  # (a batch of one takes another kernel: the same batch size with other images behind image 0)
            x2 = torch.cat([x[:1], f32(rng.standard_normal((n - 1, cin, h, w)) * 4.0)])
            alone, _ = run(sf.ALGO_OF[split], x2, res1, res2)
        assert torch.equal(alone[0], got[0]), "image 0 does not depend on the rest of the batch"


def _dgrad_case(dev, split, shape, seed):
    """dz (scaled by 2^-9, NHWC on the device), its magnitude row (the maximum in the last partial), the float64 data gradient (NHWC) and a
    base of its magnitude to accumulate into."""
    from test_gpu_train_entries import _conv_grads, _nhwc, _row

    n, cin, cout, h, w, k, s = shape
    x, wt, dz, dx64, _ = _conv_grads(n, cin, cout, h, w, k, s, k // 2, seed, dz_scale=2.0 ** -9)
    want = np.transpose(dx64, (0, 2, 3, 1))
    base = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((n, h, w, cin)).astype(np.float32) * np.float32(np.abs(want).max())).to(dev)
    return wt, dz, _nhwc(dz, dev), _row(dz, dev), want, base


def _dgrad_check(tag, run, want, base):
    """Store over stale contents, then accumulate: relative L2 < 2e-5 against float64 (after subtracting the base when accumulating)."""
    from test_gpu_train_entries import _rel

    for acc in (0, 1):
        dx = base.clone()
        run(dx, acc)
        got = dx.cpu().numpy().astype(np.float64) - (base.cpu().numpy().astype(np.float64) if acc else 0.0)
        e = _rel(got, want)
        print(f"[split forms] {tag} accumulate={acc}: rel L2 {e:.2e}")
        assert e < 2e-5, (acc, e)


@gpu
@pytest.mark.parametrize("row", DGRAD_CASES, ids=_shape_id)
def test_split_dgrad_form_vs_float64(dev, row):
    """mval_conv_dgrad_scaled on the row's form: both splits at stride 1 (k1, k3), bf16x3 on the zero-dilated stride-2 form."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _PACK_OF

    split, shape, form = row
    n, cin, cout, h, w, k, s = shape
    algo = sf.ALGO_OF[split]
    for acc in (False, True):
        f = sf.query("dgrad", split, *shape, res1=acc)
        assert f is not None and sf.name(f, s) == form, "the case must run on the form it is in the table for"
    wt, dz, dzd, row_d, want, base = _dgrad_case(dev, split, shape, 13)
    ho, wo = dz.shape[2:]
    lib, st, p = _lib.lib(), _lib._stream(), _lib._p
    pack = _PACK_OF[algo]
    wp = torch.empty(int(lib.mval_packed_weight_floats(C.c_int(pack), C.c_int(cin), C.c_int(cout), C.c_int(k))), dtype=torch.float32, device=dev)
    wd = wt.contiguous().to(dev)
    _lib._check(lib.mval_pack_conv_weights(C.c_int(pack), C.c_int(2), p(wd), p(wp), C.c_int(cin), C.c_int(cout), C.c_int(k), st), "pack")
    ones = torch.ones(max(cin, cout), dtype=torch.float32, device=dev)
    zeros = torch.zeros_like(ones)

    def run(dx, acc):
        _lib._check(lib.mval_conv_dgrad_scaled(p(dzd), p(wp), p(ones), p(zeros), p(dx), C.c_int(acc), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(cin),
                                               C.c_int(ho), C.c_int(wo), C.c_int(cout), C.c_int(k), C.c_int(s), C.c_int(k // 2), C.c_int(algo), p(row_d), st),
                    "dgrad scaled")

    _dgrad_check(_shape_id(row), run, want, base)


@gpu
@pytest.mark.parametrize("row", PARITY_CASES, ids=_shape_id)
def test_split_dgrad_parity_form_vs_float64(dev, row):
    """mval_conv_dgrad_parity (Conv2d k3 s2 p1 on even sizes as four 2x2 convs over dz) on the row's form, both splits; cin 20 (4-aligned, not
    16-aligned) on the two-wave forms, 40 / 80 (a ragged last cout sub-tile / wave) on the others."""
    from multi_view_active_learning_amd import ops

    split, shape, form = row
    n, cin, cout, h, w, k, s = shape
    for acc in (False, True):
        f = sf.query("parity", split, *shape, res1=acc)
        assert f is not None and sf.name(f) == form and f.grid_z == 4, "the case must run on the form it is in the table for"
    wt, dz, dzd, row_d, want, base = _dgrad_case(dev, split, shape, 17)
    wd = wt.to(dev)

    def run(dx, acc):
        out = ops.conv_dgrad_parity(dzd, wd, (h, w), algo=sf.ALGO_OF[split], accumulate_into=dx if acc else None, dz_amax_row=row_d)
        if not acc:
            dx.copy_(out)

    _dgrad_check(_shape_id(row), run, want, base)


_STATS = {}


@functools.lru_cache(maxsize=None)
def _train_reference(graph, args, n, hw):
    """(input, float64 output, float64 running statistics after one step) of a training graph: computed once, shared by both plans."""
    model = tg.TinyNet(tg.BUILDERS[graph], args, 1)
    x = tg.seeded_input(dict(n=n, hw=hw, seed=1))
    sd = {k_: (v.detach().clone().double() if v.dtype.is_floating_point else v.detach().clone()) for k_, v in model.state_dict().items()}
    with torch.no_grad():
        out, _ = tg.graph_forward(model._graph, sd, x, torch.float64)
    return x, out.numpy(), {k_: v.numpy() for k_, v in sd.items() if k_.endswith(("running_mean", "running_var"))}


@gpu
@pytest.mark.parametrize("key", list(_train_runs()), ids=_train_id)
def test_split_training_forward_form_vs_float64(dev, key, monkeypatch):
    """The training forward (precise kernels; batch statistics from the conv epilogue's partials where the form keeps them) of a small graph
    under the h2 / bf3 plan: the output within rtol 2e-5 / atol 2e-5 x max |out| of float64 and every running mean and variance within rtol
    2e-4 / atol 2e-5 (the bounds of test_small_graph_training_step_vs_float64) -- with the partials and, under MVAL_TRAIN_EPI_STATS=0, with the
    separate statistics pass; the differences between the two are written with the suite's _report to split_form_stats.json (their summation orders differ:
    no bit equality is asserted).  A padded pixel of a ragged tile in the sums would move a mean by a fraction of its value."""
    from multi_view_active_learning_amd import engine_train as et
    from test_gpu_train import _report

    split, graph, args, n, hw = key
    x, want_out, want_stats = _train_reference(graph, args, n, hw)
    res = {}
    for epi in ("1", "0"):
        for k_ in et._SWITCHES:
            monkeypatch.delenv(k_, raising=False)
        for k_, v in dict(PLANS[split], MVAL_TRAIN_EPI_STATS=epi).items():
            monkeypatch.setenv(k_, v)
        model = tg.TinyNet(tg.BUILDERS[graph], args, 1).to(dev).train()
        with torch.no_grad():
            out = model(x.to(dev))
        plan = next(iter(model._train_plans.values()))
        assert all(bool(t.p2_flags & et.TRAIN_STATS_PASS) == (epi == "0") for t in plan.ops) and not plan.uses_p2
        forms = _train_forms(plan, split, n)
        for conv, form in _train_runs()[key]:  # the plan ran the conv on the split algo it names, on the form the row is in the table for
            assert conv in forms and forms[conv][0] == form and forms[conv][2] == sf.ALGO_OF[split], (conv, forms.get(conv))
        got = out.cpu().numpy()
        np.testing.assert_allclose(got, want_out, rtol=2e-5, atol=2e-5 * float(np.abs(want_out).max()), err_msg=f"EPI_STATS={epi}")
        stats = {k_: v.cpu().numpy() for k_, v in model.state_dict().items() if k_.endswith(("running_mean", "running_var"))}
        assert set(stats) == set(want_stats)
        for k_, v in stats.items():
            np.testing.assert_allclose(v, want_stats[k_], rtol=2e-4, atol=2e-5, err_msg=f"{k_} EPI_STATS={epi}")
        res[epi] = (got, stats, {c: bool(v[1].bn_part) for c, v in forms.items()})
    diff = {k_: float(np.abs(res["1"][1][k_].astype(np.float64) - res["0"][1][k_]).max()) for k_ in want_stats}
    d_out = float(np.abs(res["1"][0].astype(np.float64) - res["0"][0]).max())
    print(f"[split forms] {_train_id(key)}: partials kept by {res['1'][2]}; epilogue vs separate pass: max |d out| {d_out:.2e}, max |d stat| {max(diff.values()):.2e}")
    _STATS[_train_id(key)] = dict(partials_kept=res["1"][2], max_abs_diff_out=d_out, max_abs_diff_stats=diff)
    _report("split_form_stats.json", _STATS)

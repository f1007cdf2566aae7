"""The P2 conv (csrc/conv_p2.hip: conv_p2_kernel -- every conv of the default inference plans and of the default training plan) alone, at
every inference form its dispatch picks, and on the later tiles of a workgroup's walk.

Which form a launch runs on is read from the library's own dispatch (mval_conv_p2_form: the launcher's dry run, host arithmetic, no GPU;
tests/p2_forms.py names the forms -- kernel instance + runtime path -- and holds the sweep).  The host tests hold every row of the case table
to the form it is in the table for, the table to every form a fixed sweep of shapes finds for mval_op_launch, and the forms of the two
training uses to those the small training graphs reach (tests/test_train_small_graphs.py runs them against float64 autograd) plus the forms no
training plan can reach, each with the plan rule that excludes it.  The GPU tests run each row against float64 and repeat the form assertion
on the shape they ran.

Rows were chosen from the sweep as the cheapest shape (device tensors + float64 reference) that reaches the form with, where the form's own
conditions allow it, at least two images (three where that costs nothing: an odd batch), a ragged last tile in rows and in columns (odd-tile
forms need W % OW == 0: rows only), a cout that leaves the last cout sub-tile partly empty (cout = 8 mod 16; 19 for NCHW output) and a tile
count that is no multiple of 8 (an uneven walk).  Rotated over the rows of every family (1x1, flattened 1x1, stride-2 1x1, 3x3 stride 1 and 2,
parity conv) and epilogue: ReLU / res1 / res1 + res2 / nothing, a cin with a partly filled last 32-channel chunk (8, 40, 72), on G = 2 forms
a chunk count G does not divide (72, 96), and `mag`: every image but the last scaled by 2^-10, so that a scale read from another image's row
overflows fp16 or loses ten bits.  The parity conv and the fp32 NCHW output take no residuals: ReLU or nothing.

`mag` scales an image's residuals with its input.  The residuals have magnitude rows of their own, read per image like the input's, so the
option then covers all three; and the rms bound against the exact-fp32 chain has a meaning only then.  With residuals of magnitude 1 next to
a conv output of 2^-10 the output is, to ten bits, the sum of its inputs: the exact chain holds those inputs exactly and rounds once to 24
bits, while the P2 format itself holds each of them, and the sum, to 2^-23 -- no kernel over P2 planes can stay within 1.25 x of that.
(Rounding alone, emulated on the CPU for 64 x 256 x 7 x 100 with two such residuals: 1.05e-7 at 23 bits against 4.8e-8 for float32; the
kernel measured 9.65e-8 against the exact chain's 5.73e-8 there.)"""
import functools
import os
import re
import zlib
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mfma_forms as mf
import p2_forms as pf

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]

# ---- the case table: one row per form of mval_op_launch ----
# ("conv" | "deconv" (ConvTranspose2d k4 s2 p1), (n, cin, cout, h, w, k, stride) of the conv on an h x w input, epilogue + data options, the
# form the row is in the table for).  Options: relu, res1, res2, up1 .. up3 (nearest up-sampling, 1x1 only), nchw (fp32 NCHW output), mag.
# The forms with two cout sub-tiles per wave of the 1x1 conv (`nt2`) start at 1024 tile groups: ceil(px / 64) * (cout / 128) >= 1024, so
# their rows have 32 768 pixels and 256 couts (8.4 M output elements; 33.5 M behind up1) -- the smallest the rule admits.
#
# Lines of mval_launch_conv_p2 no USE_OP launch of the product can reach, hence without a row:
#  - every branch on oms / ont / og (3x3 stride 1 at MS = 8 and the two `ont == 2` lines, 3x3 stride 2 at MS = 4, 1x1 at G = 1 or 4 and at
#    MS = 8): p2_override reads them from the environment in -DP2_TUNE measurement builds only; the product leaves them 0.  (The instances
#    <3,1,1,4,1,2,4,16,true> and <3,1,1,4,1,2,4,8> of the `ont == 2` lines ARE reached, by the NS % 8 == 0 rule above them.)
#  - the in_z / bs_z blocks, EPI 3 and the K48 instance behind out_nhwc: training launches (the other two uses).
#  - 1x1 with NT = 2 and fp32 NCHW output: launch_p2 has no such instance and answers "unsupported".
#  - pairs the sweep's domain cannot hold: NT = 2 on a 1x1 map that is NOT flattened at 8-, 16- and 32-wide tiles with EPI 0 needs 1024
#    tile groups on maps of one row or under 64 pixels -- batches of thousands of images.  Their instances are in the table by their
#    flattened and stride-2 paths.
OP_CASES = [
    ("conv", (3, 8, 8, 2, 16, 1, 1), "relu+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e0"),
    ("conv", (3, 8, 8, 13, 6, 1, 1), "relu+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e0_flat"),
    ("conv", (3, 8, 8, 4, 32, 1, 2), "relu+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e0_sub"),
    ("conv", (2, 8, 8, 2, 16, 1, 1), "relu+up1+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e1"),
    ("conv", (2, 8, 8, 4, 32, 1, 2), "relu+up1+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e1_sub"),
    ("conv", (2, 8, 19, 2, 16, 1, 1), "relu+nchw+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e2"),
    ("conv", (2, 8, 19, 13, 6, 1, 1), "relu+nchw+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e2_flat"),
    ("conv", (2, 8, 19, 4, 32, 1, 2), "relu+nchw+mag", "k1s1_g2_w2x2_nt1_ms2_tw16_e2_sub"),
    ("conv", (3, 72, 8, 1, 32, 1, 1), "res1", "k1s1_g2_w2x2_nt1_ms2_tw32_e0"),
    ("conv", (3, 72, 8, 5, 18, 1, 1), "res1", "k1s1_g2_w2x2_nt1_ms2_tw32_e0_flat"),
    ("conv", (3, 72, 8, 5, 64, 1, 2), "res1", "k1s1_g2_w2x2_nt1_ms2_tw32_e0_sub"),
    ("conv", (2, 72, 8, 1, 32, 1, 1), "res1+up2", "k1s1_g2_w2x2_nt1_ms2_tw32_e1"),
    ("conv", (2, 72, 8, 5, 64, 1, 2), "res1+up2", "k1s1_g2_w2x2_nt1_ms2_tw32_e1_sub"),
    ("conv", (2, 72, 19, 1, 32, 1, 1), "nchw", "k1s1_g2_w2x2_nt1_ms2_tw32_e2"),
    ("conv", (2, 72, 19, 5, 18, 1, 1), "nchw", "k1s1_g2_w2x2_nt1_ms2_tw32_e2_flat"),
    ("conv", (2, 72, 19, 5, 64, 1, 2), "nchw", "k1s1_g2_w2x2_nt1_ms2_tw32_e2_sub"),
    ("conv", (3, 32, 8, 4, 64, 1, 1), "res1+res2+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e0"),
    ("conv", (3, 32, 8, 7, 18, 1, 1), "res1+res2+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e0_flat"),
    ("conv", (3, 32, 8, 4, 128, 1, 2), "res1+res2+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e0_sub"),
    ("conv", (2, 32, 8, 5, 64, 1, 1), "res1+res2+up3+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e1"),
    ("conv", (2, 32, 8, 4, 128, 1, 2), "res1+res2+up3+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e1_sub"),
    ("conv", (2, 32, 19, 5, 64, 1, 1), "relu+nchw+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e2"),
    ("conv", (2, 32, 19, 7, 18, 1, 1), "relu+nchw+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e2_flat"),
    ("conv", (2, 32, 19, 4, 128, 1, 2), "relu+nchw+mag", "k1s1_g2_w2x2_nt1_ms2_tw64_e2_sub"),
    ("conv", (3, 8, 8, 5, 7, 1, 1), "", "k1s1_g2_w2x2_nt1_ms2_tw8_e0"),
    ("conv", (3, 8, 8, 5, 13, 1, 1), "", "k1s1_g2_w2x2_nt1_ms2_tw8_e0_flat"),
    ("conv", (3, 8, 8, 13, 9, 1, 2), "", "k1s1_g2_w2x2_nt1_ms2_tw8_e0_sub"),
    ("conv", (2, 8, 8, 5, 7, 1, 1), "up1", "k1s1_g2_w2x2_nt1_ms2_tw8_e1"),
    ("conv", (2, 8, 8, 13, 9, 1, 2), "up1", "k1s1_g2_w2x2_nt1_ms2_tw8_e1_sub"),
    ("conv", (2, 8, 19, 5, 7, 1, 1), "nchw", "k1s1_g2_w2x2_nt1_ms2_tw8_e2"),
    ("conv", (2, 8, 19, 5, 13, 1, 1), "nchw", "k1s1_g2_w2x2_nt1_ms2_tw8_e2_flat"),
    ("conv", (2, 8, 19, 13, 9, 1, 2), "nchw", "k1s1_g2_w2x2_nt1_ms2_tw8_e2_sub"),
    ("conv", (3, 72, 40, 2, 16, 1, 1), "relu+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e0"),
    ("conv", (3, 72, 40, 13, 6, 1, 1), "relu+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e0_flat"),
    ("conv", (3, 72, 40, 4, 32, 1, 2), "relu+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e0_sub"),
    ("conv", (2, 72, 40, 2, 16, 1, 1), "relu+up2+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e1"),
    ("conv", (2, 72, 40, 4, 32, 1, 2), "relu+up2+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e1_sub"),
    ("conv", (2, 72, 40, 2, 16, 1, 1), "relu+nchw+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e2"),
    ("conv", (2, 72, 40, 13, 6, 1, 1), "relu+nchw+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e2_flat"),
    ("conv", (2, 72, 40, 4, 32, 1, 2), "relu+nchw+mag", "k1s1_g2_w4x1_nt1_ms4_tw16_e2_sub"),
    ("conv", (3, 32, 40, 1, 32, 1, 1), "relu+res1", "k1s1_g2_w4x1_nt1_ms4_tw32_e0"),
    ("conv", (3, 32, 40, 5, 18, 1, 1), "relu+res1", "k1s1_g2_w4x1_nt1_ms4_tw32_e0_flat"),
    ("conv", (3, 32, 40, 5, 64, 1, 2), "relu+res1", "k1s1_g2_w4x1_nt1_ms4_tw32_e0_sub"),
    ("conv", (2, 32, 40, 1, 32, 1, 1), "relu+res1+up3", "k1s1_g2_w4x1_nt1_ms4_tw32_e1"),
    ("conv", (2, 32, 40, 5, 64, 1, 2), "relu+res1+up3", "k1s1_g2_w4x1_nt1_ms4_tw32_e1_sub"),
    ("conv", (2, 32, 40, 1, 32, 1, 1), "nchw", "k1s1_g2_w4x1_nt1_ms4_tw32_e2"),
    ("conv", (2, 32, 40, 5, 18, 1, 1), "nchw", "k1s1_g2_w4x1_nt1_ms4_tw32_e2_flat"),
    ("conv", (2, 32, 40, 5, 64, 1, 2), "nchw", "k1s1_g2_w4x1_nt1_ms4_tw32_e2_sub"),
    ("conv", (3, 8, 40, 4, 64, 1, 1), "relu+res1+res2+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e0"),
    ("conv", (3, 8, 40, 7, 18, 1, 1), "relu+res1+res2+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e0_flat"),
    ("conv", (3, 8, 40, 4, 128, 1, 2), "relu+res1+res2+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e0_sub"),
    ("conv", (2, 8, 40, 5, 64, 1, 1), "relu+res1+res2+up1+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e1"),
    ("conv", (2, 8, 40, 4, 128, 1, 2), "relu+res1+res2+up1+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e1_sub"),
    ("conv", (2, 8, 40, 5, 64, 1, 1), "relu+nchw+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e2"),
    ("conv", (2, 8, 40, 7, 18, 1, 1), "relu+nchw+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e2_flat"),
    ("conv", (2, 8, 40, 4, 128, 1, 2), "relu+nchw+mag", "k1s1_g2_w4x1_nt1_ms4_tw64_e2_sub"),
    ("conv", (3, 72, 40, 5, 7, 1, 1), "", "k1s1_g2_w4x1_nt1_ms4_tw8_e0"),
    ("conv", (3, 72, 40, 5, 13, 1, 1), "", "k1s1_g2_w4x1_nt1_ms4_tw8_e0_flat"),
    ("conv", (3, 72, 40, 13, 9, 1, 2), "", "k1s1_g2_w4x1_nt1_ms4_tw8_e0_sub"),
    ("conv", (2, 72, 40, 5, 7, 1, 1), "up2", "k1s1_g2_w4x1_nt1_ms4_tw8_e1"),
    ("conv", (2, 72, 40, 13, 9, 1, 2), "up2", "k1s1_g2_w4x1_nt1_ms4_tw8_e1_sub"),
    ("conv", (2, 72, 40, 5, 7, 1, 1), "nchw", "k1s1_g2_w4x1_nt1_ms4_tw8_e2"),
    ("conv", (2, 72, 40, 5, 13, 1, 1), "nchw", "k1s1_g2_w4x1_nt1_ms4_tw8_e2_flat"),
    ("conv", (2, 72, 40, 13, 9, 1, 2), "nchw", "k1s1_g2_w4x1_nt1_ms4_tw8_e2_sub"),
    ("conv", (32, 32, 256, 13, 80, 1, 1), "relu+mag", "k1s1_g2_w4x1_nt2_ms4_tw16_e0_flat"),
    ("conv", (64, 32, 256, 64, 32, 1, 2), "relu+mag", "k1s1_g2_w4x1_nt2_ms4_tw16_e0_sub"),
    ("conv", (32, 32, 256, 13, 80, 1, 1), "relu+up1+mag", "k1s1_g2_w4x1_nt2_ms4_tw16_e1"),
    ("conv", (64, 32, 256, 64, 32, 1, 2), "relu+up1+mag", "k1s1_g2_w4x1_nt2_ms4_tw16_e1_sub"),
    ("conv", (32, 40, 256, 33, 32, 1, 1), "res1", "k1s1_g2_w4x1_nt2_ms4_tw32_e0_flat"),
    ("conv", (64, 40, 256, 33, 64, 1, 2), "res1", "k1s1_g2_w4x1_nt2_ms4_tw32_e0_sub"),
    ("conv", (32, 40, 256, 33, 32, 1, 1), "up1", "k1s1_g2_w4x1_nt2_ms4_tw32_e1"),
    ("conv", (64, 40, 256, 33, 64, 1, 2), "up1", "k1s1_g2_w4x1_nt2_ms4_tw32_e1_sub"),
    ("conv", (64, 32, 256, 4, 128, 1, 1), "relu+mag", "k1s1_g2_w4x1_nt2_ms4_tw64_e0"),
    ("conv", (64, 96, 256, 7, 100, 1, 1), "res1+res2+mag", "k1s1_g2_w4x1_nt2_ms4_tw64_e0_flat"),
    ("conv", (64, 96, 256, 16, 128, 1, 2), "res1+res2+mag", "k1s1_g2_w4x1_nt2_ms4_tw64_e0_sub"),
    ("conv", (64, 96, 256, 4, 128, 1, 1), "relu+up1+mag", "k1s1_g2_w4x1_nt2_ms4_tw64_e1"),
    ("conv", (64, 96, 256, 16, 128, 1, 2), "relu+up1+mag", "k1s1_g2_w4x1_nt2_ms4_tw64_e1_sub"),
    ("conv", (64, 32, 256, 33, 18, 1, 1), "", "k1s1_g2_w4x1_nt2_ms4_tw8_e0_flat"),
    ("conv", (64, 32, 256, 24, 100, 1, 2), "", "k1s1_g2_w4x1_nt2_ms4_tw8_e0_sub"),
    ("conv", (64, 32, 256, 33, 18, 1, 1), "up1", "k1s1_g2_w4x1_nt2_ms4_tw8_e1"),
    ("conv", (64, 32, 256, 24, 100, 1, 2), "up1", "k1s1_g2_w4x1_nt2_ms4_tw8_e1_sub"),
    ("deconv", (3, 8, 8, 5, 16, 4, 2), "relu+mag", "k2s1_g1_w2x2_nt1_ms2_tw16_e0_par"),
    ("deconv", (3, 8, 8, 4, 5, 4, 2), "", "k2s1_g1_w2x2_nt1_ms2_tw8_e0_par"),
    ("deconv", (3, 32, 40, 8, 6, 4, 2), "relu+mag", "k2s1_g1_w4x1_nt1_ms3_ow6_e0_par"),
    ("deconv", (3, 8, 40, 5, 16, 4, 2), "", "k2s1_g1_w4x1_nt1_ms4_tw16_e0_par"),
    ("deconv", (3, 8, 40, 4, 5, 4, 2), "relu+mag", "k2s1_g1_w4x1_nt1_ms4_tw8_e0_par"),
    ("deconv", (3, 32, 40, 8, 12, 4, 2), "", "k2s1_g1_w4x1_nt1_ms6_ow12_e0_par"),
    ("deconv", (3, 72, 40, 8, 6, 4, 2), "relu+mag", "k2s1_g2_w4x1_nt1_ms3_ow6_e0_par"),
    ("deconv", (3, 72, 40, 4, 5, 4, 2), "", "k2s1_g2_w4x1_nt1_ms4_tw8_e0_par"),
    ("conv", (3, 8, 8, 4, 5, 3, 1), "relu+mag", "k3s1_g1_w2x2_nt1_ms2_tw8_e0"),
    ("conv", (3, 8, 8, 4, 18, 3, 1), "res1", "k3s1_g1_w2x2_nt1_ms4_tw16_e0_rs"),
    ("conv", (3, 32, 96, 8, 36, 3, 1), "res1+res2+mag", "k3s1_g1_w2x2_nt3_ms3_ow12_e0"),
    ("conv", (3, 8, 40, 8, 6, 3, 1), "", "k3s1_g1_w4x1_nt1_ms3_ow6_e0"),
    ("conv", (3, 8, 40, 4, 18, 3, 1), "relu+mag", "k3s1_g1_w4x1_nt1_ms4_ow18_e0"),
    ("conv", (3, 32, 40, 4, 9, 3, 1), "relu+res1", "k3s1_g1_w4x1_nt1_ms4_ow9_e0"),
    ("conv", (3, 8, 40, 5, 20, 3, 1), "relu+res1+res2+mag", "k3s1_g1_w4x1_nt1_ms4_tw16_e0_rs"),
    ("conv", (3, 48, 40, 5, 20, 3, 1), "", "k3s1_g1_w4x1_nt1_ms4_tw16_e0_rs_k48"),
    ("conv", (3, 32, 40, 4, 5, 3, 1), "relu+mag", "k3s1_g1_w4x1_nt1_ms4_tw8_e0"),
    ("conv", (3, 8, 40, 8, 12, 3, 1), "res1", "k3s1_g1_w4x1_nt1_ms6_ow12_e0"),
    ("conv", (3, 8, 40, 12, 9, 3, 1), "res1+res2+mag", "k3s1_g1_w4x1_nt1_ms7_ow9_e0"),
    ("conv", (3, 32, 128, 8, 6, 3, 1), "", "k3s1_g1_w4x1_nt2_ms3_ow6_e0"),
    ("conv", (3, 8, 128, 5, 16, 3, 1), "relu+mag", "k3s1_g1_w4x1_nt2_ms4_tw16_e0_rs"),
    ("conv", (3, 8, 128, 4, 8, 3, 1), "relu+res1", "k3s1_g1_w4x1_nt2_ms4_tw8_e0"),
    ("conv", (3, 32, 128, 8, 12, 3, 1), "relu+res1+res2+mag", "k3s1_g1_w4x1_nt2_ms6_ow12_e0"),
    ("conv", (3, 8, 192, 8, 18, 3, 1), "", "k3s1_g1_w4x1_nt3_ms3_ow6_e0"),
    ("conv", (3, 8, 8, 12, 7, 3, 2), "relu+mag", "k3s2_g1_w2x2_nt1_ms1_tw8_e0"),
    ("conv", (3, 8, 40, 12, 7, 3, 2), "res1", "k3s2_g1_w4x1_nt1_ms2_tw8_e0"),
    ("conv", (3, 32, 40, 7, 24, 3, 2), "res1+res2+mag", "k3s2_g1_w4x1_nt1_ms3_ow12_e0"),
    ("conv", (3, 8, 40, 16, 12, 3, 2), "", "k3s2_g1_w4x1_nt1_ms3_ow6_e0"),
]
# ---- later tiles of a workgroup: batches so large that tiles_total * groups exceeds what the device can hold resident (p2_forms.resident_cap),
# so some workgroup walks two tiles or more: LDS reuse, the prefetch of the next tile, the max |x| slots and partials kept over the walk.
# Images 0 and 1 repeated (image i = image i % 2), 32 input channels and at most 40 couts (one cout group) but for the NT = 2 row.
LATE_CASES = [
    ("conv", (82, 32, 32, 16, 64, 1, 1), "relu+res1", "k1s1_g2_w2x2_nt1_ms2_tw64_e0"),
    ("conv", (214, 32, 32, 12, 32, 1, 1), "res1+res2+up1", "k1s1_g2_w2x2_nt1_ms2_tw32_e1"),
    ("conv", (34, 32, 19, 13, 24, 1, 1), "nchw", "k1s1_g2_w2x2_nt1_ms2_tw8_e2_flat"),
    ("conv", (214, 32, 32, 17, 33, 1, 2), "relu", "k1s1_g2_w2x2_nt1_ms2_tw8_e0_sub"),
    ("conv", (242, 32, 32, 9, 20, 3, 1), "res1", "k3s1_g1_w2x2_nt1_ms4_tw16_e0_rs"),
    ("conv", (268, 32, 40, 9, 20, 3, 1), "relu+res1+res2", "k3s1_g1_w4x1_nt1_ms4_tw16_e0_rs"),
    ("conv", (202, 32, 40, 22, 18, 3, 1), "", "k3s1_g1_w4x1_nt1_ms4_ow18_e0"),
    ("conv", (162, 32, 40, 18, 22, 3, 2), "res1", "k3s2_g1_w4x1_nt1_ms2_tw8_e0"),
    ("deconv", (216, 32, 32, 17, 20, 4, 2), "relu", "k2s1_g1_w2x2_nt1_ms2_tw8_e0_par"),
    ("conv", (268, 32, 128, 12, 32, 3, 1), "relu+res1", "k3s1_g1_w4x1_nt2_ms4_tw16_e0_rs"),
]
CUS_SIZED_FOR = 320  # the LATE_CASES batches exceed resident_cap with up to this many compute units (the MI355X has 256)
OLDER_REACH = 25  # forms of mval_op_launch that the single-op cases of test_gpu_p2.py reach (test_forms_the_older_case_tables_reach)
RMS_MIN_ELEMENTS = 12960  # the smallest row of test_gpu_p2.P2_CASES: below it the ratio of two small-sample rms values is noise
# the forms of the two training uses that no case of tests/test_train_small_graphs.py reaches (test_training_forms_census): those NO training
# plan reaches (test_no_plan_reaches_the_forms_left_out), each with the plan rule of engine_train.py that excludes it.  Both are the 1x1 conv on
# at most two cout sub-tiles (kernel couts 8, 24, 32) over a map that is not run as one flattened row -- one or two rows of under 64 pixels:
# 2 x 16 and 1 x 48 on 16-wide tiles, 1 x 32 on 32-wide ones.  The dispatch of conv_p2.hip has the form, but a plan only puts a conv on the P2
# kernels whose fp16-split kernel it chose first, and mval_op_algo_supported(MVAL_ALGO_MFMA_H2) has no 1x1 conv of 32 couts or fewer on such
# a map (the plan runs it on the bf16x3 or the exact-fp32 kernel).
_H2_FWD = ("TrainPlan._p2_forward_convs takes only ops whose forward algo is ALGO_MFMA_H2, and _choose_algorithms gives that algo only where "
           "mval_op_algo_supported(ALGO_MFMA_H2) holds: not for this conv")
_H2_DGRAD = ("TrainPlan._p2_dgrads takes only ops whose dgrad_algo is ALGO_MFMA_H2, and _choose_algorithms gives that algo only where "
             "mval_op_algo_supported(ALGO_MFMA_H2) holds for the gradient's conv (cin' = cout, cout' = cin): not for this one")
PLAN_UNREACHABLE = {
    "train": {"k1s1_g2_w2x2_nt1_ms2_tw16_e3": _H2_FWD, "k1s1_g2_w2x2_nt1_ms2_tw32_e3": _H2_FWD},
    "dgrad": {"k1s1_g2_w2x2_nt1_ms2_tw16_e3": _H2_DGRAD, "k1s1_g2_w2x2_nt1_ms2_tw32_e3": _H2_DGRAD},
}
TRAIN_UNREACHED = sorted(PLAN_UNREACHABLE["train"])
DGRAD_UNREACHED = sorted(PLAN_UNREACHABLE["dgrad"])


def _row_id(row):
    kind, (n, cin, cout, h, w, k, s), o, form = row
    return f"{form}-{kind}_n{n}_c{cin}-{cout}_{h}x{w}" + ("-" + o if o else "")


def _form(row, n=None):
    kind, shape, o, _ = row
    return pf.query("op", n or shape[0], *shape[1:], kind, **pf.opts(o))


def _family(form):
    """The instance families the options are rotated over: kernel size and stride + the runtime path."""
    path = [p for p in ("par", "sub", "flat") if form.endswith("_" + p)]
    return form[:4] + ("_" + path[0] if path else "")


# ---- host tests (no GPU) ----
def test_p2_form_mirror_matches_the_header():
    """_lib.P2Form restates struct mval_p2_form of include/mval_hip.h; the entry is declared as the other two form queries are."""
    from multi_view_active_learning_amd import _lib

    text = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    body = re.search(r"typedef struct mval_p2_form \{(.*?)\} mval_p2_form;", text, flags=re.S).group(1)
    fields = [name for line in body.split(";") if line.strip() for name in re.sub(r"^\s*int32_t", "", line).replace(" ", "").split(",")]
    assert fields == [name for name, _ in _lib.P2Form._fields_] and C.sizeof(_lib.P2Form) == 4 * len(fields)
    assert fields == ["ks", "s", "g", "wn", "wm", "nt", "ms", "tw", "rs", "epi", "ow", "k48", "inz", "bsum", "th", "tile_w", "flat", "in_sub", "parities",
                      "groups", "tiles_x", "tiles_y", "tiles_total", "smem_bytes", "threads"]
    assert re.search(r"int mval_conv_p2_form\(int use, const mval_op\* op, int n_images, mval_p2_form\* form\);", text)


def test_the_query_answers_like_the_support_predicate_and_needs_no_gpu():
    """mval_conv_p2_form(USE_OP) answers exactly where mval_op_algo_supported(MVAL_ALGO_MFMA_P2) does; what the struct holds, on one launch of
    each path; the parity use has no P2 form; the data gradient only for stride 1; the in_z form is asked for with res1_off = -2."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    lib = _lib.lib()
    seen = set()
    for k, s, cin, cout, h, w, up, nchw in [(3, 1, 32, 32, 16, 16, 0, 0), (3, 1, 12, 32, 16, 16, 0, 0), (3, 1, 32, 20, 16, 16, 0, 0), (3, 1, 32, 19, 16, 16, 0, 1),
                                            (1, 1, 32, 19, 16, 16, 0, 1), (1, 1, 32, 32, 2, 8, 0, 0), (3, 1, 32, 32, 3, 16, 0, 0), (3, 1, 32, 32, 16, 16, 1, 0),
                                            (1, 2, 32, 40, 9, 9, 2, 0), (3, 2, 32, 40, 6, 9, 0, 0), (1, 1, 64, 256, 64, 64, 0, 1)]:
        for n in (1, 3, 8):
            pad = k // 2
            ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
            op = _query_op(pf.OP_CONV, k, s, pad, cin, cout, h, w, ho, wo, up=up, out_nchw=nchw, res1_off=-1, res2_off=-1, in_amax_off=1, out_amax_off=1)
            ok = bool(lib.mval_op_algo_supported(C.byref(op), C.c_int(n), C.c_int(pf.ALGO_P2)))
            assert (_lib.conv_p2_form(_lib.SPLIT_USE_OP, op, n) is not None) == ok, (k, s, cin, cout, h, w, up, nchw, n)
            assert _lib.conv_p2_form(_lib.SPLIT_USE_DGRAD_PARITY, op, n) is None and _lib.conv_p2_form(7, op, n) is None
            seen.add(ok)
    assert seen == {True, False}
    f = pf.query("op", 3, 64, 40, 33, 37, 3, 1, res1=True)
    assert f.as_dict() == dict(ks=3, s=1, g=1, wn=4, wm=1, nt=1, ms=4, tw=16, rs=1, epi=0, ow=0, k48=0, inz=0, bsum=0, th=4, tile_w=16, flat=0, in_sub=0,
                               parities=1, groups=1, tiles_x=3, tiles_y=9, tiles_total=81, smem_bytes=2 * 8 * 1 * 112 * 16 + 16, threads=256)
    f = pf.query("op", 8, 32, 256, 64, 64, 1, 1, up=1)  # (the issue's example: NT = 2 from 1024 tile groups on)
    assert (pf.name(f), f.groups, f.tiles_total) == ("k1s1_g2_w4x1_nt2_ms4_tw64_e1", 2, 8 * 64) and pf.query("op", 7, 32, 256, 64, 64, 1, 1, up=1).nt == 1
    f = pf.query("op", 2, 32, 40, 12, 16, 1, 1)  # (12 x 16 = 192 pixels as one row: 3 tiles of 64 per image)
    assert (pf.name(f), f.th, f.tile_w, f.tiles_x, f.tiles_y, f.tiles_total) == ("k1s1_g2_w4x1_nt1_ms4_tw64_e0_flat", 1, 64, 3, 1, 6)
    # (the tile width of a flattened map is still the one that pads the fewest columns: 12 x 18 = 216 pixels take 27 tiles of 8 columns, and
    # of each tile's 8 rows the one-row map fills one)
    f = pf.query("op", 2, 32, 40, 12, 18, 1, 1)
    assert (pf.name(f), f.th, f.tile_w, f.tiles_x, f.tiles_y) == ("k1s1_g2_w4x1_nt1_ms4_tw8_e0_flat", 8, 8, 27, 1)
    f = pf.query("op", 2, 64, 40, 17, 24, 1, 2)
    assert (pf.name(f), f.in_sub, f.tiles_x, f.tiles_y) == ("k1s1_g2_w4x1_nt1_ms4_tw8_e0_sub", 1, 2, 2)
    f = pf.query("op", 2, 64, 40, 8, 6, 4, 2, "deconv", relu=True)
    assert (pf.name(f), f.parities, f.th, f.tile_w, f.tiles_total) == ("k2s1_g2_w4x1_nt1_ms3_ow6_e0_par", 4, 8, 6, 2)
    assert pf.query("op", 2, 64, 40, 8, 6, 4, 2, "deconv", res1=True) is None  # (the parity conv takes no residual)
    t = pf.query("train", 2, 64, 64, 16, 16, 3, 1)
    z = pf.query("train", 2, 64, 64, 16, 16, 3, 1, inz=True)
    assert (pf.name(t), pf.name(z)) == ("k3s1_g1_w4x1_nt1_ms4_tw16_e3_rs", "k3s1_g1_w4x1_nt1_ms4_tw16_e3_rs_inz")
    assert pf.query("train", 2, 48, 64, 16, 16, 3, 1, inz=True) is None and pf.query("train", 2, 32, 32, 8, 6, 4, 2, "deconv") is None
    d = pf.query("dgrad", 2, 40, 64, 16, 16, 3, 1, res1=True)  # (the gradient's conv: 64 -> 40 channels)
    assert (pf.name(d), d.groups) == ("k3s1_g1_w4x1_nt1_ms4_tw16_e3_rs", 1) and pf.query("dgrad", 2, 40, 64, 16, 16, 3, 2) is None


def test_every_row_takes_the_form_it_is_in_the_table_for():
    bad = [(_row_id(r), f and pf.name(f)) for r in OP_CASES + LATE_CASES for f in [_form(r)] if f is None or pf.name(f) != r[3]]
    assert not bad, bad
    ids = [_row_id(r) for r in OP_CASES + LATE_CASES]
    assert len(set(ids)) == len(ids)


def test_the_table_names_every_form_the_sweep_finds():
    """Coverage and drift: the forms the sweep finds for mval_op_launch (tests/p2_forms.py: the documented domain, one pass of host
    arithmetic) are exactly the forms of the table, one row each.  A re-tuned threshold that creates a form without a row, a new instance,
    or a row whose form no shape reaches any more fails here.  Found on this dispatch: 109 forms -- 81 of the 1x1 conv (29 plain, 20 flattened,
    32 over every second pixel), 16 of 3x3 stride 1, 4 of 3x3 stride 2, 8 parity convs -- on 60 kernel instances."""
    found = pf.sweep("op")
    table = [r[3] for r in OP_CASES]
    print(f"[p2 forms] op: {len(found)} forms; " + ", ".join(f"{fam} {sum(_family(k) == fam for k in found)}" for fam in sorted({_family(k) for k in found})))
    missing, stale = set(found) - set(table), set(table) - set(found)
    assert not missing, f"forms without a row: {sorted(missing)}"
    assert not stale, f"rows whose form the sweep no longer finds: {sorted(stale)}"
    assert len(table) == len(set(table)) == len(found) == 109
    instance = lambda k: re.sub(r"_(flat|sub|par)$", "", k)
    assert len({instance(k) for k in found}) == 60
    assert {r[3] for r in LATE_CASES} <= set(found)
    assert (len(pf.sweep("train")), len(pf.sweep("dgrad"))) == (48, 32)


def test_rows_carry_the_edges_they_were_chosen_for():
    """Every row is a shape of the sweep; it has at least two images, and each of: a ragged last tile in rows, in columns, a partly empty last
    cout sub-tile, a tile count that is no multiple of 8 -- unless no shape of the sweep that reaches the form has it together with the ones
    before it.  Over every family's rows the options the table rotates all occur."""
    found = pf.sweep("op")
    bad = []
    for row in OP_CASES:
        kind, shape, o, form = row
        f = _form(row)
        cands = [(c[0], c[1], pf.query("op", *c[1], c[0], **pf.opts(c[2]))) for c in found[form]]
        if not any((c[0], c[1]) == (kind, shape) for c in cands):
            bad.append((form, "not a shape of the sweep"))
        me = (kind, shape, f)
        preds = [lambda c: c[1][0] >= 2, lambda c: c[1][1] == shape[1], lambda c: (c[1][2] == 19) if c[2].epi == 2 else c[1][2] % 16 == 8,
                 lambda c: pf.ragged("op", c[0], c[1], c[2])[0], lambda c: pf.ragged("op", c[0], c[1], c[2])[1], lambda c: c[2].tiles_total % 8 != 0]
        for i, p in enumerate(preds):  # (each edge in turn, among the shapes that have the ones before it and the row's cin)
            keep = [c for c in cands if p(c)]
            if keep:
                cands = keep
                if not p(me):
                    bad.append((form, shape, "edge", i))
    assert not bad, bad
    for fam in sorted({_family(r[3]) for r in OP_CASES}):
        rows = [r for r in OP_CASES if _family(r[3]) == fam]
        eps = {"+".join(t for t in r[2].split("+") if t in ("relu", "res1", "res2")) for r in rows}
        want = {"relu", ""} if fam.endswith("par") else {"relu", "res1", "res1+res2", ""}
        assert want <= eps, (fam, eps)
        assert any("mag" in r[2] for r in rows) and any(r[1][1] % 32 == 8 for r in rows), fam
        g2 = [r for r in rows if _form(r).g == 2]
        assert not g2 or any(r[1][1] in (72, 96) for r in g2), fam
    assert {pf.opts(r[2])["up"] for r in OP_CASES} == {0, 1, 2, 3} and any(r[1][2] == 19 for r in OP_CASES)


def test_forms_the_older_case_tables_reach():
    """The single-op cases that predate this suite (test_gpu_p2.py: P2_CASES, the transposed-conv and the stride-2 1x1 cases), held to the
    query: how many of the forms of mval_op_launch they reach."""
    import test_gpu_p2 as tp

    reached = set()
    for n, cin, cout, h, w, k, s, relu, r1, r2, up, nchw in tp.P2_CASES:
        reached.add(pf.name(pf.query("op", n, cin, cout, h, w, k, s, relu=relu, res1=r1, res2=r2, up=up, nchw=nchw)))
    cases_of = lambda fn: next(m.args[1] for m in fn.pytestmark if m.name == "parametrize")
    for n, cin, cout, h, w, relu in cases_of(tp.test_p2_transposed_conv_vs_float64):
        reached.add(pf.name(pf.query("op", n, cin, cout, h, w, 4, 2, "deconv", relu=relu)))
    for n, cin, cout, h, w in cases_of(tp.test_p2_conv1x1_stride2_vs_float64):
        reached.add(pf.name(pf.query("op", n, cin, cout, h, w, 1, 2)))
    print(f"[p2 forms] test_gpu_p2.py reaches {len(reached)} of {len(pf.sweep('op'))} forms: {sorted(reached)}")
    assert reached <= set(pf.sweep("op"))
    assert len(reached) == OLDER_REACH
    assert not any("_nt2_" in k and k.startswith("k1") for k in reached), "no single-op case ran the 1x1 conv with two cout sub-tiles per wave"


def _small_graph_forms(cases=None):
    """The forms of the training forward and of the data gradient that the default plans of tests/test_train_small_graphs.py's cases (all of
    CASES and LINEAR_CASES, or `cases`) run, read off each plan's ops."""
    import test_train_small_graphs as tsg
    from multi_view_active_learning_amd import engine_train as et

    reached = {"train": set(), "dgrad": set()}
    for case in (list(tsg.CASES.values()) + list(tsg.LINEAR_CASES.values()) if cases is None else cases):
        plan = tsg._host_plan(case, "default")
        for i, (op, t) in enumerate(zip(plan.graph.ops, plan.ops)):
            hin, win = plan.geo[i][:2]
            if t.fwd_p2:
                reached["train"].add(pf.name(pf.query("train", case["n"], op.cin, op.cout, hin, win, op.k, op.stride, inz=bool(t.zin_rel))))
            if t.p2_flags & et.TRAIN_DGRAD_P2:  # (a launch that also keeps the BatchNorm backward's sums runs the BSUM twin of the form: its own suite)
                reached["dgrad"].add(pf.name(pf.query("dgrad", case["n"], op.cin, op.cout, hin, win, op.k, op.stride, res1=not (t.first_touch & 1))))
    return reached


def test_training_forms_census():
    """The two training uses: the forms the sweep finds for mval_train_forward's convs (48, 3 of them the in_z instances) and for the data
    gradients mval_train_backward runs on these kernels (32), against those the small training graphs reach: 46 and 30 -- 22 and 13 by the
    graphs of blocks and by the first single-conv cases, 18 and 12 more by the single-conv cases chosen per form, 6 and 5 (the `nt2` forms of
    the 1x1 conv) by the ReLU-free cases of 16 images.  The rest is held equal to TRAIN_UNREACHED / DGRAD_UNREACHED, which are the forms no
    training plan reaches (PLAN_UNREACHABLE, two per use): a form that appears without a case, or a case that stops reaching its form, fails here."""
    reached = _small_graph_forms()
    for use, gap in (("train", TRAIN_UNREACHED), ("dgrad", DGRAD_UNREACHED)):
        found = set(pf.sweep(use))
        print(f"[p2 forms] {use}: {len(found)} forms, the small graphs reach {len(reached[use])}")
        assert reached[use] <= found, (use, sorted(reached[use] - found))
        assert sorted(found - reached[use]) == sorted(gap), (use, sorted(found - reached[use] - set(gap)), sorted(set(gap) - (found - reached[use])))
        assert sorted(gap) == sorted(PLAN_UNREACHABLE[use]) and len(gap) == 2
    assert (len(pf.sweep("train")), len(pf.sweep("dgrad"))) == (48, 32) and (len(reached["train"]), len(reached["dgrad"])) == (46, 30)


def _single_plan_forms(shape):
    """(training forward, data gradient) form names of conv "c" in the default plan of tiny_graphs.single at a sweep shape (None: no P2 launch)."""
    import test_train_small_graphs as tsg

    n, cin, cout, h, w, k, s = shape
    case = dict(graph="single", args=(cin, cout, k, s), n=n, hw=(h, w), seed=1)
    return tuple(f and pf.name(f) for f in tsg._c_forms(case, tsg._host_plan(case, "default")))


def test_no_plan_reaches_the_forms_left_out():
    """PLAN_UNREACHABLE: EVERY shape of the sweep that the dispatch answers with one of these forms, put behind the head as the conv of
    tiny_graphs.single, gets a default plan that runs conv c (for `dgrad`: its data gradient) on another kernel family -- and for the reason written
    down: the library's P2 query accepts the conv, its fp16-split query (what _choose_algorithms asks before a P2 pass may take the op) does not."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    lib = _lib.lib()
    for use, forms in PLAN_UNREACHABLE.items():
        for form in forms:
            cands = pf.sweep(use)[form]
            assert len(cands) >= 40 and {c[0] for c in cands} == {"conv"}
            for kind, shape, o, _ in cands:
                n, cin, cout, h, w, k, s = shape
                assert (k, s) == (1, 1) and h <= 2 and h * w < 64 and (cin if use == "dgrad" else cout) <= 32, shape
                got = _single_plan_forms(shape)[use == "dgrad"]
                assert got is None, (use, form, shape, got)
                d = _query_op(0, 1, 1, 0, cin, cout, h, w, h, w) if use == "train" else _query_op(0, 1, 1, 0, cout, cin, h, w, h, w)
                ok = lambda algo: bool(lib.mval_op_algo_supported(C.byref(d), C.c_int(n), C.c_int(algo)))
                assert ok(pf.ALGO_P2) and not ok(3), (use, form, shape)  # (3: MVAL_ALGO_MFMA_H2)


def _train_rows():
    """(use, form, shape, case) of the single-conv cases chosen per form: for every form that the graphs of blocks and the first single-conv
    cases (those without `forms`) do not reach, the first case of the table that names it."""
    import test_train_small_graphs as tsg

    seen = _small_graph_forms([c for c in tsg.CASES.values() if "forms" not in c])
    rows = []
    for cid, c in tsg.CASES.items():
        for use, form in zip(("train", "dgrad"), c.get("forms", (None, None))):
            if form is not None and form not in seen[use]:
                seen[use].add(form)
                rows.append((use, form, (c["n"],) + c["args"][:2] + c["hw"] + c["args"][2:], cid))
    return rows


def test_training_rows_carry_their_edges():
    """The single-conv cases chosen per form (tests/test_train_small_graphs.py, the cases with `forms`) as rows of the sweeps of the two
    training uses: each is a shape of its form's sweep whose plan takes the form, and it has, in this order, a ragged last tile in rows, in
    columns, a partly empty last cout sub-tile (the kernel's couts: the conv's cins for a data gradient), a tile count that is no multiple of 8
    -- unless no shape of the form's sweep WHOSE PLAN TAKES THE FORM (two or three images, the row's cin) has it together with the ones before.
    Over every family (1x1, flattened, over every second pixel, 3x3 stride 1 and 2) and use, each of the four edges occurs in some row unless
    no such shape of any of the family's rows has it."""
    rows = _train_rows()
    new = set(pf.sweep("train")) | set(pf.sweep("dgrad"))
    assert (sum(r[0] == "train" for r in rows), sum(r[0] == "dgrad" for r in rows)) == (18, 12) and all(form in new for _, form, _, _ in rows)
    kcout = lambda use, shape: shape[1] if use == "dgrad" else shape[2]
    edge = lambda use, shape: (lambda f: pf.ragged(use, "conv", shape, f) + (kcout(use, shape) % 16 == 8, f.tiles_total % 8 != 0))(pf.query(use, *shape))
    bad, have, could = [], {}, {}
    for use, form, shape, cid in rows:
        sweep = [c[1] for c in pf.sweep(use)[form] if c[0] == "conv" and "inz" not in c[2]]
        if shape not in sweep:
            bad.append((cid, use, "not a shape of the sweep"))
        cands = [c for c in sweep if c[0] >= 2 and c[1] == shape[1] and _single_plan_forms(c)[use == "dgrad"] == form]
        assert shape in cands, (cid, use)
        fam = (use, _family(form))
        me = edge(use, shape)
        for i in range(4):
            have.setdefault(fam, [False] * 4)[i] |= me[i]
            could.setdefault(fam, [False] * 4)[i] |= any(edge(use, c)[i] for c in cands)
        for i in range(4):  # (each edge in turn, among the shapes that have the ones before it)
            keep = [c for c in cands if edge(use, c)[i]]
            if keep:
                cands = keep
                if not me[i]:
                    bad.append((cid, use, form, "edge", i))
    assert not bad, bad
    assert {f for _, f in have} == {"k1s1", "k1s1_flat", "k1s1_sub", "k3s1", "k3s2"} and {u for u, _ in have} == {"train", "dgrad"}
    for fam in have:
        assert have[fam] == could[fam], (fam, have[fam], could[fam])
    print("[p2 forms] training rows, edges (rows, columns, cout sub-tile, tiles % 8) per family: " + "; ".join(f"{u} {f}: {''.join('x' if v else '-' for v in have[(u, f)])}"
                                                                                                               for u, f in sorted(have)))


def test_later_tile_rows_exceed_what_the_device_holds():
    """Every LATE_CASES row has more tile x group work items than workgroups can be resident on a device of up to CUS_SIZED_FOR compute units, an
    even batch (images 0 and 1 repeated), and between them the rows cover the families and the epilogues 0, 1 and 2."""
    assert len(LATE_CASES) <= 10
    for row in LATE_CASES:
        f = _form(row)
        assert f.tiles_total * f.groups > pf.resident_cap(f, CUS_SIZED_FOR) and row[1][0] % 2 == 0, _row_id(row)
    fams = {_family(r[3]) for r in LATE_CASES}
    assert {"k1s1", "k1s1_sub", "k3s1", "k3s2", "k2s1_par"} <= fams
    assert any("_rs" in r[3] for r in LATE_CASES) and any("_ow" in r[3] and r[3].startswith("k3s1") for r in LATE_CASES)
    assert {_form(r).epi for r in LATE_CASES} == {0, 1, 2}


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
    """test_gpu_p2._ref_conv with the transposed conv: the fused operator in the dtype of its arguments."""
    y = F.conv_transpose2d(x, w, None, stride=2, padding=1) if transposed else F.conv2d(x, w, None, stride=stride, padding=w.shape[-1] // 2)
    y = y * scale[None, :, None, None] + shift[None, :, None, None]
    if up:
        y = F.interpolate(y, scale_factor=2 ** up, mode="nearest")
    for r in (res1, res2):
        if r is not None:
            y = y + r
    return F.relu(y) if relu else y


def _inputs(row, n_distinct=None):
    """(x, wt, scale, shift, res1, res2) of a row, NCHW float32 on the CPU, as test_gpu_p2._make draws them (+ a random sign on the scale);
    `mag`: every image but the last scaled by 2^-10."""
    kind, (n, cin, cout, h, w, k, stride), o, _ = row
    n = n_distinct or n
    opt = pf.opts(o)
    transposed = kind == "deconv"
    rng = np.random.default_rng(zlib.crc32(_row_id(row).encode()))
    x = _f32(rng.standard_normal((n, cin, h, w)))
    mag = "mag" in o.split("+")
    if mag:
        assert n >= 2
        x[:-1] *= 2.0 ** -10
    taps = 4 if transposed else k * k  # (taps that meet one output pixel)
    wt = _f32(rng.standard_normal((cin, cout, k, k) if transposed else (cout, cin, k, k)) * np.sqrt(2.0 / (cin * taps)))
    scale = _f32(rng.uniform(0.5, 1.5, cout) * np.where(rng.random(cout) < 0.5, -1.0, 1.0))
    shift = _f32(rng.standard_normal(cout) * 0.1)
    ho, wo = (2 * h, 2 * w) if transposed else ((h - 1) // stride + 1, (w - 1) // stride + 1)
    ho, wo = ho << opt["up"], wo << opt["up"]
    res1 = _f32(rng.standard_normal((n, cout, ho, wo))) if opt["res1"] else None
    res2 = _f32(rng.standard_normal((n, cout, ho, wo))) if opt["res2"] else None
    for r in (res1, res2):  # (the image's residuals with it: their rows are per image too -- see the module's docstring)
        if mag and r is not None:
            r[:-1] *= 2.0 ** -10
    return x, wt, scale, shift, res1, res2


def _want64(row, t):
    kind, shape, o, _ = row
    opt = pf.opts(o)
    d = lambda v: None if v is None else v.double()
    x, wt, scale, shift, res1, res2 = t
    return _ref_conv(d(x), d(wt), d(scale), d(shift), shape[6], opt["relu"], d(res1), d(res2), opt["up"], kind == "deconv")


def _tolerance(row):
    """The bounds of the P2 conv's existing single-op tests: rtol 1e-4 with atol 2e-5, atol 3e-5 for the transposed conv and the stride-2 1x1."""
    kind, shape, _, _ = row
    return 1e-4, (3e-5 if kind == "deconv" or shape[5:] == (1, 2) else 2e-5)


def _assert_close(tag, got, want64, rtol, atol):
    """np.testing.assert_allclose(got, want64.float(), rtol, atol), in torch (the largest rows have 33 M elements); prints the figure first."""
    w = want64.float()
    err = (got - w).abs()
    excess = float((err - (atol + rtol * w.abs())).max())
    print(f"[p2 forms] {tag}: max |err| {float(err.max()):.3e}, max of |err| - (atol + rtol |want|) {excess:.3e}")
    assert torch.isfinite(got).all() and excess <= 0.0, (tag, float(err.max()), excess)


NAN_BITS = 0x7FC0DEAD  # a quiet NaN as float32, and a NaN in its upper fp16 half


def _launch_poisoned(c):
    """Fills the output region of the P2Conv `c` and the alignment padding behind it, up to the rows, with a NaN pattern, launches, and checks
    that every output element was written with a finite value (the planes themselves, or the fp32 maps), that the padding still holds the
    pattern and that the magnitude rows of the inputs behind it are untouched: a store past the map's last row or column lands there."""
    n, ho, wo, cout = c.shape
    numel, rows_at = n * ho * wo * cout, c.op.in_amax_off
    bits = c.arena.view(torch.int32)
    bits[c.out_off:rows_at] = NAN_BITS
    in_rows = bits[rows_at:c.op.out_amax_off].clone()
    c.launch()
    torch.cuda.synchronize()
    out = c.arena[c.out_off:c.out_off + numel]
    assert bool(torch.isfinite(out if c.out_nchw else out.view(torch.float16).float()).all()), "an output element was left unwritten or is not finite"
    assert bool((bits[c.out_off + numel:rows_at] == NAN_BITS).all()), "a store behind the output's last element"
    assert torch.equal(bits[rows_at:rows_at + in_rows.numel()], in_rows), "a store into the inputs' magnitude rows"


def _run_p2(row, t, dev, n=None):
    """The row's launch through ops.P2Conv on the first n images of the tensors t -> (NCHW result on the CPU, kept per-image maxima or None)."""
    from multi_view_active_learning_amd import ops

    kind, shape, o, _ = row
    opt = pf.opts(o)
    x, wt, scale, shift, res1, res2 = t
    nhwc = lambda v: None if v is None else v[:n].permute(0, 2, 3, 1).contiguous().to(dev)
    c = ops.P2Conv(nhwc(x), wt.to(dev), scale.to(dev), shift.to(dev), stride=shape[6], relu=opt["relu"], res1=nhwc(res1), res2=nhwc(res2), up=opt["up"],
                   out_nchw=opt["nchw"], transposed=kind == "deconv")
    _launch_poisoned(c)
    y = c.result()
    return (y.cpu() if opt["nchw"] else y.permute(0, 3, 1, 2).cpu()), (None if opt["nchw"] else c.kept_amax().cpu())


@gpu
@pytest.mark.parametrize("row", OP_CASES, ids=_row_id)
def test_p2_form_vs_float64(dev, row):
    """ops.P2Conv (mval_op_launch) on the row's form.  (1) elementwise against float64 at the bounds of test_gpu_p2.py (_tolerance); (2) P2
    outputs: the kept per-image max |x| equals the output's to rtol 2^-21; (3) where the exact-fp32 MFMA conv runs the same shape and the
    row has at least RMS_MIN_ELEMENTS output elements: rms <= 1.25 rms32 + 1e-8, over the batch and, with `mag`, per image; (4) the form, on the shape that ran; (5) poison: the output
    region and its padding filled with NaNs before the launch (_launch_poisoned); (6) image 0 alone gives image 0's bits, where a batch of
    one takes the same form (the 1x1 NT rule depends on the batch)."""
    from multi_view_active_learning_amd import ops

    kind, (n, cin, cout, h, w, k, stride), o, form = row
    opt = pf.opts(o)
    f = _form(row)
    assert f is not None and pf.name(f) == form, "the case must run on the form it is in the table for"
    t = _inputs(row)
    want64 = _want64(row, t)
    got, kept = _run_p2(row, t, dev)
    rtol, atol = _tolerance(row)
    _assert_close(_row_id(row), got, want64, rtol, atol)
    if kept is not None:
        assert torch.allclose(kept, got.abs().amax(dim=(1, 2, 3)), rtol=2.0 ** -21, atol=0), "kept per-image max |x|"
    if want64.numel() >= RMS_MIN_ELEMENTS and mf.query("op", n, cin, cout, h, w, k, stride, kind, **opt) is not None:
        x, wt, scale, shift, res1, res2 = t
        nhwc = lambda v: None if v is None else v.permute(0, 2, 3, 1).contiguous().to(dev)
        y = ops.fused_conv(nhwc(x), wt.to(dev), scale.to(dev), shift.to(dev), stride=stride, pad=1 if kind == "deconv" else None, relu=opt["relu"],
                           res1=nhwc(res1), res2=nhwc(res2), up=opt["up"], algo=mf.ALGO_MFMA, out_nchw=opt["nchw"],
                           kind=ops.OP_DECONV if kind == "deconv" else ops.OP_CONV)
        y = y.cpu() if opt["nchw"] else y.permute(0, 3, 1, 2).cpu()
        rms = lambda v: (v.double() - want64).pow(2).mean().sqrt().item()
        r, r32 = rms(got), rms(y)
        print(f"[p2 forms] {_row_id(row)}: rms {r:.3e}, exact fp32 {r32:.3e}")
        assert r <= 1.25 * r32 + 1e-8, (r, r32)
        if "mag" in o.split("+"):  # (per image: the small images' errors vanish in the batch's rms)
            for i in range(n):
                ri, r32i = ((v[i].double() - want64[i]).pow(2).mean().sqrt().item() for v in (got, y))
                assert ri <= 1.25 * r32i + 1e-8, ("image", i, ri, r32i)
    f1 = _form(row, n=1)
    if n > 1 and f1 is not None and pf.name(f1) == form:
        alone, _ = _run_p2(row, t, dev, n=1)
        assert _bits_equal(alone[0], got[0]), "image 0 alone has the same bits"


@gpu
@pytest.mark.parametrize("row", LATE_CASES, ids=_row_id)
def test_p2_later_tiles_of_a_workgroup(dev, row):
    """A batch of images 0 and 1 repeated, so large that some workgroup must walk two tiles or more (asserted from the device's compute units).
    Images 0 and 1 against float64 as in test_p2_form_vs_float64; every other image equals image i % 2 bit for bit, its kept maximum too: what
    a workgroup carries from tile to tile -- the LDS buffers, the prefetched next tile, the max |x| slots -- leaves no trace in the results."""
    kind, (n, cin, cout, h, w, k, stride), o, form = row
    f = _form(row)
    assert f is not None and pf.name(f) == form, "the case must run on the form it is in the table for"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r_max = pf.resident_cap(f, cus)
    assert f.tiles_total * f.groups > r_max, (f.tiles_total, f.groups, cus, r_max)
    two = _inputs(row, n_distinct=2)
    want64 = _want64(row, two)
    rep = lambda v: None if v is None else v.repeat(n // 2, 1, 1, 1)
    x, wt, scale, shift, res1, res2 = two
    got, kept = _run_p2(row, (rep(x), wt, scale, shift, rep(res1), rep(res2)), dev)
    rtol, atol = _tolerance(row)
    _assert_close(_row_id(row), got[:2], want64, rtol, atol)
    pairs = got.reshape(n // 2, 2, *got.shape[1:])
    assert _bits_equal(pairs, pairs[:1].expand_as(pairs).contiguous()), "image i differs from image i % 2"
    if kept is not None:
        assert torch.allclose(kept[:2], got[:2].abs().amax(dim=(1, 2, 3)), rtol=2.0 ** -21, atol=0)
        assert _bits_equal(kept.reshape(n // 2, 2), kept[:2].reshape(1, 2).expand(n // 2, 2).contiguous()), "kept maximum of image i differs from image i % 2's"

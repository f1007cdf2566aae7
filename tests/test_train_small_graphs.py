"""Each training conv and gradient path alone, on graphs of a few ops (tests/tiny_graphs.py) at shapes the networks never produce, against
float64 autograd.  The whole-network training tests must tolerate ReLU-mask flips (gradients at 2e-3, error distributions against an fp32
floor + 1e-3); here the inputs are made (on the float64 reference alone: golden/make_small_graph_inputs.py) so that NO mask can flip within fp32's own error, and every parameter
gradient is held to  e <= F * floor + 2e-5  per tensor (e: relative L2 against float64; floor: torch-CPU float32's; F = 2 for the exact-operand
plans, 4 for the fp16-split plan, 4 * 2^b for the default plan whose P2 scales sit b bits above the activations' maxima).

The host test builds every case's four plans on torch.device("cpu") and asserts from plan.ops that the case reaches the paths it is in the
table for; the GPU test repeats those assertions on the plan it ran, so no case passes by falling back to another kernel -- and since the
TRAIN_BSUM flag is only a request (a data gradient without room for its partials runs the plain form), it also asserts from
mval_train_bsum_launches that every flagged launch kept the sums.  The BatchNorm-in-conv halves (the 3x3 P2 conv that applies its
producer's BatchNorm while staging, the data gradient that keeps the BatchNorm backward's sums) are reached at each of their three tile
forms and edges, and compared with the separate passes on the same graphs.

The P2 conv's two training uses (conv_p2_kernel with EPI == 3: raw z as fp32 NHWC + the BatchNorm partials kept over the workgroup's tile
walk; the data gradient that adds to its slot) are reached at every form a training plan can take (tests/test_gpu_p2_forms.py holds the
census): by one conv behind the head per form on stored inputs, and -- where the form needs more pixels than the margin method can move off
zero -- by the same graph without its ReLUs (LINEAR_CASES), whose raw z is also compared per image."""
import functools
import os

import numpy as np
import pytest
import torch

import tiny_graphs as tg

ALGO_DIRECT, ALGO_MFMA, ALGO_MFMA_BF3, ALGO_MFMA_H2 = 0, 1, 2, 3

# graph, builder arguments (channel widths [, stride]), images, map size behind the stride-2 head (the input is twice that), seed of the
# parameters (and of the Gaussian batch the stored input was made from).  `inz`: the 3x3 P2 convs of this shape apply their producer's BatchNorm while staging (mval_conv_p2_inz_supported);
# `bsum`: their data gradients keep the BatchNorm backward's sums (mval_conv_p2_bsum_supported, which also admits 48 and 96 channels).  Weight-gradient tiles (tiny_graphs.wgrad_tile): 16 wide on the 16-, 12- and 9-wide
# maps (16-wide tiles pad no more columns there), 8 wide on 18 / 24 / 37 / 6 / 8; NT = 2 for cout > 32; the 4 x 6 maps are smaller than a tile and
# give 3 tiles (< PS).
CASES = {
    "blocks_c32_16x16": dict(graph="blocks", args=(32,), n=2, hw=(16, 16), seed=1, inz=True, bsum=True),
    "blocks_c48_12x18": dict(graph="blocks", args=(48,), n=2, hw=(12, 18), seed=1, inz=False, bsum=False),
    "blocks_c64_8x24": dict(graph="blocks", args=(64,), n=2, hw=(8, 24), seed=1, inz=False, bsum=False),
    "blocks_c32_21x37": dict(graph="blocks", args=(32,), n=2, hw=(21, 37), seed=1, inz=False, bsum=False),
    "blocks_c64_4x6_n3": dict(graph="blocks", args=(64,), n=3, hw=(4, 6), seed=1, inz=False, bsum=False),
    "bneck_s1_16x16": dict(graph="bneck", args=(64, 64, 1), n=2, hw=(16, 16), seed=1, inz=True, bsum=True),
    "bneck_s2_16x16": dict(graph="bneck", args=(64, 64, 2), n=2, hw=(16, 16), seed=1, inz=False, bsum=False),
    "bneck_s1_12x18": dict(graph="bneck", args=(64, 64, 1), n=2, hw=(12, 18), seed=1, inz=False, bsum=False),
    "fuse_32_64_96_16x16": dict(graph="fuse", args=(32, 64, 96), n=2, hw=(16, 16), seed=1, inz=False, bsum=False),
    "fuse_48_96_64_8x24": dict(graph="fuse", args=(48, 96, 64), n=2, hw=(8, 24), seed=1, inz=False, bsum=False),
    "deconv_64_64_32_16x16": dict(graph="deconv", args=(64, 64, 32), n=2, hw=(16, 16), seed=1, inz=False, bsum=False),
    "deconv_64_96_48_12x18": dict(graph="deconv", args=(64, 96, 48), n=2, hw=(12, 18), seed=1, inz=False, bsum=False),
    # the BatchNorm-in-conv halves (INZ: the staging of a 3x3 P2 conv; BSUM: the epilogue of its data gradient) at every tile form and edge
    # form A (W % 16 == 0, H >= 4, <= 2 cout sub-tiles: 8-row x 16-column tiles, WM = 2): a map lower than a tile; a ragged last tile row
    # (8 + 4), two tile columns, odd batch; behind a 1x1 producer (mask from z)
    "blocks_c32_4x16": dict(graph="blocks", args=(32,), n=2, hw=(4, 16), seed=1, inz=True, bsum=True),
    "blocks_c32_12x32": dict(graph="blocks", args=(32,), n=3, hw=(12, 32), seed=1, inz=True, bsum=True),
    "bneck_p32_16x16": dict(graph="bneck", args=(64, 32, 1), n=2, hw=(16, 16), seed=1, inz=True, bsum=True),
    # form B (> 2 cout sub-tiles: 4-row tiles, 4 cout waves): residual + mask bytes; ragged (4 + 2), two columns, odd batch; BSUM alone with 3
    # sub-tiles (one wave idle; INZ needs Cin % 32 == 0); 6 sub-tiles = two cout groups, the second half empty, INZ over three chunks
    "blocks_c64_16x16": dict(graph="blocks", args=(64,), n=2, hw=(16, 16), seed=1, inz=True, bsum=True),
    "blocks_c64_6x32": dict(graph="blocks", args=(64,), n=3, hw=(6, 32), seed=1, inz=True, bsum=True),
    "blocks_c48_16x16": dict(graph="blocks", args=(48,), n=2, hw=(16, 16), seed=1, inz=False, bsum=True),
    "blocks_c96_8x16": dict(graph="blocks", args=(96,), n=2, hw=(8, 16), seed=1, inz=True, bsum=True),
    # form C (8 x 8 maps, G = 2): one tile per image; odd count; BSUM alone (96 % 64 != 0: partial second chunk, two cout groups); two full
    # chunks and groups; behind a 1x1 producer; and the boundary: 8 x 8 with two sub-tiles takes neither path
    "blocks_c64_8x8": dict(graph="blocks", args=(64,), n=2, hw=(8, 8), seed=1, inz=True, bsum=True),
    "blocks_c64_8x8_n5": dict(graph="blocks", args=(64,), n=5, hw=(8, 8), seed=1, inz=True, bsum=True),
    "blocks_c96_8x8": dict(graph="blocks", args=(96,), n=2, hw=(8, 8), seed=1, inz=False, bsum=True),
    "blocks_c128_8x8": dict(graph="blocks", args=(128,), n=2, hw=(8, 8), seed=1, inz=True, bsum=True),
    "bneck_p64_8x8": dict(graph="bneck", args=(64, 64, 1), n=2, hw=(8, 8), seed=1, inz=True, bsum=True),
    "blocks_c32_8x8": dict(graph="blocks", args=(32,), n=2, hw=(8, 8), seed=1, inz=False, bsum=False),
    # two lanes keep partials in their own scratch slices at once (form A on lane 0, form C on lane 1)
    "branches_32_64_16x16": dict(graph="branches", args=(32, 64), n=2, hw=(16, 16), seed=1, inz=True, bsum=True),
    # the pre-summed apply pass ACCUMULATES into the residual's gradient slot (b0.conv2 is not its first writer), forms A and C
    "shared_c32_16x16": dict(graph="shared", args=(32,), n=2, hw=(16, 16), seed=1, inz=True, bsum=True),
    "shared_c64_8x8": dict(graph="shared", args=(64,), n=2, hw=(8, 8), seed=1, inz=True, bsum=True),
    # one conv behind the head (tiny_graphs.single) at the P2 conv's forms that no graph above reaches (tests/test_gpu_p2_forms.py holds the census):
    # a 1x1 conv whose 8 x 10 map runs as one flattened row of 16-wide tiles, and its data gradient; the stride-2 1x1 over every second pixel on
    # 16-wide tiles; 3x3 on the whole 12 x 9 map per tile and on 8 x 6-pixel odd tiles (forward and data gradient), on 7 x 9-pixel odd tiles;
    # 3x3 stride 2 at 32 couts
    "single_k1_64_64_8x10": dict(graph="single", args=(64, 64, 1, 1), n=2, hw=(8, 10), seed=1, inz=False, bsum=False),
    "single_k1s2_64_64_16x32": dict(graph="single", args=(64, 64, 1, 2), n=2, hw=(16, 32), seed=1, inz=False, bsum=False),
    "single_k3_64_64_12x9": dict(graph="single", args=(64, 64, 3, 1), n=2, hw=(12, 9), seed=1, inz=False, bsum=False),
    "single_k3_64_64_8x6_n3": dict(graph="single", args=(64, 64, 3, 1), n=3, hw=(8, 6), seed=1, inz=False, bsum=False),
    "single_k3_64_64_7x9": dict(graph="single", args=(64, 64, 3, 1), n=2, hw=(7, 9), seed=1, inz=False, bsum=False),
    "single_k3s2_32_32_16x16": dict(graph="single", args=(32, 32, 3, 2), n=2, hw=(16, 16), seed=1, inz=False, bsum=False),
    # one conv behind the head at every remaining form of the training forward (`T`) and of the data gradient (`D`) that a plan of two or three
    # images can reach (tests/test_gpu_p2_forms.py: test_training_forms_census): per form the cheapest shape of p2_forms.sweep whose default plan
    # takes it with a ragged last tile in rows and in columns where the form admits one (a flattened map has columns only; 64-wide tiles and
    # the odd-tile 3x3 forms take whole tiles only) and a tile count that is no multiple of 8; three images on maps of up to 120 pixels, two on
    # the larger ones (the stored inputs are 48 bytes per image and map pixel, and the fixture file has to stay under 1 MiB).  A cout of 8 mod
    # 16 leaves the P2 path on every 1x1 form (the fp16-split 1x1 conv, which the plan asks first, takes whole 16-cout sub-tiles only) and the
    # three-sub-tiles-per-wave 3x3 forms need 96 or 192 couts; 3x3 stride 2 keeps the path at 40.  `forms`: what conv "c" runs on in the
    # default plan, (training forward, data gradient; None: no P2 launch), asserted by _check_plan.  The 32 -> 32, 48 -> 48 and 96 -> 96 rows
    # reach the same-named form in both uses.
    # 1x1 on <= 2 cout sub-tiles (2 x 2 waves): flattened on 16-, 32- and 8-wide tiles, 64-wide tiles, 5 x 7 on one ragged 8 x 8 tile
    "single_k1_32_32_13x6_n3": dict(graph="single", args=(32, 32, 1, 1), n=3, hw=(13, 6), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w2x2_nt1_ms2_tw16_e3_flat", "k1s1_g2_w2x2_nt1_ms2_tw16_e3_flat")),
    "single_k1_32_32_5x18_n3": dict(graph="single", args=(32, 32, 1, 1), n=3, hw=(5, 18), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w2x2_nt1_ms2_tw32_e3_flat", "k1s1_g2_w2x2_nt1_ms2_tw32_e3_flat")),
    "single_k1_32_32_5x64": dict(graph="single", args=(32, 32, 1, 1), n=2, hw=(5, 64), seed=1, inz=False, bsum=False,
                                 forms=("k1s1_g2_w2x2_nt1_ms2_tw64_e3", "k1s1_g2_w2x2_nt1_ms2_tw64_e3")),
    "single_k1_32_32_5x7_n3": dict(graph="single", args=(32, 32, 1, 1), n=3, hw=(5, 7), seed=1, inz=False, bsum=False,
                                   forms=("k1s1_g2_w2x2_nt1_ms2_tw8_e3", "k1s1_g2_w2x2_nt1_ms2_tw8_e3")),
    "single_k1_32_32_5x13_n3": dict(graph="single", args=(32, 32, 1, 1), n=3, hw=(5, 13), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w2x2_nt1_ms2_tw8_e3_flat", "k1s1_g2_w2x2_nt1_ms2_tw8_e3_flat")),
    # ... over every second pixel (stride 2; its data gradient is no P2 form)
    "single_k1s2_32_32_5x32": dict(graph="single", args=(32, 32, 1, 2), n=2, hw=(5, 32), seed=1, inz=False, bsum=False,
                                   forms=("k1s1_g2_w2x2_nt1_ms2_tw16_e3_sub", None)),
    "single_k1s2_32_32_5x64": dict(graph="single", args=(32, 32, 1, 2), n=2, hw=(5, 64), seed=1, inz=False, bsum=False,
                                   forms=("k1s1_g2_w2x2_nt1_ms2_tw32_e3_sub", None)),
    "single_k1s2_32_32_5x128": dict(graph="single", args=(32, 32, 1, 2), n=2, hw=(5, 128), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w2x2_nt1_ms2_tw64_e3_sub", None)),
    "single_k1s2_32_32_13x9_n3": dict(graph="single", args=(32, 32, 1, 2), n=3, hw=(13, 9), seed=1, inz=False, bsum=False,
                                      forms=("k1s1_g2_w2x2_nt1_ms2_tw8_e3_sub", None)),
    # 1x1 on three cout sub-tiles (4 x 1 waves, one idle): the two-row and one-row maps that are NOT flattened, flattened, 64-wide tiles
    "single_k1_48_48_2x16_n3": dict(graph="single", args=(48, 48, 1, 1), n=3, hw=(2, 16), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w4x1_nt1_ms4_tw16_e3", "k1s1_g2_w4x1_nt1_ms4_tw16_e3")),
    "single_k1_48_48_1x32_n3": dict(graph="single", args=(48, 48, 1, 1), n=3, hw=(1, 32), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w4x1_nt1_ms4_tw32_e3", "k1s1_g2_w4x1_nt1_ms4_tw32_e3")),
    "single_k1_48_48_5x18_n3": dict(graph="single", args=(48, 48, 1, 1), n=3, hw=(5, 18), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w4x1_nt1_ms4_tw32_e3_flat", "k1s1_g2_w4x1_nt1_ms4_tw32_e3_flat")),
    "single_k1_48_48_5x64": dict(graph="single", args=(48, 48, 1, 1), n=2, hw=(5, 64), seed=1, inz=False, bsum=False,
                                 forms=("k1s1_g2_w4x1_nt1_ms4_tw64_e3", "k1s1_g2_w4x1_nt1_ms4_tw64_e3")),
    "single_k1s2_32_48_5x64": dict(graph="single", args=(32, 48, 1, 2), n=2, hw=(5, 64), seed=1, inz=False, bsum=False,
                                   forms=("k1s1_g2_w4x1_nt1_ms4_tw32_e3_sub", None)),
    "single_k1s2_32_48_4x128": dict(graph="single", args=(32, 48, 1, 2), n=2, hw=(4, 128), seed=1, inz=False, bsum=False,
                                    forms=("k1s1_g2_w4x1_nt1_ms4_tw64_e3_sub", None)),
    # (the data gradient of 48 -> 32 is the 32 -> 48 conv: three sub-tiles on a ragged 8 x 8 tile; its forward is the two-sub-tile form of 5x7 above)
    "single_k1_48_32_5x7_n3": dict(graph="single", args=(48, 32, 1, 1), n=3, hw=(5, 7), seed=1, inz=False, bsum=False,
                                   forms=("k1s1_g2_w2x2_nt1_ms2_tw8_e3", "k1s1_g2_w4x1_nt1_ms4_tw8_e3")),
    # 3x3 on odd tiles with three cout sub-tiles per wave (96 and 192 couts: 12- and 6-wide tiles), forward and data gradient (whose couts are
    # the conv's cins); 3x3 stride 2 on 6-wide odd tiles with a partly empty third sub-tile
    "single_k3_96_96_8x36": dict(graph="single", args=(96, 96, 3, 1), n=2, hw=(8, 36), seed=1, inz=False, bsum=False,
                                 forms=("k3s1_g1_w2x2_nt3_ms3_ow12_e3", "k3s1_g1_w2x2_nt3_ms3_ow12_e3")),
    "single_k3_32_192_8x18": dict(graph="single", args=(32, 192, 3, 1), n=2, hw=(8, 18), seed=1, inz=False, bsum=False,
                                  forms=("k3s1_g1_w4x1_nt3_ms3_ow6_e3", "k3s1_g1_w2x2_nt1_ms4_tw16_e3_rs")),
    "single_k3_192_32_8x18": dict(graph="single", args=(192, 32, 3, 1), n=2, hw=(8, 18), seed=1, inz=False, bsum=False,
                                  forms=("k3s1_g1_w2x2_nt1_ms4_tw16_e3_rs", "k3s1_g1_w4x1_nt3_ms3_ow6_e3")),
    "single_k3s2_32_40_16x12": dict(graph="single", args=(32, 40, 3, 2), n=2, hw=(16, 12), seed=1, inz=False, bsum=False,
                                    forms=("k3s2_g1_w4x1_nt1_ms3_ow6_e3", None)),
}
# ---- the shapes the margin method cannot serve: tiny_graphs.linear (no ReLU on the head or on "c": no mask exists), the seeded Gaussian batch drawn
# when the test runs, the default plan only.  `forms`: (training forward, data gradient) of conv "c", as above.
# The 1x1 conv with two cout sub-tiles per wave (`nt2`) starts at ceil(px / 64) * (cout / 128) >= 1024: 16 images of 2048 pixels or more and 256
# couts -- 32 -> 256 for the forward (plain, flattened on 64-, 16-, 32- and 8-wide tiles, over every second pixel), 256 -> 32 for the data
# gradient (whose couts are the conv's cins).  The flattened rows of 2640, 2400 and 2376 pixels have more tiles than the device holds
# workgroups (see below), so their partials cover two tiles and more.
_NT2 = "k1s1_g2_w4x1_nt2_ms4_"
_W22 = "k1s1_g2_w2x2_nt1_ms2_"
LINEAR_CASES = {
    "linear_k1_32_256_16x128": dict(graph="linear", args=(32, 256, 1, 1), n=16, hw=(16, 128), seed=1, forms=(_NT2 + "tw64_e3", _W22 + "tw64_e3")),
    "linear_k1_32_256_64x32": dict(graph="linear", args=(32, 256, 1, 1), n=16, hw=(64, 32), seed=1, forms=(_NT2 + "tw64_e3_flat", _W22 + "tw64_e3_flat")),
    "linear_k1_32_256_33x80": dict(graph="linear", args=(32, 256, 1, 1), n=16, hw=(33, 80), seed=1, forms=(_NT2 + "tw16_e3_flat", _W22 + "tw16_e3_flat")),
    "linear_k1_32_256_24x100": dict(graph="linear", args=(32, 256, 1, 1), n=16, hw=(24, 100), seed=1, forms=(_NT2 + "tw32_e3_flat", _W22 + "tw32_e3_flat")),
    "linear_k1_32_256_33x72": dict(graph="linear", args=(32, 256, 1, 1), n=16, hw=(33, 72), seed=1, forms=(_NT2 + "tw8_e3_flat", _W22 + "tw8_e3_flat")),
    "linear_k1s2_32_256_64x128": dict(graph="linear", args=(32, 256, 1, 2), n=16, hw=(64, 128), seed=1, forms=(_NT2 + "tw64_e3_sub", None)),
    "linear_k1_256_32_16x128": dict(graph="linear", args=(256, 32, 1, 1), n=16, hw=(16, 128), seed=1, forms=(_W22 + "tw64_e3", _NT2 + "tw64_e3")),
    "linear_k1_256_32_64x32": dict(graph="linear", args=(256, 32, 1, 1), n=16, hw=(64, 32), seed=1, forms=(_W22 + "tw64_e3_flat", _NT2 + "tw64_e3_flat")),
    "linear_k1_256_32_33x80": dict(graph="linear", args=(256, 32, 1, 1), n=16, hw=(33, 80), seed=1, forms=(_W22 + "tw16_e3_flat", _NT2 + "tw16_e3_flat")),
    "linear_k1_256_32_24x100": dict(graph="linear", args=(256, 32, 1, 1), n=16, hw=(24, 100), seed=1, forms=(_W22 + "tw32_e3_flat", _NT2 + "tw32_e3_flat")),
    "linear_k1_256_32_33x72": dict(graph="linear", args=(256, 32, 1, 1), n=16, hw=(33, 72), seed=1, forms=(_W22 + "tw8_e3_flat", _NT2 + "tw8_e3_flat")),
    # later tiles of a workgroup (`late`: the uses whose tiles_total * groups exceeds p2_forms.resident_cap at LATE_CUS compute units, so that some
    # workgroup walks a second tile with its (sum, sum of squares) registers, its prefetch and the NEXT image's scale): the shapes of
    # test_gpu_p2_forms.LATE_CASES as training convs -- 3x3 with row sharing at 32 and 40 couts, 1x1 on 64-wide tiles, 3x3 stride 2, the stride-2 1x1
    # over every second pixel, 18-wide odd tiles -- and an `nt2` row of 16 images.  `seq`: images of two kinds in the fixed pseudo-random order
    # of p2_fused.late_seq, A = the seeded image x 2^-10, B = as seeded, and head_bn.bias = 0 (on the reference and on the device model alike), so
    # that BatchNorm's shift does not erase the contrast at conv c's input: a scale kept from the tile walked before is 2^10 off.
    "linear_late_k3_32_32_9x20": dict(graph="linear", args=(32, 32, 3, 1), n=242, hw=(9, 20), seed=1, seq=True, late=("train", "dgrad"),
                                      forms=("k3s1_g1_w2x2_nt1_ms4_tw16_e3_rs", "k3s1_g1_w2x2_nt1_ms4_tw16_e3_rs")),
    "linear_late_k1_32_32_16x64": dict(graph="linear", args=(32, 32, 1, 1), n=82, hw=(16, 64), seed=1, seq=True, late=("train", "dgrad"),
                                       forms=(_W22 + "tw64_e3", _W22 + "tw64_e3")),
    "linear_late_k3_32_40_9x20": dict(graph="linear", args=(32, 40, 3, 1), n=268, hw=(9, 20), seed=1, seq=True, late=("train",),
                                      forms=("k3s1_g1_w4x1_nt1_ms4_tw16_e3_rs", None)),
    "linear_late_k3s2_32_40_18x22": dict(graph="linear", args=(32, 40, 3, 2), n=162, hw=(18, 22), seed=1, seq=True, late=("train",),
                                         forms=("k3s2_g1_w4x1_nt1_ms2_tw8_e3", None)),
    "linear_late_k1s2_32_32_17x33": dict(graph="linear", args=(32, 32, 1, 2), n=214, hw=(17, 33), seed=1, seq=True, late=("train",),
                                         forms=(_W22 + "tw8_e3_sub", None)),
    "linear_late_k3_32_40_22x18": dict(graph="linear", args=(32, 40, 3, 1), n=202, hw=(22, 18), seed=1, seq=True, late=("train",),
                                       forms=("k3s1_g1_w4x1_nt1_ms4_ow18_e3", None)),
    "linear_late_k1_32_256_33x80": dict(graph="linear", args=(32, 256, 1, 1), n=16, hw=(33, 80), seed=2, seq=True, late=("train", "dgrad"),
                                        forms=(_NT2 + "tw16_e3_flat", _W22 + "tw16_e3_flat")),
}
LATE_CUS = 320  # (test_gpu_p2_forms.CUS_SIZED_FOR: the MI355X has 256 compute units)
LATE_CONTRAST = 2.0 ** -6  # at conv c's input: max |A image| <= 2^-6 max |B image| (the batch mean leaves an A image about 2^-7 of a B image)
PLANS = {"default": {}, "h2": {"MVAL_TRAIN_P2": "0"}, "bf3": {"MVAL_CONV": "bf3"}, "fp32": {"MVAL_CONV": "fp32"}}
MARGIN = 64.0
# the input batch of every case: seeded Gaussian values moved off the ReLUs' zeros on the float64 reference (golden/make_small_graph_inputs.py)
INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_graph_inputs.npz")


def _model(case):
    m = tg.TinyNet(tg.BUILDERS[case["graph"]], case["args"], case["seed"])
    if case.get("seq"):
        with torch.no_grad():
            m.head_bn.bias.zero_()
    return m


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    """(x, g, Reference) of a case: computed once, shared by the four plans' tests, never modified."""
    case = CASES[case_id]
    m = _model(case)
    x = torch.from_numpy(np.load(INPUTS)[case_id])
    assert tuple(x.shape) == (case["n"], 3, 2 * case["hw"][0], 2 * case["hw"][1]) and x.dtype == torch.float32
    from multi_view_active_learning_amd.engine import _geometry

    out_hw = _geometry(m._graph, x.shape[2], x.shape[3])[0][m._graph.output]
    g = torch.randn(case["n"], tg.OUT_CHANNELS, *out_hw, generator=torch.Generator().manual_seed(1000 + case["seed"]))
    return x, g, tg.Reference(m, x, g)


def _late_seq(case):
    """The image kinds of a `seq` case ("A": scaled 2^-10, "B": as seeded), None for the others."""
    if not case.get("seq"):
        return None
    import p2_fused

    return p2_fused.late_seq(case["n"])


def _linear_input(case):
    x = tg.seeded_input(case)
    seq = _late_seq(case)
    if seq:
        x = x * torch.tensor([2.0 ** -10 if k == "A" else 1.0 for k in seq]).reshape(-1, 1, 1, 1)
    return x


@functools.lru_cache(maxsize=1)
def _linear_reference(case_id):
    """(x, g, Reference) of a LINEAR_CASES row.  One at a time: a reference holds float64 tensors of up to 100 MB each."""
    case = LINEAR_CASES[case_id]
    m = _model(case)
    x = _linear_input(case)
    from multi_view_active_learning_amd.engine import _geometry

    out_hw = _geometry(m._graph, x.shape[2], x.shape[3])[0][m._graph.output]
    g = torch.randn(case["n"], tg.OUT_CHANNELS, *out_hw, generator=torch.Generator().manual_seed(1000 + case["seed"]))
    return x, g, tg.Reference(m, x, g)


def _conv_c(plan):
    """(index, graph op, plan op) of the conv named "c" of a single / linear graph."""
    i = next(i for i, op in enumerate(plan.graph.ops) if op.conv == "c")
    return i, plan.graph.ops[i], plan.ops[i]


def _c_forms(case, plan):
    """(training forward, data gradient) forms conv "c" runs on in a default plan, as test_gpu_p2_forms._small_graph_forms reads them; None: no P2 launch."""
    import p2_forms as pf
    from multi_view_active_learning_amd import engine_train as et

    i, op, t = _conv_c(plan)
    hin, win = plan.geo[i][:2]
    fwd = pf.query("train", case["n"], op.cin, op.cout, hin, win, op.k, op.stride, inz=bool(t.zin_rel)) if t.fwd_p2 else None
    dg = None
    if t.p2_flags & et.TRAIN_DGRAD_P2:
        dg = pf.query("dgrad", case["n"], op.cin, op.cout, hin, win, op.k, op.stride, res1=not (t.first_touch & 1))
    return fwd, dg


# ---- what every case must reach, read from plan.ops ----
def _check_plan(case, plan_name, plan):
    from multi_view_active_learning_amd import _lib, engine_train as et
    import ctypes as C

    g = plan.graph
    ops = {(op.conv or op.kind): (op, t) for op, t in zip(g.ops, plan.ops)}
    has = lambda name, bit: bool(ops[name][1].p2_flags & bit)
    p2_bits = (et.TRAIN_WGRAD_X_P2 | et.TRAIN_OUT_P2_ONLY | et.TRAIN_DGRAD_P2 | et.TRAIN_WGRAD_DZ_P2 | et.TRAIN_RES1_P2 | et.TRAIN_RES2_P2 | et.TRAIN_BSUM)
    split = [name for name, (op, t) in ops.items() if op.kind == "conv" and op.bn and op.src != g.input]  # the BatchNorm'd convs behind the head
    assert ops["head"][1].op.algo == ALGO_DIRECT and ops["head"][1].op.in_nchw and ops["final_layer"][1].op.out_nchw
    if plan_name != "default":
        assert not plan.uses_p2
        for name, (op, t) in ops.items():
            assert not t.fwd_p2 and not (t.p2_flags & p2_bits) and not t.zin_rel and not t.z_out, name
            assert bool(t.p2_flags & et.TRAIN_WGRAD_FP32) == (plan_name == "fp32"), name
        want = {"h2": ALGO_MFMA_H2, "bf3": ALGO_MFMA_BF3, "fp32": ALGO_MFMA}[plan_name]
        # (the fp16-split kernels have no configuration for the fuse graphs' 4 x 4 / 2 x 6 maps: those ops run bf16x3 in the h2 plan too)
        small = lambda op_i: plan_name == "h2" and plan.geo[op_i][2] * plan.geo[op_i][3] <= 16
        for name in split:
            op, t = ops[name]
            i = g.ops.index(op)
            assert t.op.algo == (ALGO_MFMA_BF3 if small(i) and t.op.algo != want else want), (name, t.op.algo)
            if op.cout % 16:  # (40 couts: dz has a partly filled 16-channel chunk, which no MFMA data gradient reads -- the direct kernel in every plan)
                assert t.dgrad_algo == ALGO_DIRECT and t.dgrad_form == 0 and name == "c" and case["args"][1] == 40, (name, t.dgrad_algo, t.dgrad_form)
            elif plan_name == "fp32":
                assert t.dgrad_algo == ALGO_MFMA and t.dgrad_form == 0, name
            elif op.stride == 1:
                assert t.dgrad_algo == want, (name, t.dgrad_algo)
            elif op.k == 3:  # the parity data gradient is a split-kernel form
                assert t.dgrad_algo == want and t.dgrad_form == 1, (name, t.dgrad_algo, t.dgrad_form)
        if plan_name == "h2":  # the fp16x2 weight gradients get both magnitude rows
            assert all(ops[name][1].gz_amax_off > 0 and (ops[name][1].op.in_amax_off > 0) == (ops[name][1].op.algo == ALGO_MFMA_H2) for name in split)
            assert sum(ops[name][1].op.algo == ALGO_MFMA_H2 for name in split) >= len(split) - 2
    kind = case["graph"]
    if kind == "blocks":
        assert all(ops[k][1].mask_off > 0 and ops[k][1].first_touch == 3 for k in ("b0.conv2", "b1.conv2"))
        if plan_name == "default":
            for name in ("b0.conv1", "b0.conv2", "b1.conv1", "b1.conv2"):
                t = ops[name][1]
                assert t.fwd_p2 == 1 and t.op.algo == ALGO_MFMA_H2 and t.dgrad_algo == ALGO_MFMA_H2 and t.dgrad_form == 0, name
                assert has(name, et.TRAIN_WGRAD_X_P2) and has(name, et.TRAIN_WGRAD_DZ_P2) and has(name, et.TRAIN_DGRAD_P2), name
            assert all(has(k, et.TRAIN_OUT_P2_ONLY) for k in ("head", "b0.conv1", "b1.conv1"))
            assert has("b0.conv2", et.TRAIN_RES1_P2) and not has("b1.conv2", et.TRAIN_RES1_P2)  # (the head's output exists as planes only)
            inz, bsum = case["inz"], case["bsum"]
            assert [int(ops[k][1].z_out) for k in ("b0.conv1", "b1.conv1")] == [int(inz)] * 2
            assert [int(ops[k][1].zin_rel) for k in ("b0.conv2", "b1.conv2")] == [-int(inz)] * 2
            # (BatchNorm sums in the data gradient: producers without residual -- conv1 -- and with residual + mask bytes -- conv2 of block 0)
            assert [has(k, et.TRAIN_BSUM) for k in ("b0.conv2", "b1.conv1", "b1.conv2")] == [bsum] * 3
            assert not has("b0.conv1", et.TRAIN_BSUM)  # (the head keeps no dz planes)
            assert plan.n_bn_in_conv == 2 * int(inz) and plan.n_bn_bwd_in_dgrad == 3 * int(bsum)
    elif kind == "bneck":
        stride = case["args"][2]
        assert ops["bn0.conv3"][1].mask_off > 0 and ops["bn0.conv3"][1].first_touch == 3
        assert ops["bn0.downsample.0"][0].stride == stride and ops["bn0.conv2"][0].stride == stride
        lib = _lib.lib()
        covers = lambda op: bool(lib.mval_conv_wgrad_split_covers(C.c_int(op.cin), C.c_int(op.cout), C.c_int(op.k), C.c_int(op.stride)))
        wide = case["args"][1] >= 64  # (1x1 with >= 64 channels on both sides: the split kernel; 32 planes: the exact-fp32 weight gradient)
        assert covers(ops["bn0.conv1"][0]) == wide and covers(ops["bn0.conv3"][0]) == wide
        assert covers(ops["bn0.downsample.0"][0]) == (stride == 1)          # (1x1 stride 2: the exact-fp32 weight-gradient kernel)
        if stride == 2 and plan_name != "fp32":
            assert ops["bn0.conv2"][1].dgrad_form == 1  # the four-parity data gradient inside a plan
            assert ops["bn0.downsample.0"][1].dgrad_algo == ALGO_MFMA and ops["bn0.downsample.0"][1].dgrad_form == 0
        if plan_name == "default":
            for name in ("bn0.conv1", "bn0.conv2", "bn0.downsample.0", "bn0.conv3"):
                assert ops[name][1].fwd_p2 == 1, name
            for name in ("bn0.conv1", "bn0.conv3"):  # (the weight gradient reads planes where the split kernel covers the conv)
                assert has(name, et.TRAIN_WGRAD_X_P2) == wide and has(name, et.TRAIN_WGRAD_DZ_P2) == wide and has(name, et.TRAIN_DGRAD_P2), name
            # (conv3's exact-fp32 weight gradient of the narrow block reads conv2's fp32 output: it is kept beside the planes)
            assert has("bn0.conv2", et.TRAIN_WGRAD_X_P2) and has("bn0.conv2", et.TRAIN_OUT_P2_ONLY) == wide
            if stride == 1:
                assert has("bn0.downsample.0", et.TRAIN_WGRAD_X_P2) and has("bn0.downsample.0", et.TRAIN_WGRAD_DZ_P2)
                assert int(ops["bn0.conv1"][1].z_out) == int(case["inz"]) and int(ops["bn0.conv2"][1].zin_rel) == -int(case["inz"])
                assert has("bn0.conv2", et.TRAIN_BSUM) == case["bsum"]
                assert plan.n_bn_in_conv == int(case["inz"]) and plan.n_bn_bwd_in_dgrad == int(case["bsum"])
            else:
                assert ops["bn0.conv2"][1].dgrad_algo == ALGO_MFMA_H2 and not has("bn0.conv2", et.TRAIN_DGRAD_P2)
                assert not has("bn0.downsample.0", et.TRAIN_WGRAD_X_P2)
    elif kind == "fuse":
        assert plan.n_lanes == 2
        for name in ("f01", "f02", "f10", "f12"):  # one phase whose gradient slots (x0, x2) are written from both lanes
            assert has(name, et.TRAIN_LANE_ORD) and has(name, et.TRAIN_LANE_FREE), name
            assert has(name, et.TRAIN_LANE_FWD) == has(name, et.TRAIN_LANE_BWD) == (name in ("f10", "f12")), name
        assert not any(has(name, et.TRAIN_LANE_ORD) for name in ("head", "t1", "t2", "m", "final_layer"))
        assert [ops[k][0].up for k in ("f01", "f02", "f10", "f12", "m")] == [1, 2, 0, 1, 1]
        assert all(t.mask_off == 0 for _, t in ops.values())  # (upsampled sums: the unfused BatchNorm backward reads `out`)
        # first touch (bit 0 data gradient, 1 res1, 2 res2) in backward order: m stores y1 / y0 / x0, f12 stores x2 and b, f10 stores x1
        # and ACCUMULATES into x0, f02 stores a and accumulates into x2, f01 accumulates into x1 and x0
        assert [ops[k][1].first_touch for k in ("m", "f12", "f10", "f02", "f01", "t2", "t1")] == [7, 3, 2, 2, 0, 0, 0]
        if plan_name != "fp32":
            assert ops["t1"][1].dgrad_form == 1 and ops["f10"][1].dgrad_form == 1
        if plan_name == "default":
            assert ops["t1"][1].fwd_p2 == 1 and has("t1", et.TRAIN_WGRAD_X_P2) and not has("t1", et.TRAIN_WGRAD_DZ_P2)  # (x planes + dz row)
            assert ops["f10"][1].fwd_p2 == 1 and has("f10", et.TRAIN_WGRAD_X_P2)
    elif kind == "deconv":
        assert [op.kind for op, _ in ops.values()] == ["conv", "maxpool", "conv", "deconv", "conv"]
        up = ops["up"][1]
        assert up.op.algo == ALGO_MFMA and up.dgrad_algo == ALGO_MFMA and up.wd_off >= 0 and ops["up"][0].k == 4
        assert ops["maxpool"][1].first_touch == 1 and ops["c1"][1].first_touch == 1
        if plan_name == "default":  # dz as planes, x through its magnitude row (the max-pool's output is fp32)
            assert not ops["c1"][1].fwd_p2 and has("c1", et.TRAIN_DGRAD_P2) and has("c1", et.TRAIN_WGRAD_DZ_P2) and not has("c1", et.TRAIN_WGRAD_X_P2)
            assert ops["c1"][1].op.in_amax_off > 0
    elif kind in ("branches", "shared"):
        pre = ("a0", "a1", "b0", "b1") if kind == "branches" else ("b0", "b1")
        conv1, conv2 = [p + ".conv1" for p in pre], [p + ".conv2" for p in pre]
        assert all(ops[k][1].mask_off > 0 for k in conv2) and not any(ops[k][1].mask_off > 0 for k in conv1)
        if kind == "branches":
            assert plan.n_lanes == 2 and len(g.ops) == 12
            for name, (op, t) in ops.items():  # the second pair of blocks is lane 1 of the blocks' phase, forward and backward
                assert op.lane == int(name.startswith("b")) and has(name, et.TRAIN_LANE_FREE), name
                assert has(name, et.TRAIN_LANE_FWD) == has(name, et.TRAIN_LANE_BWD) == (op.lane == 1), name
            assert len({ops[k][0].phase for k in conv1 + conv2}) == 1 and ops["m"][0].up == 1 and ops["m"][1].mask_off == 0
            assert plan.geo[g.ops.index(ops["a0.conv1"][0])][:2] == tuple(2 * v for v in plan.geo[g.ops.index(ops["b0.conv1"][0])][:2])
            # first touch (bit 0 data gradient, 1 res1) in backward order: m stores b1's and a1's output gradients; on each lane conv2 of a
            # block stores its residual's slot and conv1 adds to it; t1 adds its data gradient to what a0 left in the head output's slot
            assert [ops[k][1].first_touch for k in ["m"] + conv2 + conv1 + ["t1"]] == [3, 3, 3, 3, 3, 0, 0, 0, 0, 0]
            if plan_name != "fp32":
                assert ops["t1"][1].dgrad_form == 1
        else:
            assert plan.n_lanes == 1 and len(g.ops) == 7 and ops["m"][0].src == ops["head"][0].dst and ops["m"][0].res1 == ops["b1.conv2"][0].dst
            # in backward order m stores the head output's gradient slot (and b1's): b0.conv2's residual gradient is ADDED to that slot
            # (bit 1 clear), as is b0.conv1's data gradient
            assert [ops[k][1].first_touch for k in ("m", "b1.conv2", "b1.conv1", "b0.conv2", "b0.conv1")] == [3, 3, 0, 1, 0]
            assert ops["m"][1].mask_off > 0
        if plan_name == "default":
            inz, bsum = case["inz"], case["bsum"]
            for name in conv1 + conv2:
                t = ops[name][1]
                assert t.fwd_p2 == 1 and t.op.algo == ALGO_MFMA_H2 and t.dgrad_algo == ALGO_MFMA_H2 and t.dgrad_form == 0, name
                assert has(name, et.TRAIN_WGRAD_X_P2) and has(name, et.TRAIN_WGRAD_DZ_P2) and has(name, et.TRAIN_DGRAD_P2), name
            assert [int(ops[k][1].z_out) for k in conv1] == [int(inz)] * len(pre) and not any(ops[k][1].z_out for k in conv2 + ["m"])
            assert [int(ops[k][1].zin_rel) for k in conv2] == [-int(inz)] * len(pre) and not any(ops[k][1].zin_rel for k in conv1 + ["m"])
            # every 3x3 but the first of a lane follows its producer in the list (the first follows t1 / the other lane / the head)
            first = [pre[0] + ".conv1"] + (["b0.conv1"] if kind == "branches" else [])
            want = {name for name in conv1 + conv2 if name not in first} if bsum else set()
            assert {name for name in ops if has(name, et.TRAIN_BSUM)} == want
            assert plan.n_bn_in_conv == len(pre) * int(inz) and plan.n_bn_bwd_in_dgrad == len(want)
            if kind == "branches":
                assert plan.n_bn_in_conv == 4 and plan.n_bn_bwd_in_dgrad == 6
    elif kind in ("single", "linear"):
        assert [op.conv for op in g.ops] == ["head", "c", "final_layer"] and ops["c"][0].relu == ops["head"][0].relu == (kind == "single")
        if plan_name == "default" and "forms" in case:  # conv c runs on the forms the case is in the table for; a fall-back to another kernel fails here
            import p2_forms as pf

            got = tuple(f and pf.name(f) for f in _c_forms(case, plan))
            assert got == tuple(case["forms"]), (got, case["forms"])
            assert not ops["c"][1].zin_rel and not has("c", et.TRAIN_BSUM)
    if plan_name == "default":
        assert plan.uses_p2


def _n_bsum(case):
    """Data gradients of the default plan that keep BatchNorm backward sums: every 3x3 that follows its producer in the op list."""
    if not case.get("bsum"):
        return 0
    return {"blocks": 3, "bneck": 1, "branches": 6, "shared": 3}[case["graph"]]


def _host_plan(case, plan_name):
    from multi_view_active_learning_amd import engine_train as et

    sw = dict(et._SWITCHES, **PLANS[plan_name])  # the default switches, whatever the environment says
    return et.TrainPlan(_model(case).train(), case["n"], 2 * case["hw"][0], 2 * case["hw"][1], torch.device("cpu"), sw=sw)


@pytest.mark.parametrize("case_id", list(CASES))
def test_small_graph_plans_take_the_claimed_paths(case_id):
    """No GPU: the four plans of every case, built on the CPU, take the paths the case is in the table for; and the case's inputs satisfy the
    ReLU-margin condition (every ReLU's smallest |pre-activation| in float64 is more than 64 x that tensor's largest float32 - float64
    difference)."""
    case = CASES[case_id]
    for plan_name in PLANS:
        _check_plan(case, plan_name, _host_plan(case, plan_name))
    margins = _reference(case_id)[2].relu_margins()
    assert margins and min(margins.values()) > MARGIN, margins


def _is_late(f, cus=LATE_CUS):
    import p2_forms as pf

    return f.tiles_total * f.groups > pf.resident_cap(f, cus)


@pytest.mark.parametrize("case_id", list(LINEAR_CASES))
def test_linear_plans_take_the_claimed_forms(case_id):
    """No GPU: the default plan of every ReLU-free case takes the forms it is in the table for; there is no ReLU, so no margin to hold (the margin
    dictionary is empty); a `late` use has more tile x group work items than a device of up to LATE_CUS compute units holds workgroups, the
    batch is even; and on the float64 reference the two image kinds of a `seq` case differ by 2^6 and more in max |.| at conv c's input."""
    case = LINEAR_CASES[case_id]
    plan = _host_plan(case, "default")
    _check_plan(case, "default", plan)
    forms = dict(zip(("train", "dgrad"), _c_forms(case, plan)))
    for use in case.get("late", ()):
        assert _is_late(forms[use]) and case["n"] % 2 == 0, (use, forms[use].tiles_total * forms[use].groups)
    x, g, ref = _linear_reference(case_id)
    assert ref.relu_margins() == {}
    if case.get("seq"):
        assert case.get("late") and not np.any(ref.sd64["head_bn.bias"].numpy())
        seq = _late_seq(case)
        a_in = ref.acts[torch.float64][_conv_c(plan)[1].src]
        amax = a_in.abs().amax(dim=(1, 2, 3)).numpy()
        a_max = max(amax[i] for i, k in enumerate(seq) if k == "A")
        b_max = min(amax[i] for i, k in enumerate(seq) if k == "B")  # (the weakest B image against the strongest A image)
        print(f"[small graphs] {case_id}: max |A image| / max |B image| = 2^{np.log2(a_max / b_max):.2f} ({seq.count('A')} A, {seq.count('B')} B)")
        assert min(seq.count("A"), seq.count("B")) >= case["n"] // 4 and a_max <= LATE_CONTRAST * b_max, (a_max, b_max)


def test_linear_cases_cover_the_later_tile_families():
    """At most 8 `late` rows; between them a 1x1 conv, one over every second pixel, 3x3 with row sharing, on odd tiles and at stride 2, an `nt2`
    row; the forward of each and the data gradient of three."""
    late = {k: c for k, c in LINEAR_CASES.items() if c.get("late")}
    assert 0 < len(late) <= 8 and all(c.get("seq") for c in late.values())
    fwd = [c["forms"][0] for c in late.values() if "train" in c["late"]]
    assert len(fwd) == len(late) and sum("dgrad" in c["late"] for c in late.values()) >= 3
    for mark in ("k1s1_", "_sub", "_rs", "_ow", "k3s2_", "_nt2_"):
        assert any(mark in f for f in fwd), mark


def test_small_graph_cases_cover_every_weight_gradient_form():
    """Together the cases reach the six operand forms of wb_launch (x planes / dz planes / both / x from the producer's z / fp16x2 with rows /
    bf16x3) and 16- and 8-wide tiles, NT 1 and 2, 3x3 stride 1 and 2 and 1x1 of the split weight gradient; one case has fewer tiles than slabs."""
    from multi_view_active_learning_amd import engine_train as et

    forms, tiles, few_tiles = set(), set(), False
    for case in CASES.values():
        for plan_name in PLANS:
            plan = _host_plan(case, plan_name)
            for i, (op, t) in enumerate(zip(plan.graph.ops, plan.ops)):
                if not (op.kind == "conv" and op.bn and op.k in (1, 3) and op.cin >= 16):
                    continue
                if not ((op.k == 3) or (op.stride == 1 and op.cin >= 64 and op.cout >= 64)):  # (mval_wgrad_bf3_covers)
                    continue
                xp2, zp2 = bool(t.p2_flags & et.TRAIN_WGRAD_X_P2), bool(t.p2_flags & et.TRAIN_WGRAD_DZ_P2)
                if plan_name == "default":
                    form = "XZ" if t.zin_rel else "XP2+ZP2" if xp2 and zp2 else "XP2" if xp2 else "ZP2" if zp2 else None
                else:
                    form = {"h2": "PL2_rows", "bf3": "PL3", "fp32": None}[plan_name]
                if form is None:
                    continue
                forms.add(form)
                wout, hout = plan.geo[i][3], plan.geo[i][2]
                tile = tg.wgrad_tile(op.k, op.stride, wout, op.cout)
                tw, th = tile[2], (32 if op.stride == 2 else 64) // tile[2]
                tiles.add(tile)
                few_tiles |= wout < tw and hout < th  # (one ragged tile per image: 3 tiles for 3 images, far fewer than slabs)
    assert forms == {"XP2", "ZP2", "XP2+ZP2", "XZ", "PL2_rows", "PL3"}, forms
    assert {t[2] for t in tiles} == {8, 16} and {t[3] for t in tiles} == {1, 2} and {t[:2] for t in tiles} == {(1, 1), (3, 1), (3, 2)}, tiles
    assert tiles <= tg.WGRAD_TILE_FORMS, tiles
    # the joint forms the graphs reach (3x3 stride 2 on 8-wide tiles only with cout > 32; tests/test_gpu_train_entries.py asserts all ten of its own)
    assert tiles >= {(1, 1, 16, 2), (1, 1, 8, 2), (3, 1, 16, 1), (3, 1, 16, 2), (3, 1, 8, 1), (3, 1, 8, 2), (3, 2, 8, 2)}, tiles
    assert few_tiles


# ---- the device against float64 ----
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


_RATIOS = {}


def _report(name, obj):
    """Measured figures the documents quote: written where tests/test_gpu_train.py::_report writes the suite's other measurements."""
    from test_gpu_train import _report as report

    report(name, obj)


def _gradient_check(tag, model, want, floor_of, factor):
    """Every parameter gradient against float64: e <= factor * floor + 2e-5 per tensor -> the e / floor ratios."""
    ratios, bad = [], []
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        e = tg.rel_l2(p.grad.cpu().numpy(), want[k])
        floor = tg.rel_l2(floor_of[k], want[k])
        ratios.append(e / max(floor, 1e-12))
        if not e <= factor * floor + 2e-5:
            bad.append((k, e, floor))
    print(f"[small graphs] {tag}: e / floor median {np.median(ratios):.2f} max {max(ratios):.2f} (F = {factor})")
    assert not bad, (tag, factor, bad)
    return ratios


@pytest.mark.gpu
@pytest.mark.parametrize("plan_name", list(PLANS))
@pytest.mark.parametrize("case_id", list(CASES))
def test_small_graph_training_step_vs_float64(dev, case_id, plan_name, monkeypatch):
    """One forward + backward of the case on the plan `plan_name` (default; MVAL_TRAIN_P2=0: the h2 kernels; MVAL_CONV=bf3; MVAL_CONV=fp32):
    the output, every parameter gradient and every BatchNorm running statistic against float64 autograd; then a second step with an
    all-ones output gradient into the same model without zero_grad: the gradients are the sum of the two float64 gradients."""
    _training_step(dev, monkeypatch, case_id, CASES[case_id], plan_name, *_reference(case_id))


def _z_read(plan):
    """Conv c's raw z as the forward left it in the plan's arena (fp32 NHWC at z_off) -> float64 NCHW on the host."""
    i, op, t = _conv_c(plan)
    hout, wout = plan.geo[i][2:4]
    assert t.z_off >= 0 and t.fwd_p2
    z = plan.arena[t.z_off : t.z_off + plan.n * hout * wout * op.cout].reshape(plan.n, hout, wout, op.cout)
    return z.permute(0, 3, 1, 2).cpu().double().numpy()


def _z_check(case_id, case, ref, plan, z, factor):
    """z of conv c against conv(float64 input of c, float64 weights) PER IMAGE: relative L2 e_i <= factor * floor_i + 2e-5, floor_i = the error of
    torch-CPU float32's conv of ITS input on that image -> the figures for the report."""
    import torch.nn.functional as F

    _, op, _ = _conv_c(plan)
    conv = lambda dt: F.conv2d(ref.acts[dt][op.src], ref.sd64["c.weight"].to(dt), None, stride=op.stride, padding=op.pad).double().numpy()
    z64, z32 = conv(torch.float64), conv(torch.float32)
    assert z.shape == z64.shape
    per_image = lambda a: np.sqrt(((a - z64) ** 2).sum(axis=(1, 2, 3)) / (z64 ** 2).sum(axis=(1, 2, 3)))
    e, floor = per_image(z), per_image(z32)
    ratio = e / np.maximum(floor, 1e-12)
    seq = _late_seq(case) or "B" * case["n"]
    fig = {}
    for kind in sorted(set(seq)):
        idx = [i for i, k in enumerate(seq) if k == kind]
        fig[kind] = dict(e_max=float(e[idx].max()), floor_max=float(floor[idx].max()), ratio_max=float(ratio[idx].max()))
    print(f"[small graphs] {case_id} z of c per image: " + "; ".join(f"{k}: e <= {v['e_max']:.2e}, floor <= {v['floor_max']:.2e}, e / floor <= {v['ratio_max']:.2f}"
                                                                      for k, v in fig.items()) + f" (F = {factor})")
    bad = [(i, seq[i], float(e[i]), float(floor[i])) for i in range(case["n"]) if not e[i] <= factor * floor[i] + 2e-5]
    assert not bad, (case_id, factor, bad[:8], len(bad))
    return fig


def _training_step(dev, monkeypatch, case_id, case, plan_name, x, g, ref):
    """The body of the two tests below."""
    from multi_view_active_learning_amd import _lib, engine_train as et

    margins = ref.relu_margins()
    if case["graph"] == "linear":
        assert margins == {}  # (no ReLU: no mask that could flip)
    else:
        assert margins and min(margins.values()) > MARGIN, margins  # (a condition on the inputs: no ReLU mask flips within fp32's error)
    for k in et._SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in PLANS[plan_name].items():
        monkeypatch.setenv(k, v)
    f64, f32 = torch.float64, torch.float32
    model = _model(case).to(dev).train()
    xd = x.to(dev)
    _lib.train_bsum_launches(reset=True)
    out = model(xd)
    z_c = _z_read(next(iter(model._train_plans.values()))) if case["graph"] == "linear" else None  # (after the forward, before the backward)
    out.backward(g.to(dev))
    plan = next(iter(model._train_plans.values()))
    _check_plan(case, plan_name, plan)
    # every data gradient the plan flags really kept the sums (no launch fell back to the plain form), and no other did
    assert _lib.train_bsum_launches() == plan.n_bn_bwd_in_dgrad == (_n_bsum(case) if plan_name == "default" else 0)
    assert not model.__dict__.get("_train_p2_off", False), plan.p2_slack
    want_out = ref.out[f64].numpy()
    np.testing.assert_allclose(out.detach().cpu().numpy(), want_out, rtol=2e-5, atol=2e-5 * float(np.abs(want_out).max()))
    factor = 2.0 if plan_name in ("bf3", "fp32") else 4.0
    if plan_name == "default":
        b = ref.p2_slack_bits(model._graph, list(plan._p2_act), case["n"])
        assert 0 <= b <= 8, b
        factor = 4.0 * 2.0 ** b
    z_fig = _z_check(case_id, case, ref, plan, z_c, factor) if z_c is not None else None
    r1 = _gradient_check(f"{case_id} / {plan_name} step 1", model, ref.grad1[f64], ref.grad1[f32], factor)
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            np.testing.assert_allclose(v.cpu().numpy(), ref.stats[f64][k], rtol=2e-4, atol=2e-5, err_msg=k)
    # second step, all-ones output gradient, no zero_grad: AccumulateGrad adds every slot exactly once
    out2 = model(xd)
    out2.backward(torch.ones_like(out2))
    assert next(iter(model._train_plans.values())) is plan and plan.steps == 2
    assert _lib.train_bsum_launches(reset=True) == 2 * plan.n_bn_bwd_in_dgrad
    assert torch.equal(out2.detach(), out.detach())
    both = lambda d: {k: ref.grad1[d][k] + ref.grad2[d][k] for k in ref.keys}
    r2 = _gradient_check(f"{case_id} / {plan_name} step 1 + 2", model, both(f64), both(f32), factor)
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var")):  # the momentum update applied twice (the plan is re-used)
            np.testing.assert_allclose(v.cpu().numpy(), ref.stats2[f64][k], rtol=2e-4, atol=2e-5, err_msg=k + " after step 2")
            assert not np.array_equal(ref.stats2[f64][k], ref.stats[f64][k]), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 2, k
    _RATIOS[f"{case_id}/{plan_name}"] = dict(F=factor, step1=dict(median=float(np.median(r1)), max=float(max(r1))),
                                             step12=dict(median=float(np.median(r2)), max=float(max(r2))))
    if z_fig is not None:
        _RATIOS[f"{case_id}/{plan_name}"]["z_per_image"] = z_fig
    _report("small_graph_error_ratios.json", _RATIOS)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(LINEAR_CASES))
def test_linear_training_step_vs_float64(dev, case_id, monkeypatch):
    """The ReLU-free rows (LINEAR_CASES: the `nt2` forms of the 1x1 conv, and a workgroup's later tiles with images of two magnitudes) on the
    default plan: everything test_small_graph_training_step_vs_float64 asserts, with the same bounds -- the running statistics are the check
    on the (sum, sum of squares) registers a workgroup keeps over its tile walk -- and conv c's raw z, read from the plan's arena between the
    forward and the backward, against float64 per image (_z_check; F = 4 * 2^b as for the gradients).  A scale kept from a B tile costs an A
    image ten of its bits, about 2e-4 in relative L2; checks over the whole batch are dominated by the B images and cannot see it.  For the data gradient
    only the overflow direction of a wrong scale shows, through the head's weight gradient (a scale too large merely costs bits of a dx that
    no whole-batch figure resolves): no separate check is made up for it.
    The per-image figures (worst e, floor and e / floor per image kind) go to small_graph_error_ratios.json, key `<case>/default`, z_per_image.
    Measured on an MI355X: floor 1.3e-7 .. 3.0e-7 on A and B images alike, e / floor at most 1.12 on the `nt2` rows, 0.91 .. 1.09 on the B
    images and 1.03 .. 1.24 on the A images of the later-tile rows, 3.09 on the A images of the stride-2 1x1 row (e = 4.1e-7); F is 256 or 512."""
    _training_step(dev, monkeypatch, case_id, LINEAR_CASES[case_id], "default", *_linear_reference(case_id))


def _one_step(case, x, g, dev, monkeypatch, env):
    """One forward + backward of a fresh model (the case's seeded parameters) on the default plan under the switches `env`:
    (plan, output, parameter gradients, running statistics, data gradients that kept BatchNorm sums)."""
    from multi_view_active_learning_amd import _lib, engine_train as et

    for k in et._SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = _model(case).to(dev).train()
    _lib.train_bsum_launches(reset=True)
    out = model(x.to(dev))
    out.backward(g.to(dev))
    count = _lib.train_bsum_launches(reset=True)
    plan = next(iter(model._train_plans.values()))
    assert not model.__dict__.get("_train_p2_off", False), plan.p2_slack
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    stats = {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return plan, out.detach().clone(), grads, stats, count


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", [k for k, c in CASES.items() if c["inz"] or c["bsum"]])
def test_small_graph_bn_in_conv_halves_vs_separate_passes(dev, case_id, monkeypatch):
    """The two BatchNorm-in-conv halves against the separate passes, on every tile form and edge of the table: one forward + backward of
    the default plan from the same model state as D (defaults), F (MVAL_TRAIN_BN_BWD_IN_DGRAD=0: the forward half alone) and S (also
    MVAL_TRAIN_BN_IN_CONV=0: BatchNorm apply and backward reduction as passes of their own).

    F vs S: the conv's staging computes relu(BatchNorm(z)) with the apply kernel's arithmetic, so the output, every parameter gradient and
    every running statistic are the same bits (tests/test_gpu_train.py holds this on whole networks; here at every tile form).
    D vs F: the output and the running statistics are the same bits; the gradients differ in the order of the fp32 partial sums and in
    where dz's P2 scale comes from -- rounding-level effects -- so against float64 every gradient has  e_D <= 2 * max(e_F, floor)  (floor:
    torch-CPU float32's error).  The bound is relative to the reference, not to the other kernel: a dropped border row, a wrong mask bit
    or a missed residual scatter is orders of magnitude outside it.  D's data gradients keep the sums exactly plan.n_bn_bwd_in_dgrad
    times (mval_train_bsum_launches), F's never.  Measured on an MI355X: e_D / max(e_F, floor) at most 1.16 (blocks_c32_12x32, b0.bn1.weight),
    per-case maxima 1.00 .. 1.16, medians 0.90 .. 1.00 (small_graph_error_ratios.json, key bn_in_conv_ab)."""
    from multi_view_active_learning_amd import engine_train as et

    case = CASES[case_id]
    x, g, ref = _reference(case_id)
    f64, f32 = torch.float64, torch.float32
    plan_d, out_d, g_d, st_d, n_d = _one_step(case, x, g, dev, monkeypatch, {})
    plan_f, out_f, g_f, st_f, n_f = _one_step(case, x, g, dev, monkeypatch, {"MVAL_TRAIN_BN_BWD_IN_DGRAD": "0"})
    plan_s, out_s, g_s, st_s, n_s = _one_step(case, x, g, dev, monkeypatch, {"MVAL_TRAIN_BN_BWD_IN_DGRAD": "0", "MVAL_TRAIN_BN_IN_CONV": "0"})
    _check_plan(case, "default", plan_d)
    assert not any(t.p2_flags & et.TRAIN_BSUM for t in plan_f.ops) and plan_f.n_bn_bwd_in_dgrad == 0
    assert not any(t.p2_flags & et.TRAIN_BSUM for t in plan_s.ops) and not any(t.z_out or t.zin_rel for t in plan_s.ops) and plan_s.n_bn_in_conv == 0
    assert plan_f.n_bn_in_conv == plan_d.n_bn_in_conv and [(t.z_out, t.zin_rel) for t in plan_f.ops] == [(t.z_out, t.zin_rel) for t in plan_d.ops]
    assert n_d == plan_d.n_bn_bwd_in_dgrad == _n_bsum(case) and n_f == 0 and n_s == 0, (n_d, n_f, n_s)
    if case["inz"]:  # the forward half (without it F and S are the same plan)
        assert torch.equal(out_f, out_s)
        bad = [k for k in g_s if not torch.equal(g_f[k], g_s[k])]
        assert not bad, bad
        assert all(torch.equal(st_f[k], st_s[k]) for k in st_s) and len(st_s) > 0
    # the backward half
    assert torch.equal(out_d, out_f)
    assert all(torch.equal(st_d[k], st_f[k]) for k in st_f) and len(st_f) > 0
    ratios, bad = {}, []
    for k in ref.keys:
        want = ref.grad1[f64][k]
        e_d, e_f = tg.rel_l2(g_d[k].cpu().numpy(), want), tg.rel_l2(g_f[k].cpu().numpy(), want)
        floor = tg.rel_l2(ref.grad1[f32][k], want)
        ratios[k] = e_d / max(e_f, floor, 1e-300)
        if not e_d <= 2.0 * max(e_f, floor):
            bad.append((k, e_d, e_f, floor))
    worst = max(ratios, key=ratios.get)
    print(f"[small graphs] {case_id} BN-in-conv A/B: e_D / max(e_F, floor) median {np.median(list(ratios.values())):.2f} max {ratios[worst]:.2f} ({worst}); "
          f"sums kept by {n_d} / {n_f} / {n_s} data gradients (D / F / S)")
    _RATIOS.setdefault("bn_in_conv_ab", {})[case_id] = dict(median=float(np.median(list(ratios.values()))), max=float(ratios[worst]), worst=worst,
                                                            bsum_launches=dict(D=n_d, F=n_f, S=n_s))
    _report("small_graph_error_ratios.json", _RATIOS)
    assert not bad, (case_id, bad)

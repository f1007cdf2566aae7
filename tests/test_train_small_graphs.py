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
forms and edges, and compared with the separate passes on the same graphs."""
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
}
PLANS = {"default": {}, "h2": {"MVAL_TRAIN_P2": "0"}, "bf3": {"MVAL_CONV": "bf3"}, "fp32": {"MVAL_CONV": "fp32"}}
MARGIN = 64.0
# the input batch of every case: seeded Gaussian values moved off the ReLUs' zeros on the float64 reference (golden/make_small_graph_inputs.py)
INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_graph_inputs.npz")


def _model(case):
    return tg.TinyNet(tg.BUILDERS[case["graph"]], case["args"], case["seed"])


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
            if plan_name == "fp32":
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
    if plan_name == "default":
        assert plan.uses_p2


def _n_bsum(case):
    """Data gradients of the default plan that keep BatchNorm backward sums: every 3x3 that follows its producer in the op list."""
    if not case["bsum"]:
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
    from multi_view_active_learning_amd import _lib, engine_train as et

    case = CASES[case_id]
    x, g, ref = _reference(case_id)
    margins = ref.relu_margins()
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
    _report("small_graph_error_ratios.json", _RATIOS)


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

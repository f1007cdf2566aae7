"""The case tables of tests/test_gpu_plain_ops.py: the plain VALU operators that open every network (csrc/conv_stem.hip's stem kernels,
csrc/net.hip's direct conv / transposed conv / max-pool / amax kernels) and their training counterparts (the stem and direct weight-gradient
kernels and the slab reduction of csrc/conv_wgrad.hip, csrc/train_ops.hip's max-pool backward), each run alone.

Every row names the kernel it is in the table for; which kernel a launch really runs is read from the library (mval_conv_stem_covers,
mval_conv_wgrad_path: the launchers' own predicates, host arithmetic, no GPU).  The branch a row is meant to reach inside that kernel -- a second
cout pass, a ragged tile, a second grid-stride trip -- follows from the launch geometry, restated here from the sources as plain functions
(`*_tags`); the host test holds every row to its kernel and the tables together to REQUIRED."""
import zlib

ALGO_DIRECT, OP_CONV = 0, 0
WGRAD_PATHS = ("refused", "split", "stem", "mfma", "direct")  # MVAL_WGRAD_* of include/mval_hip.h, by value


def seed(name):
    return zlib.crc32(name.encode())


# ---- 1. stem forward: conv_stem_kernel<3>, <7> and conv_direct_kernel on NCHW input ----
# (id, (n, cout, h, w), k, stride, pad, options, kernel).  cin = 3, NCHW input.  Options: relu; no_stem (MvalOp.no_stem); zero (the last
# image is all zeros and every shift <= 0, so that with the ReLU its output -- and its kept magnitude -- is 0).  Without relu the shifts
# are strongly negative: the extreme output of every image is negative.
ST_TH, ST_TW = 8, 16  # conv_stem.hip: output pixels per workgroup tile


def _stem_rows():
    rows = []
    for k in (3, 7):
        for relu in ("relu", ""):
            rows.append((f"odd_37x51_k{k}_{relu or 'lin'}", (2, 64, 37, 51), k, 2, k // 2, relu, f"stem{k}"))
            rows.append((f"below_tile_5x9_k{k}_{relu or 'lin'}", (1, 64, 5, 9), k, 2, k // 2, relu, f"stem{k}"))
            rows.append((f"five_quads_k{k}_{relu or 'lin'}", (2, 20, 18, 34), k, 2, k // 2, relu, f"stem{k}"))
        rows.append((f"one_pixel_k{k}", (1, 4, 1, 1), k, 2, k // 2, "relu", f"stem{k}"))
        rows.append((f"zero_image_k{k}", (2, 20, 18, 34), k, 2, k // 2, "relu+zero", f"stem{k}"))
        rows.append((f"cout68_k{k}", (2, 68, 18, 34), k, 2, k // 2, "relu", f"stem{k}"))
        rows.append((f"cout6_k{k}", (2, 6, 9, 11), k, 2, k // 2, "relu", "direct"))
        rows.append((f"no_stem_k{k}", (2, 64, 37, 51), k, 2, k // 2, "relu+no_stem", "direct"))
    rows.append(("cout96_k3", (1, 96, 18, 34), 3, 2, 1, "relu", "stem3"))
    rows.append(("cout92_k7_lds_63420", (1, 92, 18, 34), 7, 2, 3, "relu", "stem7"))
    rows.append(("cout96_k7_lds_65772", (1, 96, 18, 34), 7, 2, 3, "relu", "direct"))
    rows.append(("k5_s2", (2, 16, 12, 12), 5, 2, 2, "relu", "direct"))
    rows.append(("k3_s1", (2, 16, 12, 12), 3, 1, 1, "relu", "direct"))
    return rows


STEM_CASES = _stem_rows()


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def stem_lds_bytes(k, cout):
    """mval_launch_conv_stem: weights [k*k*3][cout] + the input patch [3][PH][PW | 1] of an 8 x 16 tile at stride 2."""
    ph, pw = (ST_TH - 1) * 2 + k, ((ST_TW - 1) * 2 + k) | 1
    return (k * k * 3 * cout + 3 * ph * pw) * 4


def stem_rule(cout, k, stride, pad, no_stem):
    """The stem kernel's conditions restated (cin = 3, NCHW in, NHWC out, no residual, no up-sampling): 3, 7 or 0."""
    if no_stem or stride != 2 or k not in (3, 7) or pad != k // 2 or cout % 4 or stem_lds_bytes(k, cout) > 64 * 1024:
        return 0
    return k


def stem_op(case):
    """The MvalOp of a row as ops.fused_conv builds it, for mval_conv_stem_covers."""
    from multi_view_active_learning_amd.engine import _query_op

    _, (n, cout, h, w), k, stride, pad, opt, _ = case
    ho, wo = out_hw(h, w, k, stride, pad)
    return _query_op(OP_CONV, k, stride, pad, 3, cout, h, w, ho, wo, algo=ALGO_DIRECT, in_nchw=1, relu=int("relu" in opt), res1_off=-1, res2_off=-1,
                     no_stem=int("no_stem" in opt))


def stem_tags(case):
    _, (n, cout, h, w), k, stride, pad, opt, kernel = case
    ho, wo = out_hw(h, w, k, stride, pad)
    t = {kernel if kernel != "direct" else "direct_nchw"}
    if kernel == "direct":
        if "no_stem" in opt:
            t.add("no_stem_fallback")
        elif stem_rule(cout, k, stride, pad, False) == 0 and stride == 2 and k in (3, 7) and cout % 4 == 0:
            t.add("lds_fallback")
        elif cout % 4:
            t.add("direct_cout_not_4")
        else:
            t.add("direct_not_stem_shape")
        return t
    t.add("cout_pass_1")
    if cout > 64:
        t.add("cout_pass_2")
    if cout % 64:
        t.add("idle_quads")
    if ho % ST_TH and ho > ST_TH:
        t.add("ragged_y")
    if wo % ST_TW and wo > ST_TW:
        t.add("ragged_x")
    if ho < ST_TH and wo < ST_TW:
        t.add("below_tile")
    if h % 2 and w % 2 and 2 * (ho - 1) - pad + k - 1 >= h and 2 * (wo - 1) - pad + k - 1 >= w:  # bottom / right taps outside the image
        t.add("odd_input")
    t.add("relu" if "relu" in opt else "relu_off")
    if "zero" in opt:
        t.add("zero_image")
    return t


# ---- 2. max-pool forward and amax_kernel ----
# (id, (n, c, h, w), k, stride, pad, data).  data: "normal"; "special": post-ReLU data with whole windows tied at 0, a NaN, a +inf and a
# window that is all -inf (image 0; no -0.0 anywhere).
POOL_CASES = [
    ("odd_7x9", (1, 8, 7, 9), 3, 2, 1, "normal"),
    ("one_pixel", (1, 4, 1, 1), 3, 2, 1, "normal"),
    ("amax_scalar_54", (3, 6, 5, 5), 3, 2, 1, "normal"),
    ("amax_second_trip", (1, 64, 130, 128), 3, 2, 1, "normal"),
    ("k2_s2_p0", (2, 8, 6, 10), 2, 2, 0, "normal"),
    ("special_values", (2, 8, 9, 9), 3, 2, 1, "special"),
]
# mval_amax alone: (id, n_images, per_image, offset of the base pointer in floats)
AMAX_CASES = [
    ("off_by_4_bytes", 3, 1200, 1),
    ("off_by_4_bytes_many_trips", 1, 266240, 1),
    ("one_image_whole_tensor", 1, 2 * 7 * 5 * 8, 0),
    ("vector_with_scalar_free_tail", 2, 4096, 0),
]


def amax_tags(per_image, aligned=True):
    """mval_launch_amax: float4 loads when the base pointer is 16-byte aligned and per_image % 4 == 0; at most 64 workgroups of 256 threads
    per image, each thread strides over the image."""
    vec = aligned and per_image % 4 == 0
    blocks = min(64, max(1, (per_image // 4 + 255) // 256))
    items = per_image // 4 if vec else per_image
    t = {"amax_vector" if vec else "amax_scalar"}
    if items > blocks * 256:
        t.add("amax_second_trip")
    return t


def pool_tags(case):
    _, (n, c, h, w), k, stride, pad, data = case
    ho, wo = out_hw(h, w, k, stride, pad)
    return amax_tags(ho * wo * c) | {"pool_" + data, f"pool_k{k}"}


# ---- 3. transposed conv, direct ----
# (id, (n, cin, cout, h, w), k, stride, pad)
DECONV_CASES = [
    ("1x1_cout6", (1, 8, 6, 1, 1), 4, 2, 1),
    ("odd_cout19", (3, 5, 19, 5, 7), 4, 2, 1),
    ("c64_32", (2, 64, 32, 9, 6), 4, 2, 1),
    ("k2_s2_p0", (2, 8, 12, 5, 7), 2, 2, 0),
]


# ---- 4. weight gradients: stem, direct, slab reduction ----
# (id, (n, cin, cout, h, w), k, stride, pad, x_nchw, path)
WGRAD_CASES = [
    ("stem7_64x48", (2, 3, 64, 64, 48), 7, 2, 3, 1, "stem"),
    ("stem7_40x72", (3, 3, 32, 40, 72), 7, 2, 3, 1, "stem"),
    ("stem7_18x34", (1, 3, 16, 18, 34), 7, 2, 3, 1, "stem"),
    ("stem3_one_tile", (1, 3, 16, 16, 32), 3, 2, 1, 1, "stem"),
    ("stem7_one_tile", (1, 3, 16, 16, 32), 7, 2, 3, 1, "stem"),
    ("stem3_ps7", (7, 3, 16, 16, 32), 3, 2, 1, 1, "stem"),
    ("stem7_ps7", (7, 3, 16, 16, 32), 7, 2, 3, 1, "stem"),
    ("stem3_cout48", (2, 3, 48, 20, 36), 3, 2, 1, 1, "stem"),
    ("stem7_cout48", (2, 3, 48, 20, 36), 7, 2, 3, 1, "stem"),
    ("stem3_544_tiles", (17, 3, 16, 128, 128), 3, 2, 1, 1, "stem"),
    ("stem7_544_tiles", (17, 3, 16, 128, 128), 7, 2, 3, 1, "stem"),
    ("direct_nchw_cout96", (2, 3, 96, 18, 34), 3, 2, 1, 1, "direct"),
    ("direct_nchw_cout20", (2, 3, 20, 18, 34), 3, 2, 1, 1, "direct"),
    ("direct_nchw_k5", (2, 3, 16, 12, 12), 5, 2, 2, 1, "direct"),
    ("direct_nhwc_cin8", (2, 8, 16, 9, 11), 3, 1, 1, 0, "direct"),
    ("direct_nhwc_cin18", (2, 18, 16, 9, 11), 3, 2, 1, 0, "direct"),
    ("direct_nhwc_32_pad0", (2, 32, 32, 10, 12), 3, 1, 0, 0, "direct"),
    ("direct_1x3_map", (1, 8, 8, 1, 3), 3, 1, 1, 0, "direct"),
    ("refused_128_pad0", (1, 128, 128, 6, 6), 3, 1, 0, 0, "refused"),
]
WD_OUTPUTS_PER_ROW = 256 * 8  # conv_wgrad_direct_kernel: outputs per grid row
WD_MAX_OUTPUTS = 64 * WD_OUTPUTS_PER_ROW


def wg_splits(cin, cout, target=1024):
    """conv_wgrad.hip: the slabs mval_conv_wgrad_workspace_floats promises."""
    cb = ((cin + 31) // 32) * ((cout + 31) // 32)
    return min(512, max(1, target // cb))


def stem_wgrad_tiles(n, h, w, k):
    """The stem weight gradient walks 8 x 16 tiles of the stride-2 output, one image per tile."""
    ho, wo = out_hw(h, w, k, 2, k // 2)
    return n * ((ho + ST_TH - 1) // ST_TH) * ((wo + ST_TW - 1) // ST_TW)


def wgrad_slabs(case):
    """PS: the slabs (= workgroups along x) of the stem and direct launches."""
    _, (n, cin, cout, h, w), k, stride, pad, x_nchw, path = case
    if path == "stem":
        return min(512, stem_wgrad_tiles(n, h, w, k))
    ho, wo = out_hw(h, w, k, stride, pad)
    return min(n * ho * wo, 512, wg_splits(cin, cout))


def reduce_loops(ps):
    """wgrad_reduce_kernel: parts = clamp(PS / 8, 1, 16) lane groups per output; the loops (8, 4 or 1 slabs a round) some lane group enters."""
    parts = min(16, max(1, ps // 8))
    loops = set()
    for part in range(parts):
        p = part
        while p + 7 * parts < ps:
            loops.add(8)
            p += 8 * parts
        while p + 3 * parts < ps:
            loops.add(4)
            p += 4 * parts
        if p < ps:
            loops.add(1)
    return parts, loops


def wgrad_tags(case):
    _, (n, cin, cout, h, w), k, stride, pad, x_nchw, path = case
    if path == "refused":
        return {"wgrad_refused"}
    ps = wgrad_slabs(case)
    parts, loops = reduce_loops(ps)
    t = {f"reduce_loop_{l}" for l in loops} | {f"reduce_parts_{parts}"}
    if path == "stem":
        tiles = stem_wgrad_tiles(n, h, w, k)
        t |= {f"wgrad_stem{k}", f"wgrad_stem{k}_" + ("second_trip" if tiles > ps else "one_trip")}
        if cout < 64:
            t.add("wgrad_stem_idle_wave")
    else:
        e = k * k * cin * cout
        rows = (e + WD_OUTPUTS_PER_ROW - 1) // WD_OUTPUTS_PER_ROW
        t |= {"wgrad_direct_" + ("nchw" if x_nchw else "nhwc"), "wgrad_direct_rows_" + ("1" if rows == 1 else "2+")}
        ho, wo = out_hw(h, w, k, stride, pad)
        if n * ho * wo < 8:
            t.add("wgrad_direct_few_pixels")
    return t


# ---- 5. max-pool backward ----
# (id, (n, c, h, w), k, stride, pad, data).  data: "normal"; "relu": post-ReLU data with whole windows tied at 0; "nan": one NaN.
POOLB_CASES = [
    ("one_pixel", (1, 4, 1, 1), 3, 2, 1, "normal"),
    ("odd_5x5", (2, 8, 5, 5), 3, 2, 1, "normal"),
    ("even_6x6", (3, 16, 6, 6), 3, 2, 1, "normal"),
    ("relu_ties", (2, 8, 9, 10), 3, 2, 1, "relu"),
    ("nan", (2, 8, 7, 7), 3, 2, 1, "nan"),
    ("second_trip_513x512", (1, 64, 513, 512), 3, 2, 1, "normal"),
]
POOLB_MAX_WORKGROUPS = 16384


def poolb_tags(case):
    _, (n, c, h, w), k, stride, pad, data = case
    t = {"poolb_" + data}
    if n * h * w * (c // 4) > POOLB_MAX_WORKGROUPS * 256:
        t.add("poolb_second_trip")
    return t


# every kernel and branch the tables must reach together
REQUIRED = {
    "stem3", "stem7", "cout_pass_1", "cout_pass_2", "idle_quads", "ragged_y", "ragged_x", "below_tile", "odd_input", "relu", "relu_off", "zero_image",
    "lds_fallback", "no_stem_fallback", "direct_nchw", "direct_cout_not_4", "direct_not_stem_shape",
    "amax_vector", "amax_scalar", "amax_second_trip", "pool_special", "pool_k2", "pool_k3",
    "wgrad_stem3", "wgrad_stem7", "wgrad_stem3_one_trip", "wgrad_stem7_one_trip", "wgrad_stem3_second_trip", "wgrad_stem7_second_trip",
    "wgrad_stem_idle_wave", "wgrad_direct_nchw", "wgrad_direct_nhwc", "wgrad_direct_rows_1", "wgrad_direct_rows_2+", "wgrad_direct_few_pixels",
    "wgrad_refused", "reduce_loop_8", "reduce_loop_4", "reduce_loop_1", "reduce_parts_1", "reduce_parts_16",
    "poolb_normal", "poolb_relu", "poolb_nan", "poolb_second_trip",
}


def all_tags():
    t = set()
    for c in STEM_CASES:
        t |= stem_tags(c)
    for c in POOL_CASES:
        t |= pool_tags(c)
    for _, n, per, off in AMAX_CASES:
        t |= amax_tags(per, aligned=off % 4 == 0)
    for c in WGRAD_CASES:
        t |= wgrad_tags(c)
    for c in POOLB_CASES:
        t |= poolb_tags(c)
    return t

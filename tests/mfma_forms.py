"""The kernel forms of the exact-fp32 MFMA conv (csrc/conv_mfma.hip) as the library's own dispatch reports them (mval_conv_mfma_form: host
arithmetic, no GPU), for tests/test_gpu_mfma_forms.py: a name for every form, and the fixed sweep that collects every form the dispatch can
return for each way the library uses the kernel."""
import functools
import itertools

ALGO_MFMA = 1
OP_CONV, OP_DECONV = 0, 2
USES = ("op", "train", "dgrad")  # MVAL_SPLIT_USE_OP / _TRAIN_FWD / _DGRAD
NTH = 256  # threads of every instance of conv_mfma_kernel


def query(use, n, cin, cout, h, w, k, stride, kind="conv", relu=False, res1=False, res2=False, up=0, nchw=False, pad=None, in_nchw=False):
    """The MfmaForm of one launch, or None where the library has no exact-fp32 MFMA kernel for it.  (n, cin, cout, h, w, k, stride) describe
    the forward conv on an h x w input (pad k // 2 unless given), or ConvTranspose2d(k4, s2, p1) for kind "deconv"; use "op": mval_op_launch,
    "train": the conv of mval_train_forward, "dgrad": mval_conv_dgrad of that conv (res1: accumulate) -- for a transposed conv the k4 stride-2
    conv mval_train_backward runs as its data gradient."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    if kind == "deconv":
        assert (k, stride) == (4, 2)
        pad, hout, wout = 1, 2 * h, 2 * w
    else:
        pad = k // 2 if pad is None else pad
        hout, wout = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    op = _query_op(OP_DECONV if kind == "deconv" else OP_CONV, k, stride, pad, cin, cout, h, w, hout, wout, up=up, relu=int(relu), out_nchw=int(nchw),
                   in_nchw=int(in_nchw), res1_off=0 if res1 else -1, res2_off=0 if res2 else -1, algo=ALGO_MFMA)
    return _lib.conv_mfma_form(USES.index(use), op, n)


def name(f):
    """One kernel form: the template arguments (KS, S, KC, WN x WM waves, NT, MS, NE), `tn` = several images per tile, `dil2` = the
    zero-dilated input (the data gradient of a stride-2 conv, the forward of a transposed conv)."""
    return f"k{f.ks}s{f.s}_kc{f.kc}_w{f.wn}x{f.wm}_nt{f.nt}_ms{f.ms}_ne{f.ne}" + ("_tn" if f.tn > 1 else "") + ("_dil2" if f.dil == 2 else "")


def partials_rule(f, relu=False, res1=False, res2=False, up=0, nchw=False, cout=4):
    """The launcher's rule for the batch-statistics partials (conv_bn_part_ok with NTH = 256), restated: NTH % (NTILE / 4) == 0 and
    MT * (NTILE + 4) >= 8 * NTH, and the launch has no residual, ReLU, up-sampling or NCHW output, and a cout that is a multiple of 4."""
    mt, ntile = 16 * f.ms * f.wm, 16 * f.nt * f.wn
    return NTH % (ntile // 4) == 0 and mt * (ntile + 4) >= 8 * NTH and not (relu or res1 or res2 or up or nchw) and cout % 4 == 0


# ---- the sweep: a fixed domain that collects every form the dispatch can return ----
# Batches 1 .. 32 with 11 and 19 (more than one group of 8 / 16 images per tile, the last partly filled); the maps of the split sweep
# (tests/split_forms.py: 1 x 5 to 130 x 127 and 258 x 258, sizes that are no multiple of a tile, maps under 8 rows -- several images per
# tile) and a two-row map; cin 16 .. 256 with 16 and 48, which only this family takes (16-channel
# chunks, one and three of them); cout 16 .. 256 with a ragged last cout sub-tile (19, 20, 40), a partly empty cout group (80, 144), the W48
# class (48, 96, 144: three cout blocks per wave) and the at-most-32 class; 1x1 and 3x3 at stride 1 and 2 and the transposed conv.
SWEEP_N = (1, 2, 3, 5, 8, 11, 19, 32)
SWEEP_MAPS = ((1, 5), (1, 13), (1, 16), (2, 9), (3, 5), (4, 4), (4, 6), (5, 7), (7, 5), (8, 6), (8, 8), (9, 7), (12, 9), (13, 9), (16, 12), (16, 16), (17, 16),
              (20, 24), (24, 18), (23, 19), (5, 41), (9, 37), (17, 21), (32, 24), (32, 32), (33, 31), (48, 36), (47, 37), (64, 48), (64, 64), (96, 72),
              (128, 128), (129, 129), (130, 127), (6, 10), (10, 14), (18, 26), (34, 42), (66, 74), (258, 258))
SWEEP_CIN = (16, 32, 48, 64, 96, 256)
SWEEP_COUT = (16, 19, 20, 32, 40, 48, 64, 80, 96, 144, 256)
SWEEP_KERNELS = (("conv", 1, 1), ("conv", 1, 2), ("conv", 3, 1), ("conv", 3, 2), ("deconv", 4, 2))


def cost(n, cin, cout, h, w, k, stride, kind):
    """Floats of the device tensors of one case + multiply-adds / 64 of its float64 reference: what the smallest reaching shape minimises."""
    ho, wo = (2 * h, 2 * w) if kind == "deconv" else ((h - 1) // stride + 1, (w - 1) // stride + 1)
    taps = 4 if kind == "deconv" else k * k
    return n * (h * w * cin + ho * wo * cout) + n * ho * wo * cin * cout * taps // 64


@functools.lru_cache(maxsize=None)
def sweep(use):
    """{form name: [(kind, (n, cin, cout, h, w, k, stride), (th, tw, tn), bn_part), ...] by increasing cost} over the domain above for one
    use of the kernel (th x tw x tn: the tile the launch takes; bn_part: the launch keeps the batch-statistics partials).  The shape is the
    FORWARD conv's; for the data gradient the channel roles are swapped, so that the kernel's own cin and cout run over SWEEP_CIN and
    SWEEP_COUT."""
    found = {}
    for (kind, k, s), cin, cout, (h, w), n in itertools.product(SWEEP_KERNELS, SWEEP_CIN, SWEEP_COUT, SWEEP_MAPS, SWEEP_N):
        if use == "dgrad":
            cin, cout = cout, cin
        if n * h * w * max(cin, cout) * (4 if kind == "deconv" else 1) > 48 << 20:  # (192 MB of floats in one tensor)
            continue
        f = query(use, n, cin, cout, h, w, k, s, kind)
        if f is not None:
            found.setdefault(name(f), []).append((kind, (n, cin, cout, h, w, k, s), (f.th, f.tw, f.tn), int(f.bn_part)))
    for v in found.values():
        v.sort(key=lambda c: cost(*c[1], c[0]))
    return found


def kernel_channels(use, shape):
    """(cin, cout) of the conv the kernel runs: the data gradient has the forward conv's channel roles swapped."""
    return (shape[2], shape[1]) if use == "dgrad" else (shape[1], shape[2])


def grid_hw(use, kind, shape):
    """The pixel grid a launch tiles: the conv's output (twice the input of a transposed conv); dx for the data gradient."""
    h, w, s = shape[3], shape[4], shape[6]
    if use == "dgrad":
        return h, w
    return (2 * h, 2 * w) if kind == "deconv" else ((h - 1) // s + 1, (w - 1) // s + 1)


def ragged(use, kind, shape, tile):
    """(rows, columns): does the map leave a partly filled last tile in that direction?"""
    ho, wo = grid_hw(use, kind, shape)
    return bool(ho % tile[0]), bool(wo % tile[1])

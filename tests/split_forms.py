"""The kernel forms of the split-MFMA conv (csrc/conv_mfma_split.hip) as the library's own dispatch reports them (mval_conv_split_form:
host arithmetic, no GPU), for tests/test_gpu_split_forms.py: a name for every form, and the fixed sweep that collects every form the
dispatch can return for each way the library uses the kernel."""
import functools
import itertools

ALGO_MFMA, ALGO_MFMA_BF3, ALGO_MFMA_H2 = 1, 2, 3
OP_CONV, OP_DECONV = 0, 2
ALGO_OF = {"bf3": ALGO_MFMA_BF3, "h2": ALGO_MFMA_H2}
USES = ("fwd", "train", "dgrad", "parity")
VARIANT = {0: "ne6", 1: "ne10", 2: "rows", 3: "g2"}  # MVAL_SPLIT_NE6 / _NE10 / _ROW_SHARING / _TWO_CHUNK


def query(use, split, n, cin, cout, h, w, k, stride, kind="conv", relu=False, res1=False, res2=False, up=0, nchw=False):
    """The SplitForm of one launch, or None where the library has no split kernel for it.  (n, cin, cout, h, w, k, stride) describe the
    forward conv on an h x w input (pad k // 2), or ConvTranspose2d(k4, s2, p1) for kind "deconv"; use "fwd": mval_op_launch, "train":
    the conv of mval_train_forward, "dgrad" / "parity": mval_conv_dgrad_scaled / mval_conv_dgrad_parity of that conv (res1: accumulate)."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    if kind == "deconv":
        assert (k, stride) == (4, 2)
        pad, hout, wout = 1, 2 * h, 2 * w
    else:
        pad = k // 2
        hout, wout = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    op = _query_op(OP_DECONV if kind == "deconv" else OP_CONV, k, stride, pad, cin, cout, h, w, hout, wout, up=up, relu=int(relu), out_nchw=int(nchw),
                   res1_off=0 if res1 else -1, res2_off=0 if res2 else -1, algo=ALGO_OF[split])
    return _lib.conv_split_form(USES.index(use), op, n, ALGO_OF[split])


def name(f, dil=1):
    """One kernel form: the template arguments (PL, KS, S, WN x WM waves, NT, MS), the variant (6 / 10 staging slots, row sharing, two
    chunks per stage), the tile kind (power of two, odd, several images per tile), `precise`; `dil` 2 = the zero-dilated data gradient."""
    tile = "odd" if f.odd else "tn" if f.tn > 1 else "pow2"
    return (f"{'h2' if f.pl == 2 else 'bf3'}_k{f.ks}s{f.s}_w{f.wn}x{f.wm}_nt{f.nt}_ms{f.ms}_{VARIANT[f.variant]}_{tile}" + ("_precise" if f.precise else "") +
            ("_dil2" if dil == 2 else ""))


def partials_rule(f, relu=False, res1=False, res2=False, up=0, nchw=False, cout=4):
    """The launcher's rule for the batch-statistics partials, restated: NTH % (NTILE / 4) == 0 and MT * (NTILE + 4) >= 8 * NTH, and the launch
    has no residual, ReLU, up-sampling, NCHW output (or a cout that is no multiple of 4: the scalar store path) or parity grid."""
    mt, ntile, nth = 16 * f.ms * f.wm, 16 * f.nt * f.wn, 64 * f.wn * f.wm
    return (nth % (ntile // 4) == 0 and mt * (ntile + 4) >= 8 * nth and not (relu or res1 or res2 or up or nchw) and cout % 4 == 0 and f.grid_z == 1)


# ---- the sweep: a fixed domain that collects every form the dispatch can return ----
# Batches 1 .. 32; maps from 1 x 5 to 128 x 128 (and 129 x 129 / 130 x 127: ragged maps on which 8 images pass the 128 Ki-pixel threshold of
# the 128-pixel tiles), with sizes that are no multiple of any tile (one-row maps narrower than a tile; 5 x 41, 9 x 37 and 17 x 21, which odd
# tiles do not divide either; even sizes from 6 x 10 to 258 x 258 whose halves -- the parity grids of the stride-2 data gradient -- are odd)
# and maps under 8 rows (several images per tile); cin 32 .. 256 with 48 (a
# half-empty second chunk) and 96 (an odd number of chunks: no two-chunk stage); cout 16 .. 256 with values that leave a ragged last cout
# sub-tile (19, 20, 40), a partly empty cout group (80, 144) and three cout waves (48, 96, 144); 1x1, stride-2 1x1, 3x3 stride 1 and 2 and
# the transposed conv (four 2x2 parity convs); both splits.
SWEEP_N = (1, 2, 3, 5, 8, 32)
SWEEP_MAPS = ((1, 5), (1, 13), (1, 16), (3, 5), (4, 4), (4, 6), (5, 7), (7, 5), (8, 6), (8, 8), (9, 7), (12, 9), (13, 9), (16, 12), (16, 16), (17, 16), (20, 24), (24, 18),
              (23, 19), (5, 41), (9, 37), (17, 21), (32, 24), (32, 32), (33, 31), (48, 36), (47, 37), (64, 48), (64, 64), (96, 72), (128, 128),
              (129, 129), (130, 127), (6, 10), (10, 14), (18, 26), (34, 42), (66, 74), (258, 258))
SWEEP_CIN = (32, 48, 64, 96, 256)
SWEEP_COUT = (16, 19, 20, 32, 40, 48, 64, 80, 96, 128, 144, 192, 256)
SWEEP_KERNELS = (("conv", 1, 1), ("conv", 1, 2), ("conv", 3, 1), ("conv", 3, 2), ("deconv", 4, 2))


def cost(n, cin, cout, h, w, k, stride, kind):
    """Floats of the device tensors of one case + multiply-adds / 64 of its float64 reference: what the smallest reaching shape minimises."""
    ho, wo = (2 * h, 2 * w) if kind == "deconv" else ((h - 1) // stride + 1, (w - 1) // stride + 1)
    taps = 4 if kind == "deconv" else k * k
    return n * (h * w * cin + ho * wo * cout) + n * ho * wo * cin * cout * taps // 64


@functools.lru_cache(maxsize=None)
def sweep(use):
    """{form name: [(split, kind, (n, cin, cout, h, w, k, stride), (th, tw, tn)), ...] by increasing cost} over the domain above for one use of
    the kernel (th x tw x tn: the tile the launch takes)."""
    found = {}
    for split, (kind, k, s), cin, cout, (h, w), n in itertools.product(("bf3", "h2"), SWEEP_KERNELS, SWEEP_CIN, SWEEP_COUT, SWEEP_MAPS, SWEEP_N):
        if use == "parity" and (kind, k, s) != ("conv", 3, 2):
            continue
        if use in ("train", "dgrad") and kind != "conv":
            continue
        if use in ("dgrad", "parity"):  # (the data gradient's conv has the channel roles swapped: its cout is the conv's cin)
            cin, cout = cout, cin
        if n * h * w * max(cin, cout) * (4 if kind == "deconv" else 1) > 48 << 20:  # (192 MB of floats in one tensor)
            continue
        f = query(use, split, n, cin, cout, h, w, k, s, kind)
        if f is not None:
            found.setdefault(name(f, s if use == "dgrad" else 1), []).append((split, kind, (n, cin, cout, h, w, k, s), (f.th, f.tw, f.tn)))
    for v in found.values():
        v.sort(key=lambda c: cost(*c[2], c[1]))
    return found


def grid_hw(use, kind, shape):
    """The pixel grid a launch tiles: the conv's output; the input grid of a transposed conv; dx, or one parity of it."""
    h, w, s = shape[3], shape[4], shape[6]
    if use == "dgrad":
        return h, w
    if use == "parity":
        return h // 2, w // 2
    return (h, w) if kind == "deconv" else ((h - 1) // s + 1, (w - 1) // s + 1)


def ragged(use, kind, shape, tile):
    """(rows, columns): does the map leave a partly filled last tile in that direction?"""
    ho, wo = grid_hw(use, kind, shape)
    return bool(ho % tile[0]), bool(wo % tile[1])

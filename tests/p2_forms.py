"""The kernel forms of the P2 conv (csrc/conv_p2.hip: conv_p2_kernel, every conv of the default inference and training plans) as the library's
own dispatch reports them (mval_conv_p2_form: the launcher's dry run, host arithmetic, no GPU), for tests/test_gpu_p2_forms.py: a name for
every pair of kernel instance and runtime path, and the fixed sweep that collects every form the dispatch can return for each way the library
uses the kernel."""
import functools
import itertools

from mfma_forms import cost

ALGO_P2 = 4
OP_CONV, OP_DECONV = 0, 2
USES = ("op", "train", "dgrad")  # MVAL_SPLIT_USE_OP / _TRAIN_FWD / _DGRAD


def query(use, n, cin, cout, h, w, k, stride, kind="conv", relu=False, res1=False, res2=False, up=0, nchw=False, inz=False):
    """The P2Form of one launch, or None where the library has no P2 kernel for it.  (n, cin, cout, h, w, k, stride) describe the forward conv
    on an h x w input (pad k // 2), or ConvTranspose2d(k4, s2, p1) for kind "deconv" -- answered with the 2 x 2 parity conv that is launched four
    times; use "op": mval_op_launch, "train": the conv of mval_train_forward (inz: the form that applies its producer's BatchNorm + ReLU
    while staging), "dgrad": the data gradient mval_train_backward runs on these kernels (res1: accumulate)."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    if kind == "deconv":
        assert (k, stride) == (4, 2)
        pad, hout, wout = 1, 2 * h, 2 * w
    else:
        pad = k // 2
        hout, wout = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    # (the offsets only have to name buffers: mval_op_launch's argument builder refuses an op without them)
    op = _query_op(OP_DECONV if kind == "deconv" else OP_CONV, k, stride, pad, cin, cout, h, w, hout, wout, up=up, relu=int(relu), out_nchw=int(nchw),
                   algo=ALGO_P2, in_off=0, out_off=0, w_off=0, scale_off=0, shift_off=0, bound_off=0, in_amax_off=1, out_amax_off=1,
                   res1_off=(-2 if inz else 0 if res1 else -1), res1_amax_off=1, res2_off=0 if res2 else -1, res2_amax_off=1)
    return _lib.conv_p2_form(USES.index(use), op, n)


def name(f):
    """One kernel form: the template arguments (KS, S, G chunks per stage, WN x WM waves, NT, MS, the tile width -- `tw` a power of two, `ow`
    an odd tile --, the epilogue), `rs` = row sharing, `k48` = the paired remainder of 48 input channels, `inz` / `bsum` = the training
    instances, and the runtime path: `flat` = the H x W map of a 1x1 conv run as one row, `sub` = every second input pixel (a stride-2 1x1
    conv), `par` = one of the four parity launches of a transposed conv."""
    return (f"k{f.ks}s{f.s}_g{f.g}_w{f.wn}x{f.wm}_nt{f.nt}_ms{f.ms}_" + (f"ow{f.ow}" if f.ow else f"tw{f.tw}") + f"_e{f.epi}" + ("_rs" if f.rs else "") +
            ("_k48" if f.k48 else "") + ("_inz" if f.inz else "") + ("_bsum" if f.bsum else "") + ("_flat" if f.flat else "") +
            ("_sub" if f.in_sub else "") + ("_par" if f.parities > 1 else ""))


def opts(text):
    """"relu+res1+up2" -> the keyword arguments of query (`mag`, a data option of the GPU rows, is not one of them)."""
    t = set(text.split("+")) - {"", "mag"}
    up = [int(x[2:]) for x in t if x.startswith("up")]
    assert t <= {"relu", "res1", "res2", "nchw", "inz", "up1", "up2", "up3"}, text
    d = dict(relu="relu" in t, res1="res1" in t, res2="res2" in t, nchw="nchw" in t, up=up[0] if up else 0)
    if "inz" in t:
        d["inz"] = True
    return d


# ---- the sweep: a fixed domain that collects every form the dispatch can return ----
# Widths: those the dispatch names (6, 8, 9, 12, 18, 24, 36, 72 -- as stride-2 outputs too: 12 -> 6, 24 -> 12, 36 -> 18, 72 -> 36), the multiples
# of 16 up to 128, and widths that fit none of these (5, 7, 10, 13, 20, 37, 100).  Heights that do and do not satisfy the `% 4` and `% 8`
# conditions, at stride 1 and as stride-2 outputs (4, 5, 7, 8, 12 -- the 12 x 9 whole-map form --, 13, 16, 24, 33, 64).  Couts 8 .. 256 with the
# ragged last cout sub-tile (8, 24, 40; 19: fp32 NCHW output only); cins 8 .. 256 with a partly filled last 32-channel chunk (8, 40, 72), the
# K48 class (48) and chunk counts two does not divide (96, 72).  Batches 1 .. 3 everywhere and 8 .. 64 on the 1x1 convs of 128 and 256 couts:
# the NT = 2 rule ((px + 63) / 64) * (NS / 8) >= 1024 is reached by cout 256 on 64 x 64 at n = 8, by its stride-2 form on 32 x 32 outputs at 32.
# The epilogue options: none, up 1 .. 3 and NCHW output on the 1x1 convs (the only ones that have them), residuals.
# The full product would be some millions of queries; the form depends on cin only through `== 48`, `>= 64` and the channel limits, on the batch
# only through the NT rule and on the residuals not at all (the parity conv refuses them), so the domain is the union of the products below.
SWEEP_W = (5, 6, 7, 8, 9, 10, 12, 13, 16, 18, 20, 24, 32, 36, 37, 48, 64, 72, 80, 96, 100, 112, 128)
SWEEP_H = (4, 5, 7, 8, 12, 13, 16, 24, 33, 64)
SWEEP_LOW = ((1, 32), (1, 40), (1, 48), (2, 16), (2, 24))  # (one or two rows, under 64 pixels: 1x1 maps that are NOT run as one flattened row)
SWEEP_MAPS = tuple(itertools.product(SWEEP_H, SWEEP_W)) + SWEEP_LOW
SWEEP_MAPS_FEW = ((4, 8), (8, 6), (12, 9), (8, 12), (16, 18), (24, 36), (16, 72), (13, 16), (33, 37), (64, 64))
SWEEP_CIN = (8, 32, 40, 48, 64, 72, 96, 128, 256)
SWEEP_CIN_FEW = (32, 48, 64)
SWEEP_COUT = (8, 24, 32, 40, 48, 96, 128, 192, 256)  # (+ 19 with NCHW output)
SWEEP_KERNELS = (("conv", 1, 1), ("conv", 1, 2), ("conv", 3, 1), ("conv", 3, 2), ("deconv", 4, 2))
K1 = SWEEP_KERNELS[:2]


def _domain(use):
    """(kernel, cin, cout, map, n, options) of every query of the sweep for one use."""
    P = itertools.product
    if use == "op":
        yield from P(SWEEP_KERNELS, SWEEP_CIN_FEW, SWEEP_COUT, SWEEP_MAPS, (1, 2, 3), ("",))
        yield from P(SWEEP_KERNELS, SWEEP_CIN, SWEEP_COUT, SWEEP_MAPS, (2, 3), ("",))
        yield from P(K1, SWEEP_CIN_FEW, SWEEP_COUT + (19,), SWEEP_MAPS, (1,), ("up1", "nchw"))
        yield from P(K1, SWEEP_CIN, SWEEP_COUT + (19,), SWEEP_MAPS, (2,), ("up1", "nchw"))
        yield from P(K1, (32, 40, 96), (128, 256), SWEEP_MAPS, (8, 16, 32, 64), ("", "up1"))
        yield from P(SWEEP_KERNELS, SWEEP_CIN, SWEEP_COUT + (19,), SWEEP_MAPS_FEW, (2,), ("up2", "up3", "nchw", "res1", "res1+res2", "relu+res1"))
    elif use == "train":
        yield from P(SWEEP_KERNELS[:4], SWEEP_CIN_FEW, SWEEP_COUT, SWEEP_MAPS, (1, 2, 3), ("", "inz"))
        yield from P(SWEEP_KERNELS[:4], SWEEP_CIN, SWEEP_COUT, SWEEP_MAPS, (2,), ("", "inz"))
        yield from P(K1, SWEEP_CIN_FEW, (128, 256), SWEEP_MAPS, (8, 16), ("",))
    else:  # (the data gradient of a stride-1 conv; the kernel's own cin is the conv's cout)
        yield from P((SWEEP_KERNELS[0], SWEEP_KERNELS[2]), SWEEP_COUT, SWEEP_CIN_FEW, SWEEP_MAPS, (1, 2, 3), ("", "res1"))
        yield from P((SWEEP_KERNELS[0], SWEEP_KERNELS[2]), SWEEP_COUT, SWEEP_CIN, SWEEP_MAPS, (2,), ("",))
        yield from P((SWEEP_KERNELS[0],), (128, 256), SWEEP_CIN_FEW, SWEEP_MAPS, (8, 16), ("",))


@functools.lru_cache(maxsize=None)
def sweep(use):
    """{form name: [(kind, (n, cin, cout, h, w, k, stride), options, (th, tile_w)), ...] by increasing cost} over the domain above for one use
    of the kernel.  The shape is the FORWARD conv's; the data gradient's domain has the channel roles swapped, so that the kernel's own cin
    and cout run over SWEEP_CIN and SWEEP_COUT."""
    found, seen = {}, set()
    for (kind, k, s), cin, cout, (h, w), n, o in _domain(use):
        key = (kind, (n, cin, cout, h, w, k, s), o)
        if key in seen or (cout == 19 and "nchw" not in o) or (k != 1 and "up" in o):
            continue
        if n * h * w * max(cin, cout) * (4 if kind == "deconv" else 1) > 48 << 20:  # (192 MB of floats in one tensor)
            continue
        seen.add(key)
        f = query(use, n, cin, cout, h, w, k, s, kind, **opts(o))
        if f is not None:
            found.setdefault(name(f), []).append(key + ((f.th, f.tile_w),))
    for v in found.values():
        v.sort(key=lambda c: cost(*c[1], c[0]))
    return found


def grid_hw(use, kind, shape):
    """The pixel grid a launch tiles: the conv's output before the up-sampling (the INPUT grid of a transposed conv: one parity); dx for the
    data gradient."""
    h, w, s = shape[3], shape[4], shape[6]
    if use == "dgrad" or kind == "deconv":
        return h, w
    return (h - 1) // s + 1, (w - 1) // s + 1


def ragged(use, kind, shape, f):
    """(rows, columns): does the map leave a partly filled last tile in that direction?  (A flattened map is one row of H * W pixels.)"""
    ho, wo = grid_hw(use, kind, shape)
    if f.flat:
        return False, bool((ho * wo) % f.tile_w)
    return bool(ho % f.th), bool(wo % f.tile_w)


def resident_cap(f, cus):
    """R_max: the most workgroups of the form the device can hold whatever the occupancy query answers -- per CU at most 32 waves and
    160 KiB of LDS.  A launch with tiles_total * groups above it has a workgroup that walks two tiles or more."""
    return cus * min(32 // (f.threads // 64), (160 * 1024) // f.smem_bytes)

"""The training C entries that only whole training steps reached, each against float64 conv autograd on the CPU (the bound of
test_gpu_train.py::test_conv_wgrad_and_dgrad_vs_torch: relative L2 < 2e-5, above the fp16x2 split's 2^-22 per operand):
mval_conv_wgrad_scaled with both magnitude rows over the ten tile forms of the split kernel, mval_conv_dgrad_scaled on the fp16-split
kernels, mval_conv_wgrad on the exact-fp32 kernel's 1x1 stride-2 and k4 s2 p1 forms, and mval_slab_reduce."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tiny_graphs as tg

gpu = pytest.mark.gpu

ALGO_MFMA_H2, PACK_MFMA16_H2 = 3, 3
ROW = 576  # dwords of a training magnitude row: [count, <= 512 partial maxima] (engine_train.TRAIN_AMAX_ROW)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _row(t, dev):
    """[count = 3, partials]: two partials below the tensor's maximum, the maximum itself in the LAST one (a reader that stops early
    scales by too small a value and overflows fp16)."""
    mx = float(t.abs().max())
    row = torch.zeros(ROW, dtype=torch.int32)
    row[0] = 3
    for i, v in enumerate((mx / 64.0, mx / 8.0, mx)):
        row[1 + i] = int(np.float32(v).view(np.int32))
    return row.to(dev)


def _nhwc(t, dev):
    return t.detach().permute(0, 2, 3, 1).contiguous().to(torch.float32).to(dev)


def _conv_grads(n, cin, cout, h, w, k, s, pad, seed, x_scale=1.0, dz_scale=1.0):
    """x, dz (float32 values, scaled by powers of two) and the float64 autograd gradients of y = conv2d(x, wt, stride s, padding pad)."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32) * np.float32(x_scale))
    wt = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) * 0.1).astype(np.float32))
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv2d(x64, w64, None, stride=s, padding=pad)
    dz = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32) * np.float32(dz_scale))
    y.backward(dz.double())
    return x, wt, dz, x64.grad.numpy(), w64.grad.numpy()


def _wgrad(dev, x, dz, cin, cout, k, s, pad, rows):
    from multi_view_active_learning_amd import _lib

    lib, st, p = _lib.lib(), _lib._stream(), _lib._p
    n, _, h, w = x.shape
    ho, wo = dz.shape[2:]
    xd, dzd = _nhwc(x, dev), _nhwc(dz, dev)
    lib.mval_conv_wgrad_workspace_floats.restype = C.c_size_t
    ws = torch.empty(int(lib.mval_conv_wgrad_workspace_floats(C.c_int(cin), C.c_int(cout), C.c_int(k))) + 64, device=dev)
    dw = torch.full((cout, cin, k, k), 7.0, device=dev)
    geo = (C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(cin), C.c_int(ho), C.c_int(wo), C.c_int(cout), C.c_int(k), C.c_int(s), C.c_int(pad), C.c_int(0))
    if rows:
        xr, zr = _row(x, dev), _row(dz, dev)
        _lib._check(lib.mval_conv_wgrad_scaled(p(xd), p(dzd), p(dw), p(ws), *geo, p(xr), p(zr), st), "wgrad scaled")
    else:
        _lib._check(lib.mval_conv_wgrad(p(xd), p(dzd), p(dw), p(ws), *geo, st), "wgrad")
    return dw.cpu().numpy()


# ((n, cin, cout, h, w, k, stride), the tile form (k, stride, tw, NT) the case is in the table for, id).  mval_launch_wgrad_bf3_p2 takes 16-wide
# tiles when Wout > 8 and they pad no more columns than 8-wide ones, NT = 2 cout tiles per wave when cout > 32 (always for 1x1); 64-pixel tiles
# at stride 1, 32-pixel tiles at stride 2.  test_wgrad_scaled_cases_name_all_ten_tile_forms holds every row to the launcher's rule.
WGS_CASES = [
    ((2, 64, 64, 8, 16, 1, 1), (1, 1, 16, 2), "k1_tw16"),
    ((2, 64, 128, 12, 18, 1, 1), (1, 1, 8, 2), "k1_tw8_ragged_w"),
    ((2, 32, 32, 16, 30, 3, 1), (3, 1, 16, 1), "k3s1_tw16_nt1_ragged_w"),
    ((2, 48, 48, 5, 16, 3, 1), (3, 1, 16, 2), "k3s1_tw16_nt2_c48_ragged_h"),
    ((2, 20, 32, 12, 18, 3, 1), (3, 1, 8, 1), "k3s1_tw8_nt1_cin20"),
    ((2, 32, 64, 9, 21, 3, 1), (3, 1, 8, 2), "k3s1_tw8_nt2_odd"),
    ((2, 32, 32, 12, 32, 3, 2), (3, 2, 16, 1), "k3s2_tw16_nt1"),
    ((2, 48, 48, 10, 31, 3, 2), (3, 2, 16, 2), "k3s2_tw16_nt2_c48_odd_in"),
    ((2, 20, 32, 18, 24, 3, 2), (3, 2, 16, 1), "k3s2_tw16_nt1_cin20_wout12"),
    ((2, 20, 32, 14, 16, 3, 2), (3, 2, 8, 1), "k3s2_tw8_nt1_cin20_wout8"),
    ((3, 32, 64, 13, 37, 3, 2), (3, 2, 8, 2), "k3s2_tw8_nt2_odd_wout19"),
    ((2, 48, 32, 9, 11, 3, 2), (3, 2, 8, 1), "k3s2_tw8_nt1_c48_wout6_ragged"),
    ((2, 64, 64, 4, 6, 3, 1), (3, 1, 8, 2), "k3s1_map_below_tile"),
    ((9, 32, 32, 64, 64, 3, 1), (3, 1, 16, 1), "k3s1_split_k_576_tiles"),  # 9 x 16 x 4 tiles of 4 x 16 pixels > 512 slabs: the tile loop iterates
]


def test_wgrad_scaled_cases_name_all_ten_tile_forms():
    """No GPU: every row of WGS_CASES takes the tile form it is in the table for under the launcher's own rule (tiny_graphs.wgrad_tile), and
    the rows together name all ten forms of mval_launch_wgrad_bf3_p2."""
    for (n, cin, cout, h, w, k, s), form, name in WGS_CASES:
        wout = (w + 2 * (k // 2) - k) // s + 1
        assert tg.wgrad_tile(k, s, wout, cout) == form, (name, wout)
    assert {form for _, form, _ in WGS_CASES} == tg.WGRAD_TILE_FORMS and len(tg.WGRAD_TILE_FORMS) == 10


@gpu
@pytest.mark.parametrize("case", [c for c, _, _ in WGS_CASES], ids=[i for _, _, i in WGS_CASES])
def test_conv_wgrad_scaled_with_magnitude_rows_vs_float64(dev, case):
    """The fp16x2 form of the split weight gradient (PL = 2: both magnitude rows given) on every tile form, ragged channel counts (48, cin 20),
    ragged tiles and the split-K loop; x scaled by 2^10 and dz by 2^-12 so that a wrong `unscale` (or a row read short of its last
    partial) cannot pass."""
    n, cin, cout, h, w, k, s = case
    x, wt, dz, _, dw64 = _conv_grads(n, cin, cout, h, w, k, s, k // 2, 11, x_scale=2.0 ** 10, dz_scale=2.0 ** -12)
    got = _wgrad(dev, x, dz, cin, cout, k, s, k // 2, rows=True)
    e = _rel(got, dw64)
    print(f"[wgrad scaled] {case}: rel L2 {e:.2e}")
    assert e < 2e-5, e


# (n, cin, cout, h, w, k, stride, pad) in the conv's terms.  1x1 stride 2: a Bottleneck's strided projection shortcut (WG_LAUNCH(1, 2, 64, 8));
# k4 s2 p1: the weight gradient of ConvTranspose2d(k4, s2, p1) with the activations' roles swapped -- x is the transposed conv's dz (16 x 12,
# its cout channels), dz its 8 x 6 input (its cin channels): the transposed convs 64 -> 32 and 256 -> 256 are cin 32 / cout 64 and 256 / 256
# in these conv terms (WG_LAUNCH(4, 2, 64, 12)).  Neither is a shape of the split kernel, so mval_conv_wgrad runs the exact-fp32 kernel.
WGX_CASES = [(2, 64, 128, 17, 24, 1, 2, 0), (3, 256, 512, 8, 6, 1, 2, 0), (2, 32, 64, 16, 12, 4, 2, 1), (2, 256, 256, 16, 12, 4, 2, 1)]


@gpu
@pytest.mark.parametrize("case", WGX_CASES, ids=lambda c: "n%d_c%d-%d_%dx%d_k%ds%dp%d" % c)
def test_conv_wgrad_exact_kernel_strided_forms_vs_float64(dev, case):
    n, cin, cout, h, w, k, s, pad = case
    x, wt, dz, _, dw64 = _conv_grads(n, cin, cout, h, w, k, s, pad, 12)
    assert tuple(dz.shape[2:]) == ((h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1)
    got = _wgrad(dev, x, dz, cin, cout, k, s, pad, rows=False)
    e = _rel(got, dw64)
    print(f"[wgrad exact] {case}: rel L2 {e:.2e}")
    assert e < 2e-5, e


# (n, cin, cout, h, w, k): stride-1 convs whose data gradient the training plans run on the fp16-split kernel
DG_CASES = [(2, 32, 32, 16, 16, 3), (2, 48, 48, 12, 18, 3), (3, 32, 64, 9, 7, 3), (2, 64, 64, 16, 16, 1), (2, 96, 32, 4, 4, 1), (2, 64, 256, 12, 18, 1)]


@gpu
@pytest.mark.parametrize("case", DG_CASES, ids=lambda c: "n%d_c%d-%d_%dx%d_k%d" % c)
def test_conv_dgrad_scaled_h2_vs_float64(dev, case):
    """mval_conv_dgrad_scaled, MVAL_ALGO_MFMA_H2 (weights packed MVAL_PACK_MFMA16_H2, dz's magnitude row), stride 1, k1 and k3: store (over
    stale contents) and accumulate."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import _query_op

    n, cin, cout, h, w, k = case
    x, wt, dz, dx64, _ = _conv_grads(n, cin, cout, h, w, k, 1, k // 2, 13, dz_scale=2.0 ** -9)
    lib, st, p = _lib.lib(), _lib._stream(), _lib._p
    d = _query_op(0, k, 1, k - 1 - k // 2, cout, cin, h, w, h, w)
    assert lib.mval_op_algo_supported(C.byref(d), C.c_int(n), C.c_int(ALGO_MFMA_H2)), "the case must be one the fp16-split kernel covers"
    lib.mval_packed_weight_floats.restype = C.c_size_t
    nw = int(lib.mval_packed_weight_floats(C.c_int(PACK_MFMA16_H2), C.c_int(cin), C.c_int(cout), C.c_int(k)))
    wp = torch.empty(nw, dtype=torch.float32, device=dev)
    wd = wt.contiguous().to(dev)
    _lib._check(lib.mval_pack_conv_weights(C.c_int(PACK_MFMA16_H2), C.c_int(2), p(wd), p(wp), C.c_int(cin), C.c_int(cout), C.c_int(k), st), "pack")
    ones = torch.ones(max(cin, cout), dtype=torch.float32, device=dev)
    zeros = torch.zeros_like(ones)
    dzd, row = _nhwc(dz, dev), _row(dz, dev)
    want = np.transpose(dx64, (0, 2, 3, 1))
    base = torch.from_numpy(np.random.default_rng(14).standard_normal((n, h, w, cin)).astype(np.float32) * np.float32(np.abs(want).max())).to(dev)
    for acc in (0, 1):
        dx = base.clone()
        _lib._check(lib.mval_conv_dgrad_scaled(p(dzd), p(wp), p(ones), p(zeros), p(dx), C.c_int(acc), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(cin),
                                               C.c_int(h), C.c_int(w), C.c_int(cout), C.c_int(k), C.c_int(1), C.c_int(k // 2), C.c_int(ALGO_MFMA_H2),
                                               p(row), st), "dgrad scaled")
        got = dx.cpu().numpy().astype(np.float64) - (base.cpu().numpy().astype(np.float64) if acc else 0.0)
        e = _rel(got, want)
        print(f"[dgrad scaled] {case} accumulate={acc}: rel L2 {e:.2e}")
        # (accumulate: the sum is rounded once more to float32, relative to base + dx: 2^-24 * |base + dx| / |dx| <= 2e-7 here)
        assert e < 2e-5, (acc, e)


@gpu
@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("s", [1, 7, 512])
def test_slab_reduce_vs_float64(dev, s, n):
    """mval_slab_reduce: out (+)= the sum of S slabs of n floats, accumulated in float64 (one rounding to float32, a second one when it
    accumulates): 1e-6 relative to the float64 sum."""
    from multi_view_active_learning_amd import _lib

    lib, st, p = _lib.lib(), _lib._stream(), _lib._p
    rng = np.random.default_rng(100 * s + n)
    slabs = (rng.standard_normal((s, n)) * 2.0 ** rng.integers(-8, 8, size=(s, 1))).astype(np.float32)
    out0 = rng.standard_normal(n).astype(np.float32)
    sd = torch.from_numpy(slabs).to(dev)
    want = slabs.astype(np.float64).sum(0)
    for acc in (0, 1):
        out = torch.from_numpy(out0).to(dev).clone()
        _lib._check(lib.mval_slab_reduce(p(sd), C.c_int(s), C.c_int64(n), p(out), C.c_int(acc), st), "slab reduce")
        ref = want + (out0.astype(np.float64) if acc else 0.0)
        assert _rel(out.cpu().numpy(), ref) < 1e-6, (s, n, acc)

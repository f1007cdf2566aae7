"""The plain VALU operators that open every network, each alone against a float64 torch-CPU reference of the same operation: the stem
kernels conv_stem_kernel<3> / <7> and their fallback conv_direct_kernel on NCHW input, maxpool_kernel with amax_kernel behind it,
deconv_direct_kernel, the stem and direct weight-gradient kernels with wgrad_reduce_kernel, and maxpool_bwd_kernel.

tests/plain_ops.py holds the case tables and says what each row is in them for.  The host test holds every row to the kernel it names (by the
library's own no-launch queries mval_conv_stem_covers and mval_conv_wgrad_path) and the tables together to every kernel and branch of
plain_ops.REQUIRED.  The GPU tests repeat the query on the shape they run.

Bounds.  Convs (sections 1 and 3): K products accumulated by fma in some order, then one multiply-add, so elementwise
    |got - want64| <= (K + 4) * 2^-24 * (|scale| * conv(|x|, |w|) + |shift|),
the second factor in float64; the ReLU is 1-Lipschitz, so the bound holds behind it.  Max-pool forward: exact.  Kept magnitude rows: exact.
Weight gradients: the project's bound for these kernels, relative L2 < 2e-5 (test_gpu_train.py).  Max-pool backward: at most four routed
gradients summed in fp32, |got - want64| <= 4 * 2^-24 * r with r the same backward applied to |gout|; exact zero where r = 0."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plain_ops as po

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
ids = lambda cases: [c[0] for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from multi_view_active_learning_amd import _lib

    _lib.lib()
    return torch.device("cuda:0")


def _stem_kernel_of(case):
    from multi_view_active_learning_amd import _lib

    return int(_lib.lib().mval_conv_stem_covers(C.byref(po.stem_op(case))))


def _wgrad_path_of(case):
    from multi_view_active_learning_amd import _lib

    _, (n, cin, cout, h, w), k, stride, pad, x_nchw, _ = case
    return po.WGRAD_PATHS[int(_lib.lib().mval_conv_wgrad_path(C.c_int(cin), C.c_int(cout), C.c_int(k), C.c_int(stride), C.c_int(pad), C.c_int(x_nchw)))]


def test_plain_op_rows_name_their_kernels_and_reach_every_branch():
    """No GPU: every table row runs on the kernel it names, under the library's own predicates and under the rules restated in plain_ops;
    the tile and slab counts the rows are chosen for hold; the tables together reach every kernel and branch of plain_ops.REQUIRED."""
    text = open(os.path.join(REPO, "include", "mval_hip.h")).read()
    assert re.search(r"int mval_conv_stem_covers\(const mval_op\* op\);", text)
    assert re.search(r"int mval_conv_wgrad_path\(int cin, int cout, int k, int stride, int pad, int x_nchw\);", text)
    assert [int(re.search(r"\bMVAL_WGRAD_%s\s*=\s*(\d+)" % p.upper(), text).group(1)) for p in po.WGRAD_PATHS] == list(range(5))
    for table in (po.STEM_CASES, po.POOL_CASES, po.AMAX_CASES, po.DECONV_CASES, po.WGRAD_CASES, po.POOLB_CASES):
        assert len({c[0] for c in table}) == len(table)
    # the stem forward
    for case in po.STEM_CASES:
        name, (n, cout, h, w), k, stride, pad, opt, kernel = case
        want = int(kernel[4:]) if kernel.startswith("stem") else 0
        assert po.stem_rule(cout, k, stride, pad, "no_stem" in opt) == want, name
        assert _stem_kernel_of(case) == want, name
    assert po.stem_lds_bytes(7, 92) == 63420 <= 64 * 1024 < po.stem_lds_bytes(7, 96) == 65772
    by_id = {c[0]: c for c in po.STEM_CASES}
    for k in (3, 7):
        assert po.out_hw(37, 51, k, 2, k // 2) == (19, 26)  # 3 of 8 rows in the last tile row, 10 of 16 columns in the last tile column
        assert {"ragged_y", "ragged_x", "odd_input"} <= po.stem_tags(by_id[f"odd_37x51_k{k}_relu"])
        assert "below_tile" in po.stem_tags(by_id[f"below_tile_5x9_k{k}_lin"]) and "relu_off" in po.stem_tags(by_id[f"five_quads_k{k}_lin"])
        assert "cout_pass_2" in po.stem_tags(by_id[f"cout68_k{k}"]) and "no_stem_fallback" in po.stem_tags(by_id[f"no_stem_k{k}"])
    assert "lds_fallback" in po.stem_tags(by_id["cout96_k7_lds_65772"]) and "cout_pass_2" in po.stem_tags(by_id["cout92_k7_lds_63420"])
    # the amax kernel behind the max-pool
    pool = {c[0]: po.pool_tags(c) for c in po.POOL_CASES}
    assert "amax_scalar" in pool["amax_scalar_54"] and {"amax_vector", "amax_second_trip"} <= pool["amax_second_trip"]
    amax = {name: po.amax_tags(per, aligned=off % 4 == 0) for name, _, per, off in po.AMAX_CASES}
    assert amax["off_by_4_bytes"] >= {"amax_scalar"} and amax["off_by_4_bytes_many_trips"] == {"amax_scalar", "amax_second_trip"}
    assert all(per % 4 == 0 for _, _, per, _ in po.AMAX_CASES)  # (off by four bytes is then the only reason for the scalar path)
    # the weight gradients
    for case in po.WGRAD_CASES:
        assert _wgrad_path_of(case) == case[-1], case[0]
    wg = {c[0]: c for c in po.WGRAD_CASES}
    for k in (3, 7):
        assert po.stem_wgrad_tiles(17, 128, 128, k) == 544 and po.wgrad_slabs(wg[f"stem{k}_544_tiles"]) == 512
        assert po.reduce_loops(po.wgrad_slabs(wg[f"stem{k}_544_tiles"])) == (16, {8})
        assert po.wgrad_slabs(wg[f"stem{k}_one_tile"]) == 1 and po.wgrad_slabs(wg[f"stem{k}_ps7"]) == 7
    assert po.reduce_loops(1) == (1, {1}) and po.reduce_loops(7) == (1, {4, 1})
    assert 9 * 3 * 96 == 2592 > po.WD_OUTPUTS_PER_ROW and "wgrad_direct_rows_2+" in po.wgrad_tags(wg["direct_nchw_cout96"])
    assert 9 * 128 * 128 == 147456 > po.WD_MAX_OUTPUTS == 64 * 2048
    assert po.wgrad_slabs(wg["direct_1x3_map"]) == 3
    # the max-pool backward
    assert 513 * 512 * 64 // 4 > po.POOLB_MAX_WORKGROUPS * 256 and "poolb_second_trip" in po.poolb_tags(po.POOLB_CASES[-1])
    missing = po.REQUIRED - po.all_tags()
    assert not missing, missing


# ---- 1. stem forward ----
def _conv_ref64(x, wt, sc, sh, stride, pad, relu, transposed=False):
    """(want, magnitude) in float64 (x NCHW): the fused operator, and |scale| * conv(|x|, |w|) + |shift| for the error bound."""
    conv = F.conv_transpose2d if transposed else F.conv2d
    sc64, sh64 = sc.double()[None, :, None, None], sh.double()[None, :, None, None]
    want = conv(x.double(), wt.double(), None, stride=stride, padding=pad) * sc64 + sh64
    mag = conv(x.double().abs(), wt.double().abs(), None, stride=stride, padding=pad) * sc64.abs() + sh64.abs()
    return (F.relu(want) if relu else want), mag


def _worst_ratio(got, want, bound):
    err = (got.double() - want).abs()
    assert bool(((bound > 0) | (err == 0)).all())
    return float((err / bound.clamp_min(1e-300)).max())


def _stem_data(case):
    name, (n, cout, h, w), k, stride, pad, opt, _ = case
    rng = np.random.default_rng(po.seed(name))
    x = rng.standard_normal((n, 3, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, 3, k, k)) * 0.2).astype(np.float32)
    sc = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
    sh = rng.standard_normal(cout).astype(np.float32)
    if "zero" in opt:
        x[-1] = 0.0
        sh = -np.abs(sh)
    if "relu" not in opt:
        sh = -np.abs(sh) - np.float32(4.0)
    return tuple(torch.from_numpy(a) for a in (x, wt, sc, sh))


@gpu
@pytest.mark.parametrize("case", po.STEM_CASES, ids=ids(po.STEM_CASES))
def test_stem_forward_vs_float64(dev, case, capsys):
    from multi_view_active_learning_amd import ops

    name, (n, cout, h, w), k, stride, pad, opt, kernel = case
    relu = "relu" in opt
    assert _stem_kernel_of(case) == (int(kernel[4:]) if kernel.startswith("stem") else 0)
    x, wt, sc, sh = _stem_data(case)
    want, mag = _conv_ref64(x, wt, sc, sh, stride, pad, relu)
    if not relu:  # the extreme of every image is negative: a kept magnitude that forgot the sign's removal cannot pass
        assert bool((want.amin(dim=(1, 2, 3)).abs() > want.amax(dim=(1, 2, 3)).abs()).all())
    run = lambda xs: ops.fused_conv(xs.to(dev), wt.to(dev), sc.to(dev), sh.to(dev), stride=stride, pad=pad, relu=relu, algo=ops.ALGO_DIRECT,
                                    in_nchw=True, no_stem="no_stem" in opt).clone()
    got = run(x)
    kept = ops.fused_conv.last_out_amax.clone()
    assert got.shape == (n,) + tuple(want.shape[2:]) + (cout,)
    ratio = _worst_ratio(got.permute(0, 3, 1, 2).cpu(), want, (3 * k * k + 4) * U * mag)
    with capsys.disabled():
        print(f"[stem fwd] {name}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # the kept magnitude row: exactly max |stored value| of every image
    assert torch.equal(kept.view(torch.float32), got.abs().amax(dim=(1, 2, 3)))
    if "zero" in opt:
        assert float(kept.view(torch.float32)[-1]) == 0.0 and not bool(got[-1].any())
    if n > 1:  # image 0 alone has the bits it has in the batch
        one = run(x[:1])
        assert torch.equal(one[0].view(torch.int32), got[0].view(torch.int32))
        assert torch.equal(ops.fused_conv.last_out_amax[:1], kept[:1])


# ---- 2. max-pool forward and amax_kernel ----
def _pool_data(case):
    name, (n, c, h, w), k, stride, pad, data = case
    rng = np.random.default_rng(po.seed(name))
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    if data == "special":
        x = np.maximum(x, np.float32(0.0))
        x[:, 4:, 2:7, 2:7] = 0.0  # whole windows tied at 0
        x[0, 1, 6, 6] = np.nan
        x[0, 2, 3, 7] = np.inf
        x[0, 3, 0:2, 0:2] = -np.inf  # the window of output (0, 0): rows and columns -1 .. 1
    assert not np.any(np.signbit(x) & (x == 0))  # no -0.0
    return torch.from_numpy(x)


@gpu
@pytest.mark.parametrize("case", po.POOL_CASES, ids=ids(po.POOL_CASES))
def test_maxpool_forward_and_kept_row_are_exact(dev, case):
    from multi_view_active_learning_amd import ops

    name, (n, c, h, w), k, stride, pad, data = case
    x = _pool_data(case)
    want = F.max_pool2d(x.double(), k, stride, pad)
    got = ops.fused_conv(x.permute(0, 2, 3, 1).contiguous().to(dev), k, None, None, stride=stride, pad=pad, kind=ops.OP_MAXPOOL, algo=ops.ALGO_DIRECT)
    kept = ops.fused_conv.last_out_amax.view(torch.float32).cpu()
    g = got.permute(0, 3, 1, 2).cpu().double().numpy()
    assert g.shape == tuple(want.shape)
    np.testing.assert_array_equal(np.isnan(g), np.isnan(want.numpy()))
    np.testing.assert_array_equal(g, want.numpy())  # (NaN == NaN here; every other value equal)
    if data == "special":
        assert np.isnan(g).any() and np.isposinf(g).any() and g[0, 3, 0, 0] == -np.inf and (g[:, 4:, 2, 2] == 0).all()
    clean = ~torch.isnan(want).flatten(1).any(1)
    assert bool(clean.any())
    assert torch.equal(kept[clean], want.abs().flatten(1).amax(1).float()[clean])


@gpu
@pytest.mark.parametrize("case", po.AMAX_CASES, ids=ids(po.AMAX_CASES))
def test_amax_alone(dev, case):
    """mval_amax on a base pointer off by four bytes (the scalar path although per_image % 4 == 0) and over a whole tensor as one image (the
    training forward's call after the pool); the extreme of each image is negative and sits at its last, first or middle element."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.engine import AMAX_ROW

    name, n, per, off = case
    rng = np.random.default_rng(po.seed(name))
    x = rng.standard_normal((n, per)).astype(np.float32)
    for i in range(n):
        x[i, (per - 1, 0, per // 2)[i % 3]] = -(np.abs(x[i]).max() + np.float32(1.5 + i))
    big = torch.zeros(off + n * per, dtype=torch.float32, device=dev)
    big[off:] = torch.from_numpy(x).reshape(-1).to(dev)
    xs = big[off:]
    assert (xs.data_ptr() % 16 == 0) == (off % 4 == 0)
    rows = torch.zeros(n * AMAX_ROW, dtype=torch.int32, device=dev)
    _lib._check(_lib.lib().mval_amax(_lib._p(xs), C.c_int64(per), C.c_int(n), _lib._p(rows), _lib._stream()), "mval_amax")
    rows = rows.reshape(n, AMAX_ROW).cpu()
    assert bool(((rows[:, 0] >= 1) & (rows[:, 0] <= AMAX_ROW - 1)).all())
    live = torch.arange(AMAX_ROW - 1)[None, :] < rows[:, :1]
    kept = torch.where(live, rows[:, 1:], torch.zeros_like(rows[:, 1:])).amax(1).view(torch.float32)
    assert torch.equal(kept, torch.from_numpy(np.abs(x).max(axis=1)))


# ---- 3. transposed conv, direct ----
@gpu
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "lin"])
@pytest.mark.parametrize("case", po.DECONV_CASES, ids=ids(po.DECONV_CASES))
def test_deconv_direct_vs_float64(dev, case, relu, capsys):
    from multi_view_active_learning_amd import ops

    name, (n, cin, cout, h, w), k, stride, pad = case
    rng = np.random.default_rng(po.seed(name))
    x = torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((cin, cout, k, k)) * 0.1).astype(np.float32))
    sc = torch.from_numpy((rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32))
    sh = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    want, mag = _conv_ref64(x, wt, sc, sh, stride, pad, relu, transposed=True)
    got = ops.fused_conv(x.permute(0, 2, 3, 1).contiguous().to(dev), wt.to(dev), sc.to(dev), sh.to(dev), stride=stride, pad=pad, relu=relu,
                         kind=ops.OP_DECONV, algo=ops.ALGO_DIRECT)
    kept = ops.fused_conv.last_out_amax.view(torch.float32)
    assert got.shape == (n,) + tuple(want.shape[2:]) + (cout,)
    ratio = _worst_ratio(got.permute(0, 3, 1, 2).cpu(), want, (cin * k * k + 4) * U * mag)
    with capsys.disabled():
        print(f"[deconv direct] {name} {'relu' if relu else 'lin'}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert torch.equal(kept, got.abs().amax(dim=(1, 2, 3)))


# ---- 4. weight gradients ----
SENTINEL = 12345.0


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


@gpu
@pytest.mark.parametrize("case", po.WGRAD_CASES, ids=ids(po.WGRAD_CASES))
def test_conv_wgrad_stem_direct_and_reduce_vs_float64(dev, case, capsys):
    from multi_view_active_learning_amd import _lib

    name, (n, cin, cout, h, w), k, stride, pad, x_nchw, path = case
    assert _wgrad_path_of(case) == path
    rng = np.random.default_rng(po.seed(name))
    ho, wo = po.out_hw(h, w, k, stride, pad)
    x = torch.from_numpy(rng.standard_normal((n, cin, h, w)).astype(np.float32))
    dz = torch.from_numpy(rng.standard_normal((n, cout, ho, wo)).astype(np.float32))
    lib, st, p = _lib.lib(), _lib._stream(), _lib._p
    xd = (x if x_nchw else x.permute(0, 2, 3, 1)).contiguous().to(dev)
    dzd = dz.permute(0, 2, 3, 1).contiguous().to(dev)
    lib.mval_conv_wgrad_workspace_floats.restype = C.c_size_t
    nws = int(lib.mval_conv_wgrad_workspace_floats(C.c_int(cin), C.c_int(cout), C.c_int(k)))
    assert nws == po.wg_splits(cin, cout) * k * k * cin * cout
    ws = torch.full((nws + 64,), SENTINEL, device=dev)
    dw = torch.full((cout, cin, k, k), 7.0, device=dev)
    rc = lib.mval_conv_wgrad(p(xd), p(dzd), p(dw), p(ws), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(cin), C.c_int(ho), C.c_int(wo), C.c_int(cout),
                             C.c_int(k), C.c_int(stride), C.c_int(pad), C.c_int(x_nchw), st)
    if path == "refused":
        assert rc == -1 and b"mval_conv_wgrad" in lib.mval_last_error()
        assert bool((dw == 7.0).all()) and bool((ws == SENTINEL).all())
        return
    _lib._check(rc, "mval_conv_wgrad")
    assert bool((ws[nws:] == SENTINEL).all())
    w64 = torch.zeros((cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, stride=stride, padding=pad).backward(dz.double())
    e = _rel(dw.cpu().numpy(), w64.grad.numpy())
    with capsys.disabled():
        print(f"[wgrad {path}] {name}: rel L2 {e:.2e}")
    assert e < 2e-5, e


# ---- 5. max-pool backward ----
@functools.lru_cache(maxsize=None)
def _poolb_ref(name):
    """(x, gout, gin64, r64) of a row, NCHW on the CPU, built once: the float64 F.max_pool2d backward of gout, and of |gout| (the sum of
    the magnitudes routed to each element)."""
    _, (n, c, h, w), k, stride, pad, data = {c[0]: c for c in po.POOLB_CASES}[name]
    rng = np.random.default_rng(po.seed(name))
    x = rng.standard_normal((n, c, h, w), dtype=np.float32)
    if data == "relu":
        x = np.maximum(x, np.float32(0.0))
        x[:, ::2, 2:8, 3:9] = 0.0  # whole windows tied at 0: the first maximum wins
    if data == "nan":
        x[0, 2, 3, 3] = np.nan
        x[1, 5, 0, 6] = np.nan
    x = torch.from_numpy(x)
    x64 = x.double().requires_grad_(True)
    y = F.max_pool2d(x64, k, stride, pad)
    g = torch.from_numpy(rng.standard_normal(tuple(y.shape), dtype=np.float32))
    gin64, = torch.autograd.grad(y, x64, g.double(), retain_graph=True)
    r64, = torch.autograd.grad(y, x64, g.double().abs())
    return x, g, gin64, r64


@gpu
@pytest.mark.parametrize("case", po.POOLB_CASES, ids=ids(po.POOLB_CASES))
def test_maxpool_backward_vs_float64(dev, case, capsys):
    from multi_view_active_learning_amd import _lib

    name, (n, c, h, w), k, stride, pad, data = case
    x, g, gin64, r64 = _poolb_ref(name)
    ho, wo = g.shape[2:]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xd, gd = nhwc(x).to(dev), nhwc(g).to(dev)
    lib, st, p = _lib.lib(), _lib._stream(), _lib._p
    call = lambda gin, acc: _lib._check(lib.mval_maxpool_bwd(p(gd), p(xd), p(gin), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(c), C.c_int(ho),
                                                             C.c_int(wo), C.c_int(k), C.c_int(stride), C.c_int(pad), C.c_int(acc), st), "mval_maxpool_bwd")
    got = torch.full((n, h, w, c), 3.0, device=dev)
    call(got, 0)
    want, r = nhwc(gin64), nhwc(r64)
    gc = got.cpu()
    if data == "nan":  # the gradient goes to the NaN element
        assert float(r64[0, 2, 3, 3]) > 0 and float(r64[1, 5, 0, 6]) > 0
    err = (gc.double() - want).abs()
    assert bool((gc[r == 0] == 0).all())
    ratio = float((err / (4 * U * r).clamp_min(1e-300)).max())
    with capsys.disabled():
        print(f"[maxpool bwd] {name}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # accumulate: one fp32 add of the stored gradient to the old value; exactly the old value where nothing is routed
    old = torch.from_numpy(np.random.default_rng(po.seed(name) + 1).standard_normal((n, h, w, c), dtype=np.float32)).to(dev)
    acc = old.clone()
    call(acc, 1)
    assert torch.equal(acc, old + got)
    zero = (r == 0).to(dev)
    assert torch.equal(acc[zero], old[zero])

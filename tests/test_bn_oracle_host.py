"""No GPU.  tests/bn_oracle.py against float64 torch.autograd; the P2 format's round trip; and the case tables of
tests/test_gpu_bn_entries.py held to the launchers' arithmetic (every form named) and to the conditions their inputs must meet
(decided ReLU masks, P2 bounds away from powers of two)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_oracle as bo
import test_gpu_bn_entries as T


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# (n, h, w, c, up, relu, residuals)
AUTOGRAD_CASES = [(3, 5, 3, 8, 0, 1, 2), (2, 4, 3, 16, 1, 1, 1), (2, 3, 2, 8, 2, 0, 2), (1, 3, 2, 4, 3, 1, 0), (2, 5, 3, 12, 0, 0, 0)]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=str)
def test_oracles_agree_with_float64_autograd(case):
    """out, the residual gradients, dz, dgamma and dbeta of the closed forms (mean and invstd from the float64 batch statistics) against
    autograd of F.batch_norm(training=True) + interpolate + adds + ReLU: 1e-12 relative."""
    n, h, w, c, up, relu, nres = case
    d = T.make_case(n, h, w, c, up, relu, tuple("f32" if i < nres else "none" for i in (0, 1)), seed=7)
    rng = np.random.default_rng(8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).requires_grad_(True)
    z, gamma, beta = t(d["z"]), t(d["gamma"]), t(d["beta"])
    res = [t(r) for r in d["r"] if r is not None]
    y = F.batch_norm(z.permute(0, 3, 1, 2), None, None, gamma, beta, True, 0.1, float(np.float32(T.BN_EPS)))
    if up:
        y = F.interpolate(y, scale_factor=2 ** up, mode="nearest")
    y = y.permute(0, 2, 3, 1)
    for r in res:
        y = y + r
    if relu:
        y = F.relu(y)
    gout = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(torch.from_numpy(gout.astype(np.float64)))
    st = bo.batch_stats(d["z"], T.BN_EPS)
    mean, invstd = st["mean"][0], st["invstd"][0]
    o = bo.bn_forward(d["z"], mean, invstd, d["gamma"], d["beta"], up, relu, d["r"][0], d["r"][1])
    assert _rel(o["out"], y.detach().numpy()) <= 1e-12
    g = bo.masked_gradient(gout, 1 if relu else 0, out=o["out"])
    b = bo.bn_backward(g, d["z"], mean, invstd, d["gamma"], up)
    assert _rel(b["dz"][0], z.grad.numpy()) <= 1e-12
    assert _rel(b["dgamma"][0], gamma.grad.numpy()) <= 1e-12
    assert _rel(b["dbeta"][0], beta.grad.numpy()) <= 1e-12
    for r in res:
        assert np.array_equal(bo.residual_gradient(g, None, True)[0], r.grad.numpy())
    # the four mask modes define the same masked gradient when they describe the same activation
    out32 = o["out"].astype(np.float32)
    if relu:
        assert np.array_equal(bo.masked_gradient(gout, 3, bits=bo.mask_bits(out32)), g)
        if nres == 0 and up == 0:
            assert np.array_equal(bo.masked_gradient(gout, 2, z=d["z"], mean=mean, invstd=invstd, gamma=d["gamma"], beta=d["beta"]), g)
    # has_bn = 0: the window sum and its per-channel sum
    b0 = bo.bn_backward(g, None, None, None, None, up, has_bn=False)
    assert np.array_equal(b0["gz"][0], b["gz"][0]) and _rel(b0["dbeta"][0], beta.grad.numpy()) <= 1e-12


def test_batch_stats_oracle_matches_torch_running_statistics():
    z = T.stats_data((2, 7, 5, 16))
    rm, rv = torch.linspace(-1, 1, 16, dtype=torch.float64), torch.linspace(0.5, 2, 16, dtype=torch.float64)
    want = bo.batch_stats(z, T.BN_EPS, 0.1, rm.numpy().copy(), rv.numpy().copy())
    mom = float(np.float32(0.1))
    F.batch_norm(torch.from_numpy(z.astype(np.float64)).permute(0, 3, 1, 2), rm, rv, None, None, True, mom, T.BN_EPS)
    # (1 - float32(0.1)) in float32, as the kernel, against torch's float64 1 - momentum: 2^-25 of the running term
    assert _rel(want["running_mean"][0], rm.numpy()) <= 1e-7 and _rel(want["running_var"][0], rv.numpy()) <= 1e-7
    zz = z.reshape(-1, 16).astype(np.float64)
    assert _rel(want["mean"][0], zz.mean(0)) <= 1e-14 and _rel(want["invstd"][0], 1 / np.sqrt(zz.var(0) + float(np.float32(T.BN_EPS)))) <= 1e-12


def test_p2_round_trip_within_the_formats_statement():
    rng = np.random.default_rng(1)
    n, h, w, c = 2, 5, 3, 24
    x = (rng.standard_normal((n, h, w, c)) * 2.0 ** rng.integers(-30, 4, size=(n, h, w, c))).astype(np.float32)
    x[0, 0, 0, :4] = [0.0, 2.0 ** -40, -2.0 ** -20, np.abs(x).max()]
    for slack in (1.0, 3.0, 100.0):
        bound = float(np.abs(x).max()) * slack
        s = bo.p2_scale(bound)
        assert 2.0 ** 13 <= bound * 2.0 ** s < 2.0 ** 14
        halves = bo.p2_encode(x, s)
        assert halves.shape == (n, 2, c // 8, h, w, 8) and halves.dtype == np.float16 and np.isfinite(halves.astype(np.float64)).all()
        inv = 2.0 ** -s
        err = np.abs(bo.p2_decode(halves, inv, n, c, h, w) - x.astype(np.float64))
        assert (err <= bo.p2_format_bound(x, inv)).all()
        # the layout: element (n, y, x, c) sits at [n][plane][c // 8][y][x][c % 8]
        hi, _ = bo.p2_planes(halves, n, c, h, w)
        assert hi[1, 2, 1, 13] == float(halves[1, 0, 1, 2, 1, 5])
    assert bo.p2_scale(np.nan) == 0 and bo.p2_scale(2.0 ** 14 - 1) == 0
    assert bo.p2_scale(0.0) == 0 and bo.p2_scale(np.inf) == 0 and bo.p2_scale(1.0) == 13 and bo.p2_scale(2.0 ** 13) == 0 and bo.p2_scale(2.0 ** 14) == -1
    assert bo.p2_scale(2.0 ** -120) == 110 and bo.p2_scale(2.0 ** 126) == -110
    assert bo.p2_inv_bits(3) == int(np.float32(0.125).view(np.int32))


def test_wave_map_and_launch_geometry_restated():
    assert bo.wave_map(64) == (32, 8, 8, 2) and bo.wave_map(48) == (16, 4, 16, 3) and bo.wave_map(24) == (8, 2, 32, 3)
    g = bo.launch_geometry("reduce", 48, 45)
    assert (g["lanes"], g["rows"], g["idle"]) == (12, 21, 4)
    g = bo.launch_geometry("stats", 32, 131584)
    assert (g["nb"], g["rows"], g["trips"], g["ragged"]) == (512, 32, 2, True)
    assert bo.launch_geometry("stats", 32, 131072)["trips"] == 1
    assert bo.launch_geometry("reduce", 32, 65536)["trips"] == 1 and bo.launch_geometry("reduce", 32, 65537)["trips"] == 2
    assert bo.launch_geometry("apply", 32, 65536)["trips"] == 1 and bo.launch_geometry("apply", 32, 65537)["trips"] == 2
    g = bo.launch_geometry("reduce", 1032, 12)
    assert (g["cb_passes"], g["cb_last"], g["rows"]) == (2, 2, 1)
    assert bo.launch_geometry("scalar", 19, 7000) == dict(nb=512, rows=13, idle=9, trips=2, ragged=True)


# ---- the case tables name every form ----------------------------------------------------------------------------------------------
def test_stats_cases_cover_the_loops():
    geo = [bo.launch_geometry("stats", c, n * h * w) for n, h, w, c in T.STATS_CASES]
    assert any(g["trips"] >= 2 and g["ragged"] for g in geo)
    assert any(g["trips"] == 1 and g["ragged"] for g in geo)
    assert any(g["cb_passes"] == 2 and g["cb_last"] == 2 for g in geo) and any(g["cb_passes"] == 2 and g["cb_last"] == 256 for g in geo)
    assert any(g["idle"] == 4 and g["lanes"] == 12 for g in geo)
    smallest = bo.launch_geometry("stats", 32, T.TWO_TRIP_STATS[0] * (T.TWO_TRIP_STATS[1] - 1) * T.TWO_TRIP_STATS[2])
    assert smallest["trips"] == 1, "one image row fewer fits one trip: the shape is the smallest of its kind"
    assert T.TILES_CASE[4] > 256 and T.TILES_CASE[4] % 256 != 0
    for case in T.STATS_CASES:
        z = T.stats_data(case).astype(np.float64)
        assert (np.abs(z.mean((0, 1, 2))) / z.std((0, 1, 2))).max() > 50, "E[z^2] - mean^2 must cancel"


def test_forward_cases_cover_every_form():
    geo = [bo.launch_geometry("apply", c, n * h * w, n * (h << up) * (w << up)) for n, h, w, c, up, relu, kinds in T.FWD_CASES]
    assert any(g["trips"] == 2 and g["ragged"] for g in geo) and any(g["trips"] == 1 and g["ragged"] for g in geo)
    assert {c for _, _, _, c, *_ in T.FWD_CASES} >= {4, 16, 48, 1032}
    assert {(up, sum(k != "none" for k in kinds)) for *_, up, relu, kinds in T.FWD_CASES} >= {(0, 0), (1, 1), (2, 2), (0, 1), (2, 0), (1, 2), (0, 2)}
    assert {relu for *_, relu, kinds in T.FWD_CASES} == {0, 1}
    # P2
    maps = {bo.wave_map(c)[0] for _, _, _, c, *_ in T.FWD_P2_CASES}
    assert maps == {32, 16, 8} and {c for _, _, _, c, *_ in T.FWD_P2_CASES} >= {32, 64, 48, 16, 24, 8}
    for slot in (0, 1):
        assert {kinds[slot] for *_, kinds in T.FWD_P2_CASES} == {"none", "f32", "p2"}
    assert {up for *_, up, relu, kinds in T.FWD_P2_CASES} == {0, 1, 2}
    geo = [bo.launch_geometry("apply_p2", c, n * h * w, n * (h << up) * (w << up)) for n, h, w, c, up, relu, kinds in T.FWD_P2_CASES]
    assert any(g["trips"] == 2 and g["ragged"] for g in geo)
    for cb in (32, 16, 8):  # a last pixel chunk that is not full, on each wave map
        assert any(g["partial_chunk"] for g, case in zip(geo, T.FWD_P2_CASES) if bo.wave_map(case[3])[0] == cb), cb
    assert any(kinds[0] != "none" and kinds[1] != "none" and kinds[0] != kinds[1] for *_, kinds in T.FWD_P2_CASES)
    # plane statistics: all three wave maps' planes and a second trip of its own loop
    geo = [bo.launch_geometry("plane_stats", c, n * h * w, n * (h << up) * (w << up)) for n, h, w, c, up, relu, kinds in T.PLANE_STATS_CASES]
    assert any(g["trips"] == 2 and g["ragged"] for g in geo) and {bo.wave_map(c[3])[0] for c in T.PLANE_STATS_CASES} == {32, 16, 8}


def test_backward_cases_cover_every_form():
    cases = T.BWD_CASES
    assert {(up, relu) for _, _, _, _, up, relu, has_bn, _, _ in cases if has_bn} == {(u, r) for u in range(4) for r in (0, 1)}
    assert {up for _, _, _, _, up, relu, *_ in cases if not relu and up} == {1, 2, 3}, "the no-ReLU four-at-a-time path"
    assert {ow for *_, slots, ow in cases if slots == (1, 1)} == {0, 1, 2, 3}
    assert {has_bn for *_, has_bn, _, _ in cases} == {0, 1}
    assert {c for _, _, _, c, *_ in cases} >= {4, 16, 48, 1032, 2048}
    geo = [bo.launch_geometry("reduce" if up == 0 else "reduce_up", c, n * h * w) for n, h, w, c, up, *_ in cases]
    assert any(g["trips"] >= 2 and g["ragged"] for g, case in zip(geo, cases) if case[4] == 0)
    assert any(g["trips"] >= 2 and g["ragged"] for g, case in zip(geo, cases) if case[4] > 0)
    assert any(g["cb_passes"] == 2 and g["cb_last"] == 2 for g in geo) and any(g["cb_passes"] == 2 and g["cb_last"] == 256 for g in geo)
    assert any((g["lanes"], g["rows"], g["idle"]) == (12, 21, 4) for g in geo)
    assert bo.launch_geometry("reduce", 32, T.TWO_TRIP_REDUCE[0] * (T.TWO_TRIP_REDUCE[1] - 1) * T.TWO_TRIP_REDUCE[2])["trips"] == 1
    # scalar form
    assert {(c, relu) for _, _, _, c, relu in T.SCALAR_CASES} >= {(c, r) for c in (19, 17, 1) for r in (0, 1)}
    assert all(c % 4 for _, _, _, c, _ in T.SCALAR_CASES)
    assert any(n * h * w == 7000 and bo.launch_geometry("scalar", c, 7000)["trips"] == 2 for n, h, w, c, _ in T.SCALAR_CASES)
    # fused, fp32 and P2
    for table in (T.FUSED_CASES, T.BWD_P2_CASES):
        assert {mode for _, _, _, _, mode, _, _ in table} == {0, 1, 2, 3}
        geo = [bo.launch_geometry("reduce", c, n * h * w) for n, h, w, c, *_ in table]
        assert any(g["trips"] == 2 and g["ragged"] for g in geo)
        assert any(slots == (0, 1) and ow & 2 for *_, slots, ow in table), "the apply pass re-reads the SECOND slot"
        # the mask mode the APPLY pass runs with (0 whenever the call stores a given slot), not the nominal one: all four, and
        # each of them on the two-trip shape too
        assert {T.apply_mask(mode, slots, ow) for *_, mode, slots, ow in table} == {0, 1, 2, 3}
        assert {T.apply_mask(mode, slots, ow) for *shape, mode, slots, ow in table if tuple(shape) == T.TWO_TRIP_REDUCE} == {0, 1, 2, 3}
        assert all(T.apply_mask(mode, slots, ow) == mode for *_, mode, slots, ow in table if mode in (0, 2))
        # the apply pass' own grid-stride loop: a second, ragged trip (fp32: float4 items; P2: wave items)
        geo = [bo.launch_geometry("apply" if table is T.FUSED_CASES else "apply_p2", c, n * h * w) for n, h, w, c, *_ in table]
        assert any(g["trips"] == 2 and g["ragged"] for g in geo)
    assert {T.apply_mask(mode, (0, 0) if mode == 2 else (1, 1), T.CHAIN_OVERWRITE[mode]) for *_, mode in T.CHAIN_CASES} == {0, 1, 2, 3}
    geo = [bo.launch_geometry("apply", c, n * h * w) for n, h, w, c, up, relu, has_bn, *_ in T.BWD_CASES if has_bn]
    assert any(g["trips"] == 2 and g["ragged"] for g in geo), "bn_bwd_apply_kernel's second trip"
    assert {ow for *_, slots, ow in T.FUSED_CASES if slots == (1, 1)} == {0, 1, 2, 3}
    assert {c for _, _, _, c, *_ in T.FUSED_CASES} >= {4, 16, 48, 1032, 2048}
    assert {c for _, _, _, c, *_ in T.BWD_P2_CASES} >= {32, 48, 24} and {bo.wave_map(c[3])[0] for c in T.BWD_P2_CASES} == {32, 16, 8}
    geo = [bo.launch_geometry("apply_p2", c, n * h * w) for n, h, w, c, *_ in T.BWD_P2_CASES]
    assert any(g["trips"] == 2 and g["ragged"] for g in geo) and any(g["partial_chunk"] for g in geo)
    assert {mode for *_, mode in T.CHAIN_CASES} == {0, 1, 2, 3}


# ---- the conditions on the inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.FWD_CASES + T.FWD_P2_CASES, ids=T._id)
def test_forward_inputs_decide_every_mask(case):
    """bn_forward asserts min |pre-activation| >= 2^-10 * (sum of its terms' magnitudes) on the rounded float32 inputs; the P2 cases'
    a-priori bound is not within 1e-4 of a power of two and really bounds the output."""
    n, h, w, c, up, relu, kinds = case
    d = T.make_case(n, h, w, c, up, relu, kinds, T._seed(case))
    o = T.forward_oracle(d)
    assert (np.abs(o["pre"]) >= 2.0 ** -10 * o["mag"]).all() and (np.abs(o["pre"]) >= 0.05).all()
    if "p2" in kinds:
        s = [rp[1] for rp in d["rp"] if rp is not None]
        assert len(set(s)) == len(s), "the two plane residuals' scales must differ"
    if case in T.FWD_P2_CASES:
        b = T.forward_p2_bound(d)
        assert bo.far_from_power_of_two(b) and np.abs(o["out"]).max() + o["bound"].max() <= b


@pytest.mark.parametrize("case", T.FUSED_CASES + T.BWD_P2_CASES + T.CHAIN_CASES, ids=T._id)
def test_backward_inputs_decide_every_mask(case):
    mode = case[4]
    d, out, bits, gout, relu = T.fused_case(case)
    want = T.fused_oracle(d, out, bits, gout, mode)  # (mode 2: asserts the condition on z)
    if relu:
        same = [bo.masked_gradient(gout, m, out=out, bits=bits, z=d["z"], mean=d["mean"], invstd=d["invstd"], gamma=d["gamma"], beta=d["beta"])
                for m in ((1, 3, 2) if mode == 2 else (1, 3))]
        assert all(np.array_equal(s, want["g"]) for s in same)
    if case in T.BWD_P2_CASES or case in T.CHAIN_CASES:
        assert bo.far_from_power_of_two(want["p2_bound"])
        assert (np.abs(want["dz"][0]) + want["dz"][1]).max() <= want["p2_bound"], "Samuelson's bound must hold for the data"
    if case in T.CHAIN_CASES:
        assert bo.far_from_power_of_two(T.forward_p2_bound(d))
        T.forward_oracle(d, stat_err=True)


@pytest.mark.parametrize("case", T.BWD_CASES, ids=T._id)
def test_bwd_inputs_decide_every_mask(case):
    n, h, w, c, up, relu, has_bn, slots, overwrite = case
    d = T.make_case(n, h, w, c, up, relu, tuple("f32" if s else "none" for s in slots), T._seed(case))
    out, bits, gout = T.backward_inputs(d, T._seed(case))
    o = T.forward_oracle(d)  # (with ReLU: asserts that no pre-activation is undecided)
    assert out.shape == gout.shape == (n, h << up, w << up, c)
    if relu:
        # the float32 `out` the kernel masks by has the sign pattern of the float64 pre-activation, and both kinds of mask agree on it
        assert (np.abs(o["pre"]) >= 2.0 ** -10 * o["mag"]).all() and np.array_equal(out > 0, o["pre"] > 0)
        g = bo.masked_gradient(gout, 1, out=out)
        assert np.array_equal(g, bo.masked_gradient(gout, 3, bits=bits)) and 0 < np.count_nonzero(g) < g.size
    else:
        assert np.array_equal(bo.masked_gradient(gout, 0), gout.astype(np.float64))

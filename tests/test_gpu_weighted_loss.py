"""GPU tests of the weighted training loss with hard key-point mining (csrc/loss_weighted.hip: mval_weighted_mse_fwd / _bwd and their points
forms) and of what is built on it: pose_2d_mse_weighted(_from_points), compose_joint_weights and train_step under TRAIN.LOSS.

The contract fixes every rounding, so nearly every comparison is of bits: the per-map sums against mval_frame_loss (the same kernel), the
per-map losses, the selection, the loss value and the gradient against tests/weighted_loss_oracle.py.  The two "within 1 float32 ulp"
comparisons are against today's loss, which adds the same float32 squares in float64 in another order: the order error is about n * 2^-53
relative, far below 2^-24, so the two roundings to float32 can differ only where the sum sits on a rounding boundary.
Inputs come from seeds; the one stored value is the CRC of mval_frame_loss's results from before its kernel was shared."""
import zlib

import numpy as np
import pytest
import torch

import cases
import weighted_loss_oracle as wo
from test_gpu_loss_points import _i32, _misaligned, _points, _train_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


# (n_images, J, hh, wh, heat-maps one float past a 16-byte boundary)
SHAPES = [
    (1, 1, 5, 13, False),     # scalar walk, a single map
    (3, 19, 7, 9, False),     # hw % 4 = 3, odd map bases
    (2, 19, 8, 8, False),     # float4 walk
    (2, 19, 8, 8, True),      # hw % 4 == 0 but the maps misaligned: scalar walk
    (5, 42, 64, 48, False),   # 3 072 pixels: every lane makes several trips
    (130, 3, 8, 8, False),    # more images than any per-workgroup grouping of 64 or 128
    (2, 70, 8, 8, False),     # J past one wave
]
SHAPE_IDS = ["%dx%dx%dx%d%s" % (s[0], s[1], s[2], s[3], "-offset" if s[4] else "") for s in SHAPES]
TIED = (2, 5, 11)  # joints of image 0 that are byte copies of one map and target, with equal weights and the image's largest loss
SHAPE_TOPK = [(s, k) for s in SHAPES for k in sorted({0, 1, s[1]} | ({8} if s[1] >= 8 else set()))]
SHAPE_TOPK_IDS = ["%s-top%d" % (SHAPE_IDS[SHAPES.index(s)], k) for s, k in SHAPE_TOPK]


def _i64(t):
    return t.detach().contiguous().view(torch.int64).cpu().numpy()


_CASES = {}


def _case(dev, shape):
    """One seeded case, built once and shared (no test writes into it): heat-maps, points with the special ones of test_gpu_loss_points, the
    maps gt_heatmaps renders from them under a scalar sigma and under mixed per-map sigmas, and weights uniform(0, 2) with about a third 0."""
    if shape in _CASES:
        return _CASES[shape]
    from multi_view_active_learning_amd.utils import preprocess

    n, j, hh, wh, offset = shape
    lead = n * j
    rng = np.random.default_rng(7000 + 100 * n + 10 * j + hh)
    hm = rng.standard_normal((lead, hh * wh)).astype(np.float32) * 0.5
    pt = _points(rng, lead, hh, wh, False)
    w = rng.uniform(0, 2, lead).astype(np.float32)
    w[rng.uniform(size=lead) < 1 / 3] = 0
    w[0] = 1
    sig = rng.choice([0.5, 1.0, 2.0], size=lead)
    sig[:3] = [0.5, 1.0, 2.0][: min(3, lead)]
    if j > max(TIED):
        for k in TIED[1:]:
            hm[k], pt[k], sig[k] = hm[TIED[0]], pt[TIED[0]], sig[TIED[0]]
        hm[list(TIED)] += 3.0  # far from every target: the three share the image's largest loss
        w[list(TIED)] = 1.5
    pt = torch.from_numpy(pt).to(dev)
    g1 = preprocess.gt_heatmaps(pt, 1.5, hh, wh).reshape(-1)
    gm = torch.empty((lead, hh, wh), dtype=torch.float32, device=dev)
    for s in (0.5, 1.0, 2.0):
        idx = torch.from_numpy(np.flatnonzero(sig == s)).to(dev)
        if idx.numel():
            gm[idx] = preprocess.gt_heatmaps(pt[idx], s, hh, wh)
    gm = gm.reshape(-1)
    h = torch.from_numpy(hm.reshape(-1)).to(dev)
    if offset:
        h, g1, gm = _misaligned(h), _misaligned(g1), _misaligned(gm)
    c = dict(n=n, j=j, hh=hh, wh=wh, lead=lead, h=h, pt=pt, g=g1, g_mixed=gm, sigma=1.5, sigma_mixed=torch.from_numpy(sig).to(dev), w=w,
             w_dev=torch.from_numpy(w).to(dev), denom=float(n * hh * wh))
    _CASES[shape] = c
    return c


def _dims(c):
    return c["n"], c["j"], c["hh"], c["wh"]


def _forward(c, form, w, topk, mixed=False):
    from multi_view_active_learning_amd import _lib

    if form == "points":
        return _lib.weighted_mse_points_fwd(c["h"], c["pt"], c["sigma_mixed"] if mixed else c["sigma"], w, topk, *_dims(c))
    return _lib.weighted_mse_fwd(c["h"], c["g_mixed"] if mixed else c["g"], w, topk, *_dims(c))


def _backward(c, form, wsel, grad, mixed=False):
    from multi_view_active_learning_amd import _lib

    go = torch.tensor(grad, dtype=torch.float32, device=c["h"].device)
    if form == "points":
        return _lib.weighted_mse_points_bwd(c["h"], c["pt"], c["sigma_mixed"] if mixed else c["sigma"], wsel, go, *_dims(c))
    return _lib.weighted_mse_bwd(c["h"], c["g_mixed"] if mixed else c["g"], wsel, go, *_dims(c))


# ---- 1. per-map sums ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_per_map_sums_are_frame_loss_bits(dev, shape):
    """weight = 1 and topk = 0, so per_map = S: the read form equals mval_frame_loss's per_map, the points form mval_frame_loss_points's under
    a scalar sigma, and under mixed per-map sigmas (which mval_frame_loss_points does not take) the read form on the maps gt_heatmaps renders."""
    from multi_view_active_learning_amd import _lib

    c = _case(dev, shape)
    ones = torch.ones(c["lead"], dtype=torch.float32, device=dev)
    want = _i64(_lib.frame_loss(c["h"], c["g"], None, *_dims(c))[1])
    np.testing.assert_array_equal(_i64(_forward(c, "read", ones, 0)[1]), want)
    np.testing.assert_array_equal(_i64(_lib.frame_loss_points(c["h"], c["pt"], c["sigma"], None, *_dims(c))[1]), want)
    np.testing.assert_array_equal(_i64(_forward(c, "points", ones, 0)[1]), want)
    mixed = _i64(_forward(c, "read", ones, 0, mixed=True)[1])
    np.testing.assert_array_equal(_i64(_forward(c, "points", ones, 0, mixed=True)[1]), mixed)
    np.testing.assert_array_equal(mixed, _i64(_lib.frame_loss(c["h"], c["g_mixed"], None, *_dims(c))[1]))
    assert (mixed != want).any() or c["lead"] == 1  # the sigmas do make a difference


FRAME_LOSS_CRC = 2022334304  # of _frame_loss_crc with the library of the commit before the kernel moved, on an MI355X


def _frame_loss_crc(dev):
    """CRC-32 of what mval_frame_loss returns (per-frame losses, then per-map sums) on two fixed seeded cases, one per walk, under a mask."""
    from multi_view_active_learning_amd import _lib

    crc = 0
    for n, m, hh, wh in ((3, 19, 7, 9), (4, 19, 64, 48)):
        rng = np.random.default_rng(424242 + hh)
        h = torch.from_numpy(rng.standard_normal((n, m, hh, wh)).astype(np.float32)).to(dev)
        g = torch.from_numpy(rng.uniform(0, 1, (n, m, hh, wh)).astype(np.float32)).to(dev)
        valid = torch.from_numpy((rng.uniform(size=n * m) > 0.3).astype(np.uint8)).to(dev)
        out, per_map = _lib.frame_loss(h, g, valid, n, m, hh, wh)
        crc = zlib.crc32(per_map.cpu().numpy().tobytes(), zlib.crc32(out.cpu().numpy().tobytes(), crc))
    return crc


def test_frame_loss_bits_are_the_parents(dev):
    """mval_frame_loss now runs the kernel it shares with the weighted loss (csrc/frame_loss_map.h).  Its results on a fixed seeded case
    still have the CRC that this function gave with the library of the commit before, whose kernel lived in csrc/frame_loss.hip alone."""
    assert _frame_loss_crc(dev) == FRAME_LOSS_CRC


# ---- 2.-4. loss, selection, gradient -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["read", "points"])
@pytest.mark.parametrize("shape,topk", SHAPE_TOPK, ids=SHAPE_TOPK_IDS)
def test_forward_and_backward_bits(dev, shape, topk, form):
    """per_map = float64(w) * S with S the device's own per-map sums (mval_frame_loss under the mask w != 0); wsel equals the oracle's
    selection from those per_map values, bit for bit -- in image 0 the joints 2, 5, 11 tie for the largest loss and topk = 1 cuts inside the
    tie, so only joint 2 is kept; the loss equals the oracle's sequential float64 sum rounded once; grad_h equals the float32 oracle
    ((2 d) gs) wsel for grad_out 1.0 and 0.37, and is +0.0 on every map that does not count."""
    from multi_view_active_learning_amd import _lib

    c = _case(dev, shape)
    n, j, hh, wh = _dims(c)
    loss, per_map, wsel = _forward(c, form, c["w_dev"], topk)
    S = _lib.frame_loss(c["h"], c["g"], (c["w_dev"] != 0).to(torch.uint8), n, j, hh, wh)[1].cpu().numpy().reshape(n, j)
    w = c["w"].reshape(n, j)
    want_l = wo.per_map_loss(w, S)
    got_l = per_map.cpu().numpy().reshape(n, j)
    np.testing.assert_array_equal(got_l.view(np.int64), want_l.view(np.int64))
    sel, want_wsel = wo.select(got_l, w, topk)
    got_wsel = wsel.cpu().numpy().reshape(n, j)
    np.testing.assert_array_equal(got_wsel.view(np.int32), want_wsel.view(np.int32))
    if j > max(TIED):
        assert got_l[0, TIED[0]] == got_l[0, TIED[1]] == got_l[0, TIED[2]] == got_l[0].max()
        kept = [k for k in TIED if got_wsel[0, k] != 0]
        assert kept == list(TIED[: topk if 0 < topk < 3 else 3]), (topk, kept)
    if topk:
        assert (sel.sum(1) == topk).all()
    want = wo.loss_value(got_l, sel, c["denom"])
    assert np.isfinite(want) and want > 0
    assert _i32(loss) == want.view(np.int32), (loss.item(), want)
    h = c["h"].cpu().numpy().reshape(n, j, -1)
    g = c["g"].cpu().numpy().reshape(n, j, -1)
    for grad in (1.0, 0.37):
        gh = _i32(_backward(c, form, wsel, grad)).reshape(n, j, -1)
        want_g = wo.gradient(h, g, want_wsel, grad, c["denom"]).view(np.int32)
        bad = np.argwhere((gh != want_g).any(2))
        assert bad.size == 0, "maps %r differ" % (bad[:10].tolist(),)
        assert not gh[want_wsel == 0].any() and gh.any()


def test_mixed_sigmas_both_forms(dev):
    """Per-map sigmas through both directions: the points form has the read form's bits on the maps rendered sigma group by sigma group."""
    c = _case(dev, SHAPES[1])
    a, b = _forward(c, "points", c["w_dev"], 8, mixed=True), _forward(c, "read", c["w_dev"], 8, mixed=True)
    assert _i32(a[0]) == _i32(b[0])
    np.testing.assert_array_equal(_i64(a[1]), _i64(b[1]))
    np.testing.assert_array_equal(_i32(a[2]), _i32(b[2]))
    ga, gb = _backward(c, "points", a[2], 0.37, mixed=True), _backward(c, "read", b[2], 0.37, mixed=True)
    np.testing.assert_array_equal(_i32(ga), _i32(gb))
    assert _i32(ga).any()


# ---- 3. NaN ------------------------------------------------------------------------------------------------------------------
NAN_MAP = 19 + 7  # image 1, joint 7


def _with_nan_pixel(c):
    h = c["h"].clone()
    h[NAN_MAP * c["hh"] * c["wh"] + 5] = float("nan")
    return dict(c, h=h)


def test_nan_under_a_positive_weight_ranks_first(dev):
    c = _with_nan_pixel(_case(dev, SHAPES[2]))
    w = c["w_dev"].clone()
    w[NAN_MAP] = 0.25
    for form in ("read", "points"):
        loss, per_map, wsel = _forward(c, form, w, 1)
        assert np.isnan(loss.item()) and np.isnan(per_map[NAN_MAP].item())
        kept = np.flatnonzero(wsel.cpu().numpy()[19:])
        assert kept.tolist() == [7] and wsel[NAN_MAP].item() == 0.25  # the smallest weight of the image, the first rank all the same


def test_nan_under_a_zero_weight_does_not_count(dev):
    """A NaN pixel (both forms), NaN ground truth (read form) and a NaN point (points form) under weight 0: the loss is finite and has the
    bits it has without the NaNs, wsel is 0 there and the map's gradient is exactly +0.0."""
    clean = _case(dev, SHAPES[2])
    hw = clean["hh"] * clean["wh"]
    w = clean["w_dev"].clone()
    w[NAN_MAP] = 0
    c = _with_nan_pixel(clean)
    g = c["g"].clone()
    g[NAN_MAP * hw: (NAN_MAP + 1) * hw] = float("nan")
    pt = c["pt"].clone()
    pt[NAN_MAP] = float("nan")
    c = dict(c, g=g, pt=pt)
    for form in ("read", "points"):
        for topk in (0, 8):
            loss, per_map, wsel = _forward(c, form, w, topk)
            want = _forward(clean, form, w, topk)
            assert np.isfinite(loss.item()) and _i32(loss) == _i32(want[0])
            np.testing.assert_array_equal(_i64(per_map), _i64(want[1]))
            assert _i64(per_map)[NAN_MAP] == 0 and _i32(wsel)[NAN_MAP] == 0
            gh = _backward(c, form, wsel, 0.37)
            np.testing.assert_array_equal(_i32(gh), _i32(_backward(clean, form, want[2], 0.37)))
            assert not _i32(gh).reshape(-1, hw)[NAN_MAP].any()


# ---- 5. ties to today's loss ---------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("form", ["read", "points"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_zero_one_weights_are_todays_masked_loss(dev, shape, form):
    """Weights in {0, 1} from a uint8 mask, topk = 0: the gradient has the bits of mval_masked_mse_bwd / _points_bwd under that mask, and the
    loss is within 1 float32 ulp of mval_masked_mse_fwd's (the same float32 squares added in float64 in another order; module docstring)."""
    from multi_view_active_learning_amd import _lib

    c = _case(dev, shape)
    n, j, hh, wh = _dims(c)
    mask = (c["w_dev"] != 0).to(torch.uint8)
    loss, _, wsel = _forward(c, form, mask.to(torch.float32), 0)
    go = torch.tensor(0.37, dtype=torch.float32, device=dev)
    if form == "points":
        old = _lib.masked_mse_points_fwd(c["h"], c["pt"], c["sigma"], mask, c["lead"], hh, wh, c["denom"])
        old_g = _lib.masked_mse_points_bwd(c["h"], c["pt"], c["sigma"], mask, go, c["lead"], hh, wh, c["denom"])
    else:
        old = _lib.masked_mse_fwd(c["h"], c["g"], mask, c["lead"], hh * wh, c["denom"])
        old_g = _lib.masked_mse_bwd(c["h"], c["g"], mask, go, c["lead"], hh * wh, c["denom"])
    np.testing.assert_array_equal(_i32(_backward(c, form, wsel, 0.37)), _i32(old_g))
    print("\n[weighted_loss] %s %s: weighted %r, masked %r" % (SHAPE_IDS[SHAPES.index(shape)], form, loss.item(), old.item()))
    assert old.item() > 0 and _ulps(loss.item(), old.item()) <= 1, (loss.item(), old.item())


# ---- 6. autograd and train_step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["read", "points"])
def test_autograd_equals_the_direct_calls(dev, form):
    """pose_2d_mse_weighted(_from_points)(...).backward(): loss and heatmaps.grad have the bits of the direct _lib calls, for a (J,) weight
    that broadcasts over the images and a per-image sigma; return_per_map is per_map / (h * w), detached."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError

    c = _case(dev, SHAPES[1])
    n, j, hh, wh = _dims(c)
    loss = Pose2DMeanSquaredError()
    wj = c["w"][:j].copy()
    w_full = torch.from_numpy(np.tile(wj, n)).to(dev)
    x = c["h"].reshape(n, j, hh, wh).clone().requires_grad_(True)
    go = torch.tensor(0.37, dtype=torch.float32, device=dev)
    if form == "points":
        sig = np.array([1.0, 2.0, 0.5])
        out, per_map = loss.pose_2d_mse_weighted_from_points(x, c["pt"].reshape(n, j, 2), sig, wj, topk=8, return_per_map=True)
        sig_maps = torch.from_numpy(np.repeat(sig, j)).to(dev)
        want = _lib.weighted_mse_points_fwd(c["h"], c["pt"], sig_maps, w_full, 8, n, j, hh, wh)
        want_g = _lib.weighted_mse_points_bwd(c["h"], c["pt"], sig_maps, want[2], go, n, j, hh, wh)
    else:
        out, per_map = loss.pose_2d_mse_weighted(x, c["g"].reshape(n, j, hh, wh), wj, topk=8, return_per_map=True)
        want = _forward(c, "read", w_full, 8)
        want_g = _backward(c, "read", want[2], 0.37)
    (out * 0.37).backward()
    assert _i32(out) == _i32(want[0]) and not per_map.requires_grad and per_map.shape == (n, j) and per_map.dtype == torch.float64
    np.testing.assert_array_equal(_i64(per_map), _i64(want[1].reshape(n, j) / float(hh * wh)))
    np.testing.assert_array_equal(_i32(x.grad).reshape(-1), _i32(want_g).reshape(-1))
    assert _i32(x.grad).any()
    for bad in (np.full(j, -1.0, np.float32), np.full(j, np.nan, np.float32), np.ones(j + 1, np.float32)):
        with pytest.raises(_lib.MvalError, match="pose_2d_mse_weighted"):
            loss.pose_2d_mse_weighted(x, c["g"].reshape(n, j, hh, wh), bad)
    with pytest.raises(_lib.MvalError, match="topk"):
        loss.pose_2d_mse_weighted(x, c["g"].reshape(n, j, hh, wh), wj, topk=j + 1)


def test_autograd_keeps_no_ground_truth(dev):
    """Allocated device memory after the forward, with the graph alive (the pattern of test_gpu_loss_points): the read form holds the
    (N, J, h, w) maps it was given, the points form less than an eighth of one such tensor on top of the heat-maps."""
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError
    from multi_view_active_learning_amd.utils import preprocess

    n, j, hh, wh = 8, 19, 64, 64
    map_bytes = n * j * hh * wh * 4
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((n, j, hh, wh)).astype(np.float32) * 0.5).to(dev).requires_grad_(True)
    pt = torch.from_numpy(np.stack([rng.uniform(-2, wh + 1, (n, j)), rng.uniform(-2, hh + 1, (n, j))], -1)).to(dev)
    w = torch.from_numpy(rng.uniform(0, 2, (n, j)).astype(np.float32)).to(dev)
    loss = Pose2DMeanSquaredError()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    out_p = loss.pose_2d_mse_weighted_from_points(x, pt, 1.0, w, topk=8)
    torch.cuda.synchronize()
    d_points = torch.cuda.memory_allocated() - base
    g = preprocess.gt_heatmaps(pt, 1.0, hh, wh)
    out_r = loss.pose_2d_mse_weighted(x, g, w, topk=8)
    del g  # the graph keeps it
    torch.cuda.synchronize()
    d_read = torch.cuda.memory_allocated() - base - d_points
    assert _i32(out_p) == _i32(out_r)
    assert d_read >= map_bytes, (d_read, map_bytes)
    assert 0 <= d_points < map_bytes // 8, (d_points, map_bytes)


def _one_step(c, dev, sd, data, **loss_fields):
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    m = cases.product_model(c)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    cfg = get_default_configs()
    cfg.TRAIN.LOSS_CLIP_VALUE = 1e9
    for k, v in loss_fields.items():
        setattr(cfg.TRAIN.LOSS, k, v)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    value, stepped = ActiveLearningStrategy(cfg).train_step(m, opt, data)
    torch.cuda.synchronize()
    return value, stepped, {k: t.detach().cpu().numpy().copy() for k, t in m.state_dict().items()}


def _train_batch(c, kind, dev, v=2):
    """The batch test_gpu_loss_points trains the case on (frames of v views): {images, per_view_joint_valid} with gt_heatmap, or with
    gt_points and gt_sigma."""
    from multi_view_active_learning_amd.utils import preprocess

    b = c["n"] // v
    x, _, valid = cases.train_input(c)
    hh, wh = c["h"] // 4, c["w"] // 4
    pt = _train_points(c)
    data = {"images": torch.from_numpy(x).reshape(b, v, 3, c["h"], c["w"]),
            "per_view_joint_valid": torch.from_numpy(valid).reshape(b, v, c["j"]).float()}
    if kind == "gt_heatmap":
        data["gt_heatmap"] = preprocess.gt_heatmaps(torch.from_numpy(pt).to(dev), 1.0, hh, wh).cpu().reshape(b, v, c["j"], hh, wh)
    else:
        data.update(gt_points=torch.from_numpy(pt).reshape(b, v, c["j"], 2), gt_sigma=torch.ones(b, dtype=torch.float64))
    return data, {k: torch.from_numpy(a) for k, a in cases.model_state_dict(c).items()}


@pytest.mark.parametrize("name,kind", [("r50_train", "gt_heatmap"), ("w32_train", "points")])
def test_train_step_under_ohkm(dev, name, kind):
    """One step from the same state dict under the default configuration, under OHKM_TOPK = J (all-ones weights on the valid maps, no new
    batch key: the weighted loss with nothing removed) and under OHKM_TOPK = 1: the second steps with a loss within 1 ulp of the first's,
    the third returns a strictly smaller positive loss and moves the parameters."""
    c = cases.train_cases()[name]
    data, sd = _train_batch(c, kind, dev)
    v0, s0, _ = _one_step(c, dev, sd, data)
    v1, s1, _ = _one_step(c, dev, sd, data, OHKM_TOPK=c["j"])
    v2, s2, p2 = _one_step(c, dev, sd, data, OHKM_TOPK=1)
    print("\n[weighted_loss] %s %s: default %r, topk = J %r, topk = 1 %r" % (name, kind, v0, v1, v2))
    assert s0 and s1 and s2
    assert _ulps(v0, v1) <= 1, (v0, v1)
    assert 0 < v2 < v1
    moved = [k for k in p2 if p2[k].dtype.kind == "f" and not np.array_equal(p2[k], sd[k].numpy())]
    assert len(moved) > len(p2) // 2, moved


@pytest.mark.parametrize("name,kind,views", [("r50_train", "points", 1), ("w32_train", "gt_heatmap", 2)])  # (two frames each)
def test_train_step_drops_pseudo_labels_at_weight_zero(dev, name, kind, views):
    """pseudo_label = [1, 0, ...] under PSEUDO_LABEL_WEIGHT = 0 against the same batch with frame 0's per_view_joint_valid zeroed and no
    pseudo-labelled frame: the same loss to the bit and identical parameters after the step.  Both go through the weighted loss (the key
    pseudo_label is in both batches), so the sums have one order; the default path's loss on the zeroed batch is within 1 ulp."""
    c = cases.train_cases()[name]
    data, sd = _train_batch(c, kind, dev, views)
    b = data["images"].shape[0]
    assert b == 2
    pseudo = torch.zeros(b, dtype=torch.int64)
    pseudo[0] = 1
    zeroed = data["per_view_joint_valid"].clone()
    zeroed[0] = 0
    va, sa, pa = _one_step(c, dev, sd, dict(data, pseudo_label=pseudo), PSEUDO_LABEL_WEIGHT=0.0)
    vb, sb, pb = _one_step(c, dev, sd, dict(data, pseudo_label=torch.zeros(b, dtype=torch.int64), per_view_joint_valid=zeroed), PSEUDO_LABEL_WEIGHT=0.0)
    vc, sc, pc = _one_step(c, dev, sd, dict(data, per_view_joint_valid=zeroed))
    print("\n[weighted_loss] %s %s: pseudo at weight 0 %r, zeroed %r, zeroed on the default path %r" % (name, kind, va, vb, vc))
    assert sa and sb and sc and va > 0
    assert np.float32(va).view(np.int32) == np.float32(vb).view(np.int32), (va, vb)
    assert _ulps(va, vc) <= 1, (va, vc)
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
        np.testing.assert_array_equal(pa[k], pc[k], err_msg=k)  # the gradient has the masked loss's bits


# ---- 7. empty and zero -----------------------------------------------------------------------------------------------------------
def test_no_maps(dev):
    from multi_view_active_learning_amd import _lib

    h = torch.empty((0,), dtype=torch.float32, device=dev)
    pt = torch.empty((0, 2), dtype=torch.float64, device=dev)
    w = torch.empty((0,), dtype=torch.float32, device=dev)
    go = torch.ones((), dtype=torch.float32, device=dev)
    for out in (_lib.weighted_mse_fwd(h, h, w, 0, 0, 19, 17, 23), _lib.weighted_mse_points_fwd(h, pt, 1.0, w, 3, 0, 19, 17, 23)):
        assert _i32(out[0]) == 0 and out[1].numel() == 0 and out[2].numel() == 0
    assert _lib.weighted_mse_bwd(h, h, w, go, 0, 19, 17, 23).numel() == 0
    assert _lib.weighted_mse_points_bwd(h, pt, 1.0, w, go, 0, 19, 17, 23).numel() == 0


@pytest.mark.parametrize("form", ["read", "points"])
def test_all_weights_zero_touches_no_map(dev, form):
    """Every weight 0 over heat-maps, targets and points that are NaN throughout: the loss is +0.0, per_map and wsel are +0.0, and the
    gradient is +0.0 everywhere -- no map was read."""
    n, j, hh, wh = 3, 19, 7, 9
    nan = torch.full((n * j * hh * wh,), float("nan"), dtype=torch.float32, device=dev)
    c = dict(n=n, j=j, hh=hh, wh=wh, h=nan, g=nan, pt=torch.full((n * j, 2), float("nan"), dtype=torch.float64, device=dev), sigma=1.0)
    zero = torch.zeros(n * j, dtype=torch.float32, device=dev)
    for topk in (0, 8):
        loss, per_map, wsel = _forward(c, form, zero, topk)
        assert _i32(loss) == 0 and not _i64(per_map).any() and not _i32(wsel).any()
        assert not _i32(_backward(c, form, wsel, 1.0)).any()

"""GPU tests of the training loss against rendered ground truth (csrc/loss_metric.hip: mval_masked_mse_points_fwd / _bwd) and of the
compact batch built on it: key-point targets and uint8 views through pose_2d_mse_from_points, train_step, _compute_batch_heatmap and
prepare_views(compact=True).

The contract is bit identity with the read form (mval_masked_mse_fwd / _bwd) on the maps mval_gt_heatmaps writes: the same grid, element ->
thread map and float64 accumulation order, so every comparison below is of int32 views.  The maps themselves are pinned to the reference by
the mval_gt_heatmaps goldens (tests/test_gpu_hotpath.py, tests/test_gpu_preprocess_edges.py).  Inputs come from seeds; nothing is stored."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


def _misaligned(t):
    """A copy of the flat device tensor ``t`` whose first element sits one float past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1 : 1 + t.numel()]
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# (lead, h, w, h one float past a 16-byte boundary)
SHAPES = [
    (1, 5, 13, False),      # 65 pixels: scalar walk, one map
    (9, 7, 9, False),       # 63 pixels: scalar walk, odd map bases
    (10, 8, 8, False),      # float4 walk
    (35, 64, 48, False),    # float4 walk
    (152, 96, 72, False),   # 1 050 624 elements > 1 048 576: the float4 walk makes a second trip
    (700, 17, 23, False),   # 273 700 elements, hw % 4 = 3, > 262 144: the scalar walk makes a second trip
    (10, 8, 8, True),       # hw % 4 == 0 but h misaligned: scalar walk, against the read form with both tensors offset alike
]
SHAPE_IDS = ["%dx%dx%d%s" % (s[0], s[1], s[2], "-offset" if s[3] else "") for s in SHAPES]
NAN_MAP = 7  # the map whose point is NaN where a mask hides it


def _points(rng, lead, h, w, with_nan):
    pt = np.stack([rng.uniform(0, w - 1, lead), rng.uniform(0, h - 1, lead)], 1)
    special = [(3.0, 2.0),                 # exactly on a pixel centre
               (2.5, 1.25),                # between pixels
               (-3.2, 1.0), (w + 2.7, 2.0), (1.0, -4.1), (2.0, h + 3.3),  # outside the map on each side
               (1.0e4, 1.0e4)]             # so far away that the whole map is 0.0f
    for i, p in enumerate(special[:lead]):
        pt[i] = p
    if with_nan and lead > NAN_MAP:
        pt[NAN_MAP] = (np.nan, 3.0)
    return pt


_CASES = {}


def _case(dev, shape, mask, sigmas):
    """One seeded case, built once and shared by the tests (none of them writes into it): heat-maps, points, sigma (a float or one per map),
    the mask, and the maps ``gt_heatmaps`` renders from the points -- per sigma group with its own call."""
    key = (shape, mask, sigmas)
    if key in _CASES:
        return _CASES[key]
    from multi_view_active_learning_amd.utils import preprocess

    lead, h, w, offset = shape
    rng = np.random.default_rng(1000 * lead + 10 * h + w)
    hm = torch.from_numpy(rng.standard_normal(lead * h * w).astype(np.float32) * 0.5).to(dev)
    valid = {"none": None, "some": (rng.uniform(size=lead) > 0.3).astype(np.uint8), "zero": np.zeros(lead, np.uint8)}[mask]
    if mask == "some":
        valid[0] = 1
        if lead > NAN_MAP:
            valid[NAN_MAP] = 0
    pt = torch.from_numpy(_points(rng, lead, h, w, mask != "none")).to(dev)
    if sigmas == "one":
        sigma = 1.5
        g = preprocess.gt_heatmaps(pt, sigma, h, w)
    else:
        sigma = rng.choice([0.5, 1.0, 2.0], size=lead)
        sigma[:3] = [0.5, 1.0, 2.0][: min(3, lead)]
        g = torch.empty((lead, h, w), dtype=torch.float32, device=dev)
        for s in (0.5, 1.0, 2.0):
            idx = torch.from_numpy(np.flatnonzero(sigma == s)).to(dev)
            if idx.numel():
                g[idx] = preprocess.gt_heatmaps(pt[idx], s, h, w)
    g = g.reshape(-1)
    if offset:
        hm, g = _misaligned(hm), _misaligned(g)
    c = dict(h=hm, g=g, pt=pt, sigma=sigma, valid=None if valid is None else torch.from_numpy(valid).to(dev), valid_np=valid,
             lead=lead, hh=h, wh=w, denom=float(max(1, lead // 19) * h * w))
    if mask != "none" and lead > NAN_MAP:
        assert torch.isnan(g.reshape(lead, -1)[NAN_MAP]).all()  # the read form's map under the mask is NaN throughout
    if lead > 6:
        assert not g.reshape(lead, -1)[6].any()  # the far point's map is 0.0f everywhere
    _CASES[key] = c
    return c


def _i32(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _fwd_both(c):
    from multi_view_active_learning_amd import _lib

    a = _lib.masked_mse_points_fwd(c["h"], c["pt"], c["sigma"], c["valid"], c["lead"], c["hh"], c["wh"], c["denom"])
    b = _lib.masked_mse_fwd(c["h"], c["g"], c["valid"], c["lead"], c["hh"] * c["wh"], c["denom"])
    return a, b


def _bwd_both(c, grad):
    from multi_view_active_learning_amd import _lib

    go = torch.tensor(grad, dtype=torch.float32, device=c["h"].device)
    a = _lib.masked_mse_points_bwd(c["h"], c["pt"], c["sigma"], c["valid"], go, c["lead"], c["hh"], c["wh"], c["denom"])
    b = _lib.masked_mse_bwd(c["h"], c["g"], c["valid"], go, c["lead"], c["hh"] * c["wh"], c["denom"])
    return a, b


@pytest.mark.parametrize("sigmas", ["one", "per_map"])
@pytest.mark.parametrize("mask", ["none", "some", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_forward_bits(dev, shape, mask, sigmas):
    """1. The loss has the read form's bits on the rendered maps, on both walks, at one and at two grid-stride trips, with no mask, a mixed
    mask (a NaN point under a masked map: finite, and equal) and every map masked (exactly 0.0)."""
    c = _case(dev, shape, mask, sigmas)
    a, b = _fwd_both(c)
    assert np.isfinite(a.item())
    assert _i32(a) == _i32(b), (a.item(), b.item())
    if mask == "zero":
        assert _i32(a) == 0


@pytest.mark.parametrize("grad", [1.0, 0.37])
@pytest.mark.parametrize("sigmas", ["one", "per_map"])
@pytest.mark.parametrize("mask", ["none", "some", "zero"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_backward_bits(dev, shape, mask, sigmas, grad):
    """2. grad_h equals the read form's element for element in bits; masked maps are exactly +0.0 (the NaN point's among them)."""
    c = _case(dev, shape, mask, sigmas)
    a, b = _bwd_both(c, grad)
    a, b = _i32(a).reshape(c["lead"], -1), _i32(b).reshape(c["lead"], -1)
    bad = np.flatnonzero((a != b).any(1))
    assert bad.size == 0, "maps %r differ" % (bad[:10].tolist(),)
    if c["valid_np"] is not None:
        assert not a[c["valid_np"] == 0].any()
    else:
        assert a.any()


@pytest.mark.parametrize("sigmas", ["one", "per_map"])
@pytest.mark.parametrize("mask", ["none", "some"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_against_float64(dev, shape, mask, sigmas):
    """3. Against numpy on the downloaded maps: float32(h - g), its float32 square, float64 sums.  The bounds are the project's for this loss
    (tests/test_gpu_post_edges.py::_mse_check): 2e-6 relative on the loss, rtol 1e-6 / atol 1e-12 on the gradient."""
    c = _case(dev, shape, mask, sigmas)
    lead, denom, grad = c["lead"], c["denom"], 0.37
    h = c["h"].cpu().numpy().reshape(lead, -1)
    g = c["g"].cpu().numpy().reshape(lead, -1)
    m = np.ones((lead, 1), bool) if c["valid_np"] is None else c["valid_np"].astype(bool)[:, None]
    d = np.where(m, (h - g).astype(np.float32), np.float32(0))
    want = float((d * d).astype(np.float32).astype(np.float64).sum() / denom)
    want_g = 2.0 * d.astype(np.float64) * (float(np.float32(grad)) / denom)
    loss = _fwd_both(c)[0].item()
    gh = _bwd_both(c, grad)[0].cpu().numpy().reshape(lead, -1)
    assert abs(loss - want) <= 2e-6 * abs(want), (loss, want)
    np.testing.assert_allclose(gh, want_g, rtol=1e-6, atol=1e-12)


def test_no_maps(dev):
    """lead == 0 as in the read form: the forward writes 0 / denom = 0, the backward launches nothing."""
    from multi_view_active_learning_amd import _lib

    h = torch.empty((0,), dtype=torch.float32, device=dev)
    pt = torch.empty((0, 2), dtype=torch.float64, device=dev)
    assert _lib.masked_mse_points_fwd(h, pt, 1.0, None, 0, 17, 23, 391.0).item() == 0.0
    assert _lib.masked_mse_points_bwd(h, pt, 1.0, None, torch.ones((), dtype=torch.float32, device=dev), 0, 17, 23, 391.0).numel() == 0


# ---- autograd ----------------------------------------------------------------------------------------------------------
def _autograd_inputs(dev, n, j, hh, wh, seed):
    rng = np.random.default_rng(seed)
    hm = torch.from_numpy(rng.standard_normal((n, j, hh, wh)).astype(np.float32) * 0.5).to(dev)
    pt = torch.from_numpy(np.stack([rng.uniform(-2, wh + 1, (n, j)), rng.uniform(-2, hh + 1, (n, j))], -1)).to(dev)
    valid = torch.from_numpy(rng.uniform(size=(n, j, 1, 1)) > 0.25).to(dev)
    return hm, pt, valid


@pytest.mark.parametrize("sigma_kind", ["scalar", "per_image"])
@pytest.mark.parametrize("masked", [False, True])
def test_autograd_equals_the_read_form(dev, sigma_kind, masked):
    """4. pose_2d_mse_from_points and pose_2d_mse on the materialised maps: the same loss bits and the same heatmaps.grad bits, for a scalar
    sigma, a per-image sigma (N,) and a (N, J, 1, 1) mask; the loss is scaled by 0.37 so that grad_out is not 1."""
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError
    from multi_view_active_learning_amd.utils import preprocess

    n, j, hh, wh = 6, 19, 16, 12
    hm, pt, valid = _autograd_inputs(dev, n, j, hh, wh, 5)
    valid = valid if masked else None
    if sigma_kind == "scalar":
        sigma = 1.25
        g = preprocess.gt_heatmaps(pt, sigma, hh, wh)
    else:
        sigma = np.array([1.0, 2.0, 1.0, 0.5, 2.0, 1.0])
        g = torch.stack([preprocess.gt_heatmaps(pt[i], float(sigma[i]), hh, wh) for i in range(n)])
    loss = Pose2DMeanSquaredError()
    got = []
    for form in ("points", "read"):
        x = hm.clone().requires_grad_(True)
        out = loss.pose_2d_mse_from_points(x, pt, sigma, valid) if form == "points" else loss.pose_2d_mse(x, g, valid)
        (out * 0.37).backward()
        got.append((_i32(out), _i32(x.grad)))
    assert got[0][0] == got[1][0]
    np.testing.assert_array_equal(got[0][1], got[1][1])
    assert got[0][1].any()


def test_autograd_keeps_no_ground_truth(dev):
    """4. Allocated device memory after the forward, with the graph alive: the read form holds the (N, J, h, w) maps it was given, the points
    form holds less than one such tensor on top of the heat-maps (the points, the mask, the scalar loss)."""
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError
    from multi_view_active_learning_amd.utils import preprocess

    n, j, hh, wh = 8, 19, 64, 64
    map_bytes = n * j * hh * wh * 4
    hm, pt, valid = _autograd_inputs(dev, n, j, hh, wh, 6)
    loss = Pose2DMeanSquaredError()
    x = hm.requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    out_p = loss.pose_2d_mse_from_points(x, pt, 1.0, valid)
    torch.cuda.synchronize()
    d_points = torch.cuda.memory_allocated() - base
    g = preprocess.gt_heatmaps(pt, 1.0, hh, wh)
    out_r = loss.pose_2d_mse(x, g, valid)
    del g  # the graph keeps it
    torch.cuda.synchronize()
    d_read = torch.cuda.memory_allocated() - base - d_points
    assert _i32(out_p) == _i32(out_r)
    assert d_read >= map_bytes, (d_read, map_bytes)
    assert 0 <= d_points < map_bytes // 8, (d_points, map_bytes)


def test_mixed_sal_batch(dev):
    """5. Two frames x two views in one batch, frame 0 labelled (DATA.SIGMA = 1.0), frame 1 pseudo-labelled (gt_sigma = 2.0): the loss and the
    gradient of the points form equal the read form's on maps rendered frame by frame."""
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy, select_train_target
    from multi_view_active_learning_amd.utils import preprocess

    cfg = get_default_configs()
    cfg.DATA.SIGMA, cfg.DATA.PSEUDO_LABEL_SIGMA = 1.0, 2.0
    b, v, j, hh, wh = 2, 2, 19, 16, 16
    hm, pt, valid = _autograd_inputs(dev, b * v, j, hh, wh, 7)
    data = {"gt_points": pt.reshape(b, v, j, 2).cpu(), "gt_sigma": np.array([cfg.DATA.SIGMA, cfg.DATA.PSEUDO_LABEL_SIGMA])}
    kind, target, sigma = select_train_target(data, cfg)
    assert kind == "points"
    target, sigma = ActiveLearningStrategy._stage_train_points(target, sigma)
    assert target.is_cuda and sigma.is_cuda and sigma.cpu().tolist() == [1.0, 1.0, 2.0, 2.0]
    st = ActiveLearningStrategy(cfg)
    pv = valid.reshape(b, v, j).to(torch.uint8)
    g = torch.stack([preprocess.gt_heatmaps(pt.reshape(b, v, j, 2)[f], s, hh, wh) for f, s in enumerate((1.0, 2.0))])
    x_p, x_r = hm.clone().requires_grad_(True), hm.clone().requires_grad_(True)
    out_p = st._compute_batch_loss_points(target, sigma, x_p, pv, st.loss)
    out_r = st._compute_batch_loss(g, x_r, pv, st.loss)
    out_p.backward()
    out_r.backward()
    assert _i32(out_p) == _i32(out_r)
    np.testing.assert_array_equal(_i32(x_p.grad), _i32(x_r.grad))
    # and it is the sigmas that make the difference: one sigma for both frames gives another loss
    assert _i32(st._compute_batch_loss_points(target, 1.0, hm, pv, st.loss)) != _i32(out_r)


# ---- train_step --------------------------------------------------------------------------------------------------------
def _train_points(c):
    """The centres cases.train_input draws (same generator, same order), as float64 (n, j, 2) heat-map pixels."""
    rng = np.random.default_rng(c["seed"] + 1000)
    hh, wh = c["h"] // 4, c["w"] // 4
    pt = np.zeros((c["n"], c["j"], 2))
    for idx in np.ndindex(c["n"], c["j"]):
        pt[idx] = rng.uniform(0, wh - 1), rng.uniform(0, hh - 1)
    return pt


def _one_step(c, dev, sd, data):
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    m = cases.product_model(c)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    cfg = get_default_configs()
    cfg.DATA.SIGMA = 3.0  # not the batch's: gt_sigma must win
    cfg.TRAIN.LOSS_CLIP_VALUE = 1e9
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    value, stepped = ActiveLearningStrategy(cfg).train_step(m, opt, data)
    torch.cuda.synchronize()
    return value, stepped, {k: t.detach().cpu().numpy().copy() for k, t in m.state_dict().items()}


@pytest.mark.parametrize("name", ["r50_train", "w32_train"])
def test_train_step_from_points(dev, name):
    """6. One training step from {images, gt_heatmap} and one from {images, gt_points, gt_sigma}, both from the same state dict, with points
    whose rendered maps ARE the batch's gt_heatmap: the same loss value and the same ``stepped``.  The read-form step is run twice first:
    where its parameters are bit-reproducible the two forms' parameters must be equal bit for bit, where they are not, within the spread
    of the two read-form runs (per tensor, the largest absolute difference; the test prints which held).
    On the MI355X the read-form step was bit-reproducible for both r50_train and w32_train, so the first branch held: the parameters (and
    BatchNorm buffers) after the points-form step equal the read form's bit for bit."""
    from multi_view_active_learning_amd.utils import preprocess

    c = cases.train_cases()[name]
    v = 2
    b = c["n"] // v
    x, _, valid = cases.train_input(c)
    hh, wh = c["h"] // 4, c["w"] // 4
    pt = _train_points(c)
    gt = preprocess.gt_heatmaps(torch.from_numpy(pt).to(dev), 1.0, hh, wh).cpu()
    sd = {k: torch.from_numpy(a) for k, a in cases.model_state_dict(c).items()}
    common = {"images": torch.from_numpy(x).reshape(b, v, 3, c["h"], c["w"]),
              "per_view_joint_valid": torch.from_numpy(valid).reshape(b, v, c["j"]).float()}
    read = dict(common, gt_heatmap=gt.reshape(b, v, c["j"], hh, wh))
    points = dict(common, gt_points=torch.from_numpy(pt).reshape(b, v, c["j"], 2), gt_sigma=torch.ones(b, dtype=torch.float64))
    v1, s1, p1 = _one_step(c, dev, sd, read)
    v2, s2, p2 = _one_step(c, dev, sd, read)
    v3, s3, p3 = _one_step(c, dev, sd, points)
    assert s1 and s2 and s3
    assert v1 == v2 == v3, (v1, v2, v3)
    reproducible = all(np.array_equal(p1[k], p2[k], equal_nan=True) for k in p1)
    print("\n[loss_points] %s: read-form parameters bit-reproducible: %s" % (name, reproducible))
    for k in p1:
        if reproducible:
            np.testing.assert_array_equal(p3[k], p1[k], err_msg=k)
        else:
            spread = np.abs(p1[k].astype(np.float64) - p2[k].astype(np.float64)).max()
            dist = min(np.abs(p3[k].astype(np.float64) - p[k].astype(np.float64)).max() for p in (p1, p2))
            assert dist <= spread, (k, dist, spread)


# ---- uint8 views ---------------------------------------------------------------------------------------------------------
def test_uint8_views_through_the_model(dev):
    """7. _compute_batch_heatmap of (2, 2, H, W, 3) uint8 equals, bit for bit, that of normalize_views_u8(...) as (2, 2, 3, H, W) float32, on
    the r50 fixture at 128 x 96, the smallest input the suite runs that model at."""
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy
    from multi_view_active_learning_amd.utils import preprocess

    c = dict(cases.train_cases()["r50_train"], n=4)
    m = cases.product_model(c)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in cases.model_state_dict(c).items()}, strict=True)
    m = m.to(dev).eval()
    u8 = torch.from_numpy(np.random.default_rng(8).integers(0, 256, size=(2, 2, c["h"], c["w"], 3), dtype=np.uint8))
    f32 = preprocess.normalize_views_u8(u8.to(dev).reshape(4, c["h"], c["w"], 3)).reshape(2, 2, 3, c["h"], c["w"])
    with torch.no_grad():
        a = ActiveLearningStrategy._compute_batch_heatmap(m, {"images": u8}).clone()
        b = ActiveLearningStrategy._compute_batch_heatmap(m, {"images": f32.cpu()}).clone()
    assert a.shape == (4, c["j"], c["h"] // 4, c["w"] // 4) and torch.isfinite(a).all()
    np.testing.assert_array_equal(_i32(a), _i32(b))
    with pytest.raises(ValueError, match="uint8 images"):
        ActiveLearningStrategy._compute_batch_heatmap(m, {"images": u8.permute(0, 1, 4, 2, 3).contiguous()})


def test_prepare_views_compact(dev):
    """7. prepare_views(compact=True) on decoded test views (cases.resample_image, as tests/test_gpu_preprocess_edges.py builds them): images
    is resize_views_u8's, gt_points renders to the default call's gt_heatmap in bits and trains to the same loss bits, no gt_heatmap is
    returned, the other keys are equal, and the default call's key set is today's."""
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError
    from multi_view_active_learning_amd.utils import preprocess

    pc = cases.preprocess_cases()["outside"]
    _, kp3d, cam = cases.preprocess_inputs(pc)
    imgs = [torch.from_numpy(cases.resample_image(k, pc["h0"], pc["w0"], seed=s)).to(dev) for k, s in (("noise", 1), ("stripes", 0), ("checker", 0))]
    boxes = [pc["box"], (10, 20, 130, 170), (-15, -5, 200, 120)]
    args = (imgs, boxes, [cam] * 3, kp3d, pc["scale"], pc["in_w"], pc["in_h"], pc["stride"], pc["sigma"])
    full = preprocess.prepare_views(*args)
    small = preprocess.prepare_views(*args, compact=True)
    assert set(full) == {"images", "gt_heatmap", "proj_matrices", "2d_keypoints", "2d_after_crop", "square_box"}
    assert set(small) == (set(full) - {"gt_heatmap"}) | {"gt_points"}
    sq = [preprocess.scale_bbox(preprocess.get_square_bbox(tuple(bx)), pc["scale"]) for bx in boxes]
    assert small["images"].dtype == torch.uint8 and small["images"].shape == (3, pc["in_h"], pc["in_w"], 3)
    assert torch.equal(small["images"], preprocess.resize_views_u8(imgs, sq, pc["in_w"], pc["in_h"]))
    np.testing.assert_array_equal(_i32(preprocess.normalize_views_u8(small["images"])), _i32(full["images"]))
    hh, wh = pc["in_h"] // pc["stride"], pc["in_w"] // pc["stride"]
    pts = small["gt_points"]
    assert pts.is_cuda and pts.dtype == torch.float64 and pts.shape == (3, 19, 2)
    np.testing.assert_array_equal(_i32(preprocess.gt_heatmaps(pts, pc["sigma"], hh, wh)), _i32(full["gt_heatmap"]))
    for k in ("proj_matrices", "2d_keypoints", "2d_after_crop", "square_box"):
        np.testing.assert_array_equal(small[k], full[k], err_msg=k)
    hm = torch.from_numpy(np.random.default_rng(9).standard_normal((3, 19, hh, wh)).astype(np.float32)).to(dev)
    loss = Pose2DMeanSquaredError()
    assert _i32(loss.pose_2d_mse_from_points(hm, pts, pc["sigma"])) == _i32(loss.pose_2d_mse(hm, full["gt_heatmap"]))


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """8. sigma <= 0 (or NaN) as a scalar, null arguments, non-positive sizes and hh * wh past INT32_MAX - 1024 return -1 from the C entries with
    mval_last_error() naming the entry, and nothing is launched: out and grad_h keep their sentinels.  A sigma <= 0 inside an array and points
    that are not (N, J, 2) are refused by the wrappers that upload them (the entries cannot read a device array without a synchronise), with
    the entry's name in the message."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.pose_estimators.loss import Pose2DMeanSquaredError

    lib = _lib.lib()
    lead, hh, wh = 3, 4, 5
    h = torch.zeros(lead * hh * wh, dtype=torch.float32, device=dev)
    pt = torch.ones((lead, 2), dtype=torch.float64, device=dev)
    out = torch.full((), 7.0, dtype=torch.float32, device=dev)
    ws = torch.zeros(2048, dtype=torch.float64, device=dev)
    go = torch.ones((), dtype=torch.float32, device=dev)
    gh = torch.full_like(h, 7.0)
    sm = torch.ones(lead, dtype=torch.float64, device=dev)
    ok = dict(h=h, pt=pt, sigma=1.0, sm=None, out=out, ws=ws, go=go, gh=gh, lead=lead, hh=hh, wh=wh, denom=20.0)

    def fwd(a):
        return lib.mval_masked_mse_points_fwd(_lib._p(a["h"]), _lib._p(a["pt"]), C.c_double(a["sigma"]), _lib._p(a["sm"]), _lib._p(None), _lib._p(a["out"]),
                                              _lib._p(a["ws"]), C.c_longlong(a["lead"]), C.c_int(a["hh"]), C.c_int(a["wh"]), C.c_double(a["denom"]), _lib._stream())

    def bwd(a):
        return lib.mval_masked_mse_points_bwd(_lib._p(a["h"]), _lib._p(a["pt"]), C.c_double(a["sigma"]), _lib._p(a["sm"]), _lib._p(None), _lib._p(a["go"]),
                                              _lib._p(a["gh"]), C.c_longlong(a["lead"]), C.c_int(a["hh"]), C.c_int(a["wh"]), C.c_double(a["denom"]), _lib._stream())

    both = [dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(h=None), dict(pt=None), dict(hh=0), dict(wh=-1), dict(lead=-1),
            dict(denom=0.0), dict(hh=65536, wh=65536), dict(hh=46341, wh=46341)]
    for bad in both + [dict(out=None), dict(ws=None)]:
        assert fwd(dict(ok, **bad)) == -1 and b"mval_masked_mse_points_fwd" in lib.mval_last_error(), bad
    for bad in both + [dict(go=None), dict(gh=None)]:
        assert bwd(dict(ok, **bad)) == -1 and b"mval_masked_mse_points_bwd" in lib.mval_last_error(), bad
    torch.cuda.synchronize()
    assert out.item() == 7.0 and bool((gh == 7.0).all())
    # the scalar is not looked at where per-map sigmas are given, and the good call goes through
    assert fwd(dict(ok, sigma=0.0, sm=sm)) == 0 and bwd(dict(ok, sigma=0.0, sm=sm)) == 0 and fwd(ok) == 0 and bwd(ok) == 0
    torch.cuda.synchronize()
    assert out.item() != 7.0 and not bool((gh == 7.0).any())

    for sig in (np.array([1.0, 0.0, 1.0]), torch.tensor([1.0, -2.0, 1.0]), np.array([1.0, np.nan, 1.0])):
        with pytest.raises(_lib.MvalError, match="mval_masked_mse_points_fwd.*positive"):
            _lib.masked_mse_points_fwd(h, pt, sig, None, lead, hh, wh, 20.0)
        with pytest.raises(_lib.MvalError, match="mval_masked_mse_points_bwd.*positive"):
            _lib.masked_mse_points_bwd(h, pt, sig, None, go, lead, hh, wh, 20.0)
    with pytest.raises(_lib.MvalError, match="mval_masked_mse_points_fwd.*sigmas"):
        _lib.masked_mse_points_fwd(h, pt, np.ones(lead + 1), None, lead, hh, wh, 20.0)
    with pytest.raises(_lib.MvalError, match="mval_masked_mse_points_fwd.*points"):
        _lib.masked_mse_points_fwd(h, pt[:2], 1.0, None, lead, hh, wh, 20.0)
    loss = Pose2DMeanSquaredError()
    hm = h.reshape(1, lead, hh, wh)
    for bad_pt in (pt, pt.reshape(1, lead * 2), torch.ones((1, lead, 3), dtype=torch.float64, device=dev), torch.ones((1, lead + 1, 2), device=dev)):
        with pytest.raises(_lib.MvalError, match="points"):
            loss.pose_2d_mse_from_points(hm, bad_pt, 1.0)
    for bad_sigma in (0.0, -1.0, float("nan"), np.array([1.0, 0.0, 1.0]), np.array([[-1.0]])):
        with pytest.raises(_lib.MvalError, match="positive"):
            loss.pose_2d_mse_from_points(hm, pt.reshape(1, lead, 2), bad_sigma)

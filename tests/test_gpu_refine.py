"""GPU tests of the sub-pixel decode: ``mval_refine_keypoints`` against the float64 oracle of
tests/refine_oracle.py -- conf and the quarter offsets bit for bit, the taylor points equal or adjacent float32 (the float64 log of
the device and numpy's may differ in their last bit, which cannot move a result by more than its final float32 rounding) --, a point
outside its map, and the calls that carry the refinement: triangulate_batch (plain, under both masks, from the network's arg-max
keys), the scoring pass and the evaluation."""
import numpy as np
import pytest
import torch

import cases
import refine_oracle as ro
from multi_view_active_learning_amd import synth

pytestmark = pytest.mark.gpu
MARGIN = 1e-6  # every accept decision of the oracle is at least this far from flipping: far above an ulp of a float64 log


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _same_bits(a, b):
    """torch.equal that takes NaN for what it is: the same bits."""
    if a.dtype.is_floating_point:
        as_int = torch.int64 if a.dtype == torch.float64 else torch.int32
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _equal_or_adjacent(got, want):
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    return (got == want) | (got == up) | (got == down)


# ---- the kernel against the oracle -------------------------------------------------------------------------------------------
SHAPES = [(2, 3, 5, 8, 8), (1, 2, 3, 12, 16), (3, 2, 19, 6, 5), (2, 3, 43, 5, 5)]


def _planted(hh, wh):
    """Maps that reach every branch, each (name, map, peak or None): ``peak`` is handed to the kernel in place of the map's own
    arg-max (only the plateau needs that)."""
    out = []
    for name, block in (("ok", ro.BLOCK_OK), ("far", ro.BLOCK_FAR), ("notmax", ro.BLOCK_NOTMAX)):
        out.append((name, ro.block_map(block, hh, wh), None))
    out.append(("plateau", ro.block_map(ro.BLOCK_PLATEAU, hh, wh), (2, 2)))
    rng = np.random.default_rng(hh * 100 + wh)
    for px, py in [(0, 0), (wh - 1, 0), (0, hh - 1), (wh - 1, hh - 1), (2, 0), (2, hh - 1), (0, 2), (wh - 1, 2)]:
        m = rng.uniform(0.1, 0.5, (hh, wh)).astype(np.float32)
        m[py, px] = 1.0
        out.append(("border", m, None))
    m = ro.block_map(ro.BLOCK_OK, hh, wh)
    m[2, 2] = np.nan
    out.append(("nan_peak", m, None))
    m = ro.block_map(ro.BLOCK_OK, hh, wh)
    m[2, 2] = m[2, 3] = np.inf  # (the neighbour comes later in the flat order: the peak stays at (2, 2))
    out.append(("inf_neighbour", m, None))
    m = ro.block_map(ro.BLOCK_OK, hh, wh)
    m[3, 3] = -np.inf
    out.append(("minus_inf_neighbour", m, None))
    m = np.full((hh, wh), -0.5, np.float32)  # negative neighbours: the 1e-10 floor under the logarithm
    m[2, 2], m[2, 3], m[2, 1], m[1, 2], m[3, 2], m[3, 3] = 1.0, 0.25, -0.125, 0.5, 0.0, -0.0
    out.append(("negative_neighbours", m, None))
    m = np.full((hh, wh), -1.0, np.float32)
    m[2, 2] = 0.0
    out.append(("nonpos", m, None))
    return out


_CASES = {}


def _case(shape, stride):
    """(hm, valid, kp_in, oracle results per method) of one shape: synth-style Gaussians with noise 0.02 and the planted maps.  The
    noise seed is advanced until every taylor decision of the ORACLE is at least MARGIN from flipping; no map is left out."""
    if (shape, stride) in _CASES:
        return _CASES[(shape, stride)]
    b, v, j, hh, wh = shape
    n_maps = b * v * j
    plants = _planted(hh, wh)
    valid = np.ones((b, j), np.uint8)
    valid[0, j // 2] = 0
    if b > 1:
        valid[b - 1, j - 1] = 0
    free = np.flatnonzero(np.broadcast_to(valid[:, None, :], (b, v, j)).reshape(-1))  # (a planted map keeps a valid joint)
    if len(free) < len(plants) + 4:  # the smallest batch: three of them, the other maps stay Gaussians
        plants = [next(p for p in plants if p[0] == name) for name in ("nan_peak", "negative_neighbours", "ok")]
    at = free[np.linspace(0, len(free) - 1, len(plants)).astype(int)]  # spread over the batch, its first and last valid map included
    assert len(set(at.tolist())) == len(plants)
    ys, xs = np.mgrid[0:hh, 0:wh].astype(np.float32)
    for seed in range(100):
        rng = np.random.default_rng([seed, hh, wh, n_maps])
        cx, cy = rng.uniform(1.0, wh - 2.0, n_maps), rng.uniform(1.0, hh - 2.0, n_maps)
        hm = np.exp(-((xs[None] - cx[:, None, None].astype(np.float32)) ** 2 + (ys[None] - cy[:, None, None].astype(np.float32)) ** 2) / np.float32(2.0))
        hm = (hm + 0.02 * rng.standard_normal(hm.shape, dtype=np.float32)).astype(np.float32)
        for i, (_, m, _) in zip(at, plants):
            hm[i] = m
        hm = hm.reshape(shape)
        kp_in = ro.hard_decode(hm, stride, valid)
        for i, (_, _, peak) in zip(at, plants):
            if peak is not None:
                kp_in.reshape(n_maps, 2)[i] = np.asarray(peak) * stride
        kp_in[valid[:, None, :].repeat(v, 1) == 0] = 0
        want = {method: ro.refine_batch(hm, stride, method, valid, kp_in) for method in ro.METHODS}
        if (np.abs(want["taylor"][3]) >= MARGIN).all():
            break
    else:
        raise AssertionError("no noise seed keeps every taylor decision %g from flipping" % MARGIN)
    _CASES[(shape, stride)] = hm, valid, kp_in, want, [p[0] for p in plants], at
    return _CASES[(shape, stride)]


@pytest.mark.parametrize("shape", SHAPES, ids=["8x8", "12x16", "6x5", "5x5_258maps"])
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("method", ro.METHODS)
def test_kernel_equals_the_oracle(dev, method, stride, shape):
    from multi_view_active_learning_amd import _lib

    b, v, j, hh, wh = shape
    hm, valid, kp_in, want, names, at = _case(shape, stride)
    kp_w, conf_w, status, margin = want[method]
    assert (np.abs(want["taylor"][3]) >= MARGIN).all()  # (on the oracle, before anything is compared)
    flat = status.reshape(-1)
    if b * v * j >= 30:  # every branch is reached
        seen = set(want["taylor"][2].reshape(-1).tolist())
        assert seen == set(ro.STATUSES), seen
    for i, name in zip(at, names):
        expect = {"plateau": "notmax", "nan_peak": "nonfinite", "inf_neighbour": "nonfinite", "minus_inf_neighbour": "nonfinite",
                  "negative_neighbours": None}.get(name, name)
        if method == "quarter" and expect in ("far", "notmax", "nonpos"):
            expect = "ok"
        assert expect is None or flat[i] == expect, (name, flat[i])
    t_hm, t_valid = torch.from_numpy(hm).to(dev), torch.from_numpy(valid).to(dev)
    # the device's own hard decode, split by the width, is the oracle's (the plateau's peak is the one entry handed in)
    own = _lib.argmax_decode(t_hm, t_valid, b, v, j, hh, wh, stride, wh).cpu().numpy()
    differs = (own != kp_in).any(-1).reshape(-1)
    assert set(np.flatnonzero(differs).tolist()) <= {int(i) for i, n in zip(at, names) if n == "plateau"}
    kp, conf = _lib.refine_keypoints(t_hm, torch.from_numpy(kp_in).to(dev), t_valid, b, v, j, hh, wh, stride, method)
    assert kp.shape == (b, v, j, 2) and kp.dtype == torch.float32 and conf.shape == (b, v, j) and conf.dtype == torch.float32
    kp, conf = kp.cpu().numpy(), conf.cpu().numpy()
    np.testing.assert_array_equal(_bits(conf), _bits(conf_w))
    if method == "quarter":
        np.testing.assert_array_equal(_bits(kp), _bits(kp_w))
    else:
        ok = _equal_or_adjacent(kp, kp_w)
        print("taylor %s stride %d: %d of %d coordinates adjacent, not equal" % (shape, stride, int((kp != kp_w).sum()), kp.size))
        assert ok.all(), (kp[~ok], kp_w[~ok], status[~ok.all(-1)])
    assert (kp[valid[:, None, :].repeat(v, 1) == 0] == 0).all() and (conf[valid[:, None, :].repeat(v, 1) == 0] == 0).all()
    moved = (kp != kp_in.astype(np.float32)).any(-1)
    assert moved.sum() > moved.size // 4  # (the refinement does something on this input)


@pytest.mark.parametrize("method", ro.METHODS)
def test_without_valid_and_without_conf(dev, method):
    """valid = NULL (every joint decoded) and conf = NULL (not written) are accepted by the entry."""
    import ctypes as C

    from multi_view_active_learning_amd import _lib

    shape = SHAPES[0]
    b, v, j, hh, wh = shape
    hm, _, _, _, _, _ = _case(shape, 4)
    kp_in = ro.hard_decode(hm, 4)
    kp_w, conf_w = ro.refine_batch(hm, 4, method)[:2]
    t_hm, t_kp = torch.from_numpy(hm).to(dev), torch.from_numpy(kp_in).to(dev)
    kp, conf = _lib.refine_keypoints(t_hm, t_kp, None, b, v, j, hh, wh, 4, method)
    np.testing.assert_array_equal(_bits(conf.cpu().numpy()), _bits(conf_w))
    assert _equal_or_adjacent(kp.cpu().numpy(), kp_w).all()
    out = torch.full((b, v, j, 2), -7.0, dtype=torch.float32, device=dev)
    rc = _lib.lib().mval_refine_keypoints(C.c_int(_lib.REFINE_IDS[method]), _lib._p(t_hm), _lib._p(t_kp), C.c_void_p(0), _lib._p(out),
                                          C.c_void_p(0), C.c_int(b), C.c_int(v), C.c_int(j), C.c_int(hh), C.c_int(wh), C.c_int(4), _lib._stream())
    assert rc == 0 and _same_bits(out, kp)
    with pytest.raises(_lib.MvalError):
        _lib.refine_keypoints(t_hm, t_kp, None, b, v, j, hh, wh, 4, "dark")
    with pytest.raises(_lib.MvalError):
        _lib.refine_keypoints(t_hm, t_kp, None, b, v, j, hh, wh, 0, method)
    empty = _lib.refine_keypoints(t_hm[:0], t_kp[:0], None, 0, v, j, hh, wh, 4, method)
    assert empty[0].shape == (0, v, j, 2) and empty[1].shape == (0, v, j)


@pytest.mark.parametrize("method", ro.METHODS)
def test_a_point_outside_the_map_is_handed_through(dev, method):
    """px = wh (what a decode split by the height can give on a non-square map), py = hh and a negative coordinate, each planted
    in a MIDDLE map of the batch -- even a missing check would read a neighbouring map, not unallocated memory.  The point
    comes back unrefined with conf NaN; every other map's result is unchanged."""
    from multi_view_active_learning_amd import _lib

    shape, stride = SHAPES[1], 4
    b, v, j, hh, wh = shape
    hm, valid, kp_in, _, _, _ = _case(shape, stride)
    valid = np.ones_like(valid)
    t_hm, t_valid = torch.from_numpy(hm).to(dev), torch.from_numpy(valid).to(dev)
    base_kp, base_conf = _lib.refine_keypoints(t_hm, torch.from_numpy(kp_in).to(dev), t_valid, b, v, j, hh, wh, stride, method)
    bad = kp_in.copy().reshape(-1, 2)
    plants = {1: (wh * stride, 3 * stride), 2: (2 * stride, hh * stride), 3: (-stride, 2 * stride), 4: (3 * stride, -1)}
    for i, xy in plants.items():
        bad[i] = xy
    kp, conf = _lib.refine_keypoints(t_hm, torch.from_numpy(bad.reshape(kp_in.shape)).to(dev), t_valid, b, v, j, hh, wh, stride, method)
    kp, conf = kp.cpu().numpy().reshape(-1, 2), conf.cpu().numpy().reshape(-1)
    for i, xy in plants.items():
        assert kp[i].tolist() == [float(xy[0]), float(xy[1])] and np.isnan(conf[i]), (i, kp[i], conf[i])
    rest = [i for i in range(b * v * j) if i not in plants]
    np.testing.assert_array_equal(_bits(kp[rest]), _bits(base_kp.cpu().numpy().reshape(-1, 2)[rest]))
    np.testing.assert_array_equal(_bits(conf[rest]), _bits(base_conf.cpu().numpy().reshape(-1)[rest]))


# ---- plumbing: triangulate_batch -----------------------------------------------------------------------------------------------
def _rig(noise, n=2, v=4, j=5, hh=24, wh=32, stride=4, seed=2):
    """The small rig of DESIGN.md 6.4: ring_cameras(v, 96, 128), joints_3d(1, n, j, sigma_mm=150), heat-map seed 2."""
    proj = np.stack([synth.ring_cameras(v, hh * stride, wh * stride)] * n)
    kp3d = synth.joints_3d(1, n, j, sigma_mm=150)
    hm = synth.gaussian_heatmaps(seed, proj, kp3d, hh, wh, stride, noise=noise)
    return hm, proj, kp3d


def _same_results(a, b, skip=()):
    assert set(a) - set(skip) == set(b) - set(skip)
    for k in a:
        if k not in skip:
            assert _same_bits(a[k], b[k]), k


@pytest.mark.parametrize("method", ro.METHODS)
def test_triangulate_batch_refines_then_triangulates(dev, method):
    """triangulate_batch(refine=m) is, bit for bit in every returned tensor, the unrefined triangulate_batch on the key-points
    ``_lib.refine_keypoints`` returned; ``triangulation`` and ``decode_keypoints`` hand the same points on."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import decode_keypoints, triangulate_batch, triangulation

    hm, proj, _ = _rig(0.02, v=3)
    b, v, j, hh, wh = hm.shape
    valid = np.ones((b, j), np.uint8)
    valid[1, 3] = 0
    t_hm, t_valid = torch.from_numpy(hm).to(dev), torch.from_numpy(valid).to(dev)
    hard = _lib.argmax_decode(t_hm, t_valid, b, v, j, hh, wh, 4, wh)
    kp, conf = _lib.refine_keypoints(t_hm, hard, t_valid, b, v, j, hh, wh, 4, method)
    got = triangulate_batch(t_hm, torch.from_numpy(proj), 4, torch.from_numpy(valid), refine=method)
    want = triangulate_batch(t_hm, torch.from_numpy(proj), 4, torch.from_numpy(valid), keypoints_2d=kp)
    _same_results(got, want, skip=("keypoints_conf",))
    assert _same_bits(got["keypoints_2d"], kp) and _same_bits(got["keypoints_conf"], conf) and "keypoints_conf" not in want
    for quirk in (True, False):  # no effect under a refinement; a hard decode handed in is refined, not decoded again
        _same_results(got, triangulate_batch(t_hm, torch.from_numpy(proj), 4, torch.from_numpy(valid), refine=method, mirror_nonsquare_quirk=quirk))
    _same_results(got, triangulate_batch(t_hm, torch.from_numpy(proj), 4, torch.from_numpy(valid), refine=method, keypoints_2d=hard))
    plain = triangulate_batch(t_hm, torch.from_numpy(proj), 4, torch.from_numpy(valid), mirror_nonsquare_quirk=False)
    assert plain["keypoints_2d"].dtype == torch.int64 and torch.equal(plain["keypoints_2d"], hard) and "keypoints_conf" not in plain
    assert not _same_bits(plain["keypoints_3d"], got["keypoints_3d"])
    d_kp, d_conf = decode_keypoints(t_hm, 4, torch.from_numpy(valid), refine=method)
    assert _same_bits(d_kp, kp) and _same_bits(d_conf, conf)
    d_kp, d_conf = decode_keypoints(t_hm, 4, torch.from_numpy(valid))
    assert d_conf is None and torch.equal(d_kp, _lib.argmax_decode(t_hm, t_valid, b, v, j, hh, wh, 4, hh))
    one = triangulation(t_hm[0], proj[0], 4, valid[0], refine=method)
    np.testing.assert_array_equal(_bits(one["keypoints_2d"]), _bits(kp[0].cpu().numpy()))
    np.testing.assert_array_equal(_bits(one["keypoints_conf"]), _bits(conf[0].cpu().numpy()))
    np.testing.assert_array_equal(_bits(one["keypoints_3d"]), _bits(got["keypoints_3d"][0].cpu().numpy()))
    assert "keypoints_conf" not in triangulation(t_hm[0], proj[0], 4, valid[0])


@pytest.mark.parametrize("mask", ["view_valid", "view_joint_valid"])
@pytest.mark.parametrize("method", ro.METHODS)
def test_triangulate_batch_refines_under_a_mask(dev, method, mask):
    """V = 3, J = 5: the same identity under ``view_valid`` and under ``view_joint_valid``; absent entries of keypoints_2d and
    keypoints_conf are 0, and maps of NaNs in absent views change nothing."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    hm, proj, _ = _rig(0.02, v=3)
    b, v, j, hh, wh = hm.shape
    valid = torch.ones(b, j, dtype=torch.uint8)
    if mask == "view_valid":
        m = np.array([[1, 0, 1], [1, 1, 1]], bool)
        present = np.broadcast_to(m[:, :, None], (b, v, j))
    else:
        m = np.ones((b, v, j), bool)
        m[0, 1, 2] = m[1, 0, 4] = m[1, 2, 0] = False
        m[0, :2, 3] = False  # one view left: not used
        present = m
    kw = {mask: torch.from_numpy(m)}
    t_hm = torch.from_numpy(hm).to(dev)
    hard = _lib.argmax_decode(t_hm, valid.to(dev), b, v, j, hh, wh, 4, wh)
    kp, conf = _lib.refine_keypoints(t_hm, hard, valid.to(dev), b, v, j, hh, wh, 4, method)
    got = triangulate_batch(t_hm, torch.from_numpy(proj), 4, valid, refine=method, **kw)
    want = triangulate_batch(t_hm, torch.from_numpy(proj), 4, valid, keypoints_2d=kp, **kw)
    _same_results(got, want, skip=("keypoints_conf",))
    here = torch.from_numpy(present.copy()).to(dev)
    assert not got["keypoints_2d"][~here].any() and not got["keypoints_conf"][~here].any()
    assert _same_bits(got["keypoints_2d"][here], kp[here]) and _same_bits(got["keypoints_conf"][here], conf[here])
    assert (got["keypoints_conf"][here] > 0.5).all()
    nan_hm = hm.copy()
    nan_hm[~present] = np.nan
    _same_results(got, triangulate_batch(torch.from_numpy(nan_hm).to(dev), torch.from_numpy(proj), 4, valid, refine=method, **kw))


@pytest.mark.parametrize("w", [96, 64], ids=["16x24", "16x16"])
def test_keys_path_equals_the_maps_path(dev, w, monkeypatch):
    """The smallest network case of the GPU tests (HRNet-W32, 3 images, 5 joints), whose plan keeps arg-max keys, at 16 x 24 and
    16 x 16 maps: triangulate_batch(refine="taylor") on the network's tensor -- hard decode from the keys, split by the width --
    equals the same call on its clone, which has no keys."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = dict(cases.model_cases()["w32_small"], w=w)
    m = cases.product_model(c)
    m.load_state_dict({k: torch.from_numpy(a) for k, a in cases.model_state_dict(c).items()}, strict=True)
    m = m.to(dev).eval()
    with torch.no_grad():
        hm = m(torch.from_numpy(cases.model_input(c)).to(dev))
    n, j, hh, wh = hm.shape
    assert (n, j, hh, wh) == (3, 5, 16, w // 4) and _lib.argmax_keys_of(hm) is not None
    proj = torch.from_numpy(synth.ring_cameras(n, 64, w)[None])
    valid = torch.ones(1, j)
    used = []
    real = _lib.argmax_from_keys
    monkeypatch.setattr(_lib, "argmax_from_keys", lambda *a: (used.append(a[-1]), real(*a))[1])
    from_keys = triangulate_batch(hm.reshape(1, n, j, hh, wh), proj, 4, valid, refine="taylor")
    assert used == [wh]  # (decoded from the keys, split by the width)
    from_maps = triangulate_batch(hm.clone().reshape(1, n, j, hh, wh), proj, 4, valid, refine="taylor")
    assert used == [wh]
    _same_results(from_keys, from_maps)
    assert from_keys["keypoints_2d"].dtype == torch.float32
    assert (from_keys["keypoints_2d"] != from_keys["keypoints_2d"].round()).any()  # (sub-pixel points)


# ---- accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 0.02])
def test_accuracy_on_the_small_rig(dev, noise):
    """V = 4, J = 5, N = 2, 24 x 32 maps, stride 4.  The mean distance to the true joints orders taylor < quarter < hard, and the
    device's keypoints_3d are a numpy DLT of the oracle's float32 points to 1e-6 mm (a plumbing check: the DLT's own parity is
    held far tighter elsewhere).  The vote's threshold is set so high that it keeps every view, as the CPU measurement of
    DESIGN.md 6.4 did (all views as inliers); expected there, in mm: hard 41.1 / 38.8, quarter 19.6 / 17.0, taylor 4.5e-5 / 2.9
    at noise 0 / 0.02."""
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    hm, proj, kp3d = _rig(noise)
    b, v, j, hh, wh = hm.shape
    truth = kp3d.transpose(0, 2, 1).astype(np.float64)  # (N, J, 3)
    t_hm = torch.from_numpy(hm).to(dev)
    mean = {}
    for method in ("none",) + ro.METHODS:
        r = triangulate_batch(t_hm, torch.from_numpy(proj), 4, torch.ones(b, j), refine=method, mirror_nonsquare_quirk=False,
                              reprojection_error_epsilon=1e9)
        assert (r["joint_inliers"] == v).all()
        got = r["keypoints_3d"].cpu().numpy()
        pts = ro.hard_decode(hm, 4).astype(np.float32) if method == "none" else ro.refine_batch(hm, 4, method)[0]
        want = np.array([[ro.dlt(pts[bi, :, ji].astype(np.float64), proj[bi]) for ji in range(j)] for bi in range(b)])
        print("noise %g %s: max |device - numpy DLT| = %.3e mm" % (noise, method, np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
        mean[method] = float(np.linalg.norm(got - truth, axis=-1).mean())
    print("noise %g: mean distance to the true joints in mm: %r" % (noise, mean))
    assert mean["taylor"] < mean["quarter"] < mean["none"]


# ---- strategy ------------------------------------------------------------------------------------------------------------------
def _sal_setup(dev):
    from multi_view_active_learning_amd.config import get_default_configs

    c = cases.sal_cases()["hp"]
    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = c["stride"]
    loader, heatmaps = cases.build_sal_loader(c)
    tl = [{k: torch.from_numpy(a) for k, a in dp.items()} for dp in loader]

    def model():
        it = iter(heatmaps)
        return lambda images: torch.from_numpy(next(it)).to(dev)

    return c, cfg, tl, model, heatmaps


@pytest.mark.parametrize("strategy", ["TRIANGULATION", "HP"])
def test_score_batch_under_decode_refine(dev, strategy):
    """score_batch under AL.DECODE_REFINE = "taylor" is the table built by hand from triangulate_batch(refine="taylor")."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy, score_heatmaps_batch
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c, cfg, tl, model, heatmaps = _sal_setup(dev)
    cfg.AL.STRATEGY = strategy
    b, v, j = c["b"], c["v"], c["j"]
    differs = False
    for dp, hm in zip(tl, heatmaps):
        t = torch.from_numpy(hm).to(dev)
        cfg.AL.DECODE_REFINE = "none"
        st = ActiveLearningStrategy(cfg)
        st._pending_checks = []
        plain = st.score_batch(t, dp)
        cfg.AL.DECODE_REFINE = "taylor"
        st = ActiveLearningStrategy(cfg)
        st._pending_checks = []
        tab = st.score_batch(t, dp)
        hm5 = t.reshape(b, v, j, *t.shape[2:])
        jv = dp["joint_valid"].reshape(b, j)
        r = triangulate_batch(hm5, dp["proj_matrices"], c["stride"], jv, refine="taylor")
        pred32 = r["keypoints_3d"].to(torch.float32)
        _, per = _lib.mkpe(pred32.contiguous(), dp["3d_keypoints"].to(dev, torch.float32).contiguous(), jv.to(dev, torch.float32).contiguous(),
                           b, j, dp["3d_keypoints"].shape[1])
        assert _same_bits(tab[:, 0], dp["pose"].to(dev, torch.float64)) and _same_bits(tab[:, 1], dp["frame_id"].to(dev, torch.float64))
        assert _same_bits(tab[:, 3], r["metric"].to(torch.float32).to(torch.float64))
        assert _same_bits(tab[:, 4], r["inlier_count"].to(torch.float64)) and _same_bits(tab[:, 5], per.to(torch.float64))
        assert _same_bits(tab[:, 6:], pred32.to(torch.float64).reshape(b, 3 * j))
        if strategy == "TRIANGULATION":
            assert _same_bits(tab[:, 2], r["metric"])
        else:
            al = score_heatmaps_batch("HP", cfg.AL.HP_CONFIG, hm5, jv)[0]
            assert _same_bits(tab[:, 2], al.to(torch.float32).to(torch.float64))
            assert _same_bits(tab[:, 2], plain[:, 2])  # (the heat-map statistic does not depend on the decode)
        differs = differs or not _same_bits(tab[:, 6:], plain[:, 6:])
    assert differs  # (the refinement matters on this input)


def test_sal_dicts_over_two_strategies(dev):
    """_compute_sal_dicts over two strategies under AL.DECODE_REFINE = "taylor" gives the pred_3d_keypoints of the single-strategy
    pass (decode from the one heat-map launch, split by the width, there; from triangulate_batch's own decode here)."""
    import math

    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    def same(x, y):  # (the per-sample MKPE of this loader is NaN, as it is without a refinement: equal if both are)
        return list(x) == list(y) and all(x[g] == y[g] or (math.isnan(x[g]) and math.isnan(y[g])) for g in x)

    c, cfg, tl, model, _ = _sal_setup(dev)
    cfg.AL.DECODE_REFINE = "taylor"
    cfg.AL.STRATEGY = "TRIANGULATION"
    single = ActiveLearningStrategy(cfg)._compute_sal_dict(tl, model())
    dicts = ActiveLearningStrategy(cfg)._compute_sal_dicts(tl, model(), ("TRIANGULATION", "HP"))
    assert list(dicts) == ["TRIANGULATION", "HP"]
    for s in dicts:
        assert dicts[s]["pred_3d_keypoints"] == single["pred_3d_keypoints"] and len(single["pred_3d_keypoints"]) == c["b"] * c["nbatch"]
        assert same(dicts[s]["sal_metric"], single["sal_metric"]) and same(dicts[s]["mkpe"], single["mkpe"])
    assert same(dicts["TRIANGULATION"]["al_metric"], single["al_metric"])
    cfg.AL.DECODE_REFINE = "none"
    assert ActiveLearningStrategy(cfg)._compute_sal_dict(tl, model())["pred_3d_keypoints"] != single["pred_3d_keypoints"]


def test_evaluate_mkpe_under_decode_refine(dev):
    """evaluate_mkpe on the rig's heat-maps (a stand-in estimator hands them out): lower under EVAL.DECODE_REFINE = "taylor" than
    under "none", and AL.DECODE_REFINE has no say in it.  (On these non-square maps "none" is the reference's split by the
    height, 1335 mm on the MI355X; the refined decodes gave 16.99 mm and 2.87 mm, the figures of the accuracy test.)"""
    from multi_view_active_learning_amd.config import get_default_configs
    from multi_view_active_learning_amd.strategy import ActiveLearningStrategy

    hm, proj, kp3d = _rig(0.02)
    b, v, j, hh, wh = hm.shape
    loader = [{"images": torch.zeros(b, v, 3, 8, 8), "pose": torch.arange(b), "frame_id": torch.arange(b), "proj_matrices": torch.from_numpy(proj),
               "joint_valid": torch.ones(b, j), "3d_keypoints": torch.from_numpy(kp3d)}]
    model = lambda images: torch.from_numpy(hm.reshape(b * v, j, hh, wh)).to(dev)  # noqa: E731
    cfg = get_default_configs()
    cfg.POSE_ESTIMATOR.STRIDE = 4
    value = {}
    for method in ("none", "quarter", "taylor"):
        cfg.EVAL.DECODE_REFINE = method
        value[method] = float(ActiveLearningStrategy(cfg).evaluate_mkpe(loader, model).item())
    print("evaluate_mkpe on the rig, noise 0.02, in mm: %r" % (value,))
    assert value["taylor"] < value["none"] and value["quarter"] < value["none"]
    cfg.EVAL.DECODE_REFINE = "none"
    cfg.AL.DECODE_REFINE = "taylor"
    assert float(ActiveLearningStrategy(cfg).evaluate_mkpe(loader, model).item()) == value["none"]
    cfg.EVAL.DECODE_REFINE = "dark"
    with pytest.raises(ValueError, match="'none', 'quarter', 'taylor'"):
        ActiveLearningStrategy(cfg).evaluate_mkpe(loader, model)

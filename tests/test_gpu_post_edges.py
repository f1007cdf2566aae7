"""GPU tests of the post stage (decode, triangulation, XE, masked MSE, MKPE / PCK, k-center, nearest centre) at the branches
and sizes the golden-vector tests of tests/test_gpu_hotpath.py never reach.  Every input below names the branch of the kernel
it reaches and the arithmetic that shows it.  References are float64 numpy / torch-CPU / ``oracle`` code on the same seeded or
constructed inputs, never a second device path."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import cases
from oracle import coreset as ocoreset
from oracle import geometry, models

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from multi_view_active_learning_amd import _lib

    _lib.lib()  # fail loudly when the extension is missing
    return torch.device("cuda:0")


def _say(capsys, text):
    with capsys.disabled():
        print("\n[post_edges] " + text)


def _misaligned(a, dev):
    """A device copy of ``a`` whose first element sits one float past a 16-byte boundary: a slice buf[1:1+n] of a flat
    buffer (torch allocations are at least 256-byte aligned).  Contiguous, so the wrappers pass its pointer on as it is."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = buf[1 : 1 + flat.numel()]
    t.copy_(flat)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


# =====================================================================================================================
# 1. triangulation
# =====================================================================================================================
@pytest.mark.parametrize("name", list(cases.triangulation_edge_cases()))
def test_triangulation_edges_vs_reference_golden(dev, name):
    """ransac_dlt_kernel at the lane-group sizes no other golden has -- PG = 16 (V = 5, 6: 10 / 15 pairs), PG = 32 with 21 pairs
    (V = 7), PG = 64 (V = 9, 10, 11: 36 / 45 / 55 of 64 lanes vote, one problem per wave) -- and frame_reduce_kernel /
    np_pairwise_sum with 129 (J = 130, one invalid) and 512 valid joints: more than 128 addends take the recursive branch of
    numpy's pairwise sum, 512 is the documented limit.  Expected outputs: the real reference (triangulation_edges.npz); the
    CPU half (tests/test_oracle_golden.py::test_triangulation_edges) shows that no vote of these cases is undecidable."""
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    c = cases.triangulation_edge_cases()[name]
    z = np.load(os.path.join(G, "triangulation_edges.npz"))
    hm, proj, valid = cases.build_triangulation_case(c)
    r = triangulate_batch(torch.from_numpy(hm).to(dev), torch.from_numpy(proj), c["stride"], torch.from_numpy(valid))
    np.testing.assert_array_equal(r["keypoints_2d"].cpu().numpy(), z[name + "/keypoints_2d"])
    np.testing.assert_array_equal(r["inlier_count"].cpu().numpy(), z[name + "/inlier_count"])
    np.testing.assert_allclose(r["keypoints_3d"].cpu().numpy(), z[name + "/keypoints_3d"], rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(r["metric"].cpu().numpy(), z[name + "/metric"], rtol=1e-9)


def _per_joint_problem(v, b=3, j=7):
    """Integer key-points: projections of random 3-D points rounded to the pixel, +-6 px noise (some views fall out of the vote), one view per frame moved far
    away from V = 4 on (an outlier the vote must reject)."""
    from multi_view_active_learning_amd import synth

    rng = np.random.default_rng(700 + v)
    proj = np.stack([synth.ring_cameras(v, 256, 256, seed=900 + 10 * v + i) for i in range(b)])
    x = synth.joints_3d(800 + v, b, j).astype(np.float64)
    kp = np.stack([synth.project(proj[i], x[i].T) for i in range(b)])  # (b, v, j, 2)
    kp = np.round(kp) + rng.integers(-6, 7, size=kp.shape)
    if v >= 4:
        for i in range(b):
            kp[i, rng.integers(0, v)] += rng.integers(40, 90, size=(j, 2))
    return proj, kp.astype(np.int64)


@pytest.mark.parametrize("v", list(range(2, 12)))
def test_ransac_per_joint_outputs_vs_oracle(dev, v, capsys):
    """joint_err / joint_inliers / kp3d of mval_triangulate_ransac joint by joint against oracle.geometry.triangulate_ransac
    for every V the kernel accepts.  B * J = 21 problems leave dead lane groups in the last workgroup: V = 2 (PG = 1, 64 per
    wave) 21 of 64; V = 3 (PG = 4, 16 per wave) 5 of 16; V = 4 (PG = 8) 5 of 8; V = 5, 6 (PG = 16) 1 of 4; V = 7, 8 (PG = 32)
    1 of 2; V >= 9 (PG = 64) one problem per wave with 36 / 45 / 55 voting lanes.  One joint is invalid (zeros).  int64 and
    float32 key-points holding the same integers must give identical bits; valid = None equals an all-ones mask.

    The vote is a strict e < eps on a float64 whose last bits differ between the device (FMA) and numpy: a problem for which
    the oracle's own error lies within 1e-6 px of eps for some (pair, view) is undecidable and left out, at most 1 % of the
    problems (21 problems: none).  Checked on the CPU for the seeds used here: 0 undecidable problems for every V."""
    from multi_view_active_learning_amd import _lib

    b, j, eps = 3, 7, 5.0
    proj, kp = _per_joint_problem(v, b, j)
    valid = np.ones((b, j), np.uint8)
    valid[1, 2] = 0
    pt = torch.from_numpy(proj).to(dev)
    vt = torch.from_numpy(valid).to(dev)
    out_i = _lib.triangulate_ransac(torch.from_numpy(kp).to(dev), pt, vt, b, v, j, eps)
    out_f = _lib.triangulate_ransac(torch.from_numpy(kp.astype(np.float32)).to(dev), pt, vt, b, v, j, eps)
    for a, f in zip(out_i, out_f):
        assert torch.equal(a, f)
    ones = torch.ones((b, j), dtype=torch.uint8, device=dev)
    for a, f in zip(_lib.triangulate_ransac(torch.from_numpy(kp).to(dev), pt, None, b, v, j, eps),
                    _lib.triangulate_ransac(torch.from_numpy(kp).to(dev), pt, ones, b, v, j, eps)):
        assert torch.equal(a, f)
    k3, jerr, jinl, metric, cnt = [t.cpu().numpy() for t in out_i]
    undecidable = 0
    for bi, ji in itertools.product(range(b), range(j)):
        if not valid[bi, ji]:
            assert jinl[bi, ji] == 0 and jerr[bi, ji] == 0 and not k3[bi, ji].any()
            continue
        if geometry.ransac_vote_margin(proj[bi], kp[bi, :, ji], eps) <= 1e-6:
            undecidable += 1
            continue
        x, e, n = geometry.triangulate_ransac(proj[bi], kp[bi, :, ji], 64, eps)
        assert jinl[bi, ji] == n, (bi, ji, jinl[bi, ji], n)
        np.testing.assert_allclose(k3[bi, ji], x, rtol=1e-9, atol=1e-6)
        np.testing.assert_allclose(jerr[bi, ji], e, rtol=1e-9)
    _say(capsys, f"ransac per joint V={v}: undecidable {undecidable} of {b * j - 1}, inliers {sorted(set(jinl.ravel().tolist()))}")
    assert undecidable <= 0.01 * (b * j)
    if undecidable == 0:
        for bi in range(b):
            ok = valid[bi].astype(bool)
            np.testing.assert_allclose(metric[bi], np.mean(jerr[bi][ok]), rtol=1e-12)
            assert cnt[bi] == jinl[bi][ok].min()


def test_frame_without_valid_joint(dev):
    """frame_reduce_kernel with n == 0: metric NaN and inlier_count -1 for that frame, the other frames of the same call
    bit-identical to a call without it; utils.triangulation.triangulation raises the reference's ValueError (np.min([]))."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulation

    b, v, j = 3, 4, 7
    proj, kp = _per_joint_problem(v, b, j)
    valid = np.ones((b, j), np.uint8)
    valid[1] = 0
    pt, kt = torch.from_numpy(proj).to(dev), torch.from_numpy(kp).to(dev)
    k3, jerr, jinl, metric, cnt = _lib.triangulate_ransac(kt, pt, torch.from_numpy(valid).to(dev), b, v, j, 5.0)
    k3a, jerra, jinla, metrica, cnta = _lib.triangulate_ransac(kt, pt, None, b, v, j, 5.0)
    assert np.isnan(metric[1].item()) and cnt[1].item() == -1
    assert not k3[1].any().item() and not jinl[1].any().item()
    for f in (0, 2):
        assert torch.equal(metric[f], metrica[f]) and torch.equal(cnt[f], cnta[f]) and torch.equal(k3[f], k3a[f])
        assert torch.equal(jerr[f], jerra[f]) and cnt[f].item() >= 2
    hm = torch.zeros((v, j, 16, 16), device=dev)
    with pytest.raises(ValueError):
        triangulation(hm, torch.from_numpy(proj[0]), 4, torch.zeros(j))


@pytest.mark.parametrize("v", [1, 12])
def test_ransac_view_count_outside_the_limits(dev, v):
    """V = 1 (the reference asserts >= 2 points) and V = 12 (C(12,2) = 66 > 64 iterations: the reference samples pairs from
    python's RNG) return the documented error and launch nothing: the output buffers keep their sentinel values."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd.utils.triangulation import triangulate_batch

    b, j = 2, 5
    kp = torch.zeros((b, v, j, 2), dtype=torch.int64, device=dev)
    proj = torch.ones((b, v, 3, 4), dtype=torch.float64, device=dev)
    with pytest.raises(_lib.MvalError):
        _lib.triangulate_ransac(kp, proj, None, b, v, j, 5.0)
    k3 = torch.full((b, j, 3), -7.0, dtype=torch.float64, device=dev)
    jerr = torch.full((b, j), -7.0, dtype=torch.float64, device=dev)
    jinl = torch.full((b, j), -7, dtype=torch.int32, device=dev)
    metric = torch.full((b,), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((b,), -7, dtype=torch.int32, device=dev)
    rc = _lib.lib().mval_triangulate_ransac(_lib._p(kp), C.c_int(0), _lib._p(proj), _lib._p(None), _lib._p(k3), _lib._p(jerr),
                                            _lib._p(jinl), _lib._p(metric), _lib._p(cnt), C.c_int(b), C.c_int(v), C.c_int(j),
                                            C.c_double(5.0), _lib._stream())
    assert rc != 0
    torch.cuda.synchronize()
    for t in (k3, jerr, jinl, metric, cnt):
        assert (t == -7).all().item()
    with pytest.raises(AssertionError if v == 1 else NotImplementedError):
        triangulate_batch(torch.zeros((b, v, j, 8, 8), device=dev), proj, 4, torch.ones((b, j)))


@pytest.mark.parametrize("hw", [(17, 23), (96, 72)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("bvj", [(1, 3, 3), (1, 2, 3), (1, 1, 3), (2, 4, 5)], ids=lambda s: "x".join(map(str, s)))
def test_xe_shapes_and_far_points(dev, hw, bvj):
    """xe_kernel: 17 x 23 = 391 pixels is no multiple of 64 (the last trip of the lane loop is partial: 391 = 6 * 64 + 7),
    96 x 72 = 6912 is the C4 / C5 map; B * V * J = 9, 6, 3 maps leave 1, 2, 3 of a workgroup's 4 waves live (40: none dead).
    Joint 0 is put a million mm to the side (outside every view's grid); with the pixel rows of the cameras scaled by 1e4 its
    reprojection lies tens of thousands of pixels away in every view: the target underflows to 0 and the result is
    mean(hm^2) summed over the views.  Reference: oracle.geometry.compute_xe, rtol 1e-9."""
    from multi_view_active_learning_amd import _lib
    from multi_view_active_learning_amd import synth

    hh, wh = hw
    b, v, j = bvj
    rng = np.random.default_rng(hh * 100 + b * 17 + v)
    proj = np.stack([synth.ring_cameras(v, hh, wh, seed=40 + i) for i in range(b)])
    kp3d = rng.standard_normal((b, j, 3)) * 150.0
    kp3d[:, 0] = [1e6, 2e6, 1.5e6]
    hm = rng.standard_normal((b, v, j, hh, wh)).astype(np.float32)
    for sigma in (1.0, 2.5):
        got = _lib.reprojection_xe(torch.from_numpy(kp3d).to(dev), torch.from_numpy(proj).to(dev), torch.from_numpy(hm).to(dev),
                                   b, v, j, hh, wh, sigma).cpu().numpy()
        want = np.array([geometry.compute_xe(kp3d[i], proj[i], hm[i], sigma) for i in range(b)])
        np.testing.assert_allclose(got, want, rtol=1e-9)
    far = proj.copy()
    far[:, :, :2] *= 1e4  # pixel rows scaled: every reprojection of joint 0 moves > 1e4 px away from the grid
    for i in range(b):
        for vi in range(v):
            assert np.abs(geometry.project(far[i, vi], kp3d[i, :1])).min() > 1e4
    only0 = _lib.reprojection_xe(torch.from_numpy(kp3d[:, :1].copy()).to(dev), torch.from_numpy(far).to(dev),
                                 torch.from_numpy(hm[:, :, :1].copy()).to(dev), b, v, 1, hh, wh, 1.0).cpu().numpy()
    np.testing.assert_allclose(only0, [geometry.compute_xe(kp3d[i, :1], far[i], hm[i, :, :1], 1.0) for i in range(b)], rtol=1e-9)
    np.testing.assert_allclose(only0, (hm[:, :, 0].astype(np.float64) ** 2).mean(axis=(2, 3)).sum(axis=1), rtol=1e-12)


def test_xe_point_on_principal_plane(dev):
    """xe_kernel's ``w == 0 -> 1`` guard (utils/triangulation.py:397-399): camera 0 looks down +z from the origin and the point
    has z = 0, so w is exactly 0 and the reprojection is (u, v) undivided = (3, 2) -- inside the 17 x 23 grid; camera 1 sees
    the same point with w = 5."""
    from multi_view_active_learning_amd import _lib

    hh, wh = 17, 23
    proj = np.array([[[[1.0, 0, 8, 0], [0, 1.0, 8, 0], [0, 0, 1, 0]], [[10.0, 0, 2, 5], [0, 10.0, 1, 10], [0, 0, 1, 5]]]])
    kp3d = np.array([[[3.0, 2.0, 0.0]]])
    assert (proj[0, 0, 2, :3] @ kp3d[0, 0] + proj[0, 0, 2, 3]) == 0.0
    np.testing.assert_array_equal(geometry.project(proj[0, 0], kp3d[0]), [[3.0, 2.0]])
    hm = np.random.default_rng(3).standard_normal((1, 2, 1, hh, wh)).astype(np.float32)
    got = _lib.reprojection_xe(torch.from_numpy(kp3d).to(dev), torch.from_numpy(proj).to(dev), torch.from_numpy(hm).to(dev),
                               1, 2, 1, hh, wh, 1.5).cpu().numpy()
    np.testing.assert_allclose(got, [geometry.compute_xe(kp3d[0], proj[0], hm[0], 1.5)], rtol=1e-9)


# =====================================================================================================================
# 2. decode
# =====================================================================================================================
def _soft_argmax_f64(hm):
    """Soft-arg-max evaluated in float64: softmax over the map, expectation of the pixel grid -> (..., 2) = (x, y)."""
    x = np.asarray(hm, dtype=np.float64)
    *lead, h, w = x.shape
    flat = x.reshape(*lead, h * w)
    e = np.exp(flat - flat.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    xs, ys = np.tile(np.arange(w, dtype=np.float64), h), np.repeat(np.arange(h, dtype=np.float64), w)
    return np.stack([(p * xs).sum(-1), (p * ys).sum(-1)], axis=-1)


@pytest.mark.parametrize("hw", [(64, 64), (64, 48), (96, 72), (17, 23)], ids=lambda s: "%dx%d" % s)
def test_soft_argmax_sizes_and_ranges(dev, hw, capsys):
    """soft_argmax_kernel at the product map sizes 64 x 64 (C2), 64 x 48 (C1), 96 x 72 (C4 / C5) and the odd 17 x 23
    (391 = 6 * 64 + 7 pixels: partial last trip), with 1, 5 and 7 maps per call (n_maps % 4 = 1, 1, 3: dead waves in the
    last workgroup).  Inputs: noise * 3 (today's range), noise * 30 (exp spans e^-200..1: only ``- m`` keeps the sum
    useful), a constant map (the exact centre), one spike of height 50 per map (the peak's coordinates), and maps shifted
    by +1e4 -- values on a 1/64 grid so that the shift is exact in float32: ``p - m`` is then the same number, and the result
    must equal the unshifted one BIT FOR BIT (without the max subtraction expf(1e4) overflows).

    Reference: the float64 soft-arg-max.  Tolerance: 4 x the largest error of the float32 oracle
    (oracle.geometry.spatial_soft_argmax2d) against that float64 value over the same inputs of this shape -- two float32
    summation orders of one length differ by a small multiple of each other's error, while an indexing mistake costs
    >= 1 px * weight -- with a floor of 1 ulp of the coordinate range.  The measured ratio is printed."""
    from multi_view_active_learning_amd import _lib

    hh, wh = hw
    scale = 4.0
    rng = np.random.default_rng(hh * 1000 + wh)
    batches = [(rng.standard_normal((n, hh, wh)) * 3).astype(np.float32) for n in (1, 5, 7)]
    batches.append((rng.standard_normal((5, hh, wh)) * 30).astype(np.float32))
    batches.append(np.full((1, hh, wh), 0.75, np.float32))
    spikes = np.zeros((7, hh, wh), np.float32)
    peaks = [(0, 0), (hh - 1, wh - 1), (0, wh - 1), (hh - 1, 0), (hh // 2, wh // 3), (1, 63 % wh), (hh - 2, 64 % wh)]
    for k, (y, x) in enumerate(peaks):
        spikes[k, y, x] = 50.0
    batches.append(spikes)
    grid = (np.round(rng.standard_normal((5, hh, wh)) * 3 * 64) / 64).astype(np.float32)
    shifted = grid + np.float32(1e4)
    assert np.array_equal(shifted.astype(np.float64) - 1e4, grid.astype(np.float64))  # the shift is exact
    batches += [grid, shifted]

    dev_err = ora_err = 0.0
    outs = []
    for m in batches:
        got = _lib.soft_argmax(torch.from_numpy(m).to(dev), len(m), hh, wh, scale).cpu().numpy().astype(np.float64)
        ref = _soft_argmax_f64(m) * scale
        ora = geometry.spatial_soft_argmax2d(m).astype(np.float64) * scale
        assert np.isfinite(got).all()
        dev_err, ora_err = max(dev_err, np.abs(got - ref).max()), max(ora_err, np.abs(ora - ref).max())
        outs.append((got, ref))
    ulp = float(np.spacing(np.float32((max(hh, wh) - 1) * scale)))
    tol = max(4.0 * ora_err, ulp)
    _say(capsys, f"soft-arg-max {hh}x{wh}: device err {dev_err:.3e}, float32 oracle err {ora_err:.3e}, ratio "
                 f"{dev_err / ora_err if ora_err else float('inf'):.2f}, 1 ulp of range {ulp:.3e}, tolerance {tol:.3e}")
    for got, ref in outs:
        np.testing.assert_allclose(got, ref, rtol=0, atol=tol)
    np.testing.assert_allclose(outs[4][1], [[(wh - 1) / 2 * scale, (hh - 1) / 2 * scale]], rtol=1e-12)  # constant: the centre
    np.testing.assert_allclose(outs[5][1], [[x * scale, y * scale] for y, x in peaks], rtol=0, atol=1e-12)  # spike: its place
    np.testing.assert_array_equal(outs[7][0], outs[6][0])  # shifted == unshifted, bit for bit


def _argmax_want(flat_maps, valid, b, v, j, stride, split):
    idx = torch.argmax(torch.from_numpy(flat_maps), dim=-1).numpy().reshape(b, v, j)
    want = np.stack([(idx % split) * stride, (idx // split) * stride], axis=-1).astype(np.int64)
    if valid is not None:
        want[np.broadcast_to(valid.reshape(b, 1, j) == 0, (b, v, j))] = 0
    return want


@pytest.mark.parametrize("hw", [(64, 48), (32, 24), (17, 23)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset4B"])
def test_argmax_alignment_signed_zero_nan_inf(dev, hw, aligned, capsys):
    """argmax_decode_kernel.  _lib.argmax_decode passes the pointer of any CONTIGUOUS tensor on unchanged, so a slice
    buf[1:1+n] of a flat buffer reaches the kernel 4 bytes past a 16-byte boundary: with npix % 4 == 0 (64 x 48 = 3072,
    32 x 24 = 768) every map base is then misaligned ((4 + 4 * npix * k) % 16 = 4) and the scalar path runs although
    ``(npix & 3) == 0``; 17 x 23 = 391 takes it for the size.  (b, v, j) = (1, 1, 5), (1, 2, 3), (1, 1, 7), (2, 3, 19): 5, 6,
    7 maps leave 1, 2, 3 live waves in the last workgroup; with and without a valid mask; both split widths.
    Constructed maps: -0.0 before +0.0 and the reverse (they compare equal: first index wins), two NaNs (the first wins),
    +inf twice (the first), all in the last float4 of a lane's trip or across lanes.  Reference: torch.argmax on the CPU and
    oracle.geometry.argmax_decode (which splits with the height), exact."""
    from multi_view_active_learning_amd import _lib

    hh, wh = hw
    npix = hh * wh
    rng = np.random.default_rng(npix + int(aligned))
    for b, v, j in ((1, 1, 5), (1, 2, 3), (1, 1, 7), (2, 3, 19)):
        n = b * v * j
        hm = rng.standard_normal((n, npix)).astype(np.float32)
        hm[0] = -1.0
        hm[0, 5], hm[0, 300] = -0.0, 0.0           # -0.0 first
        hm[1] = -1.0
        hm[1, 6], hm[1, 258] = 0.0, -0.0           # +0.0 first, the other in the same lane's next trip (258 = 6 + 252)
        hm[2, 77], hm[2, 311] = np.nan, np.nan     # two NaNs
        hm[2, 3] = np.inf                          # ... which beat +inf
        if n > 3:
            hm[3, 130], hm[3, 129 + 64] = np.inf, np.inf
            hm[4, npix - 1] = 99.0                 # the very last pixel
        assert int(torch.argmax(torch.from_numpy(hm[0]))) == 5 and int(torch.argmax(torch.from_numpy(hm[1]))) == 6
        assert int(torch.argmax(torch.from_numpy(hm[2]))) == 77
        t = torch.from_numpy(hm).to(dev) if aligned else _misaligned(hm, dev)
        assert (t.data_ptr() % 16 == 0) == aligned
        valid = np.ones((b, j), np.uint8)
        valid[0, j - 1] = 0
        for vmask in (None, valid):
            vt = None if vmask is None else torch.from_numpy(vmask).to(dev)
            for split in (hh, wh):
                got = _lib.argmax_decode(t, vt, b, v, j, hh, wh, 4, split).cpu().numpy()
                np.testing.assert_array_equal(got, _argmax_want(hm, vmask, b, v, j, 4, split))
                if split == hh:
                    for bi in range(b):
                        want = geometry.argmax_decode(hm.reshape(b, v, j, hh, wh)[bi], 4, np.ones(j) if vmask is None else vmask[bi])
                        np.testing.assert_array_equal(got[bi], want)


# =====================================================================================================================
# 3. loss and metrics
# =====================================================================================================================
def _mse_check(dev, lead, hw, valid_kind, offset, seed, grad=1.0):
    from multi_view_active_learning_amd import _lib

    rng = np.random.default_rng(seed)
    h = rng.standard_normal((lead, hw)).astype(np.float32)
    g = rng.standard_normal((lead, hw)).astype(np.float32)
    valid = {"none": None, "some": (rng.uniform(size=lead) > 0.3).astype(np.uint8), "zero": np.zeros(lead, np.uint8)}[valid_kind]
    denom = float(max(1, lead // 19) * hw)
    if offset:
        ht, gt = _misaligned(h, dev), _misaligned(g, dev)
    else:
        ht, gt = torch.from_numpy(h).to(dev).reshape(-1), torch.from_numpy(g).to(dev).reshape(-1)
    vt = None if valid is None else torch.from_numpy(valid).to(dev)
    loss = _lib.masked_mse_fwd(ht, gt, vt, lead, hw, denom).item()
    go = torch.tensor(grad, dtype=torch.float32, device=dev)
    gh = _lib.masked_mse_bwd(ht, gt, vt, go, lead, hw, denom).cpu().numpy().reshape(lead, hw)
    d = h.astype(np.float64) - g.astype(np.float64)
    m = np.ones((lead, 1)) if valid is None else valid.astype(np.float64)[:, None]
    want = float((d * d * m).sum() / denom)
    want_g = 2.0 * d * m * (float(np.float32(grad)) / denom)
    assert abs(loss - want) <= 2e-6 * abs(want), (loss, want)
    np.testing.assert_allclose(gh, want_g, rtol=1e-6, atol=1e-12)  # element by element: a skipped tail shows as zeros / garbage
    if valid_kind == "zero":
        assert loss == 0.0 and not gh.any()
    return loss


@pytest.mark.parametrize("valid_kind", ["some", "none", "zero"])
def test_masked_mse_scalar_paths(dev, valid_kind):
    """mse_partial_kernel's scalar path and mse_bwd_kernel, float64 numpy reference (the kernel accumulates in float64):
    hw = 17 * 23 = 391 (hw % 4 = 3: scalar for the size), lead = 6 * 19; hw = 64 * 48 = 3072 (hw % 4 == 0) seen from a
    one-float offset (both pointers 4 bytes past a 16-byte boundary: scalar for the alignment), and the same aligned (vector
    path) for comparison.  valid = NULL, a mixed mask, and every map invalid (loss exactly 0, gradient exactly zero)."""
    _mse_check(dev, 6 * 19, 17 * 23, valid_kind, False, 1)
    a = _mse_check(dev, 12, 64 * 48, valid_kind, True, 2, grad=0.37)
    b = _mse_check(dev, 12, 64 * 48, valid_kind, False, 2, grad=0.37)
    assert abs(a - b) <= 2e-6 * abs(b)


@pytest.mark.parametrize("lead,hw", [(400, 3072), (3200, 391)], ids=["vec_1228800", "scalar_1251200"])
@pytest.mark.parametrize("valid_kind", ["some", "none"])
def test_masked_mse_second_grid_stride_trip(dev, lead, hw, valid_kind):
    """The grid-stride loops running again.  400 * 3072 = 1 228 800 elements, hw % 4 == 0: the forward launches 1024 x 256
    threads over 307 200 float4s > 262 144 (second trip; in elements 1 228 800 > 1 048 576); the backward launches
    4096 x 256 = 1 048 576 threads < 1 228 800 (second trip).  3200 * 391 = 1 251 200 elements, hw % 4 = 3: the forward's
    scalar loop makes five trips (1 251 200 / 262 144), the backward two."""
    assert lead * hw > 1024 * 256 * 4 and lead * hw > 4096 * 256
    _mse_check(dev, lead, hw, valid_kind, False, lead)


def test_masked_mse_no_maps(dev):
    """lead == 0: the forward still launches one workgroup and writes 0 / denom = 0; the backward launches nothing."""
    from multi_view_active_learning_amd import _lib

    h = torch.empty((0,), dtype=torch.float32, device=dev)
    out = _lib.masked_mse_fwd(h, h, None, 0, 391, 391.0)
    assert out.item() == 0.0
    gh = _lib.masked_mse_bwd(h, h, None, torch.ones((), dtype=torch.float32, device=dev), 0, 391, 391.0)
    assert gh.numel() == 0


@pytest.mark.parametrize("s", [257, 1000, 5000])
@pytest.mark.parametrize("j", [19, 2])
def test_pck3d_many_samples(dev, s, j):
    """pck3d_kernel's sample loop ``for (s = threadIdx.x; s < S; s += 256)``: S = 257 gives thread 0 a second trip (and only
    it), S = 1000 three or four trips (1000 = 3 * 256 + 232), S = 5000 twenty (5000 = 19 * 256 + 136); J = 2 is the minimum the
    entry point accepts (PCKh needs joints 0 and 1).  Noisy samples and the ``ties`` construction of cases.pck_arrays
    (integer offsets: distances land ON the thresholds 1, 2, 3).  Exact equality of the fractions with the oracle."""
    from multi_view_active_learning_amd import _lib

    for noise, thr_sets in ((2.0, ((1, 2, 3, 4, 5),)), (40.0, ((10, 25, 50, 100, 150),)), (0.0, ((1, 2, 3, 4, 5),))):
        pred, gt, valid = cases.pck_arrays(dict(seed=100 + s + j, s=s, j=j, noise=noise, p_valid=0.8))
        pt, gt_t, vt = (torch.from_numpy(a).to(dev) for a in (pred, gt, valid))
        for thr in thr_sets:
            hits, counts = _lib.pck3d(pt, gt_t, vt, thr, 0)
            hits, counts = hits.cpu().tolist(), counts.cpu().tolist()
            assert counts == valid.sum(0).astype(np.int64).tolist()
            for row, t in zip(hits, thr):
                assert [k / c for k, c in zip(row, counts)] == models.compute_3d_pck(pred, gt, valid, t, j)
        thr_h = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)
        hits, counts = _lib.pck3d(pt, gt_t, None, thr_h, 1)
        assert counts.cpu().tolist() == [s] * j
        for row, t in zip(hits.cpu().tolist(), thr_h):
            assert [k / s for k in row] == models.compute_3d_pckh(pred, gt, t, j)


@pytest.mark.parametrize("j", [1, 64, 65, 130, 1024])
@pytest.mark.parametrize("s", [1, 63, 65, 3000])
def test_mkpe_joint_and_sample_counts(dev, j, s):
    """mkpe_total_kernel with J beyond one wave -- its block is ceil(J / 64) * 64 threads: 64 (J = 1, 64), 128 (J = 65: 63 idle
    lanes in the second wave), 192 (J = 130), 1024 (J = 1024, the limit) -- and S = 3000 sequential float32 additions per
    joint; mkpe_per_sample_kernel with S = 1, 63, 65, 3000 (blocks of 64 samples: 1 / 63 / 1 / 56 live lanes in the last).
    Reference oracle.models.compute_mkpe, 2e-6 relative; a joint that is never valid gives NaN (0 / 0) on both sides."""
    from multi_view_active_learning_amd import _lib

    rng = np.random.default_rng(j * 10000 + s)
    pred = (rng.standard_normal((s, j, 3)) * 100).astype(np.float32)
    gt = (rng.standard_normal((s, 4, j)) * 100).astype(np.float32)
    valid = (rng.uniform(size=(s, j)) > 0.2).astype(np.float32)
    valid[0] = 1
    pl, gl = [torch.from_numpy(p) for p in pred], [torch.from_numpy(x) for x in gt]
    for never in (False, True):
        if never:
            valid[:, j // 2] = 0
        vl = [torch.from_numpy(x) for x in valid]
        out, per = _lib.mkpe(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(valid).to(dev), s, j, 4)
        got, want = out.item(), models.compute_mkpe(pl, gl, vl).item()
        if never:
            assert np.isnan(got) and np.isnan(want)
        else:
            assert np.isfinite(want) and abs(got - want) <= 2e-6 * abs(want), (got, want)
        per = per.cpu().numpy()
        rows = range(s) if s <= 65 else sorted(set(range(0, s, 13)) | set(range(s - 130, s)))
        for i in rows:
            w = models.compute_mkpe([pl[i]], [gl[i]], [vl[i]]).item()
            assert (np.isnan(per[i]) and np.isnan(w)) or abs(per[i] - w) <= 2e-6 * abs(w), (i, per[i], w)
        assert np.isnan(per).sum() == (valid.min(axis=1) == 0).sum()


# =====================================================================================================================
# 4. core-set
# =====================================================================================================================
def _kcenter_oracle(feat, labeled, n_select):
    """oracle.coreset.kcenter_greedy's picks, the min_distances they leave (replayed with the oracle's distance), and the
    smallest relative gap between the best and the second-best candidate over the steps (inf with fewer than two rows)."""
    picks, _ = ocoreset.kcenter_greedy(feat, labeled, n_select)
    md = np.min(ocoreset.euclidean_expanded(feat, feat[list(labeled)]), axis=1) if len(labeled) else np.full(len(feat), np.inf)
    gap = np.inf
    for p in picks:
        if len(md) > 1 and np.isfinite(md).all():
            top = np.partition(md, -2)[-2:]
            gap = min(gap, (top[1] - top[0]) / top[1])
        md = np.minimum(md, ocoreset.euclidean_expanded(feat, feat[[p]])[:, 0])
    return picks, md, gap


def _kcenter_device(dev, feat, labeled, n_select, min_dist=None):
    from multi_view_active_learning_amd import _lib

    lab = torch.as_tensor(list(labeled), dtype=torch.int64, device=dev) if len(labeled) else None
    picks, md = _lib.kcenter_select(feat, lab, n_select, min_dist)
    return picks.cpu().tolist(), md


# distances: 1e-9 relative; the self-distance of a picked row is the square root of pure rounding noise (0 on the device,
# up to ~1e-3 from BLAS in the oracle), hence the absolute term -- as in test_coreset_vs_reference_golden
MD_TOL = dict(rtol=1e-9, atol=1e-3)
MIN_GAP = 1e-9  # a seed is admissible only if the oracle's own best and second-best differ by more than this at every step


def test_kcenter_grid_stride_pool(dev, capsys):
    """kc_init_kernel / kc_step_kernel past their grids: n_obs = 300 000 > 1024 * 256 = 262 144, so workgroups 0..147 make a
    second trip through both loops (37 856 rows), including the __syncthreads() inside kc_init_kernel's loop.  D = 57;
    300 000 * 57 * 8 B = 136.8 MB of features (as much again transposed).  3 labelled rows (n_labeled % 4 = 3), 6 picks,
    then a continuation call (have_min_dist = 1, no new centres) of 2 more.  The random seed is admissible: the oracle's
    smallest relative gap (printed) exceeds 1e-9 -- asserted below on the oracle's own numbers."""
    import time

    n, d = 300_000, 57
    assert n > 1024 * 256
    feat = np.random.default_rng(2024).standard_normal((n, d)) * 300.0
    labeled = [n - 3, n - 2, n - 1]
    t0 = time.time()
    picks, md, gap = _kcenter_oracle(feat, labeled, 8)
    t_oracle = time.time() - t0
    _say(capsys, f"k-center 300000 x 57: oracle min relative gap {gap:.3e}, oracle time {t_oracle:.1f} s, picks {picks}")
    assert gap > MIN_GAP
    ft = torch.from_numpy(feat).to(dev)
    got6, mdt = _kcenter_device(dev, ft, labeled, 6)
    assert got6 == picks[:6]
    got2, mdt = _kcenter_device(dev, ft, [], 2, mdt)
    assert got2 == picks[6:]
    np.testing.assert_allclose(mdt.cpu().numpy(), md, **MD_TOL)


def test_kcenter_exact_ties_across_workgroups_and_trips(dev):
    """Exact ties.  Integer-valued features (|x| <= 2000, D = 8: every product, sum and square root argument is an exact
    float64 integer in any order) with the farthest row A three times -- index 10 (workgroup 0), 300 (workgroup 1) and
    262 144 + 5 (workgroup 0 again, second trip of the grid-stride loop) -- and the second-farthest row B at 262 144 + 6 and
    299 999: the lowest index must win each time, so the picks are 10, then 262 150 (a second-trip row beating a later
    one).  Distances are exact: compared for equality.  The small pool (1000 rows, 4 workgroups) does the same without
    the second trip."""
    for n, dup in ((300_000, (10, 300, 262_144 + 5)), (1000, (10, 300, 777))):
        rng = np.random.default_rng(n)
        feat = rng.integers(-50, 51, size=(n, 8)).astype(np.float64)
        feat[list(dup)] = 2000.0
        b_rows = (262_144 + 6, n - 1) if n > 262_144 else (600, n - 1)
        feat[list(b_rows)] = -1000.0
        labeled = [0, 1]
        picks, md, _ = _kcenter_oracle(feat, labeled, 4)
        assert picks[:2] == [dup[0], b_rows[0]]
        got, mdt = _kcenter_device(dev, torch.from_numpy(feat).to(dev), labeled, 4)
        assert got == picks, (n, got, picks)
        np.testing.assert_array_equal(mdt.cpu().numpy(), md)


@pytest.mark.parametrize("n,d,labeled", [
    (1, 57, []), (2, 57, [1]), (63, 57, [62]), (257, 57, [256]),                          # n_obs < 64, = 1, 257 = 256 + 1
    (1000, 1, [999]), (1000, 512, [999]),                                                  # D = 1, D = 512 (the limit)
    (1000, 57, [998, 999]), (1000, 57, [997, 998, 999]),                                   # n_labeled % 4 = 2, 3
    (1000, 57, list(range(994, 1000))), (1000, 57, list(range(993, 1000))),                # 6, 7: a full group of four + 2, 3
], ids=lambda p: str(len(p)) if isinstance(p, list) else str(p))
def test_kcenter_small_pools_dims_and_label_counts(dev, n, d, labeled, capsys):
    """kc_init_kernel stages the labelled centres four at a time: n_labeled = 2, 3, 6, 7 end on a partial group (nc = 2, 3);
    n_obs = 1, 2, 63 leave most of the one workgroup dead, 257 puts a single row in the second; D = 1 and D = 512 are the
    ends of the accepted range.  n_obs = 1 has no labelled row: every distance starts at +inf and the pick is row 0.  No
    more rows are selected than are unlabelled (after that the oracle's arg-max is over rounding noise).  Seeds admissible:
    the oracle's smallest relative gap is printed and asserted > 1e-9."""
    feat = np.random.default_rng(n * 1000 + d + len(labeled)).standard_normal((n, d)) * 300.0
    n_select = min(5, n - len(labeled))
    picks, md, gap = _kcenter_oracle(feat, labeled, n_select)
    _say(capsys, f"k-center n={n} D={d} labelled={len(labeled)}: oracle min relative gap {gap:.3e}")
    assert gap > MIN_GAP
    got, mdt = _kcenter_device(dev, torch.from_numpy(feat).to(dev), labeled, n_select)
    assert got == picks
    np.testing.assert_allclose(mdt.cpu().numpy(), md, **MD_TOL)


def test_kcenter_nan_row(dev):
    """A NaN row is the maximum (np.argmax) and is picked first; its distances are NaN and spread through ``minimum``, so
    every later pick is row 0 -- exactly what numpy does in the oracle."""
    n, d = 1000, 57
    feat = np.random.default_rng(5).standard_normal((n, d)) * 300.0
    feat[417, 3] = np.nan
    labeled = [998, 999]
    picks, md, _ = _kcenter_oracle(feat, labeled, 3)
    assert picks == [417, 0, 0] and np.isnan(md).all()
    got, mdt = _kcenter_device(dev, torch.from_numpy(feat).to(dev), labeled, 3)
    assert got == picks
    assert torch.isnan(mdt).all().item()
    got1, mdt1 = _kcenter_device(dev, torch.from_numpy(feat).to(dev), labeled, 1)
    assert got1 == [417]
    m = mdt1.cpu().numpy()
    assert np.isnan(m).all()


def test_kcenter_no_labelled_rows_and_no_picks(dev):
    """include/mval_hip.h: n_labeled == 0 with have_min_dist == 0 starts every distance at +inf, so the first pick is row 0
    (np.argmax(None) == 0 in the reference) -- unreachable from CoreSet, which raises IndexError on an empty labelled set.
    n_select == 0 leaves ``picks`` untouched and ``min_dist`` initialised (minimum over the labelled rows; +inf without any)."""
    from multi_view_active_learning_amd import _lib

    n, d = 257, 57
    feat = np.random.default_rng(77).standard_normal((n, d)) * 300.0
    ft = torch.from_numpy(feat).to(dev)
    picks, md, gap = _kcenter_oracle(feat, [], 4)
    assert picks[0] == 0 and gap > MIN_GAP
    got, mdt = _kcenter_device(dev, ft, [], 4)
    assert got == picks
    np.testing.assert_allclose(mdt.cpu().numpy(), md, **MD_TOL)

    def raw(labeled, n_select):
        sentinel = torch.full((4,), -7, dtype=torch.int64, device=dev)
        md = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        norms = torch.empty((n,), dtype=torch.float64, device=dev)
        ws = torch.empty((_lib.kcenter_workspace_bytes(n, d) // 8 + 1,), dtype=torch.float64, device=dev)
        lab = torch.as_tensor(labeled, dtype=torch.int64, device=dev) if labeled else None
        rc = _lib.lib().mval_kcenter_select(_lib._p(ft), C.c_longlong(n), C.c_int(d), _lib._p(lab), C.c_longlong(len(labeled)),
                                            C.c_int(n_select), C.c_int(0), _lib._p(norms), _lib._p(md), _lib._p(sentinel),
                                            _lib._p(ws), _lib._stream())
        assert rc == 0
        return sentinel.cpu().tolist(), md.cpu().numpy()

    s, m = raw([], 0)
    assert s == [-7] * 4 and np.isposinf(m).all()
    s, m = raw([3, 200], 0)
    assert s == [-7] * 4
    np.testing.assert_allclose(m, np.min(ocoreset.euclidean_expanded(feat, feat[[3, 200]]), axis=1), **MD_TOL)
    s, m = raw([], 1)
    assert s == [0, -7, -7, -7]


@pytest.mark.parametrize("n", [1, 255, 257])
def test_nearest_center_exact_ties(dev, n):
    """nearest_center_kernel: one thread per row, n = 1, 255, 257 (n % 256 != 0: 255 / 1 live threads in the last
    workgroup).  Integer-valued rows and centres make every distance an exact float64 integer, so rows exactly between two
    (or three) centres are true ties and the lower centre index must win; K = 1 and D = 1 are the smallest sizes.
    Reference: np.argmin of the float64 squared distances."""
    from multi_view_active_learning_amd import _lib

    rng = np.random.default_rng(n)
    for d, centers in ((4, np.array([[0, 0, 0, 0], [2, 0, 0, 0], [0, 2, 0, 0], [2, 0, 0, 0]], np.float64)),
                       (1, np.array([[-1.0], [1.0], [3.0]])), (3, np.array([[5.0, -2.0, 1.0]]))):
        x = rng.integers(-3, 4, size=(n, d)).astype(np.float64)
        x[0] = ([1, 0, 0, 0], [0], [0, 0, 0])[(4, 1, 3).index(d)]   # between centres 0 and 1 (D = 4, 1)
        if n > 2:
            x[1] = ([1, 1, 0, 0], [2], [0, 0, 0])[(4, 1, 3).index(d)]  # 0 = 1 = 2 = 3 tie ; between 1 and 2
            x[n - 1] = ([2, 2, 0, 0], [2], [1, 1, 1])[(4, 1, 3).index(d)]  # 1 = 2 = 3 tie
        d2 = ((x[:, None, :] - centers[None]) ** 2).sum(-1)
        want = np.argmin(d2, axis=1)
        ties = int((np.ptp(np.sort(d2, axis=1)[:, :2], axis=1) == 0).sum()) if len(centers) > 1 else 0
        assert len(centers) == 1 or ties >= 1
        got = _lib.nearest_center(torch.from_numpy(x).to(dev), torch.from_numpy(centers).to(dev)).cpu().numpy()
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("rows", [3, 4])
def test_coreset_features_rows_and_roots(dev, rows):
    """coreset_features_kernel with poses of 3 and of 4 columns (x, y, z[, confidence]), the root joint first and last, J = 19
    and the minimum J = 1, and n = 0 (nothing launched, an empty table).  Exact equality with the reference's expression
    (utils/coreset.py:40-46): transpose, rows 0..2 minus the root column, flattened coordinate-major."""
    from multi_view_active_learning_amd import _lib

    rng = np.random.default_rng(rows)
    for n, j in ((5, 19), (300, 19), (2, 1), (0, 19)):
        pose = rng.standard_normal((n, j, rows)) * 300.0
        for root in sorted({0, j - 1}):
            got = _lib.coreset_features(torch.from_numpy(pose).to(dev), root, n, j, rows).cpu().numpy()
            want = np.zeros((n, 3 * j))
            for i in range(n):
                p = pose[i].transpose([1, 0])
                want[i] = (p[0:3, :] - p[0:3, root : root + 1]).flatten()
            assert got.shape == (n, 3 * j)
            np.testing.assert_array_equal(got, want)

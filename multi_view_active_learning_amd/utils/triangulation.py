"""Keypoint decode + RANSAC-DLT triangulation -- drop-in for the hot-path part of the
reference's utils/triangulation.py (:168-484).

``triangulation(...)`` keeps the reference signature and result dict for one frame
(utils/triangulation.py:168-233) and is a thin view over ``triangulate_batch`` which
processes a whole batch of frames with three HIP launches (arg-max decode, pairwise
RANSAC + DLT, per-frame reduction) instead of V*J device->host syncs and
J*(C(V,2)+1) LAPACK calls per frame.  float64 geometry, SVD-free (csrc/triangulate.hip).

Rigs with more view pairs than ``n_iters`` (from 12 views on at the default 64): the reference
shuffles the pair list of every valid joint with python's ``random`` and keeps the first
``n_iters`` (utils/triangulation.py:279-282).  ``draw_view_pairs`` makes those draws on the host,
in the reference's order, and the device triangulates the drawn pairs (up to 32 views).

Frames with missing views: ``view_valid`` (B, V) makes every frame's result what these functions give on that frame's
present views alone -- what the per-sample reference computes when it is handed the views that exist -- with all frames
of a batch in one triangulation launch.

Joints missing from single views: ``view_joint_valid`` (B, V, J) makes the present views a property of the problem (frame,
joint): every joint is triangulated from the views that have it, a joint with fewer than two of them is left out of the
frame's metric and inlier count, and ``peak_mask`` builds such a mask on the device from the heat-maps' own peak heights
(DESIGN.md 6.3).

Sub-pixel decode: ``refine`` = "quarter" | "taylor" refines the hard arg-max inside its 3x3 neighbourhood (``mval_refine_keypoints``,
DESIGN.md 6.4) and hands float32 key-points to the unchanged triangulation entries; "none", the default, is the reference's decode.

3-D refinement: ``refine_3d`` = "lm" moves every triangulated joint from the DLT point of its inlier views to the minimiser of the
reprojection error over the views within eps of that point (``mval_refine_points_3d``, one launch after the triangulation,
DESIGN.md 6.5).  It is a defined stand-in for the reference's ``direct_optimization``, which itself keeps raising.

Lens distortion: ``undistort`` = "brown" inverts the reference's own forward model (k1, k2, p1, p2, k3) for every decoded key-point
(``mval_undistort_keypoints``, one launch between the decode and the triangulation): the network's peaks sit at
distorted pixels, the triangulation takes them for pinhole observations.  ``undistort_keypoints`` is the direct form.

Confidence weights: ``weights`` = "conf" | a (B, V, J) tensor multiplies the DLT rows of every (view, joint) entry by its weight, in
RANSAC's pair solves and in the final solve, and breaks ties between equally large inlier sets by their summed weight
(``mval_triangulate_ransac_weighted``, the same one launch); ``return_inlier_mask`` hands RANSAC's winning set out.
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

from .. import _lib
from ..config import check_decode_refine, check_refine_3d, check_triangulation_weights, check_undistort


def _device_of(heatmaps):
    if not torch.is_tensor(heatmaps) or not heatmaps.is_cuda:
        raise _lib.MvalError("heatmaps must be a HIP tensor: the hot path has no CPU implementation")
    return heatmaps.device


def _as_valid_u8(valid, shape, device):
    if valid is None:
        return None
    v = torch.as_tensor(valid)
    v = (v != 0).to(torch.uint8).reshape(shape)
    return v.to(device).contiguous()


PAIR_PAD = 255  # a view index no rig has (at most 32 views): an entry naming it takes no part in the vote


def _draw_view_pairs_vj(valid, V, n_iters, rng, vj):
    """``vj`` (B, V, J) bool (a ``view_valid`` broadcast over the joints): the masked tables of ``draw_view_pairs``, one present
    set per problem."""
    b, j = valid.shape
    n_present = vj.sum(axis=1)  # (B, J)
    n_pairs = n_present * (n_present - 1) // 2
    out = np.full((b, j, max(1, int(np.minimum(n_pairs, n_iters).max(initial=0))), 2), PAIR_PAD, dtype=np.uint8)
    lex_of = {}  # present set -> its lexicographic pairs (the joints of a frame mostly share a few sets)
    for bi in range(b):
        for ji in range(j):
            n = int(n_pairs[bi, ji])
            if n == 0:  # fewer than two present views: nothing to triangulate, nothing drawn
                continue
            key = vj[bi, :, ji].tobytes()
            if key not in lex_of:
                lex_of[key] = np.array(list(itertools.combinations(np.flatnonzero(vj[bi, :, ji]).tolist(), 2)), dtype=np.uint8).reshape(-1, 2)
            lex = lex_of[key]
            if n <= n_iters:
                out[bi, ji, :n] = lex
                continue
            out[bi, ji] = 0  # (a problem that draws fills all P = n_iters entries; the row of an invalid joint stays zero)
            if valid[bi, ji]:
                order = list(range(n))
                rng.shuffle(order)
                out[bi, ji] = lex[order[:n_iters]]
    return out


def draw_view_pairs(valid, V, n_iters, rng, view_valid=None, view_joint_valid=None):
    """The view pairs the reference samples for every joint of a batch (utils/triangulation.py:279-282):
    valid (B, J) -> uint8 ndarray (B, J, P, 2), P = min(n_iters, C(V,2)).

    For b ascending, j ascending, valid joints only (the reference skips an invalid joint before the draw,
    :210-211), ``rng.shuffle`` permutes a list as long as ``itertools.combinations(range(V), 2)`` and the first
    ``n_iters`` pairs are kept: ``rng`` (the ``random`` module or a ``random.Random``) is left in the state the
    reference leaves it in.  The rows of an invalid joint stay zero.  With C(V,2) <= n_iters the reference draws
    nothing: neither does this, and every row is the lexicographic list.

    ``view_valid`` (B, V), nonzero = present: what the reference draws when it is handed each frame's present views
    alone, in ORIGINAL view indices.  Frame b with n_b present views: C(n_b, 2) <= n_iters -> the lexicographic pairs of
    its present views, nothing drawn; otherwise per valid joint a shuffle of a list of length C(n_b, 2), first
    ``n_iters`` kept.  Frames in batch order, valid joints ascending: ``rng`` ends in the reference's state.
    P = max over frames of min(C(n_b, 2), n_iters), at least 1; shorter rows, and those of a frame with n_b < 2 (which
    draws nothing), are padded with ``PAIR_PAD`` = 255.  The rows of an invalid joint stay zero in a frame that draws.

    ``view_joint_valid`` (B, V, J), nonzero = joint j is usable in view v (ANDed with ``view_valid`` where both are given):
    one table per problem, as the reference would draw for that joint's slice of the views.  Problem (b, j) with n_bj
    present views: C(n_bj, 2) <= n_iters -> the lexicographic pairs of its present views, nothing drawn; otherwise, for a
    valid joint, one shuffle of a list of length C(n_bj, 2), first ``n_iters`` kept.  Frames in batch order, valid joints
    ascending, joints with n_bj < 2 drawing nothing: ``rng`` ends in the state the reference's per-joint calls, made in
    that order, leave it in.  P = max over problems of min(C(n_bj, 2), n_iters), at least 1; padding and invalid joints as
    above, so a mask that is the same for every joint of a frame gives the ``view_valid`` tables."""
    valid = torch.as_tensor(valid).cpu().numpy() != 0
    b, j = valid.shape
    if view_valid is not None or view_joint_valid is not None:
        vj = np.ones((b, V, j), dtype=bool)
        if view_joint_valid is not None:
            vj = torch.as_tensor(view_joint_valid).cpu().numpy().reshape(b, V, j) != 0
        if view_valid is not None:
            vj = vj & (torch.as_tensor(view_valid).cpu().numpy().reshape(b, V, 1) != 0)
        return _draw_view_pairs_vj(valid, V, n_iters, rng, vj)
    # (unmasked: what the masked body gives with an all-ones mask, without its B x J python loop on the sampled hot path)
    lex = np.array(list(itertools.combinations(range(V), 2)), dtype=np.uint8).reshape(-1, 2)
    n = len(lex)
    if n <= n_iters:
        return np.broadcast_to(lex, (b, j, n, 2)).copy()
    out = np.zeros((b, j, n_iters, 2), dtype=np.uint8)
    for bi, ji in zip(*np.nonzero(valid)):  # row-major: b ascending, j ascending
        order = list(range(n))  # shuffle's draws depend on the length alone
        rng.shuffle(order)
        out[bi, ji] = lex[order[:n_iters]]
    return out


_LEX_TABLES = {}  # (V, device) -> (1, C(V,2), 2) uint8: the pair list of a rig whose pairs all fit n_iters


def _lexicographic_pairs(v, dev):
    key = (v, str(dev))
    if key not in _LEX_TABLES:
        lex = np.array(list(itertools.combinations(range(v), 2)), dtype=np.uint8).reshape(1, -1, 2)
        _LEX_TABLES[key] = torch.from_numpy(lex).to(dev)
    return _LEX_TABLES[key]


def triangulate_batch(
    heatmaps,
    proj_matricies,
    stride,
    valid_joints,
    use_soft_argmax=False,
    use_reprojection_xe=False,
    sigma=None,
    n_iters=64,
    reprojection_error_epsilon=5,
    mirror_nonsquare_quirk=True,
    keypoints_2d=None,
    pair_rng=None,
    valid_joints_host=None,
    view_valid=None,
    view_valid_host=None,
    view_joint_valid=None,
    view_joint_valid_host=None,
    refine="none",
    refine_3d="none",
    refine_3d_weights=None,
    refine_3d_epsilon=None,
    undistort="none",
    intrinsics=None,
    distortion=None,
    weights=None,
    return_inlier_mask=False,
):
    """heatmaps (B,V,J,Hh,Wh) f32 HIP tensor, proj (B,V,3,4), valid (B,J) ->
    dict of HIP tensors: keypoints_3d (B,J,3) f64, keypoints_2d (B,V,J,2) i64|f32,
    metric (B,) f64, inlier_count (B,) i32 (-1 where no joint is valid), joint_error,
    joint_inliers (B,J).

    ``mirror_nonsquare_quirk``: the reference splits the flat arg-max index with
    ``shape[2]`` (the map HEIGHT) for both x and y (utils/evaluation.py:25-26).
    True reproduces that bit for bit; False uses the geometrically correct width.

    ``keypoints_2d``: key-points already decoded from these heat-maps (the fused scoring pass,
    ``_lib.score_decode_maps``): the decode launch, i.e. a second read of the heat-maps, is skipped.

    ``pair_rng``: with more view pairs than ``n_iters`` the reference samples pairs from python's global
    ``random``; pass that module (or a ``random.Random``) to draw them here in the reference's order
    (``draw_view_pairs``: frames in batch order, valid joints ascending).  None raises NotImplementedError
    there.  Nothing is drawn when all C(V,2) pairs fit ``n_iters``.  At most 32 views.

    ``valid_joints_host``: ``valid_joints`` once more, on the host, for callers that hand the mask in as a device
    tensor: the draw reads the mask on the host, and copying a device mask back blocks the host on the current
    stream.  The drawn table goes up through pinned memory without blocking.

    ``view_valid`` (B, V), nonzero = the view is present in that frame (None: every view is, today's path call for
    call).  Each frame's result is what this function gives on that frame's present views alone, bit for bit; all frames
    go through ONE triangulation launch, however their present sets differ.  Nothing of an absent view is used (its
    heat-maps and matrix may hold NaN); ``keypoints_2d`` comes back dense with the rows of absent views zero.  A frame
    with fewer than two present views and a valid joint gets inlier_count -2, metric NaN and keypoints_3d 0 (the
    reference asserts two views); without a valid joint it is -1 as ever.  Up to 11 views nothing of the mask is needed
    on the host; beyond, the pair tables are built per frame from its present views (``draw_view_pairs``), from
    ``view_valid_host`` -- the mask once more on the host, as ``valid_joints_host`` -- where given.

    ``view_joint_valid`` (B, V, J), nonzero = joint j is usable in view v of frame b; ANDed with ``view_valid[:, :, None]``
    where that is given too.  Per joint the result is what this function gives on that joint's present views alone (B = 1,
    J = 1), bit for bit for a valid joint with two or more of them; all problems go through ONE triangulation launch.
    Nothing of an absent entry is used (its heat-map may hold NaN); ``keypoints_2d`` comes back dense with absent entries
    zero.  A valid joint with fewer than two present views is written like an invalid one (keypoints_3d, joint_error,
    joint_inliers 0); ``metric`` and ``inlier_count`` run over the USED joints (valid, two or more present views), and the
    result carries ``joint_used`` (B, J) uint8 = joint_inliers > 0.  No valid joint: inlier_count -1; a valid joint but no
    used one: -2, metric NaN.  Up to 11 views nothing of the mask is needed on the host; beyond, the per-problem pair
    tables are drawn from ``view_joint_valid_host`` where given -- a mask that exists on the device alone is copied back,
    which blocks the host on the current stream.

    ``refine``: "none" (today's path call for call) | "quarter" | "taylor", the sub-pixel refinement of the hard arg-max
    (``config.check_decode_refine``).  The hard decode is then made with ``split_width = wh`` whatever ``mirror_nonsquare_quirk`` says -- the
    reference's split by the height has no neighbourhood to refine in --, a ``keypoints_2d`` handed in must be that int64 decode,
    and the result carries the refined ``keypoints_2d`` (float32) and ``keypoints_conf`` (B, V, J) float32, the maps' values at
    their peaks (0 for absent entries and invalid joints).  Not together with ``use_soft_argmax``: ValueError.

    ``refine_3d``: "none" (today's path call for call: no new launch, no new keys) | "lm": one more launch
    (``mval_refine_points_3d``) moves every triangulated joint from its DLT point to the minimiser of the
    reprojection error over its support set -- the present views within ``refine_3d_epsilon`` (None: ``reprojection_error_epsilon``)
    of the DLT point.  The result's ``keypoints_3d`` are then the refined points, ``keypoints_3d_dlt`` the points before,
    ``joint_error`` and ``metric`` are recomputed from the refined points (the XE metric too), and ``joint_support`` (B, J) int32
    = the size of the support set and ``joint_status`` (B, J) int32 (0 not refined, k > 0 converged after k iterations, < 0
    the iteration cap was reached) are added; ``joint_inliers`` and ``inlier_count`` stay RANSAC's.  ``refine_3d_weights``:
    None | "conf" (``keypoints_conf``: needs ``refine`` != "none", else ValueError) | a (B, V, J) tensor; a view whose weight is
    non-finite or <= 0 leaves the support set.  The launch runs on the current stream and adds no host sync.

    ``undistort``: "none" (today's path call for call: no new launch, no new keys) | "brown": one more launch
    (``mval_undistort_keypoints``) between the decode -- whichever it was: the int64 hard decode, ``keypoints_2d``
    handed in, the soft-arg-max, a refined decode -- and the triangulation moves every key-point from its distorted pixel to the
    pinhole pixel of the same ray, with ``intrinsics`` (B, V, 3, 3), the K of ``proj_matricies`` = K [R|t], and ``distortion``
    (B, V, 5) = k1, k2, p1, p2, k3 (zeros: a view without distortion, handed through); both are needed, else ValueError.  The
    result's ``keypoints_2d`` are then the undistorted float32 points -- what was triangulated --, ``keypoints_2d_distorted`` the
    decode as it was, and ``undistort_status`` (B, V, J) int32: 0 not processed or no distortion, k > 0 converged after k
    iterations, < 0 handed through at the distorted position (``_lib.UNDISTORT_FOLD``, ``_lib.UNDISTORT_NOCONV``).  Nothing of an
    absent view is read (its K and distortion may hold NaN).  Not together with ``use_reprojection_xe``: ValueError.

    ``weights``: None (today's path call for call) | "conf" (``keypoints_conf``: needs ``refine`` != "none", else ValueError) | a
    (B, V, J) tensor, with any decode: the triangulation goes through ``mval_triangulate_ransac_weighted``, still one
    launch.  The two DLT rows of a (view, joint) entry are multiplied by its weight, in every pair solve and in the final solve;
    the vote and ``joint_error`` stay unweighted (pixels); among equally large inlier sets the larger summed weight wins, then the
    earlier pair.  An entry whose weight is not finite and > 0 is absent, as under ``view_joint_valid`` (its key-point may be NaN):
    a valid joint with fewer than two usable views is written like an invalid one, ``metric`` and ``inlier_count`` run over the used
    joints (-2 / NaN for a frame with a valid joint but no used one), and the result carries ``joint_used`` (B, J) uint8.  All-ones
    weights give the unweighted bits.  Beyond 11 views the pair tables are drawn from the masks alone, as without weights: a table
    entry naming a view with an unusable weight sits out on the device.  The launches after the triangulation take the same
    effective presence (present AND usable) as their per-entry mask: ``refine_3d`` takes its own vote as ever, over the usable entries
    -- an unused joint stays 0 with status 0, and the refined ``metric`` runs over the used joints --, and the XE metric sums the
    usable entries' maps.

    ``return_inlier_mask``: the result carries ``joint_inlier_mask`` (B, J) int32, bit v = view v is in RANSAC's winning set, the
    views of the final DLT (0 for an invalid or unused joint; its population count is ``joint_inliers``); always there under
    ``weights``.  Without ``weights`` every other key has the bits of the call without it."""
    check_undistort(undistort, use_reprojection_xe)
    weights = check_triangulation_weights(weights, refine)
    weighted = not (isinstance(weights, str) and weights == "none")
    if undistort != "none" and (intrinsics is None or distortion is None):
        raise ValueError("undistort=%r needs intrinsics (B, V, 3, 3) and distortion (B, V, 5)" % (undistort,))
    dev = _device_of(heatmaps)
    check_decode_refine(refine, use_soft_argmax)
    check_refine_3d(refine_3d, refine_3d_weights, refine)
    if heatmaps.dim() != 5:
        raise ValueError("heatmaps must be (B, V, J, Hh, Wh)")
    b, v, j, hh, wh = heatmaps.shape
    if undistort != "none":
        intrinsics, distortion = _camera_tensors(intrinsics, distortion, b, v)
    if v < 2:
        raise AssertionError("need at least two views")  # reference: assert len(points) >= 2
    if v > _lib.PAIRS_MAX_VIEWS:
        raise NotImplementedError("at most %d views (got %d): the device's inlier mask is 32 bits wide" % (_lib.PAIRS_MAX_VIEWS, v))
    per_joint = view_joint_valid is not None
    masked = view_valid is not None or per_joint
    sampled = not masked and v * (v - 1) // 2 > n_iters  # (under a mask the frames decide one by one: _masked_pair_tables)
    if sampled and pair_rng is None:
        raise NotImplementedError(_NEEDS_RNG)
    if (sampled or (masked and v > 11)) and n_iters < 1:
        raise ValueError("n_iters must be at least 1")
    hm = heatmaps.to(torch.float32).contiguous()
    proj = torch.as_tensor(proj_matricies).to(device=dev, dtype=torch.float64).reshape(b, v, 3, 4).contiguous()
    valid = _as_valid_u8(valid_joints, (b, j), dev)
    vv = _as_valid_u8(view_valid, (b, v), dev)
    vj = _as_valid_u8(view_joint_valid, (b, v, j), dev)
    if per_joint and vv is not None:
        vj = vj & vv[:, :, None]
    conf = None
    if refine != "none":
        kp2d = keypoints_2d if keypoints_2d is not None else _lib.argmax_decode(hm, valid, b, v, j, hh, wh, int(stride), wh)
        kp2d, conf = _lib.refine_keypoints(hm, kp2d, valid, b, v, j, hh, wh, int(stride), refine)
    elif keypoints_2d is not None:
        kp2d = keypoints_2d
    elif use_soft_argmax:
        kp2d = _lib.soft_argmax(hm, b * v * j, hh, wh, float(stride)).reshape(b, v, j, 2)
    else:
        kp2d = _lib.argmax_decode(hm, valid, b, v, j, hh, wh, int(stride), hh if mirror_nonsquare_quirk else wh)
    undistorted = None
    if undistort != "none":  # (the kernel reads the mask itself: K and distortion of an absent view may be NaN)
        kp2d_distorted = kp2d
        kp2d, undistort_status = _lib.undistort_keypoints(kp2d.contiguous(), intrinsics.to(dev), distortion.to(dev), valid, b, v, j,
                                                          view_valid=None if per_joint else vv, view_joint_valid=vj if per_joint else None)
        undistorted = {"keypoints_2d_distorted": kp2d_distorted, "undistort_status": undistort_status}
    if masked:
        # (the map kernels still decode the maps of absent views; a select, not a product: such a row may be NaN)
        present = vj.bool()[:, :, :, None] if per_joint else vv.bool()[:, :, None, None]
        kp2d = torch.where(present, kp2d, torch.zeros((), dtype=kp2d.dtype, device=dev))
        if conf is not None:
            conf = torch.where(present[..., 0], conf, torch.zeros((), dtype=conf.dtype, device=dev))
    eps = float(reprojection_error_epsilon)
    mask = dict(view_valid=None if per_joint else vv, view_joint_valid=vj if per_joint else None)  # the effective mask: one or none
    if sampled or (masked and v > 11):
        host_valid = valid_joints_host if valid_joints_host is not None else valid_joints
        host_valid = torch.ones((b, j)) if host_valid is None else torch.as_tensor(host_valid).reshape(b, j)
    pairs = None  # up to 11 views: lane p takes lexicographic pair p and sits out if a view is absent, no host knowledge of a mask
    if masked and v > 11:
        host_mask = None  # the effective mask once more, on the host
        if view_valid is not None:
            host_mask = torch.as_tensor(view_valid_host if view_valid_host is not None else view_valid).reshape(b, v)
        if per_joint:
            host_vj = torch.as_tensor(view_joint_valid_host if view_joint_valid_host is not None else view_joint_valid).reshape(b, v, j)
            host_mask = host_vj if host_mask is None else (host_vj.cpu() != 0) & (host_mask.reshape(b, v, 1).cpu() != 0)
        pairs = _masked_pair_tables(host_valid, host_mask, v, n_iters, pair_rng).pin_memory().to(dev, non_blocking=True)
    elif sampled:
        pairs = torch.from_numpy(draw_view_pairs(host_valid, v, n_iters, pair_rng)).pin_memory().to(dev, non_blocking=True)
    elif v > 11:  # all pairs, more than the 64 the one-lane-per-pair entry holds
        pairs = _lexicographic_pairs(v, dev)
    jmask = None
    post_mask = mask  # what the launches after the triangulation take for presence
    if weighted or return_inlier_mask:
        w = None
        if weighted:  # "conf": the peak heights, absent entries already 0
            w = conf if isinstance(weights, str) else torch.as_tensor(weights).to(device=dev, dtype=torch.float32).reshape(b, v, j).contiguous()
            # the entry's effective presence, present AND usable, per entry: the 3-D refinement and the XE metric see the joints
            # and views the triangulation saw (comparisons and selects only: an absent entry's weight may be NaN)
            usable = torch.isfinite(w) & (w > 0)
            if masked:
                usable = usable & (vj.bool() if per_joint else vv.bool()[:, :, None])
            post_mask = dict(view_valid=None, view_joint_valid=usable.to(torch.uint8).contiguous())
        kp3d, jerr, jinl, metric, inl, jmask = _lib.triangulate_ransac_weighted(kp2d, proj, valid, b, v, j, eps, pairs=pairs, weights=w,
                                                                                want_inlier_mask=True, **mask)
    elif pairs is None:
        kp3d, jerr, jinl, metric, inl = _lib.triangulate_ransac(kp2d, proj, valid, b, v, j, eps, **mask)
    else:
        kp3d, jerr, jinl, metric, inl = _lib.triangulate_ransac_pairs(kp2d, proj, valid, pairs, b, v, j, eps, **mask)
    refined = None
    if refine_3d != "none":
        weights = refine_3d_weights
        if isinstance(weights, str):  # "conf" (check_refine_3d): the peak heights, absent entries already 0
            weights = conf
        elif weights is not None:
            weights = torch.as_tensor(weights).to(device=dev, dtype=torch.float32).reshape(b, v, j).contiguous()
        kp3d_dlt = kp3d
        kp3d, jerr, support, status, metric = _lib.refine_points_3d(
            kp2d, proj, valid, kp3d, jerr, jinl, b, v, j, eps if refine_3d_epsilon is None else float(refine_3d_epsilon),
            weights=weights, **post_mask)
        refined = {"keypoints_3d_dlt": kp3d_dlt, "joint_support": support, "joint_status": status}
    if use_reprojection_xe:
        xe = _lib.reprojection_xe(kp3d, proj, hm, b, v, j, hh, wh, float(sigma), **post_mask)
        # (-2: fewer than two views / no used joint: NaN, the reference never reaches _compute_xe)
        metric = torch.where(inl == -2, metric, xe) if masked or weighted else xe
    out = {
        "keypoints_3d": kp3d,
        "keypoints_2d": kp2d,
        "metric": metric,
        "inlier_count": inl,
        "joint_error": jerr,
        "joint_inliers": jinl,
    }
    if conf is not None:
        out["keypoints_conf"] = conf
    if refined is not None:
        out.update(refined)
    if undistorted is not None:
        out.update(undistorted)
    if jmask is not None:
        out["joint_inlier_mask"] = jmask
    if per_joint or weighted:
        out["joint_used"] = (jinl > 0).to(torch.uint8)  # a used joint's winning pair is in its own inlier set: >= 2
    return out


def decode_keypoints(heatmaps, stride, valid_joints=None, refine="none"):
    """The 2-D key-points alone: heatmaps (B, V, J, Hh, Wh) f32 HIP tensor, valid_joints (B, J) or None -> (keypoints_2d, conf).
    "none": the hard arg-max (B, V, J, 2) int64 as ``triangulate_batch`` decodes it by default (the reference's split), conf None.
    "quarter" | "taylor": the refined key-points float32, split by the width, and conf (B, V, J) float32, the peak values."""
    _device_of(heatmaps)
    check_decode_refine(refine)
    if heatmaps.dim() != 5:
        raise ValueError("heatmaps must be (B, V, J, Hh, Wh)")
    b, v, j, hh, wh = heatmaps.shape
    hm = heatmaps.to(torch.float32).contiguous()
    valid = _as_valid_u8(valid_joints, (b, j), hm.device)
    if refine == "none":
        return _lib.argmax_decode(hm, valid, b, v, j, hh, wh, int(stride), hh), None
    kp2d = _lib.argmax_decode(hm, valid, b, v, j, hh, wh, int(stride), wh)
    return _lib.refine_keypoints(hm, kp2d, valid, b, v, j, hh, wh, int(stride), refine)


def _camera_tensors(intrinsics, distortion, b, v):
    """``intrinsics`` (B, V, 3, 3) and ``distortion`` (B, V, 5), anything ``torch.as_tensor`` takes, as contiguous float64 tensors
    where they are; any other shape: ValueError (no device work yet)."""
    K, dist = torch.as_tensor(intrinsics), torch.as_tensor(distortion)
    if tuple(K.shape) != (b, v, 3, 3) or tuple(dist.shape) != (b, v, 5):
        raise ValueError("intrinsics must be (%d, %d, 3, 3) and distortion (%d, %d, 5) = k1, k2, p1, p2, k3 per view, got %r and %r"
                         % (b, v, b, v, tuple(K.shape), tuple(dist.shape)))
    return K.to(torch.float64).contiguous(), dist.to(torch.float64).contiguous()


def undistort_keypoints(keypoints_2d, intrinsics, distortion, valid_joints=None, view_valid=None, view_joint_valid=None):
    """The undistortion alone (``mval_undistort_keypoints``): keypoints_2d (B, V, J, 2) int64 | float32 HIP tensor in
    pixels of the network's input, intrinsics (B, V, 3, 3), distortion (B, V, 5) = k1, k2, p1, p2, k3 -> (keypoints float32
    (B, V, J, 2), status int32 (B, V, J)) as ``triangulate_batch(undistort="brown")`` returns them.  valid_joints (B, J),
    view_valid (B, V) and view_joint_valid (B, V, J) (ANDed with view_valid where both are given) say which entries exist:
    the others come back (0, 0) with status 0, and nothing of them is read."""
    if not torch.is_tensor(keypoints_2d) or keypoints_2d.dim() != 4 or keypoints_2d.shape[-1] != 2:
        raise ValueError("keypoints_2d must be a (B, V, J, 2) tensor")
    if keypoints_2d.dtype not in (torch.int64, torch.float32):
        raise ValueError("keypoints_2d must be int64 (the hard decode) or float32, got %s" % (keypoints_2d.dtype,))
    b, v, j = keypoints_2d.shape[:3]
    K, dist = _camera_tensors(intrinsics, distortion, b, v)
    dev = _device_of(keypoints_2d)
    valid = _as_valid_u8(valid_joints, (b, j), dev)
    vv = _as_valid_u8(view_valid, (b, v), dev)
    vj = _as_valid_u8(view_joint_valid, (b, v, j), dev)
    if vj is not None and vv is not None:
        vj, vv = vj & vv[:, :, None], None
    return _lib.undistort_keypoints(keypoints_2d.contiguous(), K.to(dev), dist.to(dev), valid, b, v, j, view_valid=vv, view_joint_valid=vj)


_NEEDS_RNG = ("more view pairs than n_iters: the reference samples pairs from python's global RNG there "
              "(pass pair_rng=random to draw them in its order)")


def _masked_pair_tables(host_valid, host_view_valid, v, n_iters, pair_rng):
    """The per-problem pair tables of a masked batch with more than 11 views, as a host tensor (``draw_view_pairs``); without
    ``pair_rng`` only where no frame (no problem) has more present pairs than ``n_iters``.  ``host_view_valid``: (B, V), or
    the effective (B, V, J) mask of a batch with ``view_joint_valid``."""
    host_vv = (host_view_valid != 0).cpu().numpy()
    n_present = host_vv.sum(axis=1)
    if bool((n_present * (n_present - 1) // 2 > n_iters).any()) and pair_rng is None:
        raise NotImplementedError(_NEEDS_RNG)
    if host_vv.ndim == 3:
        return torch.from_numpy(draw_view_pairs(host_valid, v, n_iters, pair_rng, view_joint_valid=host_vv))
    return torch.from_numpy(draw_view_pairs(host_valid, v, n_iters, pair_rng, host_vv))


def peak_mask(heatmaps, min_peak):
    """The peak gate: heatmaps (B, V, J, h, w) f32 HIP tensor -> (B, V, J) uint8 on the device, 1 where some element of the
    map is ``>= min_peak``.  A comparison, so a map of NaNs is absent; exact, equal to
    ``(heatmaps >= min_peak).flatten(-2).any(-1)``.  One read of the maps (``mval_peak_mask``), no host sync: a mask for
    ``view_joint_valid`` where no annotation says which joints a view sees."""
    _device_of(heatmaps)
    if heatmaps.dim() != 5:
        raise ValueError("heatmaps must be (B, V, J, Hh, Wh)")
    b, v, j, hh, wh = heatmaps.shape
    hm = heatmaps.to(torch.float32).contiguous()
    return _lib.peak_mask(hm, float(min_peak), b * v * j, hh, wh).reshape(b, v, j)


def triangulation(
    heatmaps,
    proj_matricies,
    stride,
    valid_joints,
    use_soft_argmax=False,
    use_reprojection_xe=False,
    sigma=None,
    n_iters=64,
    reprojection_error_epsilon=5,
    direct_optimization=False,
    view_valid=None,
    view_joint_valid=None,
    refine="none",
    refine_3d="none",
    refine_3d_weights=None,
    undistort="none",
    intrinsics=None,
    distortion=None,
    weights=None,
    return_inlier_mask=False,
):
    """One frame, reference signature and return types (utils/triangulation.py:168-233):
    heatmaps (V,J,Hh,Wh), proj (V,3,4), valid (J,) -> {"keypoints_3d": ndarray (J,3) f64,
    "keypoints_2d": ndarray (V,J,2) int64|f32, "metric": float, "inlier_count": int}.
    ``view_valid`` (V,): the views present in this frame (``triangulate_batch``); fewer than two of them with a valid
    joint raise the reference's AssertionError.  ``view_joint_valid`` (V, J): the views each joint is usable in; a valid joint
    but none with two such views raises the same AssertionError.  ``refine``: the sub-pixel decode of ``triangulate_batch``; the
    result then also holds "keypoints_conf": ndarray (V, J) f32.  ``refine_3d`` = "lm" (with ``refine_3d_weights`` None | "conf" |
    (V, J)): the 3-D refinement of ``triangulate_batch``; "keypoints_3d" are then the refined points and the result also holds
    "keypoints_3d_dlt" (J, 3) f64, "joint_error" (J,) f64, "joint_support" and "joint_status" (J,) int32.  ``undistort`` = "brown"
    with ``intrinsics`` (V, 3, 3) and ``distortion`` (V, 5): the undistortion of ``triangulate_batch``; "keypoints_2d" are then the
    undistorted float32 points and the result also holds "keypoints_2d_distorted" (V, J, 2) and "undistort_status" (V, J) int32.
    ``weights`` None | "conf" | (V, J) and ``return_inlier_mask``: the confidence-weighted triangulation of ``triangulate_batch``; the
    result then also holds "joint_inlier_mask" (J,) int32 and, under weights, "joint_used" (J,) uint8; a valid joint but none with
    two usable views raises the AssertionError above."""
    if direct_optimization:
        raise NotImplementedError(
            "direct_optimization (scipy Huber least-squares, off in every reference call site): its result is where "
            "scipy's iteration stops, not a minimum, so there is nothing to hold a device version to"
        )
    import random
    r = triangulate_batch(
        heatmaps.unsqueeze(0),
        torch.as_tensor(proj_matricies).unsqueeze(0),
        stride,
        torch.as_tensor(valid_joints).reshape(1, -1),
        use_soft_argmax,
        use_reprojection_xe,
        sigma,
        n_iters,
        reprojection_error_epsilon,
        pair_rng=random,
        view_valid=None if view_valid is None else torch.as_tensor(view_valid).reshape(1, -1),
        view_joint_valid=None if view_joint_valid is None else torch.as_tensor(view_joint_valid).unsqueeze(0),
        refine=refine,
        **({} if refine_3d == "none" and refine_3d_weights is None else dict(
            refine_3d=refine_3d,
            refine_3d_weights=refine_3d_weights if refine_3d_weights is None or isinstance(refine_3d_weights, str)
            else torch.as_tensor(refine_3d_weights).unsqueeze(0))),
        **({} if undistort == "none" and intrinsics is None and distortion is None else dict(
            undistort=undistort, intrinsics=None if intrinsics is None else torch.as_tensor(intrinsics).unsqueeze(0),
            distortion=None if distortion is None else torch.as_tensor(distortion).unsqueeze(0))),
        **({} if weights is None and not return_inlier_mask else dict(
            weights=weights if weights is None or isinstance(weights, str) else torch.as_tensor(weights).unsqueeze(0),
            return_inlier_mask=return_inlier_mask)),
    )
    inl = int(r["inlier_count"][0].item())
    if inl == -2:
        raise AssertionError("need at least two views")  # reference: assert len(points) >= 2
    if inl < 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")  # np.min([])
    out = {
        "keypoints_3d": r["keypoints_3d"][0].cpu().numpy(),
        "keypoints_2d": r["keypoints_2d"][0].cpu().numpy(),
        "metric": float(r["metric"][0].item()),
        "inlier_count": inl,
    }
    if "keypoints_conf" in r:
        out["keypoints_conf"] = r["keypoints_conf"][0].cpu().numpy()
    if "joint_status" in r:
        for key in ("keypoints_3d_dlt", "joint_error", "joint_support", "joint_status"):
            out[key] = r[key][0].cpu().numpy()
    if "undistort_status" in r:
        for key in ("keypoints_2d_distorted", "undistort_status"):
            out[key] = r[key][0].cpu().numpy()
    if "joint_inlier_mask" in r:
        for key in ("joint_inlier_mask",) + (() if weights is None or (isinstance(weights, str) and weights == "none") else ("joint_used",)):
            out[key] = r[key][0].cpu().numpy()
    return out

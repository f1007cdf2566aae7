"""Masked heat-map MSE -- drop-in for reference pose_estimators/loss.py:10-24.

``pose_2d_mse`` = sum(where(valid, (h - gt)^2, 0)) / (N * H * W): the divisor omits J
(SURVEY Appendix A.12).  Forward and backward are single fused HIP reductions
(``mval_masked_mse_fwd`` / ``_bwd``) wrapped in an autograd Function.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib


class _MaskedMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, heatmaps, gt, valid, denom):
        h = heatmaps.contiguous()
        g = gt.to(dtype=torch.float32).contiguous()
        lead = h.shape[0] * h.shape[1]
        hw = h.shape[-1] * h.shape[-2]
        if valid is None:
            v = None
        else:
            v = valid.expand(h.shape[0], h.shape[1], 1, 1).reshape(lead).to(torch.uint8).contiguous()
        out = _lib.masked_mse_fwd(h, g, v, lead, hw, denom)
        ctx.save_for_backward(h, g, v if v is not None else torch.empty(0, device=h.device))
        ctx.has_valid = v is not None
        ctx.dims = (lead, hw, denom)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, g, v = ctx.saved_tensors
        lead, hw, denom = ctx.dims
        gh = _lib.masked_mse_bwd(h, g, v if ctx.has_valid else None, grad_out.contiguous(), lead, hw, denom)
        return gh, None, None, None


def _valid_per_map(valid, n, j):
    """joint_valid broadcastable to (N, J, 1, 1) -> the (N * J,) uint8 mask the kernels read (None stays None)."""
    if valid is None:
        return None
    return valid.expand(n, j, 1, 1).reshape(n * j).to(torch.uint8).contiguous()


class _MaskedMSEPoints(torch.autograd.Function):
    """``_MaskedMSE`` against the Gaussian maps of key-points, rendered per pixel in both directions
    (``mval_masked_mse_points_fwd`` / ``_bwd``).  Saved for the backward: the heat-maps, the points, the sigmas and the mask --
    no (N, J, h, w) ground truth exists at any time."""

    @staticmethod
    def forward(ctx, heatmaps, pt, sigma, valid, denom):
        h = heatmaps.contiguous()
        n, j, hh, wh = h.shape
        v = _valid_per_map(valid, n, j)
        out = _lib.masked_mse_points_fwd(h, pt, sigma, v, n * j, hh, wh, denom)
        per_map = torch.is_tensor(sigma)
        none = torch.empty(0, device=h.device)
        ctx.save_for_backward(h, pt, sigma if per_map else none, v if v is not None else none)
        ctx.sigma = None if per_map else sigma
        ctx.has_valid = v is not None
        ctx.dims = (n * j, hh, wh, denom)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, pt, sm, v = ctx.saved_tensors
        lead, hh, wh, denom = ctx.dims
        gh = _lib.masked_mse_points_bwd(h, pt, sm if ctx.sigma is None else ctx.sigma, v if ctx.has_valid else None,
                                        grad_out.contiguous(), lead, hh, wh, denom)
        return gh, None, None, None, None


class _WeightedMSE(torch.autograd.Function):
    """The weighted / hard-key-point-mining loss against ground truth in memory (``mval_weighted_mse_fwd`` / ``_bwd``).  Returns
    (loss, per-map weight * sum of squared errors (N * J,) f64, not differentiable).  Saved for the backward: the heat-maps, the
    ground truth and ``wsel`` (the weights of the maps the selection kept, 0 elsewhere)."""

    @staticmethod
    def forward(ctx, heatmaps, gt, weight, topk):
        h = heatmaps.contiguous()
        g = gt.to(dtype=torch.float32).contiguous()
        n, j, hh, wh = h.shape
        out, per_map, wsel = _lib.weighted_mse_fwd(h, g, weight, topk, n, j, hh, wh)
        ctx.save_for_backward(h, g, wsel)
        ctx.mark_non_differentiable(per_map)
        return out, per_map

    @staticmethod
    def backward(ctx, grad_out, _grad_per_map):
        h, g, wsel = ctx.saved_tensors
        n, j, hh, wh = h.shape
        return _lib.weighted_mse_bwd(h, g, wsel, grad_out.contiguous(), n, j, hh, wh), None, None, None


class _WeightedMSEPoints(torch.autograd.Function):
    """``_WeightedMSE`` against the Gaussian maps of key-points, rendered per pixel in both directions
    (``mval_weighted_mse_points_fwd`` / ``_bwd``).  Saved for the backward: the heat-maps, the points, the sigmas and ``wsel`` -- no
    (N, J, h, w) ground truth exists at any time."""

    @staticmethod
    def forward(ctx, heatmaps, pt, sigma, weight, topk):
        h = heatmaps.contiguous()
        n, j, hh, wh = h.shape
        out, per_map, wsel = _lib.weighted_mse_points_fwd(h, pt, sigma, weight, topk, n, j, hh, wh)
        per_map_sigma = torch.is_tensor(sigma)
        ctx.save_for_backward(h, pt, sigma if per_map_sigma else torch.empty(0, device=h.device), wsel)
        ctx.sigma = None if per_map_sigma else sigma
        ctx.mark_non_differentiable(per_map)
        return out, per_map

    @staticmethod
    def backward(ctx, grad_out, _grad_per_map):
        h, pt, sm, wsel = ctx.saved_tensors
        n, j, hh, wh = h.shape
        gh = _lib.weighted_mse_points_bwd(h, pt, sm if ctx.sigma is None else ctx.sigma, wsel, grad_out.contiguous(), n, j, hh, wh)
        return gh, None, None, None, None


def _weights_per_map(joint_weight, n, j, device, what):
    """joint_weight broadcastable to (N, J) -> the (N * J,) float32 weights the kernels read, on ``device``; weights that arrive on
    the host are checked there (finite, >= 0), a device tensor is taken as it is (``_lib.loss_weights``)."""
    w = torch.as_tensor(joint_weight).detach().to(torch.float32)
    try:
        w = torch.broadcast_to(w, (n, j))
    except RuntimeError:
        raise _lib.MvalError("%s: joint_weight %s does not broadcast to (%d, %d)" % (what, tuple(w.shape), n, j)) from None
    return _lib.loss_weights(w.reshape(n * j), n * j, device, what)


def _check_topk(topk, j, what):
    if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)) or not 0 <= topk <= j:
        raise _lib.MvalError("%s: topk %r is not an integer in [0, %d]" % (what, topk, j))
    return int(topk)


def _points_target(heatmaps, points, sigma, what):
    """points (N, J, 2) as float64 on the heat-maps' device, and sigma as the kernels take it: a positive float, or one per map
    ((N * J,) float64 on the device) from a tensor / array broadcastable to (N, J) -- a (N,) one is per image."""
    n, j, hh, wh = heatmaps.shape
    points = torch.as_tensor(points)
    if tuple(points.shape) != (n, j, 2):
        raise _lib.MvalError("%s: points %s are not (%d, %d, 2)" % (what, tuple(points.shape), n, j))
    pt = points.detach().to(device=heatmaps.device, dtype=torch.float64).contiguous()
    if not torch.is_tensor(sigma) and np.ndim(sigma) == 0:
        sigma = float(sigma)
        if not sigma > 0:
            raise _lib.MvalError("%s: sigma must be positive, got %r" % (what, sigma))
    else:
        s = torch.as_tensor(sigma).detach().to(torch.float64)
        if s.dim() == 1 and s.shape[0] == n:
            s = s.reshape(n, 1)
        s = torch.broadcast_to(s, (n, j)).reshape(n * j)
        sigma = _lib._points_sigma(s, n * j, heatmaps.device, what)[1]
    return pt, sigma


def _per_frame_args(heatmaps, joint_valid):
    """(B, V, J, h, w) float32 heat-maps, contiguous, and the (B * V * J,) uint8 mask of ``joint_valid`` (or None)."""
    if heatmaps.dim() != 5:
        raise _lib.MvalError("per-frame loss: heat-maps must be (B, V, J, h, w), got %s" % (tuple(heatmaps.shape),))
    h = heatmaps.to(dtype=torch.float32).contiguous()
    b, v, j = h.shape[:3]
    if joint_valid is None:
        return h, None
    valid = torch.broadcast_to(torch.as_tensor(joint_valid).to(h.device) != 0, (b, v, j))
    return h, valid.to(torch.uint8).contiguous().reshape(b * v * j)


class Pose2DMeanSquaredError:
    def pose_2d_mse(self, heatmaps, gt_heatmaps, joint_valid=None):
        """heatmaps, gt (N, J, H, W); joint_valid broadcastable (N, J, 1, 1) bool/uint8."""
        denom = heatmaps.shape[0] * heatmaps.shape[-1] * heatmaps.shape[-2]
        return _MaskedMSE.apply(heatmaps, gt_heatmaps, joint_valid, float(denom))

    def pose_2d_mse_from_points(self, heatmaps, points, sigma, joint_valid=None):
        """``pose_2d_mse`` against the Gaussian maps of ``points`` without materialising them, forward and backward
        (``mval_masked_mse_points_fwd`` / ``_bwd``): loss and ``heatmaps.grad`` are bit-identical to
        ``pose_2d_mse(heatmaps, utils.preprocess.gt_heatmaps(points, sigma, h, w), joint_valid)``.
        heatmaps (N, J, h, w); points (N, J, 2) in heat-map pixels, taken to float64 on the heat-maps' device; sigma a float, or a
        tensor / array broadcastable to (N, J) -- a (N,) one is per image (labelled frames DATA.SIGMA, pseudo-labelled ones
        DATA.PSEUDO_LABEL_SIGMA in one batch); joint_valid and the divisor (N * h * w, J omitted) as in ``pose_2d_mse``.
        Every sigma must be > 0: checked for a float and for an array that arrives on the host."""
        n, j, hh, wh = heatmaps.shape
        pt, sigma = _points_target(heatmaps, points, sigma, "pose_2d_mse_from_points")
        return _MaskedMSEPoints.apply(heatmaps, pt, sigma, joint_valid, float(n * hh * wh))

    def pose_2d_mse_weighted(self, heatmaps, gt_heatmaps, joint_weight, topk=0, return_per_map=False):
        """``pose_2d_mse`` with per-joint weights and online hard key-point mining (``mval_weighted_mse_fwd`` / ``_bwd``, DESIGN.md
        3.7c).  heatmaps, gt (N, J, h, w); joint_weight broadcastable to (N, J), finite and >= 0 (checked where it arrives on the
        host, else MvalError; a device tensor is taken as it is); topk an integer in [0, J].
          l[n, j] = joint_weight[n, j] * sum over pixels of (h - gt)^2     (a map of weight 0 is not read: its NaNs do not count)
          per image the topk largest l count (NaN first, ties to the lowest joint), all of them for topk = 0
          loss = sum of the counted l / (N * h * w)
        The divisor omits J as ``pose_2d_mse``'s does and there is NO division by topk: topk = J is the weighted loss, a smaller
        topk only removes terms (HRNet's JointsOHKMMSELoss divides by topk and carries a factor 0.5).  The weight multiplies the
        squared error: HRNet's ``target_weight`` t multiplies prediction and target, so it corresponds to joint_weight = t ** 2.
        With weights in {0, 1} and topk = 0 the gradient is ``pose_2d_mse``'s under that mask, bit for bit.
        ``return_per_map``: also l / (h * w) as a detached (N, J) float64 tensor, for logging."""
        what = "pose_2d_mse_weighted"
        n, j, hh, wh = heatmaps.shape
        if tuple(gt_heatmaps.shape) != (n, j, hh, wh):
            raise _lib.MvalError("%s: ground truth %s does not match heat-maps %s" % (what, tuple(gt_heatmaps.shape), (n, j, hh, wh)))
        w = _weights_per_map(joint_weight, n, j, heatmaps.device, what)
        out, per_map = _WeightedMSE.apply(heatmaps, gt_heatmaps, w, _check_topk(topk, j, what))
        return (out, per_map.detach().reshape(n, j) / float(hh * wh)) if return_per_map else out

    def pose_2d_mse_weighted_from_points(self, heatmaps, points, sigma, joint_weight, topk=0, return_per_map=False):
        """``pose_2d_mse_weighted`` against the Gaussian maps of ``points`` without materialising them, forward and backward
        (``mval_weighted_mse_points_fwd`` / ``_bwd``): bit-identical to
        ``pose_2d_mse_weighted(heatmaps, utils.preprocess.gt_heatmaps(points, sigma, h, w), joint_weight, topk)``.  points and sigma
        as in ``pose_2d_mse_from_points``; a point under weight 0 may be NaN."""
        what = "pose_2d_mse_weighted_from_points"
        n, j, hh, wh = heatmaps.shape
        pt, sigma = _points_target(heatmaps, points, sigma, what)
        w = _weights_per_map(joint_weight, n, j, heatmaps.device, what)
        out, per_map = _WeightedMSEPoints.apply(heatmaps, pt, sigma, w, _check_topk(topk, j, what))
        return (out, per_map.detach().reshape(n, j) / float(hh * wh)) if return_per_map else out

    def pose_2d_mse_single_batch(self, heatmap, gt_heatmap):
        """loss.py:22-24: sum((h - gt)^2) / (H * W)."""
        h = heatmap.reshape(1, -1, heatmap.shape[-2], heatmap.shape[-1])
        g = gt_heatmap.reshape(1, -1, gt_heatmap.shape[-2], gt_heatmap.shape[-1])
        return _MaskedMSE.apply(h, g, None, float(heatmap.shape[-1] * heatmap.shape[-2]))

    def pose_2d_mse_per_frame(self, heatmaps, gt_heatmaps, joint_valid=None):
        """``pose_2d_mse_single_batch(heatmaps[b], gt_heatmaps[b])`` of every frame b from two launches
        (``mval_frame_loss``): heatmaps, gt (B, V, J, h, w); joint_valid broadcastable to (B, V, J), the maps that count
        (all by default).  Returns a (B,) float32 HIP tensor; a measurement, no autograd."""
        h, valid = _per_frame_args(heatmaps.detach(), joint_valid)
        if tuple(gt_heatmaps.shape) != tuple(h.shape):
            raise _lib.MvalError("per-frame loss: ground truth %s does not match heat-maps %s" % (tuple(gt_heatmaps.shape), tuple(h.shape)))
        g = gt_heatmaps.detach().to(dtype=torch.float32).contiguous()
        b, v, j, hh, wh = h.shape
        return _lib.frame_loss(h, g, valid, b, v * j, hh, wh)[0]

    def pose_2d_mse_per_frame_from_points(self, heatmaps, points, sigma, joint_valid=None):
        """``pose_2d_mse_per_frame`` against the Gaussian maps of ``points`` (B, V, J, 2) float64, heat-map pixels, without
        materialising them (``mval_frame_loss_points``): bit-identical to
        ``pose_2d_mse_per_frame(heatmaps, utils.preprocess.gt_heatmaps(points, sigma, h, w))``."""
        h, valid = _per_frame_args(heatmaps.detach(), joint_valid)
        b, v, j, hh, wh = h.shape
        if tuple(points.shape) != (b, v, j, 2):
            raise _lib.MvalError("per-frame loss: points %s are not (%d, %d, %d, 2)" % (tuple(points.shape), b, v, j))
        pt = points.detach().to(dtype=torch.float64).contiguous()
        return _lib.frame_loss_points(h, pt, sigma, valid, b, v * j, hh, wh)[0]

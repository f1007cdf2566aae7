"""Hot-path entry points of the reference's ``ActiveLearningStrategy`` (strategy.py):

  _compute_batch_heatmap :772-782     _compute_batch_loss :762-770
  _compute_mpe/_compute_hp/_compute_bsb :1149-1215
  _compute_sal_dict :1004-1147        selection part of _sal_pseudo_labeling :932-949
  train_step (inner loop body :460-487)   _evaluate_all core :597-636
  cluster :137-191 (over a loader; cluster_dict is its pass without the file)

Same names, arguments and result types, so that the reference's orchestration code
(experiment dirs, checkpoints, TensorBoard -- out of scope here) can call them unchanged.
What changes is the execution model: a batch of frames is scored by a handful of HIP
launches with NO per-sample device->host synchronisation and NO per-sample collective;
ranks exchange ONE packed table per scoring pass (two RCCL collectives: a size exchange, then the data gather) instead of the
reference's 8 tiny all_gathers per sample (strategy.py:1106-1114).
"""
from __future__ import annotations

import math
import random
from collections import OrderedDict
from heapq import nlargest

import numpy as np
import torch

from . import _lib
from .pose_estimators.loss import Pose2DMeanSquaredError
from .utils import coreset, evaluation, flip_test, preprocess, triangulation

_KIND = {"HP": _lib.SCORE_HP, "MPE": _lib.SCORE_MPE, "BSB": _lib.SCORE_BSB}


def _reduce_mode(kind: str, config: str) -> int:
    """Precision/order of the reference's aggregation: HP values are python
    floats (float64 sum), MPE/BSB values are np.float32 (float32 sum)."""
    if config == "AVG":
        return _lib.REDUCE_AVG_F64 if kind == "HP" else _lib.REDUCE_AVG_F32
    if config == "STD":
        return _lib.REDUCE_STD_F64 if kind == "HP" else _lib.REDUCE_STD_F32
    raise NotImplementedError("AL.%s_CONFIG should be either AVG or STD." % kind)


def _score_heatmaps(configs, heatmaps, joint_valid, stride=0, mirror_nonsquare_quirk=True, decode=False, view_valid=None,
                    view_joint_valid=None):
    """The heat-map scorer behind the three public functions below.  ``configs`` maps "HP" / "MPE" / "BSB" to "AVG" / "STD";
    heatmaps (B,V,J,Hh,Wh) f32 HIP, joint_valid (B,J).  ONE launch reads the heat-maps -- one kind without ``decode``:
    mval_score_maps; one kind with it: mval_score_decode_maps; several kinds: mval_score_decode_maps_all (csrc/scoring.hip builds
    them from the same stages: a statistic has the same bits whichever computes it) --, then ``mval_score_reduce_masked`` per kind.
    Returns an OrderedDict kind -> (out (B,) float64, per_map (B,V,J), n_peaks (B,V,J), valid, keypoints_2d or None).
    ``view_valid`` (B,V), nonzero = present: ``out`` is reduced over the present views of each frame alone
    (MVAL_MASK_VIEWS).  The map launch is unchanged -- per_map, n_peaks and keypoints_2d still hold entries for
    the maps of absent views, which every consumer ignores.
    ``view_joint_valid`` (B,V,J), nonzero = the joint is usable in that view (ANDed with ``view_valid`` where both are given):
    ``out`` is the reference's list of per-map values with the absent entries deleted -- same order, same arithmetic, n the
    entries left (MVAL_MASK_VIEW_JOINT)."""
    modes = OrderedDict((kind, _reduce_mode(kind, configs[kind])) for kind in configs)
    for kind in modes:
        if kind not in _KIND:
            raise NotImplementedError("no heat-map statistic %r" % (kind,))
    b, v, j, hh, wh = heatmaps.shape
    hm = heatmaps.to(torch.float32).contiguous()
    valid = (torch.as_tensor(joint_valid) != 0).to(torch.uint8).reshape(b, j).to(hm.device).contiguous()
    split_width = hh if mirror_nonsquare_quirk else wh
    vv = vj = None  # the effective mask: one or none
    if view_valid is not None:
        vv = (torch.as_tensor(view_valid) != 0).to(torch.uint8).reshape(b, v).to(hm.device).contiguous()
    if view_joint_valid is not None:
        vj = (torch.as_tensor(view_joint_valid) != 0).to(torch.uint8).reshape(b, v, j).to(hm.device)
        vj, vv = (vj if vv is None else vj & vv[:, :, None]).contiguous(), None
    reduce = lambda stat, mode: _lib.score_reduce(stat, valid, b, v, j, mode, view_valid=vv, view_joint_valid=vj)  # noqa: E731
    if len(modes) == 1:
        (kind,) = modes
        if decode:
            stat, cnt, kp2d = _lib.score_decode_maps(_KIND[kind], hm, valid, b, v, j, hh, wh, int(stride), split_width)
        else:
            (stat, cnt), kp2d = _lib.score_maps(_KIND[kind], hm, b * v * j, hh, wh), None
        stats, counts = {kind: stat}, {kind: cnt}  # (HP has no peaks: the kernel writes 0)
    else:
        stat, n_peaks, kp2d = _lib.score_decode_maps_all(hm, valid, b, v, j, hh, wh, int(stride), split_width, decode=decode)
        stats = {kind: stat[_KIND[kind]] for kind in modes}
        counts = {"HP": torch.zeros_like(n_peaks[0]) if "HP" in modes else None, "MPE": n_peaks[0], "BSB": n_peaks[1]}
    return OrderedDict((kind, (reduce(stats[kind], mode), stats[kind].reshape(b, v, j),
                               counts[kind].reshape(b, v, j), valid, kp2d)) for kind, mode in modes.items())


def score_heatmaps_batch(kind: str, config: str, heatmaps, joint_valid, view_valid=None, view_joint_valid=None):
    """heatmaps (B,V,J,Hh,Wh) f32 HIP, joint_valid (B,J) -> (B,) float64 HIP tensor holding
    the value the reference's ``_compute_{hp,mpe,bsb}`` returns for each frame (exactly
    representable float32 where the reference's result is float32); then per_map, n_peaks, valid.
    ``view_valid`` (B,V): the value over each frame's present views alone; ``view_joint_valid`` (B,V,J): over its present
    (view, joint) entries (``_score_heatmaps``)."""
    return _score_heatmaps({kind: config}, heatmaps, joint_valid, view_valid=view_valid, view_joint_valid=view_joint_valid)[kind][:4]


def score_decode_heatmaps_batch(kind: str, config: str, heatmaps, joint_valid, stride, mirror_nonsquare_quirk=True, view_valid=None,
                                view_joint_valid=None):
    """``score_heatmaps_batch`` + the hard arg-max decode of ``triangulate_batch`` from ONE read of the heat-maps
    (csrc/scoring.hip, DECODE): what a pool-scoring pass needs per map (strategy.py:1027-1090 reads every heat-map in
    get_scaled_pred_corrdinates AND in _compute_{hp,mpe,bsb}).  Returns (out, per_map, n_peaks, valid, keypoints_2d)."""
    return _score_heatmaps({kind: config}, heatmaps, joint_valid, stride, mirror_nonsquare_quirk, decode=True, view_valid=view_valid,
                           view_joint_valid=view_joint_valid)[kind]


def score_decode_heatmaps_all(configs, heatmaps, joint_valid, stride, mirror_nonsquare_quirk=True, decode=True, view_valid=None,
                              view_joint_valid=None):
    """``score_decode_heatmaps_batch`` for several kinds from ONE read of the heat-maps: ``configs`` maps "HP" / "MPE" / "BSB"
    to "AVG" / "STD".  Returns an OrderedDict kind -> (out, per_map, n_peaks, valid, keypoints_2d), each entry what
    ``score_decode_heatmaps_batch(kind, config, ...)`` returns (keypoints_2d None without ``decode``)."""
    return _score_heatmaps(configs, heatmaps, joint_valid, stride, mirror_nonsquare_quirk, decode, view_valid, view_joint_valid)


AL_STRATEGIES = ("HP", "MPE", "BSB", "TRIANGULATION", "CORESET", "RANDOM")


def check_strategies(strategies):
    """The strategy list of a multi-strategy pass as a tuple: known names (NotImplementedError, as ``score_batch`` raises
    for an unknown AL.STRATEGY), at least one, no duplicates (ValueError)."""
    names = tuple(strategies)
    for s in names:
        if s not in AL_STRATEGIES:
            raise NotImplementedError("unknown AL strategy %r (one of %s)" % (s, ", ".join(AL_STRATEGIES)))
    if not names:
        raise ValueError("at least one AL strategy expected")
    if len(set(names)) != len(names):
        raise ValueError("duplicate AL strategy in %r" % (names,))
    return names


def split_strategy_tables(per_rank, n_strategies):
    """Per-rank tables of a multi-strategy pass, [pose, frame_id, -, sal_metric, inlier_count, mkpe, keypoints_3d(3J),
    al_metric of strategy 0 .. E-1], -> one list of per-rank ``tables_to_sal_dict`` tables per strategy: the base
    columns with that strategy's al_metric in column 2."""
    out = []
    for e in range(n_strategies):
        tabs = []
        for tab in per_rank:
            tab = np.asarray(tab)
            w = tab.shape[1] - n_strategies
            if w < 6 or (w - 6) % 3:
                raise ValueError("split_strategy_tables: %d columns do not hold 6 + 3J + %d" % (tab.shape[1], n_strategies))
            t = tab[:, :w].copy()
            t[:, 2] = tab[:, w + e]
            tabs.append(t)
        out.append(tabs)
    return out


def _empty_sal_dict():
    return {k: OrderedDict() for k in ("al_metric", "sal_metric", "inlier_count", "pred_3d_keypoints", "mkpe")}


def tables_to_sal_dict(per_rank, batch_sizes, sal_dict=None):
    """Packed per-rank tables [pose, frame_id, al_metric, sal_metric, inlier_count, mkpe,
    keypoints_3d(3J)] -> the reference's five dicts, inserted in its gather order
    (for batch: for sample: for rank; strategy.py:1024,1036,1115-1145).

    ``batch_sizes``: one list of batch sizes PER RANK (a single flat list = every rank has that
    structure, the DistributedSampler case).  Ranks may be ragged (a short last shard, a short
    last batch): the walk covers the longest structure and skips what a rank does not have, so
    every rank builds the identical dict from the identical gathered inputs."""
    if sal_dict is None:
        sal_dict = _empty_sal_dict()
    j = (per_rank[0].shape[1] - 6) // 3
    if len(batch_sizes) == 0 or np.isscalar(batch_sizes[0]):
        batch_sizes = [list(batch_sizes)] * len(per_rank)
    if len(batch_sizes) != len(per_rank):
        raise ValueError("tables_to_sal_dict: one batch-size list per rank expected")
    sizes = [[int(x) for x in b] for b in batch_sizes]
    for r, (tab, b) in enumerate(zip(per_rank, sizes)):
        if sum(b) != tab.shape[0]:
            raise ValueError("tables_to_sal_dict: rank %d has %d rows but batch sizes sum to %d" % (r, tab.shape[0], sum(b)))
    from .parallel import reference_gather_order

    for r, row in reference_gather_order(sizes):
        e = per_rank[r][row]
        guid = "%s-%s" % (int(e[0]), int(e[1]))
        sal_dict["sal_metric"][guid] = float(e[3])
        sal_dict["inlier_count"][guid] = float(e[4])
        sal_dict["pred_3d_keypoints"][guid] = e[6:].reshape(j, 3).tolist()
        sal_dict["al_metric"][guid] = float(e[2])
        sal_dict["mkpe"][guid] = float(e[5])
    return sal_dict


_SMALL_KEYS = ("proj_matrices", "joint_valid", "3d_keypoints", "pose", "frame_id", "view_valid", "view_joint_valid")


def _stage_batch(dp, mask_keys=(), camera_keys=()):
    """The batch's SMALL tensors (cameras, validity, ground truth, ids) as device tensors, uploaded on the caller's stream BEFORE the
    network is launched, through pinned staging (torch's caching host allocator) with non_blocking copies.  Why: score_batch /
    evaluate_mkpe run inside the side-stream context (parallel.PostStream), and a pageable host -> device copy issued there blocks the
    host until the side stream -- which has just waited for this batch's network -- drains, so the NEXT batch's network could not be
    enqueued meanwhile.  A ``joint_valid`` that arrives on the host also stays there as ``joint_valid_host``: the
    view-pair draw of a rig with more than 11 views (utils.triangulation.draw_view_pairs) reads it, and copying the staged mask back
    would be such a blocking copy; a ``view_valid`` (frames with missing views) likewise stays as ``view_valid_host``, which that
    draw reads too, and so does a ``view_joint_valid`` (joints missing from single views) as ``view_joint_valid_host``.
    ``mask_keys``: further batch keys to stage like ``view_joint_valid`` (the key AL.VIEW_JOINT_VALID_KEY names).  ``camera_keys``:
    further batch keys to stage like ``proj_matrices`` (``intrinsics`` and ``distortion`` under UNDISTORT "brown").  Returns a shallow
    copy of ``dp``; host-only runs (no HIP device) get ``dp`` back."""
    if not torch.cuda.is_available() or not isinstance(dp, dict):
        return dp
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(dp)
    for k in _SMALL_KEYS + tuple(k for k in tuple(mask_keys) + tuple(camera_keys) if k not in _SMALL_KEYS):
        if k not in dp:
            continue
        t = torch.as_tensor(dp[k])
        if not t.is_cuda:
            if k in ("joint_valid", "view_valid", "view_joint_valid") or k in mask_keys:
                out[k + "_host"] = t
            t = t.contiguous()
            t = (t if t.is_pinned() else t.pin_memory()).to(dev, non_blocking=True)
        out[k] = t
    return out


TRAIN_TARGET_KEYS = ("gt_heatmap", "gt_points", "2d_keypoints")


def select_train_target(data, al_cfg):
    """What a training batch is compared against -- (kind, target, sigma), chosen as the CLUSTER pass chooses its target
    (``_stage_cluster_targets``); no device work:
      "gt_heatmap"  ``data["gt_heatmap"]`` itself, where the batch has it (the reference's loader); sigma None
      "points"      else ``data["gt_points"]`` (B, V, J, 2), float64 heat-map pixels -- what ``prepare_views(compact=True)`` returns
      "points"      else ``data["2d_keypoints"] / POSE_ESTIMATOR.STRIDE`` in float64
    and a KeyError naming the three keys otherwise.  For "points", sigma is the batch's ``gt_sigma`` ((B,), one per frame) where
    present, else DATA.SIGMA; a caller that mixes pseudo-labelled frames into a batch sets DATA.PSEUDO_LABEL_SIGMA for those
    frames (dataset/dataset.py:123-132).
    ``2d_keypoints`` is float32 in the reference's batch, while its ``gt_heatmap`` is rendered from the float64 projection: the maps
    of ``2d_keypoints / STRIDE`` are close to the reference's but not its bits.  ``gt_points`` is the exact path."""
    if "gt_heatmap" in data:
        return "gt_heatmap", data["gt_heatmap"], None
    if "gt_points" in data:
        pts = torch.as_tensor(data["gt_points"]).to(torch.float64)
    elif "2d_keypoints" in data:
        pts = torch.as_tensor(data["2d_keypoints"]).to(torch.float64) / al_cfg.POSE_ESTIMATOR.STRIDE
    else:
        raise KeyError("train_step: a batch needs one of %s" % ", ".join(repr(k) for k in TRAIN_TARGET_KEYS))
    return "points", pts, data["gt_sigma"] if "gt_sigma" in data else al_cfg.DATA.SIGMA


def _stage_small(t):
    """A small host tensor on the current device, staged like ``_SMALL_KEYS``: pinned, non-blocking, on the caller's stream."""
    if t.is_cuda:
        return t
    t = t.contiguous()
    return (t if t.is_pinned() else t.pin_memory()).to(torch.device("cuda", torch.cuda.current_device()), non_blocking=True)


def compose_joint_weights(per_view_joint_valid, loss_cfg, data):
    """The per-map weights of the weighted training loss (``pose_2d_mse_weighted``) as a (B, V, J) float32 host
    tensor, or None where nothing asks for them: every field of ``loss_cfg`` (TRAIN.LOSS, checked by ``check_train_loss``; None
    reads as the defaults) at its default and neither ``data[WEIGHT_KEY]`` nor ``data["pseudo_label"]`` in the batch.  Otherwise
      w[b, v, j] = (valid != 0 ? 1 : 0) * JOINT_WEIGHTS[j] * (pseudo_label[b] ? PSEUDO_LABEL_WEIGHT : 1) * data[WEIGHT_KEY][b, v, j]
    in float32, the factors applied in that order (an empty JOINT_WEIGHTS, a missing ``pseudo_label`` and a missing key are 1).
    ``pseudo_label`` is (B,), nonzero for a pseudo-labelled frame: the loader that sets ``gt_sigma`` per frame sets it too.  A
    device tensor among the inputs keeps the result on the device; the loss checks weights only where they are on the host."""
    from .config import check_train_loss

    valid = torch.as_tensor(per_view_joint_valid)
    if valid.dim() != 3:
        raise ValueError("compose_joint_weights: per_view_joint_valid must be (B, V, J), got %s" % (tuple(valid.shape),))
    b, v, j = valid.shape
    joint_weights, topk, pseudo_weight, key = ((), 0, 1.0, "") if loss_cfg is None else check_train_loss(loss_cfg, j)
    extra = data[key] if key and key in data else None
    pseudo = data["pseudo_label"] if "pseudo_label" in data else None
    if not joint_weights and topk == 0 and pseudo_weight == 1.0 and key == "" and extra is None and pseudo is None:
        return None
    w = (valid != 0).to(torch.float32)
    if joint_weights:
        w = w * torch.tensor(joint_weights, dtype=torch.float32, device=w.device).reshape(1, 1, j)
    if pseudo is not None:
        pseudo = torch.as_tensor(pseudo)
        if tuple(pseudo.shape) != (b,):
            raise ValueError("compose_joint_weights: pseudo_label must be (B,) = (%d,), got %s" % (b, tuple(pseudo.shape)))
        factor = torch.where(pseudo != 0, torch.tensor(pseudo_weight, dtype=torch.float32, device=pseudo.device),
                             torch.ones((), dtype=torch.float32, device=pseudo.device))
        w = _times(w, factor.reshape(b, 1, 1))
    if extra is not None:
        extra = torch.as_tensor(extra).to(torch.float32)
        if tuple(extra.shape) != (b, v, j):
            raise ValueError("compose_joint_weights: data[%r] must be (B, V, J) = %s, got %s" % (key, (b, v, j), tuple(extra.shape)))
        w = _times(w, extra)
    return w


def _times(w, factor):
    """w * factor in float32; where one of the two is on the device, there."""
    if factor.is_cuda != w.is_cuda:
        w, factor = (w.to(factor.device), factor) if factor.is_cuda else (w, factor.to(w.device))
    return w * factor


class ActiveLearningStrategy:
    def __init__(self, al_cfg):
        self.al_cfg = al_cfg
        self.num_joints = al_cfg.DATA.NUM_JOINTS
        self.joint_root_index = 2 if al_cfg.DATA.TYPE == "panoptic" else 21  # strategy.py:34-37
        self.loss = Pose2DMeanSquaredError()

    @property
    def kmeans(self):
        """The SAL pose clusters (strategy.py:38-52), fitted on the device on first access: for
        ``EXPR_TYPE == "SAL"`` with a ``SAL.CLUSTER_FILE_PATH``, ``KMeans(SAL.NUM_CLUSTERS,
        random_state=RANDOM_SEED)`` on the file's root-relative poses; otherwise None.  Hand it to
        ``select_sal_guids(..., kmeans_centers=st.kmeans)``."""
        if "_kmeans" not in self.__dict__:
            cfg = self.al_cfg
            km = None
            if cfg.EXPR_TYPE == "SAL" and cfg.SAL.CLUSTER_FILE_PATH != "":
                from .utils.experiment_io import read_cluster_features
                from .utils.kmeans import KMeans

                feats = read_cluster_features(cfg.SAL.CLUSTER_FILE_PATH, self.joint_root_index)
                km = KMeans(cfg.SAL.NUM_CLUSTERS, random_state=cfg.RANDOM_SEED).fit(feats)
            self._kmeans = km
        return self._kmeans

    # ---- model glue ---------------------------------------------------------------
    @staticmethod
    def _batch_images_nchw(data):
        """The batch's images as the network takes them: (B,V,C,H,W) -> (B*V,C,H,W), frame-major / view-minor.  A compact batch
        carries the resized views as uint8 (B,V,H,W,3), a quarter of the bytes, and is normalised on the device
        (``mval_normalize_views_u8``) into the float32 tensor the reference's loader would have uploaded, bit for bit."""
        images = data["images"].cuda()
        if images.dtype == torch.uint8:
            if images.dim() != 5 or images.shape[4] != 3:
                raise ValueError("uint8 images must be (B, V, H, W, 3), got %s" % (tuple(images.shape),))
            h, w = images.shape[2], images.shape[3]
            return preprocess.normalize_views_u8(images.reshape([-1, h, w, 3]))
        c, h, w = images.shape[2], images.shape[3], images.shape[4]
        return images.reshape([-1, c, h, w])

    @staticmethod
    def _compute_batch_heatmap(pose_estimator, data):
        """strategy.py:772-782: the network on ``_batch_images_nchw`` (float32 or uint8 compact batches)."""
        return pose_estimator(ActiveLearningStrategy._batch_images_nchw(data))

    def _compute_batch_heatmap_flip(self, pose_estimator, data, mode):
        """``_compute_batch_heatmap`` under the flip test ``mode`` "mirror" | "mirror_shift" (DESIGN.md 6.8): the same batch
        (``_batch_images_nchw``: a uint8 compact batch is normalised once and the float32 result is mirrored), then
        ``flip_test_heatmaps`` -- the network, the mirrored batch, the network again, the merge, all on the caller's stream.  The
        merged maps carry their arg-max keys."""
        return flip_test.flip_test_heatmaps(pose_estimator, self._batch_images_nchw(data), self._flip_pairs(), mode)

    def _flip_pairs(self):
        """``flip_pairs`` of the config's DATA node, resolved on first use (a bad DATA.FLIP_PAIRS raises there)."""
        if "_flip_pairs_table" not in self.__dict__:
            self._flip_pairs_table = flip_test.flip_pairs(self.al_cfg.DATA)
        return self._flip_pairs_table

    def _flip_kwargs(self, node):
        """What a pass hands to ``_pool_loop`` for the FLIP_TEST of the config node ``node`` ("AL" | "EVAL"), read and checked once
        per pass: nothing under "none" or where the field is absent (the call is then the one it always was), else ``flip=mode`` --
        and the pair table is resolved, so that a bad one raises before the pass starts."""
        from .config import check_flip_test

        cfg = getattr(self.al_cfg, node)
        mode = check_flip_test(cfg.FLIP_TEST if "FLIP_TEST" in cfg else "none")
        if mode == "none":
            return {}
        self._flip_pairs()
        return {"flip": mode}

    @staticmethod
    def _compute_batch_loss(gt_heatmap, heatmaps, per_view_joint_valid, loss):
        """strategy.py:762-770."""
        _, _, j, h, w = gt_heatmap.shape
        return loss.pose_2d_mse(
            heatmaps, gt_heatmap.reshape([-1, j, h, w]), per_view_joint_valid.reshape([-1, j, 1, 1])
        )

    @staticmethod
    def _stage_train_points(points, sigma):
        """The points target (B, V, J, 2) float64 and its sigma on the device.  A per-frame sigma (B,) becomes one per image
        (B * V,); it is checked here, on the host, because the loss kernels cannot refuse a device array."""
        points = _stage_small(points)
        if not torch.is_tensor(sigma) and np.ndim(sigma) == 0:
            return points, float(sigma)
        b, v = points.shape[0], points.shape[1]
        s = torch.as_tensor(sigma).to(torch.float64).reshape(-1)
        if s.shape[0] != b:
            raise ValueError("train_step: gt_sigma must be (B,) = (%d,), got %s" % (b, tuple(torch.as_tensor(sigma).shape)))
        if not s.is_cuda and not bool((s > 0).all()):
            raise ValueError("train_step: every gt_sigma must be positive")
        return points, _stage_small(s.reshape(b, 1).expand(b, v).reshape(b * v))

    @staticmethod
    def _compute_batch_loss_points(points, sigma, heatmaps, per_view_joint_valid, loss):
        """``_compute_batch_loss`` against the maps of points (B, V, J, 2), not materialised."""
        j = heatmaps.shape[1]
        return loss.pose_2d_mse_from_points(heatmaps, points.reshape([-1, j, 2]), sigma, per_view_joint_valid.reshape([-1, j, 1, 1]))

    def train_step(self, pose_estimator, optimizer, data, lr_scheduler=None):
        """Body of the training inner loop (strategy.py:460-487): zero_grad -> heat-maps ->
        masked MSE -> host guard (NaN / inf / > LOSS_CLIP_VALUE skips the step)
        -> backward -> optimizer step -> scheduler step.  Returns (loss_value, stepped).
        The target is ``select_train_target``'s: ``gt_heatmap`` where the batch has it, else the maps of ``gt_points`` (or of
        ``2d_keypoints / STRIDE``, close to the reference's maps but not their bits) under ``gt_sigma`` / DATA.SIGMA, rendered
        inside the loss kernels and never materialised; ``images`` may be uint8 (``_compute_batch_heatmap``).
        Where ``compose_joint_weights`` returns weights -- a TRAIN.LOSS field off its default, a ``pseudo_label`` or the
        TRAIN.LOSS.WEIGHT_KEY tensor in the batch -- the loss is ``pose_2d_mse_weighted`` (``_from_points``) under them and
        TRAIN.LOSS.OHKM_TOPK; otherwise the calls are the ones they always were."""
        optimizer.zero_grad()
        kind, target, sigma = select_train_target(data, self.al_cfg)
        if kind == "points":  # the small tensors go up before the network, like _stage_batch's
            target, sigma = self._stage_train_points(target, sigma)
        loss_cfg = self.al_cfg.TRAIN.LOSS if "LOSS" in self.al_cfg.TRAIN else None
        weights = compose_joint_weights(data["per_view_joint_valid"], loss_cfg, data)
        if weights is not None:  # TRAIN.LOSS, pseudo_label or the WEIGHT_KEY tensor ask for the weighted loss: they go up here too
            if not weights.is_cuda and not bool((torch.isfinite(weights) & (weights >= 0)).all()):  # (the loss checks host weights only)
                raise ValueError("train_step: every loss weight must be finite and >= 0")
            weights = _stage_small(weights)
            topk = loss_cfg.OHKM_TOPK if loss_cfg is not None and "OHKM_TOPK" in loss_cfg else 0
        heatmaps = self._compute_batch_heatmap(pose_estimator, data)
        if kind == "gt_heatmap":
            gt = target.cuda()
        if weights is not None:
            j = heatmaps.shape[1]
            if kind == "gt_heatmap":
                batch_loss = self.loss.pose_2d_mse_weighted(heatmaps, gt.reshape((-1, j) + tuple(gt.shape[-2:])), weights.reshape(-1, j), topk)
            else:
                batch_loss = self.loss.pose_2d_mse_weighted_from_points(heatmaps, target.reshape([-1, j, 2]), sigma, weights.reshape(-1, j), topk)
        else:
            pv = data["per_view_joint_valid"].to(torch.uint8).cuda()
            if kind == "gt_heatmap":
                batch_loss = self._compute_batch_loss(gt, heatmaps, pv, self.loss)
            else:
                batch_loss = self._compute_batch_loss_points(target, sigma, heatmaps, pv, self.loss)
        value = batch_loss.data.item()
        ok = not (math.isnan(value) or math.isinf(value) or value > self.al_cfg.TRAIN.LOSS_CLIP_VALUE)
        if ok:
            batch_loss.backward()
            optimizer.step()
        if lr_scheduler is not None:
            lr_scheduler.step()
        return value, ok

    # ---- per-frame scorers (reference signatures) ---------------------------------------
    def _score_one(self, kind, config, heatmaps, joint_valid):
        out, _, n_peaks, valid = score_heatmaps_batch(kind, config, heatmaps.unsqueeze(0), torch.as_tensor(joint_valid).reshape(1, -1))
        if kind == "BSB":
            bad = (n_peaks[0] < 2) & (valid[0].bool()[None, :])
            if bool(bad.any().item()):
                raise IndexError("list index out of range")  # strategy.py:1208 with < 2 peaks
        if bool((n_peaks < 0).any().item()):
            raise _lib.MvalError("peak list overflow (> 2048 local maxima in one heat-map)")
        v = out[0].item()
        if config == "AVG":
            return float(v)
        return np.float64(v) if kind == "HP" else np.float32(v)

    def _compute_mpe(self, heatmaps, joint_valid):
        return self._score_one("MPE", self.al_cfg.AL.MPE_CONFIG, heatmaps, joint_valid)

    def _compute_hp(self, heatmaps, joint_valid):
        return self._score_one("HP", self.al_cfg.AL.HP_CONFIG, heatmaps, joint_valid)

    def _compute_bsb(self, heatmaps, joint_valid):
        return self._score_one("BSB", self.al_cfg.AL.BSB_CONFIG, heatmaps, joint_valid)

    # ---- joints missing from single views ------------------------------------------------
    def _mask_keys(self):
        """The batch keys that hold a per-(view, joint) visibility mask: ``view_joint_valid`` itself and the key that
        AL.VIEW_JOINT_VALID_KEY names."""
        from .config import check_view_joint_valid

        key, _ = check_view_joint_valid(self.al_cfg.AL.VIEW_JOINT_VALID_KEY, self.al_cfg.AL.MIN_PEAK)
        return ("view_joint_valid",) + ((key,) if key not in ("", "view_joint_valid") else ())

    def _stage_masked(self, dp):
        """``_stage_batch`` that also stages the key AL.VIEW_JOINT_VALID_KEY names (and keeps its host copy) and, under AL.UNDISTORT
        or EVAL.UNDISTORT "brown", the batch's ``intrinsics`` and ``distortion`` where it has them (``_batch_cameras`` raises where
        it has not)."""
        from .config import UNDISTORT_KEYS

        cfg = self.al_cfg
        nodes = [cfg[n] for n in ("AL", "EVAL") if n in cfg]
        brown = any("UNDISTORT" in n and n.UNDISTORT != "none" for n in nodes)
        return _stage_batch(dp, self._mask_keys()[1:], UNDISTORT_KEYS if brown else ())

    @staticmethod
    def _batch_cameras(dp, b):
        """The arguments ``triangulate_batch(undistort="brown")`` takes from a batch of ``b`` frames: its ``intrinsics`` (B, V, 3, 3) and
        ``distortion`` (B, V, 5) -- what ``prepare_views(with_cameras=True)`` returns per frame --, or KeyError naming both keys."""
        from .config import UNDISTORT_KEYS

        if not all(k in dp for k in UNDISTORT_KEYS):
            raise KeyError("UNDISTORT 'brown': the batch needs the keys %s (prepare_views(with_cameras=True))"
                           % " and ".join(repr(k) for k in UNDISTORT_KEYS))
        K, dist = (torch.as_tensor(dp[k]) for k in UNDISTORT_KEYS)
        return {"intrinsics": K.reshape(b, -1, 3, 3), "distortion": dist.reshape(b, -1, 5)}

    def _view_joint_valid(self, hm, dp):
        """The ONE place where a batch's per-(view, joint) mask is resolved.  hm (B,V,J,h,w) on the device.  Sources, ANDed:
        the batch's own ``view_joint_valid``; the batch key AL.VIEW_JOINT_VALID_KEY names (KeyError when the batch lacks it);
        with AL.MIN_PEAK > 0 the peak gate ``triangulation.peak_mask(hm, AL.MIN_PEAK)``, computed on the device without a host
        sync.  Returns (mask (B,V,J) uint8 on the device, host copy or None) -- (None, None) when nothing is given, which is
        every batch under the default config that has no ``view_joint_valid`` key.  The host copy (read by the pair draw of
        rigs with more than 11 views) exists when every source has one: ``<key>_host`` from ``_stage_batch``, or a tensor that
        is on the host anyway; the peak gate has none, and triangulate_batch then copies the device mask back (one blocking
        copy per batch, V > 11 only: DESIGN.md 6.3).  ``view_valid`` is not folded in here: the callees AND it."""
        from .config import check_view_joint_valid

        key, min_peak = check_view_joint_valid(self.al_cfg.AL.VIEW_JOINT_VALID_KEY, self.al_cfg.AL.MIN_PEAK)
        b, v, j = hm.shape[:3]
        mask, host, host_ok = None, None, True
        for name in self._mask_keys():
            if name != "view_joint_valid" and name not in dp:
                raise KeyError("AL.VIEW_JOINT_VALID_KEY %r: the batch has no such key" % (name,))
            if dp.get(name) is None:
                continue
            m = torch.as_tensor(dp[name])
            h = dp.get(name + "_host", None if m.is_cuda else m)
            m = (m.reshape(b, v, j) != 0).to(hm.device)
            mask = m if mask is None else mask & m
            if h is None:
                host_ok = False
            else:
                h = torch.as_tensor(h).reshape(b, v, j) != 0
                host = h if host is None else host & h
        if min_peak > 0.0:
            gate = triangulation.peak_mask(hm, min_peak).bool()
            mask = gate if mask is None else mask & gate
            host_ok = False
        if mask is None:
            return None, None
        return mask.to(torch.uint8).contiguous(), host if host_ok else None

    # ---- pool scoring ---------------------------------------------------------------
    def _score_columns(self, heatmaps, dp, strategies):
        """Everything the reference does per sample inside _compute_sal_dict (strategy.py:1036-1094,1134), for a whole
        batch, on device, for each of ``strategies``: one heat-map launch (when HP, MPE or BSB is among them; with the hard
        arg-max decode unless AL.USE_SOFTARGMAX), one triangulation.  heatmaps (B*V,J,h,w).  Returns float64 HIP columns
        (ids [pose, frame_id], rest [sal_metric, inlier_count, mkpe, keypoints_3d(3J)], al_metric per strategy).
        A batch with ``view_valid`` (B, V) -- frames with missing views -- is scored and triangulated over each frame's
        present views alone; one with a per-(view, joint) mask (``_view_joint_valid``) over each joint's present views, and
        its per-sample MKPE leaves out the joints nobody triangulated (``joint_valid & joint_used``).
        AL.DECODE_REFINE "quarter" | "taylor": the decode of the heat-map launch is split by the width and refined before
        the triangulation (``triangulate_batch(refine=...)``); "none" is the path above call for call.
        AL.REFINE_3D "lm" (with AL.REFINE_3D_WEIGHTS "none" | "conf"): every triangulated joint is refined by
        ``triangulate_batch(refine_3d=...)``, and sal_metric, the TRIANGULATION metric, the per-sample MKPE and
        the key-point columns come from the refined points; "none" adds no launch.
        AL.UNDISTORT "brown": the decoded key-points are undistorted with the batch's ``intrinsics`` and ``distortion`` before the
        triangulation (``triangulate_batch(undistort=...)``; KeyError when the batch lacks them, ValueError together
        with AL.USE_REPROJECTION_XE); "none" reads neither key and adds no launch.
        AL.TRIANGULATION_WEIGHTS "conf" (needs AL.DECODE_REFINE): the triangulation weights every (view, joint) entry by its peak
        height (``triangulate_batch(weights="conf")``), and the per-sample MKPE leaves out the joints without two
        usable views (``joint_valid & joint_used``); "none" is the path above call for call."""
        from .config import check_decode_refine, check_refine_3d, check_triangulation_weights, check_undistort

        cfg = self.al_cfg
        undistort = check_undistort(cfg.AL.UNDISTORT if "UNDISTORT" in cfg.AL else "none", cfg.AL.USE_REPROJECTION_XE)
        refine = check_decode_refine(cfg.AL.DECODE_REFINE if "DECODE_REFINE" in cfg.AL else "none", cfg.AL.USE_SOFTARGMAX)
        refine_3d, weights_3d = check_refine_3d(cfg.AL.REFINE_3D if "REFINE_3D" in cfg.AL else "none",
                                                cfg.AL.REFINE_3D_WEIGHTS if "REFINE_3D_WEIGHTS" in cfg.AL else "none", refine)
        tri_weights = check_triangulation_weights(cfg.AL.TRIANGULATION_WEIGHTS if "TRIANGULATION_WEIGHTS" in cfg.AL else "none", refine)
        dev = heatmaps.device
        pose = torch.as_tensor(dp["pose"]).reshape(-1)
        b = pose.shape[0]
        _, j, hh, wh = heatmaps.shape
        hm = heatmaps.reshape(b, -1, j, hh, wh)
        joint_valid = torch.as_tensor(dp["joint_valid"]).reshape(b, j)
        view_valid = dp.get("view_valid")
        vj, vj_host = self._view_joint_valid(hm, dp)
        configs = OrderedDict((s, getattr(cfg.AL, s + "_CONFIG")) for s in strategies if s in _KIND)
        scored, kp2d = {}, None
        if configs:
            # one read of every heat-map for the uncertainty statistics and the key-point decode
            if refine == "none":
                scored = _score_heatmaps(configs, hm, joint_valid, cfg.POSE_ESTIMATOR.STRIDE, decode=not cfg.AL.USE_SOFTARGMAX,
                                         view_valid=view_valid, view_joint_valid=vj)
            else:  # (the refinement works in the neighbourhood of the geometric peak: no split by the height)
                scored = _score_heatmaps(configs, hm, joint_valid, cfg.POSE_ESTIMATOR.STRIDE, mirror_nonsquare_quirk=False, decode=True,
                                         view_valid=view_valid, view_joint_valid=vj)
            kp2d = next(iter(scored.values()))[4]
        refined = {} if refine == "none" else {"refine": refine}
        if refine_3d != "none":
            refined.update(refine_3d=refine_3d, refine_3d_weights=None if weights_3d == "none" else weights_3d)
        if undistort != "none":
            refined.update(undistort=undistort, **self._batch_cameras(dp, b))
        if tri_weights != "none":
            refined.update(weights=tri_weights)
        r = triangulation.triangulate_batch(
            hm, dp["proj_matrices"], cfg.POSE_ESTIMATOR.STRIDE, joint_valid,
            cfg.AL.USE_SOFTARGMAX, cfg.AL.USE_REPROJECTION_XE, cfg.AL.REPROJECTION_SIGMA,
            keypoints_2d=kp2d,
            pair_rng=random,  # more than n_iters view pairs (12 views on): the reference's draws, frames in batch order
            valid_joints_host=dp.get("joint_valid_host"),
            view_valid=view_valid, view_valid_host=dp.get("view_valid_host"),
            view_joint_valid=vj, view_joint_valid_host=vj_host, **refined,
        )
        pred32 = r["keypoints_3d"].to(torch.float32)  # torch.Tensor(results["keypoints_3d"]) (:1046)
        sal_metric = r["metric"].to(torch.float32).to(torch.float64)  # torch.Tensor([metric]) (:1061)
        # frames with missing views: an absent view has no peak list to run short, the deferred peak checks count it as fine
        absent = None if view_valid is None or not configs else (torch.as_tensor(view_valid).reshape(b, -1) == 0).to(dev)[:, :, None]
        if vj is not None and configs:  # likewise an absent (view, joint) entry
            absent = (vj == 0) if absent is None else absent | (vj == 0)
        als = []
        for s in strategies:
            if s == "RANDOM":
                al = torch.cat([torch.rand(1) for _ in range(b)]).to(torch.float64).to(dev)
            elif s == "TRIANGULATION":
                al = r["metric"].to(torch.float64)  # torch.tensor([np.float64]) keeps float64 (:1075)
            elif s in _KIND:
                al, _, n_peaks, valid = scored[s][:4]
                if absent is not None:
                    n_peaks = torch.where(absent, torch.full_like(n_peaks, 2), n_peaks)
                self._pending_checks.append((s, n_peaks, valid))
                if configs[s] == "AVG" or s != "HP":
                    al = al.to(torch.float32).to(torch.float64)  # torch.tensor(python float) is float32
            elif s == "CORESET":
                al = torch.zeros(b, dtype=torch.float64, device=dev)
            else:
                raise NotImplementedError()
            als.append(al[:, None])
        gt = torch.as_tensor(dp["3d_keypoints"]).to(dev)
        scored_joints = joint_valid.to(dev)
        if vj is not None or tri_weights != "none":  # a joint nobody triangulated is not scored as a prediction at the origin
            scored_joints = ((scored_joints != 0) & r["joint_used"].bool()).to(scored_joints.dtype)
        mk = evaluation.mkpe_per_sample(pred32, gt, scored_joints)
        self._pending_checks.append(("INLIER", r["inlier_count"], None))
        ids = [pose.to(dev, torch.float64)[:, None], torch.as_tensor(dp["frame_id"]).reshape(b).to(dev, torch.float64)[:, None]]
        rest = [sal_metric[:, None], r["inlier_count"].to(torch.float64)[:, None], mk.to(torch.float64)[:, None],
                pred32.to(torch.float64).reshape(b, 3 * j)]
        return ids, rest, als

    def score_batch(self, heatmaps, dp):
        """``_score_columns`` under AL.STRATEGY as a (B, 6 + 3J) float64 HIP table:
        [pose, frame_id, al_metric, sal_metric, inlier_count, mkpe, keypoints_3d(3J)]."""
        ids, rest, als = self._score_columns(heatmaps, dp, (self.al_cfg.AL.STRATEGY,))
        return torch.cat(ids + als + rest, dim=1)

    def score_batch_all(self, heatmaps, dp, strategies):
        """``score_batch`` for several strategies from one network output: one heat-map launch, one triangulation.  Returns
        a (B, 6 + 3J + E) float64 HIP table: ``score_batch``'s columns with column 2 left 0, then the al_metric of each
        strategy, each what ``score_batch`` writes under that AL.STRATEGY."""
        ids, rest, als = self._score_columns(heatmaps, dp, strategies)
        return torch.cat(ids + [torch.zeros_like(als[0])] + rest + als, dim=1)

    def _pool_loop(self, data_loader, pose_estimator, body, inputs=None, stage=_stage_batch, flip="none"):
        """The loop of a pass over a pool: per batch ``stage(dp)`` (small tensors to the device BEFORE the network launch: no
        host-blocking copy on the side stream), the network, then ``body(*args)`` on the side stream (parallel.PostStream:
        beside the next batch's network), where ``args = inputs(heatmaps, dp)`` names every device tensor the body reads --
        by default the heat-maps, their arg-max keys where the network kept them, and the batch.  Nothing is copied to the
        host; the caller's stream has joined the side stream when the list of the bodies' results is returned.
        ``flip`` "mirror" | "mirror_shift": the heat-maps of every batch are ``_compute_batch_heatmap_flip``'s -- two forwards and the
        merge on the caller's stream, before the side stream takes over; the merged tensor has arg-max keys like a network output."""
        from .parallel import PostStream

        heatmaps_of = self._compute_batch_heatmap
        if flip != "none":  # (resolved once per pass: the default path runs the line it always ran)
            heatmaps_of = lambda pe, dp: self._compute_batch_heatmap_flip(pe, dp, flip)  # noqa: E731

        if inputs is None:
            inputs = lambda hm, dp: (hm, _lib.argmax_keys_of(hm) if torch.is_tensor(hm) and hm.is_cuda else None, dp)  # noqa: E731
        post, results = PostStream(), []
        with torch.no_grad():
            for dp in data_loader:
                dp = stage(dp)
                args = inputs(heatmaps_of(pose_estimator, dp), dp)
                with post.batch(*args):
                    results.append(body(*args))
        post.join()
        return results

    def _gather_score_tables(self, tables, width):
        """The tail of a scoring pass: the per-batch tables (B, width) -> ``gather_tables``' (per-rank host tables, per-rank
        batch sizes), or None for an empty loader without a collective to take part in."""
        from .parallel import _collectives_on, gather_tables

        sizes = [t.shape[0] for t in tables]
        if not tables:
            if not _collectives_on():
                return None
            # an empty shard still takes part in the pass's collective (the other ranks would hang otherwise)
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
            tables = [torch.zeros((0, width), dtype=torch.float64, device=dev)]
        # the reference's per-sample error behaviour is checked once per pass -- AFTER the collectives (a rank that raised
        # before them would leave the others waiting); the flag travels with the size exchange
        err = None
        try:
            self._raise_deferred_errors()
        except Exception as e:  # noqa: BLE001
            err = e
        gathered = gather_tables(torch.cat(tables, dim=0), sizes, error_flag=int(err is not None))
        if err is not None:
            raise err
        return gathered

    def _compute_sal_dict(self, data_loader, pose_estimator):
        """strategy.py:1004-1147.  Same five OrderedDicts keyed "<pose>-<frame_id>", filled in
        the reference's gather order (batch -> sample -> rank), but with one device->host
        copy and (when torch.distributed is initialised) one all_gather for the whole pass."""
        self._pending_checks = []
        tables = self._pool_loop(data_loader, pose_estimator, lambda hm, _keys, dp: self.score_batch(hm, dp), stage=self._stage_masked,
                                 **self._flip_kwargs("AL"))
        gathered = self._gather_score_tables(tables, 6 + 3 * self.num_joints)
        return _empty_sal_dict() if gathered is None else tables_to_sal_dict(*gathered)

    def _compute_sal_dicts(self, data_loader, pose_estimator, strategies):
        """One pass over the pool for SEVERAL strategies: an OrderedDict strategy -> sal_dict in the order given, each equal
        (values and key order) to ``_compute_sal_dict`` with AL.STRATEGY set to that strategy.  Per batch one network call,
        one heat-map launch, one triangulation; per pass the one size exchange and one gather of ``gather_tables``
        (the table is E columns wider).  Errors of a strategy that was not asked for are not raised."""
        strategies = check_strategies(strategies)
        self._pending_checks = []
        tables = self._pool_loop(data_loader, pose_estimator, lambda hm, _keys, dp: self.score_batch_all(hm, dp, strategies),
                                 stage=self._stage_masked, **self._flip_kwargs("AL"))
        gathered = self._gather_score_tables(tables, 6 + 3 * self.num_joints + len(strategies))
        if gathered is None:
            return OrderedDict((s, _empty_sal_dict()) for s in strategies)
        split = split_strategy_tables(gathered[0], len(strategies))
        return OrderedDict((s, tables_to_sal_dict(tabs, gathered[1])) for s, tabs in zip(strategies, split))


    def _raise_deferred_errors(self):
        """Error behaviour of the reference's per-sample loop, checked once per pass."""
        for kind, t, valid in self._pending_checks:
            if kind == "INLIER":
                bad = t[t < 0]
                if bad.numel():  # the reference stops at its first bad frame
                    if int(bad[0].item()) == -2:  # fewer than two present views (view_valid), or no used joint (view_joint_valid)
                        raise AssertionError("need at least two views")
                    raise ValueError("zero-size array to reduction operation minimum which has no identity")
            else:
                if bool((t < 0).any().item()):
                    raise _lib.MvalError("peak list overflow (> 2048 local maxima in one heat-map)")
                if kind == "BSB" and bool(((t < 2) & valid.bool()[:, None, :]).any().item()):
                    raise IndexError("list index out of range")
        self._pending_checks = []

    # ---- the CLUSTER pass (strategy.py:137-191) -----------------------------------------------------------------------
    @staticmethod
    def _batch_guid_ids(dp):
        """A batch's ``pose`` and ``frame_id`` as (B,) tensors; each arrives as (B,) or (B, 1)."""
        ids = []
        for k in ("pose", "frame_id"):
            t = torch.as_tensor(dp[k])
            if t.dim() > 2 or (t.dim() == 2 and t.shape[1] != 1):
                raise ValueError("cluster pass: %s must be (B,) or (B, 1), got %s" % (k, tuple(t.shape)))
            ids.append(t.reshape(-1))
        if ids[0].shape != ids[1].shape:
            raise ValueError("cluster pass: %d poses for %d frame ids" % (ids[0].shape[0], ids[1].shape[0]))
        return ids

    @staticmethod
    def _stage_cluster_targets(dp):
        """``_stage_batch`` plus the LOSS pass's target -- ``gt_heatmap`` where the batch has it, else ``2d_keypoints`` -- on
        the device, uploaded like the small tensors: pinned, non-blocking, on the caller's stream before the network."""
        out = _stage_batch(dp)
        key = "gt_heatmap" if "gt_heatmap" in dp else "2d_keypoints"
        if key in dp and torch.cuda.is_available():
            out = dict(out)
            out[key] = _stage_small(torch.as_tensor(dp[key]))
        return out

    def _frame_losses(self, heatmaps, dp):
        """The device stage of the LOSS pass: heatmaps (B*V, J, h, w) -> (B,) float32, frame b's
        ``pose_2d_mse_single_batch(heatmaps[b], gt_heatmap[b])`` (strategy.py:182-187) for the whole batch in two launches.
        Against ``gt_heatmap`` (B, V, J, h, w) where the batch carries it (the reference's loader); otherwise against the
        maps of ``2d_keypoints / POSE_ESTIMATOR.STRIDE`` with DATA.SIGMA (what ``prepare_views`` renders), not materialised."""
        cfg = self.al_cfg
        b = self._batch_guid_ids(dp)[0].shape[0]
        _, j, hh, wh = heatmaps.shape
        hm = heatmaps.reshape(b, -1, j, hh, wh)
        if "gt_heatmap" in dp:
            return self.loss.pose_2d_mse_per_frame(hm, torch.as_tensor(dp["gt_heatmap"]).to(hm.device).reshape(hm.shape))
        if "2d_keypoints" not in dp:
            raise KeyError("cluster pass (LOSS): a batch needs 'gt_heatmap' or '2d_keypoints'")
        pt = torch.as_tensor(dp["2d_keypoints"]).to(hm.device).to(torch.float64).reshape(b, -1, j, 2) / cfg.POSE_ESTIMATOR.STRIDE
        return self.loss.pose_2d_mse_per_frame_from_points(hm, pt, cfg.DATA.SIGMA)

    def cluster_dict(self, data_loader, pose_estimator=None, cluster_type=None):
        """The dict of the reference's ``cluster()`` (strategy.py:161-189), keyed "<pose>-<frame_id>" like ``sal_dict``:
        "POSE" -> ``data["3d_keypoints"][idx].tolist()``, the (>= 3, J) poses ``read_cluster_features`` reads (no network,
        no device work); "LOSS" -> the frame's heat-map loss under ``pose_estimator`` as a python float.  ``cluster_type``
        defaults to AL.CLUSTER.TYPE.  A batch's loss runs beside the next batch's network and nothing is copied to the host
        inside the loop; the pass ends with the one size exchange and one packed gather of ``gather_tables`` (rows
        [pose, frame_id, loss] or [pose, frame_id, rows * J values]), rebuilt in ``reference_gather_order``, so every rank
        returns the same dict -- in dataset order under strided shards."""
        from .config import cluster_type as _cluster_type
        from .parallel import _collectives_on, gather_tables, reference_gather_order

        kind = _cluster_type(self.al_cfg.AL.CLUSTER.TYPE if cluster_type is None else cluster_type)
        tables, sizes, j = [], [], 0
        if kind == "POSE":
            for dp in data_loader:
                pose, frame = self._batch_guid_ids(dp)
                kp = torch.as_tensor(dp["3d_keypoints"]).cpu()
                j = int(kp.shape[-1])
                tables.append(torch.cat([pose.cpu().to(torch.float64)[:, None], frame.cpu().to(torch.float64)[:, None],
                                         kp.to(torch.float64).reshape(pose.shape[0], -1)], dim=1))
                sizes.append(pose.shape[0])
        else:
            def loss_rows(heatmaps, dp):
                loss = self._frame_losses(heatmaps, dp)
                pose, frame = self._batch_guid_ids(dp)
                return torch.stack([pose.to(loss.device, torch.float64), frame.to(loss.device, torch.float64), loss.to(torch.float64)], dim=1)

            tables = self._pool_loop(data_loader, pose_estimator, loss_rows, inputs=lambda hm, dp: (hm, dp), stage=self._stage_cluster_targets)
            sizes = [t.shape[0] for t in tables]
        # rows travel flattened with [row width, J] in front of the batch sizes: a rank with an empty shard does not know the
        # width of the others' rows (POSE: rows * J) and still takes part in the collectives
        width = tables[0].shape[1] if tables else 3
        if tables:
            local = torch.cat(tables, dim=0).reshape(-1)
        else:
            on_device = kind == "LOSS" and torch.cuda.is_available()
            local = torch.zeros((0,), dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()) if on_device else "cpu")
        if _collectives_on() and not local.is_cuda and torch.distributed.get_backend() == "nccl":
            local = local.to(torch.device("cuda", torch.cuda.current_device()))  # (POSE rows are host data; RCCL gathers device tensors)
        per_rank, heads = gather_tables(local, [width, j] + sizes)
        per_rank = [np.asarray(t).reshape(-1, h[0]) for t, h in zip(per_rank, heads)]
        out = OrderedDict()
        for r, row in reference_gather_order([h[2:] for h in heads]):
            e = per_rank[r][row]
            guid = "%s-%s" % (int(e[0]), int(e[1]))
            out[guid] = float(e[2]) if kind == "LOSS" else e[2:].reshape(-1, heads[r][1]).tolist()
        return out

    def cluster(self, pose_estimator, data_loader, rank=0):
        """The reference's ``cluster()`` (strategy.py:137-191) over a loader: eval mode, for LOSS with a non-empty
        AL.CLUSTER.RESTORE_FROM that checkpoint restored first, ``cluster_dict``, and on rank 0 the dict written to
        AL.CLUSTER.SAVE_PATH (``experiment_io.write_cluster_file``).  Returns the dict (the same on every rank)."""
        from .config import cluster_type as _cluster_type
        from .utils import experiment_io

        c = self.al_cfg.AL.CLUSTER
        kind = _cluster_type(c.TYPE)
        if not c.SAVE_PATH:
            raise ValueError("AL.CLUSTER.SAVE_PATH is empty: cluster() has nowhere to write")
        if pose_estimator is not None and hasattr(pose_estimator, "eval"):
            pose_estimator.eval()
        if kind == "LOSS" and c.RESTORE_FROM != "":
            experiment_io.restore_checkpoint(c.RESTORE_FROM, pose_estimator)
        out = self.cluster_dict(data_loader, pose_estimator, kind)
        if rank == 0:
            experiment_io.write_cluster_file(c.SAVE_PATH, out)
        return out

    def select_al_guids(self, sal_dict, al_num_frames, labeled_dict=None, metric=None):
        """Selection part of _sal_pseudo_labeling (strategy.py:932-949): NaN filter, then
        CORESET -> CoreSet(pred_3d_keypoints, labeled, root, metric).select_batch(N), else
        heapq.nlargest(N, ...) (stable: ties keep gather order).  ``metric`` None reads
        AL.CORESET_METRIC where the config has it ("euclidean", what the reference always uses, otherwise); every rank
        runs the same greedy loop on the gathered predictions, so the metric needs no collective of its own."""
        al_metric_dict = {g: m for g, m in sal_dict["al_metric"].items() if not math.isnan(m)}
        if self.al_cfg.AL.STRATEGY == "CORESET":
            if metric is None:
                metric = self.al_cfg.AL.CORESET_METRIC if "CORESET_METRIC" in self.al_cfg.AL else "euclidean"
            cs = coreset.CoreSet(sal_dict["pred_3d_keypoints"], labeled_dict, self.joint_root_index, metric=metric)
            return cs.select_batch(al_num_frames)
        return nlargest(al_num_frames, al_metric_dict, key=al_metric_dict.get)

    def select_sal_guids(self, sal_dict, al_guids, pseudo_label_guids, pseudo_num_frames, kmeans_centers=None,
                         device=None):
        """Pseudo-label filter of _sal_pseudo_labeling (strategy.py:952-1001): keep frames that were not
        sampled by AL, are not pseudo-labelled yet, have a finite sal_metric and MORE than SAL.INLIER_THRESHOLD
        inliers; sort ascending by sal_metric (stable); then either fill SAL.NUM_CLUSTERS pose clusters with
        pseudo_num_frames // NUM_CLUSTERS frames each (cluster of a frame = nearest of ``kmeans_centers``,
        (K, 3J) float64 or a fitted ``utils.kmeans.KMeans`` such as ``self.kmeans``, to its root-relative pose -- ONE device launch for all candidates instead of a
        ``kmeans.predict`` per frame) or, without clusters, ``random.sample`` of the best 2 N (python's
        global RNG, exactly like the reference)."""
        al = set(al_guids)
        done = set(pseudo_label_guids)
        thr = self.al_cfg.SAL.INLIER_THRESHOLD
        sal_metric_dict = {
            g: m for g, m in sal_dict["sal_metric"].items()
            if g not in al and not math.isnan(m) and g not in done and sal_dict["inlier_count"][g] > thr
        }
        sal_guids = sorted(sal_metric_dict, key=sal_metric_dict.get)
        if kmeans_centers is None:
            return random.sample(sal_guids[: 2 * pseudo_num_frames], pseudo_num_frames)
        k = self.al_cfg.SAL.NUM_CLUSTERS
        if not sal_guids:
            return []
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        pose = torch.as_tensor(np.asarray([sal_dict["pred_3d_keypoints"][g] for g in sal_guids], dtype=np.float64)).to(device)
        n, j, rows = pose.shape
        feat = _lib.coreset_features(pose.contiguous(), self.joint_root_index, n, j, rows)
        if hasattr(kmeans_centers, "cluster_centers_"):  # a fitted KMeans (utils/kmeans.py, e.g. ``self.kmeans``)
            kmeans_centers = kmeans_centers.cluster_centers_
        centers = torch.as_tensor(np.asarray(kmeans_centers, dtype=np.float64)).to(device).contiguous()
        labels = _lib.nearest_center(feat, centers).cpu().tolist()
        counter = [0] * k
        per_cluster_count = pseudo_num_frames // k
        out = []
        for g, c in zip(sal_guids, labels):
            if counter[c] < per_cluster_count:
                counter[c] += 1
                out.append(g)
        return out

    # ---- evaluation core (strategy.py:597-636) ----------------------------------------
    def evaluate_mkpe(self, data_loader, pose_estimator):
        """_evaluate_all's MKPE path: heat-maps -> hard arg-max triangulation -> MPJPE over the
        whole loader (one size exchange + one packed data gather instead of 3 all_gathers per sample).  A batch with a
        per-(view, joint) mask (``_view_joint_valid``) is triangulated joint by joint from the views that have the joint, and the
        validity column it contributes is ``joint_valid & joint_used``: a joint nobody triangulated is left out.
        EVAL.DECODE_REFINE "quarter" | "taylor": the sub-pixel decode of ``triangulate_batch(refine=...)``.
        EVAL.REFINE_3D "lm" (with EVAL.REFINE_3D_WEIGHTS "none" | "conf"): the 3-D refinement of ``triangulate_batch(refine_3d=...)``
        (DESIGN.md 6.5); MKPE and the 3-D PCK(h) figures of ``evaluate_all`` then come from the refined points.
        EVAL.UNDISTORT "brown": the undistortion of ``triangulate_batch(undistort=...)`` with the batch's ``intrinsics`` and
        ``distortion`` (KeyError when a batch lacks them).
        EVAL.TRIANGULATION_WEIGHTS "conf" (needs EVAL.DECODE_REFINE): the confidence-weighted triangulation of
        ``triangulate_batch(weights="conf")``; the validity column is then ``joint_valid & joint_used`` too.
        EVAL.FLIP_TEST "mirror" | "mirror_shift": the heat-maps are the flip-test average of two forwards."""
        from .config import check_decode_refine, check_refine_3d, check_triangulation_weights, check_undistort

        ev = self.al_cfg.EVAL
        undistort = check_undistort(ev.UNDISTORT if "UNDISTORT" in ev else "none")
        refine = check_decode_refine(ev.DECODE_REFINE if "DECODE_REFINE" in ev else "none")
        refine_3d, weights_3d = check_refine_3d(ev.REFINE_3D if "REFINE_3D" in ev else "none",
                                                ev.REFINE_3D_WEIGHTS if "REFINE_3D_WEIGHTS" in ev else "none", refine)
        refined = {} if refine == "none" else {"refine": refine}
        if refine_3d != "none":
            refined.update(refine_3d=refine_3d, refine_3d_weights=None if weights_3d == "none" else weights_3d)
        tri_weights = check_triangulation_weights(ev.TRIANGULATION_WEIGHTS if "TRIANGULATION_WEIGHTS" in ev else "none", refine)
        if tri_weights != "none":
            refined.update(weights=tri_weights)

        def inputs(hm, dp):
            b = torch.as_tensor(dp["pose"]).reshape(-1).shape[0] if "pose" in dp else dp["images"].shape[0]
            jv = torch.as_tensor(dp["joint_valid"]).reshape(b, hm.shape[1])
            return hm, _lib.argmax_keys_of(hm) if hm.is_cuda else None, dp, jv

        def triangulate(hm, _keys, dp, jv):  # (decode + triangulation of a batch beside the next batch's network)
            (b, j), (hh, wh) = jv.shape, hm.shape[2:]
            hm5 = hm.reshape(b, -1, j, hh, wh)
            vj, vj_host = self._view_joint_valid(hm5, dp)
            cameras = {} if undistort == "none" else dict(undistort=undistort, **self._batch_cameras(dp, b))
            r = triangulation.triangulate_batch(hm5, dp["proj_matrices"],
                                                self.al_cfg.POSE_ESTIMATOR.STRIDE, jv, pair_rng=random,
                                                valid_joints_host=dp.get("joint_valid_host"),
                                                view_valid=dp.get("view_valid"), view_valid_host=dp.get("view_valid_host"),
                                                view_joint_valid=vj, view_joint_valid_host=vj_host, **refined, **cameras)
            scored = jv.to(hm.device, torch.float32)
            if vj is not None or tri_weights != "none":
                scored = ((scored != 0) & r["joint_used"].bool()).to(torch.float32)
            return (r["keypoints_3d"].to(torch.float32), torch.as_tensor(dp["3d_keypoints"]).to(hm.device, torch.float32), scored)

        rows = self._pool_loop(data_loader, pose_estimator, triangulate, inputs, stage=self._stage_masked, **self._flip_kwargs("EVAL"))
        preds, gts, valids = ([r[k] for r in rows] for k in range(3))
        sizes = [p.shape[0] for p in preds]
        from .parallel import all_gather_reference_order as gather

        j = self.num_joints if not preds else preds[0].shape[1]
        rows = 3 if not gts else gts[0].shape[1]
        if preds:
            # ONE packed table per pass: [pred 3J | gt rows*J | valid J] per sample
            local = torch.cat([torch.cat(preds).reshape(-1, 3 * j), torch.cat(gts).reshape(-1, rows * j),
                               torch.cat(valids).reshape(-1, j)], dim=1)
        else:  # an empty shard still takes part in the collective
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
            local = torch.zeros((0, (4 + rows) * j), dtype=torch.float32, device=dev)
        # the reference appends its per-sample all_gathers batch by batch, sample by sample, rank by rank
        # (strategy.py:600-636): same row order here, so the float32 sample-order sums of compute_mkpe match
        table = gather(local, sizes)
        pred = table[:, : 3 * j].reshape(-1, j, 3)
        gt = table[:, 3 * j : (3 + rows) * j].reshape(-1, rows, j)
        valid = table[:, (3 + rows) * j :]
        out, _ = _lib.mkpe(pred.contiguous(), gt.contiguous(), valid.contiguous(), pred.shape[0], pred.shape[1], gt.shape[1])
        self._eval_tables = (pred, gt, valid)
        return out

    def evaluate_all(self, data_loader, pose_estimator):
        """_evaluate_all (strategy.py:584-649): MKPE + 3-D PCK at 1..5 mm (+ PCKh for panoptic data) over the
        whole loader; returns the reference's result dict."""
        mkpe = self.evaluate_mkpe(data_loader, pose_estimator)
        pred, gt, valid = self._eval_tables
        j = pred.shape[1]
        thresholds, pcks = evaluation.compute_3d_pck_figure(pred, gt, valid, j)
        results = {"mkpe": mkpe.item(), "thresholds": thresholds, "pcks": pcks}
        if self.al_cfg.DATA.TYPE == "panoptic":
            t, p = evaluation.compute_3d_pckh_figure(pred, gt, j)
            results["pckh_thresholds"], results["pckh_pcks"] = t, p
        return results

    # ---- 2-D PCKh (strategy.py:548-582, 784-789) ----------------------------------------------------------------------
    def _compute_pred_labels(self, pose_estimator, data, heatmaps):
        """strategy.py:784-789: the batch's box-scaled hard arg-max key-points, boxes from ``data["square_box"]`` reshaped to
        (-1, 4) -- as ONE (N, J, 2) float32 HIP tensor from one launch (the reference returns N x J pairs of 0-d tensors).
        Decoded from the arg-max keys the network kept for ``heatmaps`` where it did (no second read of the maps), from the
        maps otherwise."""
        boxes = torch.as_tensor(data["square_box"]).to(heatmaps.device).reshape(-1, 4)
        keys = _lib.argmax_keys_of(heatmaps) if heatmaps.is_cuda and _lib.epilogue_decode_enabled() else None
        if keys is not None and tuple(keys.shape) != (heatmaps.shape[0], _lib.ARGMAX_SLOTS, heatmaps.shape[1]):
            keys = None  # (kept for another factorisation of the maps: see _lib.argmax_decode)
        return evaluation.pred_coordinates_batch(heatmaps, boxes, keys)[:, : self.num_joints]

    @staticmethod
    def _stage_pckh_targets(dp):
        """``_stage_batch`` plus what the 2-D PCKh pass reads -- ``square_box`` and ``2d_after_crop`` -- on the device, uploaded
        like the small tensors: pinned, non-blocking, on the caller's stream before the network.  With ``view_valid`` also
        ``view_rows``, the row numbers of the present images."""
        out = _stage_batch(dp)
        if torch.cuda.is_available() and isinstance(dp, dict):
            out = dict(out)
            for key in ("square_box", "2d_after_crop"):
                if key in dp:
                    out[key] = _stage_small(torch.as_tensor(dp[key]))
            if dp.get("view_valid") is not None:
                # frames with missing views: the rows of the present images, listed on the host from the loader's mask
                # (``view_valid_host``, or the caller's own host copy under that key) and uploaded with the rest.  Only a mask
                # that exists on the device alone is read back, which blocks the host on the current stream
                host = out.get("view_valid_host", dp["view_valid"])
                out["view_rows"] = _stage_small(torch.nonzero(torch.as_tensor(host).reshape(-1) != 0).reshape(-1))
        return out

    def evaluate_2d_pckh(self, data_loader, pose_estimator, thresholds=None):
        """_evaluate_2d_pckh (strategy.py:548-582): PCKh of the 2-D network itself, per view, over the whole loader ->
        (thresholds, pcks), ``thresholds`` defaulting to the reference's 0.1 .. 1.0.  Per batch one decode launch beside the
        next batch's network; per pass ONE packed gather of [pred 2J | gt 2J] float32 rows (the reference: two all_gathers
        per batch) and one counter launch for all thresholds.  The ground truth is ``2d_after_crop`` reshaped to
        (-1, J, 2) with J = DATA.NUM_JOINTS, where the reference hard-codes 19 (strategy.py:567).  The gathered tables stay
        in ``self._eval2d_tables``.  A batch with ``view_valid`` (B, V) contributes the rows of its present images only."""
        j = self.num_joints

        def decode(hm, _keys, dp):
            pred = self._compute_pred_labels(pose_estimator, dp, hm)
            gt = torch.as_tensor(dp["2d_after_crop"]).to(hm.device, torch.float32).reshape(-1, j, 2)
            if pred.shape != gt.shape:
                raise ValueError("2-D PCKh: %s predictions for %s ground-truth key-points" % (tuple(pred.shape), tuple(gt.shape)))
            rows = torch.cat([pred.reshape(-1, 2 * j), gt.reshape(-1, 2 * j)], dim=1)
            if dp.get("view_rows") is not None:  # the images of absent views are not scored: S counts present images
                rows = rows.index_select(0, dp["view_rows"])
            return rows

        rows = self._pool_loop(data_loader, pose_estimator, decode, stage=self._stage_pckh_targets, **self._flip_kwargs("EVAL"))
        from .parallel import all_gather_reference_order as gather

        if rows:
            local = torch.cat(rows)
        else:  # an empty shard still takes part in the collective
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
            local = torch.zeros((0, 4 * j), dtype=torch.float32, device=dev)
        table = gather(local, [r.shape[0] for r in rows])
        pred, gt = table[:, : 2 * j].reshape(-1, j, 2), table[:, 2 * j :].reshape(-1, j, 2)
        self._eval2d_tables = (pred, gt)
        return evaluation.compute_pckh_figure(pred, gt, j, evaluation.PCKH_THRESHOLDS if thresholds is None else thresholds)

    def evaluate(self, data_loader, pose_estimator, metric=None):
        """The evaluation EVAL.METRIC names (``metric`` overrides it; config.EVAL_METRICS): a dict with "metric",
        "thresholds" and "pcks", plus "mkpe" whenever the 3-D pass ran --
          "2DPCKH"  ``evaluate_2d_pckh``
          "3DPCK"   ``evaluate_mkpe``, then 3-D PCK at 1..5 mm over valid joints (``evaluate_all``'s "pcks")
          "3DPCKH"  ``evaluate_mkpe``, then 3-D PCKh at 0.1..1.0 (``evaluate_all``'s "pckh_pcks")
          "MKPE"    ``evaluate_mkpe`` only; thresholds and pcks are None."""
        from .config import check_eval_metric

        metric = check_eval_metric(self.al_cfg.EVAL.METRIC if metric is None else metric)
        if metric == "2DPCKH":
            thresholds, pcks = self.evaluate_2d_pckh(data_loader, pose_estimator)
            return {"metric": metric, "thresholds": thresholds, "pcks": pcks}
        mkpe = self.evaluate_mkpe(data_loader, pose_estimator)
        pred, gt, valid = self._eval_tables
        thresholds = pcks = None
        if metric == "3DPCK":
            thresholds, pcks = evaluation.compute_3d_pck_figure(pred, gt, valid, pred.shape[1])
        elif metric == "3DPCKH":
            thresholds, pcks = evaluation.compute_3d_pckh_figure(pred, gt, pred.shape[1])
        return {"metric": metric, "thresholds": thresholds, "pcks": pcks, "mkpe": mkpe.item()}

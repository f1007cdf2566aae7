"""Experiment configuration tree with the reference's field names and defaults
(config.py:14-106, dataset/config.py:10-51).  Only the hot-path knobs are consumed by
this package: POSE_ESTIMATOR.{TYPE,STRIDE,HRNET.*}, DATA.{NUM_JOINTS,INPUT_WIDTH,
INPUT_HEIGHT,TYPE}, AL.{STRATEGY,USE_SOFTARGMAX,USE_REPROJECTION_XE,REPROJECTION_SIGMA,
MPE_CONFIG,HP_CONFIG,BSB_CONFIG,ITER_AMOUNT,INFERENCE.BATCH_SIZE}, TRAIN.{BATCH_SIZE,
LOSS_CLIP_VALUE,OPTIM.*}, NUM_GPUS; the rest is carried so that a reference YAML merges."""
from .cfgnode import CfgNode as CN
from .pose_estimators.config import get_default_configs as _pose_defaults


def _data_defaults():
    d = CN()
    d.INPUT_WIDTH = 256
    d.INPUT_HEIGHT = 256
    d.SCALE_BBOX = 1.0
    d.SIGMA = 1.0
    d.PSEUDO_LABEL_SIGMA = 1.0
    d.TYPE = "panoptic"  # or "ih26m"
    d.EPOCH_SIZE = 2000
    d.NUM_JOINTS = 19  # 42 for ih26m
    d.NUM_AUG = 0
    d.AUG_MAGNITUDE = 0
    d.USE_ROTATION = True
    d.USE_IMAGE_AUG = True
    d.USE_CONST_AUG_MAGNITUDE = True
    d.ROTATE_TARGETS = "none"  # not in the reference (its Rotate drops the rotated heat-maps): utils.augmentation.ROTATE_TARGETS
    # not in the reference (which has no flip test): the left/right joint pairs [[a, b], ...] of the skeleton for (AL|EVAL).FLIP_TEST;
    # empty = the default of DATA.TYPE (utils.flip_test.flip_pairs)
    d.FLIP_PAIRS = []
    return d


def get_default_configs():
    c = CN()
    c.EXPR_NAME = "EXPR"
    c.EXPR_TYPE = "SUPERVISED"
    c.COMMENT = "N/A"
    c.RANDOM_SEED = 1307
    c.NUM_GPUS = 1

    c.SAL = CN()
    c.SAL.NUM_FRAMES = [0, 20, 20, 30, 30, 40, 40, 50, 50, 50]
    c.SAL.INLIER_THRESHOLD = 7
    c.SAL.CLUSTER_FILE_PATH = ""
    c.SAL.NUM_CLUSTERS = 10

    c.AL = CN()
    c.AL.STRATEGY = "RANDOM"  # HP | BSB | RANDOM | MPE | TRIANGULATION | CORESET
    c.AL.INITIAL_AMOUNT = 200
    c.AL.ITER_AMOUNT = 100
    c.AL.START_ITER = 0
    c.AL.ITERATIONS = 10
    c.AL.USE_SOFTARGMAX = False
    c.AL.USE_REPROJECTION_XE = False
    c.AL.REPROJECTION_SIGMA = 1.0
    c.AL.MPE_CONFIG = "AVG"
    c.AL.BSB_CONFIG = "AVG"
    c.AL.HP_CONFIG = "AVG"
    c.AL.CORESET_METRIC = "euclidean"  # not in the reference (it never passes another): the names of _lib.KC_METRIC_IDS
    # not in the reference (which has no per-(view, joint) visibility in its post stage): check_view_joint_valid below.  With both at
    # their defaults only a batch's own "view_joint_valid" key masks anything
    c.AL.VIEW_JOINT_VALID_KEY = ""  # a batch key whose (B, V, J) tensor is the visibility mask, e.g. "per_view_joint_valid"
    c.AL.MIN_PEAK = 0.0  # > 0: a (view, joint) entry also needs a heat-map value >= this (utils.triangulation.peak_mask)
    # not in the reference (which decodes to whole heat-map pixels): the sub-pixel decode of the pool-scoring passes, "none" |
    # "quarter" | "taylor" (check_decode_refine below); not together with USE_SOFTARGMAX
    c.AL.DECODE_REFINE = "none"
    # not in the reference (whose direct_optimization has no defined result): the 3-D refinement of every triangulated joint in the
    # pool-scoring passes, "none" | "lm", and its weights, "none" | "conf" (the peak heights of DECODE_REFINE); check_refine_3d
    # below, DESIGN.md 6.5
    c.AL.REFINE_3D = "none"
    c.AL.REFINE_3D_WEIGHTS = "none"
    # not in the reference (whose post stage takes the distorted peaks for pinhole observations): the undistortion of the decoded
    # key-points before the triangulation of the pool-scoring passes, "none" | "brown"; the batch then carries "intrinsics" and
    # "distortion" (check_undistort below); not together with USE_REPROJECTION_XE
    c.AL.UNDISTORT = "none"
    # not in the reference (whose DLT takes every inlier view at the same weight): per-entry weights inside the triangulation of the
    # pool-scoring passes, "none" | "conf" (the peak heights of DECODE_REFINE); check_triangulation_weights below, DESIGN.md 6.7
    c.AL.TRIANGULATION_WEIGHTS = "none"
    # not in the reference (which runs the network once per image): the flip test of the pool-scoring passes, "none" | "mirror" |
    # "mirror_shift" -- a second forward on the mirrored images, flipped back (and moved one column: HRNet's SHIFT_HEATMAP) and
    # averaged with the first before anything decodes; check_flip_test below, DESIGN.md 6.8
    c.AL.FLIP_TEST = "none"
    c.AL.CLUSTER = CN()  # EXPR_TYPE "CLUSTER" (strategy.py:137-191): what ActiveLearningStrategy.cluster writes
    c.AL.CLUSTER.TYPE = "LOSS"  # LOSS | POSE (cluster_type below)
    c.AL.CLUSTER.SAVE_PATH = ""
    c.AL.CLUSTER.RESTORE_FROM = ""  # not in the reference's config.py, though its cluster() reads it: a checkpoint to restore first (LOSS)
    c.AL.INFERENCE = CN()
    c.AL.INFERENCE.BATCH_SIZE = 2
    c.AL.INFERENCE.NUM_WORKERS = 2

    c.TRAIN = CN()
    c.TRAIN.LOSS_CLIP_VALUE = 10.0
    c.TRAIN.BATCH_SIZE = 2
    c.TRAIN.NUM_WORKERS = 2
    c.TRAIN.LOG_EVERY_ITER = 500
    c.TRAIN.OPTIM = CN()
    c.TRAIN.OPTIM.TOTAL_STEPS = 5000
    c.TRAIN.OPTIM.LR = 0.001
    c.TRAIN.OPTIM.LR_DECAY_STEP_SIZE = 3000
    # not in the reference (whose one loss is the masked MSE): per-joint weights and hard key-point mining of the training loss
    # (check_train_loss, strategy.compose_joint_weights); at these defaults train_step is what it always was
    c.TRAIN.LOSS = CN()
    c.TRAIN.LOSS.JOINT_WEIGHTS = []  # DATA.NUM_JOINTS floats >= 0 (HRNet's USE_DIFFERENT_JOINTS_WEIGHT, squared), or empty: every joint 1
    c.TRAIN.LOSS.OHKM_TOPK = 0  # per image only the OHKM_TOPK joints of the largest weighted loss count (JointsOHKMMSELoss); 0: all
    c.TRAIN.LOSS.PSEUDO_LABEL_WEIGHT = 1.0  # factor on every joint of a frame whose batch entry pseudo_label is nonzero
    c.TRAIN.LOSS.WEIGHT_KEY = ""  # name of a batch key holding (B, V, J) weights >= 0 ("" = none)

    c.EVAL = CN()
    c.EVAL.METRIC = "3DPCK"
    c.EVAL.DECODE_REFINE = "none"  # not in the reference: AL.DECODE_REFINE for evaluate_mkpe / evaluate_all
    c.EVAL.REFINE_3D = "none"  # not in the reference: AL.REFINE_3D / AL.REFINE_3D_WEIGHTS for evaluate_mkpe / evaluate_all
    c.EVAL.REFINE_3D_WEIGHTS = "none"
    c.EVAL.UNDISTORT = "none"  # not in the reference: AL.UNDISTORT for evaluate_mkpe / evaluate_all
    c.EVAL.TRIANGULATION_WEIGHTS = "none"  # not in the reference: AL.TRIANGULATION_WEIGHTS for evaluate_mkpe / evaluate_all
    c.EVAL.FLIP_TEST = "none"  # not in the reference: AL.FLIP_TEST for evaluate_mkpe / evaluate_all / evaluate_2d_pckh / evaluate

    c.POSE_ESTIMATOR = _pose_defaults()
    c.DATA = _data_defaults()
    return c


CLUSTER_TYPES = ("LOSS", "POSE")


def cluster_type(value):
    """A valid AL.CLUSTER.TYPE, or NotImplementedError naming the accepted ones."""
    if value not in CLUSTER_TYPES:
        raise NotImplementedError("AL.CLUSTER.TYPE %r: accepted are %s" % (value, " and ".join(repr(t) for t in CLUSTER_TYPES)))
    return value


EVAL_METRICS = ("2DPCKH", "3DPCK", "3DPCKH", "MKPE")  # the four the reference's EVAL.METRIC comment lists


def check_eval_metric(value):
    """A valid EVAL.METRIC, or NotImplementedError naming the accepted ones."""
    if value not in EVAL_METRICS:
        raise NotImplementedError("EVAL.METRIC %r: accepted are %s" % (value, ", ".join(repr(m) for m in EVAL_METRICS)))
    return value


def check_rotate_targets(value):
    """A valid DATA.ROTATE_TARGETS (utils.augmentation.ROTATE_TARGETS: what RandAugment's Rotate does to the training targets), or ValueError
    naming the accepted ones."""
    from .utils.augmentation import ROTATE_TARGETS

    if value not in ROTATE_TARGETS:
        raise ValueError("DATA.ROTATE_TARGETS %r: accepted are %s" % (value, ", ".join(repr(m) for m in ROTATE_TARGETS)))
    return value


def check_view_joint_valid(key, min_peak):
    """Valid AL.VIEW_JOINT_VALID_KEY (a string; "" = no named key) and AL.MIN_PEAK (a finite number >= 0; 0 = no peak gate), or
    ValueError saying what is accepted.  Returns (key, float(min_peak))."""
    if not isinstance(key, str):
        raise ValueError("AL.VIEW_JOINT_VALID_KEY %r: accepted is a string, the name of a batch key (\"\" for none)" % (key,))
    if isinstance(min_peak, bool) or not isinstance(min_peak, (int, float)) or not 0.0 <= float(min_peak) < float("inf"):
        raise ValueError("AL.MIN_PEAK %r: accepted is a finite number >= 0 (0 switches the peak gate off)" % (min_peak,))
    return key, float(min_peak)


DECODE_REFINES = ("none", "quarter", "taylor")  # "none": the reference's hard arg-max; the others: the names of _lib.REFINE_IDS


def check_decode_refine(value, use_softargmax=False):
    """A valid AL.DECODE_REFINE / EVAL.DECODE_REFINE / ``refine=`` of utils.triangulation, or ValueError naming the accepted ones --
    also for a refinement together with the soft-arg-max (AL.USE_SOFTARGMAX, ``use_soft_argmax``): the refinements start from the
    hard arg-max, the soft-arg-max has none."""
    if not isinstance(value, str) or value not in DECODE_REFINES:
        raise ValueError("decode refinement %r: accepted are %s" % (value, ", ".join(repr(m) for m in DECODE_REFINES)))
    if value != "none" and use_softargmax:
        raise ValueError("decode refinement %r together with the soft-arg-max (AL.USE_SOFTARGMAX / use_soft_argmax): a refinement "
                         "(accepted are %s) starts from the hard arg-max, use one or the other" % (value, ", ".join(repr(m) for m in DECODE_REFINES)))
    return value


REFINE_3DS = ("none", "lm")  # "none": the DLT point of the inlier views; "lm": its reprojection-error minimiser (mval_refine_points_3d)
REFINE_3D_WEIGHTS = ("none", "conf")  # "conf": the peak heights a decode refinement returns (keypoints_conf)


def check_refine_3d(value, weights="none", decode_refine="none"):
    """A valid (AL|EVAL).REFINE_3D / ``refine_3d=`` of utils.triangulation with its (AL|EVAL).REFINE_3D_WEIGHTS / ``refine_3d_weights=``
    (None reads as "none"; a tensor is the caller's own weights and is checked where it is used), or ValueError naming the
    accepted ones -- also for weights without a refinement, and for "conf" without a decode refinement (``decode_refine``
    "none"): only a refined decode returns the confidences.  Returns (value, weights)."""
    if not isinstance(value, str) or value not in REFINE_3DS:
        raise ValueError("3-D refinement %r: accepted are %s" % (value, ", ".join(repr(m) for m in REFINE_3DS)))
    if weights is None:
        weights = "none"
    named = isinstance(weights, str)
    if (named and weights not in REFINE_3D_WEIGHTS) or not (named or hasattr(weights, "shape")):
        raise ValueError("3-D refinement weights %r: accepted are %s (or a (B, V, J) tensor handed to triangulate_batch)"
                         % (weights, ", ".join(repr(m) for m in REFINE_3D_WEIGHTS)))
    if value == "none" and not (named and weights == "none"):
        raise ValueError("3-D refinement weights without a 3-D refinement (accepted are %s): set REFINE_3D / refine_3d to 'lm'"
                         % ", ".join(repr(m) for m in REFINE_3DS))
    if named and weights == "conf" and decode_refine == "none":
        raise ValueError("3-D refinement weights 'conf' need a decode refinement (DECODE_REFINE / refine = 'quarter' | 'taylor'): "
                         "the hard arg-max returns no confidences")
    return value, weights


TRIANGULATION_WEIGHTS = ("none", "conf")  # "none": every inlier view at the same weight; "conf": the peak heights a decode refinement returns


def check_triangulation_weights(value, refine="none"):
    """A valid (AL|EVAL).TRIANGULATION_WEIGHTS / ``weights=`` of utils.triangulation (None reads as "none"; a tensor is the caller's
    own weights and is checked where it is used), or ValueError naming the accepted ones -- also for "conf" without a decode
    refinement (``refine`` "none"): only a refined decode returns the confidences.  Returns the value."""
    if value is None:
        value = "none"
    named = isinstance(value, str)
    if (named and value not in TRIANGULATION_WEIGHTS) or not (named or hasattr(value, "shape")):
        raise ValueError("triangulation weights %r: accepted are %s (or a (B, V, J) tensor handed to triangulate_batch)"
                         % (value, ", ".join(repr(m) for m in TRIANGULATION_WEIGHTS)))
    if named and value == "conf" and refine == "none":
        raise ValueError("triangulation weights 'conf' need a decode refinement (DECODE_REFINE / refine = 'quarter' | 'taylor'): "
                         "the hard arg-max returns no confidences")
    return value


UNDISTORTS = ("none", "brown")  # "none": the decoded peaks as they are; "brown": the inverse of the k1, k2, p1, p2, k3 polynomial (mval_undistort_keypoints)
UNDISTORT_KEYS = ("intrinsics", "distortion")  # what a batch carries under "brown": (B, V, 3, 3) and (B, V, 5) (prepare_views(with_cameras=True))


def check_undistort(value, use_reprojection_xe=False):
    """A valid (AL|EVAL).UNDISTORT / ``undistort=`` of utils.triangulation, or ValueError naming the accepted ones -- also for "brown"
    together with the XE metric (AL.USE_REPROJECTION_XE, ``use_reprojection_xe``): that metric compares a map rendered at the
    pinhole reprojection with the predicted map, whose peaks are at distorted pixels."""
    if not isinstance(value, str) or value not in UNDISTORTS:
        raise ValueError("undistortion %r: accepted are %s" % (value, ", ".join(repr(m) for m in UNDISTORTS)))
    if value != "none" and use_reprojection_xe:
        raise ValueError("undistortion %r together with the XE metric (AL.USE_REPROJECTION_XE / use_reprojection_xe): the rendered map "
                         "sits at the pinhole reprojection and the predicted one at distorted pixels (accepted are %s)"
                         % (value, ", ".join(repr(m) for m in UNDISTORTS)))
    return value


FLIP_TESTS = ("none", "mirror", "mirror_shift")  # "mirror": HRNet's TEST.FLIP_TEST; "mirror_shift": with its TEST.SHIFT_HEATMAP (mval_flip_merge_heatmaps)


def check_flip_test(value):
    """A valid (AL|EVAL).FLIP_TEST / ``mode`` of utils.flip_test, or ValueError naming the accepted ones."""
    if not isinstance(value, str) or value not in FLIP_TESTS:
        raise ValueError("flip test %r: accepted are %s" % (value, ", ".join(repr(m) for m in FLIP_TESTS)))
    return value


def check_train_loss(loss_node, num_joints):
    """A valid TRAIN.LOSS node for ``num_joints`` joints, or ValueError saying what is accepted.  Returns
    (joint_weights: a tuple of num_joints floats or (), ohkm_topk, pseudo_label_weight, weight_key)."""
    jw = loss_node.JOINT_WEIGHTS if "JOINT_WEIGHTS" in loss_node else []
    topk = loss_node.OHKM_TOPK if "OHKM_TOPK" in loss_node else 0
    pw = loss_node.PSEUDO_LABEL_WEIGHT if "PSEUDO_LABEL_WEIGHT" in loss_node else 1.0
    key = loss_node.WEIGHT_KEY if "WEIGHT_KEY" in loss_node else ""

    def weight(x):
        return not isinstance(x, bool) and isinstance(x, (int, float)) and 0.0 <= float(x) < float("inf")

    if not isinstance(jw, (list, tuple)) or len(jw) not in (0, num_joints) or not all(weight(x) for x in jw):
        raise ValueError("TRAIN.LOSS.JOINT_WEIGHTS %r: accepted are %d finite numbers >= 0 (one per joint), or an empty list" % (jw, num_joints))
    if isinstance(topk, bool) or not isinstance(topk, int) or not 0 <= topk <= num_joints:
        raise ValueError("TRAIN.LOSS.OHKM_TOPK %r: accepted is an integer in [0, %d] (0 = every joint counts)" % (topk, num_joints))
    if not weight(pw):
        raise ValueError("TRAIN.LOSS.PSEUDO_LABEL_WEIGHT %r: accepted is a finite number >= 0" % (pw,))
    if not isinstance(key, str):
        raise ValueError("TRAIN.LOSS.WEIGHT_KEY %r: accepted is a string, the name of a batch key (\"\" for none)" % (key,))
    return tuple(float(x) for x in jw), topk, float(pw), key

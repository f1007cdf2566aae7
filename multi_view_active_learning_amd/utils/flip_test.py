"""Flip test (not in the reference): HRNet's and Simple Baselines' TEST.FLIP_TEST / TEST.SHIFT_HEATMAP at inference.

The network runs a second time on the horizontally mirrored batch; its maps are flipped back (columns reversed, left/right
joint channels swapped), under "mirror_shift" moved one column to the right, and averaged with the first output --
``mval_flip_merge_heatmaps``, which also writes the arg-max keys of the averaged maps, so that everything downstream (decode,
statistics, refinement, triangulation) runs on the merged tensor as it runs on a network output.
"""
import torch

from .. import _lib
from ..config import FLIP_TESTS, check_flip_test  # noqa: F401  (FLIP_TESTS: "none" | "mirror" | "mirror_shift")

# the left/right joint pairs of DATA.TYPE's skeleton
_DEFAULT_PAIRS = {
    # CMU Panoptic's 19 joints (0 neck, 1 nose, 2 body centre = the reference's joint_root_index; 3-8 left shoulder, elbow, wrist,
    # hip, knee, ankle; 9-14 the right ones; 15 / 16 left eye / ear, 17 / 18 right eye / ear)
    "panoptic": (19, ((3, 9), (4, 10), (5, 11), (6, 12), (7, 13), (8, 14), (15, 17), (16, 18))),
    # InterHand2.6M's 42 joints: right hand 0-20, left hand 21-41 (root 21)
    "ih26m": (42, tuple((j, j + 21) for j in range(21))),
}


def flip_pairs(data_cfg):
    """The channel of every joint's mirror twin, a list of DATA.NUM_JOINTS ints (a centre joint maps to itself): from
    DATA.FLIP_PAIRS where it is non-empty (a list of [a, b] pairs; joints it does not name map to themselves), else the default of
    DATA.TYPE.  ValueError unless the result is a permutation of range(NUM_JOINTS) that is its own inverse."""
    j = int(data_cfg.NUM_JOINTS)
    given = list(data_cfg.FLIP_PAIRS) if "FLIP_PAIRS" in data_cfg else []
    if given:
        pairs = given
    else:
        if data_cfg.TYPE not in _DEFAULT_PAIRS:
            raise ValueError("flip pairs: no default for DATA.TYPE %r (known are %s): set DATA.FLIP_PAIRS"
                             % (data_cfg.TYPE, ", ".join(repr(t) for t in _DEFAULT_PAIRS)))
        n, pairs = _DEFAULT_PAIRS[data_cfg.TYPE]
        if n != j:
            raise ValueError("flip pairs: the default of DATA.TYPE %r is for %d joints, DATA.NUM_JOINTS is %d: set DATA.FLIP_PAIRS"
                             % (data_cfg.TYPE, n, j))
    table = list(range(j))
    for pair in pairs:
        if len(pair) != 2:
            raise ValueError("flip pairs: %r is not a pair [a, b]" % (pair,))
        a, b = int(pair[0]), int(pair[1])
        if not (0 <= a < j and 0 <= b < j):
            raise ValueError("flip pairs: %r names a joint outside 0..%d" % (list(pair), j - 1))
        if table[a] != a or table[b] != b:
            raise ValueError("flip pairs: %r names a joint that another pair has already" % (list(pair),))
        table[a], table[b] = b, a
    return check_pairs(table, j)


def check_pairs(pairs, num_joints):
    """``pairs`` as a list of ints, or ValueError unless it is a permutation of range(num_joints) that is its own inverse."""
    table = [int(p) for p in pairs]
    if len(table) != num_joints:
        raise ValueError("flip pairs: %d entries for %d joints" % (len(table), num_joints))
    if any(not 0 <= p < num_joints for p in table):
        raise ValueError("flip pairs: an entry outside 0..%d in %r" % (num_joints - 1, table))
    if any(table[p] != i for i, p in enumerate(table)):
        raise ValueError("flip pairs: %r is not its own inverse (pairs[pairs[j]] == j for every joint)" % (table,))
    return table


_PAIRS_DEV = {}  # (device index, tuple of pairs) -> int32 device tensor


def pairs_on_device(pairs, device):
    """The int32 device copy ``mval_flip_merge_heatmaps`` reads, made once per (device, pairs)."""
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), tuple(int(p) for p in pairs))
    t = _PAIRS_DEV.get(key)
    if t is None:
        t = _PAIRS_DEV[key] = torch.tensor(key[1], dtype=torch.int32, device=torch.device("cuda", key[0]))
    return t


def _shift_of(mode):
    mode = check_flip_test(mode)
    if mode == "none":
        raise ValueError("flip test 'none' merges nothing: the caller uses the first forward as it is")
    return mode == "mirror_shift"


def merge_flipped(hm, hm_mirrored, pairs, mode):
    """(N, J, hh, wh) float32 maps of a batch and of its mirror image -> their flip-test average under ``mode`` "mirror" |
    "mirror_shift", with its arg-max keys remembered (``_lib.argmax_keys_of``).  ``pairs``: ``flip_pairs``' list, checked here."""
    shift = _shift_of(mode)
    if hm.dim() != 4:
        raise _lib.MvalError("merge_flipped: heat-maps must be (N, J, hh, wh), got %s" % (tuple(hm.shape),))
    return _lib.flip_merge_heatmaps(hm, hm_mirrored, pairs_on_device(check_pairs(pairs, hm.shape[1]), hm.device), shift)


def flip_test_heatmaps(pose_estimator, images_nchw, pairs, mode):
    """The network on ``images_nchw`` (N, 3, H, W) float32, the mirror, the network on the mirrored batch (the same cached plan:
    every forward returns a tensor of its own) and the merge, all on the current stream -> the merged maps."""
    _shift_of(mode)
    hm = pose_estimator(images_nchw)
    hm_mirrored = pose_estimator(_lib.mirror_images(images_nchw.contiguous()))
    return merge_flipped(hm, hm_mirrored, pairs, mode)

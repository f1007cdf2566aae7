"""Host oracle of the flip test (include/mval_hip.h: mval_mirror_images, mval_flip_merge_heatmaps) in numpy float32:
the mirror, the merge with the add-then-halve order of the entry, and torch.argmax's choice on a map."""
import numpy as np


def mirror(x):
    """Every row of the last dimension reversed (a copy, bit for bit)."""
    return np.ascontiguousarray(np.asarray(x)[..., ::-1])


def merge(hm, hm_mirrored, pairs, shift):
    """(N, J, hh, wh) float32 maps of a batch and of its mirror image -> (hm + f) * 0.5 in float32, one add and then one multiply,
    where f is hm_mirrored flipped back: channel pairs[j], columns reversed and, with ``shift``, moved one column to the right
    (column 0 keeps its own value) -- HRNet's flip_back, then its SHIFT_HEATMAP, then the average."""
    hm, hm_mirrored = np.asarray(hm), np.asarray(hm_mirrored)
    assert hm.dtype == np.float32 and hm_mirrored.dtype == np.float32 and hm.shape == hm_mirrored.shape and hm.ndim == 4
    f = hm_mirrored[:, list(pairs)][..., ::-1].copy()
    if shift:
        f[..., 1:] = f.copy()[..., :-1]
    with np.errstate(invalid="ignore"):  # (inf - inf is a NaN the entry produces as well)
        s = (hm + f).astype(np.float32)
        return (s * np.float32(0.5)).astype(np.float32)


def first_argmax(m):
    """The flat index torch.argmax picks on one map: the first NaN where there is one, else the first of the largest values
    (-0 == +0)."""
    flat = np.asarray(m).reshape(-1)
    nan = np.isnan(flat)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(flat))

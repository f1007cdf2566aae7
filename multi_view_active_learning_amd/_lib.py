"""ctypes binding of the C-ABI shared library ``csrc/libmval_hip.so`` (include/mval_hip.h).

The library is the product: every hot-path entry point of this package ends in one of
these calls.  There is no CPU fallback -- if the library has not been built
(``python -c 'import __graft_entry__ as g; g.build()'``) or an input is not a HIP tensor,
the call raises.  Device pointers are borrowed from torch tensors that the caller keeps
alive; launches go to torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MVAL_LIB_TAG=<tag>: a variant library built by `MVAL_BUILD_TAG=<tag> MVAL_EXTRA_CFLAGS=... python -m ...build` -- measurement A/B only)
LIB_PATH = os.path.join(_HERE, "csrc", "libmval_hip" + ("_" + os.environ["MVAL_LIB_TAG"] if os.environ.get("MVAL_LIB_TAG") else "") + ".so")

_lock = threading.Lock()
_lib = None


class MvalError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raises if it is missing."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise MvalError(
                        f"{LIB_PATH} not found: the HIP extension is not built. "
                        "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                        "There is no CPU fallback for the hot path."
                    )
                l = C.CDLL(LIB_PATH)
                l.mval_last_error.restype = C.c_char_p
                l.mval_kcenter_workspace_bytes.restype = C.c_size_t
                l.mval_frame_loss_workspace_bytes.restype = C.c_size_t
                l.mval_weighted_mse_workspace_bytes.restype = C.c_size_t
                l.mval_kmeans_workspace_bytes.restype = C.c_size_t
                l.mval_net_create.restype = C.c_void_p
                l.mval_packed_weight_floats.restype = C.c_size_t
                l.mval_op_flops.restype = C.c_double
                _lib = l
    return _lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = lib().mval_last_error()
        raise MvalError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_device(*tensors):
    """Launches go to the CURRENT device's current stream: every tensor of a call must live there (a tensor on
    another GPU would be addressed from the wrong device's stream)."""
    cur = torch.cuda.current_device()
    for t in tensors:
        if t is not None and torch.is_tensor(t) and t.is_cuda and t.device.index != cur:
            raise MvalError(f"tensor on cuda:{t.device.index} but the current device is cuda:{cur}: "
                            "call torch.cuda.set_device() (one process per GPU) or wrap the call in torch.cuda.device()")


def _p(t):
    """Device pointer of a contiguous HIP tensor (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise MvalError("hot-path tensors must live on the HIP device (no CPU path)")
    if not t.is_contiguous():
        raise MvalError("hot-path tensors must be contiguous")
    _same_device(t)
    return C.c_void_p(t.data_ptr())


def _req(t, dtype, name):
    if t.dtype != dtype:
        raise MvalError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


# --------------------------------------------------------------------------
# keypoint decode / triangulation
# --------------------------------------------------------------------------
# Decode from the heat-map layer's epilogue: a forward whose final kernel kept arg-max keys of every map
# (mval_net_forward_keys) remembers them for the tensor it returned; argmax_decode of THAT tensor (any reshape of it,
# unmodified) then needs no second read of the heat-maps.  MVAL_EPILOGUE_DECODE=0 switches the mechanism off.
ARGMAX_SLOTS = 128  # MVAL_ARGMAX_SLOTS (include/mval_hip.h): partial keys per map
_ARGMAX_KEYS = {}  # id(network output) -> (weak reference to it, keys [n_images, ARGMAX_SLOTS, joints] int64 bit patterns)


def epilogue_decode_enabled():
    return os.environ.get("MVAL_EPILOGUE_DECODE", "1") != "0"


def forget_argmax_keys(t):
    """Drop the remembered keys of a network output: for callers that write into it through its data pointer (any kernel of
    this package launched on it in place) -- torch's version counter, which argmax_keys_of relies on, does not see such writes."""
    base = t._base if t._base is not None else t
    _ARGMAX_KEYS.pop(id(base), None)


def remember_argmax_keys(out, keys):
    k = id(out)
    _ARGMAX_KEYS[k] = (weakref.ref(out, lambda _r, k=k: _ARGMAX_KEYS.pop(k, None)), keys)


def argmax_keys_of(hm):
    """The keys of the network output `hm` is (a full view of), or None: unknown tensor, a slice, or written to since."""
    base = hm._base if hm._base is not None else hm
    e = _ARGMAX_KEYS.get(id(base))
    if e is None or e[0]() is not base:
        return None
    try:
        if base._version != 0:
            return None
    except RuntimeError:  # inference-mode tensors track no version: nothing tells whether the maps were written to since
        return None
    if hm.numel() != base.numel() or hm.data_ptr() != base.data_ptr() or not hm.is_contiguous() or hm.dtype != torch.float32:
        return None
    return e[1]


def argmax_from_keys(keys, valid, b, v, j, stride, split_width):
    out = torch.empty((b, v, j, 2), dtype=torch.int64, device=keys.device)
    _check(
        lib().mval_argmax_from_keys(_p(_req(keys, torch.int64, "argmax keys")), _p(valid), _p(out), C.c_int(b), C.c_int(v), C.c_int(j),
                                    C.c_int(stride), C.c_int(split_width), _stream()),
        "mval_argmax_from_keys",
    )
    return out


def argmax_decode(hm, valid, b, v, j, hh, wh, stride, split_width):
    keys = argmax_keys_of(hm) if epilogue_decode_enabled() else None
    # the keys are laid out [image][slot][joint of the PLAN]: only the caller's factorisation that matches it may use them
    # (b = n * J, v = 1, j = 1 has the same element count and would index them wrongly: ADVICE round 3)
    if keys is not None and tuple(keys.shape) == (b * v, ARGMAX_SLOTS, j) and hm.numel() == b * v * j * hh * wh:
        return argmax_from_keys(keys, valid, b, v, j, stride, split_width)
    out = torch.empty((b, v, j, 2), dtype=torch.int64, device=hm.device)
    _check(
        lib().mval_argmax_decode(
            _p(_req(hm, torch.float32, "heatmaps")), _p(valid), _p(out),
            C.c_int(b), C.c_int(v), C.c_int(j), C.c_int(hh), C.c_int(wh),
            C.c_int(stride), C.c_int(split_width), _stream(),
        ),
        "mval_argmax_decode",
    )
    return out


def pred_coordinates_from_keys(keys, boxes, hh, wh):
    """mval_pred_coordinates_from_keys: keys (N, ARGMAX_SLOTS, J) int64 bit patterns of maps of hh x wh, boxes (N,4) f32 -> xy (N,J,2) f32."""
    if keys.dim() != 3 or keys.shape[1] != ARGMAX_SLOTS or tuple(boxes.shape) != (keys.shape[0], 4):
        raise MvalError(f"pred_coordinates_from_keys: keys (N, {ARGMAX_SLOTS}, J) and boxes (N, 4), got {tuple(keys.shape)} and {tuple(boxes.shape)}")
    n, _, j = keys.shape
    out = torch.empty((n, j, 2), dtype=torch.float32, device=keys.device)
    _check(
        lib().mval_pred_coordinates_from_keys(_p(_req(keys, torch.int64, "argmax keys")), _p(_req(boxes, torch.float32, "boxes")),
                                              _p(out), C.c_longlong(n), C.c_int(j), C.c_int(hh), C.c_int(wh), _stream()),
        "mval_pred_coordinates_from_keys",
    )
    return out


def pred_coordinates(hm, boxes, keys=None):
    """mval_pred_coordinates: hm (N,J,hh,wh) f32, boxes (N,4) f32 (left, top, right, bottom) -> xy (N,J,2) f32, the hard arg-max
    branch of the reference's get_pred_coordinates.  With ``keys`` (N, ARGMAX_SLOTS, J) int64 bit patterns -- the keys the
    network kept for ``hm`` (argmax_keys_of) -- mval_pred_coordinates_from_keys: ``hm`` then only gives the shape and is not read."""
    if hm.dim() != 4:
        raise MvalError(f"pred_coordinates: heat-maps must be (N, J, hh, wh), got {tuple(hm.shape)}")
    n, j, hh, wh = hm.shape
    if tuple(boxes.shape) != (n, 4):
        raise MvalError(f"pred_coordinates: boxes must be ({n}, 4), got {tuple(boxes.shape)}")
    if keys is not None:
        if tuple(keys.shape) != (n, ARGMAX_SLOTS, j):
            raise MvalError(f"pred_coordinates: keys must be ({n}, {ARGMAX_SLOTS}, {j}), got {tuple(keys.shape)}")
        return pred_coordinates_from_keys(keys, boxes, hh, wh)
    out = torch.empty((n, j, 2), dtype=torch.float32, device=hm.device)
    _check(
        lib().mval_pred_coordinates(_p(_req(hm, torch.float32, "heatmaps")), _p(_req(boxes, torch.float32, "boxes")), _p(out),
                                    C.c_longlong(n), C.c_int(j), C.c_int(hh), C.c_int(wh), _stream()),
        "mval_pred_coordinates",
    )
    return out


def soft_argmax(hm, n_maps, hh, wh, scale):
    out = torch.empty((n_maps, 2), dtype=torch.float32, device=hm.device)
    _check(
        lib().mval_soft_argmax(
            _p(_req(hm, torch.float32, "heatmaps")), _p(out), C.c_longlong(n_maps),
            C.c_int(hh), C.c_int(wh), C.c_float(scale), _stream(),
        ),
        "mval_soft_argmax",
    )
    return out


# MVAL_REFINE_* (include/mval_hip.h): the sub-pixel refinements of mval_refine_keypoints, under the names the config uses
REFINE_QUARTER, REFINE_TAYLOR = 1, 2
REFINE_IDS = {"quarter": REFINE_QUARTER, "taylor": REFINE_TAYLOR}


def refine_keypoints(hm, kp2d, valid, b, v, j, hh, wh, stride, method):
    """mval_refine_keypoints: hm (b,v,j,hh,wh) f32, kp2d (b,v,j,2) int64 -- the hard decode made with split_width = wh --,
    valid (b,j) uint8 or None, method a name of REFINE_IDS -> (kp f32 (b,v,j,2), conf f32 (b,v,j))."""
    if not isinstance(method, str) or method not in REFINE_IDS:
        raise MvalError(f"refine_keypoints: method {method!r}: accepted are " + ", ".join(repr(k) for k in REFINE_IDS))
    if tuple(kp2d.shape) != (b, v, j, 2) or hm.numel() != b * v * j * hh * wh:
        raise MvalError(f"refine_keypoints: heat-maps of {b * v * j * hh * wh} elements and kp2d ({b}, {v}, {j}, 2), got "
                        f"{hm.numel()} and {tuple(kp2d.shape)}")
    out = torch.empty((b, v, j, 2), dtype=torch.float32, device=hm.device)
    conf = torch.empty((b, v, j), dtype=torch.float32, device=hm.device)
    _check(
        lib().mval_refine_keypoints(
            C.c_int(REFINE_IDS[method]), _p(_req(hm, torch.float32, "heatmaps")), _p(_req(kp2d, torch.int64, "keypoints_2d")), _p(valid),
            _p(out), _p(conf), C.c_int(b), C.c_int(v), C.c_int(j), C.c_int(hh), C.c_int(wh), C.c_int(int(stride)), _stream(),
        ),
        "mval_refine_keypoints",
    )
    return out, conf


# Presence masks (include/mval_hip.h): the `_masked` entries take (mask, mask_kind) -- nothing, view_valid (B, V) uint8 on the
# device, nonzero = the view is present in that frame, or view_joint_valid (B, V, J) uint8, nonzero = joint j is usable in view
# v of frame b.  The wrappers below take them as keyword arguments and always call the `_masked` entry.
MASK_NONE, MASK_VIEWS, MASK_VIEW_JOINT = 0, 1, 2  # MVAL_MASK_*

# The entries below carry ctypes argtypes, set on first use, where the older wrappers convert every argument by hand
# (C.c_int(b), ...): a masked entry differs from its unmasked sibling by two arguments in the middle of a long list, and with
# argtypes a call that leaves one out fails in ctypes with an argument-count error instead of shifting every later argument.
# The older entries are left as they are.
_VOIDP, _INT, _DOUBLE = C.c_void_p, C.c_int, C.c_double
_VIEWS_ARGTYPES = {
    "mval_triangulate_ransac_masked": [_VOIDP, _INT] + [_VOIDP] * 3 + [_INT] + [_VOIDP] * 5 + [_INT] * 3 + [_DOUBLE, _VOIDP],
    "mval_triangulate_ransac_pairs_masked": [_VOIDP, _INT] + [_VOIDP] * 3 + [_INT, _VOIDP] + [_INT] * 2 + [_VOIDP] * 5 + [_INT] * 3 + [_DOUBLE, _VOIDP],
    "mval_reprojection_xe_masked": [_VOIDP] * 4 + [_INT] + [_VOIDP] * 2 + [_INT] * 5 + [_DOUBLE, _VOIDP],
    "mval_score_reduce_masked": [_VOIDP] * 3 + [_INT, _VOIDP] + [_INT] * 4 + [_VOIDP],
    "mval_peak_mask": [_VOIDP, C.c_float, _VOIDP, C.c_longlong, _INT, _INT, _VOIDP],
}


def _views_entry(name):
    f = getattr(lib(), name)
    if f.argtypes is None:
        f.argtypes, f.restype = _VIEWS_ARGTYPES[name], C.c_int
    return f


def _mask_arg(view_valid, view_joint_valid, b, v, j):
    """(mask, mask_kind) of a `_masked` entry from the wrappers' two keywords, at most one of which is given."""
    if view_valid is not None and view_joint_valid is not None:
        raise MvalError("view_valid or view_joint_valid, not both (AND them into view_joint_valid)")
    if view_joint_valid is not None:
        _req(view_joint_valid, torch.uint8, "view_joint_valid")
        if tuple(view_joint_valid.shape) != (b, v, j):
            raise MvalError(f"view_joint_valid: expected ({b}, {v}, {j}), got {tuple(view_joint_valid.shape)}")
        return view_joint_valid, MASK_VIEW_JOINT
    if view_valid is not None:
        _req(view_valid, torch.uint8, "view_valid")
        if tuple(view_valid.shape) != (b, v):
            raise MvalError(f"view_valid: expected ({b}, {v}), got {tuple(view_valid.shape)}")
        return view_valid, MASK_VIEWS
    return None, MASK_NONE


def _triangulate(entry, kp2d, proj, valid, mask, kind, b, v, j, eps, table=()):
    """What the two triangulation entries share: key-points float32 or int64, the five outputs, the call.  ``table``: the
    arguments an entry takes between the mask and the outputs."""
    kp_is_f32 = 1 if kp2d.dtype == torch.float32 else 0
    if not kp_is_f32:
        _req(kp2d, torch.int64, "keypoints_2d")
    dev = proj.device
    kp3d = torch.empty((b, j, 3), dtype=torch.float64, device=dev)
    jerr = torch.empty((b, j), dtype=torch.float64, device=dev)
    jinl = torch.empty((b, j), dtype=torch.int32, device=dev)
    metric = torch.empty((b,), dtype=torch.float64, device=dev)
    inl = torch.empty((b,), dtype=torch.int32, device=dev)
    _check(
        _views_entry(entry)(
            _p(kp2d), kp_is_f32, _p(_req(proj, torch.float64, "proj_matricies")), _p(valid), _p(mask), kind, *table,
            _p(kp3d), _p(jerr), _p(jinl), _p(metric), _p(inl), b, v, j, eps, _stream(),
        ),
        entry,
    )
    return kp3d, jerr, jinl, metric, inl


PAIRS_MAX_VIEWS = 32  # MVAL_PAIRS_MAX_VIEWS (include/mval_hip.h): views mval_triangulate_ransac_pairs accepts


def triangulate_ransac_pairs(kp2d, proj, valid, pairs, b, v, j, eps, *, view_valid=None, view_joint_valid=None):
    """mval_triangulate_ransac_pairs_masked: pairs (B, J, P, 2) uint8, one table per problem, or (1, P, 2), one shared by all.
    Under a mask the result is over the present views of each frame / problem; the table names original view indices, entries
    >= V (255: padding) or naming an absent view take no part."""
    _req(pairs, torch.uint8, "pairs")
    shared = pairs.dim() == 3
    if pairs.shape[-1] != 2 or (tuple(pairs.shape[:-2]) != (1,) if shared else tuple(pairs.shape[:-2]) != (b, j)):
        raise MvalError(f"pairs: expected (1, P, 2) or ({b}, {j}, P, 2), got {tuple(pairs.shape)}")
    mask, kind = _mask_arg(view_valid, view_joint_valid, b, v, j)
    return _triangulate("mval_triangulate_ransac_pairs_masked", kp2d, proj, valid, mask, kind, b, v, j, eps,
                        table=(_p(pairs), pairs.shape[-2], int(shared)))


def triangulate_ransac(kp2d, proj, valid, b, v, j, eps, *, view_valid=None, view_joint_valid=None):
    """mval_triangulate_ransac_masked (V <= 11); under a mask over the present views of each frame / (frame, joint) problem."""
    mask, kind = _mask_arg(view_valid, view_joint_valid, b, v, j)
    return _triangulate("mval_triangulate_ransac_masked", kp2d, proj, valid, mask, kind, b, v, j, eps)


_VIEWS_ARGTYPES["mval_triangulate_ransac_weighted"] = ([_VOIDP, _INT] + [_VOIDP] * 3 + [_INT, _VOIDP] + [_INT] * 2 + [_VOIDP] * 7 + [_INT] * 3
                                                       + [_DOUBLE, _VOIDP])


def triangulate_ransac_weighted(kp2d, proj, valid, b, v, j, eps, *, pairs=None, view_valid=None, view_joint_valid=None, weights=None,
                                want_inlier_mask=False):
    """mval_triangulate_ransac_weighted: ``triangulate_ransac`` (pairs None, V <= 11) or ``triangulate_ransac_pairs`` with per-entry
    ``weights`` (b, v, j) float32 inside the DLT and the ranking -- an entry whose weight is not finite and > 0 is absent -- and / or
    the winning inlier set handed out -> (kp3d, joint_err, joint_inliers, metric, inlier_count, joint_inlier_mask (b, j) int32 with
    bit v = view v is in the set, or None when not asked for)."""
    mask, kind = _mask_arg(view_valid, view_joint_valid, b, v, j)
    kp_is_f32 = 1 if kp2d.dtype == torch.float32 else 0
    if not kp_is_f32:
        _req(kp2d, torch.int64, "keypoints_2d")
    if tuple(kp2d.shape) != (b, v, j, 2):
        raise MvalError(f"triangulate_ransac_weighted: kp2d ({b}, {v}, {j}, 2), got {tuple(kp2d.shape)}")
    if weights is not None and tuple(_req(weights, torch.float32, "weights").shape) != (b, v, j):
        raise MvalError(f"triangulate_ransac_weighted: weights ({b}, {v}, {j}), got {tuple(weights.shape)}")
    table = (_p(None), 0, 0)
    if pairs is not None:
        _req(pairs, torch.uint8, "pairs")
        shared = pairs.dim() == 3
        if pairs.shape[-1] != 2 or (tuple(pairs.shape[:-2]) != (1,) if shared else tuple(pairs.shape[:-2]) != (b, j)):
            raise MvalError(f"pairs: expected (1, P, 2) or ({b}, {j}, P, 2), got {tuple(pairs.shape)}")
        table = (_p(pairs), pairs.shape[-2], int(shared))
    dev = proj.device
    kp3d = torch.empty((b, j, 3), dtype=torch.float64, device=dev)
    jerr = torch.empty((b, j), dtype=torch.float64, device=dev)
    jinl = torch.empty((b, j), dtype=torch.int32, device=dev)
    jmask = torch.empty((b, j), dtype=torch.int32, device=dev) if want_inlier_mask else None
    metric = torch.empty((b,), dtype=torch.float64, device=dev)
    inl = torch.empty((b,), dtype=torch.int32, device=dev)
    _check(
        _views_entry("mval_triangulate_ransac_weighted")(
            _p(kp2d), kp_is_f32, _p(_req(proj, torch.float64, "proj_matricies")), _p(valid), _p(mask), kind, *table, _p(weights),
            _p(kp3d), _p(jerr), _p(jinl), _p(jmask), _p(metric), _p(inl), b, v, j, float(eps), _stream(),
        ),
        "mval_triangulate_ransac_weighted",
    )
    return kp3d, jerr, jinl, metric, inl, jmask


def peak_mask(hm, min_peak, n_maps, hh, wh):
    """mval_peak_mask: (n_maps,) uint8, 1 where some element of the map is >= min_peak."""
    out = torch.empty((n_maps,), dtype=torch.uint8, device=hm.device)
    _check(
        _views_entry("mval_peak_mask")(_p(_req(hm, torch.float32, "heatmaps")), float(min_peak), _p(out), n_maps, hh, wh, _stream()),
        "mval_peak_mask",
    )
    return out


REFINE3D_MAX_ITERS = 32  # MVAL_REFINE3D_MAX_ITERS
_VIEWS_ARGTYPES["mval_refine_points_3d"] = [_VOIDP, _INT] + [_VOIDP] * 3 + [_INT] + [_VOIDP] * 10 + [_INT] * 3 + [_DOUBLE, _VOIDP]


def refine_points_3d(kp2d, proj, valid, kp3d, joint_err, joint_inliers, b, v, j, eps, view_valid=None, view_joint_valid=None,
                     weights=None):
    """mval_refine_points_3d: the triangulation's kp3d (b,j,3) f64, joint_err (b,j) f64 and joint_inliers (b,j) i32 with the
    inputs it had -- kp2d (b,v,j,2) int64|float32, proj (b,v,3,4) f64, valid (b,j) uint8 or None, at most one of view_valid
    (b,v) / view_joint_valid (b,v,j) uint8 -- and optional weights (b,v,j) float32 ->
    (kp3d refined (b,j,3) f64, joint_err (b,j) f64, joint_support (b,j) i32, joint_status (b,j) i32, metric (b,) f64)."""
    mask, kind = _mask_arg(view_valid, view_joint_valid, b, v, j)
    kp_is_f32 = 1 if kp2d.dtype == torch.float32 else 0
    if not kp_is_f32:
        _req(kp2d, torch.int64, "keypoints_2d")
    if tuple(kp2d.shape) != (b, v, j, 2) or tuple(kp3d.shape) != (b, j, 3) or tuple(joint_err.shape) != (b, j) or tuple(joint_inliers.shape) != (b, j):
        raise MvalError(f"refine_points_3d: kp2d ({b}, {v}, {j}, 2), kp3d ({b}, {j}, 3), joint_err and joint_inliers ({b}, {j}), got "
                        f"{tuple(kp2d.shape)}, {tuple(kp3d.shape)}, {tuple(joint_err.shape)} and {tuple(joint_inliers.shape)}")
    if weights is not None and tuple(_req(weights, torch.float32, "weights").shape) != (b, v, j):
        raise MvalError(f"refine_points_3d: weights ({b}, {v}, {j}), got {tuple(weights.shape)}")
    dev = proj.device
    out = torch.empty((b, j, 3), dtype=torch.float64, device=dev)
    jerr = torch.empty((b, j), dtype=torch.float64, device=dev)
    support = torch.empty((b, j), dtype=torch.int32, device=dev)
    status = torch.empty((b, j), dtype=torch.int32, device=dev)
    metric = torch.empty((b,), dtype=torch.float64, device=dev)
    inl = torch.empty((b,), dtype=torch.int32, device=dev)  # (rewritten with the triangulation's own values)
    _check(
        _views_entry("mval_refine_points_3d")(
            _p(kp2d), kp_is_f32, _p(_req(proj, torch.float64, "proj_matricies")), _p(valid), _p(mask), kind, _p(weights),
            _p(_req(kp3d, torch.float64, "keypoints_3d")), _p(_req(joint_err, torch.float64, "joint_error")),
            _p(_req(joint_inliers, torch.int32, "joint_inliers")), _p(out), _p(jerr), _p(support), _p(status), _p(metric), _p(inl),
            b, v, j, float(eps), _stream(),
        ),
        "mval_refine_points_3d",
    )
    return out, jerr, support, status, metric


UNDISTORT_MAX_ITERS, UNDISTORT_FOLD, UNDISTORT_NOCONV = 16, -1, -2  # MVAL_UNDISTORT_*
_VIEWS_ARGTYPES["mval_undistort_keypoints"] = [_VOIDP, _INT] + [_VOIDP] * 4 + [_INT] + [_VOIDP] * 2 + [_INT] * 3 + [_VOIDP]


def undistort_keypoints(kp2d, K, dist, valid, b, v, j, view_valid=None, view_joint_valid=None):
    """mval_undistort_keypoints: kp2d (b,v,j,2) int64|float32, K (b,v,3,3) f64, dist (b,v,5) f64 = k1, k2, p1, p2, k3, valid (b,j)
    uint8 or None, at most one of view_valid (b,v) / view_joint_valid (b,v,j) uint8 -> (kp f32 (b,v,j,2), status i32 (b,v,j):
    0 not processed or no distortion, k > 0 converged after k iterations, UNDISTORT_FOLD / UNDISTORT_NOCONV handed through)."""
    mask, kind = _mask_arg(view_valid, view_joint_valid, b, v, j)
    kp_is_f32 = 1 if kp2d.dtype == torch.float32 else 0
    if not kp_is_f32:
        _req(kp2d, torch.int64, "keypoints_2d")
    if tuple(kp2d.shape) != (b, v, j, 2) or tuple(K.shape) != (b, v, 3, 3) or tuple(dist.shape) != (b, v, 5):
        raise MvalError(f"undistort_keypoints: kp2d ({b}, {v}, {j}, 2), K ({b}, {v}, 3, 3) and dist ({b}, {v}, 5), got "
                        f"{tuple(kp2d.shape)}, {tuple(K.shape)} and {tuple(dist.shape)}")
    if valid is not None and tuple(_req(valid, torch.uint8, "valid").shape) != (b, j):
        raise MvalError(f"undistort_keypoints: valid ({b}, {j}), got {tuple(valid.shape)}")
    out = torch.empty((b, v, j, 2), dtype=torch.float32, device=kp2d.device)
    status = torch.empty((b, v, j), dtype=torch.int32, device=kp2d.device)
    _check(
        _views_entry("mval_undistort_keypoints")(
            _p(kp2d), kp_is_f32, _p(_req(K, torch.float64, "intrinsics")), _p(_req(dist, torch.float64, "distortion")), _p(valid),
            _p(mask), kind, _p(out), _p(status), b, v, j, _stream(),
        ),
        "mval_undistort_keypoints",
    )
    return out, status


_VIEWS_ARGTYPES["mval_mirror_images"] = [_VOIDP, _VOIDP, C.c_longlong, _INT, _VOIDP]
_VIEWS_ARGTYPES["mval_flip_merge_heatmaps"] = [_VOIDP] * 3 + [_INT] + [_VOIDP] * 2 + [C.c_longlong] + [_INT] * 3 + [_VOIDP]


def mirror_images(x, out=None):
    """mval_mirror_images: a float32 tensor whose last dimension is the image width (an NCHW batch) -> the same with every row
    reversed, bit for bit.  ``out``: a tensor of x's shape to write to (it must not overlap x; arg-max keys remembered for it are
    forgotten), else a new one."""
    if x.dim() < 1:
        raise MvalError("mirror_images: the last dimension is the row, got a 0-d tensor")
    _req(x, torch.float32, "images")
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    elif out.shape != x.shape:
        raise MvalError(f"mirror_images: out must be {tuple(x.shape)}, got {tuple(out.shape)}")
    else:
        forget_argmax_keys(out)
    w = x.shape[-1]
    if w == 0:  # (nothing to copy, and no row length the entry takes)
        return out
    _check(_views_entry("mval_mirror_images")(_p(x), _p(_req(out, torch.float32, "out")), x.numel() // w, w, _stream()), "mval_mirror_images")
    return out


def flip_merge_heatmaps(hm, hm_mirrored, pairs_dev, shift, keep_keys=True, out=None):
    """mval_flip_merge_heatmaps: hm and hm_mirrored (N,J,hh,wh) f32 -- the network on a batch and on its mirror image --,
    pairs_dev (J,) int32 on the device (the channel of each joint's mirror twin), shift: move the flipped-back map one column to
    the right -> merged (N,J,hh,wh) f32 = (hm + flipped-back hm_mirrored) * 0.5.  With ``keep_keys`` the launch also writes the
    arg-max keys of ``merged`` and they are remembered for it (``argmax_keys_of(merged)``), as a forward's are for its output.
    ``out``: a tensor of hm's shape to write to, else a new one.  It must overlap neither input and must be a tensor of its own, not
    a view of another: the keys are remembered per base tensor, and a view's would be found for nothing or for the wrong maps."""
    if hm.dim() != 4 or hm_mirrored.shape != hm.shape:
        raise MvalError(f"flip_merge_heatmaps: two heat-map tensors (N, J, hh, wh) of one shape, got {tuple(hm.shape)} and {tuple(hm_mirrored.shape)}")
    n, j, hh, wh = hm.shape
    if tuple(pairs_dev.shape) != (j,):
        raise MvalError(f"flip_merge_heatmaps: pairs must be ({j},), got {tuple(pairs_dev.shape)}")
    if out is None:
        out = torch.empty_like(hm, memory_format=torch.contiguous_format)
    elif out.shape != hm.shape or out._base is not None:
        raise MvalError(f"flip_merge_heatmaps: out must be a tensor of its own (no view) of shape {tuple(hm.shape)}, got "
                        f"{'a view of ' if out._base is not None else ''}{tuple(out.shape)}")
    keys = torch.empty((n, ARGMAX_SLOTS, j), dtype=torch.int64, device=hm.device) if keep_keys else None
    _check(
        _views_entry("mval_flip_merge_heatmaps")(
            _p(_req(hm, torch.float32, "heatmaps")), _p(_req(hm_mirrored, torch.float32, "mirrored heatmaps")),
            _p(_req(pairs_dev, torch.int32, "pairs")), 1 if shift else 0, _p(_req(out, torch.float32, "out")), _p(keys), n, j, hh, wh, _stream(),
        ),
        "mval_flip_merge_heatmaps",
    )
    if keep_keys:
        remember_argmax_keys(out, keys)
    else:
        forget_argmax_keys(out)
    return out


def reprojection_xe(kp3d, proj, hm, b, v, j, hh, wh, sigma, *, view_valid=None, view_joint_valid=None):
    """mval_reprojection_xe_masked: (b,) float64; under a mask the sum over the present views / entries of each frame."""
    mask, kind = _mask_arg(view_valid, view_joint_valid, b, v, j)
    out = torch.empty((b,), dtype=torch.float64, device=hm.device)
    ws = torch.empty((b * v * j,), dtype=torch.float64, device=hm.device)
    _check(
        _views_entry("mval_reprojection_xe_masked")(
            _p(_req(kp3d, torch.float64, "keypoints_3d")), _p(_req(proj, torch.float64, "proj")),
            _p(_req(hm, torch.float32, "heatmaps")), _p(mask), kind, _p(out), _p(ws), b, v, j, hh, wh, sigma, _stream(),
        ),
        "mval_reprojection_xe_masked",
    )
    return out


# --------------------------------------------------------------------------
# uncertainty scorers
# --------------------------------------------------------------------------
SCORE_HP, SCORE_MPE, SCORE_BSB = 0, 1, 2
REDUCE_AVG_F64, REDUCE_AVG_F32, REDUCE_STD_F64, REDUCE_STD_F32 = 0, 1, 2, 3


def score_maps(kind, hm, n_maps, hh, wh):
    """Per-map statistic (float32) + per-map peak count (int32)."""
    out = torch.empty((n_maps,), dtype=torch.float32, device=hm.device)
    cnt = torch.empty((n_maps,), dtype=torch.int32, device=hm.device)
    _check(
        lib().mval_score_maps(
            C.c_int(kind), _p(_req(hm, torch.float32, "heatmaps")), _p(out), _p(cnt),
            C.c_longlong(n_maps), C.c_int(hh), C.c_int(wh), _stream(),
        ),
        "mval_score_maps",
    )
    return out, cnt


def score_decode_maps(kind, hm, valid, b, v, j, hh, wh, stride, split_width):
    """Per-map statistic + peak count + hard arg-max key-points (B,V,J,2) int64 from ONE read of the heat-maps."""
    n_maps = b * v * j
    out = torch.empty((n_maps,), dtype=torch.float32, device=hm.device)
    cnt = torch.empty((n_maps,), dtype=torch.int32, device=hm.device)
    kp = torch.empty((b, v, j, 2), dtype=torch.int64, device=hm.device)
    _check(
        lib().mval_score_decode_maps(
            C.c_int(kind), _p(_req(hm, torch.float32, "heatmaps")), _p(valid), _p(out), _p(cnt), _p(kp),
            C.c_int(b), C.c_int(v), C.c_int(j), C.c_int(hh), C.c_int(wh), C.c_int(stride), C.c_int(split_width), _stream(),
        ),
        "mval_score_decode_maps",
    )
    return out, cnt, kp


def score_decode_maps_all(hm, valid, b, v, j, hh, wh, stride, split_width, decode=True):
    """HP, MPE and BSB of every map (+ the hard arg-max key-points when ``decode``) from ONE read of the heat-maps:
    (stat (3, n) float32 in SCORE_HP/_MPE/_BSB order, n_peaks (2, n) int32 for MPE and BSB, kp2d (B,V,J,2) int64 or None)."""
    n_maps = b * v * j
    out = torch.empty((3, n_maps), dtype=torch.float32, device=hm.device)
    cnt = torch.empty((2, n_maps), dtype=torch.int32, device=hm.device)
    kp = torch.empty((b, v, j, 2), dtype=torch.int64, device=hm.device) if decode else None
    _check(
        lib().mval_score_decode_maps_all(
            _p(_req(hm, torch.float32, "heatmaps")), _p(valid), _p(out), _p(cnt), _p(kp),
            C.c_int(b), C.c_int(v), C.c_int(j), C.c_int(hh), C.c_int(wh), C.c_int(stride), C.c_int(split_width), _stream(),
        ),
        "mval_score_decode_maps_all",
    )
    return out, cnt, kp


def score_reduce(per_map, valid, b, v, j, mode, *, view_valid=None, view_joint_valid=None):
    """mval_score_reduce_masked: (b,) float64; under a mask over the present views / (view, joint) entries of each frame."""
    mask, kind = _mask_arg(view_valid, view_joint_valid, b, v, j)
    out = torch.empty((b,), dtype=torch.float64, device=per_map.device)
    _check(
        _views_entry("mval_score_reduce_masked")(
            _p(_req(per_map, torch.float32, "per_map")), _p(valid), _p(mask), kind, _p(out), b, v, j, mode, _stream(),
        ),
        "mval_score_reduce_masked",
    )
    return out


# --------------------------------------------------------------------------
# loss / metric
# --------------------------------------------------------------------------
def masked_mse_fwd(h, g, valid, lead, hw, denom):
    out = torch.zeros((), dtype=torch.float32, device=h.device)
    ws = torch.empty((2048,), dtype=torch.float64, device=h.device)
    _check(
        lib().mval_masked_mse_fwd(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(g, torch.float32, "gt")), _p(valid), _p(out), _p(ws),
            C.c_longlong(lead), C.c_longlong(hw), C.c_double(denom), _stream(),
        ),
        "mval_masked_mse_fwd",
    )
    return out


def masked_mse_bwd(h, g, valid, grad_out, lead, hw, denom):
    gh = torch.empty_like(h)
    _check(
        lib().mval_masked_mse_bwd(
            _p(h), _p(g), _p(valid), _p(_req(grad_out, torch.float32, "grad")), _p(gh),
            C.c_longlong(lead), C.c_longlong(hw), C.c_double(denom), _stream(),
        ),
        "mval_masked_mse_bwd",
    )
    return gh


def _points_sigma(sigma, lead, device, what):
    """(scalar sigma, per-map sigmas (lead,) f64 on ``device`` or None) of the points form.  The C entry checks the scalar; it
    cannot look at a device array without a synchronise, so an array is checked here, while it is on the host, and staged through
    pinned memory.  An array that is already on the device is taken as it is: a sigma <= 0 there makes the loss NaN or inf."""
    if not (torch.is_tensor(sigma) or hasattr(sigma, "__len__") or hasattr(sigma, "shape")):
        return float(sigma), None
    t = torch.as_tensor(sigma).to(torch.float64).reshape(-1)
    if t.numel() != lead:
        raise MvalError(f"{what}: {t.numel()} sigmas for {lead} maps")
    if not t.is_cuda:
        if lead and not bool((t > 0).all()):
            raise MvalError(f"{what}: sigma must be positive")
        t = t.contiguous()
        t = (t if t.is_pinned() or not torch.cuda.is_available() else t.pin_memory()).to(device, non_blocking=True)
    return 1.0, t.contiguous()


def _points_args(h, pt, lead, hh, wh, what):
    if h.numel() != lead * hh * wh:
        raise MvalError(f"{what}: heat-maps {tuple(h.shape)} are not {lead} maps of {hh} x {wh}")
    if pt.numel() != lead * 2:
        raise MvalError(f"{what}: points {tuple(pt.shape)} are not ({lead}, 2)")
    if not pt.is_cuda:
        raise MvalError(f"{what}: points must be a HIP tensor")


def masked_mse_points_fwd(h, pt, sigma, valid, lead, hh, wh, denom):
    """``masked_mse_fwd`` against the maps mval_gt_heatmaps renders from pt (lead, 2) f64, without them.  sigma: a float, or one
    per map ((lead,) array or tensor, host or device)."""
    what = "mval_masked_mse_points_fwd"
    _points_args(h, pt, lead, hh, wh, what)
    s, sm = _points_sigma(sigma, lead, h.device, what)
    out = torch.zeros((), dtype=torch.float32, device=h.device)
    ws = torch.empty((2048,), dtype=torch.float64, device=h.device)
    _check(
        lib().mval_masked_mse_points_fwd(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(pt, torch.float64, "points")), C.c_double(s), _p(sm), _p(valid),
            _p(out), _p(ws), C.c_longlong(lead), C.c_int(hh), C.c_int(wh), C.c_double(denom), _stream(),
        ),
        what,
    )
    return out


def masked_mse_points_bwd(h, pt, sigma, valid, grad_out, lead, hh, wh, denom):
    what = "mval_masked_mse_points_bwd"
    _points_args(h, pt, lead, hh, wh, what)
    s, sm = _points_sigma(sigma, lead, h.device, what)
    gh = torch.empty_like(h)
    _check(
        lib().mval_masked_mse_points_bwd(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(pt, torch.float64, "points")), C.c_double(s), _p(sm), _p(valid),
            _p(_req(grad_out, torch.float32, "grad")), _p(gh),
            C.c_longlong(lead), C.c_int(hh), C.c_int(wh), C.c_double(denom), _stream(),
        ),
        what,
    )
    return gh


def frame_loss_workspace_bytes(n_frames: int, maps_per_frame: int) -> int:
    return int(lib().mval_frame_loss_workspace_bytes(C.c_longlong(n_frames), C.c_int(maps_per_frame)))


def _frame_loss_outputs(h, n_frames, maps_per_frame):
    out = torch.empty((n_frames,), dtype=torch.float32, device=h.device)
    per_map = torch.empty((frame_loss_workspace_bytes(n_frames, maps_per_frame) // 8,), dtype=torch.float64, device=h.device)
    return out, per_map


def frame_loss(h, g, valid, n_frames, maps_per_frame, hh, wh):
    """h, g (n_frames, maps_per_frame, hh, wh) f32, valid (n_frames * maps_per_frame,) u8 or None -> (per-frame loss
    (n_frames,) f32, every map's sum of squared errors (n_frames * maps_per_frame,) f64)."""
    out, per_map = _frame_loss_outputs(h, n_frames, maps_per_frame)
    _check(
        lib().mval_frame_loss(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(g, torch.float32, "gt")), _p(valid), _p(out), _p(per_map),
            C.c_longlong(n_frames), C.c_int(maps_per_frame), C.c_int(hh), C.c_int(wh), _stream(),
        ),
        "mval_frame_loss",
    )
    return out, per_map


def frame_loss_points(h, pt, sigma, valid, n_frames, maps_per_frame, hh, wh):
    """``frame_loss`` against the maps mval_gt_heatmaps renders from pt (n_frames * maps_per_frame, 2) f64, without them."""
    out, per_map = _frame_loss_outputs(h, n_frames, maps_per_frame)
    _check(
        lib().mval_frame_loss_points(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(pt, torch.float64, "points")), C.c_double(float(sigma)), _p(valid),
            _p(out), _p(per_map), C.c_longlong(n_frames), C.c_int(maps_per_frame), C.c_int(hh), C.c_int(wh), _stream(),
        ),
        "mval_frame_loss_points",
    )
    return out, per_map


def weighted_mse_workspace_bytes(n_images: int, n_joints: int) -> int:
    return int(lib().mval_weighted_mse_workspace_bytes(C.c_longlong(n_images), C.c_int(n_joints)))


def loss_weights(weight, lead, device, what):
    """The (lead,) f32 per-map weights of the weighted loss on ``device``.  Like ``_points_sigma``: weights that arrive on the host are
    checked there (finite and >= 0) and staged through pinned memory; a device tensor is taken as it is -- a NaN there makes the
    loss NaN, a negative weight a loss that ranks and sums as the contract says but means nothing."""
    t = torch.as_tensor(weight).to(torch.float32).reshape(-1)
    if t.numel() != lead:
        raise MvalError(f"{what}: {t.numel()} weights for {lead} maps")
    if not t.is_cuda:
        if lead and not bool((torch.isfinite(t) & (t >= 0)).all()):
            raise MvalError(f"{what}: weights must be finite and >= 0")
        t = t.contiguous()
        t = (t if t.is_pinned() or not torch.cuda.is_available() else t.pin_memory()).to(device, non_blocking=True)
    return t.contiguous()


def _weighted_outputs(h, n_images, n_joints):
    lead = n_images * n_joints
    out = torch.zeros((), dtype=torch.float32, device=h.device)
    per_map = torch.empty((lead,), dtype=torch.float64, device=h.device)
    wsel = torch.empty((lead,), dtype=torch.float32, device=h.device)
    ws = torch.empty((max(1, weighted_mse_workspace_bytes(n_images, n_joints) // 8),), dtype=torch.float64, device=h.device)
    return out, per_map, wsel, ws


def weighted_mse_fwd(h, g, weight, topk, n_images, n_joints, hh, wh):
    """The weighted / hard-key-point-mining loss (mval_weighted_mse_fwd): h, g (n_images, n_joints, hh, wh) f32, weight
    (n_images * n_joints,) f32 >= 0, topk in [0, n_joints] (0: every joint counts) -> (loss () f32, every map's weight * sum of
    squared errors (lead,) f64, the weights of the selected maps and 0 elsewhere (lead,) f32: what the backward reads)."""
    what = "mval_weighted_mse_fwd"
    lead = n_images * n_joints
    if h.numel() != lead * hh * wh or g.numel() != h.numel():
        raise MvalError(f"{what}: heat-maps {tuple(h.shape)} / ground truth {tuple(g.shape)} are not {lead} maps of {hh} x {wh}")
    w = loss_weights(weight, lead, h.device, what)
    out, per_map, wsel, ws = _weighted_outputs(h, n_images, n_joints)
    _check(
        lib().mval_weighted_mse_fwd(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(g, torch.float32, "gt")), _p(w), C.c_int(topk), _p(out), _p(per_map),
            _p(wsel), _p(ws), C.c_longlong(n_images), C.c_int(n_joints), C.c_int(hh), C.c_int(wh), _stream(),
        ),
        what,
    )
    return out, per_map, wsel


def weighted_mse_points_fwd(h, pt, sigma, weight, topk, n_images, n_joints, hh, wh):
    """``weighted_mse_fwd`` against the maps mval_gt_heatmaps renders from pt (lead, 2) f64, without them.  sigma: a float, or one
    per map ((lead,) array or tensor, host or device)."""
    what = "mval_weighted_mse_points_fwd"
    lead = n_images * n_joints
    _points_args(h, pt, lead, hh, wh, what)
    s, sm = _points_sigma(sigma, lead, h.device, what)
    w = loss_weights(weight, lead, h.device, what)
    out, per_map, wsel, ws = _weighted_outputs(h, n_images, n_joints)
    _check(
        lib().mval_weighted_mse_points_fwd(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(pt, torch.float64, "points")), C.c_double(s), _p(sm), _p(w),
            C.c_int(topk), _p(out), _p(per_map), _p(wsel), _p(ws), C.c_longlong(n_images), C.c_int(n_joints), C.c_int(hh),
            C.c_int(wh), _stream(),
        ),
        what,
    )
    return out, per_map, wsel


def weighted_mse_bwd(h, g, wsel, grad_out, n_images, n_joints, hh, wh):
    """grad_h = ((2 (h - g)) * grad_out / (n_images * hh * wh)) * wsel[map], +0.0 on the maps with wsel == 0 (not read)."""
    gh = torch.empty_like(h)
    _check(
        lib().mval_weighted_mse_bwd(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(g, torch.float32, "gt")), _p(_req(wsel, torch.float32, "wsel")),
            _p(_req(grad_out, torch.float32, "grad")), _p(gh), C.c_longlong(n_images), C.c_int(n_joints), C.c_int(hh), C.c_int(wh),
            _stream(),
        ),
        "mval_weighted_mse_bwd",
    )
    return gh


def weighted_mse_points_bwd(h, pt, sigma, wsel, grad_out, n_images, n_joints, hh, wh):
    what = "mval_weighted_mse_points_bwd"
    lead = n_images * n_joints
    _points_args(h, pt, lead, hh, wh, what)
    s, sm = _points_sigma(sigma, lead, h.device, what)
    gh = torch.empty_like(h)
    _check(
        lib().mval_weighted_mse_points_bwd(
            _p(_req(h, torch.float32, "heatmaps")), _p(_req(pt, torch.float64, "points")), C.c_double(s), _p(sm),
            _p(_req(wsel, torch.float32, "wsel")), _p(_req(grad_out, torch.float32, "grad")), _p(gh), C.c_longlong(n_images),
            C.c_int(n_joints), C.c_int(hh), C.c_int(wh), _stream(),
        ),
        what,
    )
    return gh


def mkpe(pred, gt, valid, s, j, gt_rows):
    """pred (S,J,3) f32, gt (S,gt_rows,J) f32, valid (S,J) f32 -> scalar f32 (+ per-sample (S,))."""
    out = torch.empty((), dtype=torch.float32, device=pred.device)
    per = torch.empty((s,), dtype=torch.float32, device=pred.device)
    _check(
        lib().mval_mkpe(
            _p(_req(pred, torch.float32, "pred")), _p(_req(gt, torch.float32, "gt")),
            _p(_req(valid, torch.float32, "valid")), _p(out), _p(per),
            C.c_longlong(s), C.c_int(j), C.c_int(gt_rows), _stream(),
        ),
        "mval_mkpe",
    )
    return out, per


def pck3d(pred, gt, valid, thresholds, mode):
    """3-D PCK (mode 0, mm thresholds over valid joints) / PCKh (mode 1) counters: pred (S,J,3) f32, gt (S,R,J) f32,
    valid (S,J) f32 or None -> hits (T,J) int64, counts (J,) int64 (device)."""
    s, j, _ = pred.shape
    thr = torch.as_tensor(list(thresholds), dtype=torch.float64).to(pred.device)
    hits = torch.empty((thr.numel(), j), dtype=torch.int64, device=pred.device)
    counts = torch.empty((j,), dtype=torch.int64, device=pred.device)
    _check(
        lib().mval_pck3d(
            _p(_req(pred, torch.float32, "pred")), _p(_req(gt, torch.float32, "gt")),
            _p(_req(valid, torch.float32, "valid")) if valid is not None else _p(None), _p(thr), C.c_int(thr.numel()),
            C.c_int(mode), _p(hits), _p(counts), C.c_longlong(s), C.c_int(j), C.c_int(gt.shape[1]), _stream(),
        ),
        "mval_pck3d",
    )
    return hits, counts


def pckh2d(pred, gt, thresholds, n_keypoints, kp0=0, kp1=1):
    """2-D PCKh counters: pred, gt (S,J,2) f32, head = the distance between gt joints kp0 and kp1 -> hits (T, n_keypoints) int64
    (device), one launch for all thresholds."""
    if pred.dim() != 3 or pred.shape[2] != 2 or pred.shape != gt.shape:
        raise MvalError(f"pckh2d: pred and gt must both be (S, J, 2), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    s, j, _ = pred.shape
    thr = torch.as_tensor(list(thresholds), dtype=torch.float64).to(pred.device)
    hits = torch.empty((thr.numel(), int(n_keypoints)) if 0 < int(n_keypoints) <= j else (0,), dtype=torch.int64, device=pred.device)
    _check(
        lib().mval_pckh2d(
            _p(_req(pred, torch.float32, "pred")), _p(_req(gt, torch.float32, "gt")), _p(thr), C.c_int(thr.numel()),
            C.c_int(kp0), C.c_int(kp1), _p(hits), C.c_longlong(s), C.c_int(j), C.c_int(int(n_keypoints)), _stream(),
        ),
        "mval_pckh2d",
    )
    return hits


# --------------------------------------------------------------------------
# training step
# --------------------------------------------------------------------------
def train_bsum_launches(reset: bool = False) -> int:
    """mval_train_bsum_launches: data gradients of the training backward that kept their producer's BatchNorm backward sums since the
    library was loaded or the count was last reset (TrainPlan.n_bn_bwd_in_dgrad per step unless a launch fell back to the plain form)."""
    return int(lib().mval_train_bsum_launches(C.c_int(1 if reset else 0)))


# --------------------------------------------------------------------------
# which split-MFMA kernel a launch runs on (host arithmetic: needs no GPU)
# --------------------------------------------------------------------------
SPLIT_NE6, SPLIT_NE10, SPLIT_ROW_SHARING, SPLIT_TWO_CHUNK = 0, 1, 2, 3  # MVAL_SPLIT_* (include/mval_hip.h): mval_split_form.variant
SPLIT_USE_OP, SPLIT_USE_TRAIN_FWD, SPLIT_USE_DGRAD, SPLIT_USE_DGRAD_PARITY = 0, 1, 2, 3  # MVAL_SPLIT_USE_*


class SplitForm(C.Structure):
    """include/mval_hip.h: struct mval_split_form."""

    _fields_ = [(name, C.c_int32) for name in ("pl", "ks", "s", "wn", "wm", "nt", "ms", "g", "variant", "th", "tw", "tn", "odd", "precise",
                                               "grid_x", "grid_y", "grid_z", "bn_part_ok", "bn_part")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def conv_split_form(use, op, n_images, algo):
    """mval_conv_split_form: the kernel form (SplitForm) the library's launch of the MvalOp ``op`` under ``use`` (SPLIT_USE_*) and ``algo``
    (MVAL_ALGO_MFMA_BF3 / _H2) ends on, or None where it has no split kernel for it."""
    form = SplitForm()
    ok = lib().mval_conv_split_form(C.c_int(use), C.byref(op), C.c_int(n_images), C.c_int(algo), C.byref(form))
    return form if ok else None


class MfmaForm(C.Structure):
    """include/mval_hip.h: struct mval_mfma_form."""

    _fields_ = [(name, C.c_int32) for name in ("ks", "s", "kc", "wn", "wm", "nt", "ms", "ne", "th", "tw", "tn", "dil", "nbuf", "grid_x", "grid_y",
                                               "bn_part_ok", "bn_part")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def conv_mfma_form(use, op, n_images):
    """mval_conv_mfma_form: the kernel form (MfmaForm) of the exact-fp32 MFMA conv the library's launch of the MvalOp ``op`` under ``use``
    (SPLIT_USE_OP / _TRAIN_FWD / _DGRAD) ends on, or None where it has no such kernel for it."""
    form = MfmaForm()
    ok = lib().mval_conv_mfma_form(C.c_int(use), C.byref(op), C.c_int(n_images), C.byref(form))
    return form if ok else None


class P2Form(C.Structure):
    """include/mval_hip.h: struct mval_p2_form."""

    _fields_ = [(name, C.c_int32) for name in ("ks", "s", "g", "wn", "wm", "nt", "ms", "tw", "rs", "epi", "ow", "k48", "inz", "bsum", "th", "tile_w",
                                               "flat", "in_sub", "parities", "groups", "tiles_x", "tiles_y", "tiles_total", "smem_bytes", "threads")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def conv_p2_form(use, op, n_images):
    """mval_conv_p2_form: the kernel form (P2Form) of the P2 conv the library's launch of the MvalOp ``op`` under ``use`` (SPLIT_USE_OP /
    _TRAIN_FWD / _DGRAD) ends on, or None where it has no P2 kernel for it."""
    form = P2Form()
    ok = lib().mval_conv_p2_form(C.c_int(use), C.byref(op), C.c_int(n_images), C.byref(form))
    return form if ok else None


def fused_p2_form(op, n_images):
    """mval_fused_p2_form: the tiling (P2Form: th, tile_w, tiles_*, groups, parities, smem_bytes, threads) of the fused P2 launch -- BasicBlock,
    Bottleneck, stem, fuse-up -- mval_op_launch runs for the MvalOp ``op``, or None where it has no such kernel for it."""
    form = P2Form()
    ok = lib().mval_fused_p2_form(C.byref(op), C.c_int(n_images), C.byref(form))
    return form if ok else None


# --------------------------------------------------------------------------
# core-set (k-center greedy)
# --------------------------------------------------------------------------
def kcenter_workspace_bytes(n_obs: int, d: int) -> int:
    return int(lib().mval_kcenter_workspace_bytes(C.c_longlong(n_obs), C.c_int(d)))


# MVAL_KC_* (include/mval_hip.h): the distance forms of mval_kcenter_select_metric, and sklearn's names for them
KC_EUCLIDEAN, KC_L1, KC_COSINE, KC_CHEBYSHEV = 0, 1, 2, 3
KC_METRIC_IDS = {
    "euclidean": KC_EUCLIDEAN, "l2": KC_EUCLIDEAN,
    "manhattan": KC_L1, "l1": KC_L1, "cityblock": KC_L1,
    "cosine": KC_COSINE,
    "chebyshev": KC_CHEBYSHEV,
}


def kcenter_metric_id(metric) -> int:
    """The MVAL_KC_* id of one of sklearn's metric names; NotImplementedError (naming the accepted ones) otherwise."""
    if not isinstance(metric, str) or metric not in KC_METRIC_IDS:
        raise NotImplementedError(f"core-set metric {metric!r}: accepted are " + ", ".join(repr(k) for k in KC_METRIC_IDS))
    return KC_METRIC_IDS[metric]


def kcenter_select(feat, labeled_idx, n_select, min_dist=None, metric="euclidean"):
    """feat (n_obs, D) f64; labeled_idx (L,) int64 or None; metric: a name of KC_METRIC_IDS.  Returns (picks int64
    (n_select,), min_dist f64 (n_obs,)).  "euclidean" / "l2" go to mval_kcenter_select, the others to
    mval_kcenter_select_metric."""
    mid = kcenter_metric_id(metric)
    n_obs, d = feat.shape
    dev = feat.device
    picks = torch.empty((n_select,), dtype=torch.int64, device=dev)
    md = torch.empty((n_obs,), dtype=torch.float64, device=dev) if min_dist is None else min_dist
    norms = torch.empty((n_obs,), dtype=torch.float64, device=dev)
    ws = torch.empty((kcenter_workspace_bytes(n_obs, d) // 8 + 1,), dtype=torch.float64, device=dev)
    nl = 0 if labeled_idx is None else int(labeled_idx.numel())
    args = (
        _p(_req(feat, torch.float64, "features")), C.c_longlong(n_obs), C.c_int(d),
        _p(labeled_idx if nl else None), C.c_longlong(nl), C.c_int(n_select),
        C.c_int(0 if min_dist is None else 1),
        _p(norms), _p(md), _p(picks), _p(ws), _stream(),
    )
    if mid == KC_EUCLIDEAN:
        _check(lib().mval_kcenter_select(*args), "mval_kcenter_select")
    else:
        _check(lib().mval_kcenter_select_metric(C.c_int(mid), *args), "mval_kcenter_select_metric")
    return picks, md


def nearest_center(feat, centers):
    """feat (n, D) f64, centers (K, D) f64 (device) -> (n,) int32 labels."""
    n, d = feat.shape
    out = torch.empty((n,), dtype=torch.int32, device=feat.device)
    _check(
        lib().mval_nearest_center(_p(_req(feat, torch.float64, "feat")), _p(_req(centers, torch.float64, "centers")),
                                  C.c_longlong(n), C.c_int(d), C.c_int(centers.shape[0]), _p(out), _stream()),
        "mval_nearest_center",
    )
    return out


def kmeans_workspace_bytes(n: int, d: int, k: int, n_trials: int) -> int:
    return int(lib().mval_kmeans_workspace_bytes(C.c_longlong(n), C.c_int(d), C.c_int(k), C.c_int(n_trials)))


def kmeans_fit(x, k, init_centers, first_idx, rand_u, n_trials, max_iter, tol):
    """One KMeans initialisation + Lloyd run on x (n, D) f64 (device).  init_centers (K, D) f64 or None (k-means++
    with first_idx and rand_u ((K-1)*n_trials,) f64).  Returns device tensors (centers (K, D) f64, labels (n,) int32,
    inertia (1,) f64, n_iter (1,) int32, init_idx (K,) int64)."""
    n, d = x.shape
    dev = x.device
    centers = torch.empty((k, d), dtype=torch.float64, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    inertia = torch.empty((1,), dtype=torch.float64, device=dev)
    n_iter = torch.empty((1,), dtype=torch.int32, device=dev)
    init_idx = torch.empty((k,), dtype=torch.int64, device=dev)
    ws = torch.empty((kmeans_workspace_bytes(n, d, k, n_trials) // 8 + 1,), dtype=torch.float64, device=dev)
    _check(
        lib().mval_kmeans_fit(
            _p(_req(x, torch.float64, "X")), C.c_longlong(n), C.c_int(d), C.c_int(k),
            _p(None if init_centers is None else _req(init_centers, torch.float64, "init")), C.c_longlong(first_idx),
            _p(None if rand_u is None else _req(rand_u, torch.float64, "rand_u")), C.c_int(n_trials),
            C.c_int(max_iter), C.c_double(tol), _p(centers), _p(labels), _p(inertia), _p(n_iter), _p(init_idx),
            _p(ws), _stream(),
        ),
        "mval_kmeans_fit",
    )
    return centers, labels, inertia, n_iter, init_idx


def coreset_features(pose, root_idx, n, j, rows):
    """pose (n, j, rows>=3) f64 [joint, coord] -> (n, 3j) f64 root-relative, coord-major."""
    out = torch.empty((n, 3 * j), dtype=torch.float64, device=pose.device)
    _check(
        lib().mval_coreset_features(
            _p(_req(pose, torch.float64, "pose")), _p(out), C.c_longlong(n), C.c_int(j), C.c_int(rows),
            C.c_int(root_idx), _stream(),
        ),
        "mval_coreset_features",
    )
    return out

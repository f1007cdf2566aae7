"""Per-view input pipeline on the device: the reference's ``ActiveLearningDataset.prepare_single_view``
(dataset/dataset.py:158-220) for a batch of views: the "val"/"test" split by default, the "train" split with a
``utils.augmentation.RandAugment`` (resize to uint8, the augmentation's Pillow ops on the device, then the normalisation).

Host (numpy float64, the reference's own arithmetic): square / scaled box (utils/triangulation.py:96-134),
camera update after crop and resize (:44-67), projection of the 3-D joints (:153-165, 433-484).
Device (csrc/preprocess.hip): BGR flip, zero-filled crop, PIL LANCZOS resize (bit-exact with Pillow's
8-bit resampler), ImageNet normalisation, Gaussian ground-truth heat-maps; csrc/augment.hip: RandAugment.  JPEG decode stays
outside.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib


def get_square_bbox(bbox):
    """utils/triangulation.py:96-118."""
    left, upper, right, lower = bbox
    width, height = right - left, lower - upper
    if width > height:
        y_center = (upper + lower) // 2
        upper = y_center - width // 2
        lower = upper + width
    else:
        x_center = (left + right) // 2
        left = x_center - height // 2
        right = left + height
    return left, upper, right, lower


def scale_bbox(bbox, scale):
    """utils/triangulation.py:121-134."""
    left, upper, right, lower = bbox
    width, height = right - left, lower - upper
    x_center, y_center = (right + left) // 2, (lower + upper) // 2
    new_width, new_height = int(scale * width), int(scale * height)
    new_left = x_center - new_width // 2
    new_upper = y_center - new_height // 2
    return new_left, new_upper, new_left + new_width, new_upper + new_height


def _project(K, R, t, dist, X):
    """project_3d_points_with_camera (utils/triangulation.py:153-165): X (N, 3) -> (N, 2) float64."""
    if dist is not None:
        Kd = np.asarray(dist, dtype=np.float64).flatten()
        x = np.asarray(R.dot(X.T) + t)
        x[0:2, :] = x[0:2, :] / x[2, :]
        r = x[0, :] * x[0, :] + x[1, :] * x[1, :]
        x[0, :] = (x[0, :] * (1 + Kd[0] * r + Kd[1] * r * r + Kd[4] * r * r * r) + 2 * Kd[2] * x[0, :] * x[1, :]
                   + Kd[3] * (r + 2 * x[0, :] * x[0, :]))
        x[1, :] = (x[1, :] * (1 + Kd[0] * r + Kd[1] * r * r + Kd[4] * r * r * r) + 2 * Kd[3] * x[0, :] * x[1, :]
                   + Kd[2] * (r + 2 * x[1, :] * x[1, :]))
        x[0, :] = K[0, 0] * x[0, :] + K[0, 1] * x[1, :] + K[0, 2]
        x[1, :] = K[1, 0] * x[0, :] + K[1, 1] * x[1, :] + K[1, 2]
        return x.T[:, :2]
    h = np.concatenate([X, np.ones((X.shape[0], 1))], axis=1) @ K.dot(np.hstack([R, t])).T
    w = h[:, 2:3].copy()
    w[w == 0] = 1.0
    return h[:, :2] / w


class _ViewDesc(C.Structure):
    """include/mval_hip.h: struct mval_view_desc."""

    _fields_ = [("img", C.c_void_p), ("h0", C.c_int32), ("w0", C.c_int32), ("left", C.c_int32), ("top", C.c_int32),
                ("right", C.c_int32), ("bottom", C.c_int32), ("tmp_off", C.c_int64)]


# Descriptor uploads of resize_views: a small ring of pinned host buffers per device, copied with non_blocking=True on the current
# stream (a pageable copy would stall the host until the stream drains -- a batch pipeline then loses the overlap of the next
# batch's launches with the GPU's work); a slot is reused only after the event recorded behind its last copy has completed.
_DESC_RING = {}


def _upload_descs(raw: bytes, dev):
    key = dev.index
    ring = _DESC_RING.setdefault(key, {"k": 0, "slots": [None] * 4})
    i = ring["k"] % 4
    ring["k"] += 1
    slot = ring["slots"][i]
    if slot is None or slot[0].numel() < len(raw):
        slot = [torch.empty(max(len(raw), 16384), dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
        ring["slots"][i] = slot
    else:
        slot[1].synchronize()
    slot[0][: len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    out = slot[0][: len(raw)].to(dev, non_blocking=True)
    slot[1].record(torch.cuda.current_stream(dev))
    return out


def _resize(images, boxes, in_w, in_h, as_u8):
    what = "resize_views_u8" if as_u8 else "resize_views"
    if not images or any((not torch.is_tensor(im)) or (not im.is_cuda) or im.dtype != torch.uint8 for im in images):
        raise _lib.MvalError(what + ": images must be uint8 HIP tensors (h0, w0, 3)")
    dev = images[0].device
    images = [im.contiguous() for im in images]
    descs = (_ViewDesc * len(images))()
    rows = 0
    for d, im, b in zip(descs, images, boxes):
        left, top, right, bottom = (int(v) for v in b)
        if right <= left or bottom <= top:
            raise ValueError(what + ": empty box %r" % (b,))
        d.img, d.h0, d.w0 = im.data_ptr(), im.shape[0], im.shape[1]
        d.left, d.top, d.right, d.bottom = left, top, right, bottom
        d.tmp_off = rows * in_w * 3
        rows += bottom - top
    lib = _lib.lib()
    lib.mval_prepare_views_workspace_bytes.restype = C.c_size_t
    ws = torch.empty(int(lib.mval_prepare_views_workspace_bytes(C.c_int(len(images)), C.c_int64(rows), C.c_int(in_w), C.c_int(in_h))),
                     dtype=torch.uint8, device=dev)
    dd = _upload_descs(bytes(descs), dev)
    if as_u8:
        out = torch.empty((len(images), in_h, in_w, 3), dtype=torch.uint8, device=dev)
        fn, name = lib.mval_resize_views_u8, "mval_resize_views_u8"
    else:
        out = torch.empty((len(images), 3, in_h, in_w), dtype=torch.float32, device=dev)
        fn, name = lib.mval_prepare_views, "mval_prepare_views"
    _lib._check(
        fn(_lib._p(dd), C.c_int(len(images)), C.c_int(max(d.bottom - d.top for d in descs)),
           C.c_int(max(d.right - d.left for d in descs)), C.c_int(in_w), C.c_int(in_h), _lib._p(out),
           _lib._p(ws), _lib._stream()),
        name)
    return out


def resize_views(images, boxes, in_w, in_h):
    """Pixel half of prepare_single_view for a list of decoded RGB images (uint8 HIP tensors (h0, w0, 3)) and
    their SQUARE boxes: (V, 3, in_h, in_w) float32 on the device (BGR order, ImageNet-normalised)."""
    return _resize(images, boxes, in_w, in_h, False)


def resize_views_u8(images, boxes, in_w, in_h):
    """resize_views up to the resized bytes: (V, in_h, in_w, 3) uint8 on the device in the reference's channel order (BGR),
    the image the training split hands to its augmentation.  normalize_views_u8 of it equals resize_views bit for bit."""
    return _resize(images, boxes, in_w, in_h, True)


def normalize_views_u8(images_u8):
    """normalize_image (utils/triangulation.py:137-145): (V, H, W, 3) uint8 HIP tensor -> (V, 3, H, W) float32."""
    if (not torch.is_tensor(images_u8)) or (not images_u8.is_cuda) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 \
            or images_u8.shape[3] != 3:
        raise _lib.MvalError("normalize_views_u8: images must be a uint8 HIP tensor (V, H, W, 3)")
    images_u8 = images_u8.contiguous()
    v, h, w, _ = images_u8.shape
    out = torch.empty((v, 3, h, w), dtype=torch.float32, device=images_u8.device)
    _lib._check(_lib.lib().mval_normalize_views_u8(_lib._p(images_u8), C.c_int(v), C.c_int(h), C.c_int(w), _lib._p(out), _lib._stream()),
                "mval_normalize_views_u8")
    return out


def gt_heatmaps(pt, sigma, h, w):
    """dataset.py:198-207: pt (..., 2) float64 heat-map-pixel coordinates (HIP tensor) -> (..., h, w) float32."""
    pt = pt.to(torch.float64).contiguous()
    if not pt.is_cuda:
        raise _lib.MvalError("gt_heatmaps: points must be a HIP tensor")
    n = pt.numel() // 2
    out = torch.empty(tuple(pt.shape[:-1]) + (h, w), dtype=torch.float32, device=pt.device)
    _lib._check(_lib.lib().mval_gt_heatmaps(_lib._p(pt), C.c_int64(n), C.c_double(float(sigma)), C.c_int(h), C.c_int(w),
                                            _lib._p(out), _lib._stream()), "mval_gt_heatmaps")
    return out


def prepare_views(images, boxes, cameras, kp_3d, scale_bbox_factor, in_w, in_h, gt_stride, sigma, augmentation=None, compact=False,
                  with_cameras=False):
    """Batch of views of one or more frames: images (list of uint8 HIP tensors (h0, w0, 3) RGB), boxes (list of
    (left, top, right, bottom)), cameras (list of dicts R, t, K, dist), kp_3d ((>=3, J) array, or one per
    view).  Returns the reference's per-view entries stacked over views: images (V,3,H,W) and gt_heatmap
    (V,J,h,w) on the device; proj_matrices (V,3,4) float64, 2d_keypoints / 2d_after_crop (V,J,2) float32,
    square_box (V,4) float32 on the host.
    augmentation: None (the "val"/"test" split), or a utils.augmentation.RandAugment (the "train" split, dataset.py:212-213): its ops are drawn
    per view in order (one plan, drawn once, before the image ops) and run on the resized uint8 views before the normalisation.  What its
    Rotate does to the targets is the augmentation's ``rotate_targets``: "none" -- gt_heatmap / gt_points are unchanged (the reference drops the
    rotated maps); "maps" -- gt_heatmap is ``rotate_maps`` of the rendered maps under the same plan (the reference with its Rotate keeping the
    maps; no compact form: ValueError before any draw or device work); "points" -- the projected float64 points go through
    ``utils.augmentation.rotate_points(pt, plan, in_w, in_h)`` before the division by gt_stride, for gt_points and for the maps rendered from
    them.  2d_keypoints, 2d_after_crop, proj_matrices, square_box and the validity masks stay as they are in every mode: the reference with
    its Rotate fixed would not change them either.
    compact: True returns the batch in its small form -- images as the resized (and, with an augmentation, augmented) uint8 views (V,H,W,3),
    what ``resize_views_u8`` gives, and gt_points (V,J,2) float64 on the device, the heat-map-pixel positions ``gt_heatmaps`` is handed
    otherwise, instead of gt_heatmap; the other keys are unchanged.  ``strategy.train_step`` and everything that goes through
    ``_compute_batch_heatmap`` take such a batch: the views are normalised and the maps rendered on the device, to the same bits.
    with_cameras: True adds two host float64 keys, what ``triangulate_batch(undistort="brown")`` and AL.UNDISTORT / EVAL.UNDISTORT need
    beside proj_matrices = K [R|t]: intrinsics (V,3,3), the K after update_after_crop and update_after_resize, and distortion (V,5) =
    k1, k2, p1, p2, k3 of the polynomial gt_heatmap / gt_points / 2d_keypoints were projected through (zeros for a camera without
    ``dist``, which is projected without it).  False, the default, returns today's keys."""
    v = len(images)
    rotate_targets = "none" if augmentation is None else getattr(augmentation, "rotate_targets", "none")
    if rotate_targets == "maps" and compact:
        raise ValueError("prepare_views: rotate_targets='maps' rotates rendered heat-maps and a compact batch has none: use 'points'")
    kps = kp_3d if isinstance(kp_3d, (list, tuple)) else [kp_3d] * v
    sq, proj, pts, pts_crop, intrinsics, distortion = [], [], [], [], [], []
    for box, cam, kp in zip(boxes, cameras, kps):
        bbox = scale_bbox(get_square_bbox(tuple(int(b) for b in box)), scale_bbox_factor)
        K = np.array(cam["K"], dtype=np.float64).copy()
        R = np.array(cam["R"], dtype=np.float64)
        t = np.array(cam["t"], dtype=np.float64).reshape(3, 1)
        K[0, 2], K[1, 2] = K[0, 2] - bbox[0], K[1, 2] - bbox[1]            # Camera.update_after_crop
        skel = np.array(np.asarray(kp).transpose([1, 0]))[:, :3].astype(np.float64)
        pts_crop.append(_project(K, R, t, cam.get("dist"), skel))
        height, width = bbox[3] - bbox[1], bbox[2] - bbox[0]               # image shape before the resize
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]                # Camera.update_after_resize
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx * (in_w / width), fy * (in_h / height), cx * (in_w / width), cy * (in_h / height)
        proj.append(K.dot(np.hstack([R, t])))
        intrinsics.append(K)
        distortion.append(np.zeros(5) if cam.get("dist") is None else np.asarray(cam["dist"], dtype=np.float64).flatten()[:5])
        pts.append(_project(K, R, t, cam.get("dist"), skel))
        sq.append(bbox)
    plan = None
    if augmentation is None:
        out_images = resize_views_u8(images, sq, in_w, in_h) if compact else resize_views(images, sq, in_w, in_h)
    else:
        out_images = resize_views_u8(images, sq, in_w, in_h)
        plan = augmentation.draw(v)
        out_images = augmentation.apply(out_images, plan, inplace=True)
        if not compact:
            out_images = normalize_views_u8(out_images)
    pt = np.stack(pts)
    if rotate_targets == "points":
        from .augmentation import rotate_points

        gt_points = torch.from_numpy(rotate_points(pt, plan, in_w, in_h) / gt_stride).to(out_images.device)
    else:
        gt_points = torch.from_numpy(pt / gt_stride).to(out_images.device)
    if compact:
        target = {"gt_points": gt_points}
    else:
        target = {"gt_heatmap": gt_heatmaps(gt_points, sigma, in_h // gt_stride, in_w // gt_stride)}
        if rotate_targets == "maps":
            target["gt_heatmap"] = augmentation.rotate_maps(target["gt_heatmap"], plan, inplace=True)
    cameras = {"intrinsics": np.stack(intrinsics), "distortion": np.stack(distortion)} if with_cameras else {}
    return {
        "images": out_images,
        **target,
        **cameras,
        "proj_matrices": np.stack(proj),
        "2d_keypoints": pt.astype(np.float32),
        "2d_after_crop": np.stack(pts_crop).astype(np.float32),
        "square_box": np.asarray(sq, dtype=np.float32),
    }

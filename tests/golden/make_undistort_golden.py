"""Generate the undistortion goldens on the CPU, with the REAL reference loaded through oracle.ref_harness (build container
only; nothing of the device):

    python tests/golden/make_undistort_golden.py

  undistort.npz  per case of undistort_cases.undistort_cases() (``<case>/...``):
                 K (B, V, 3, 3) after the reference's Camera.update_after_crop and update_after_resize, dist (B, V, 5) (zeros for
                 a camera without ``dist``), R, t, proj = Camera.projection (B, V, 3, 4), joints (B, J, 3);
                 p_dist (B, V, J, 2): the reference's project_3d_points_with_camera -- the distorted pixels the training targets
                 sit at (for a fold entry: the drawn pixel beyond the monotone radius); p_pin: the reference's
                 _project_3d_points_to_image_plane_without_distortion of Camera.projection (NaN for a fold entry);
                 fold_entry (B, V, J) bool; kp_f32 = f32(p_dist), kp_i64 = i64(round(p_dist));
                 f32/out64, f32/status, i64/out64, i64/status: tests/undistort_oracle.py on those two inputs under the case's masks;
                 gap_reference (B, V, J): |oracle(float64 p_dist) - p_pin| in px (largest coordinate; 0 where not compared);
                 gap_chain, gap_distorted (B, J) in mm (cases with e2e): |X - joint| for X = oracle.geometry.triangulate_ransac
                 over the joint's present views of f32(oracle(kp_f32)) and of kp_f32 itself.

A joint is admitted only if det J >= 0.25 at its true point in every present view and its pixels lie in [0, 512); it is redrawn
otherwise, so no entry is left out of any comparison.  A fold entry is admitted only if, for both key-point types, the oracle stops
with FOLD, its failing det J is below -1e-3 and every earlier one above 1e-3: an implementation one ulp away decides the same.
Asserted per e2e case: mean(gap_distorted) >= 100 * max(gap_chain).  The summary printed at the end is what DESIGN.md 6.6 quotes.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import undistort_cases as uc  # noqa: E402
import undistort_oracle as uo  # noqa: E402
from oracle import geometry, ref_harness  # noqa: E402


def present_mask(c):
    valid, vv, vj = uc.masks(c)
    return valid, vv, vj, uo.present(c["b"], c["v"], c["j"], None, vv, vj)  # (an invalid joint still gets an admitted point)


def draw_fold_pixel(rng, K, dist):
    """A pixel beyond the lens's monotone radius at which the oracle stops with FOLD, with margin, as float32 and as int64."""
    while True:
        rho, phi = rng.uniform(0.6, 1.1), rng.uniform(0.0, 2 * np.pi)
        n = rho * np.array([np.cos(phi), np.sin(phi)])
        p = K[:2, :2] @ n + K[:2, 2]
        if not ((p > -512).all() and (p < 512).all()):
            continue
        ok = True
        for q in (p.astype(np.float32).astype(np.float64), np.round(p)):
            _, _, st, dets = uo.undistort_point(q[0], q[1], K, dist)
            ok = ok and st == uo.FOLD and dets[-1] < -uc.FOLD_MARGIN and all(d > uc.FOLD_MARGIN for d in dets[:-1])
        if ok:
            return p


def run(name, c, out, tri):
    rng = np.random.default_rng(c["seed"])
    b, v, j = c["b"], c["v"], c["j"]
    valid, vv, vj, present = present_mask(c)
    K, dist, R, t, proj = np.zeros((b, v, 3, 3)), np.zeros((b, v, 5)), np.zeros((b, v, 3, 3)), np.zeros((b, v, 3)), np.zeros((b, v, 3, 4))
    cams = {}
    for bi in range(b):
        for vi in range(v):
            k0, r, tt = uc.draw_camera(rng, vi, v, c["skew"])
            box = uc.square_box(k0, r, tt)
            cam = tri.Camera(r, tt, k0, uc.lens_of(c, vi))
            cam.update_after_crop(box)
            cam.update_after_resize((box[3] - box[1], box[2] - box[0]), c["in_w"], c["in_h"])
            cams[bi, vi] = cam
            K[bi, vi], R[bi, vi], t[bi, vi], proj[bi, vi] = cam.K, cam.R, cam.t[:, 0], cam.projection
            if cam.dist is not None:
                dist[bi, vi] = cam.dist
    joints, p_dist, p_pin = np.zeros((b, j, 3)), np.zeros((b, v, j, 2)), np.zeros((b, v, j, 2))
    fold_entry = np.zeros((b, v, j), bool)
    min_det_true, redraws = np.inf, 0
    for bi in range(b):
        for ji in range(j):
            while True:
                X = uc.draw_joint(rng)
                pd = np.stack([tri.project_3d_points_with_camera(cams[bi, vi], X[None].copy())[0] for vi in range(v)])
                pp = np.stack([tri._project_3d_points_to_image_plane_without_distortion(cams[bi, vi].projection, X[None].copy())[0] for vi in range(v)])
                dets = []
                for vi in range(v):
                    n = R[bi, vi] @ X + t[bi, vi]
                    dets.append(uo.det_jacobian(n[0] / n[2], n[1] / n[2], dist[bi, vi]))
                pres = present[bi, :, ji]
                if ji in c["fold"] or ((np.array(dets)[pres] >= uc.MIN_DET).all() and (pd[pres] >= 0).all() and (pd[pres] < 512).all()):
                    break
                redraws += 1
            joints[bi, ji], p_dist[bi, :, ji], p_pin[bi, :, ji] = X, pd, pp
            if ji in c["fold"]:
                fold_entry[bi, :, ji] = True
                for vi in range(v):
                    p_dist[bi, vi, ji], p_pin[bi, vi, ji] = draw_fold_pixel(rng, K[bi, vi], dist[bi, vi]), np.nan
            else:
                min_det_true = min(min_det_true, np.array(dets)[pres].min())
    kp_f32, kp_i64 = p_dist.astype(np.float32), np.round(p_dist).astype(np.int64)
    out.update({f"{name}/K": K, f"{name}/dist": dist, f"{name}/R": R, f"{name}/t": t, f"{name}/proj": proj, f"{name}/joints": joints,
                f"{name}/p_dist": p_dist, f"{name}/p_pin": p_pin, f"{name}/fold_entry": fold_entry, f"{name}/kp_f32": kp_f32,
                f"{name}/kp_i64": kp_i64})
    iters, min_det_iter = [], np.inf
    res = {}
    for kind, kp in (("f32", kp_f32), ("i64", kp_i64)):
        r = res[kind] = uo.undistort_batch(kp, K, dist, valid, vv, vj)
        out[f"{name}/{kind}/out64"], out[f"{name}/{kind}/status"] = r["out64"], r["status"]
        assert (r["status"][fold_entry & present & valid[:, None, :]] == uo.FOLD).all()
        ran = ~fold_entry & present & valid[:, None, :] & (dist != 0).any(-1)[:, :, None]
        assert (r["status"][ran] > 0).all(), (name, kind, r["status"])
        assert (r["status"][~(present & valid[:, None, :])] == 0).all()
        iters += r["status"][ran].tolist()
        min_det_iter = min([min_det_iter] + [min(d) for e, d in r["dets"].items() if not fold_entry[e]])
    # the oracle on the float64 distorted points against the reference's pinhole projection
    gap_ref = np.zeros((b, v, j))
    for bi, vi, ji in zip(*np.nonzero(present & ~fold_entry)):
        x, y, st, _ = uo.undistort_point(p_dist[bi, vi, ji, 0], p_dist[bi, vi, ji, 1], K[bi, vi], dist[bi, vi])
        got = p_dist[bi, vi, ji] if st == 0 else np.array([x, y])
        assert st >= 0
        gap_ref[bi, vi, ji] = np.abs(got - p_pin[bi, vi, ji]).max()
    out[f"{name}/gap_reference"] = gap_ref
    line = (f"{name:18s} (B, V, J) = ({b}, {v:2d}, {j:2d}): {redraws:2d} redraws, iterations {min(iters)}..{max(iters)}, min det J "
            f"{min_det_true:.3f} at the true points / {min_det_iter:.3f} over the iterates, gap_reference max {gap_ref.max():.1e} px")
    if c["e2e"]:
        und = res["f32"]["out"]
        gap_chain, gap_dist = np.zeros((b, j)), np.zeros((b, j))
        for bi in range(b):
            for ji in range(j):
                views = np.flatnonzero(present[bi, :, ji])
                if not valid[bi, ji] or len(views) < 2:
                    continue
                for kp, gap in ((und, gap_chain), (kp_f32, gap_dist)):
                    X, _, _ = geometry.triangulate_ransac(proj[bi][views], kp[bi, views, ji].astype(np.float64), uc.N_ITERS, uc.EPS)
                    gap[bi, ji] = np.linalg.norm(X - joints[bi, ji])
        used = (gap_dist > 0) | (gap_chain > 0)
        assert gap_dist[used].mean() >= 100 * gap_chain.max(), (name, gap_dist[used].mean(), gap_chain.max())
        out[f"{name}/gap_chain"], out[f"{name}/gap_distorted"] = gap_chain, gap_dist
        line += (f", gap_chain max {gap_chain.max():.1e} mm, gap_distorted mean {gap_dist[used].mean():.2f} max {gap_dist.max():.2f} mm, "
                 f"pixel shift mean {np.abs(p_dist - p_pin)[present & ~fold_entry].mean():.2f} px")
    print(line)


def main():
    ns = ref_harness.load()
    out = {}
    for name, c in uc.undistort_cases().items():
        run(name, c, out, ns.triangulation)
    out["meta/numpy_version"] = np.array(np.__version__)
    np.savez_compressed(uc.GOLDEN, **out)
    print("wrote", uc.GOLDEN, os.path.getsize(uc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

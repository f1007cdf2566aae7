"""Generate the 3-D refinement goldens on the CPU (numpy only, nothing of the device):

    python tests/golden/make_refine3d_golden.py

  refine3d.npz  per case of refine3d_cases.refine3d_cases() and key-point type (``<case>/i64/...``, ``<case>/f32/...``):
                the inputs (proj, kp, valid, view_valid, view_joint_valid, weights where the case has them), the DLT point of
                every problem by oracle/geometry.py's ``triangulate_ransac`` on the problem's present views (x0, with err0 and
                inliers0; every pair in lexicographic order, n_iters = 496), the support set S at that point (support
                (B, V, J) bool), the float64 oracle's point, status and joint error (tests/refine3d_oracle.py), the minimum
                of the same cost in long double (xmin; the DLT point where the problem is not refined) and
                gap_oracle = |oracle - xmin| in mm.  ``meta/...``: numpy's version and np.finfo(np.longdouble).

Every problem must be decidable between two float64 implementations: min |err - eps| over its present views at the DLT
point >= 1e-6 px (asserted).  The summary printed at the end -- iterations and gaps per number of views -- is what
DESIGN.md 6.5 quotes.
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

import refine3d_cases as rc  # noqa: E402
import refine3d_oracle as ro  # noqa: E402
from oracle import geometry  # noqa: E402

MARGIN = 1e-6


def dlt_points(d, kp):
    """-> x0 (B, J, 3), err0 (B, J), inliers0 (B, J): an invalid joint and one with fewer than two present views are zeros."""
    b, v, j = kp.shape[:3]
    x0, err0, inl0 = np.zeros((b, j, 3)), np.zeros((b, j)), np.zeros((b, j), np.int32)
    for bi in range(b):
        for ji in range(j):
            views = np.flatnonzero(rc.present_views(d, bi, ji))
            if not d["valid"][bi, ji] or len(views) < 2:
                continue
            x0[bi, ji], err0[bi, ji], inl0[bi, ji] = geometry.triangulate_ransac(d["proj"][bi][views], kp[bi, views, ji].astype(np.float64),
                                                                               rc.N_ITERS, rc.EPS)
    return x0, err0, inl0


def run(name, c, out, stats):
    d = rc.build(c)
    for key in ("proj", "joints", "valid", "view_valid", "view_joint_valid", "weights"):
        if d[key] is not None:
            out[f"{name}/{key}"] = d[key]
    for kind in ("i64", "f32"):
        kp = d["kp_" + kind]
        x0, err0, inl0 = dlt_points(d, kp)
        r = ro.refine_batch(kp, d["proj"], x0, err0, rc.EPS, d["valid"], d["view_valid"], d["view_joint_valid"], d["weights"])
        xmin, gap = x0.copy(), np.zeros(x0.shape[:2])
        for bi in range(c["b"]):
            for ji in range(c["j"]):
                present = rc.present_views(d, bi, ji)
                if d["valid"][bi, ji] and present.sum() >= 2:
                    errs = np.array([ro.half_distance(d["proj"][bi, v], x0[bi, ji], kp[bi, v, ji].astype(np.float64)) for v in np.flatnonzero(present)])
                    assert np.abs(errs - rc.EPS).min() >= MARGIN, (name, kind, bi, ji)
                if r["joint_status"][bi, ji] == 0:
                    continue
                S = np.flatnonzero(r["support"][bi, :, ji])
                w = np.ones(len(S)) if d["weights"] is None else d["weights"][bi, S, ji].astype(np.float64)
                xmin[bi, ji], rel = ro.minimise_longdouble(d["proj"][bi, S], kp[bi, S, ji].astype(np.float64), w, r["keypoints_3d"][bi, ji])
                assert rel < 1e-16, (name, kind, bi, ji, rel)
                gap[bi, ji] = np.linalg.norm(r["keypoints_3d"][bi, ji] - xmin[bi, ji])
                stats.setdefault(c["v"], []).append((int(r["joint_status"][bi, ji]), gap[bi, ji], len(S)))
        p = f"{name}/{kind}/"
        out.update({p + "kp": kp, p + "x0": x0, p + "err0": err0, p + "inliers0": inl0, p + "support": r["support"],
                    p + "x": r["keypoints_3d"], p + "status": r["joint_status"], p + "joint_error": r["joint_error"],
                    p + "xmin": xmin, p + "gap_oracle": gap})
        if c["outlier"]:  # the moved view is in nobody's support set
            for bi in range(c["b"]):
                assert not r["support"][bi, bi % c["v"]].any(), (name, kind, bi)


def main():
    out, stats = {}, {}
    for name, c in rc.refine3d_cases().items():
        run(name, c, out, stats)
    fi = np.finfo(np.longdouble)
    out["meta/numpy_version"] = np.array(np.__version__)
    out["meta/longdouble"] = np.array([fi.bits, fi.nmant, fi.precision], np.int64)
    out["meta/longdouble_eps"] = np.array(float(fi.eps))
    assert fi.nmant >= 63, "np.longdouble is no wider than float64 here: the minimum would be no better than the oracle"
    np.savez_compressed(rc.GOLDEN, **out)
    for v, rows in sorted(stats.items()):
        it, gaps = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        print(f"V={v:2d}: {len(rows):3d} refined problems, iterations {np.abs(it).min()}..{np.abs(it).max()} ({(it < 0).sum()} at the cap), "
              f"gap_oracle max {gaps.max():.2e} mm median {np.median(gaps):.2e} mm -> tolerance {4 * gaps.max():.2e} mm")
    print("wrote", rc.GOLDEN, os.path.getsize(rc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

"""numpy restatement of Pillow 12.2.0's Image.rotate(angle, resample=BICUBIC) on a mode-"F" image, the rule csrc/augment.hip's
aug_rotate_maps_kernel implements (ImagingGenericTransform with affine_transform and bicubic_filter32F), and of the point form
utils.augmentation.rotate_points.  Written from Pillow's behaviour, independent of the package under test.

  coordinates   xin = p0 (x + 0.5) + p1 (y + 0.5) + p2, yin likewise, float64, every operation rounded on its own; outside [0, w) x [0, h)
                the output is +0.0f; else subtract 0.5, floor, taps f - 1 .. f + 2 clamped to the map
  along a row   the four taps are float32 and the coefficient sums are float32 (C's float + float), left to right:
                p2 = -v1 + v3, p3 = 2 (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4; widened, v = v2 + d (p2 + d (p3 + d p4)) in float64
  across rows   the same expression with float64 taps (the row results) and float64 sums
  result        one cast to float32, no clip
"""
import math

import numpy as np


def coefficients(angle, w, h):
    """PIL.Image.Image.rotate's matrix for the default centre (output pixel centre -> input position); None where Pillow copies."""
    angle = angle % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _cubic(v1, v2, v3, v4, d, sums):
    """Geometry.c's BICUBIC with the coefficient sums in the taps' own type (float32 along a row, float64 across rows)."""
    two = sums(2)
    p2 = -v1 + v3
    p3 = two * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    f = np.float64
    return v2.astype(f) + d * (p2.astype(f) + d * (p3.astype(f) + d * p4.astype(f)))


def rotate_map(m, angle, row_sums=np.float32):
    """One (h, w) float32 map through Image.rotate(angle, BICUBIC).  row_sums=np.float64 gives the all-float64 variant (NOT Pillow's:
    the tests use it to show that their inputs tell the two apart)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    h, w = m.shape
    c = coefficients(float(angle), w, h)
    if c is None:
        return m.copy()
    yy, xx = np.mgrid[0:h, 0:w]
    xc, yc = xx + 0.5, yy + 0.5
    with np.errstate(all="ignore"):
        xin = c[0] * xc + c[1] * yc + c[2]
        yin = c[3] * xc + c[4] * yc + c[5]
        inside = (xin >= 0.0) & (yin >= 0.0) & (xin < w) & (yin < h)
        xin, yin = xin - 0.5, yin - 0.5
        fx, fy = np.floor(xin), np.floor(yin)
        dx, dy = xin - fx, yin - fy
        fx, fy = fx.astype(np.int64), fy.astype(np.int64)
        xs = [np.clip(fx - 1 + t, 0, w - 1) for t in range(4)]
        rows = []
        for t in range(4):
            ys = np.clip(fy - 1 + t, 0, h - 1)
            taps = [m[ys, x].astype(row_sums) for x in xs]
            rows.append(_cubic(taps[0], taps[1], taps[2], taps[3], dx, row_sums))
        out = _cubic(rows[0], rows[1], rows[2], rows[3], dy, np.float64).astype(np.float32)
    out[~inside] = 0.0
    return out


def rotate_maps(maps, angles, row_sums=np.float32):
    """Every (h, w) map of an array (..., h, w) through the angles in order."""
    maps = np.asarray(maps, dtype=np.float32)
    out = np.empty_like(maps)
    for idx in np.ndindex(maps.shape[:-2]):
        m = maps[idx]
        for a in angles:
            m = rotate_map(m, a, row_sums)
        out[idx] = m
    return out


def pillow_rotate_map(m, angle):
    """The same through Pillow itself."""
    from PIL import Image

    return np.asarray(Image.fromarray(np.ascontiguousarray(m, dtype=np.float32)).rotate(angle, resample=Image.BICUBIC)).copy()


def point_through(x, y, angle, w, h):
    """Where the content at (x, y) of a w x h image is after rotate(angle): the solution of the forward map's 2 x 2 system
    (numpy.linalg.solve), float64."""
    c = coefficients(float(angle), w, h)
    if c is None:
        return float(x), float(y)
    s = np.linalg.solve(np.array([[c[0], c[1]], [c[3], c[4]]]), np.array([x + 0.5 - c[2], y + 0.5 - c[5]]))
    return float(s[0] - 0.5), float(s[1] - 0.5)

"""
``myolo.measure`` -- per-instance measurements of detection masks: the record of 13 exact integer sums over a pasted
mask that MaskYOLO.detect(measure=True) takes on the device (Net.measure_masks, myolo_measure_masks), its statement on the host
(measure_dense: what the device is held to, integer for integer), and what is derived from it (properties, table, write_csv).  numpy only.

The record of one mask m(x, y), x the column and y the row (pixel indices), 0 outside its h x w frame:

    0  area            number of set pixels
    1  visible_area    set pixels that no EARLIER mask of the same image holds (the order of the last axis / of the slots)
    2  sx, 3 sy        sum of x, of y over the set pixels
    4  sxx, 5 syy, 6 sxy    sum of x*x, y*y, x*y
    7  perimeter       unit edges between a set pixel and a 4-neighbour that is 0 or outside the frame
    8  quads           positions (x, y) with m(x,y) & m(x+1,y) & m(x,y+1) & m(x+1,y+1)
    9..12  x1, y1, x2, y2   the tight box of the set pixels, far corner exclusive (extract_bboxes' order); zeros for an empty mask

With h, w <= LIMIT every word fits int64 (sxx <= h*w*w^2 < 2^61).  pairs = (4*area - perimeter) / 2 is the number of 4-adjacent set pairs and
euler_number = area - pairs + quads the number of 4-connected pieces minus the number of holes: #outer loops - #hole loops of contour.trace.
"""
import csv
import math
from fractions import Fraction

import numpy as np

WORDS = 13
FIELDS = ("area", "visible_area", "sx", "sy", "sxx", "syy", "sxy", "perimeter", "quads", "x1", "y1", "x2", "y2")
LIMIT = 32768             # the largest h or w: beyond it sxx and sxy may leave int64

TABLE_FIELDS = ("image", "instance", "class_id", "score", "area", "visible_area", "length", "width", "orientation", "perimeter", "euler_number",
                "bbox", "centroid")


def measure_dense(full_masks):
    """bool [h,w,n] (detect()'s full_masks) -> int64 [n,13]: the record of every plane, visible_area in the order of the last axis.
    ValueError for h or w > LIMIT."""
    m = np.asarray(full_masks)
    if m.ndim != 3:
        raise ValueError("measure_dense: a [h,w,n] array of masks is expected (got shape %s)" % (tuple(m.shape),))
    m = m.astype(bool)
    h, w, n = m.shape
    if h > LIMIT or w > LIMIT:
        raise ValueError("measure_dense: a %d x %d frame, above %d on a side: the second moments may leave int64" % (h, w, LIMIT))
    out = np.zeros((n, WORDS), np.int64)
    covered = np.zeros((h, w), bool)
    for k in range(n):
        p = m[:, :, k]
        y, x = np.nonzero(p)
        y, x = y.astype(np.int64), x.astype(np.int64)
        r = out[k]
        r[0] = y.size
        r[1] = np.count_nonzero(p & ~covered)
        covered |= p
        r[2], r[3] = x.sum(), y.sum()
        r[4], r[5], r[6] = (x * x).sum(), (y * y).sum(), (x * y).sum()
        z = np.zeros((h + 2, w + 2), bool)                 # the frame's zero surround: an edge of the frame bounds like a clear neighbour
        z[1:-1, 1:-1] = p
        r[7] = np.count_nonzero(z[1:, :] != z[:-1, :]) + np.count_nonzero(z[:, 1:] != z[:, :-1])
        r[8] = np.count_nonzero(p[:-1, :-1] & p[:-1, 1:] & p[1:, :-1] & p[1:, 1:])
        if y.size:
            r[9], r[10], r[11], r[12] = x.min(), y.min(), x.max() + 1, y.max() + 1
    return out


def euler_number(raw):
    """int64 [...,13] -> area - pairs + quads, pairs = (4*area - perimeter) / 2 (always an integer)"""
    raw = np.asarray(raw, np.int64)
    return raw[..., 0] - (4 * raw[..., 0] - raw[..., 7]) // 2 + raw[..., 8]


def _moments(rec):
    """one record as Python ints -> (cx, cy, major, minor, orientation, eccentricity): every quotient formed exactly (A * sxx leaves 64 bits) and
    rounded to float64 once, then the square roots and the arc tangent"""
    A, sx, sy, sxx, syy, sxy = (int(v) for v in (rec[0], rec[2], rec[3], rec[4], rec[5], rec[6]))
    if A == 0:
        return float("nan"), float("nan"), 0.0, 0.0, 0.0, 0.0
    mxx, myy, mxy = Fraction(A * sxx - sx * sx, A * A), Fraction(A * syy - sy * sy, A * A), Fraction(A * sxy - sx * sy, A * A)
    half_sum = float((mxx + myy) / 2)
    root = math.sqrt(float(((mxx - myy) / 2) ** 2 + mxy ** 2))
    lam_hi, lam_lo = half_sum + root, max(half_sum - root, 0.0)            # (lam- >= 0 exactly; a rounding may leave it just below)
    orientation = 0.5 * math.atan2(float(2 * mxy), float(mxx - myy))
    ecc = math.sqrt(max(1.0 - lam_lo / lam_hi, 0.0)) if lam_hi > 0.0 else 0.0
    return float(Fraction(sx, A)), float(Fraction(sy, A)), 4.0 * math.sqrt(lam_hi), 4.0 * math.sqrt(lam_lo), orientation, ecc


def properties(raw):
    """int64 [n,13] records -> a dict of arrays over the n instances: "raw" (the records), "area", "visible_area", "perimeter", "euler_number"
    (int64 [n]), "bbox" (int32 [n,4]: x1, y1, x2, y2), and in float64 "centroid" [n,2] = (sx/A, sy/A) in pixel-index coordinates,
    "major_axis_length" / "minor_axis_length" = 4 sqrt(lam+-), lam+- the eigenvalues of the central second moments mu = (A*s.. - s.*s.)/A^2
    (regionprops' ellipse of equal normalised second moments, without its 1/12 term), "orientation" = 0.5 atan2(2 mu_xy, mu_xx - mu_yy) radians
    (the major axis from +x towards +y, which is down the screen; 0 for an isotropic blob) and "eccentricity" = sqrt(1 - lam-/lam+) (0 when
    lam+ is 0; lam- is taken as 0 where a rounding leaves it below).  An empty mask has a NaN centroid and zeros elsewhere."""
    raw = np.ascontiguousarray(raw, dtype=np.int64)
    if raw.ndim != 2 or raw.shape[1] != WORDS:
        raise ValueError("properties: int64 [n,%d] records expected (got shape %s)" % (WORDS, tuple(raw.shape)))
    n = raw.shape[0]
    fl = np.array([_moments(rec) for rec in raw.tolist()], dtype=np.float64).reshape(n, 6)
    return {"raw": raw, "area": raw[:, 0].copy(), "visible_area": raw[:, 1].copy(), "perimeter": raw[:, 7].copy(),
            "euler_number": euler_number(raw), "bbox": raw[:, 9:13].astype(np.int32), "centroid": fl[:, 0:2].copy(),
            "major_axis_length": fl[:, 2].copy(), "minor_axis_length": fl[:, 3].copy(), "orientation": fl[:, 4].copy(),
            "eccentricity": fl[:, 5].copy()}


def table(results, names=None, scale=1.0):
    """detect(measure=True)'s result dicts -> one dict per instance, in order, with TABLE_FIELDS: image = names[i] (None: the index i),
    instance = its index within the image, class_id, score, and from "measurements": area, visible_area, length / width (the major / minor axis
    lengths), orientation (radians), perimeter, euler_number, bbox (x1, y1, x2, y2) and centroid (x, y).  scale = units per pixel: lengths,
    the perimeter and the coordinates of bbox and centroid are multiplied by it, areas by scale**2."""
    rows = []
    for i, r in enumerate(results):
        if "measurements" not in r:
            raise ValueError("table: result %d holds no \"measurements\" (detect(..., measure=True) adds them)" % i)
        p = r["measurements"]
        for k in range(len(r["class_ids"])):
            rows.append({"image": i if names is None else names[i], "instance": k, "class_id": int(r["class_ids"][k]),
                         "score": float(r["confidence_scores"][k]), "area": int(p["area"][k]) * scale ** 2,
                         "visible_area": int(p["visible_area"][k]) * scale ** 2, "length": float(p["major_axis_length"][k]) * scale,
                         "width": float(p["minor_axis_length"][k]) * scale, "orientation": float(p["orientation"][k]),
                         "perimeter": int(p["perimeter"][k]) * scale, "euler_number": int(p["euler_number"][k]),
                         "bbox": tuple(int(v) * scale for v in p["bbox"][k]), "centroid": tuple(float(v) * scale for v in p["centroid"][k])})
    return rows


CSV_COLUMNS = ("image", "instance", "class_id", "score", "area", "visible_area", "length", "width", "orientation", "perimeter", "euler_number",
               "bbox_x1", "bbox_y1", "bbox_x2", "bbox_y2", "centroid_x", "centroid_y")


def write_csv(path, rows):
    """table()'s rows as a CSV file with the header CSV_COLUMNS: bbox and centroid are spread over one column per coordinate, floats are
    written with repr (they read back to the same float64)"""
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(CSV_COLUMNS)
        for r in rows:
            flat = [r[c] for c in CSV_COLUMNS[:11]] + list(r["bbox"]) + list(r["centroid"])
            wr.writerow([repr(v) if isinstance(v, float) else v for v in flat])

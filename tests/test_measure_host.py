"""myolo/measure.py on the host: measure_dense -- the statement the device's records are held to -- against explicit Python-int
loops and against contour.trace (perimeter = length of the loops, area = their signed areas, Euler number = outer loops - holes), closed forms,
properties against a Fraction computation where a float64 product of the raw words goes wrong, invariance under translation, table / write_csv,
and detect.check_args(measure=True)."""
import csv
import math
from fractions import Fraction

import numpy as np
import pytest

from myolo import contour, detect
from myolo import measure as M
from myolo.config import make_config, ShapesConfig


def _loops(p):
    """the record of one bool [h,w] plane by explicit loops over Python ints (visible_area: the plane alone)"""
    h, w = p.shape
    get = lambda x, y: bool(p[y, x]) if 0 <= x < w and 0 <= y < h else False         # noqa: E731
    area = sx = sy = sxx = syy = sxy = per = quads = 0
    xs, ys = [], []
    for y in range(h):
        for x in range(w):
            if not get(x, y):
                continue
            area += 1
            sx, sy, sxx, syy, sxy = sx + x, sy + y, sxx + x * x, syy + y * y, sxy + x * y
            per += sum(not get(x + dx, y + dy) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)))
            quads += get(x + 1, y) and get(x, y + 1) and get(x + 1, y + 1)
            xs.append(x), ys.append(y)
    box = [min(xs), min(ys), max(xs) + 1, max(ys) + 1] if area else [0, 0, 0, 0]
    return [area, area, sx, sy, sxx, syy, sxy, per, quads] + box


def _random_masks():
    """sizes 1 .. 40 on either side at densities 0 .. 1, n in {1, 3}"""
    rng = np.random.default_rng(5)
    out = []
    for i in range(60):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        dens = (0.0, 1.0, 0.5)[i] if i < 3 else rng.random()
        out.append(rng.random((h, w, 1 if i % 2 else 3)) < dens)
    return out


MASKS = _random_masks()


def _loop_length(loop):
    q = np.asarray(loop, np.int64)
    return int(np.abs(q - np.roll(q, -1, axis=0)).sum())


def test_measure_dense_equals_the_loops():
    assert M.WORDS == 13 == len(M.FIELDS)
    for m in MASKS:
        got = M.measure_dense(m)
        assert got.dtype == np.int64 and got.shape == (m.shape[2], 13)
        seen = np.zeros(m.shape[:2], bool)
        for k in range(m.shape[2]):
            want = _loops(m[:, :, k])
            want[1] = int((m[:, :, k] & ~seen).sum())
            seen |= m[:, :, k]
            assert got[k].tolist() == want, (m.shape, k)


def test_visible_area_of_an_overlapping_stack():
    rng = np.random.default_rng(7)
    m = np.zeros((30, 41, 5), bool)
    m[2:20, 3:30, 0] = True
    m[10:28, 15:40, 1] = True
    m[:, :, 2] = m[:, :, 0]                                # a duplicated plane: nothing of it is visible
    m[:, :, 3] = rng.random((30, 41)) < 0.4
    m[5:8, 5:8, 4] = True                                  # wholly under plane 0
    r = M.measure_dense(m)
    assert r[:, 1].sum() == m.any(axis=2).sum()
    assert r[0, 1] == r[0, 0] and r[2, 1] == 0 and r[4, 1] == 0 and 0 < r[1, 1] < r[1, 0]
    assert np.array_equal(r[:, 0], m.sum(axis=(0, 1)))
    # the order of the last axis decides
    assert M.measure_dense(m[:, :, ::-1])[0, 1] == m[:, :, 4].sum()


def test_identities_against_contour_trace():
    n = 0
    for m in MASKS:
        r = M.measure_dense(m)
        euler = M.euler_number(r)
        for k in range(m.shape[2]):
            loops = contour.trace(m[:, :, k])
            areas = [contour.signed_area(l) for l in loops]
            assert r[k, 7] == sum(_loop_length(l) for l in loops), (m.shape, k)
            assert r[k, 0] == sum(areas), (m.shape, k)
            assert (4 * r[k, 0] - r[k, 7]) % 2 == 0
            assert euler[k] == sum(a > 0 for a in areas) - sum(a < 0 for a in areas), (m.shape, k)
            n += len(loops)
    assert n > 500


def _one(p):
    return M.properties(M.measure_dense(np.asarray(p, bool)[:, :, None]))


@pytest.mark.parametrize("a,b", [(7, 3), (3, 7), (5, 5), (1, 9), (12, 1)])
def test_rectangle(a, b):
    """a wide, b high, at (4, 2) of a 20 x 20 frame"""
    p = np.zeros((20, 20), bool)
    p[2:2 + b, 4:4 + a] = True
    q = _one(p)
    assert q["area"][0] == a * b and q["perimeter"][0] == 2 * (a + b) and q["raw"][0, 8] == (a - 1) * (b - 1) and q["euler_number"][0] == 1
    assert q["bbox"].dtype == np.int32 and q["bbox"][0].tolist() == [4, 2, 4 + a, 2 + b]
    assert np.allclose(q["centroid"][0], [4 + (a - 1) / 2.0, 2 + (b - 1) / 2.0], rtol=0, atol=1e-12)
    assert q["major_axis_length"][0] == pytest.approx(4 * math.sqrt((max(a, b) ** 2 - 1) / 12.0), rel=1e-14, abs=1e-14)
    assert q["minor_axis_length"][0] == pytest.approx(4 * math.sqrt((min(a, b) ** 2 - 1) / 12.0), rel=1e-14, abs=1e-14)
    if a > b:
        assert q["orientation"][0] == 0.0
    elif a < b:
        assert q["orientation"][0] == pytest.approx(math.pi / 2, rel=1e-15)
    else:
        assert q["orientation"][0] == 0.0 and q["eccentricity"][0] == 0.0          # isotropic
    if min(a, b) == 1:
        assert q["eccentricity"][0] == 1.0 and q["minor_axis_length"][0] == 0.0


def test_small_closed_forms():
    p = np.zeros((5, 6), bool)
    p[3, 2] = True
    q = _one(p)                                            # one pixel
    assert q["area"][0] == 1 and q["perimeter"][0] == 4 and q["euler_number"][0] == 1 and q["major_axis_length"][0] == 0.0
    assert q["minor_axis_length"][0] == 0.0 and q["eccentricity"][0] == 0.0 and q["centroid"][0].tolist() == [2.0, 3.0]
    assert q["bbox"][0].tolist() == [2, 3, 3, 4]
    p[2, 3] = True
    q = _one(p)                                            # two diagonal pixels: two 4-connected pieces
    assert q["euler_number"][0] == 2 and q["perimeter"][0] == 8 and q["raw"][0, 8] == 0
    assert q["orientation"][0] == pytest.approx(-math.pi / 4, rel=1e-15)           # up and to the right on the screen: from +x towards -y
    ring = np.ones((6, 7), bool)
    ring[2:4, 2:5] = False
    q = _one(ring)
    assert q["euler_number"][0] == 0 and q["area"][0] == 36 and q["perimeter"][0] == 2 * (6 + 7) + 2 * (2 + 3)
    yy, xx = np.mgrid[:6, :8]
    q = _one((yy + xx) % 2 == 0)                           # checkerboard: every pixel a piece, every edge a boundary
    assert q["area"][0] == 24 and q["perimeter"][0] == 96 and q["raw"][0, 8] == 0 and q["euler_number"][0] == 24
    q = _one(np.zeros((4, 4), bool))
    assert not q["raw"].any() and np.isnan(q["centroid"]).all() and q["bbox"][0].tolist() == [0, 0, 0, 0]
    for key in ("major_axis_length", "minor_axis_length", "orientation", "eccentricity", "area", "perimeter", "euler_number"):
        assert q[key][0] == 0, key
    full = _one(np.ones((9, 4), bool))                     # the frame's own edge bounds like a clear neighbour
    assert full["perimeter"][0] == 26 and full["euler_number"][0] == 1
    assert M.properties(np.zeros((0, 13), np.int64))["centroid"].shape == (0, 2)
    with pytest.raises(ValueError):
        M.measure_dense(np.zeros((1, 32769, 1), bool))
    with pytest.raises(ValueError):
        M.properties(np.zeros((2, 12), np.int64))


def _exact(rec):
    """the float fields of one record, every quotient exact (Fraction) and rounded once"""
    A, _, sx, sy, sxx, syy, sxy = (int(v) for v in rec[:7])
    mxx, myy, mxy = Fraction(A * sxx - sx * sx, A * A), Fraction(A * syy - sy * sy, A * A), Fraction(A * sxy - sx * sy, A * A)
    root = math.sqrt(float(((mxx - myy) / 2) ** 2 + mxy ** 2))
    hi, lo = float((mxx + myy) / 2) + root, max(float((mxx + myy) / 2) - root, 0.0)
    return (float(Fraction(sx, A)), float(Fraction(sy, A)), 4 * math.sqrt(hi), 4 * math.sqrt(lo),
            0.5 * math.atan2(float(2 * mxy), float(mxx - myy)), math.sqrt(max(1 - lo / hi, 0.0)) if hi > 0 else 0.0)


def test_properties_near_2_to_60_equal_the_fraction_computation():
    """records of long thin blobs far from the origin of a 32768 x 32768 frame: A * syy and sy * sy are ~2^58 and agree in their leading bits, so
    a float64 product of the raw words leaves the small central moment with an error of ~1e-8 of itself, four orders above the 1e-12 the device
    path is compared at; properties forms the quotient exactly"""
    recs = []
    for (a, b, x0, y0) in ((3000, 7, 29000, 32761), (5, 3000, 32763, 29000), (1, 1, 32767, 32767), (9, 4, 32700, 32750)):
        xs, ys = np.meshgrid(np.arange(x0, x0 + a, dtype=np.int64), np.arange(y0, y0 + b, dtype=np.int64))
        xs, ys = xs.ravel()[:-1] if a * b > 1 else xs.ravel(), ys.ravel()[:-1] if a * b > 1 else ys.ravel()      # (not quite a rectangle)
        recs.append([xs.size, xs.size, xs.sum(), ys.sum(), (xs * xs).sum(), (ys * ys).sum(), (xs * ys).sum(), 0, 0, x0, y0, x0 + a, y0 + b])
    # the full 32768 x 32768 frame, the largest record there is: sxx = 2^60 / 3
    n = 32768
    s1, s2 = n * (n - 1) // 2, (n - 1) * n * (2 * n - 1) // 6
    recs.append([n * n, n * n, n * s1, n * s1, n * s2, n * s2, s1 * s1, 4 * n, (n - 1) ** 2, 0, 0, n, n])
    raw = np.array(recs, np.int64)
    assert raw[-1, 4] > 2 ** 58
    q = M.properties(raw)
    naive_wrong = 0
    for i, rec in enumerate(raw.tolist()):
        cx, cy, major, minor, ori, ecc = _exact(rec)
        assert q["centroid"][i].tolist() == [cx, cy]
        assert q["major_axis_length"][i] == major and q["minor_axis_length"][i] == minor, i
        assert q["orientation"][i] == ori and q["eccentricity"][i] == ecc, i
        f = [float(v) for v in rec]
        for s, ss in ((2, 4), (3, 5)):
            naive, exact = (f[0] * f[ss] - f[s] * f[s]) / (f[0] * f[0]), float(Fraction(rec[0] * rec[ss] - rec[s] ** 2, rec[0] ** 2))
            naive_wrong += abs(naive - exact) > 1e-10 * exact
    assert naive_wrong >= 2                                 # the case holds what it is meant to hold
    assert q["major_axis_length"][-1] == pytest.approx(4 * math.sqrt((n * n - 1) / 12.0), rel=1e-15)
    assert q["major_axis_length"][3] == pytest.approx(4 * math.sqrt((81 - 1) / 12.0), rel=0.05)


def test_translation_leaves_the_shape_fields():
    rng = np.random.default_rng(9)
    blob = rng.random((13, 17)) < 0.6
    a, b = np.zeros((64, 80), bool), np.zeros((64, 80), bool)
    a[1:14, 2:19] = blob
    b[40:53, 55:72] = blob
    qa, qb = _one(a), _one(b)
    for key in ("area", "perimeter", "euler_number"):
        assert qa[key][0] == qb[key][0], key
    for key in ("major_axis_length", "minor_axis_length", "orientation", "eccentricity"):
        assert qa[key][0] == pytest.approx(qb[key][0], rel=1e-12, abs=1e-12), key
    assert np.allclose(qb["centroid"][0] - qa["centroid"][0], [53, 39], rtol=0, atol=1e-9)
    assert (qb["bbox"][0] - qa["bbox"][0]).tolist() == [53, 39, 53, 39]


def test_table_and_write_csv_round_trip(tmp_path):
    m0 = np.zeros((20, 30, 2), bool)
    m0[2:8, 3:15, 0] = True
    m0[5:12, 10:14, 1] = True
    m1 = np.zeros((10, 10, 1), bool)
    m1[1:4, 1:9, 0] = True
    results = []
    for m, ids, sc in ((m0, [2, 1], [0.9, 0.8]), (m1, [3], [0.7]), (np.zeros((5, 5, 0), bool), [], [])):
        results.append({"class_ids": np.array(ids, np.int32), "confidence_scores": np.array(sc, np.float32),
                        "measurements": M.properties(M.measure_dense(m))})
    rows = M.table(results, names=["a.jpg", "b.jpg", "c.jpg"], scale=0.5)
    assert [(r["image"], r["instance"], r["class_id"]) for r in rows] == [("a.jpg", 0, 2), ("a.jpg", 1, 1), ("b.jpg", 0, 3)]
    assert all(set(r) == set(M.TABLE_FIELDS) for r in rows)
    assert rows[0]["area"] == 72 * 0.25 and rows[1]["visible_area"] == (28 - 12) * 0.25 and rows[0]["perimeter"] == 36 * 0.5
    assert rows[0]["length"] == pytest.approx(0.5 * 4 * math.sqrt(143 / 12.0)) and rows[0]["width"] == pytest.approx(0.5 * 4 * math.sqrt(35 / 12.0))
    assert rows[2]["bbox"] == (0.5, 0.5, 4.5, 2.0) and rows[2]["centroid"] == (2.25, 1.0) and rows[2]["euler_number"] == 1
    assert rows[0]["score"] == float(np.float32(0.9))
    plain = M.table(results)
    assert [r["image"] for r in plain] == [0, 0, 1] and plain[0]["area"] == 72 and plain[0]["bbox"] == (3, 2, 15, 8)
    path = str(tmp_path / "m.csv")
    M.write_csv(path, rows)
    with open(path, newline="") as f:
        back = list(csv.DictReader(f))
    assert len(back) == 3 and tuple(back[0].keys()) == M.CSV_COLUMNS
    for r, s in zip(rows, back):
        assert s["image"] == r["image"] and int(s["instance"]) == r["instance"] and int(s["class_id"]) == r["class_id"]
        for key in ("score", "area", "visible_area", "length", "width", "orientation", "perimeter"):
            assert float(s[key]) == r[key], key
        assert int(s["euler_number"]) == r["euler_number"]
        assert tuple(float(s[c]) for c in ("bbox_x1", "bbox_y1", "bbox_x2", "bbox_y2")) == r["bbox"]
        assert (float(s["centroid_x"]), float(s["centroid_y"])) == r["centroid"]
    with pytest.raises(ValueError):
        M.table([{"class_ids": np.zeros(0, np.int32), "confidence_scores": np.zeros(0, np.float32)}])


def test_check_args_refuses_measure_with_selected_only():
    img = [np.zeros((8, 8, 3), np.uint8)]
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1)
    detect.check_args(cfg, img, "image", "dense", False, None, measure=True)
    detect.check_args(cfg, img, "image", "rle", False, 40, True)
    cfg2 = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    detect.check_args(cfg2, img, "image", "dense", False, None)
    with pytest.raises(ValueError, match="measure=True"):
        detect.check_args(cfg2, img, "image", "dense", False, None, measure=True)

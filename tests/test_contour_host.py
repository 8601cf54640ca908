"""Mask outlines on the host (myolo/contour.py): the tracer's known answers, its order rules, the exact round trip through the
polygon fill, simplify's bound, and the two writers that take mask_format="polygon" results (via.via_annotations, rle.coco_results)."""
import json

import numpy as np
import pytest

from myolo import contour
from myolo.polygon import polygon_mask


def _lists(loops):
    return [l.tolist() for l in loops]


def _fill(loops, shape):
    """the XOR over the loops of the polygon fill at pixel centres"""
    out = np.zeros(shape, bool)
    for l in loops:
        out ^= polygon_mask(l[:, 1] - 0.5, l[:, 0] - 0.5, shape)
    return out


def _ring():
    m = np.ones((3, 3), bool)
    m[1, 1] = False
    return m


def _random_masks():
    rng = np.random.default_rng(7)
    out = []
    for i in range(60):
        h, w = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        out.append(rng.random((h, w)) < (0.25, 0.5, 0.75)[i % 3])
    yy, xx = np.mgrid[:7, :9]
    out.append((yy + xx) % 2 == 0)
    blob = np.zeros((12, 11), bool)
    blob[2:10, 1:9] = True
    blob[4:7, 3:6] = False
    blob[5, 4] = True                                  # an island inside the hole
    out.append(blob)
    return out


def test_known_answers():
    assert _lists(contour.trace(np.array([[1, 0], [0, 1]]))) == [[[0, 0], [1, 0], [1, 1], [0, 1]], [[1, 1], [2, 1], [2, 2], [1, 2]]]
    assert _lists(contour.trace(_ring())) == [[[0, 0], [3, 0], [3, 3], [0, 3]], [[1, 1], [1, 2], [2, 2], [2, 1]]]
    assert _lists(contour.trace(np.ones((1, 1), bool))) == [[[0, 0], [1, 0], [1, 1], [0, 1]]]
    assert _lists(contour.trace(np.ones((4, 6), bool))) == [[[0, 0], [6, 0], [6, 4], [0, 4]]]
    assert contour.trace(np.zeros((5, 3), bool)) == []
    # the other diagonal: the two pixels stay apart too
    assert _lists(contour.trace(np.array([[0, 1], [1, 0]]))) == [[[1, 0], [2, 0], [2, 1], [1, 1]], [[0, 1], [1, 1], [1, 2], [0, 2]]]
    for l in contour.trace(_ring()):
        assert l.dtype == np.int32 and l.ndim == 2 and l.shape[1] == 2
    with pytest.raises(ValueError):
        contour.trace(np.zeros((2, 2, 2), bool))


def test_checkerboard_has_four_vertices_a_pixel():
    yy, xx = np.mgrid[:7, :9]
    board = (yy + xx) % 2 == 0
    loops = contour.trace(board)
    assert len(loops) == board.sum() == 32 and all(len(l) == 4 for l in loops)
    ys, xs = np.nonzero(board)                          # row-major: the order of the loops' smallest keys
    for l, y, x in zip(loops, ys, xs):
        assert l.tolist() == [[x, y], [x + 1, y], [x + 1, y + 1], [x, y + 1]]


def test_round_trip_through_the_polygon_fill_is_exact():
    for m in _random_masks():
        loops = contour.trace(m)
        assert np.array_equal(_fill(loops, m.shape), m), m.astype(int)
        # the signed areas add up to the pixel count: outer loops positive, holes negative
        assert sum(contour.signed_area(l) for l in loops) == m.sum()


def test_loop_order_and_start_vertex():
    for m in _random_masks():
        h, w = m.shape
        loops = contour.trace(m)
        firsts = []
        for l in loops:
            n = len(l)
            assert n >= 4 and n % 2 == 0
            step = np.roll(l, -1, axis=0) - l
            assert ((step == 0).sum(axis=1) == 1).all()                            # axis-parallel edges of non-zero length
            horizontal = step[:, 1] == 0
            assert (horizontal != np.roll(horizontal, 1)).all()                    # every vertex is a turn
            assert (l[:, 0] >= 0).all() and (l[:, 0] <= w).all() and (l[:, 1] >= 0).all() and (l[:, 1] <= h).all()
            # the first vertex is the loop's smallest corner in (Y, X) order; an outer loop leaves it heading east, a hole heading south
            order = np.lexsort((l[:, 0], l[:, 1]))
            assert order[0] == 0 or (l[order[0]] == l[0]).all()
            area = contour.signed_area(l)
            assert area != 0 and ((step[0] > 0).tolist() == ([True, False] if area > 0 else [False, True]))
            firsts.append((int(l[0, 1]), int(l[0, 0]), 0 if area > 0 else 1))
        assert firsts == sorted(firsts)
        assert len(contour.outer_loops(loops)) == sum(contour.signed_area(l) > 0 for l in loops)
    assert [contour.signed_area(l) for l in contour.trace(_ring())] == [9.0, -1.0]
    assert _lists(contour.outer_loops(contour.trace(_ring()))) == [[[0, 0], [3, 0], [3, 3], [0, 3]]]


def _disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[:h, :w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def test_simplify():
    loop = contour.trace(_disc(40, 44, 19, 22, 15))[0]
    assert len(loop) > 40
    same = contour.simplify(loop, 0)
    assert same.dtype == loop.dtype and np.array_equal(same, loop)
    with pytest.raises(ValueError):
        contour.simplify(loop, -1.0)
    last = len(loop)
    for tol in (0.5, 1.0, 2.5):
        s = contour.simplify(loop, tol)
        assert s.dtype == loop.dtype and 3 <= len(s) <= last and (s[0] == loop[0]).all()
        last = len(s)
        # a subsequence of the loop ...
        at = [int(np.flatnonzero((loop == p).all(axis=1))[0]) for p in s]
        assert at == sorted(at) and len(set(at)) == len(at)
        # ... and every vertex of the loop within tol of the simplified outline
        closed = np.concatenate([s, s[:1]])
        dist = np.min([contour._distance(loop, closed[i], closed[i + 1]) for i in range(len(s))], axis=0)
        assert dist.max() <= tol + 1e-9, (tol, dist.max())
    assert len(contour.simplify(loop, 2.5)) < len(loop) // 2
    square = contour.trace(np.ones((5, 5), bool))[0]
    assert np.array_equal(contour.simplify(square, 1.0), square)


def _results():
    """two images' worth of mask_format="polygon" results, made from masks: (results, masks)"""
    a = np.stack([_disc(30, 40, 12, 15, 9), _disc(30, 40, 20, 30, 6)], axis=2)
    ring = np.zeros((25, 20), bool)
    ring[3:20, 2:17] = True
    ring[8:12, 6:10] = False
    two = np.zeros((25, 20), bool)
    two[1:5, 1:6] = True
    two[10:20, 8:15] = True
    b = np.stack([ring, two], axis=2)
    out = []
    for m, ids in ((a, [1, 2]), (b, [2, 1])):
        n = m.shape[2]
        out.append({"bboxes": np.zeros((n, 4), np.float32), "class_ids": np.asarray(ids, np.int32),
                    "confidence_scores": np.linspace(0.9, 0.5, n).astype(np.float32),
                    "polygons": [contour.trace(m[:, :, i]) for i in range(n)]})
    return out, [a, b]


def test_via_annotations_round_trip_through_load_via(tmp_path):
    from PIL import Image
    from myolo.via import load_via, via_annotations
    results, masks = _results()
    names = ["a.png", "b.png"]
    folder = tmp_path / "data" / "val"
    folder.mkdir(parents=True)
    for name, m in zip(names, masks):
        Image.fromarray(np.zeros(m.shape[:2] + (3,), np.uint8)).save(str(folder / name))
    ann = via_annotations(results, names, class_names=["BG", "soup", "rice"])
    text = json.dumps(ann)                                                   # ready for json.dump
    (folder / "via_pred_annotation.json").write_text(text)
    assert [e["filename"] for e in ann.values()] == names
    # image a: two hole-free single-piece masks -> one region each, filled back exactly
    ds = load_via(str(tmp_path / "data"), "val", class_attribute="class", class_names=["soup", "rice"])
    got, ids = ds.load_mask(0)
    assert ids.tolist() == [1, 2] and np.array_equal(got, masks[0])
    ra = ann["a.png-1"]["regions"]
    assert [r["region_attributes"]["instance"] for r in ra] == [0, 1] and [r["region_attributes"]["class"] for r in ra] == ["soup", "rice"]
    assert ra[0]["region_attributes"]["score"] == pytest.approx(0.9) and ra[0]["shape_attributes"]["name"] == "polygon"
    first = results[0]["polygons"][0][0]
    assert ra[0]["shape_attributes"]["all_points_x"] == (first[:, 0] - 0.5).tolist()
    assert ra[0]["shape_attributes"]["all_points_y"] == (first[:, 1] - 0.5).tolist()
    # image b: the ring loses its hole (one region, the filled rectangle), the two-piece mask gives two regions of instance 1
    got, ids = ds.load_mask(1)
    rb = ann["b.png-1"]["regions"]
    assert [r["region_attributes"]["instance"] for r in rb] == [0, 1, 1] and ids.tolist() == [2, 1, 1]
    filled = masks[1][:, :, 0].copy()
    filled[8:12, 6:10] = True
    assert np.array_equal(got[:, :, 0], filled) and np.array_equal(got[:, :, 1] | got[:, :, 2], masks[1][:, :, 1])
    # class ids as strings without names; a tolerance shortens the outlines; the argument checks
    assert via_annotations(results, names)["a.png-1"]["regions"][1]["region_attributes"]["class"] == "2"
    coarse = via_annotations(results, names, tolerance=1.5)["a.png-1"]["regions"][0]["shape_attributes"]["all_points_x"]
    assert 3 <= len(coarse) < len(ra[0]["shape_attributes"]["all_points_x"])
    with pytest.raises(ValueError):
        via_annotations(results, names[:1])
    with pytest.raises(ValueError):
        via_annotations([{"class_ids": [], "full_masks": None}], ["x.png"])


def test_coco_results_on_polygon_results():
    from myolo import rle
    results, masks = _results()
    rows = rle.coco_results(results, [7, np.int64(8)], category_ids=[0, 11, 22])
    json.dumps(rows)
    assert [(r["image_id"], r["category_id"]) for r in rows] == [(7, 11), (7, 22), (8, 22), (8, 11)]
    for r, m in zip(rows, (masks[0][:, :, 0], masks[0][:, :, 1], masks[1][:, :, 0], masks[1][:, :, 1])):
        ys, xs = np.nonzero(m)
        assert r["bbox"] == [float(xs.min()), float(ys.min()), float(xs.max() + 1 - xs.min()), float(ys.max() + 1 - ys.min())]
        assert set(r) == {"image_id", "category_id", "segmentation", "bbox", "area", "score"}
        assert all(isinstance(v, int) for part in r["segmentation"] for v in part)
    outer = contour.outer_loops(results[0]["polygons"][0])
    assert rows[0]["segmentation"] == [outer[0].reshape(-1).tolist()] and rows[0]["area"] == float(masks[0][:, :, 0].sum())
    assert len(rows[2]["segmentation"]) == 1 and rows[2]["area"] == 17.0 * 15.0            # the hole is dropped
    assert len(rows[3]["segmentation"]) == 2 and rows[3]["area"] == float(masks[1][:, :, 1].sum())
    assert rows[1]["score"] == pytest.approx(0.5)


def test_check_args_takes_polygon():
    from myolo import detect
    from myolo.config import make_config, ShapesConfig
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1)
    im = np.zeros((40, 30, 3), np.uint8)
    for render in (False, True):
        detect.check_args(cfg, [im], "image", "polygon", render)
    with pytest.raises(ValueError):
        detect.check_args(cfg, [im], "image", "png", False)
    only = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    with pytest.raises(ValueError, match="DETECT_MASKS_FOR_SELECTED_ONLY"):
        detect.check_args(only, [im], "image", "polygon", False)
    detect.check_args(only, [im], "image", "dense", False)


def test_the_entry_is_declared_and_bound():
    import os
    import re
    from myolo import _ext as X
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "myolo_hip_internal.h")).read(), flags=re.S)
    decl = dict(re.findall(r"\bint\s+(myolo_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S))
    assert len(X.SIGS["myolo_contour_masks"]) == decl["myolo_contour_masks"].count(",") + 1 == 19
    assert "myolo_contour_masks_ws_bytes" in X.exported_symbols()
    assert "myolo_contour_masks" not in open(os.path.join(root, "include", "myolo_hip.h")).read()
    lib = X.load()
    assert lib.myolo_contour_masks(*[None if t is X.P else 0 for t in X.SIGS["myolo_contour_masks"]]) == -1
    assert lib.myolo_last_error_string().startswith(b"contour_masks:")
    # the workspace planner is host arithmetic: it does not grow with the frame's area (<= 64 * B * K bytes per extra row or column at a fixed cap)
    B, K, cap = 4, 10, 1 << 16
    base = X.contour_masks_ws_bytes(B, K, 416, 416, cap)
    assert base >= 4 * B * K * 417
    for h, w in ((417, 416), (416, 417), (3000, 4000), (4000, 3000), (1, 1)):
        grown = X.contour_masks_ws_bytes(B, K, h, w, cap)
        assert grown - base <= 64 * B * K * (max(h - 416, 0) + max(w - 416, 0)), (h, w)
    assert X.contour_masks_ws_bytes(1, 1, 3000, 4000, 16) - X.contour_masks_ws_bytes(1, 1, 2999, 4000, 16) <= 64
    assert X.contour_masks_ws_bytes(B, K, 416, 416, 2 * cap) > base

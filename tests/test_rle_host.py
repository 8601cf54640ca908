"""myolo/rle.py on the host: COCO's run-length format as DESIGN.md section 15 states it -- known answers (the first is pycocotools' own test
vector), round trips, canonical form, column-major order, area / bbox against numpy, and coco_results through json."""
import json

import numpy as np
import pytest

from myolo import rle

KNOWN = [
    ([6, 1, 40, 4, 5, 4, 5, 4, 21], "61X13mN000`0"),
    ([0, 5, 3], "053"),
    ([173056], "PPY5"),
    ([100000, 2000, 3, 70000, 1], "PeQ3`n13P]R2N"),
]


def _mask_4x3():
    m = np.zeros((4, 3), np.uint8)
    m[1:3, 0] = 1
    m[0, 1] = 1
    m[3, 2] = 1
    return m


@pytest.mark.parametrize("counts,string", KNOWN)
def test_known_strings_both_directions(counts, string):
    assert rle.to_string(counts) == string
    got = rle.from_string(string)
    assert got.dtype == np.int64 and got.tolist() == counts
    assert rle.from_string(string.encode("ascii")).tolist() == counts


def test_known_counts():
    assert rle.encode(_mask_4x3())["counts"].tolist() == [1, 2, 1, 1, 6, 1]
    assert rle.encode(np.ones((2, 2)))["counts"].tolist() == [0, 4]
    assert rle.encode(np.zeros((2, 2)))["counts"].tolist() == [4]
    r = rle.encode(_mask_4x3())
    assert r["size"] == [4, 3] and r["counts"].dtype == np.int64 and r["counts"].ndim == 1


def test_column_major_order_is_used():
    m = _mask_4x3()
    a, b = rle.encode(m), rle.encode(np.ascontiguousarray(m.T))
    assert b["size"] == [3, 4]
    assert a["counts"].tolist() != b["counts"].tolist()
    assert b["counts"].tolist() == [1, 1, 1, 1, 2, 1, 4, 1]       # m.T column by column = m row by row: 010 100 100 001
    # a row-major reading of m would give exactly the transposed mask's counts
    v = m.reshape(-1)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], v)))).tolist()
    assert np.diff([0] + edges + [v.size]).tolist() == b["counts"].tolist()


def _canonical(r, m):
    c = r["counts"]
    h, w = m.shape
    assert r["size"] == [h, w] and int(c.sum()) == h * w
    assert (c[1:] > 0).all() and c[0] >= 0
    assert (c[0] == 0) == bool(m[0, 0])
    assert rle.area(r) == int(c[1::2].sum()) == int(np.count_nonzero(m))


def _cases():
    rng = np.random.default_rng(5)
    out = []
    for h, w in ((1, 1), (1, 7), (7, 1), (5, 9)):
        for p in (0.2, 0.5, 0.8):
            out.append(rng.random((h, w)) < p)
        out.append(np.ones((h, w), bool))
        out.append(np.zeros((h, w), bool))
        first = np.zeros((h, w), bool)
        first[0, 0] = True
        last = np.zeros((h, w), bool)
        last[-1, -1] = True
        out += [first, last]
    return out


def test_round_trip_and_canonical_form():
    for m in _cases():
        r = rle.encode(m)
        _canonical(r, m)
        d = rle.decode(r)
        assert d.dtype == bool and d.shape == m.shape and np.array_equal(d, m)
        # through the compressed string as well
        assert np.array_equal(rle.decode({"size": r["size"], "counts": rle.to_string(r["counts"])}), m)
    assert rle.encode(np.zeros((5, 9)))["counts"].tolist() == [45] and rle.encode(np.ones((5, 9)))["counts"].tolist() == [0, 45]


def test_encode_takes_any_dtype_and_refuses_other_ranks():
    m = _mask_4x3()
    for t in (bool, np.uint8, np.int32, np.float32):
        assert rle.encode(m.astype(t))["counts"].tolist() == [1, 2, 1, 1, 6, 1]
    with pytest.raises(ValueError):
        rle.encode(np.zeros((2, 2, 2)))
    with pytest.raises(ValueError):
        rle.decode({"size": [2, 2], "counts": np.array([3])})


def test_string_round_trip_random_counts_and_negative_deltas():
    rng = np.random.default_rng(6)
    for first in (0, 1):
        for n in (1, 2, 3, 4, 9, 40):
            c = rng.integers(1, 1 << 20, n)
            c[0] = first
            assert rle.from_string(rle.to_string(c)).tolist() == c.tolist()
    # deltas against counts[i-2] that are negative, -1, -16, -17 (the sign bit of a five-bit group) and large
    c = [5, 1 << 19, 900000, 3, 899999, 2, 899983, 1, 899966, 1 << 20, 1, 1, 33, 17, 1, 1]
    s = rle.to_string(c)
    assert rle.from_string(s).tolist() == c
    assert all(48 <= ord(ch) < 48 + 64 for ch in s)
    with pytest.raises(ValueError):
        rle.from_string("P")                                      # ends inside a count
    with pytest.raises(ValueError):
        rle.from_string("0 1")


def test_area_and_bbox_against_numpy():
    rng = np.random.default_rng(7)
    masks = _cases()
    for _ in range(100):
        h, w = rng.integers(1, 12, 2)
        masks.append(rng.random((h, w)) < rng.random() * 0.6)
    col = np.zeros((6, 5), bool)
    col[:, 1:3] = True                                             # one run over a column joint
    masks.append(col)
    for m in masks:
        r = rle.encode(m)
        assert rle.area(r) == int(m.sum())
        ys, xs = np.nonzero(m)
        want = [0, 0, 0, 0] if not len(ys) else [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]
        assert rle.bbox(r) == want, (m.astype(int), rle.bbox(r), want)
        assert rle.bbox({"size": r["size"], "counts": rle.to_string(r["counts"])}) == want


def test_counts_from_boundaries():
    assert rle.counts_from_boundaries([], 12).tolist() == [12]
    assert rle.counts_from_boundaries(np.array([0], np.uint32), 4).tolist() == [0, 4]
    assert rle.counts_from_boundaries(np.array([1, 3, 4, 5, 11], np.uint32), 12).tolist() == [1, 2, 1, 1, 6, 1]


def test_coco_results_round_trip_through_json():
    rng = np.random.default_rng(8)
    h, w = 9, 13
    full = rng.random((h, w, 3)) < 0.4
    dense = {"bboxes": np.array([[1.5, 2.0, 7.0, 8.5], [0.0, 0.0, 13.0, 9.0], [3.0, 1.0, 4.0, 2.0]], np.float32),
             "class_ids": np.array([2, 1, 3], np.int32), "confidence_scores": np.array([0.9, 0.5, 0.25], np.float32), "full_masks": full}
    as_rle = {k: v for k, v in dense.items() if k != "full_masks"}
    as_rle["rle_masks"] = [rle.encode(full[:, :, i]) for i in range(3)]
    empty = {"bboxes": np.zeros((0, 4), np.float32), "class_ids": np.zeros(0, np.int32), "confidence_scores": np.zeros(0, np.float32),
             "rle_masks": []}
    a = rle.coco_results([dense, empty], [np.int64(17), 18])
    b = rle.coco_results([as_rle, empty], [17, 18])
    assert a == b and len(a) == 3
    back = json.loads(json.dumps(a))
    assert back == a
    for i, d in enumerate(back):
        assert set(d) == {"image_id", "category_id", "segmentation", "bbox", "score"}
        assert d["image_id"] == 17 and d["category_id"] == int(dense["class_ids"][i])
        assert isinstance(d["segmentation"]["counts"], str) and d["segmentation"]["size"] == [h, w]
        assert np.array_equal(rle.decode(d["segmentation"]), full[:, :, i])
        x1, y1, x2, y2 = dense["bboxes"][i].tolist()
        assert d["bbox"] == [x1, y1, x2 - x1, y2 - y1]
        assert abs(d["score"] - float(dense["confidence_scores"][i])) == 0
    mapped = rle.coco_results([as_rle], ["img"], category_ids={1: 11, 2: 22, 3: 33})
    assert [d["category_id"] for d in mapped] == [22, 11, 33] and mapped[0]["image_id"] == "img"
    with pytest.raises(ValueError):
        rle.coco_results([dense], [1, 2])


def test_against_pycocotools():
    mask_util = pytest.importorskip("pycocotools.mask")
    rng = np.random.default_rng(9)
    for h, w in ((1, 1), (5, 9), (37, 91), (416, 416)):
        m = rng.random((h, w)) < 0.3
        if h > 30:
            m = np.kron(m[:h // 8 + 1, :w // 8 + 1], np.ones((8, 8), bool))[:h, :w]           # longer runs
        theirs = mask_util.encode(np.asfortranarray(m.astype(np.uint8)))
        ours = rle.encode(m)
        assert list(theirs["size"]) == ours["size"]
        assert theirs["counts"].decode("ascii") == rle.to_string(ours["counts"])
        assert np.array_equal(mask_util.decode(theirs).astype(bool), rle.decode(ours))
        assert int(mask_util.area(theirs)) == rle.area(ours)
        assert [int(t) for t in mask_util.toBbox(theirs)] == rle.bbox(ours)

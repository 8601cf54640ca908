"""The host side of max_detections: the numpy restatement of myolo_select_detections' contract (tests/select_ref.py) at
K = 10 against detect.select; the reassembly of the column blocks that Net.rle_masks / contour_masks / overlap_counts cut a sel wider than 16
into; Selection.from_device; the argument check; and the list consumers on 40 instances.

Under NumPy >= 2 detect.select compares a float32 score with the Python float threshold in float32, where select_ref (and the kernel) compare in
double: the two differ only at score == float32(cs_threshold) != cs_threshold.  The inputs here avoid that value: the thresholds 0.0 and 0.5 are
float32 numbers themselves."""
import os

import numpy as np
import pytest

from myolo import detect as D
from myolo import engine as E
from myolo import rle
from myolo.config import make_config, ShapesConfig
from select_ref import clustered_det, select_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _host_rows(det, cs_threshold, image_shape):
    keep, nmb, boxes, scores, class_ids = D.select(det, cs_threshold, image_shape)
    return keep[nmb], boxes[nmb], scores[nmb], class_ids[nmb]


@pytest.mark.parametrize("R", [1, 7, 40, 147])
@pytest.mark.parametrize("thr", [0.0, 0.5])
def test_select_ref_at_ten_equals_detect_select(R, thr):
    rng = np.random.default_rng(100 + R)
    det = clustered_det(rng, 3, R)
    for shape in ([224, 224, 3], [96, 64, 3]):
        sel, picked, count = select_ref(det, 3, 10, thr, shape)
        dropped = 0
        for b in range(3):
            rows, boxes, scores, class_ids = _host_rows(det[b], thr, shape)
            m = len(rows)
            assert count[b] == m and sel[b, :m].tolist() == rows.tolist() and (sel[b, m:] == -1).all()
            assert np.array_equal(picked[b, :m, :4], boxes) and np.array_equal(picked[b, :m, 4], scores)
            assert np.array_equal(picked[b, :m, 5].astype(np.int32), class_ids) and not picked[b, m:].any()
            live = ((det[b, :, 2] - det[b, :, 0]) * (det[b, :, 3] - det[b, :, 1]) > 0).sum()
            dropped += min(10, int(live)) - m
        if R >= 40:
            assert dropped > 0                                           # the threshold or NMB has removed something


def test_select_ref_on_the_reference_nmb_rows():
    """the boxes / classes of tests/golden/ref_host_nmb.npz (the reference's own NMB inputs and outputs) as detections in score order"""
    fx = np.load(os.path.join(GOLDEN, "ref_host_nmb.npz"))
    cases = suppressed = 0
    for k in range(int(fx["n_nmb"])):
        boxes, cls, idx, par = (fx["nmb_%02d_%s" % (k, name)] for name in ("boxes", "cls", "idx", "par"))
        n = len(boxes)
        if n == 0:
            continue
        det = np.zeros((1, n, 6), np.float32)
        det[0, :, :4], det[0, :, 4], det[0, :, 5] = boxes, 1.0 - np.arange(n) / 64.0, cls
        shape = [int(par[1]), int(par[2]), int(par[3])]
        sel, picked, count = select_ref(det, 1, 10, 0.0, shape)
        rows = _host_rows(det[0], 0.0, shape)[0]
        assert sel[0, :count[0]].tolist() == rows.tolist() and (sel[0, count[0]:] == -1).all()
        live = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) > 0
        if live.all() and n <= 10 and len(set(idx.tolist())) == n:
            # at the fixture's own threshold: what the reference's NMB kept
            sel, _, count = select_ref(det, 1, 10, 0.0, shape, nms_threshold=float(par[0]))
            assert idx[sel[0, :count[0]]].tolist() == fx["nmb_%02d_out" % k].tolist(), k
            suppressed += n - int(count[0])
            cases += 1
    assert cases >= 20 and suppressed >= 10


def test_select_ref_ties_and_more_slots_than_rows():
    det = np.zeros((1, 5, 6), np.float32)
    for r in range(5):
        det[0, r] = (0.18 * r, 0.0, 0.18 * r + 0.1, 0.1, 0.5 if r in (1, 3, 4) else 0.25 + 0.01 * r, 1)
    sel, picked, count = select_ref(det, 1, 8, 0.0, [64, 64, 3])
    assert sel[0].tolist() == [4, 3, 1, 2, 0, -1, -1, -1] and count[0] == 5              # equal scores: the higher row first
    assert np.array_equal(picked[0, :5], det[0, [4, 3, 1, 2, 0]])
    assert select_ref(det, 0, 8, 0.0, [64, 64, 3])[0].tolist() == [[-1] * 8]             # no live image


# ------------------------------------------------------------------------------------------------ the column blocks
def _rle_block(lens, rng):
    """a (run_off, bounds) pair with the given boundary counts per slot, the values random"""
    off = np.zeros(len(lens) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    return off, rng.integers(0, 1 << 31, int(off[-1])).astype(np.uint32)


def test_sel_column_blocks_cut_40_into_16_16_8():
    sel = np.arange(80, dtype=np.int32).reshape(2, 40)
    blocks = E.sel_column_blocks(sel)
    assert [b.shape for b in blocks] == [(2, 16), (2, 16), (2, 8)] and all(b.flags["C_CONTIGUOUS"] and b.dtype == np.int32 for b in blocks)
    assert np.array_equal(np.concatenate(blocks, axis=1), sel)
    assert [b.shape for b in E.sel_column_blocks(sel[:, :17])] == [(2, 16), (2, 1)]
    assert E.SEL_BLOCK == 16 and E.SEL_MAX == 128 and E.sel_width(sel) == 40 and E.sel_width(sel[0]) == 0


def test_join_rle_blocks_by_hand():
    """B = 2, K = 40 as 16 + 16 + 8, the middle block all empty: slot s = b * 40 + k holds block j's slot b * k_j + (k - 16 j)"""
    rng = np.random.default_rng(5)
    B, widths = 2, (16, 16, 8)
    lens = [rng.integers(0, 7, B * w) for w in widths]
    lens[1][:] = 0
    lens[0][3] = lens[2][9] = 0                                           # empty slots between live ones
    blocks = [_rle_block(l, rng) for l in lens]
    run_off, bounds = E.join_rle_blocks(blocks, B)
    assert run_off.dtype == np.int32 and run_off.shape == (81,) and bounds.dtype == np.uint32 and bounds.size == run_off[-1] == sum(l.sum() for l in lens)
    for b in range(B):
        for k in range(40):
            j, kk = (0, k) if k < 16 else ((1, k - 16) if k < 32 else (2, k - 32))
            off, bd = blocks[j]
            s_in, s = b * widths[j] + kk, b * 40 + k
            assert bounds[run_off[s]:run_off[s + 1]].tolist() == bd[off[s_in]:off[s_in + 1]].tolist(), (b, k)
    # a single block comes back as it is
    one_off, one_bd = E.join_rle_blocks(blocks[:1], B)
    assert np.array_equal(one_off, blocks[0][0]) and np.array_equal(one_bd, blocks[0][1])
    # every block empty
    off, bd = E.join_rle_blocks([_rle_block(np.zeros(B * w, np.int64), rng) for w in widths], B)
    assert not off.any() and bd.size == 0 and bd.dtype == np.uint32


def test_join_loop_blocks_by_hand():
    B, widths = 2, (16, 16, 8)
    blocks = [[[np.full((3, 2), 1000 * j + s, np.int32)] if (j != 1 and s % 5) else [] for s in range(B * w)] for j, w in enumerate(widths)]
    out = E.join_loop_blocks(blocks, B)
    assert len(out) == 80
    for b in range(B):
        for k in range(40):
            j, kk = (0, k) if k < 16 else ((1, k - 16) if k < 32 else (2, k - 32))
            assert out[b * 40 + k] is blocks[j][b * widths[j] + kk], (b, k)


def test_join_overlap_blocks_by_hand():
    rng = np.random.default_rng(7)
    B, T, widths = 2, 3, (16, 16, 8)
    area_gt = rng.integers(0, 99, (B, T)).astype(np.int32)
    blocks = [(rng.integers(0, 99, (B, w, T)).astype(np.int32), rng.integers(0, 99, (B, w)).astype(np.int32), area_gt.copy(),
               rng.integers(0, 99, (B, w, 4)).astype(np.int32)) for w in widths]
    blocks[1] = tuple(np.zeros_like(a) if i != 2 else a for i, a in enumerate(blocks[1]))
    inter, area_pred, ag, win = E.join_overlap_blocks(blocks)
    assert inter.shape == (B, 40, T) and area_pred.shape == (B, 40) and win.shape == (B, 40, 4) and np.array_equal(ag, area_gt)
    for j, c in enumerate((0, 16, 32)):
        w = widths[j]
        assert np.array_equal(inter[:, c:c + w], blocks[j][0]) and np.array_equal(area_pred[:, c:c + w], blocks[j][1])
        assert np.array_equal(win[:, c:c + w], blocks[j][3])
    import torch
    got = E.join_overlap_blocks([tuple(torch.from_numpy(a) for a in blk) for blk in blocks])
    assert all(torch.is_tensor(g) and np.array_equal(g.numpy(), w) for g, w in zip(got, (inter, area_pred, ag, win)))


# ------------------------------------------------------------------------------------------------ the record and the argument
def test_selection_from_device_fills_the_host_record():
    """from the reference selection at K = 10 the record equals the host constructor's, field for field; at K = 40 it holds more rows"""
    rng = np.random.default_rng(3)
    det = clustered_det(rng, 3, 147)
    shape = [224, 224, 3]
    host = D.Selection(det, 2, 0.0, shape)
    sel, picked, _ = select_ref(det, 2, 10, 0.0, shape)
    dev = D.Selection.from_device(sel, picked, 2)
    assert dev.n == host.n == 2 and np.array_equal(dev.sel, host.sel) and dev.sel.dtype == host.sel.dtype and len(dev.picked) == 2
    for k in range(2):
        for a, b in zip(dev.picked[k], host.picked[k]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
        assert np.array_equal(dev.rows(k), host.rows(k))
        ra, rb = dev.result(k, (100, 60, 3)), host.result(k, (100, 60, 3))
        assert set(ra) == set(rb) and all(ra[key].dtype == rb[key].dtype and np.array_equal(ra[key], rb[key]) for key in ra)
    sel, picked, count = select_ref(det, 3, 40, 0.0, shape)
    wide = D.Selection.from_device(sel, picked, 3)
    assert wide.sel.shape == (3, 40) and [len(wide.rows(k)) for k in range(3)] == count.tolist() and count.max() > 16
    assert (np.diff(wide.result(0, shape)["confidence_scores"]) <= 0).all()


def test_max_detections_argument():
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4)
    for ok in (None, 1, 10, 16, 17, 128, np.int64(40)):
        D.check_max_detections(cfg, ok)
    for bad in (0, 129, -1, True, False, 2.5, 10.0, "10", np.bool_(True)):
        with pytest.raises(ValueError, match="max_detections"):
            D.check_max_detections(cfg, bad)
    D.check_max_detections(cfg, 16, render=True)
    with pytest.raises(ValueError, match="one pass"):
        D.check_max_detections(cfg, 17, render=True)
    only = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    D.check_max_detections(only, None)
    with pytest.raises(ValueError, match="DETECT_MASKS_FOR_SELECTED_ONLY"):
        D.check_max_detections(only, 10)
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="max_detections"):
        D.check_args(cfg, [img], "image", "dense", False, 0)
    D.check_args(cfg, [img], "image", "rle", False, 40)


# ------------------------------------------------------------------------------------------------ the consumers that loop over lists
def test_list_consumers_take_forty_instances():
    from myolo import contour, via
    from myolo.render import instance_colors
    n, h, w = 40, 48, 64
    full = np.zeros((h, w, n), bool)
    for i in range(n):
        y, x = 4 * (i // 8) + 2, 7 * (i % 8) + 2
        full[y:y + 3 + i % 3, x:x + 4, i] = True
    base = {"bboxes": np.array([[7 * (i % 8) + 2, 4 * (i // 8) + 2, 7 * (i % 8) + 6, 4 * (i // 8) + 5 + i % 3] for i in range(n)], np.float32),
            "class_ids": (np.arange(n) % 3 + 1).astype(np.int32), "confidence_scores": np.linspace(0.9, 0.1, n).astype(np.float32)}
    dense = dict(base, full_masks=full)
    coded = dict(base, rle_masks=[rle.encode(full[:, :, i]) for i in range(n)])
    poly = dict(base, polygons=[contour.trace(full[:, :, i]) for i in range(n)])
    a, b, c = rle.coco_results([dense], [7]), rle.coco_results([coded], [7]), rle.coco_results([poly], [7])
    assert len(a) == len(b) == len(c) == n and a == b
    assert [r["score"] for r in a] == [float(s) for s in base["confidence_scores"]] and [r["category_id"] for r in c] == base["class_ids"].tolist()
    assert [r["area"] for r in c] == [float(full[:, :, i].sum()) for i in range(n)]
    ann = via.via_annotations([poly], ["forty.png"])
    regions = ann["forty.png-1"]["regions"]
    assert len(regions) == n and [r["region_attributes"]["instance"] for r in regions] == list(range(n))
    colors = instance_colors(n)
    assert len(colors) == n and len(set(colors)) == n and all(0.0 <= v <= 1.0 for col in colors for v in col)


# ------------------------------------------------------------------------------------------------ the build and the binding
def test_select_kernels_are_built_without_contraction_and_bound():
    import re
    import __graft_entry__ as G
    from myolo import _ext as X
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert ("select_kernels.hip", ["-ffp-contract=off"]) in G.UNITS
    src = open(os.path.join(root, "mask-yolo_amd", "csrc", "select_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.lower()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "myolo_hip_internal.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+myolo_select_detections\s*\(", txt)
    assert "myolo_select_detections" in X.exported_symbols() and len(X.SIGS["myolo_select_detections"]) == 13
    lib = X.load()
    # the argument check comes before any launch: no device is needed to be refused
    assert lib.myolo_select_detections(None, 1, 1, 1, 1, 0.0, 0.7, 224, 224, None, None, None, None) == -1
    assert lib.myolo_last_error_string().startswith(b"select_detections: null pointer")

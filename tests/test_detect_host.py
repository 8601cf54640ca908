"""The batch selection record of the detection pipeline (myolo/detect.py) on the host: no Net, no GPU.  Crafted [B,R,6]
detections on the 128 x 128 Shapes config, one image per case the per-image rule (detect.select) branches on, and a padding image."""
import numpy as np

from myolo import detect as D
from myolo.config import make_config, ShapesConfig

CFG = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=6)
R, CS = 24, 0.35
NO_AREA, CROWD, ALL_LOW, TWINS, PLAIN, PADDING = range(6)


def _batch():
    """[6,R,6] float32 rows (x1, y1, x2, y2, score, class): what each image holds is named by its index above"""
    rng = np.random.default_rng(31)
    det = np.zeros((6, R, 6), np.float32)                                  # (rows left at zero are boxes without area)
    det[NO_AREA, :5] = [(0.2, 0.3, 0.2, 0.9, 0.9, 1), (0.1, 0.5, 0.6, 0.5, 0.8, 2), (0.4, 0.4, 0.5, 0.3, 0.7, 1),     # zero width, zero height,
                        (0.5, 0.2, 0.4, 0.6, 0.95, 3), (0.0, 0.0, 0.0, 0.0, 0.99, 1)]                                 # negative height, negative width, a point
    for r in range(0, R, 2):                                               # 12 boxes with area above the threshold between rows without area: disjoint
        x, y = (r // 2) % 4 * 0.25, (r // 2) // 4 * 0.25                   # cells of a 4 x 3 grid, so NMB removes none and the top ten decide
        det[CROWD, r] = (x + 0.01, y + 0.01, x + 0.2, y + 0.2, 0.4 + 0.02 * rng.permutation(12)[r // 2] + 0.001 * r, 1 + r % 3)
    det[ALL_LOW, :6, :2] = rng.random((6, 2)) * 0.5
    det[ALL_LOW, :6, 2:4] = det[ALL_LOW, :6, :2] + 0.3
    det[ALL_LOW, :6, 4], det[ALL_LOW, :6, 5] = rng.random(6) * 0.3, 2      # every score under cs_threshold
    det[TWINS, :4] = [(0.10, 0.10, 0.50, 0.50, 0.60, 2), (0.11, 0.10, 0.51, 0.50, 0.90, 2),     # same class, IoU ~0.95: the weaker one goes
                      (0.10, 0.11, 0.50, 0.51, 0.80, 3), (0.60, 0.60, 0.90, 0.95, 0.50, 2)]     # the same place in another class stays
    det[PLAIN, 3], det[PLAIN, 7] = (0.2, 0.2, 0.7, 0.6, 0.5, 1), (0.1, 0.6, 0.4, 0.9, 0.7, 3)
    det[PADDING] = det[CROWD]                                              # a padding image repeats a live one: nothing of it may be reported
    return det


DET = _batch()
N_LIVE = 5
SELECTION = D.Selection(DET, N_LIVE, CS, CFG.IMAGE_SHAPE)


def test_sel_is_the_per_image_rule_then_minus_one():
    s = SELECTION
    assert s.sel.dtype == np.int32 and s.sel.shape == (6, D.SLOTS) and s.n == N_LIVE and len(s.picked) == N_LIVE
    for k in range(N_LIVE):
        keep, nmb, boxes, scores, class_ids = D.select(DET[k], CS, CFG.IMAGE_SHAPE)
        m = len(nmb)
        assert np.array_equal(s.sel[k, :m], keep[nmb]) and (s.sel[k, m:] == -1).all(), k
        assert np.array_equal(s.rows(k), keep[nmb]) and s.rows(k).dtype == np.int32
        got_boxes, got_ids, got_scores = s.picked[k]
        assert np.array_equal(got_boxes, boxes[nmb]) and np.array_equal(got_ids, class_ids[nmb]) and np.array_equal(got_scores, scores[nmb])
        assert np.array_equal(DET[k][s.rows(k), 4], got_scores)            # sel names rows of the image's own detections, in reporting order
    assert (s.sel[PADDING] == -1).all()


def test_each_case_selects_what_the_rule_says():
    s = SELECTION
    assert len(s.rows(NO_AREA)) == 0 and len(s.rows(ALL_LOW)) == 0
    crowd = s.rows(CROWD)
    by_score = [r for r in np.argsort(DET[CROWD, :, 4])[::-1] if DET[CROWD, r, 4] > 0]
    assert len(by_score) == 12 and crowd.tolist() == by_score[:D.SLOTS]     # more than ten above the threshold: the ten best, best first
    assert s.rows(TWINS).tolist() == [1, 2, 3]                             # row 0 overlaps row 1 above 0.7 in the same class
    assert s.rows(PLAIN).tolist() == [7, 3]


def test_result_scales_the_boxes_to_the_frame_in_their_dtype():
    s = SELECTION
    for k in range(N_LIVE):
        boxes, class_ids, scores = s.picked[k]
        for h, w in ((128, 128), (200, 150), (1, 1)):
            r = s.result(k, (h, w, 3))
            assert list(r) == ["bboxes", "class_ids", "confidence_scores"]
            want = boxes * np.array([w, h, w, h], dtype=boxes.dtype)
            assert r["bboxes"].dtype == boxes.dtype == np.float32 and r["bboxes"].tobytes() == want.tobytes(), (k, h, w)
            assert r["class_ids"] is class_ids and r["confidence_scores"] is scores
    assert np.array_equal(s.result(PLAIN, (200, 150))["bboxes"][0], np.float32([0.1, 0.6, 0.4, 0.9]) * np.float32([150, 200, 150, 200]))


def test_an_empty_image_gives_empty_arrays_of_the_right_dtypes():
    for k in (NO_AREA, ALL_LOW):
        r = SELECTION.result(k, (61, 97))
        assert r["bboxes"].shape == (0, 4) and r["bboxes"].dtype == np.float32
        assert r["class_ids"].shape == (0,) and r["class_ids"].dtype == np.int32
        assert r["confidence_scores"].shape == (0,) and r["confidence_scores"].dtype == np.float32


def test_a_batch_of_nothing_but_padding():
    s = D.Selection(DET, 0, CS, CFG.IMAGE_SHAPE)
    assert s.n == 0 and s.picked == [] and (s.sel == -1).all()

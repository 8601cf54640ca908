"""myolo/evaluate.py: the metric definitions on hand-worked cases and against a brute-force restatement in exact
rationals.  No GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

from myolo.evaluate import Evaluator, T20_THRESHOLDS, average_precision, box_counts, iou_meets, match_image


# ---------------------------------------------------------------------------------------------------- helpers to state cases in boxes only
def _img(dets, gts, size=40):
    """dets: [(score, class, [x1,y1,x2,y2])], gts: [(class, [x1,y1,x2,y2])] (class 0 = padding) -> the arguments of Evaluator.add_image with
    rectangular masks (mask == box, so the mask and box metrics agree)."""
    K, T = len(dets), len(gts)
    pm = np.zeros((K, size, size), bool)
    gm = np.zeros((T, size, size), bool)
    for k, (_, _, (x1, y1, x2, y2)) in enumerate(dets):
        pm[k, y1:y2, x1:x2] = True
    for t, (_, (x1, y1, x2, y2)) in enumerate(gts):
        gm[t, y1:y2, x1:x2] = True
    inter = np.array([[int((pm[k] & gm[t]).sum()) for t in range(T)] for k in range(K)], np.int64).reshape(K, T)
    return dict(scores=np.array([d[0] for d in dets], np.float64), class_ids=np.array([d[1] for d in dets], np.int64),
                gt_class_ids=np.array([g[0] for g in gts], np.int64), mask_inter=inter,
                area_pred=pm.sum(axis=(1, 2)).astype(np.int64), area_gt=gm.sum(axis=(1, 2)).astype(np.int64),
                win=np.array([d[2] for d in dets], np.int64).reshape(K, 4), gt_boxes=np.array([g[1] for g in gts], np.int64).reshape(T, 4))


def _run(images):
    ev = Evaluator()
    for im in images:
        ev.add_image(**im)
    return ev.result()


A, B_, C_ = [0, 0, 10, 10], [20, 0, 30, 10], [0, 20, 10, 30]      # three disjoint 10 x 10 boxes
FAR = [30, 30, 40, 40]


# ---------------------------------------------------------------------------------------------------- the threshold rule
def test_threshold_rule_at_exact_equality():
    assert iou_meets(1, 2, 10) and not iou_meets(1, 2, 11)
    assert iou_meets(19, 20, 19)
    assert not iou_meets(0, 0, 10)                                  # a union of 0 is IoU 0
    assert T20_THRESHOLDS == tuple(range(10, 20))
    # the same through match_image: inter 1 / union 2 is a true positive at 0.50 and a false positive at 0.55
    for t20, want in ((10, True), (11, False)):
        tp, match = match_image([0.9], [1], [1], [[1]], [[2]], t20)
        assert bool(tp[0]) is want and match[0] == (0 if want else -1)
    assert match_image([0.9], [1], [1], [[19]], [[20]], 19)[0][0]


def test_box_counts_end_exclusive():
    inter, union = box_counts([[0, 0, 10, 10], [5, 5, 15, 15], [0, 0, 0, 0]], [[0, 0, 10, 10], [10, 10, 20, 20]])
    assert inter.tolist() == [[100, 0], [25, 25], [0, 0]]
    assert union.tolist() == [[100, 200], [175, 175], [100, 100]]


# ---------------------------------------------------------------------------------------------------- hand-worked cases
def test_three_detections_one_class_ap():
    """two instances; by score: a hit (P 1, R 1/2), a miss (P 1/2, R 1/2), a hit (P 2/3, R 1) -> AP = 1/2 * 1 + 1/2 * 2/3"""
    r = _run([_img([(0.9, 1, A), (0.8, 1, FAR), (0.7, 1, B_)], [(1, A), (1, B_)])])
    want = 0.5 * 1 + 0.5 * (2.0 / 3.0)
    for k in ("mask_ap50", "mask_ap", "box_ap50", "box_ap"):
        assert abs(r[k] - want) < 1e-15, (k, r[k])
    assert r["n_images"] == 1 and r["n_gt"] == 2 and r["n_det"] == 3
    assert r["mean_matched_mask_iou"] == 1.0
    pc = r["per_class"]
    assert list(pc) == [1] and pc[1]["n_gt"] == 2 and pc[1]["n_det"] == 3
    assert abs(pc[1]["mask_ap50"] - want) < 1e-15 and abs(pc[1]["box_ap50"] - want) < 1e-15
    assert abs(average_precision([True, False, True], 2) - want) < 1e-15


def test_duplicate_detection_is_a_false_positive():
    im = _img([(0.9, 1, A), (0.8, 1, A)], [(1, A)])
    tp, match = match_image(im["scores"], im["class_ids"], im["gt_class_ids"], im["mask_inter"], np.full((2, 1), 100), 10)
    assert tp.tolist() == [True, False] and match.tolist() == [0, -1]
    r = _run([im])
    assert r["mask_ap50"] == 1.0 and r["box_ap50"] == 1.0           # recall 1 is reached at precision 1; the duplicate comes after
    # a duplicate ranked in front of a second instance's hit costs precision there: P = 1, 1/2, 2/3 at R = 1/2, 1/2, 1
    r = _run([_img([(0.9, 1, A), (0.8, 1, A), (0.7, 1, B_)], [(1, A), (1, B_)])])
    assert abs(r["mask_ap50"] - (0.5 + 0.5 * 2.0 / 3.0)) < 1e-15


def test_wrong_class_detection_with_iou_one():
    r = _run([_img([(0.9, 2, A)], [(1, A)])])
    assert r["mask_ap50"] == 0.0 and r["box_ap"] == 0.0 and r["n_det"] == 1 and r["n_gt"] == 1
    assert list(r["per_class"]) == [1]                              # class 2 has detections and no ground truth: left out of the mean


def test_classes_without_detections_or_without_ground_truth():
    # class 1: perfect; class 2: ground truth, no detections (AP 0); class 3: detections, no ground truth (not in the mean)
    r = _run([_img([(0.9, 1, A), (0.8, 3, C_)], [(1, A), (2, B_)])])
    assert r["mask_ap50"] == 0.5 and r["box_ap50"] == 0.5 and r["mask_ap"] == 0.5
    assert sorted(r["per_class"]) == [1, 2] and r["per_class"][2]["mask_ap50"] == 0.0 and r["per_class"][2]["n_det"] == 0
    assert average_precision([], 3) == 0.0


def test_image_with_neither_and_padding_slots():
    empty = _img([], [(0, [0, 0, 0, 0]), (0, [0, 0, 0, 0])])
    r = _run([empty])
    assert r == {"mask_ap50": 0.0, "mask_ap": 0.0, "box_ap50": 0.0, "box_ap": 0.0, "per_class": {}, "mean_matched_mask_iou": 0.0,
                 "n_images": 1, "n_gt": 0, "n_det": 0}
    # an empty image beside a real one changes the image count only; a padding slot (class 0) under a detection is no instance
    one = _img([(0.9, 1, A)], [(1, A), (0, A)])
    r1, r2 = _run([one]), _run([empty, one])
    assert r1["n_gt"] == 1 and r1["mask_ap"] == 1.0
    assert {k: v for k, v in r2.items() if k != "n_images"} == {k: v for k, v in r1.items() if k != "n_images"} and r2["n_images"] == 2


def test_equal_scores_go_to_the_lower_slot_then_the_earlier_image():
    # one instance, two exact detections of equal score: slot 0 takes it
    im = _img([(0.5, 1, A), (0.5, 1, A)], [(1, A)])
    tp, _ = match_image(im["scores"], im["class_ids"], im["gt_class_ids"], im["mask_inter"], np.full((2, 1), 100), 10)
    assert tp.tolist() == [True, False]
    # between images: a miss and a hit of equal score; the earlier image's detection is ranked first
    miss, hit = _img([(0.5, 1, FAR)], [(1, A)]), _img([(0.5, 1, A)], [(1, A)])
    assert abs(_run([hit, miss])["mask_ap50"] - 0.5) < 1e-15        # P, R: (1, 1/2), (1/2, 1/2)
    assert abs(_run([miss, hit])["mask_ap50"] - 0.25) < 1e-15       # P, R: (0, 0), (1/2, 1/2)


def test_equal_ious_go_to_the_lower_ground_truth_index_and_larger_iou_wins():
    # a detection midway between two instances (IoU 2/3 with each) takes index 0
    left, mid = [0, 0, 10, 10], [2, 0, 12, 10]
    im = _img([(0.9, 1, [3, 0, 13, 10])], [(1, [1, 0, 11, 10]), (1, [5, 0, 15, 10])])
    assert im["mask_inter"].tolist() == [[80, 80]]
    tp, match = match_image(im["scores"], im["class_ids"], im["gt_class_ids"], im["mask_inter"], np.full((1, 2), 120), 10)
    assert match.tolist() == [0]
    # the larger IoU wins whatever its index: 8/12 against 10/10
    im = _img([(0.9, 1, mid)], [(1, left), (1, mid)])
    union = im["area_pred"][:, None] + im["area_gt"][None, :] - im["mask_inter"]
    assert match_image(im["scores"], im["class_ids"], im["gt_class_ids"], im["mask_inter"], union, 10)[1].tolist() == [1]


# ---------------------------------------------------------------------------------------------------- brute force in exact rationals
def _brute(images):
    """The whole specification again with explicit loops and Fractions (no helper of myolo.evaluate).  images: [(dets, gts)] with
    dets = [(score, class, {gt index: (inter, union)} for masks, the same for boxes)], gts = [class].
    -> (tp flags [image][det][kind][threshold], result dict of Fractions)"""
    flags = []
    for dets, gts in images:
        f = [[[False] * 10 for _ in range(2)] for _ in dets]
        for kind in range(2):
            for ti in range(10):
                thr = Fraction(10 + ti, 20)
                order = list(range(len(dets)))
                for a in range(len(order)):                         # selection sort: score descending, then slot ascending
                    for b in range(a + 1, len(order)):
                        ia, ib = order[a], order[b]
                        if dets[ib][0] > dets[ia][0] or (dets[ib][0] == dets[ia][0] and ib < ia):
                            order[a], order[b] = ib, ia
                used = set()
                for i in order:
                    best, best_iou = None, None
                    for j in range(len(gts)):
                        if gts[j] == 0 or gts[j] != dets[i][1] or j in used:
                            continue
                        inter, union = dets[i][2 + kind][j]
                        iou = Fraction(inter, union) if union else Fraction(0)
                        if union == 0 or iou < thr:
                            continue
                        if best is None or iou > best_iou:
                            best, best_iou = j, iou
                    if best is not None:
                        used.add(best)
                        f[i][kind][ti] = True
        flags.append(f)
    classes = sorted({g for _, gts in images for g in gts if g != 0})
    out = {}
    for kind, name in ((0, "mask"), (1, "box")):
        per_thr = []
        for ti in range(10):
            aps = []
            for c in classes:
                n_gt = sum(1 for _, gts in images for g in gts if g == c)
                pool = [(dets[i][0], im, i, flags[im][i][kind][ti]) for im, (dets, _) in enumerate(images) for i in range(len(dets))
                        if dets[i][1] == c]
                pool.sort(key=lambda r: (-r[0], r[1], r[2]))
                prec, rec, tp = [], [], 0
                for n, r in enumerate(pool):
                    tp += 1 if r[3] else 0
                    prec.append(Fraction(tp, n + 1))
                    rec.append(Fraction(tp, n_gt))
                for n in range(len(prec) - 2, -1, -1):
                    prec[n] = max(prec[n], prec[n + 1])
                ap, prev = Fraction(0), Fraction(0)
                for n in range(len(prec)):
                    if rec[n] != prev:
                        ap += (rec[n] - prev) * prec[n]
                        prev = rec[n]
                aps.append(ap)
            per_thr.append(sum(aps, Fraction(0)) / len(aps) if aps else Fraction(0))
        out[name + "_ap50"] = per_thr[0]
        out[name + "_ap"] = sum(per_thr, Fraction(0)) / 10
    return flags, out


def _random_case(rng):
    """a few images of small rectangles on a coarse lattice (so that equal IoUs, equal scores and exact thresholds do happen)"""
    size, images, args = 12, [], []
    for _ in range(int(rng.integers(1, 5))):
        K, T = int(rng.integers(0, 6)), int(rng.integers(0, 5))

        def box():
            x1, y1 = int(rng.integers(0, 4)) * 2, int(rng.integers(0, 4)) * 2
            return [x1, y1, x1 + int(rng.integers(1, 4)) * 2, y1 + int(rng.integers(1, 4)) * 2]
        gts = [(int(rng.integers(0, 3)), box()) for _ in range(T)]
        dets = []
        for _k in range(K):
            bx = list(gts[int(rng.integers(0, T))][1]) if T and rng.random() < 0.6 else box()
            if rng.random() < 0.4:
                bx[2] += 2
            dets.append((float(rng.integers(1, 6)) / 8.0, int(rng.integers(1, 3)), bx))
        im = _img(dets, gts, size=size)
        # masks that are NOT the boxes: thin the pasted masks' counts so that mask and box metrics differ
        shrink = rng.integers(0, 2, size=im["mask_inter"].shape)
        im["mask_inter"] = np.maximum(im["mask_inter"] - shrink * (im["mask_inter"] // 3), 0)
        args.append(im)
        mu = im["area_pred"][:, None] + im["area_gt"][None, :] - im["mask_inter"]
        bi, bu = box_counts(im["win"], im["gt_boxes"])
        images.append(([(d[0], d[1], {j: (int(im["mask_inter"][k, j]), int(mu[k, j])) for j in range(T)},
                         {j: (int(bi[k, j]), int(bu[k, j])) for j in range(T)}) for k, d in enumerate(dets)], [g[0] for g in gts]))
    return args, images


def test_200_random_cases_against_brute_force():
    rng = np.random.default_rng(20240)
    seen_tp = seen_fp = 0
    for case in range(200):
        args, images = _random_case(rng)
        flags, want = _brute(images)
        ev = Evaluator()
        for im in args:
            ev.add_image(**im)
        got = ev.result()
        for k, v in want.items():
            assert abs(got[k] - float(v)) < 1e-12, (case, k, got[k], float(v))
        # true-positive flags, exactly, through match_image itself
        for im, (dets, gts), f in zip(args, images, flags):
            if not dets:
                continue
            mu = im["area_pred"][:, None] + im["area_gt"][None, :] - im["mask_inter"]
            bi, bu = box_counts(im["win"], im["gt_boxes"])
            for kind, (inter, union) in enumerate(((im["mask_inter"], mu), (bi, bu))):
                for ti, t20 in enumerate(T20_THRESHOLDS):
                    tp, _ = match_image(im["scores"], im["class_ids"], im["gt_class_ids"], inter, union, t20)
                    assert tp.tolist() == [f[i][kind][ti] for i in range(len(dets))], (case, kind, t20)
                    seen_tp += int(tp.sum())
                    seen_fp += int((~tp).sum())
    assert seen_tp > 500 and seen_fp > 500                          # the cases do exercise both outcomes


def test_image_order_does_not_matter_without_score_ties():
    rng = np.random.default_rng(7)
    args = []
    while len(args) < 6:
        a, _ = _random_case(rng)
        args += a
    score = 0.99
    for im in args:                                                 # distinct scores over the whole set
        for k in range(len(im["scores"])):
            im["scores"][k] = score
            score -= 0.01
    want = _run(args)
    assert want["n_det"] > 5 and want["n_gt"] > 5
    for _ in range(5):
        got = _run([args[i] for i in rng.permutation(len(args))])
        assert got == want


def test_average_precision_refuses_a_class_without_ground_truth():
    with pytest.raises(ValueError):
        average_precision([True], 0)

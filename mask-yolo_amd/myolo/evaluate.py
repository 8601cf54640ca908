"""
Task metrics: mask and box average precision of a set of detections against ground truth.

Pure numpy / Python integers, importable without a GPU.  The reference never published a metric, so the definitions here ARE the
specification:

* An IoU is a pair of integers (inter, union), union = area_a + area_b - inter; a union of 0 is IoU 0.  Thresholds are t20 / 20 for
  t20 = 10 .. 19 (0.50 .. 0.95) and "IoU >= threshold" is 20 * inter >= t20 * union in integers: no floating-point comparison decides a match.
* match_image: detections by descending score (ties: lower slot); each takes, among the ground-truth instances of its own class that are
  not taken yet and meet the threshold, the one with the largest IoU (cross-multiplied integers; ties: lower index).  It is then a true
  positive, otherwise a false positive.  Ground-truth slots with class id 0 are padding.
* average_precision: per class over the whole dataset, VOC-2010 all-point interpolation (what matterport's compute_ap does per image).
  mAP = the mean over the classes that have ground truth.

The counts come from MaskYOLO.evaluate (myolo_mask_overlap_counts: pasted mask against ground-truth plane, on the device) or from any
other source of the same integers.
"""
import math

import numpy as np

T20_THRESHOLDS = tuple(range(10, 20))          # IoU thresholds 0.50 .. 0.95 in twentieths


def iou_meets(inter, union, t20):
    """IoU = inter / union >= t20 / 20, in integers (a union of 0 is IoU 0: never)."""
    inter, union = int(inter), int(union)
    return union > 0 and 20 * inter >= int(t20) * union


def mask_unions(inter, area_pred, area_gt):
    """[K,T] unions of K pasted masks and T ground-truth planes from their pixel counts (int64)."""
    inter = np.asarray(inter, np.int64)
    return np.asarray(area_pred, np.int64)[:, None] + np.asarray(area_gt, np.int64)[None, :] - inter


def box_counts(win, gt_boxes):
    """(inter [K,T], union [K,T]) int64 pixel counts between K windows and T boxes, both [x1,y1,x2,y2] with x2 / y2 exclusive: the paste
    window myolo_mask_overlap_counts returns and the tight box extract_bboxes makes.  An empty box has area 0."""
    a = np.asarray(win, np.int64).reshape(-1, 4)
    b = np.asarray(gt_boxes, np.int64).reshape(-1, 4)
    area_a = np.maximum(a[:, 2] - a[:, 0], 0) * np.maximum(a[:, 3] - a[:, 1], 0)
    area_b = np.maximum(b[:, 2] - b[:, 0], 0) * np.maximum(b[:, 3] - b[:, 1], 0)
    iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    inter = np.maximum(iw, 0) * np.maximum(ih, 0)
    inter = np.where((area_a[:, None] > 0) & (area_b[None, :] > 0), inter, 0)
    return inter, area_a[:, None] + area_b[None, :] - inter


def match_image(scores, class_ids, gt_class_ids, inter, union, t20):
    """One image at one threshold -> (tp [N] bool, match [N] int: the ground-truth index a true positive took, -1 for a false positive).
    scores / class_ids [N] of the detections (slot order), gt_class_ids [T] (0 = padding), inter / union [N,T] integer counts."""
    n, t = len(scores), len(gt_class_ids)
    inter = np.asarray(inter, np.int64).reshape(n, t)
    union = np.asarray(union, np.int64).reshape(n, t)
    order = sorted(range(n), key=lambda i: (-float(scores[i]), i))
    taken = [False] * t
    tp = np.zeros(n, bool)
    match = np.full(n, -1, np.int64)
    for i in order:
        best, bi, bu = -1, 0, 1
        for j in range(t):
            g = int(gt_class_ids[j])
            if g == 0 or g != int(class_ids[i]) or taken[j]:
                continue
            a, u = int(inter[i, j]), int(union[i, j])
            if not iou_meets(a, u, t20):
                continue
            if best < 0 or a * bu > bi * u:             # a / u > bi / bu; equal IoUs keep the lower index
                best, bi, bu = j, a, u
        if best >= 0:
            taken[best] = True
            tp[i], match[i] = True, best
    return tp, match


def average_precision(tp_sorted, n_gt):
    """AP of one class: tp_sorted = its pooled detections' true-positive flags by descending score, n_gt = its ground-truth instances.
    Cumulative precision / recall, precision replaced by its running maximum from the right, sum of (r_i - r_{i-1}) * p_i over the
    points where recall changes.  Ground truth and no detections: 0."""
    tp = np.asarray(tp_sorted, bool)
    if n_gt <= 0:
        raise ValueError("average_precision: a class without ground truth has no AP")
    if tp.size == 0:
        return 0.0
    ctp = np.cumsum(tp).astype(np.float64)
    precision = ctp / np.arange(1, tp.size + 1, dtype=np.float64)
    recall = ctp / float(n_gt)
    precision = np.maximum.accumulate(precision[::-1])[::-1]
    prev = np.concatenate([[0.0], recall[:-1]])
    return float(np.sum((recall - prev) * precision))       # (the difference is 0 where recall does not change)


class Evaluator(object):
    """Accumulates images, then result().  One record per detection: (class, score, image id, slot, true-positive flags at the ten
    thresholds for masks and for boxes, IoU of the mask match at 0.50)."""

    def __init__(self):
        self._det = []             # (class, score, image id, slot, tp_mask [10], tp_box [10], matched mask iou at 0.50 or None)
        self._n_gt = {}            # class -> ground-truth instances
        self._n_images = 0

    def add_image(self, scores, class_ids, gt_class_ids, mask_inter, area_pred, area_gt, win, gt_boxes, image_id=None):
        """One image: scores / class_ids [N] of its selected detections in slot order, gt_class_ids [T] (0 = padding), and the counts of
        myolo_mask_overlap_counts for those N slots: mask_inter [N,T], area_pred [N], area_gt [T], win [N,4]; gt_boxes [T,4]
        ([x1,y1,x2,y2], end-exclusive).  image_id orders equal scores between images (default: the number of images added before)."""
        scores = np.asarray(scores, np.float64).reshape(-1)
        class_ids = np.asarray(class_ids, np.int64).reshape(-1)
        gt_class_ids = np.asarray(gt_class_ids, np.int64).reshape(-1)
        n, t = scores.size, gt_class_ids.size
        image_id = self._n_images if image_id is None else image_id
        self._n_images += 1
        for g in gt_class_ids:
            if g != 0:
                self._n_gt[int(g)] = self._n_gt.get(int(g), 0) + 1
        if n == 0:
            return
        m_inter = np.asarray(mask_inter, np.int64).reshape(n, t)
        m_union = mask_unions(m_inter, np.asarray(area_pred).reshape(n), np.asarray(area_gt).reshape(t))
        b_inter, b_union = box_counts(np.asarray(win).reshape(n, 4), np.asarray(gt_boxes).reshape(t, 4))
        tp_m = np.zeros((n, len(T20_THRESHOLDS)), bool)
        tp_b = np.zeros((n, len(T20_THRESHOLDS)), bool)
        iou50 = [None] * n
        for ti, t20 in enumerate(T20_THRESHOLDS):
            tp_m[:, ti], match = match_image(scores, class_ids, gt_class_ids, m_inter, m_union, t20)
            if t20 == 10:
                for i in np.nonzero(match >= 0)[0]:
                    iou50[i] = float(m_inter[i, match[i]]) / float(m_union[i, match[i]])
            tp_b[:, ti], _ = match_image(scores, class_ids, gt_class_ids, b_inter, b_union, t20)
        for i in range(n):
            self._det.append((int(class_ids[i]), float(scores[i]), image_id, i, tp_m[i], tp_b[i], iou50[i]))

    def result(self):
        classes = sorted(c for c, n in self._n_gt.items() if n > 0)
        by_class = {}
        for d in self._det:
            by_class.setdefault(d[0], []).append(d)
        nt = len(T20_THRESHOLDS)
        ap_m = np.zeros((len(classes), nt))
        ap_b = np.zeros((len(classes), nt))
        per_class = {}
        for ci, c in enumerate(classes):
            dets = sorted(by_class.get(c, []), key=lambda d: (-d[1], d[2], d[3]))
            for ti in range(nt):
                ap_m[ci, ti] = average_precision([d[4][ti] for d in dets], self._n_gt[c])
                ap_b[ci, ti] = average_precision([d[5][ti] for d in dets], self._n_gt[c])
            per_class[c] = {"mask_ap50": float(ap_m[ci, 0]), "box_ap50": float(ap_b[ci, 0]), "n_gt": self._n_gt[c], "n_det": len(dets)}

        def mean(a):
            return float(math.fsum(a.ravel()) / a.size) if a.size else 0.0
        ious = [d[6] for d in self._det if d[6] is not None]
        return {
            "mask_ap50": mean(ap_m[:, 0]), "mask_ap": mean(ap_m),
            "box_ap50": mean(ap_b[:, 0]), "box_ap": mean(ap_b),
            "per_class": per_class,
            "mean_matched_mask_iou": float(math.fsum(ious) / len(ious)) if ious else 0.0,     # (fsum: exact, so the order of add_image calls cannot show)
            "n_images": self._n_images, "n_gt": int(sum(self._n_gt.values())), "n_det": len(self._det),
        }

"""The contract of myolo_select_detections (include/myolo_hip_internal.h) restated in numpy for any K: detect.select with
its 10 replaced by K -- the rows with area, a STABLE argsort of their scores reversed (descending score, ties by the higher row first), the first
K, those with float(score) >= float(cs_threshold), myolo_utils.NMB -- over the live images of a batch."""
import numpy as np

from myolo import myolo_utils as mutils


def select_ref(det, n_live, K, cs_threshold, image_shape, nms_threshold=0.7):
    """det [B,R,6] float32 -> sel [B,K] int32 (-1 = empty), picked [B,K,6] float32 (zeros = empty), count [B] int32"""
    det = np.asarray(det)
    assert det.dtype == np.float32 and det.ndim == 3 and det.shape[2] == 6
    B = det.shape[0]
    sel = np.full((B, K), -1, np.int32)
    picked = np.zeros((B, K, 6), np.float32)
    count = np.zeros(B, np.int32)
    for b in range(n_live):
        boxes, scores, class_ids = det[b, :, :4], det[b, :, 4], det[b, :, 5].astype(np.int32)
        keep = np.where((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) > 0)[0]
        boxes, scores, class_ids = boxes[keep], scores[keep], class_ids[keep]
        top = np.argsort(scores, kind="stable")[::-1][:K]
        kept = np.array([i for i in top if float(scores[i]) >= float(cs_threshold)], dtype=np.int64)
        nmb = mutils.NMB(boxes[kept], class_ids[kept], kept, image_shape, nms_threshold=nms_threshold) if len(kept) else kept
        rows = keep[np.asarray(nmb, dtype=np.int64)]
        count[b] = len(rows)
        sel[b, :len(rows)] = rows
        picked[b, :len(rows)] = det[b, rows]
    return sel, picked, count


def clustered_det(rng, B, R, classes=(0, 1, 80), dead=0.15, negative=0.1):
    """det [B,R,6] that NMB has work on: boxes jittered around a few centres per image (pairs on both sides of IoU 0.7), class ids from `classes`,
    DISTINCT scores in (0, 1), a share `dead` of the rows without area (x2 == x1, or one extent negative) and a share `negative` with BOTH
    extents negative (their product is positive: such a row is live)"""
    det = np.zeros((B, R, 6), np.float32)
    for b in range(B):
        n_c = max(1, R // 6)
        centres = rng.random((n_c, 2)) * 0.6 + 0.2
        sizes = rng.random((n_c, 2)) * 0.25 + 0.1
        which = rng.integers(0, n_c, R)
        c = centres[which] + rng.normal(0.0, 0.012, (R, 2))
        s = sizes[which] * (1.0 + rng.normal(0.0, 0.04, (R, 2)))
        det[b, :, 0:2], det[b, :, 2:4] = c - s / 2, c + s / 2
        det[b, :, 4] = (rng.permutation(R) + 1.0) / (R + 1.0)
        det[b, :, 5] = np.asarray(classes, np.float32)[(which + rng.integers(0, 2, R) * (rng.random(R) < 0.2)) % len(classes)]
        u = rng.random(R)
        for r in np.flatnonzero(u < dead):
            if r % 2:
                det[b, r, 2] = det[b, r, 0]                                  # zero width
            else:
                det[b, r, 3] = det[b, r, 1] - np.float32(0.1)                # one negative extent: a negative product
        for r in np.flatnonzero((u >= dead) & (u < dead + negative)):
            det[b, r, :4] = det[b, r, [2, 3, 0, 1]]                          # both negative
    return det

"""numpy restatement of the copy-paste contract ("Copy-paste") -- a helper of the copy-paste tests, not a test.  Written from the
contract's text: sets and loops over slots, no bit tricks beyond reading select[b] as a 32-bit pattern.  The targets are tests/augment_ref.py's."""
import numpy as np

import augment_ref as R


def accepted(class_ids, donor, select, b, T):
    """-> (d, A, dropped): the donor image, the accepted donor slots in ascending order, the selected live slots that found no free slot"""
    B = len(class_ids)
    d = int(donor[b])
    bits = int(select[b]) & 0xffffffff
    S = [t for t in range(T) if (bits >> t) & 1 and class_ids[d][t] != 0] if 0 <= d < B else []
    free = T - sum(1 for t in range(T) if class_ids[b][t] != 0)
    A = S[:free]
    return d, A, len(S) - len(A)


def paste_image(images, masks, class_ids, donor, select, b, T):
    """One output image.  images [B,H,W,3] float32, masks [B,H,W,T], class_ids [B,T].
    -> image float32 [H,W,3], masks uint8 [H,W,T], boxes int32 [T,4], ids int32 [T], dropped int"""
    H, W = images.shape[1:3]
    d, A, dropped = accepted(class_ids, donor, select, b, T)
    U = np.zeros((H, W), bool)
    for t in A:
        U |= masks[d][:, :, t] != 0
    image = images[b].copy()
    if A:
        image[U] = images[d][U]
    cands = [(class_ids[b][t], (masks[b][:, :, t] != 0) & ~U) for t in range(T) if class_ids[b][t] != 0]
    cands += [(class_ids[d][t], masks[d][:, :, t] != 0) for t in A]
    out_masks, out_ids, out_boxes = np.zeros((H, W, T), np.uint8), np.zeros(T, np.int32), np.zeros((T, 4), np.int32)
    n = 0
    for cls, m in cands:
        if not m.any():
            continue
        cols, rws = np.where(m.any(axis=0))[0], np.where(m.any(axis=1))[0]
        out_masks[:, :, n], out_ids[n] = m, cls
        out_boxes[n] = (cols[0], rws[0], cols[-1] + 1, rws[-1] + 1)
        n += 1
    return image, out_masks, out_boxes, out_ids, dropped


def copy_paste_batch(images, masks, class_ids, donor, select, H, W, T, G, A, C, anchors):
    """The whole contract for a batch.  -> dict of augment_ref.augment_batch's six arrays and "dropped" int32 [B]."""
    B = len(images)
    images = np.asarray(images, np.float32)
    out = dict(images=np.zeros((B, H, W, 3), np.float32), gt_masks=np.zeros((B, H, W, T), np.uint8),
               gt_boxes=np.zeros((B, T, 4), np.int32), gt_ids=np.zeros((B, T), np.int32),
               y_true=np.zeros((B, G, G, A, 5 + C), np.float32), true_boxes=np.zeros((B, T, 4), np.float32), dropped=np.zeros(B, np.int32))
    for b in range(B):
        img, m, boxes, ids, dropped = paste_image(images, masks, class_ids, donor, select, b, T)
        n = int((ids != 0).sum())
        yt, tb = R.encode_targets_raw(boxes[:n], ids[:n], H, W, G, A, C, T, anchors)
        out["images"][b], out["gt_masks"][b], out["gt_boxes"][b], out["gt_ids"][b], out["dropped"][b] = img, m, boxes, ids, dropped
        out["y_true"][b], out["true_boxes"][b] = yt.astype(np.float32), tb.astype(np.float32)
    return out

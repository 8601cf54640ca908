"""numpy restatement of the mosaic contract ("Mosaic") -- a helper of the mosaic tests, not a test.  Written from the contract's text on
top of tests/augment_ref.py: the source position, the nearest mask tap and the bilinear image tap are that contract's, read per tile from the
tile's image through the tile's row; the instances are the 4T candidates (q, t) in q-major order."""
import numpy as np

import augment_ref as R


def compose(tiles, src, rows):
    """Mosaic.compose, entry by entry in the order its docstring states; an identity tile copies the row."""
    B = len(src)
    out = np.zeros((B, 4, 8), np.float64)
    for b in range(B):
        for q in range(4):
            r, a = np.asarray(rows[src[b][q]], np.float64), np.asarray(tiles[b][q], np.float64)
            if a.tolist() == [1., 0., 0., 0., 1., 0.]:
                out[b, q] = r
                continue
            out[b, q] = [r[0] * a[0] + r[1] * a[3], r[0] * a[1] + r[1] * a[4], (r[0] * a[2] + r[1] * a[5]) + r[2],
                         r[3] * a[0] + r[4] * a[3], r[3] * a[1] + r[4] * a[4], (r[3] * a[2] + r[4] * a[5]) + r[5], r[6], r[7]]
    return out


def warped_masks(masks, p):
    """the nearest tap of every output pixel: masks [H,W,T] 0/1, p float64[8] -> bool [H,W,T]"""
    H, W = masks.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    x, y = xx.astype(np.float64), yy.astype(np.float64)
    sx = (p[0] * x + p[1] * y) + p[2]
    sy = (p[3] * x + p[4] * y) + p[5]
    fx, fy = np.floor(sx + 0.5), np.floor(sy + 0.5)
    inside = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    ix = np.where(inside, fx, 0).astype(np.int64)
    iy = np.where(inside, fy, 0).astype(np.int64)
    return (np.asarray(masks)[iy, ix, :] != 0) & inside[:, :, None]


def mosaic_image(images, masks, class_ids, src, rows, centre, cval, T):
    """One output image.  images [B,H,W,3] uint8, masks [B,H,W,T], class_ids [B,T]; src int[4], rows float64 [4,8], centre (cx, cy).
    -> image float32 [H,W,3], masks uint8 [H,W,T], boxes int32 [T,4], ids int32 [T], dropped int"""
    H, W = images.shape[1:3]
    yy, xx = np.mgrid[0:H, 0:W]
    tile = (xx >= centre[0]).astype(np.int64) + 2 * (yy >= centre[1])
    image = np.zeros((H, W, 3), np.float32)
    out_masks, out_ids, out_boxes = np.zeros((H, W, T), np.uint8), np.zeros(T, np.int32), np.zeros((T, 4), np.int32)
    n = dropped = 0
    for q in range(4):
        s, p = int(src[q]), np.asarray(rows[q], np.float64)
        here = tile == q
        image[here] = R.augment_image(images[s], masks[s], class_ids[s], p, cval, T)[0][here]
        warped = warped_masks(masks[s], p) & here[:, :, None]
        for t in range(T):
            m = warped[:, :, t]
            if class_ids[s][t] == 0 or not m.any():
                continue
            if n == T:
                dropped += 1
                continue
            cols, rws = np.where(m.any(axis=0))[0], np.where(m.any(axis=1))[0]
            out_masks[:, :, n], out_ids[n] = m, class_ids[s][t]
            out_boxes[n] = (cols[0], rws[0], cols[-1] + 1, rws[-1] + 1)
            n += 1
    return image, out_masks, out_boxes, out_ids, dropped


def mosaic_batch(images, masks, class_ids, quad_src, quad_rows, centre, cval, H, W, T, G, A, C, anchors):
    """The whole contract for a batch.  -> dict of augment_ref.augment_batch's six arrays and "dropped" int32 [B]."""
    B = len(images)
    out = dict(images=np.zeros((B, H, W, 3), np.float32), gt_masks=np.zeros((B, H, W, T), np.uint8),
               gt_boxes=np.zeros((B, T, 4), np.int32), gt_ids=np.zeros((B, T), np.int32),
               y_true=np.zeros((B, G, G, A, 5 + C), np.float32), true_boxes=np.zeros((B, T, 4), np.float32), dropped=np.zeros(B, np.int32))
    for b in range(B):
        img, m, boxes, ids, dropped = mosaic_image(images, masks, class_ids, quad_src[b], quad_rows[b], centre[b], cval, T)
        n = int((ids != 0).sum())
        yt, tb = R.encode_targets_raw(boxes[:n], ids[:n], H, W, G, A, C, T, anchors)
        out["images"][b], out["gt_masks"][b], out["gt_boxes"][b], out["gt_ids"][b], out["dropped"][b] = img, m, boxes, ids, dropped
        out["y_true"][b], out["true_boxes"][b] = yt.astype(np.float32), tb.astype(np.float32)
    return out

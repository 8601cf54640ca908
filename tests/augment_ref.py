"""numpy restatement of the on-device augmentation contract ("On-device augmentation") -- a helper of the augmentation tests, not
a test.  Written from the contract's text, one IEEE binary64 operation per step in the order stated (numpy never fuses a multiply-add), so the
kernels must reproduce every bit of it."""
import numpy as np


def encode_targets(boxes, class_ids, cfg):
    """BatchGenerator._encode's target arithmetic for ONE image on boxes [n,(x1,y1,x2,y2)]: -> y_true [G,G,A,5+C], true_boxes [T,4] (float64)."""
    G, A, C, T = cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES, cfg.TRUE_BOX_BUFFER
    H, W = cfg.IMAGE_SHAPE[0], cfg.IMAGE_SHAPE[1]
    return encode_targets_raw(boxes, class_ids, H, W, G, A, C, T, np.asarray(cfg.ANCHORS, np.float64))


def encode_targets_raw(boxes, class_ids, H, W, G, A, C, T, anchors):
    anc = np.asarray(anchors, np.float64).reshape(-1, 2)
    aw, ah = anc[:, 0], anc[:, 1]
    y_true = np.zeros((G, G, A, 5 + C))
    true_boxes = np.zeros((T, 4))
    cell_w, cell_h = float(W) / G, float(H) / G
    tbi = 0
    for i in range(len(boxes)):
        x1, y1, x2, y2 = [int(v) for v in boxes[i]]
        cx = .5 * (x1 + x2) / cell_w
        cy = .5 * (y1 + y2) / cell_h
        gx, gy = int(np.floor(cx)), int(np.floor(cy))
        if gx < G and gy < G:
            bw = (x2 - x1) / cell_w
            bh = (y2 - y1) / cell_h
            inter = np.minimum(bw, aw) * np.minimum(bh, ah)
            iou = inter / (bw * bh + aw * ah - inter)
            a = int(np.argmax(iou))                      # first maximum
            y_true[gy, gx, a, 0:4] = [cx, cy, bw, bh]
            y_true[gy, gx, a, 4] = 1.
            y_true[gy, gx, a, 5 + int(class_ids[i])] = 1.
            true_boxes[tbi] = [cx, cy, bw, bh]
            tbi = (tbi + 1) % T
    return y_true, true_boxes


def augment_image(image, masks, class_ids, p, cval, T):
    """One image.  image [H,W,3] uint8, masks [H,W,T] 0/1, class_ids [T] (0 = empty slot), p float64[8].
    -> image float32 [H,W,3], masks uint8 [H,W,T], boxes int32 [T,4], ids int32 [T] (compacted, unused slots zero)."""
    H, W = image.shape[:2]
    p = np.asarray(p, np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    x, y = xx.astype(np.float64), yy.astype(np.float64)
    sx = (p[0] * x + p[1] * y) + p[2]
    sy = (p[3] * x + p[4] * y) + p[5]

    # masks: nearest
    fx_, fy_ = np.floor(sx + 0.5), np.floor(sy + 0.5)
    inside = (fx_ >= 0) & (fx_ < W) & (fy_ >= 0) & (fy_ < H)
    ix = np.where(inside, fx_, 0).astype(np.int64)
    iy = np.where(inside, fy_, 0).astype(np.int64)
    warped = (np.asarray(masks)[iy, ix, :] != 0) & inside[:, :, None]          # [H,W,T]
    out_masks = np.zeros((H, W, T), np.uint8)
    out_ids = np.zeros(T, np.int32)
    out_boxes = np.zeros((T, 4), np.int32)
    n = 0
    for t in range(T):
        if class_ids[t] == 0 or not warped[:, :, t].any():
            continue
        m = warped[:, :, t]
        cols = np.where(m.any(axis=0))[0]
        rows = np.where(m.any(axis=1))[0]
        out_masks[:, :, n] = m
        out_ids[n] = class_ids[t]
        out_boxes[n] = (cols[0], rows[0], cols[-1] + 1, rows[-1] + 1)
        n += 1

    # image: bilinear, taps outside the frame read cval
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    img = image.astype(np.float64)

    def tap(yf, xf):
        ok = (xf >= 0) & (xf < W) & (yf >= 0) & (yf < H)
        xi = np.where(ok, xf, 0).astype(np.int64)
        yi = np.where(ok, yf, 0).astype(np.int64)
        return np.where(ok[:, :, None], img[yi, xi, :], float(cval))
    p00, p01 = tap(y0f, x0f), tap(y0f, x0f + 1)
    p10, p11 = tap(y0f + 1, x0f), tap(y0f + 1, x0f + 1)
    fx, fy = fx[:, :, None], fy[:, :, None]
    top = (1 - fx) * p00 + fx * p01
    bot = (1 - fx) * p10 + fx * p11
    v = (1 - fy) * top + fy * bot
    v = np.minimum(np.maximum(p[6] * v + p[7], 0.0), 255.0)
    return (v / 255.0).astype(np.float32), out_masks, out_boxes, out_ids


def augment_batch(images, masks, class_ids, params, cval, H, W, T, G, A, C, anchors):
    """The whole contract for a batch.  -> dict of the six arrays (y_true / true_boxes already cast to float32)."""
    B = len(images)
    out = dict(images=np.zeros((B, H, W, 3), np.float32), gt_masks=np.zeros((B, H, W, T), np.uint8),
               gt_boxes=np.zeros((B, T, 4), np.int32), gt_ids=np.zeros((B, T), np.int32),
               y_true=np.zeros((B, G, G, A, 5 + C), np.float32), true_boxes=np.zeros((B, T, 4), np.float32))
    for b in range(B):
        img, m, boxes, ids = augment_image(images[b], masks[b], class_ids[b], params[b], cval, T)
        n = int((ids != 0).sum())
        yt, tb = encode_targets_raw(boxes[:n], ids[:n], H, W, G, A, C, T, anchors)
        out["images"][b], out["gt_masks"][b], out["gt_boxes"][b], out["gt_ids"][b] = img, m, boxes, ids
        out["y_true"][b], out["true_boxes"][b] = yt.astype(np.float32), tb.astype(np.float32)
    return out


def pack_samples(samples, T):
    """load_image_gt samples -> (images uint8 [B,H,W,3], masks uint8 [B,H,W,T], ids int32 [B,T]) as the device augmenter takes them."""
    B = len(samples)
    H, W = samples[0][0].shape[:2]
    images = np.stack([s[0] for s in samples]).astype(np.uint8)
    masks = np.zeros((B, H, W, T), np.uint8)
    ids = np.zeros((B, T), np.int32)
    for b, s in enumerate(samples):
        n = s[1].shape[0]
        ids[b, :n] = s[1]
        masks[b, :, :, :n] = s[3]
    return images, masks, ids


def augment_cfg_batch(samples, params, cfg, cval=0.0):
    images, masks, ids = pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    H, W = cfg.IMAGE_SHAPE[0], cfg.IMAGE_SHAPE[1]
    return augment_batch(images, masks, ids, params, cval, H, W, cfg.TRUE_BOX_BUFFER, cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES,
                         np.asarray(cfg.ANCHORS, np.float64))

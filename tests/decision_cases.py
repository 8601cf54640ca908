"""Edge tables for the decision kernels of csrc/exact_kernels.hip ("Edge tables of the exact kernels"): the inputs, as plain numpy, at
which target assignment, box decoding and the loss counts can go wrong.  tests/test_decision_cases_host.py proves with the oracle alone that every
case sits on the edge it names and that a wrong rule changes its output; tests/test_gpu_decisions.py holds the kernels to the oracle on them.

Every builder is cached: the tables are built once per session and must not be modified by a test."""
import functools

import numpy as np

from oracle import np_ops as O
from myolo.config import make_config, ShapesConfig

F32 = np.float32
MASK = 28


# ------------------------------------------------------------------------------------------------------------------------------------------
# target assignment
# ------------------------------------------------------------------------------------------------------------------------------------------
def targets_cfg(size, nbox, T):
    """R = (size / 32)^2 * nbox proposals per image, T ground-truth slots."""
    return make_config(ShapesConfig, IMAGE_SHAPE=[size, size, 3], N_BOX=nbox, ANCHORS=[1.0, 1.0] * nbox, TRUE_BOX_BUFFER=T, MAX_GT_INSTANCES=T)


def _blank(name, size, nbox, T, B, edge):
    R = (size // 32) ** 2 * nbox
    return dict(name=name, size=size, nbox=nbox, T=T, B=B, R=R, edge=edge,
                prop=np.zeros((B, R, 4), F32), gt_ids=np.zeros((B, T), np.int32), gt_boxes=np.zeros((B, T, 4), np.int32),
                gt_masks=np.zeros((B, size, size, T), bool))


def _put_box(c, b, k, box_px, cls, shape="ellipse"):
    """ground-truth slot k of image b: pixel box (x1, y1, x2, y2), x2 / y2 exclusive, and a mask inside it"""
    x1, y1, x2, y2 = box_px
    c["gt_boxes"][b, k] = box_px
    c["gt_ids"][b, k] = cls
    yy, xx = np.mgrid[0:c["size"], 0:c["size"]]
    inside = (xx >= x1) & (xx < x2) & (yy >= y1) & (yy < y2)
    if shape == "ellipse":
        w, h = x2 - x1, y2 - y1
        inside &= ((xx - (x1 + w / 2)) ** 2 / (w / 2) ** 2 + (yy - (y1 + h / 2)) ** 2 / (h / 2) ** 2) <= 1
    elif shape == "stripes":
        inside &= (xx + 2 * yy) % 3 != 0
    c["gt_masks"][b, :, :, k] = inside


def gt_norm(c, b, k):
    return O.norm_boxes(c["gt_boxes"][b, k:k + 1], c["size"], c["size"])[0]


def _near(rng, c, b, k):
    """a proposal within 3 % of slot k's box on every side: IoU >= (0.94 / 1.06)^2 = 0.78"""
    g = gt_norm(c, b, k)
    w, h = g[2] - g[0], g[3] - g[1]
    j = (rng.random(4).astype(F32) - F32(0.5)) * F32(0.06) * np.array([w, h, w, h], F32)
    return (g + j).astype(F32)


def _far(rng):
    """a proposal of side 0.01 .. 0.02: at most 4e-4 of area, IoU < 0.05 with any box used here (sides >= 0.1)"""
    ctr, s = rng.random(2) * 0.9 + 0.05, rng.random(2) * 0.01 + 0.01
    return np.concatenate([ctr - s / 2, ctr + s / 2]).astype(F32)


def _grid_boxes(c, b, n, rng):
    """n boxes tiled over the image, one per tile"""
    size = c["size"]
    per = int(np.ceil(np.sqrt(n)))
    tile = size // per
    for k in range(n):
        x0, y0 = (k % per) * tile, (k // per) * tile
        _put_box(c, b, k, [x0 + 1, y0 + 1, x0 + tile - 1, y0 + tile - 1], 1 + k % 3, ("ellipse", "box", "stripes")[k % 3])


def _four_images(name, size, nbox, T, seed):
    """image 0: every slot used, proposals mixed; 1: no slot used; 2: every proposal positive; 3: boxes but no positive proposal"""
    c = _blank(name, size, nbox, T, 4, "T = %d: all slots used / none used / all proposals positive / none positive" % T)
    rng = np.random.default_rng(seed)
    R = c["R"]
    _grid_boxes(c, 0, T, rng)
    _grid_boxes(c, 2, max(1, T // 2), rng)
    _grid_boxes(c, 3, max(1, T // 3), rng)
    for r in range(R):
        c["prop"][0, r] = _near(rng, c, 0, (T - 1 - 4 * (r // 3)) % T) if r % 3 == 0 else _far(rng)     # slots T - 1, T - 5, ...
        c["prop"][1, r] = _far(rng) if r % 2 else _near(rng, c, 0, r % T)
        c["prop"][2, r] = _near(rng, c, 2, r % max(1, T // 2))
        c["prop"][3, r] = _far(rng)
    return c


def _chunk_case(name, size, nbox, every, border_rows, seed):
    """R > 256: image 0 has a positive every `every` rows (all 256-proposal chunks, the ragged last one included); image 1 has positives on the
    chunk borders only"""
    c = _blank(name, size, nbox, 10, 2, "R = %d: positives in every 256-chunk and on the chunk borders")
    c["edge"] = c["edge"] % c["R"]
    rng = np.random.default_rng(seed)
    for b in range(2):
        _put_box(c, b, 0, [10, 20, 90, 100], 1)
        _put_box(c, b, 1, [size - 120, size - 100, size - 20, size - 10], 2, "stripes")
        _put_box(c, b, 2, [120, 10, 200, 80], 3, "box")
    R = c["R"]
    for r in range(R):
        c["prop"][0, r] = _near(rng, c, 0, r % 3) if r % every == 0 else _far(rng)
        c["prop"][1, r] = _near(rng, c, 1, r % 3) if r in border_rows else _far(rng)
    return c


def _search_iou_half():
    """-> (box_px, p_eq, p_lo): IoU(p_eq, box) == float32(0.5) under O.overlaps; p_lo is p_eq with x2 one float32 step lower and IoU < 0.5"""
    size = 96
    just_below = np.nextafter(F32(0.5), F32(0), dtype=F32)
    found = [s for s in _iou_half_candidates(size)]
    best = [s for s in found if s[3] == just_below] or found          # prefer a neighbour whose IoU is the float32 just below 0.5
    if not best:
        raise AssertionError("no proposal with IoU == 0.5 found")
    return best[0][:3]


def _iou_half_candidates(size):
    for x2px in range(40, 90):
        for y2px in range(30, 90, 7):
            g = O.norm_boxes(np.array([[8, 6, x2px, y2px]], np.int32), size, size)
            mid = F32(g[0, 0] + (g[0, 2] - g[0, 0]) / F32(2))
            x = np.nextafter(mid, F32(-1), dtype=F32)
            for _ in range(8):
                x = np.nextafter(x, F32(-1), dtype=F32)
            prev = None
            for _ in range(24):
                p = np.array([[g[0, 0], g[0, 1], x, g[0, 3]]], F32)
                v = O.overlaps(p, g)[0, 0]
                if prev is not None and v == F32(0.5) and prev[1] < F32(0.5):
                    yield [8, 6, x2px, y2px], p[0], prev[0], prev[1]
                prev = (p[0], v)
                x = np.nextafter(x, F32(2), dtype=F32)


def _search_sample_box(size, step):
    """-> (a, lo, hi): a square proposal [lo, hi]^2 whose 28 sample coordinates, as tf.image.crop_and_resize (O._crop_coords) computes them in
    float32, are exactly a + step * i"""
    span = step * (MASK - 1)
    for a in range(0, int(size - 1 - span) + 1):
        lo0, hi0 = F32(a) / F32(size - 1), F32(a + span) / F32(size - 1)
        for dl in range(-2, 3):
            for dh in range(-2, 3):
                lo, hi = lo0, hi0
                for _ in range(abs(dl)):
                    lo = np.nextafter(lo, F32(np.sign(dl) * 4), dtype=F32)
                for _ in range(abs(dh)):
                    hi = np.nextafter(hi, F32(np.sign(dh) * 4), dtype=F32)
                co = O._crop_coords(np.array([lo], F32), np.array([hi], F32), size, MASK)[0]
                if np.array_equal(co, (a + step * np.arange(MASK)).astype(F32)):
                    yield a, lo, hi


@functools.lru_cache(maxsize=None)
def target_cases():
    cases = []
    # ---- sizes ----------------------------------------------------------------------------------------------------------------------------
    cases.append(_four_images("r45_t1", 96, 5, 1, 21))                                  # R < 64, T = 1
    cases.append(_four_images("r48_t64", 128, 3, 64, 22))                               # R < 64, T = 64 (the entry's limit)
    c = _blank("r147", 224, 3, 10, 2, "R = 147: three waves, the last one ragged")
    rng = np.random.default_rng(23)
    for b in range(2):
        _put_box(c, b, 0, [10, 20, 90, 100], 1)
        _put_box(c, b, 1, [100, 110, 200, 210], 2, "stripes")
        _put_box(c, b, 2, [120, 10, 200, 80], 3, "box")
        for r in range(c["R"]):
            c["prop"][b, r] = _near(rng, c, b, r % 3) if (r + b) % 2 == 0 else _far(rng)
    cases.append(c)
    cases.append(_chunk_case("r294_chunks", 224, 6, 5, (0, 255, 256, 293), 24))        # 7 * 7 * 6: two chunks, 38 rows in the last
    cases.append(_chunk_case("r676_chunks", 416, 4, 17, (255, 256, 511, 512, 675), 25))  # 13 * 13 * 4: three chunks

    # ---- IoU exactly 0.5 and one step below -----------------------------------------------------------------------------------------------
    box, p_eq, p_lo = _search_iou_half()
    c = _blank("iou_half", 96, 5, 4, 1, "row 0: IoU == 0.5 (positive); row 1: x2 one float32 step lower, IoU < 0.5 (negative)")
    rng = np.random.default_rng(26)
    _put_box(c, 0, 0, box, 2)
    for r in range(c["R"]):
        c["prop"][0, r] = _far(rng)
    c["prop"][0, 0], c["prop"][0, 1] = p_eq, p_lo
    c["prop"][0, 7] = _near(rng, c, 0, 0)
    cases.append(c)

    # ---- equal ground-truth boxes, behind a slot that trim_zeros removes --------------------------------------------------------------------
    c = _blank("equal_gt", 96, 5, 4, 2, "slots 1 and 2 hold the same box (classes 1 / 2, different masks) behind a trimmed slot 0: the first kept wins")
    rng = np.random.default_rng(27)
    for b in range(2):
        _put_box(c, b, 0, [0, 0, 1, 1], 3, "box")                                       # normalises to all zeros: trimmed, its mask pixel stays
        _put_box(c, b, 1, [20, 30, 70, 80], 1, "ellipse")
        _put_box(c, b, 2, [20, 30, 70, 80], 2, "stripes")
        for r in range(c["R"]):
            c["prop"][b, r] = _near(rng, c, b, 1) if r % 2 == b else _far(rng)
    cases.append(c)

    # ---- zero-area proposals: NaN against a zero-area box (image 0), 0 against ordinary boxes (image 1) -------------------------------------
    c = _blank("zero_area", 96, 5, 4, 2, "zero-area proposals: IoU NaN against the 1-pixel-wide box of image 0 (dropped), 0 in image 1 (negative)")
    rng = np.random.default_rng(28)
    _put_box(c, 0, 0, [5, 5, 6, 9], 1, "box")                                           # x1 == x2 once normalised, not all zeros: kept
    _put_box(c, 0, 1, [30, 30, 80, 70], 2)
    _put_box(c, 1, 1, [30, 30, 80, 70], 2)
    for b in range(2):
        for r in range(c["R"]):
            if r % 4 == 1:                                                              # zero area: x1 == x2, or y1 == y2, or the all-zero row
                p = _far(rng)
                c["prop"][b, r] = [(p[0], p[1], p[0], p[3]), (p[0], p[1], p[2], p[1]), (0, 0, 0, 0)][(r // 4) % 3]
            else:
                c["prop"][b, r] = _near(rng, c, b, 1) if r % 4 == 0 else _far(rng)
    cases.append(c)

    # ---- a proposal with x2 < x1 --------------------------------------------------------------------------------------------------------------
    c = _blank("flipped", 96, 5, 4, 1, "rows 0 and 3: a matching box with x1 and x2 swapped: area < 0, intersection 0, negative")
    rng = np.random.default_rng(29)
    _put_box(c, 0, 0, [30, 30, 80, 70], 2)
    for r in range(c["R"]):
        c["prop"][0, r] = _near(rng, c, 0, 0) if r % 5 == 1 else _far(rng)
    for r in (0, 3):
        p = _near(rng, c, 0, 0)
        c["prop"][0, r] = [p[2], p[1], p[0], p[3]]
    cases.append(c)

    # ---- a positive proposal reaching outside the image -------------------------------------------------------------------------------------
    c = _blank("outside", 96, 5, 4, 1, "positive proposals reaching past the image's corners: their outside samples are 0")
    rng = np.random.default_rng(30)
    _put_box(c, 0, 0, [0, 0, 40, 40], 1, "box")
    _put_box(c, 0, 1, [50, 50, 96, 96], 2, "box")
    for r in range(c["R"]):
        c["prop"][0, r] = _far(rng)
    c["prop"][0, 2] = [-0.05, -0.04, 0.43, 0.42]
    c["prop"][0, 5] = [0.5, 0.52, 1.06, 1.05]
    c["prop"][0, 9] = _near(rng, c, 0, 0)
    cases.append(c)

    # ---- samples exactly on pixel centres, the last one on pixel H - 1 ----------------------------------------------------------------------
    size = 96
    a, lo, hi = next(s for s in _search_sample_box(size, 1.0) if s[0] + MASK - 1 == size - 1)
    c = _blank("pixel_centres", size, 5, 4, 1, "row 4: every sample on a pixel centre (%d .. %d), the last on pixel H - 1" % (a, size - 1))
    rng = np.random.default_rng(31)
    _put_box(c, 0, 0, [a, a, size, size], 3, "stripes")
    for r in range(c["R"]):
        c["prop"][0, r] = _far(rng)
    c["prop"][0, 4] = [lo, lo, hi, hi]
    c["sample_lo_hi"] = (a, lo, hi)
    cases.append(c)

    # ---- a bilinear value of exactly 0.5 ------------------------------------------------------------------------------------------------------
    a, lo, hi = next(s for s in _search_sample_box(size, 0.5) if s[0] >= 8)
    c = _blank("bilinear_half", size, 5, 4, 1, "row 6: samples every half pixel over columns of alternating 1 / 0: values of exactly 0.5 round to 0")
    rng = np.random.default_rng(32)
    _put_box(c, 0, 0, [a, a, a + 15, a + 15], 1, "box")
    yy, xx = np.mgrid[0:size, 0:size]
    c["gt_masks"][0, :, :, 0] = ((xx % 2 == 0) & (yy < a + 8)) | ((yy >= a + 8) & (xx < a + 5))
    for r in range(c["R"]):
        c["prop"][0, r] = _far(rng)
    c["prop"][0, 6] = [lo, lo, hi, hi]
    c["sample_lo_hi"] = (a, lo, hi)
    cases.append(c)
    for c in cases:
        for k in ("prop", "gt_ids", "gt_boxes", "gt_masks"):
            c[k].setflags(write=False)
    return tuple(cases)


def target_case(name):
    return next(c for c in target_cases() if c["name"] == name)


TARGET_NAMES = ("r45_t1", "r48_t64", "r147", "r294_chunks", "r676_chunks", "iou_half", "equal_gt", "zero_area", "flipped", "outside",
                "pixel_centres", "bilinear_half")


@functools.lru_cache(maxsize=None)
def target_reference(name):
    """O.mask_targets of the case: (rois, class ids, masks, n_pos), computed once"""
    c = target_case(name)
    out = O.mask_targets(c["prop"], c["gt_ids"], c["gt_boxes"], c["gt_masks"], targets_cfg(c["size"], c["nbox"], c["T"]))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# decode and detections
# ------------------------------------------------------------------------------------------------------------------------------------------
# coordinate and confidence logits around the clamp of det_expf / myolo_expf ([-86, 88]); sigmoid(-88) = 1 / (1 + e^88) is a subnormal
SPECIAL_LOGITS = np.array([v for m in (0.0, 1e-30, 85.9, 86.0, 88.0, 88.1, 100.0, 3e38, np.inf) for v in (m, -m)], F32)

DECODE_SHAPES = (("g1a1c1", 4, 1, 1, 1), ("g1a3c2", 4, 1, 3, 2), ("g13a5c81", 2, 13, 5, 81), ("g7a3c4_441", 3, 7, 3, 4))


@functools.lru_cache(maxsize=None)
def decode_case(name):
    """-> dict(y_pred [B, G, G, A, 5 + C], anchors [2 A]): the s-th special row's column j (j < 5) holds SPECIAL_LOGITS[(s + 7 j) % 18], two rows out of three being special
    (every value in every column once there are 54 rows; the 4- and 12-row grids hold what fits), an ordinary logit otherwise; the class logits
    cycle through: all equal, a tie of two maxima, the maximum in the last slot, -0 against +0, random"""
    _, B, G, A, C = next(s for s in DECODE_SHAPES if s[0] == name)
    rng = np.random.default_rng(40 + G + A + C)
    total = B * G * G * A
    yp = (rng.standard_normal((total, 5 + C)) * 2).astype(F32)
    n, s = len(SPECIAL_LOGITS), 0
    for i in range(total):
        if i % 3 != 2 or total < n:
            for j in range(5):
                yp[i, j] = SPECIAL_LOGITS[(s + 7 * j) % n]
            s += 1
        kind = i % 5
        cl = yp[i, 5:]
        if kind == 0:
            cl[:] = F32(rng.standard_normal())
        elif kind == 1 and C > 1:
            lo_i, hi_i = sorted(rng.choice(C, 2, replace=False).tolist())
            cl[lo_i] = cl[hi_i] = F32(np.abs(cl).max() + 1)
        elif kind == 2:
            cl[C - 1] = F32(np.abs(cl).max() + 1)
        elif kind == 3:
            cl[:] = F32(-0.0)
            cl[C - 1] = F32(0.0)
    anchors = (rng.random(2 * A) * 4 + 0.5).astype(F32)
    yp = yp.reshape(B, G, G, A, 5 + C)
    yp.setflags(write=False)
    anchors.setflags(write=False)
    return dict(name=name, B=B, G=G, A=A, C=C, y_pred=yp, anchors=anchors)


@functools.lru_cache(maxsize=None)
def decode_reference(name):
    c = decode_case(name)
    with np.errstate(over="ignore"):
        prop, det = O.yolo_decode(c["y_pred"], c["anchors"], c["G"]), O.yolo_detections(c["y_pred"], c["anchors"], c["G"])
    prop.setflags(write=False)
    det.setflags(write=False)
    return prop, det


# ------------------------------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------------------------------
WH_LIMIT = 12.0          # beyond it the oracle's loss_wh overflows float32


def loss_cfg(G, A, C, T):
    cw = (0.25 + 0.5 * (np.arange(C) % 5)).astype(F32)                                   # non-uniform: 0.25 .. 2.25
    anchors = [float(v) for v in (1.0 + 0.75 * np.arange(2 * A) % 5)]
    return make_config(ShapesConfig, IMAGE_SHAPE=[32 * G, 32 * G, 3], N_BOX=A, ANCHORS=anchors, NUM_CLASSES=C, CLASS_WEIGHTS=cw,
                       TRUE_BOX_BUFFER=T, MAX_GT_INSTANCES=T, COORD_SCALE=2.0, NO_OBJECT_SCALE=0.5, CLASS_SCALE=1.5)


# name, B, G, A, C, T, objects per image ("full" = every true-box slot), logit scale
LOSS_SHAPES = (("one_predictor", 1, 1, 1, 2, 1, 1, 4.0),
               ("b257", 257, 1, 1, 2, 1, 1, 4.0),
               ("full_t64_c81", 4, 13, 5, 81, 64, "full", 4.0),
               ("no_object", 3, 7, 3, 2, 1, 0, 4.0),
               ("two_in_a_cell", 2, 7, 3, 2, 64, 2, 4.0))


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """-> dict(y_true, y_pred [B, G, G, A, 5 + C], true_boxes [B, 1, 1, 1, T, 4]).  Every object k of an image has its own cell (except in
    two_in_a_cell: one cell, two anchors); its own predictor predicts it loosely, and ANOTHER anchor of the same cell predicts it tightly: that
    predictor has no object of its own and a best IoU above 0.6 that only the object's true-box slot gives it, so it leaves the no-object mask."""
    _, B, G, A, C, T, nobj, scale = next(s for s in LOSS_SHAPES if s[0] == name)
    cfg = loss_cfg(G, A, C, T)
    rng = np.random.default_rng(50 + B + G + C + T)
    yp = (rng.standard_normal((B, G, G, A, 5 + C)) * scale).astype(F32)
    yp[..., 2:4] = np.clip(yp[..., 2:4], -WH_LIMIT, WH_LIMIT)
    yt = np.zeros_like(yp)
    tb = np.zeros((B, 1, 1, 1, T, 4), F32)
    anc = np.asarray(cfg.ANCHORS, F32).reshape(A, 2)
    for b in range(B):
        n = T if nobj == "full" else nobj
        if name == "b257" and b % 3 == 2:
            n = 0
        cells = rng.permutation(G * G)[:n] if name != "two_in_a_cell" else np.full(n, rng.integers(0, G * G))
        for k in range(n):
            gy, gx = int(cells[k]) // G, int(cells[k]) % G
            a = k % A if name == "two_in_a_cell" else int(rng.integers(0, A))
            box = np.array([gx + 0.2 + 0.6 * rng.random(), gy + 0.2 + 0.6 * rng.random(), 0.5 + 3 * rng.random(), 0.5 + 3 * rng.random()], F32)
            yt[b, gy, gx, a, :4] = box
            yt[b, gy, gx, a, 4] = 1
            yt[b, gy, gx, a, 5 + int(rng.integers(0, C))] = 1
            tb[b, 0, 0, 0, k] = box
            off = np.array([box[0] - gx, box[1] - gy], np.float64)
            xy_logit = np.log(off / (1 - off))

            def pred(an, dw):
                return np.concatenate([xy_logit, np.log(box[2:4].astype(np.float64) / anc[an]) + dw]).astype(F32)
            yp[b, gy, gx, a, :4] = pred(a, 0.25)                                          # its own predictor: IoU about 0.6
            if A > 1 and name != "two_in_a_cell":
                yp[b, gy, gx, (a + 1) % A, :4] = pred((a + 1) % A, 0.02)                  # a neighbour without an object: IoU about 0.95
            elif name == "two_in_a_cell" and k == n - 1:
                yp[b, gy, gx, 2, :4] = pred(2, 0.02)
    for arr in (yt, yp, tb):
        arr.setflags(write=False)
    return dict(name=name, B=B, G=G, A=A, C=C, T=T, cfg=cfg, y_true=yt, y_pred=yp, true_boxes=tb, n_objects=int(yt[..., 4].sum()))


@functools.lru_cache(maxsize=None)
def loss_reference(name, warmup):
    c = loss_case(name)
    return O.yolo_loss(c["y_true"], c["y_pred"], c["true_boxes"], c["cfg"], want_grad=True, warmup=bool(warmup))

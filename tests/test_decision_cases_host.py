"""The edge tables of tests/decision_cases.py, proved on the CPU with the oracle alone (no GPU): every case sits on the edge it names, and every
case is SENSITIVE -- a numpy restatement of the rule (built from the oracle's own pieces, equal to the oracle with no rule changed) gives another
output on it once one deliberately wrong rule is switched in.  The tables below name, case by case, the edge and the wrong rules it catches;
tests/test_gpu_decisions.py then holds the kernels to the oracle on the same inputs.

WRONG RULES for target assignment (restate_targets):
  nan_skipped        the row maximum skips a NaN IoU (`if (iou > best)`: the kernel before the NaN rule of DESIGN.md) instead of propagating it
  gt                 positive when max IoU > 0.5 instead of >= 0.5
  last_max           the last of equal maxima wins instead of the first
  arg_untrimmed      the winning index is read against the untrimmed slots instead of the kept ones
  drop_zero_area     a zero-area proposal is dropped as padding instead of being a negative
  sort_corners       a proposal's corners are put in order first
  clamp_outside      a sample outside the image reads the edge pixel instead of 0
  strict_upper       a sample on pixel H - 1 exactly counts as outside
  half_away          a bilinear 0.5 rounds away from zero instead of to even
  no_chunk_carry     the ranks of a 256-proposal chunk start again at 0
  ragged_chunk_lost  the proposals of the last, partial chunk are not placed
  subsample_third    at most R / 3 positives are kept (Mask R-CNN's ROI_POSITIVE_RATIO, commented out in the reference)
  t_limit_32         only the first 32 ground-truth slots are looked at"""
import numpy as np
import pytest

import decision_cases as DC
from oracle import np_ops as O

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------------------
# target assignment
# ------------------------------------------------------------------------------------------------------------------------------------------
def _crop_one(mask2d, box_xyxy, rule):
    """crop_and_resize of one [H, W] 0 / 1 mask to 28 x 28 over the proposal (x1, y1, x2, y2), float32 in the oracle's operation order"""
    H, W = mask2d.shape
    x1, y1, x2, y2 = [np.array([v], F32) for v in box_xyxy]
    iy = O._crop_coords(y1, y2, H, DC.MASK)[0]
    ix = O._crop_coords(x1, x2, W, DC.MASK)[0]
    if "strict_upper" in rule:
        vy, vx = ~((iy < 0) | (iy >= F32(H - 1))), ~((ix < 0) | (ix >= F32(W - 1)))
    else:
        vy, vx = ~((iy < 0) | (iy > F32(H - 1))), ~((ix < 0) | (ix > F32(W - 1)))
    if "clamp_outside" in rule:
        iy, ix = np.clip(iy, 0, F32(H - 1)), np.clip(ix, 0, F32(W - 1))
        vy, vx = np.ones_like(vy), np.ones_like(vx)
    ty, lx = np.floor(iy), np.floor(ix)
    wy, wx = (iy - ty).astype(F32)[:, None], (ix - lx).astype(F32)[None, :]
    tyi, byi = np.clip(ty, 0, H - 1).astype(int)[:, None], np.clip(np.ceil(iy), 0, H - 1).astype(int)[:, None]
    lxi, rxi = np.clip(lx, 0, W - 1).astype(int)[None, :], np.clip(np.ceil(ix), 0, W - 1).astype(int)[None, :]
    m = mask2d.astype(F32)
    top = m[tyi, lxi] + (m[tyi, rxi] - m[tyi, lxi]) * wx
    bot = m[byi, lxi] + (m[byi, rxi] - m[byi, lxi]) * wx
    val = (top + (bot - top) * wy).astype(F32)
    return np.where(vy[:, None] & vx[None, :], val, F32(0)).astype(F32)


def restate_targets(c, rule=()):
    """the kernel's structure in numpy: IoU rows, their maximum, flags, ranks by chunks of 256, scatter, crop and round"""
    rule = frozenset(rule)
    size, R, T = c["size"], c["R"], c["T"]
    gtn_all = O.norm_boxes(c["gt_boxes"], size, size)
    rois, cls = np.zeros((c["B"], R, 4), F32), np.zeros((c["B"], R), np.int32)
    masks, npos_out = np.zeros((c["B"], R, DC.MASK, DC.MASK), F32), np.zeros(c["B"], np.int32)
    for b in range(c["B"]):
        prop, gtn = c["prop"][b], gtn_all[b]
        keep = np.where(np.abs(gtn).sum(1) != 0)[0]
        if "t_limit_32" in rule:
            keep = keep[keep < 32]
        p = prop
        if "sort_corners" in rule:
            p = np.stack([np.minimum(p[:, 0], p[:, 2]), np.minimum(p[:, 1], p[:, 3]), np.maximum(p[:, 0], p[:, 2]), np.maximum(p[:, 1], p[:, 3])], 1)
        ov = O.overlaps(p, gtn[keep])
        finite = np.where(np.isnan(ov), F32(-np.inf), ov)
        if len(keep) == 0:
            best, arg = np.full(R, -np.inf, F32), np.zeros(R, int)
        else:
            best = finite.max(1) if "nan_skipped" in rule else ov.max(1)
            arg = (len(keep) - 1 - np.argmax(finite[:, ::-1], 1)) if "last_max" in rule else np.argmax(finite, 1)
        pos = (best > F32(0.5)) if "gt" in rule else (best >= F32(0.5))
        neg = best < F32(0.5)
        if "drop_zero_area" in rule:
            neg &= ((prop[:, 3] - prop[:, 1]) * (prop[:, 2] - prop[:, 0])) != 0
        if "subsample_third" in rule:
            pos &= (np.cumsum(pos) <= R // 3)
        if "ragged_chunk_lost" in rule and R > 256:
            pos[(R // 256) * 256:] = False
            neg[(R // 256) * 256:] = False
        rank_p, rank_n = np.cumsum(pos) - pos, np.cumsum(neg) - neg
        npos = int(pos.sum())
        if "no_chunk_carry" in rule:
            for r0 in range(256, R, 256):
                rank_p[r0:r0 + 256] -= rank_p[r0]
                rank_n[r0:r0 + 256] -= rank_n[r0]
        src = np.full(R, -1)
        for r in range(R):
            if pos[r] or neg[r]:
                src[rank_p[r] if pos[r] else npos + rank_n[r]] = r
        slot = arg if "arg_untrimmed" in rule else (keep[arg] if len(keep) else arg)
        for d in range(R):
            r = src[d]
            if r < 0:
                continue
            rois[b, d] = prop[r]
            if d < npos:
                cls[b, d] = c["gt_ids"][b, slot[r]]
                v = _crop_one(c["gt_masks"][b, :, :, slot[r]], p[r], rule)
                masks[b, d] = np.floor(v + F32(0.5)) if "half_away" in rule else np.rint(v)
        npos_out[b] = npos
    return rois, cls, masks, npos_out


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# case -> the wrong rules that must change its output
TARGET_RULES = {
    "r45_t1": ("subsample_third",),
    "r48_t64": ("subsample_third", "t_limit_32"),
    "r147": ("subsample_third",),
    "r294_chunks": ("no_chunk_carry", "ragged_chunk_lost"),
    "r676_chunks": ("no_chunk_carry", "ragged_chunk_lost"),
    "iou_half": ("gt",),
    "equal_gt": ("last_max", "arg_untrimmed"),
    "zero_area": ("nan_skipped", "drop_zero_area"),
    "flipped": ("sort_corners",),
    "outside": ("clamp_outside",),
    "pixel_centres": ("strict_upper",),
    "bilinear_half": ("half_away",),
}


def test_every_target_case_is_listed():
    assert tuple(c["name"] for c in DC.target_cases()) == DC.TARGET_NAMES
    assert set(TARGET_RULES) == set(DC.TARGET_NAMES) and all(TARGET_RULES.values())
    for c in DC.target_cases():
        assert c["size"] <= 416 and c["B"] <= 4 and c["T"] <= 64


@pytest.mark.parametrize("name", DC.TARGET_NAMES)
def test_targets_restatement_is_the_oracle(name):
    assert _same(restate_targets(DC.target_case(name)), DC.target_reference(name))


@pytest.mark.parametrize("name,rule", [(n, r) for n in DC.TARGET_NAMES for r in TARGET_RULES[n]])
def test_targets_wrong_rule_changes_the_case(name, rule):
    c = DC.target_case(name)
    got, want = restate_targets(c, (rule,)), DC.target_reference(name)
    assert not _same(got, want), "%s (%s) does not notice the wrong rule %r" % (name, c["edge"], rule)
    print("%-14s %-18s caught   [%s]" % (name, rule, c["edge"]))


def _row_max(c, b):
    gtn = O.norm_boxes(c["gt_boxes"][b], c["size"], c["size"])
    keep = np.abs(gtn).sum(1) != 0
    return O.overlaps(c["prop"][b], gtn[keep]), keep


def test_target_sizes():
    R = {n: DC.target_case(n)["R"] for n in DC.TARGET_NAMES}
    assert R["r45_t1"] == 45 and R["r48_t64"] == 48 and R["r147"] == 147 and R["r294_chunks"] == 294 and R["r676_chunks"] == 676
    assert 256 < R["r294_chunks"] <= 512 and R["r294_chunks"] % 64 != 0 and R["r676_chunks"] > 512
    assert DC.target_case("r45_t1")["T"] == 1 and DC.target_case("r48_t64")["T"] == 64
    for name in ("r45_t1", "r48_t64"):
        c, npos = DC.target_case(name), DC.target_reference(name)[3]
        used = (c["gt_boxes"].reshape(4, c["T"], 4) != 0).any(2).sum(1)
        assert used[0] == c["T"] and used[1] == 0, "image 0 uses every slot, image 1 none"
        assert 0 < npos[0] < c["R"] and npos[1] == 0 and npos[2] == c["R"] and npos[3] == 0 and used[3] > 0
        # an unused slot is NOT trimmed: its pixel row of zeros normalises to (0, 0, -1 / (W - 1), -1 / (H - 1))
        assert _row_max(c, 1)[1].all()
    # R = 48, one positive in three: the 16 positives of the T = 64 image belong to slots 63, 59, ... 3 -- both halves of the slot range
    cls, npos = DC.target_reference("r48_t64")[1], DC.target_reference("r48_t64")[3]
    assert npos[0] == 16 and np.array_equal(cls[0, :16], DC.target_case("r48_t64")["gt_ids"][0, 63 - 4 * np.arange(16)])
    for name in ("r294_chunks", "r676_chunks"):
        c = DC.target_case(name)
        for b in range(2):
            pos = np.where(_row_max(c, b)[0].max(1) >= F32(0.5))[0]
            chunks = set((pos // 256).tolist())
            assert chunks == set(range((c["R"] + 255) // 256)), "positives in every 256-chunk, the ragged last one included"
        pos = np.where(_row_max(c, 1)[0].max(1) >= F32(0.5))[0]
        assert c["R"] - 1 in pos and 255 in pos and 256 in pos, "image 1: positives on the chunk borders"


def test_iou_half_is_exact():
    c = DC.target_case("iou_half")
    ov, _ = _row_max(c, 0)
    assert ov.dtype == np.float32 and ov[0, 0] == F32(0.5) and ov[1, 0] < F32(0.5)
    assert np.array_equal(c["prop"][0, 0, [0, 1, 3]], c["prop"][0, 1, [0, 1, 3]])
    assert np.nextafter(c["prop"][0, 0, 2], F32(0), dtype=F32) == c["prop"][0, 1, 2], "the neighbour's x2 is one float32 step lower"
    print("IoU %r and %r (0.5 - %g)" % (ov[0, 0], ov[1, 0], 0.5 - float(ov[1, 0])))
    rois, cls, _, npos = DC.target_reference("iou_half")
    assert npos[0] == 2 and np.array_equal(rois[0, 0], c["prop"][0, 0]) and np.array_equal(rois[0, 1], c["prop"][0, 7])
    assert np.array_equal(rois[0, 2], c["prop"][0, 1]), "the neighbour is the first negative"


def test_equal_gt_first_kept_wins():
    c = DC.target_case("equal_gt")
    assert np.array_equal(c["gt_boxes"][0, 1], c["gt_boxes"][0, 2]) and c["gt_ids"][0, 1] != c["gt_ids"][0, 2]
    assert not np.array_equal(c["gt_masks"][0, :, :, 1], c["gt_masks"][0, :, :, 2])
    ov, keep = _row_max(c, 0)
    assert keep.tolist() == [False, True, True, True], "slot 0 (pixel box 0, 0, 1, 1) normalises to zeros and is trimmed"
    assert np.array_equal(ov[:, 0], ov[:, 1])
    _, cls, _, npos = DC.target_reference("equal_gt")
    assert npos.min() > 0 and all((cls[b, :npos[b]] == c["gt_ids"][b, 1]).all() for b in range(2))


def test_zero_area_nan_and_zero():
    c = DC.target_case("zero_area")
    area = (c["prop"][..., 3] - c["prop"][..., 1]) * (c["prop"][..., 2] - c["prop"][..., 0])
    g = O.norm_boxes(c["gt_boxes"][0], 96, 96)[0]
    assert g[0] == g[2] and np.abs(g).sum() != 0, "the 1-pixel-wide box has x1 == x2 once normalised and is kept"
    ov0, ov1 = _row_max(c, 0)[0], _row_max(c, 1)[0]
    zero = area[0] == 0
    assert zero.sum() == 11 and np.array_equal(area[1] == 0, zero)
    assert np.isnan(ov0[zero, 0]).all() and not np.isnan(ov0[~zero]).any() and not np.isnan(ov0[:, 1:]).any()
    assert not np.isnan(ov1).any() and (ov1[zero] == 0).all()
    rois, _, _, npos = DC.target_reference("zero_area")
    # image 0: the 11 proposals are dropped, the tail is zero-padded; image 1: they are negatives, in place
    assert (np.abs(rois[0, 45 - 11:]).sum() == 0) and (np.abs(rois[0, :45 - 11]).sum(1) != 0).all()
    first_neg = np.where(ov1.max(1) < F32(0.5))[0]
    assert np.array_equal(rois[1, npos[1]:], c["prop"][1, first_neg])
    # the kernel before the NaN rule keeps them as negatives: image 0 changes, image 1 does not
    old = restate_targets(c, ("nan_skipped",))
    assert not np.array_equal(old[0][0], rois[0]) and np.array_equal(old[0][1], rois[1])
    assert (np.abs(old[0][0]).sum(1) != 0).sum() == 45 - 3, "every proposal but the three all-zero rows is placed by the old rule"


def test_flipped_proposal_is_negative():
    c = DC.target_case("flipped")
    ov = _row_max(c, 0)[0]
    for r in (0, 3):
        assert c["prop"][0, r, 2] < c["prop"][0, r, 0] and (ov[r] == 0).all(), "x2 < x1: intersection 0, IoU 0 (not NaN)"
    assert restate_targets(c, ("sort_corners",))[3][0] == DC.target_reference("flipped")[3][0] + 2


def test_outside_samples_are_zero():
    c = DC.target_case("outside")
    rois, _, masks, npos = DC.target_reference("outside")
    assert npos[0] == 3 and np.array_equal(rois[0, 0], c["prop"][0, 2]) and np.array_equal(rois[0, 1], c["prop"][0, 5])
    assert rois[0, 0, 0] < 0 and rois[0, 0, 1] < 0 and rois[0, 1, 2] > 1 and rois[0, 1, 3] > 1
    assert (masks[0, 0, :2, :] == 0).all() and (masks[0, 0, :, :2] == 0).all() and masks[0, 0, 4:20, 4:20].all()
    assert (masks[0, 1, -2:, :] == 0).all() and (masks[0, 1, :, -2:] == 0).all() and masks[0, 1, 4:20, 4:20].all()


def test_pixel_centre_samples():
    c = DC.target_case("pixel_centres")
    a, lo, hi = c["sample_lo_hi"]
    co = O._crop_coords(np.array([lo], F32), np.array([hi], F32), 96, 28)[0]
    assert np.array_equal(co, np.arange(a, a + 28).astype(F32)) and co[-1] == 95
    _, _, masks, npos = DC.target_reference("pixel_centres")
    assert npos[0] == 1 and np.array_equal(masks[0, 0], c["gt_masks"][0, a:, a:, 0].astype(F32)), "the crop IS the mask's pixels"
    assert masks[0, 0, -1].any() and masks[0, 0, :, -1].any()


def test_bilinear_half_count():
    c = DC.target_case("bilinear_half")
    a, lo, hi = c["sample_lo_hi"]
    co = O._crop_coords(np.array([lo], F32), np.array([hi], F32), 96, 28)[0]
    assert np.array_equal(co, (a + 0.5 * np.arange(28)).astype(F32))
    v = _crop_one(c["gt_masks"][0, :, :, 0], c["prop"][0, 6], ())
    # sample rows a .. a + 7 (15 of them) lie in the columns of alternating 1 / 0: every sample between two columns (14 of 28) is 0.5; the 12
    # rows a + 8 .. a + 13.5 lie in the block that ends between columns a + 4 and a + 5: one 0.5 each; row a + 7.5 averages a striped row and
    # a block row: 0.5 on the 2 + 4 whole columns where the two differ and between columns a + 4 and a + 5
    n_half = int((v == F32(0.5)).sum())
    print("bilinear values of exactly 0.5: %d" % n_half)
    assert n_half == 15 * 14 + 12 + 7
    _, _, masks, npos = DC.target_reference("bilinear_half")
    assert npos[0] == 1 and (masks[0, 0][v == F32(0.5)] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------------
# decode and detections
# ------------------------------------------------------------------------------------------------------------------------------------------
DECODE_NAMES = tuple(s[0] for s in DC.DECODE_SHAPES)
TINY = np.finfo(np.float32).tiny


def test_decode_shapes():
    shapes = {(s[2], s[3], s[4]) for s in DC.DECODE_SHAPES}
    assert {(1, 1, 1), (1, 3, 2), (13, 5, 81)} <= shapes
    assert any((s[1] * s[2] * s[2] * s[3]) % 256 != 0 and s[1] * s[2] * s[2] * s[3] > 256 for s in DC.DECODE_SHAPES)
    assert all(s[1] <= 4 for s in DC.DECODE_SHAPES)
    want = {0.0, 1e-30, 85.9, 86.0, 88.0, 88.1, 100.0, 3e38, np.inf}
    assert {float(F32(v)) for v in want} | {-float(F32(v)) for v in want} == set(DC.SPECIAL_LOGITS.tolist())
    assert np.signbit(DC.SPECIAL_LOGITS[1]) and DC.SPECIAL_LOGITS[1] == 0


@pytest.mark.parametrize("name", DECODE_NAMES)
def test_decode_case_is_on_its_edges(name):
    c = DC.decode_case(name)
    yp = c["y_pred"].reshape(-1, 5 + c["C"])
    assert not np.isnan(yp).any()
    prop, det = DC.decode_reference(name)
    assert not np.isnan(prop).any() and not np.isnan(det).any()
    if yp.shape[0] >= 54:
        for j in range(5):
            assert set(DC.SPECIAL_LOGITS.tolist()) <= set(yp[:, j].tolist()) and np.signbit(yp[yp[:, j] == 0, j]).any()
    # the clamp: logits beyond [-86, 88] give the clamp's value; a confidence logit of -88 and below gives a SUBNORMAL sigmoid
    conf = det.reshape(-1, 6)[:, 4]
    sub = (conf > 0) & (conf < TINY)
    assert sub.sum() > 0 and np.array_equal(sub, yp[:, 4] <= -88), "sigmoid(-88) = 1 / (1 + e^88) is about 6e-39"
    assert O.det_sigmoid(F32(-88.0)) == O.det_sigmoid(F32(-np.inf)) and 5e-39 < float(O.det_sigmoid(F32(-88.0))) < 7e-39
    assert O.det_expf(F32(-86.0)) == O.det_expf(F32(-100.0)) and O.det_expf(F32(-85.9)) > O.det_expf(F32(-86.0))
    # wrong rules: subnormal results flushed to zero; the upper clamp at 86 instead of 88
    flushed = np.where(np.abs(det) < TINY, F32(0), det)
    assert not np.array_equal(flushed, det), "a flushed subnormal sigmoid goes unnoticed"
    low = O.yolo_detections(np.minimum(np.maximum(c["y_pred"], F32(-86)), F32(86)), c["anchors"], c["G"])
    assert not np.array_equal(low, det), "a clamp at 86 goes unnoticed"
    # class column
    cl = yp[:, 5:]
    assert np.array_equal(det.reshape(-1, 6)[:, 5], np.argmax(cl, 1).astype(F32))
    if c["C"] > 1:
        mx = cl.max(1, keepdims=True)
        ties = (cl == mx).sum(1)
        assert (ties == c["C"]).any() and (ties == 2).any(), "all equal, and a tie of two"
        assert ((np.argmax(cl, 1) == c["C"] - 1) & (ties == 1)).any(), "the maximum in the last slot"
        zeros = (cl == 0).all(1)
        assert (zeros & np.signbit(cl[:, 0]) & ~np.signbit(cl[:, -1])).any(), "-0 against +0"
        last_wins = c["C"] - 1 - np.argmax(cl[:, ::-1], 1)                                # `>=`: the last maximum
        by_bits = np.argmax(np.ascontiguousarray(cl[zeros]).view(np.int32), 1)            # compared as integers, -0 lies below +0
        assert (last_wins != np.argmax(cl, 1)).any() and (by_bits == c["C"] - 1).all()
    print("%-12s total %5d: %d subnormal confidences, %d clamped logits" % (name, yp.shape[0], sub.sum(), (np.abs(yp[:, :5]) > 88).sum()))


# ------------------------------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------------------------------
LOSS_NAMES = tuple(s[0] for s in DC.LOSS_SHAPES)


def restate_counts(c, warm, thr=0.6, slots=None, own_box_only=False, no_object_term=True, first=None):
    """n_coord and n_conf (terms 6 and 7) from the oracle's pieces -> (n_coord, n_conf, best IoU per predictor)"""
    cfg, yt, yp = c["cfg"], c["y_true"], c["y_pred"]
    tb = c["true_boxes"][..., :slots, :] if slots else c["true_boxes"]
    anc = np.asarray(cfg.ANCHORS, F32).reshape(1, 1, 1, c["A"], 2)
    pxy = (O.det_sigmoid(yp[..., 0:2]) + O.cell_grid(c["G"])).astype(F32)
    pwh = (O.det_expf(yp[..., 2:4]) * anc).astype(F32)
    t4 = yt[..., 4]
    if own_box_only:
        best = O._iou_centre(pxy, pwh, yt[..., 0:2], yt[..., 2:4])[0]
    else:
        best = O._iou_centre(pxy[..., None, :], pwh[..., None, :], tb[..., 0:2], tb[..., 2:4])[0].max(-1)
    conf_mask = (best < F32(thr)).astype(F32) * (F32(1) - t4) * F32(cfg.NO_OBJECT_SCALE) * F32(no_object_term) + t4 * F32(cfg.OBJECT_SCALE)
    coord = np.ones_like(t4) if warm else t4 * F32(cfg.COORD_SCALE)
    if first:
        conf_mask, coord = conf_mask.reshape(-1)[:first], coord.reshape(-1)[:first]
    return float((coord > 0).sum()), float((conf_mask > 0).sum()), best


def test_loss_shapes():
    tot = {s[0]: s[1] * s[2] * s[2] * s[3] for s in DC.LOSS_SHAPES}
    assert tot["one_predictor"] == 1 and tot["b257"] == 257 and 2000 < tot["full_t64_c81"] < 5000
    assert {s[5] for s in DC.LOSS_SHAPES} == {1, 64} and {s[4] for s in DC.LOSS_SHAPES} == {2, 81}
    assert all(s[1] <= 4 for s in DC.LOSS_SHAPES if s[0] != "b257")
    for name in LOSS_NAMES:
        c = DC.loss_case(name)
        assert np.abs(c["y_pred"][..., 2:4]).max() <= DC.WH_LIMIT
        assert len(set(np.asarray(c["cfg"].CLASS_WEIGHTS).tolist())) > 1 and len(c["cfg"].CLASS_WEIGHTS) == c["C"]


@pytest.mark.parametrize("name", LOSS_NAMES)
@pytest.mark.parametrize("warm", [0, 1])
def test_loss_case_is_on_its_edges(name, warm):
    c, ref = DC.loss_case(name), DC.loss_reference(name, warm)
    total = c["B"] * c["G"] * c["G"] * c["A"]
    assert all(np.isfinite(float(v)) for k, v in ref.items() if k != "grad") and np.isfinite(ref["grad"]).all()
    n_coord, n_conf, best = restate_counts(c, warm)
    assert (n_coord, n_conf) == (float(ref["n_coord"]), float(ref["n_conf"])), "the restatement is the oracle"
    assert n_coord == (total if warm else c["n_objects"])
    other = DC.loss_reference(name, 1 - warm)
    assert float(other["loss_wh"]) != float(ref["loss_wh"]), "the warm-up flag goes unnoticed"
    if name == "no_object":
        assert c["n_objects"] == 0 and n_conf == total and float(ref["loss_class"]) == 0
        assert restate_counts(c, warm, no_object_term=False)[1] == 0
        assert (ref["grad"][..., 5:] == 0).all() and (warm or (ref["grad"][..., :4] == 0).all())
        return
    t4 = c["y_true"][..., 4]
    uniform = type(c["cfg"])()
    uniform.CLASS_WEIGHTS = np.ones(c["C"], F32)
    flat = O.yolo_loss(c["y_true"], c["y_pred"], c["true_boxes"], uniform, warmup=bool(warm))
    assert float(flat["loss_class"]) != float(ref["loss_class"]), "uniform class weights go unnoticed"
    if name == "b257":
        assert restate_counts(c, warm, first=256)[1] == n_conf - 1, "the 257th predictor is counted"
    if name in ("full_t64_c81", "two_in_a_cell"):
        # predictors without an object of their own that a true-box slot takes out of the no-object mask
        out = (t4 == 0) & (best >= F32(0.6))
        assert out.sum() >= c["n_objects"] // (1 if name == "full_t64_c81" else 2) and n_conf == total - out.sum()
        assert restate_counts(c, warm, own_box_only=True)[1] == total, "the true-box buffer goes unnoticed"
        print("%-14s warm %d: %d predictors leave the no-object mask" % (name, warm, out.sum()))
    if name == "full_t64_c81":
        near = ((best >= 0.5) & (best < 0.7) & (t4 == 0)).sum()
        assert restate_counts(c, warm, thr=0.5)[1] < n_conf < restate_counts(c, warm, thr=0.7)[1], "no best IoU on either side of 0.6"
        print("%d best IoUs in [0.5, 0.7)" % near)
        assert (c["true_boxes"][:, 0, 0, 0, :, 2] > 0).all(), "every true-box slot is used"
        assert restate_counts(c, warm, slots=63)[1] == n_conf + c["B"], "the last slot (T = 64) goes unnoticed"
    if name == "two_in_a_cell":
        cells = np.argwhere(t4 == 1)
        for b in range(c["B"]):
            mine = cells[cells[:, 0] == b]
            assert len(mine) == 2 and (mine[0, 1:3] == mine[1, 1:3]).all() and mine[0, 3] != mine[1, 3]

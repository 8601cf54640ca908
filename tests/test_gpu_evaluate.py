"""MaskYOLO.evaluate on the GPU: myolo_mask_overlap_counts against the existing paste (myolo_unmold_masks) bit for bit,
evaluate() against an Evaluator fed from detect_many's result dicts, the device-produced stream against the host loader, and a
ground-truth-as-prediction sanity case."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X                                            # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.evaluate import Evaluator                                   # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402
from myolo.shapes import make_shapes_samples                           # noqa: E402

DEV = "cuda"
MH = MW = 28
R = 12                      # detection rows per image in the kernel cases: 8 special ones (below) + 4 random


# ------------------------------------------------------------------------------------------------ kernel against the existing paste
def _case(B, K, T, C, H, W, seed):
    """-> masks [B,R,28,28,C], det [B,R,6], sel [B,K] (-1 = empty), gt [B,H,W,T].  Rows 0-7 of every image are the boxes a paste can get
    wrong: 0 the full image, 1 a one-pixel window, 2 partly outside [0,1], 3 wholly outside (above 1), 4 wholly outside (below 0: the clamps
    leave a one-pixel column), 5 zero width (x1 == x2: no pixel is in the window), 6 an all-high mask (the clip=True path), 7 a mask that is all
    below 0.5; rows 8-11 random boxes with random masks."""
    rng = np.random.default_rng(seed)
    masks = rng.random((B, R, MH, MW, C), dtype=np.float32)
    det = np.zeros((B, R, 6), np.float32)
    for b in range(B):
        lo = rng.random((R, 2)) * 0.7
        det[b, :, 0:2] = lo
        det[b, :, 2:4] = lo + 0.05 + rng.random((R, 2)) * 0.5
        det[b, :, 4] = rng.random(R)
        det[b, :, 5] = rng.integers(0, C, R)
        det[b, 0, :4] = (0.0, 0.0, 1.0, 1.0)
        det[b, 1, :4] = (0.5, 0.5, 0.5 + 1.2 / W, 0.5 + 1.2 / H)
        det[b, 2, :4] = (-0.2, 0.4, 0.6, 1.3)
        det[b, 3, :4] = (1.2, 1.1, 1.5, 1.6)
        det[b, 4, :4] = (-0.5, -0.6, -0.2, -0.1)
        det[b, 5, :4] = (0.3, 0.2, 0.3, 0.8)
        for r, (a, z) in ((6, (0.5, 1.0)), (7, (0.0, 0.499))):
            masks[b, r, :, :, int(det[b, r, 5])] = (a + (z - a) * rng.random((MH, MW))).astype(np.float32)
    sel = np.full((B, K), -1, np.int32)
    for b in range(B):
        if B == 3 and b == 1:
            continue                                               # an image whose slots are all empty
        if K == 1:
            sel[b, 0] = (3 * b + T + C) % R
        else:
            rows = rng.permutation(R)[:K]
            rows[rng.integers(0, K, 2)] = -1                        # some slots empty, in the middle as well
            if b == 0:
                rows[:8] = np.arange(8)                             # every special row is selected at least once
                rows[8:] = (-1, 9)
            sel[b] = rows
    gt = (rng.random((B, H, W, T)) < 0.4).astype(np.uint8)
    for b in range(B):
        if T >= 3:
            gt[b, :, :, 0], gt[b, :, :, 1] = 1, 0                   # planes that are all ones / all zeros beside the random ones
        else:
            k = (b + C) % 3
            if k < 2:
                gt[b, :, :, 0] = 1 - k
    return masks, det, sel, gt


def _window(d, H, W):
    """unmold_kernel's window (csrc/exact_kernels.hip, unmold_window) restated in numpy float32"""
    f = np.float32
    x1 = min(max(0, int(f(d[0]) * f(W))), W)
    x2 = min(max(1, int(f(d[2]) * f(W))), W)
    y1 = min(max(0, int(f(d[1]) * f(H))), H)
    y2 = min(max(1, int(f(d[3]) * f(H))), H)
    return [x1, y1, x2, y2]


def _paste(masks_d, det_d, rows, H, W):
    """myolo_unmold_masks on the chosen rows of one image -> [H,W,n] bool"""
    idx = torch.as_tensor(np.asarray(rows, np.int64), device=DEV)
    m, d = masks_d.index_select(0, idx).contiguous(), det_d.index_select(0, idx).contiguous()
    n = len(rows)
    full = torch.empty(H, W, n, dtype=torch.uint8, device=DEV)
    ws = torch.empty(n, dtype=torch.int32, device=DEV)
    X.call("myolo_unmold_masks", X.ptr(m), X.ptr(d), X.ptr(full), n, MH, MW, int(m.shape[3]), H, W, ws.data_ptr(), ws.numel() * 4, X.stream())
    return full.cpu().numpy().astype(bool)


def _reference(masks, det, sel, gt, H, W):
    B, K = sel.shape
    T = gt.shape[3]
    inter, ap, ag, win = np.zeros((B, K, T), np.int32), np.zeros((B, K), np.int32), np.zeros((B, T), np.int32), np.zeros((B, K, 4), np.int32)
    for b in range(B):
        g = gt[b].astype(bool)
        ag[b] = g.reshape(-1, T).sum(0)
        slots = [k for k in range(K) if sel[b, k] >= 0]
        if not slots:
            continue
        full = _paste(torch.as_tensor(masks[b], device=DEV), torch.as_tensor(det[b], device=DEV), [sel[b, k] for k in slots], H, W)
        for i, k in enumerate(slots):
            ap[b, k] = full[:, :, i].sum()
            inter[b, k] = (full[:, :, i, None] & g).reshape(-1, T).sum(0)
            win[b, k] = _window(det[b, sel[b, k]], H, W)
    return inter, ap, ag, win


def _counts(masks, det, sel, gt):
    """the entry itself, through ctypes (no engine): -> four int32 numpy arrays"""
    B, K = sel.shape
    H, W, T = gt.shape[1:]
    C = masks.shape[4]
    md, dd, sd, gd = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (masks, det, sel, gt))
    out = [torch.full(s, -7, dtype=torch.int32, device=DEV) for s in ((B, K, T), (B, K), (B, T), (B, K, 4))]
    ws = torch.empty(B * K, dtype=torch.int32, device=DEV)
    sel_h = np.ascontiguousarray(sel)
    X.call("myolo_mask_overlap_counts", X.ptr(md), X.ptr(dd), X.ptr(sd), sel_h.ctypes.data, X.ptr(gd), *[X.ptr(o) for o in out],
           B, R, K, T, MH, MW, C, H, W, ws.data_ptr(), ws.numel() * 4, X.stream())
    return [o.cpu().numpy() for o in out]


def _check(B, K, T, C, H, W, seed):
    masks, det, sel, gt = _case(B, K, T, C, H, W, seed)
    want = _reference(masks, det, sel, gt, H, W)
    got = _counts(masks, det, sel, gt)
    for name, g, w in zip(("inter", "area_pred", "area_gt", "win"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])
    return sel, got


@pytest.mark.parametrize("C", [1, 4, 81])
@pytest.mark.parametrize("T", [1, 10])
@pytest.mark.parametrize("K", [1, 10])
@pytest.mark.parametrize("B", [1, 3])
def test_overlap_counts_equal_the_paste_70x70(B, K, T, C):
    """H = W = 70: neither H * W (4900 = 76 * 64 + 36: a partial last wave) nor W is a multiple of 64, and an image takes five workgroups"""
    sel, (inter, ap, ag, win) = _check(B, K, T, C, 70, 70, seed=1000 + 100 * B + 10 * K + T + C)
    empty = sel < 0
    assert not inter[empty].any() and not ap[empty].any() and not win[empty].any()           # empty slots give zeros
    if K == 10:
        # the case does hold what it is meant to: the full window, a one-pixel window, the all-high mask pasted over its whole window
        assert win[0, 0].tolist() == [0, 0, 70, 70] and (win[0, 1, 2:] - win[0, 1, :2]).tolist() == [1, 1]
        assert (win[0, 5, 2] - win[0, 5, 0]) == 0 and ap[0, 5] == 0 and ap[0, 3] == 0
        w6 = win[0, 6]
        assert ap[0, 6] == (w6[2] - w6[0]) * (w6[3] - w6[1]) > 0 and ap[0, 7] == 0


def test_overlap_counts_equal_the_paste_224x224():
    """224 x 224, B = 4, K = T = 10: 49 workgroups per image, so the strip partition and the sum over workgroups carry the result"""
    _check(4, 10, 10, 4, 224, 224, seed=5)


def test_overlap_counts_two_runs_bit_identical():
    masks, det, sel, gt = _case(3, 10, 10, 4, 70, 70, seed=11)
    a, b = _counts(masks, det, sel, gt), _counts(masks, det, sel, gt)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_overlap_counts_refuses_bad_arguments():
    lib = X.load()
    B, K, T, C, H, W = 1, 10, 10, 4, 70, 70
    masks, det, sel, gt = _case(B, K, T, C, H, W, seed=3)
    md, dd, sd, gd = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (masks, det, sel, gt))
    out = [torch.zeros(s, dtype=torch.int32, device=DEV) for s in ((B, 16, 32), (B, 16), (B, 32), (B, 16, 4))]
    ws = torch.empty(64, dtype=torch.int32, device=DEV)
    sel_big = np.full((B, 17), -1, np.int32)

    def call(masks_p=None, sel_h=sel, K=K, T=T, ws_bytes=ws.numel() * 4, ws_p=None):
        return lib.myolo_mask_overlap_counts(X.ptr(md) if masks_p is None else masks_p, X.ptr(dd), X.ptr(sd), sel_h.ctypes.data, X.ptr(gd),
                                             *[X.ptr(o) for o in out], B, R, K, T, MH, MW, C, H, W, ws.data_ptr() if ws_p is None else ws_p,
                                             ws_bytes, X.stream())
    assert call() == 0
    bad = sel.copy()
    bad[0, 3] = R
    for kw in (dict(masks_p=ctypes.c_void_p(None)), dict(K=17, sel_h=sel_big), dict(T=33), dict(sel_h=bad), dict(ws_bytes=B * K * 4 - 1),
               dict(ws_p=ctypes.c_void_p(None))):
        assert call(**kw) == -1, kw
        assert b"mask_overlap_counts" in lib.myolo_last_error_string(), kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the models this file shares (and the ones its tests left as cyclic garbage: a Net refers to itself) are destroyed HERE, with the device
    idle -- not by a collection that happens to start inside a later test"""
    yield
    import gc
    _MODELS.clear()
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _model(dtype):
    if dtype not in _MODELS:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4, INFERENCE_DTYPE=dtype)
        _MODELS[dtype] = (cfg, MaskYOLO(mode="inference", config=cfg, seed=4))
    return _MODELS[dtype]


def _from_result_dicts(cfg, samples, results):
    """the same metric from detect()'s result dicts: overlaps counted in numpy from full_masks, windows from bboxes"""
    H, W = cfg.IMAGE_SHAPE[:2]
    T = cfg.MAX_GT_INSTANCES
    ev = Evaluator()
    for (_, class_ids, boxes, gmasks), d in zip(samples, results):
        m = min(T, len(class_ids))
        gt_ids, gt_boxes = np.zeros(T, np.int32), np.zeros((T, 4), np.int32)
        gt_ids[:m], gt_boxes[:m] = class_ids[:m], boxes[:m]
        g = np.zeros((H, W, T), bool)
        g[:, :, :m] = gmasks[:, :, :m]
        full = d["full_masks"].astype(bool)
        n = full.shape[2]
        inter = np.array([[int((full[:, :, k] & g[:, :, t]).sum()) for t in range(T)] for k in range(n)], np.int64).reshape(n, T)
        win = np.array([[min(max(0, int(bb[0])), W), min(max(0, int(bb[1])), H), min(max(1, int(bb[2])), W), min(max(1, int(bb[3])), H)]
                        for bb in d["bboxes"]], np.int64).reshape(n, 4)
        ev.add_image(d["confidence_scores"], d["class_ids"], gt_ids, inter, full.sum(axis=(0, 1)), g.sum(axis=(0, 1)), win, gt_boxes)
    return ev.result()


def _same(a, b):
    assert set(a) == set(b)
    for k in ("n_images", "n_gt", "n_det"):
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ("mask_ap50", "mask_ap", "box_ap50", "box_ap", "mean_matched_mask_iou"):
        assert abs(a[k] - b[k]) <= 1e-12, (k, a[k], b[k])
    assert sorted(a["per_class"]) == sorted(b["per_class"])
    for c, pa in a["per_class"].items():
        pb = b["per_class"][c]
        assert pa["n_gt"] == pb["n_gt"] and pa["n_det"] == pb["n_det"], (c, pa, pb)
        assert abs(pa["mask_ap50"] - pb["mask_ap50"]) <= 1e-12 and abs(pa["box_ap50"] - pb["box_ap50"]) <= 1e-12, (c, pa, pb)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_evaluate_equals_evaluator_fed_from_detect_results(dtype):
    """evaluate() on eight Shapes images at 128 x 128, batch 4, seeded random weights and cs_threshold 0 (so that detections exist), against an
    Evaluator fed from the result dicts of detect_many -- detect()'s dicts at the batch shape evaluate() runs (detect() itself forwards one image
    per launch, whose fp32 sums may differ in the last bits: tests/test_gpu_step.py::test_detect_many_equals_detect_per_image)."""
    cfg, m = _model(dtype)
    samples = make_shapes_samples(8, cfg, seed=77)
    got = m.evaluate(samples, cs_threshold=0.0)
    want = _from_result_dicts(cfg, samples, m.detect_many([s[0] for s in samples], cs_threshold=0.0))
    assert got["n_images"] == 8 and got["n_gt"] >= 8 and got["n_det"] >= 8
    _same(got, want)
    # a short last batch is padded and its padding ignored; max_samples cuts the set
    got6 = m.evaluate(samples, cs_threshold=0.0, max_samples=6)
    _same(got6, _from_result_dicts(cfg, samples[:6], m.detect_many([s[0] for s in samples[:6]], cs_threshold=0.0)))


def test_evaluate_resnet50_81_classes():
    nc = 81
    cfg = make_config(ShapesConfig, BACKBONE="resnet50", IMAGE_SHAPE=[128, 128, 3], BATCH_SIZE=2, NUM_CLASSES=nc,
                      LABELS=["background"] + ["class%d" % i for i in range(1, nc)])
    m = MaskYOLO(mode="inference", config=cfg, seed=4)
    samples = make_shapes_samples(2, cfg, seed=78)
    got = m.evaluate(samples, cs_threshold=0.0)
    assert got["n_images"] == 2 and got["n_det"] >= 1
    _same(got, _from_result_dicts(cfg, samples, m.detect_many([s[0] for s in samples], cs_threshold=0.0)))


def test_evaluate_shapes_stream_equals_evaluate_on_the_host_loader():
    cfg, m = _model("bf16")
    got = m.evaluate_shapes_stream(8, seed=77, cs_threshold=0.0)
    want = m.evaluate(make_shapes_samples(8, cfg, seed=77), cs_threshold=0.0)
    _same(got, want)
    # a window of the stream that is no multiple of the batch, from an offset
    _same(m.evaluate_shapes_stream(5, seed=77, start_index=2, cs_threshold=0.0),
          m.evaluate(make_shapes_samples(5, cfg, seed=77, start_index=2), cs_threshold=0.0))


def test_evaluate_needs_inference_mode():
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4)
    with pytest.raises(AssertionError):
        MaskYOLO(mode="training", config=cfg).evaluate([])


# ------------------------------------------------------------------------------------------------ sanity: the ground truth as prediction
def test_ground_truth_as_prediction_scores_one():
    """det and masks overwritten with each image's own ground truth: its boxes as rows of score 1, and in the one-hot class plane the mask
    downsampled to 28 x 28 from the ground truth inside its box.  The ground truth is built so that the paste gives it back EXACTLY -- shapes
    drawn on a 28 x 28 grid and enlarged by whole pixels, 1 x or 2 x (at 1 x the resize reads mask pixels; at 2 x the bilinear weights are
    (3/4, 1/4) per axis, the nearest mask pixel alone weighs 9/16 >= 1/2 and the other three together 7/16 < 1/2, so the threshold returns
    the nearest pixel), boxes on whole pixels of a 128 x 128 image (a power of two: the normalised corners are exact) -- so every IoU is 1
    and mask_ap = box_ap = 1.0 exactly, at all ten thresholds.  Net.overlap_counts and the Evaluator, no weights."""
    cfg, m = _model("fp32")
    H = W = 128
    T, C = cfg.MAX_GT_INSTANCES, cfg.NUM_CLASSES
    yy, xx = np.mgrid[0:28, 0:28]
    shapes = {1: np.ones((28, 28), bool),                                                     # square
              2: (2 * xx - 27) ** 2 + (2 * yy - 27) ** 2 <= 28 ** 2,                          # disc touching all four sides
              3: np.abs(2 * xx - 27) <= yy + 1}                                               # triangle, apex up
    for s in shapes.values():
        assert s.any(0).all() and s.any(1).all()                                              # tight in its 28 x 28 grid
    rng = np.random.default_rng(12)
    B = 3
    gt = np.zeros((B, H, W, T), np.uint8)
    gt_ids, gt_boxes = np.zeros((B, T), np.int32), np.zeros((B, T, 4), np.int32)
    det = np.zeros((B, T, 6), np.float32)
    masks = np.zeros((B, T, 28, 28, C), np.float32)
    sel = np.full((B, 10), -1, np.int32)
    for b, n in enumerate((4, 1, 0)):                                                         # an image without ground truth too
        for j in range(n):
            cls, f = int(rng.integers(1, 4)), int(rng.integers(1, 3))
            x1, y1 = int(rng.integers(0, W - 28 * f + 1)), int(rng.integers(0, H - 28 * f + 1))
            big = np.kron(shapes[cls], np.ones((f, f), bool))
            gt[b, y1:y1 + 28 * f, x1:x1 + 28 * f, j] = big
            gt_ids[b, j], gt_boxes[b, j] = cls, (x1, y1, x1 + 28 * f, y1 + 28 * f)
            det[b, j] = (x1 / W, y1 / H, (x1 + 28 * f) / W, (y1 + 28 * f) / H, 1.0, cls)
            masks[b, j, :, :, cls] = big.reshape(28, f, 28, f).mean(axis=(1, 3))              # the block average: 0 / 1 here
            sel[b, j] = j
    counts = m.net.overlap_counts(torch.as_tensor(det, device=DEV), torch.as_tensor(masks, device=DEV), sel, torch.as_tensor(gt, device=DEV))
    inter, ap, ag, win = [t.cpu().numpy() for t in counts]
    ev = Evaluator()
    for b in range(B):
        n = int((sel[b] >= 0).sum())
        ev.add_image(det[b, :n, 4], det[b, :n, 5], gt_ids[b], inter[b, :n], ap[b, :n], ag[b], win[b, :n], gt_boxes[b])
    r = ev.result()
    assert r["n_gt"] == 5 and r["n_det"] == 5 and r["n_images"] == 3
    assert r["mask_ap"] == 1.0 and r["box_ap"] == 1.0 and r["mask_ap50"] == 1.0 and r["box_ap50"] == 1.0
    assert r["mean_matched_mask_iou"] == 1.0

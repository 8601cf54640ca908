"""max_detections through the public path: detect / detect_many / evaluate with the selection made on the device.  At
max_detections=10 every result equals the host selection's, key for key and array for array; at 40 an image reports more than sixteen instances
through the dense, run-length and polygon forms and through evaluate(); Net.rle_masks / contour_masks / overlap_counts take K = 40 in column blocks
of 16 and give what their host references give."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X                                            # noqa: E402
from myolo import contour, rle                                         # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.evaluate import Evaluator                                   # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402
from myolo.shapes import make_shapes_samples                           # noqa: E402

DEV = "cuda"
MH = MW = 28
SEED = 4                    # of the random weights: with it image 0 below reports more than sixteen instances at max_detections=40 (asserted)
_STATE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the model this file shares is destroyed HERE, with the device idle -- not by a collection that happens to start inside a later test"""
    yield
    import gc
    _STATE.clear()
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _model():
    if "model" not in _STATE:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], ALPHA=0.5, BATCH_SIZE=2)
        _STATE["model"] = (cfg, MaskYOLO(mode="inference", config=cfg, seed=SEED))
    return _STATE["model"]


def _picture(h, w, seed):
    """a Shapes-like picture of any size: a flat background with a few filled rectangles and discs"""
    rng = np.random.default_rng(seed)
    img = np.empty((h, w, 3), np.uint8)
    img[:] = rng.integers(0, 256, 3)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(3):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), max(2, int(min(h, w) * rng.uniform(0.15, 0.35)))
        inside = (np.abs(yy - cy) <= r) & (np.abs(xx - cx) <= r) if rng.random() < 0.5 else (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        img[inside] = rng.integers(0, 256, 3)
    return img


SIZES = ((224, 224), (224, 224), (200, 150), (224, 224), (61, 97), (224, 224))      # batch 2: whole batches at the frame and mixed ones


def _images():
    return [_picture(h, w, 30 + k) for k, (h, w) in enumerate(SIZES)]


def _results(**kw):
    """detect_many over the six images at cs_threshold 0, computed once per set of arguments and left unchanged"""
    key = tuple(sorted(kw.items()))
    if key not in _STATE:
        _STATE[key] = _model()[1].detect_many(_images(), cs_threshold=0.0, **kw)
    return _STATE[key]


def _equal(a, b, what):
    """two result dicts, key for key and array for array"""
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for key in a:
        if key == "rle_masks":
            assert [m["size"] for m in a[key]] == [m["size"] for m in b[key]], (what, key)
            assert all(x["counts"].dtype == y["counts"].dtype and np.array_equal(x["counts"], y["counts"]) for x, y in zip(a[key], b[key])), (what, key)
            assert len(a[key]) == len(b[key]), (what, key)
        elif key == "polygons":
            assert len(a[key]) == len(b[key]) and [len(l) for l in a[key]] == [len(l) for l in b[key]], (what, key)
            for la, lb in zip(a[key], b[key]):
                assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(la, lb)), (what, key)
        else:
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (what, key)


# ------------------------------------------------------------------------------------------------ ten on the device = ten on the host
@pytest.mark.parametrize("render", [False, True])
@pytest.mark.parametrize("fmt", ["dense", "rle", "polygon"])
def test_ten_on_the_device_equals_the_host_selection(fmt, render):
    cfg, m = _model()
    imgs = _images()
    host = _results(mask_format=fmt, render=render)
    dev = _results(mask_format=fmt, render=render, max_detections=10)
    assert len(host) == len(dev) == len(imgs) and sum(len(r["class_ids"]) for r in host) >= len(imgs)
    for k, (a, b) in enumerate(zip(dev, host)):
        assert ("rendered" in a) == render
        _equal(a, b, "image %d" % k)
    # detect() itself: one image per launch, at the frame and resized
    for k in (0, 2, 4):
        a = m.detect(imgs[k], cs_threshold=0.0, mask_format=fmt, render=render, save_path=None, max_detections=10)
        b = m.detect(imgs[k], cs_threshold=0.0, mask_format=fmt, render=render, save_path=None)
        assert len(a) == len(b) == 1
        _equal(a[0], b[0], "detect %d" % k)
    # ... and in the network's frame
    if fmt == "rle" and not render:
        for a, b in zip(m.detect_many(imgs, cs_threshold=0.0, mask_format=fmt, mask_frame="network", max_detections=10),
                        m.detect_many(imgs, cs_threshold=0.0, mask_format=fmt, mask_frame="network")):
            _equal(a, b, "network frame")


# ------------------------------------------------------------------------------------------------ forty
def test_forty_reports_more_than_sixteen_instances():
    cfg, m = _model()
    imgs = _images()
    dense = _results(max_detections=40)
    coded = _results(mask_format="rle", max_detections=40)
    poly = _results(mask_format="polygon", max_detections=40)
    counts = [len(r["class_ids"]) for r in dense]
    print("instances per image at max_detections=40:", counts, "at the host's ten:", [len(r["class_ids"]) for r in _results()])
    assert max(counts) > 16 and max(counts) <= 40, counts
    for k, (d, c, p) in enumerate(zip(dense, coded, poly)):
        n = len(d["class_ids"])
        h, w = imgs[k].shape[:2]
        assert d["full_masks"].shape == (h, w, n) and d["bboxes"].shape == (n, 4) and d["confidence_scores"].shape == (n,)
        assert (np.diff(d["confidence_scores"]) <= 0).all(), k
        for key in ("bboxes", "class_ids", "confidence_scores"):
            assert np.array_equal(d[key], c[key]) and np.array_equal(d[key], p[key]) and d[key].dtype == c[key].dtype == p[key].dtype, (k, key)
        assert len(c["rle_masks"]) == len(p["polygons"]) == n
        for i in range(n):
            plane = d["full_masks"][:, :, i].astype(bool)
            assert c["rle_masks"][i]["size"] == [h, w] and np.array_equal(rle.decode(c["rle_masks"][i]), plane), (k, i)
            assert c["rle_masks"][i]["counts"].tolist() == rle.encode(plane)["counts"].tolist(), (k, i)
            want = contour.trace(plane)
            assert len(p["polygons"][i]) == len(want) and all(np.array_equal(x, y) for x, y in zip(p["polygons"][i], want)), (k, i)
    # the first ten of forty are the host's ten wherever NMB met no candidate beyond the tenth ... and always its best one
    for d, t in zip(dense, _results()):
        if len(t["class_ids"]):
            assert d["confidence_scores"][0] == t["confidence_scores"][0]
    # detect() on the image with the most instances
    k = int(np.argmax(counts))
    one = m.detect(imgs[k], cs_threshold=0.0, mask_format="rle", max_detections=40)[0]
    own = m.detect(imgs[k], cs_threshold=0.0, max_detections=40)[0]
    assert len(one["class_ids"]) == len(own["class_ids"]) > 16 and np.array_equal(one["confidence_scores"], own["confidence_scores"])
    assert all(np.array_equal(rle.decode(x), own["full_masks"][:, :, i].astype(bool)) for i, x in enumerate(one["rle_masks"]))
    # sixteen is the most an overlay holds
    with pytest.raises(ValueError, match="one pass"):
        m.detect_many(imgs[:2], cs_threshold=0.0, render=True, max_detections=40)
    with pytest.raises(ValueError, match="one pass"):
        m.detect(imgs[0], cs_threshold=0.0, render=True, max_detections=17)
    got = m.detect_many(imgs[:2], cs_threshold=0.0, render=True, max_detections=16)
    assert all(r["rendered"].shape == im.shape for r, im in zip(got, imgs))


# ------------------------------------------------------------------------------------------------ the consumers in column blocks
R = 14
K40 = 40


def _block_case(frames, C, seed):
    """masks [2,R,28,28,C], det [2,R,6], sel [2,40]: columns 0-15 and 32-39 live with empty slots sprinkled in, columns 16-31 (the whole middle
    block) empty; the rows repeat (R = 14 < the live slots) and include windows partly and wholly outside the frame"""
    rng = np.random.default_rng(seed)
    masks = rng.random((2, R, MH, MW, C), dtype=np.float32)
    det = np.zeros((2, R, 6), np.float32)
    for b in range(2):
        lo = rng.random((R, 2)) * 0.7
        det[b, :, 0:2], det[b, :, 2:4] = lo, lo + 0.05 + rng.random((R, 2)) * 0.5
        det[b, :, 4], det[b, :, 5] = rng.random(R), rng.integers(0, C, R)
        det[b, 0, :4] = (0.0, 0.0, 1.0, 1.0)
        det[b, 1, :4] = (-0.2, 0.4, 0.6, 1.3)
        det[b, 2, :4] = (1.2, 1.1, 1.5, 1.6)
        det[b, 3, :4] = (0.3, 0.2, 0.3, 0.8)
        masks[b, 0, :, :, int(det[b, 0, 5])] = 0.5 + 0.5 * rng.random((MH, MW), dtype=np.float32)
    sel = np.full((2, K40), -1, np.int32)
    i = 0
    for b in range(2):
        for k in list(range(16)) + list(range(32, 40)):
            if k % 5 == 3 or (b == 1 and k == 0):
                continue
            sel[b, k] = i % R
            i += 1
    return masks, det, sel, np.asarray(frames, np.int32).reshape(2, 2)


def _paste(masks_b, det_b, rows, H, W):
    """myolo_unmold_masks on the chosen rows of one image -> [H,W,n] bool: the oracle"""
    idx = torch.as_tensor(np.asarray(rows, np.int64), device=DEV)
    m = torch.as_tensor(masks_b, device=DEV).index_select(0, idx).contiguous()
    d = torch.as_tensor(det_b, device=DEV).index_select(0, idx).contiguous()
    n = len(rows)
    full = torch.empty(H, W, n, dtype=torch.uint8, device=DEV)
    ws = torch.empty(n, dtype=torch.int32, device=DEV)
    X.call("myolo_unmold_masks", X.ptr(m), X.ptr(d), X.ptr(full), n, MH, MW, int(m.shape[3]), H, W, ws.data_ptr(), ws.numel() * 4, X.stream())
    return full.cpu().numpy().astype(bool)


def _planes(masks, det, sel, frames):
    """{(b, k): the pasted plane} of every live slot"""
    out = {}
    for b in range(sel.shape[0]):
        live = [k for k in range(sel.shape[1]) if sel[b, k] >= 0]
        dense = _paste(masks[b], det[b], [sel[b, k] for k in live], int(frames[b, 0]), int(frames[b, 1]))
        for i, k in enumerate(live):
            out[(b, k)] = dense[:, :, i]
    return out


def test_net_rle_and_contour_masks_at_forty_slots():
    cfg, m = _model()
    masks, det, sel, frames = _block_case([(37, 91), (70, 70)], 4, seed=40)
    md, dd = torch.as_tensor(masks, device=DEV), torch.as_tensor(det, device=DEV)
    planes = _planes(masks, det, sel, frames)
    assert len(planes) > 32 and (sel[:, 16:32] == -1).all()
    run_off, bounds = m.net.rle_masks(dd, md, sel, frames)
    loops = m.net.contour_masks(dd, md, sel, frames)
    assert run_off.dtype == np.int32 and run_off.shape == (2 * K40 + 1,) and bounds.dtype == np.uint32 and bounds.size == run_off[-1] and len(loops) == 2 * K40
    set_pixels = 0
    for b in range(2):
        H, W = int(frames[b, 0]), int(frames[b, 1])
        for k in range(K40):
            s = b * K40 + k
            mine = bounds[run_off[s]:run_off[s + 1]]
            if sel[b, k] < 0:
                assert mine.size == 0 and loops[s] == [], (b, k)
                continue
            plane = planes[(b, k)]
            set_pixels += int(plane.sum())
            assert rle.counts_from_boundaries(mine, H * W).tolist() == rle.encode(plane)["counts"].tolist(), (b, k)
            want = contour.trace(plane)
            assert len(loops[s]) == len(want) and all(x.dtype == np.int32 and np.array_equal(x, y) for x, y in zip(loops[s], want)), (b, k)
    assert set_pixels > 0
    # the first sixteen columns alone are today's single call, and give the same slots
    off16, b16 = m.net.rle_masks(dd, md, np.ascontiguousarray(sel[:, :16]), frames)
    for b in range(2):
        for k in range(16):
            assert np.array_equal(b16[off16[b * 16 + k]:off16[b * 16 + k + 1]], bounds[run_off[b * K40 + k]:run_off[b * K40 + k + 1]])
    # 129 slots are refused here; 17 are refused by the entry points, as before
    wide = np.full((2, 129), -1, np.int32)
    for fn in (m.net.rle_masks, m.net.contour_masks):
        with pytest.raises(ValueError, match="at most 128"):
            fn(dd, md, wide, frames)
    with pytest.raises(ValueError):
        m.net.rle_masks(dd, md, sel.astype(np.int64), frames)


def _window(d, H, W):
    """unmold_kernel's window (csrc/exact_kernels.hip, unmold_window) restated in numpy float32"""
    f = np.float32
    return [min(max(0, int(f(d[0]) * f(W))), W), min(max(0, int(f(d[1]) * f(H))), H), min(max(1, int(f(d[2]) * f(W))), W),
            min(max(1, int(f(d[3]) * f(H))), H)]


@pytest.mark.parametrize("T", [1, 32])
@pytest.mark.parametrize("frame", [(37, 91), (70, 70)], ids=["37x91", "70x70"])
def test_net_overlap_counts_at_forty_slots(frame, T):
    cfg, m = _model()
    H, W = frame
    masks, det, sel, frames = _block_case([frame, frame], 4, seed=41 + T)
    gt = (np.random.default_rng(T).random((2, H, W, T)) < 0.4).astype(np.uint8)
    md, dd, gd = (torch.as_tensor(a, device=DEV) for a in (masks, det, gt))
    inter, area_pred, area_gt, win = [t.cpu().numpy() for t in m.net.overlap_counts(dd, md, sel, gd)]
    assert inter.shape == (2, K40, T) and area_pred.shape == (2, K40) and area_gt.shape == (2, T) and win.shape == (2, K40, 4)
    assert all(a.dtype == np.int32 for a in (inter, area_pred, area_gt, win))
    planes = _planes(masks, det, sel, frames)
    for b in range(2):
        g = gt[b].astype(bool)
        assert np.array_equal(area_gt[b], g.reshape(-1, T).sum(0))
        for k in range(K40):
            if sel[b, k] < 0:
                assert not inter[b, k].any() and area_pred[b, k] == 0 and not win[b, k].any(), (b, k)
                continue
            plane = planes[(b, k)]
            assert area_pred[b, k] == plane.sum() and np.array_equal(inter[b, k], (plane[:, :, None] & g).reshape(-1, T).sum(0)), (b, k)
            assert win[b, k].tolist() == _window(det[b, sel[b, k]], H, W), (b, k)
    # a pinned host tensor, as detect.overlap_counts hands it over
    pin = torch.from_numpy(sel.copy()).pin_memory()
    again = [t.cpu().numpy() for t in m.net.overlap_counts(dd, md, pin, gd)]
    assert all(np.array_equal(a, b) for a, b in zip(again, (inter, area_pred, area_gt, win)))
    with pytest.raises(ValueError, match="at most 128"):
        m.net.overlap_counts(dd, md, np.full((2, 129), -1, np.int32), gd)


# ------------------------------------------------------------------------------------------------ evaluate
def _from_result_dicts(cfg, samples, results):
    """the metric from detect()'s result dicts: overlaps counted in numpy from full_masks, windows from bboxes"""
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


def test_evaluate_at_forty_equals_the_evaluator_fed_from_detect_many():
    cfg, m = _model()
    samples = make_shapes_samples(5, cfg, seed=77)                      # batch 2: a short last batch
    imgs = [s[0] for s in samples]
    dicts = m.detect_many(imgs, cs_threshold=0.0, max_detections=40)
    got = m.evaluate(samples, cs_threshold=0.0, max_detections=40)
    assert got["n_images"] == 5 and got["n_det"] == sum(len(d["class_ids"]) for d in dicts)
    assert max(len(d["class_ids"]) for d in dicts) > 16
    _same(got, _from_result_dicts(cfg, samples, dicts))
    ten = m.evaluate(samples, cs_threshold=0.0)
    assert got["n_det"] > ten["n_det"]
    _same(m.evaluate(samples, cs_threshold=0.0, max_detections=10), ten)
    # the device-produced stream takes the same argument
    _same(m.evaluate_shapes_stream(5, seed=77, cs_threshold=0.0, max_detections=40), got)
    _same(m.evaluate_shapes_stream(5, seed=77, cs_threshold=0.0, max_detections=10), m.evaluate_shapes_stream(5, seed=77, cs_threshold=0.0))


# ------------------------------------------------------------------------------------------------ the argument
def test_max_detections_is_checked():
    cfg, m = _model()
    p = _picture(40, 30, 2)
    for bad in (0, 129, True, 2.5):
        with pytest.raises(ValueError, match="max_detections"):
            m.detect(p, max_detections=bad)
        with pytest.raises(ValueError, match="max_detections"):
            m.detect_many([p], max_detections=bad)
        with pytest.raises(ValueError, match="max_detections"):
            m.evaluate([], max_detections=bad)
        with pytest.raises(ValueError, match="max_detections"):
            m.evaluate_shapes_stream(2, max_detections=bad)
    with pytest.raises(TypeError):
        m.detect_many([p], None, 0.35, 3, "image", "dense", False, 10)               # keyword only
    cfg2 = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    m2 = MaskYOLO(mode="inference", config=cfg2, seed=4)
    assert "full_masks" in m2.detect(p, cs_threshold=0.0)[0]
    for call in (lambda: m2.detect(p, max_detections=10), lambda: m2.detect_many([p], max_detections=10), lambda: m2.evaluate([], max_detections=10),
                 lambda: m2.evaluate_shapes_stream(1, max_detections=10)):
        with pytest.raises(ValueError, match="DETECT_MASKS_FOR_SELECTED_ONLY"):
            call()

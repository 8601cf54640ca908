"""The device segment rasteriser (csrc/segment_kernels.hip: myolo_segment_masks) against its host restatement (myolo.coco.segment_mask_sampled)
and against the real scikit-image masks of the committed VIA outlines, bit for bit; Net.stage_segments against the host-mask route; MaskYOLO.train() and
MaskYOLO.evaluate() on a COCODataset without a single load_mask call.

(Not here: a COCO ground truth fed back as the prediction scoring 1.0.  tests/test_gpu_evaluate.py builds that case inline in one test function,
from masks made for an exact paste, and has no helper that takes a dataset.)"""
import numpy as np
import pytest

from test_coco_host import CATS, flat_xy, hand_rles, rle_segment, scaled_parts, write_coco
from test_polygon_host import fixture_cases

pytestmark = pytest.mark.gpu

KEYS = ("images", "true_boxes", "y_true", "gt_ids", "gt_boxes", "gt_masks")
CHUNK = 256            # SEG_CHUNK: the vertices of a part staged at a time
GROUP = 32             # SEG_GROUP: the slots of a register, and the parts whose row extents are formed at a time


def _pack(slots, B, T):
    """slots[b][t] = None or (parts: list of [k,2] arrays, counts or None) -> the six tables of myolo_segment_masks (without src_h)"""
    verts, part_off, slot_part, bounds, slot_bound = [np.zeros((0, 2))], [0], [], [], []
    nv = nb = 0
    for b in range(B):
        for t in range(T):
            slot_part.append(len(part_off) - 1)
            slot_bound.append(nb)
            if slots[b][t] is None:
                continue
            parts, counts = slots[b][t]
            for p in parts:
                verts.append(np.asarray(p, np.float64))
                nv += len(p)
                part_off.append(nv)
            if counts is not None:
                bd = np.cumsum(np.asarray(counts, np.int64))[:-1]
                bounds.append(bd)
                nb += len(bd)
    slot_part.append(len(part_off) - 1)
    slot_bound.append(nb)
    bounds = np.concatenate(bounds) if bounds else np.zeros(0, np.int64)
    return (np.concatenate(verts), np.array(part_off, np.int32), np.array(slot_part, np.int32), bounds.astype(np.int32),
            np.array(slot_bound, np.int32))


def _run_kernel(tables, src_h, rows, cols, B, H, W, T, boxes=True, prefill=9):
    import torch
    from myolo import _ext as X
    dev = torch.device("cuda:0")
    verts, part_off, slot_part, bounds, slot_bound = tables
    # what the kernel trusts
    assert part_off[0] == 0 and part_off[-1] == len(verts) and (np.diff(part_off) >= 0).all()
    assert slot_part.shape == slot_bound.shape == (B * T + 1,) and (np.diff(slot_part) >= 0).all() and (np.diff(slot_bound) >= 0).all()
    assert slot_part[-1] == len(part_off) - 1 and slot_bound[-1] == len(bounds) and slot_part[0] == 0 and slot_bound[0] == 0
    assert rows.shape == (B, H) and cols.shape == (B, W) and src_h.shape == (B,)
    assert all(a.dtype == np.int32 for a in (part_off, slot_part, bounds, slot_bound, src_h, rows, cols)) and verts.dtype == np.float64
    for b in range(B):
        assert 0 <= rows[b].min() and rows[b].max() < src_h[b] and cols[b].min() >= 0
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.size else None for a in (verts, part_off, slot_part, bounds, slot_bound, src_h, rows, cols)]
    out = torch.full((B, H, W, T), prefill, dtype=torch.uint8, device=dev)
    bx = torch.full((B, T, 4), -7, dtype=torch.int32, device=dev) if boxes else None
    X.call("myolo_segment_masks", *[X.ptr(t) for t in d], X.ptr(out), X.ptr(bx), B, H, W, T, X.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), (bx.cpu().numpy() if boxes else None)


def _expected(slots, src, rows, cols, B, H, W, T):
    from myolo.coco import segment_mask_sampled
    want = np.zeros((B, H, W, T), np.uint8)
    for b in range(B):
        for t in range(T):
            if slots[b][t] is None:
                continue
            parts, counts = slots[b][t]
            m = segment_mask_sampled(list(parts), rows[b], cols[b])
            if counts is not None:
                m = m | segment_mask_sampled(rle_segment(src[b][0], src[b][1], counts), rows[b], cols[b])
            want[b, :, :, t] = m
    return want


@pytest.mark.parametrize("T", [5, 34])
def test_kernel_equals_the_host_restatement(T):
    """B = 3, H = 40, W = 56: rows of 56 pixels (no multiple of 64), 40 rows in workgroups of 4.  Image 0 has identity tables, image 1 is sampled
    from 37 x 53, image 2 down from 97 x 131.  T = 5: byte stores; T = 34: halfword stores and a second group of slots.  The output starts as 9s:
    an element nobody wrote shows."""
    from myolo import rle
    from myolo.myolo_utils import extract_bboxes, mask_index_tables
    c = fixture_cases()
    B, H, W = 3, 40, 56
    src = [(40, 56), (37, 53), (97, 131)]

    def fx(name):
        return c["verts"][c["names"].index(name)]
    lens = [len(fx("syn/chunk%+d/0" % d)) for d in (-1, 0, 1)]
    assert lens == [CHUNK - 1, CHUNK, CHUNK + 1] and len(fx("syn/one_int/0")) == 1
    hr1, hr2 = hand_rles(37, 53), hand_rles(97, 131)
    many = [np.array([[2., 2.], [9., 4.], [5., 11.]]) * [1 + .2 * (k % 5), 1 + .3 * (k % 7)] + [2 * k, 3 * k] for k in range(GROUP + 1)]
    slots = [
        # the chunk boundary as one part and as two parts of one slot; empty; one vertex; parts AND a code in one slot
        [([fx("syn/chunk-1/0")], None), ([fx("syn/chunk+0/0"), fx("syn/chunk+1/0")], None), None, ([fx("syn/one_int/0")], None),
         (scaled_parts(40, 56)[:2], hand_rles(40, 56)["lead0"])],
        # every hand-made code, over the whole 37 x 53 image
        [([], hr1["zero"]), ([], hr1["one"]), ([], hr1["lead0"]), ([], hr1["midzero"]), ([], hr1["alternate"])],
        # three parts with overlaps; a part wholly outside the frame; GROUP + 1 parts in one slot; alternating pixels (12706 boundaries); a long outline
        [(scaled_parts(97, 131), None), ([fx("syn/outside/1")], None), (many, None), ([], hr2["alternate"]), ([fx("syn/long1500/1")], None)],
    ]
    rs = np.random.RandomState(T)
    for b, (h, w) in enumerate(src):
        for t in range(5, T):                                   # T = 34: parts, codes, both and empty slots in turn, into the second group
            kind = (t + 1) % 4
            parts = [scaled_parts(h, w)[(t + j) % 3] + (t % 5) for j in range(1 + t % 2)]
            counts = rle.encode(rs.rand(h, w) > .7)["counts"]
            slots[b].append([None, (parts, None), ([], counts), (parts, counts)][kind])
    tables = [mask_index_tables(h, w, [H / h, W / w]) for h, w in src]
    rows = np.stack([t[0] for t in tables]).astype(np.int32)
    cols = np.stack([t[1] for t in tables]).astype(np.int32)
    assert np.array_equal(rows[0], np.arange(H)) and rows[1].max() == 36 and cols[2].max() == 130
    src_h = np.array([h for h, _ in src], np.int32)
    want = _expected(slots, src, rows, cols, B, H, W, T)
    assert want[0, :, :, 0].any() and want[0, :, :, 3].sum() == 1 and not want[0, :, :, 2].any() and want[0, :, :, 4].any()
    assert not want[1, :, :, 0].any() and want[1, :, :, 1].all() and want[1, :, :, 4].any() and not want[1, :, :, 4].all()
    assert want[2, :, :, 0].any() and not want[2, :, :, 1].any() and want[2, :, :, 2].any() and want[2, :, :, 3].any()
    packed = _pack(slots, B, T)
    got, boxes = _run_kernel(packed, src_h, rows, cols, B, H, W, T)
    assert got.max() <= 1, "an element was left unwritten"
    for b in range(B):
        for t in range(T):
            assert np.array_equal(got[b, :, :, t], want[b, :, :, t]), (b, t, int((got[b, :, :, t] != want[b, :, :, t]).sum()))
    want_boxes = np.stack([extract_bboxes(want[b]) for b in range(B)])
    assert boxes.dtype == np.int32 and np.array_equal(boxes, want_boxes), np.argwhere(boxes != want_boxes)[:5]
    assert not boxes[0, 2].any() and not boxes[1, 0].any() and list(boxes[1, 1]) == [0, 0, W, H]
    # the same call again, and without boxes
    again, boxes2 = _run_kernel(packed, src_h, rows, cols, B, H, W, T)
    assert again.tobytes() == got.tobytes() and boxes2.tobytes() == boxes.tobytes()
    plain, none = _run_kernel(packed, src_h, rows, cols, B, H, W, T, boxes=False)
    assert none is None and plain.tobytes() == got.tobytes()


def test_argument_checks():
    import torch
    from myolo import _ext as X
    lib = X.load()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    p = X.ptr(buf)
    s = X.stream()
    assert lib.myolo_segment_masks(p, p, p, p, p, p, p, p, None, p, 1, 1, 1, 1, s) == -1 and b"null" in lib.myolo_last_error_string()
    assert lib.myolo_segment_masks(p, p, None, p, p, p, p, p, p, p, 1, 1, 1, 1, s) == -1 and b"null" in lib.myolo_last_error_string()
    assert lib.myolo_segment_masks(p, p, p, p, p, p, p, p, p, p, 1, 1, 1, 0, s) == -1 and b"T=0" in lib.myolo_last_error_string()
    assert lib.myolo_segment_masks(p, p, p, p, p, p, p, p, p, p, 0, 1, 1, 1, s) == -1
    # verts, bounds and boxes may be NULL: one empty slot
    out = torch.full((1, 1, 1, 1), 9, dtype=torch.uint8, device="cuda:0")
    z = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    X.call("myolo_segment_masks", None, X.ptr(z), X.ptr(z), None, X.ptr(z), X.ptr(z), X.ptr(z), X.ptr(z), X.ptr(out), None, 1, 1, 1, 1, s)
    torch.cuda.synchronize()
    assert int(out.item()) == 0


@pytest.mark.parametrize("size", [64, 224])
def test_single_part_segments_equal_the_polygon_kernel_on_the_via_outlines(size):
    """the 228 committed VIA outlines, one image per annotated image and one slot per outline, recast as single-part segments: myolo_segment_masks
    writes the fixture's real scikit-image mask of every outline, sampled by the image's tables (the reference was the retired polygon kernel)"""
    from myolo.myolo_utils import mask_index_tables
    c = fixture_cases()
    n_real = int(c["fx"]["n_real"])
    assert n_real == 228
    images = {}
    for k in range(n_real):
        assert c["names"][k].startswith("real/")
        images.setdefault(c["names"][k].rsplit("/", 1)[0], []).append(k)
    B, T = len(images), max(len(v) for v in images.values())
    H = W = size
    assert (B, T) == (116, 8)
    slots, rows, cols, src_h = [], [], [], []
    ref = np.zeros((B, H, W, T), np.uint8)
    for b, ks in enumerate(images.values()):
        h, w = [int(v) for v in c["frames"][ks[0]]]
        r, cc = mask_index_tables(h, w, [H / h, W / w])
        rows.append(r)
        cols.append(cc)
        src_h.append(h)
        slots.append([([c["verts"][k]], None) for k in ks] + [None] * (T - len(ks)))
        for t, k in enumerate(ks):
            ref[b, :, :, t] = c["masks"][k][r][:, cc]
    rows, cols, src_h = np.stack(rows).astype(np.int32), np.stack(cols).astype(np.int32), np.array(src_h, np.int32)
    packed = _pack(slots, B, T)
    assert len(packed[1]) - 1 == n_real
    got, _ = _run_kernel(packed, src_h, rows, cols, B, H, W, T)
    assert ref.max() == 1 and ref.any(axis=(1, 2)).sum() == n_real          # every outline sets a sampled pixel at both sizes
    assert got.tobytes() == ref.tobytes(), int((got != ref).sum())


# ---------------------------------------------------------------- the routes
def _small_cfg():
    from myolo.config import ShapesConfig, make_config
    return make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], ALPHA=0.5, BATCH_SIZE=2)


def _coco_dataset(tmp_path, n_images, crowd="keep", outside_in=None):
    """images of several sizes with at most four annotations each: multi-part polygons, one-part polygons and run-length codes (one a crowd);
    outside_in: the image that gets, between its first and second annotation, a square wholly outside its frame (an instance without a pixel)"""
    from myolo import rle
    from myolo.coco import load_coco
    sizes = [(80, 100), (64, 64), (50, 70), (120, 90), (64, 96), (33, 47)][:n_images]
    images = [(10 + i, "img_%d.png" % i, h, w) for i, (h, w) in enumerate(sizes)]
    cat = [c for c, _ in CATS]
    anns = []
    for i, (h, w) in enumerate(sizes):
        parts = scaled_parts(h, w)
        yy, xx = np.mgrid[0:h, 0:w]
        disc = (yy - .6 * h) ** 2 + (xx - .4 * w) ** 2 <= (.25 * min(h, w)) ** 2
        code = rle.encode(disc)
        segs = [[flat_xy(parts[0])], [flat_xy(parts[1] * .5), flat_xy(parts[2] * [.5, 1.0])],
                {"size": [h, w], "counts": rle.to_string(code["counts"]) if i % 2 else [int(v) for v in code["counts"]]},
                [flat_xy(parts[2])]][:2 + i % 3]
        if i == outside_in:
            segs.insert(1, [[w + 5., 2., w + 9., 2., w + 9., 6., w + 5., 6.]])
        for j, s in enumerate(segs):
            anns.append({"id": 100 * i + j, "image_id": 10 + i, "category_id": cat[(i + j) % 3], "iscrowd": int(isinstance(s, dict) and i == 1),
                         "segmentation": s})
    path = write_coco(tmp_path / "coco", images, anns, CATS)
    return load_coco(path, str(tmp_path / "coco"), crowd=crowd)


def test_segment_route_equals_the_host_mask_route(tmp_path):
    """Net.stage_segments (segments up, masks decoded on the device) against Net.stage_augmented fed load_mask's output for the same samples, with
    identity rows: the six device arrays, bit for bit."""
    import torch
    from myolo.augment import DeviceAugmenter, IDENTITY_ROW
    from myolo.model import MaskYOLO
    from myolo.myolo_utils import BatchGenerator, load_image_gt
    cfg = _small_cfg()
    ds = _coco_dataset(tmp_path, 4)
    assert max(len(ds.load_segments(i)[0]) for i in ds.image_ids) <= cfg.TRUE_BOX_BUFFER
    assert any(isinstance(s, dict) for i in ds.image_ids for s in ds.load_segments(i)[0])
    model = MaskYOLO(mode="training", config=cfg)
    net = model.net
    host = [list(load_image_gt(ds, cfg, i)) + [int(i)] for i in ds.image_ids]
    seg = model._collect_segments(ds)
    assert all(len(h[1]) == len(s[1]) for h, s in zip(host, seg))                   # no segment came out empty at 64 x 64
    gen_h = BatchGenerator(host, cfg, 'training', shuffle=False, norm=True)
    gen_s = BatchGenerator(seg, cfg, 'training', shuffle=False, norm=True)
    aug = DeviceAugmenter(cfg, net.dev)
    row_of = lambda inst: IDENTITY_ROW                                               # noqa: E731
    for i in range(2):
        a = net.stage_augmented(lambda arrays: gen_h.fill_raw(i, arrays, row_of), 2, aug)
        fill, n_verts, n_parts, n_bounds = gen_s.segment_batch(i, row_of)
        b = net.stage_segments(fill, 2, aug, n_verts=n_verts, n_parts=n_parts, n_bounds=n_bounds)
        torch.cuda.synchronize()
        for k in KEYS:
            x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (i, k, int((x != y).sum()))
        assert (b["gt_ids"].cpu().numpy() != 0).sum() == len(host[2 * i][1]) + len(host[2 * i + 1][1]) and b["gt_masks"].cpu().numpy().any()


def test_train_on_a_coco_dataset_takes_the_segment_route(tmp_path):
    from myolo.model import MaskYOLO
    cfg = _small_cfg()
    ds = _coco_dataset(tmp_path, 4)
    calls = []
    real = ds.load_mask
    ds.load_mask = lambda i: (calls.append(i), real(i))[1]

    def run(**kw):
        model = MaskYOLO(mode="training", config=cfg)
        hist = model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", verbose=0, **kw)
        assert len(hist) == 1 and np.all(np.isfinite(hist)), hist
        assert model.host_times["steps"] == 2 and model.host_times["polygon_batches"] == 0
        return hist[0], model.host_times["segment_batches"]

    l_dev, n_dev = run()
    assert n_dev == 2 and calls == []
    l_host, n_host = run(device_polygons=False)
    assert n_host == 0 and sorted(calls) == [0, 1, 2, 3]
    print("epoch loss: segment route %.9g, host-mask route %.9g" % (l_dev, l_host))
    assert abs(l_dev - l_host) < 1e-3 * max(1.0, abs(l_host)), (l_dev, l_host)          # the same inputs reach the same step


def test_evaluate_on_a_coco_dataset_decodes_the_ground_truth_on_the_device(tmp_path):
    """evaluate(coco_ds) against evaluate() on the rows load_image_gt gives for the same dataset (today's path): seeded random weights,
    cs_threshold 0, six images in batches of four (a short last batch); the device route never asks for a mask."""
    import gc
    import torch
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO
    from myolo.myolo_utils import load_image_gt
    from test_gpu_evaluate import _same
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4)
    ds = _coco_dataset(tmp_path, 6, outside_in=2)
    rows = [load_image_gt(ds, cfg, i) for i in ds.image_ids]                         # (before load_mask is wrapped)
    # image 2's second annotation has no pixel: load_image_gt has dropped it and closed the gap; the device route finds it by its area
    assert len(rows) == 6 and all(len(r[1]) == len(ds.load_segments(i)[0]) - (i == 2) <= cfg.MAX_GT_INSTANCES for i, r in enumerate(rows))
    assert len(ds.load_segments(2)[0]) == 5 and not ds.load_mask(2)[0][:, :, 1].any()
    calls = []
    real = ds.load_mask
    ds.load_mask = lambda i: (calls.append(i), real(i))[1]
    m = MaskYOLO(mode="inference", config=cfg, seed=4)
    try:
        got = m.evaluate(ds, cs_threshold=0.0)
        assert calls == []
        want = m.evaluate(rows, cs_threshold=0.0)
        assert got["n_images"] == 6 and got["n_gt"] == sum(len(r[1]) for r in rows) and got["n_det"] >= 6
        _same(got, want)
        _same(m.evaluate(ds, cs_threshold=0.0, max_samples=3), m.evaluate(rows[:3], cs_threshold=0.0))
        assert calls == []
    finally:
        del m
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.synchronize()

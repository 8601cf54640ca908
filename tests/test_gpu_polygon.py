"""VIA outlines through the device rasteriser as one-part segments (csrc/segment_kernels.hip: myolo_segment_masks) against the host restatement and
against the real scikit-image output of the fixture, bit for bit; the route through Net.stage_segments against the host-mask route through
Net.stage_augmented; and MaskYOLO.train() on a VIADataset without a single load_mask call."""
import json
import os

import numpy as np
import pytest

from test_gpu_segments import _pack as pack_segments, _run_kernel as run_segments
from test_polygon_host import _write_dataset, fixture_cases

pytestmark = pytest.mark.gpu

KEYS = ("images", "true_boxes", "y_true", "gt_ids", "gt_boxes", "gt_masks")


def _pack(slots, B, T):
    """slots[b][t] = [k,2] array or None -> the five tables of myolo_segment_masks with every outline a one-part segment"""
    tables = pack_segments([[None if p is None else ([p], None) for p in row] for row in slots], B, T)
    assert len(tables[1]) - 1 == sum(p is not None for row in slots for p in row) and tables[3].size == 0          # one part per outline, no code
    return tables


def _run_kernel(tables, src, rows, cols, B, H, W, T):
    """src: the (h, w) of every source image.  boxes = NULL, as Net.stage_segments calls the entry; the output starts as 9s"""
    got, _ = run_segments(tables, np.array([h for h, _ in src], np.int32), rows, cols, B, H, W, T, boxes=False)
    return got


@pytest.mark.parametrize("T", [5, 34])
def test_kernel_equals_the_host_fill_on_synthetic_outlines(T):
    """B = 3, H = 40, W = 56: rows of 56 pixels (no multiple of 64), 40 rows in workgroups of 4, a non-square frame.  Image 0 has identity tables,
    image 1 is sampled down from 97 x 131, image 2 up from 17 x 23.  T = 5: byte stores; T = 34: halfword stores and a second group of slots
    (the kernel gathers 32 slots per register).  The output starts as 9s: an element nobody wrote shows."""
    from myolo.myolo_utils import mask_index_tables
    from myolo.polygon import polygon_mask_sampled
    c = fixture_cases()
    B, H, W = 3, 40, 56
    src = [(40, 56), (97, 131), (17, 23)]
    want_names = [["syn/long1500/0", "syn/chunk-1/0", None, "syn/chunk+0/0", "syn/chunk+1/0"],
                  ["syn/float/1", None, "syn/outside/1", "syn/long1500/1", "syn/star/1"],
                  ["syn/int/2", "syn/hrect/5", None, "syn/long_int/2", "syn/ring/2"]]
    more = [[n for n in c["names"] if n.startswith("syn/") and n.endswith("/%d" % f) and tuple(c["frames"][c["names"].index(n)]) == src[f]]
            for f in range(3)]
    slots = []
    for b in range(B):
        names = list(want_names[b])
        extra = [n for n in more[b] if n not in names]
        while len(names) < T:                                   # T = 34: more of the same frame's synthetics, an empty slot now and then
            names.append(None if len(names) % 7 == 0 else extra[len(names) % len(extra)])
        slots.append([None if n is None else c["verts"][c["names"].index(n)] for n in names[:T]])
    tables = [mask_index_tables(h, w, [H / h, W / w]) for h, w in src]
    rows = np.stack([t[0] for t in tables]).astype(np.int32)
    cols = np.stack([t[1] for t in tables]).astype(np.int32)
    assert np.array_equal(rows[0], np.arange(H)) and rows[1].max() == 96 and cols[2].max() == 22
    want = np.zeros((B, H, W, T), np.uint8)
    for b in range(B):
        for t in range(T):
            if slots[b][t] is not None:
                want[b, :, :, t] = polygon_mask_sampled(slots[b][t][:, 0], slots[b][t][:, 1], rows[b], cols[b])
    assert want[0, :, :, 0].any() and want[1, :, :, 3].any() and want[2, :, :, 3].any() and not want[1, :, :, 2].any()
    got = _run_kernel(_pack(slots, B, T), src, rows, cols, B, H, W, T)
    assert got.max() <= 1, "an element was left unwritten"
    for b in range(B):
        for t in range(T):
            assert np.array_equal(got[b, :, :, t], want[b, :, :, t]), (b, t, int((got[b, :, :, t] != want[b, :, :, t]).sum()))
    # (the argument checks -- null masks, T = 0, B = 0 -- stand in tests/test_gpu_segments.py::test_argument_checks)


def test_kernel_equals_scikit_image_on_the_food_validation_annotations():
    """the seven annotated images of golden/via/food/val, H = W = 64, T = 8 (word stores): the fixture's real scikit-image masks, sampled by the
    host tables, are what the kernel writes."""
    from myolo.myolo_utils import mask_index_tables
    c = fixture_cases()
    B, H, W, T = 7, 64, 64, 8
    slots, rows, cols, src = [], [], [], []
    want = np.zeros((B, H, W, T), np.uint8)
    total = 0
    for b in range(B):
        ks = [k for k, n in enumerate(c["names"]) if n.startswith("real/food/val/%d/" % b)]
        assert 1 <= len(ks) <= T
        h, w = [int(v) for v in c["frames"][ks[0]]]
        src.append((h, w))
        r, cc = mask_index_tables(h, w, [H / h, W / w])
        rows.append(r)
        cols.append(cc)
        for t, k in enumerate(ks):
            want[b, :, :, t] = c["masks"][k][r][:, cc]
            assert want[b, :, :, t].any()
        slots.append([c["verts"][k] for k in ks] + [None] * (T - len(ks)))
        total += len(ks)
    assert total == 21
    got = _run_kernel(_pack(slots, B, T), src, np.stack(rows).astype(np.int32), np.stack(cols).astype(np.int32), B, H, W, T)
    assert got.tobytes() == want.tobytes(), int((got != want).sum())


def _small_cfg():
    from myolo.config import ShapesConfig, make_config
    return make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], ALPHA=0.5, BATCH_SIZE=2)


def _via_dataset(tmp_path, n_images, tiny_in=None):
    """food/val's first images as a VIADataset; tiny_in: the image that gets, between its first and second region, a square around ONE source
    pixel which the 64 x 64 tables do not sample"""
    from myolo.myolo_utils import mask_index_tables
    from myolo.via import load_via
    root, kept = _write_dataset(tmp_path, n_images=n_images)
    if tiny_in is not None:
        c = fixture_cases()
        h, w = [int(v) for v in c["frames"][c["names"].index("real/food/val/%d/0" % tiny_in)]]
        rows, cols = mask_index_tables(h, w, [64 / h, 64 / w])
        r, cc = int(rows[10]) + 2, int(cols[10]) + 2
        assert r not in rows and cc not in cols
        path = os.path.join(root, "val", "via_food_annotation.json")
        d = json.load(open(path))
        key = [k for k in d if d[k]["filename"] == "img_%d.png" % tiny_in][0]
        tiny = {"shape_attributes": {"name": "polygon", "all_points_x": [cc - .4, cc + .4, cc + .4, cc - .4],
                                     "all_points_y": [r - .4, r - .4, r + .4, r + .4]}, "region_attributes": {}}
        d[key]["regions"].insert(1, tiny)
        json.dump(d, open(path, "w"))
    return load_via(root, "val"), kept


def test_polygon_route_equals_the_host_mask_route(tmp_path):
    """Net.stage_segments (outlines up as one-part segments, masks filled on the device) against Net.stage_augmented fed load_mask's output for the
    same samples: the six device arrays, bit for bit, with identity rows and with drawn rows (flip and rotation)."""
    import torch
    from myolo.augment import Augmentation, DeviceAugmenter, IDENTITY_ROW
    from myolo.model import MaskYOLO
    from myolo.myolo_utils import BatchGenerator, load_image_gt
    cfg = _small_cfg()
    ds, kept = _via_dataset(tmp_path, 2, tiny_in=1)
    model = MaskYOLO(mode="training", config=cfg)
    net = model.net
    host = [list(load_image_gt(ds, cfg, i)) + [int(i)] for i in ds.image_ids]
    poly = model._collect_segments(ds, load="load_polygons")
    assert all(len(s) == 1 and np.array_equal(s[0], p) for inst in poly for s, p in zip(inst[2], ds.load_polygons(inst[4])[0]))
    assert [inst[5] for inst in poly] == [ds.image_info[i]["height"] for i in ds.image_ids]         # the real source heights
    # the tiny outline: one pixel at full resolution, nothing in the network frame -- load_image_gt has dropped it, the polygon samples still hold it
    n1 = len(kept[1]["regions"])
    assert ds.load_mask(1)[0][:, :, 1].sum() == 1 and len(poly[1][2]) == n1 + 1 and len(host[1][1]) == n1 >= 2
    gen_h = BatchGenerator(host, cfg, 'training', shuffle=False, norm=True)
    gen_p = BatchGenerator(poly, cfg, 'training', shuffle=False, norm=True)
    aug = DeviceAugmenter(cfg, net.dev)
    drawn = Augmentation(fliplr=1.0, rotate=(-30, 30), seed=3)
    for name, rows in (("identity", [IDENTITY_ROW, IDENTITY_ROW]), ("drawn", [drawn.params(0, i, 64, 64) for i in range(2)])):
        row_of = lambda inst: rows[inst[4]]                                          # noqa: E731
        a = net.stage_augmented(lambda arrays: gen_h.fill_raw(0, arrays, row_of), 2, aug)
        fill, n_verts, n_parts, n_bounds = gen_p.segment_batch(0, row_of)
        assert n_parts == len(poly[0][2]) + len(poly[1][2]) and n_bounds == 0
        b = net.stage_segments(fill, 2, aug, n_verts=n_verts, n_parts=n_parts, n_bounds=n_bounds)
        torch.cuda.synchronize()
        for k in KEYS:
            x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, k, int((x != y).sum()))
        ids = b["gt_ids"].cpu().numpy()
        if name == "identity":
            # dropped on the device and the rest compacted: n1 live slots in front, and slot 1 holds what was region 2 of the file
            assert (ids[1] != 0).sum() == n1 and (ids[1][:n1] != 0).all()
            want = ds.load_mask(1)[0][:, :, 2][poly[1][3][0]][:, poly[1][3][1]]
            assert np.array_equal(b["gt_masks"].cpu().numpy()[1, :, :, 1], want.astype(np.uint8))
        assert (ids != 0).sum() >= 3 and b["gt_masks"].cpu().numpy().any()


def test_train_on_a_via_dataset_takes_the_polygon_route(tmp_path):
    from myolo.model import MaskYOLO
    cfg = _small_cfg()
    ds, _ = _via_dataset(tmp_path, 4)
    calls = []
    real = ds.load_mask
    ds.load_mask = lambda i: (calls.append(i), real(i))[1]

    def run(**kw):
        model = MaskYOLO(mode="training", config=cfg)
        hist = model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", verbose=0, **kw)
        assert len(hist) == 1 and np.all(np.isfinite(hist)), hist
        assert model.host_times["steps"] == 2
        return hist[0], model.host_times["polygon_batches"]

    l_dev, n_dev = run()
    assert n_dev == 2 and calls == []
    l_host, n_host = run(device_polygons=False)
    assert n_host == 0 and sorted(calls) == [0, 1, 2, 3]
    print("epoch loss: polygon route %.9g, host-mask route %.9g" % (l_dev, l_host))
    assert abs(l_dev - l_host) < 1e-3 * max(1.0, abs(l_host)), (l_dev, l_host)          # the same inputs reach the same step

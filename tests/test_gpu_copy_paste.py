"""Copy-paste on the device (myolo_copy_paste_batch, csrc/augment_kernels.hip): against the numpy restatement of the contract
(tests/copy_paste_ref.py) through the C-ABI, against the first stage where the two must agree (zero select), on a case made by hand, through its
refusals, and through MaskYOLO.train(copy_paste=...) on the dense, polygon and segment routes.  Every comparison is bit for bit."""
import numpy as np
import pytest

import augment_ref as R
import copy_paste_ref as CP

pytestmark = pytest.mark.gpu

FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))
KEYS = ("images", "true_boxes", "y_true", "gt_ids", "gt_boxes", "gt_masks")
ANCHORS = np.array([0.6, 0.7, 1.4, 1.2], np.float64)
G, A, C = 2, 2, 8


def _assert_bit_equal(got, want, keys=KEYS + ("dropped",)):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))


class Entry(object):
    """myolo_copy_paste_batch on one set of operands, outputs pre-filled with values the kernels never write"""

    def __init__(self, images, masks, ids, donor, select):
        import torch
        from myolo import _ext as X
        self.X, self.torch = X, torch
        self.B, self.H, self.W, self.T = masks.shape
        dev = torch.device("cuda:0")
        self.host_src = (images, masks, ids, np.asarray(donor, np.int32), np.asarray(select, np.int32))
        self.src = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in self.host_src + (ANCHORS,)]
        B, H, W, T = self.B, self.H, self.W, self.T
        self.out = dict(images=torch.full((B, H, W, 3), -1., device=dev), gt_masks=torch.full((B, H, W, T), 9, dtype=torch.uint8, device=dev),
                        gt_boxes=torch.full((B, T, 4), -1, dtype=torch.int32, device=dev), gt_ids=torch.full((B, T), -1, dtype=torch.int32, device=dev),
                        y_true=torch.full((B, G, G, A, 5 + C), -1., device=dev), true_boxes=torch.full((B, T, 4), -1., device=dev),
                        dropped=torch.full((B,), -7, dtype=torch.int32, device=dev))
        self.ws = torch.empty(X.copy_paste_ws_bytes(B, T), dtype=torch.uint8, device=dev)
        self.untouched = {k: v.cpu().numpy() for k, v in self.out.items()}

    def call(self, **kw):
        X, o, s = self.X, self.out, self.src
        a = dict(images=X.ptr(s[0]), masks=X.ptr(s[1]), ids=X.ptr(s[2]), donor=X.ptr(s[3]), select=X.ptr(s[4]), out_images=X.ptr(o["images"]),
                 out_ids=X.ptr(o["gt_ids"]), y_true=X.ptr(o["y_true"]), dropped=X.ptr(o["dropped"]), H=self.H, T=self.T, ws_bytes=self.ws.numel())
        a.update(kw)
        return X.load().myolo_copy_paste_batch(a["images"], a["masks"], a["ids"], a["donor"], a["select"], X.ptr(s[5]), a["out_images"],
                                               X.ptr(o["gt_masks"]), X.ptr(o["gt_boxes"]), a["out_ids"], a["y_true"], X.ptr(o["true_boxes"]),
                                               a["dropped"], self.B, a["H"], self.W, a["T"], G, A, C, self.ws.data_ptr(), a["ws_bytes"], X.stream())

    def host(self):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def want(self):
        s = self.host_src
        return CP.copy_paste_batch(s[0], s[1], s[2], s[3], s[4], self.H, self.W, self.T, G, A, C, ANCHORS)


def _scene(B, H, W, T, seed):
    """random floats; rectangles (mask bytes 1 or 255) in the live slots: image 0 has every slot live, image 1 the first T // 2 (one with T = 1),
    image 2 only its LAST slot (none with T = 1), the others a random number in random slots; with T >= 3 images 1.. also have set pixels in one
    slot whose class id is 0.  Tables: the chain 0 <- 1 <- 2 <- 0 with every slot selected (bit 31 with T = 32: image 1 accepts slot 31 of image
    2), then an image that takes from itself and one that takes from image 1, with random selections."""
    rs = np.random.RandomState(seed)
    images = rs.random_sample((B, H, W, 3)).astype(np.float32)
    masks = np.zeros((B, H, W, T), np.uint8)
    ids = np.zeros((B, T), np.int32)
    for b in range(B):
        live = (list(range(T)), list(range(max(1, T // 2))), [T - 1] if T > 1 else [])[b] if b < 3 else \
            sorted(rs.choice(T, rs.randint(0, T + 1), replace=False).tolist())
        for t in live:
            y0, x0 = rs.randint(0, H - 4), rs.randint(0, W - 4)
            h, w = rs.randint(3, H // 2 + 1), rs.randint(3, W // 2 + 1)
            masks[b, y0:y0 + h, x0:x0 + w, t] = 1 if t % 2 == 0 else 255
            ids[b, t] = 1 + rs.randint(0, 7)
        dead = [t for t in range(T) if t not in live]
        if T >= 3 and b >= 1 and dead:
            masks[b, H // 4:H // 2, :, dead[0]] = 1                 # set pixels, no instance
    every = np.array([(1 << T) - 1], np.uint32).view(np.int32)[0]
    donor = np.array([1, 2, 0, 3, 1][:B], np.int32)
    select = np.array([every] * 3 + [rs.randint(1, 1 << min(T, 30)) for _ in range(B - 3)], np.int32)
    return images, masks, ids, donor, select


CASES = [(37, 29, 3, 5), (37, 29, 3, 6), (64, 64, 3, 4), (37, 91, 5, 3), (64, 64, 5, 32), (64, 64, 3, 1)]


def check_scene_is_not_vacuous(e, want):
    """asserted on the restatement's outputs: some image accepts an instance, some image counts a rejected one, and -- with T >= 2; with one slot an
    image that has an own instance has no free slot, so nothing can be pasted over one -- some own instance loses pixels to a paste"""
    images, masks, ids, donor, select = e.host_src
    B, T = e.B, e.T
    plans = [CP.accepted(ids, donor, select, b, T) for b in range(B)]
    assert any(len(a) > 0 for _, a, _ in plans) and (want["dropped"] > 0).any()
    assert want["dropped"].tolist() == [n for _, _, n in plans]
    if T >= 2:
        lost = 0
        for b, (d, acc, _) in enumerate(plans):
            U = np.zeros(masks.shape[1:3], bool)
            for t in acc:
                U |= masks[d][:, :, t] != 0
            lost += sum(int(((masks[b][:, :, t] != 0) & U).any()) for t in range(T) if ids[b][t] != 0)
        assert lost > 0
    if T == 32:
        assert select[1] < 0 and 31 in plans[1][1]                  # bit 31 selected and accepted


@pytest.mark.parametrize("H,W,B,T", CASES)
def test_entry_equals_the_restatement(H, W, B, T):
    """through the C-ABI: 37 x 29 (1073 pixels: a ragged last workgroup in the stats and in the render pass; T = 5: byte loads and mask bytes per image
    no multiple of four, T = 6: two-byte loads), 64 x 64 with T = 4 and 32 (words, several workgroups per image, bit 31), 37 x 91 with T = 3 and
    B = 5, T = 1.  Image 1 is donor and receiver: it must be read as it was before the paste.  Two calls give the same bytes."""
    e = Entry(*_scene(B, H, W, T, seed=1))                      # (a seed under which every case passes check_scene_is_not_vacuous)
    want = e.want()
    check_scene_is_not_vacuous(e, want)
    assert e.call() == 0
    got = e.host()
    _assert_bit_equal(got, want)
    for o in e.out.values():
        o.fill_(3)
    assert e.call() == 0
    _assert_bit_equal(e.host(), got)
    # the targets are given together or not at all
    assert e.call(y_true=None) == -1 and e.X.load().myolo_last_error_string().startswith(b"copy_paste_batch: y_true and true_boxes")


def test_zero_select_reproduces_the_first_stage():
    """select all zero behind myolo_augment_batch (a full warp, so that instances are dropped and compacted): all six outputs are the first stage's
    byte for byte, whatever the donors, and nothing is counted"""
    from myolo.augment import Augmentation, DeviceAugmenter
    from myolo.config import ShapesConfig, make_config
    from myolo.shapes import make_shapes_samples
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=3)
    samples = make_shapes_samples(3, cfg, seed=1234)
    aug = Augmentation(seed=4, **FULL)
    rows = np.stack([aug.params(0, i, 64, 64) for i in range(3)])
    images, masks, ids = R.pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    dev = DeviceAugmenter(cfg, cval=aug.cval)
    plain = dev.apply(images, masks, ids, rows)
    want = {k: v.cpu().numpy() for k, v in plain.items() if k in KEYS}
    assert (want["gt_ids"] != 0).sum() >= 3 and "paste_dropped" not in plain and "_paste_src" not in plain
    for donor in ([0, 1, 2], [1, 2, 0]):
        d = dev.apply(images, masks, ids, rows, copy_paste=(np.array(donor, np.int32), np.zeros(3, np.int32)))
        _assert_bit_equal({k: v.cpu().numpy() for k, v in d.items() if k in KEYS}, want, keys=KEYS)
        assert d["paste_dropped"].cpu().numpy().tolist() == [0, 0, 0]
    # the 'yolo' form of the dict carries the same arrays
    y = dev.apply(images, masks, ids, rows, yolo=True, copy_paste=(np.array([1, 2, 0], np.int32), np.zeros(3, np.int32)))
    assert sorted(k for k in y if not k.startswith("_")) == ["images", "paste_dropped", "true_boxes", "y_true"]
    assert y["y_true"].cpu().numpy().tobytes() == want["y_true"].tobytes() and y["_gt"][0].cpu().numpy().tobytes() == want["gt_ids"].tobytes()
    # tables are checked before anything is uploaded
    for bad in ((np.array([0, 1, 3], np.int32), np.zeros(3, np.int32)), (np.array([0, 1, 2], np.int32), np.array([0, 1 << cfg.TRUE_BOX_BUFFER, 0], np.int32))):
        with pytest.raises(ValueError, match="copy-paste tables"):
            dev.apply(images, masks, ids, rows, copy_paste=bad)


def test_paste_case_by_hand():
    """64 x 64, T = 4.  Image 0 has A (rows 10..29, columns 10..39), B (rows 40..49, columns 40..49) and a slot with pixels whose class id is 0, so two
    free slots; image 1 offers three instances and all are selected: the first (rows 5..34, columns 30..63) cuts A down to columns 10..29, the
    second (rows 38..51, columns 38..51) covers B wholly, the third (rows 55..59, columns 0..7) finds no free slot: it is counted and its pixels
    stay out of the image.  Image 1 takes nothing."""
    H = W = 64
    T = 4
    rs = np.random.RandomState(3)
    images = rs.random_sample((2, H, W, 3)).astype(np.float32)
    masks = np.zeros((2, H, W, T), np.uint8)
    ids = np.zeros((2, T), np.int32)
    masks[0, 10:30, 10:40, 0], ids[0, 0] = 1, 1                 # A
    masks[0, 40:50, 40:50, 1], ids[0, 1] = 1, 2                 # B
    masks[0, 0:64, 0:5, 2] = 1                                  # class id 0: no instance, but no free slot lost either: F = 4 - 2
    masks[1, 5:35, 30:64, 0], ids[1, 0] = 1, 5
    masks[1, 38:52, 38:52, 1], ids[1, 1] = 1, 6
    masks[1, 55:60, 0:8, 2], ids[1, 2] = 1, 7
    e = Entry(images, masks, ids, [1, 1], [0b1111, 0])
    assert e.call() == 0
    got = e.host()
    _assert_bit_equal(got, e.want())
    assert got["dropped"].tolist() == [1, 0]
    assert got["gt_ids"][0].tolist() == [1, 5, 6, 0]
    assert got["gt_boxes"][0].tolist() == [[10, 10, 30, 30], [30, 5, 64, 35], [38, 38, 52, 52], [0, 0, 0, 0]]
    m = got["gt_masks"][0]
    assert m.sum(axis=(0, 1)).tolist() == [20 * 20, 30 * 34, 14 * 14, 0] and m.max() == 1
    img = got["images"][0]
    pasted = np.zeros((H, W), bool)
    pasted[5:35, 30:64] = pasted[38:52, 38:52] = True
    assert img[pasted].tobytes() == images[1][pasted].tobytes() and img[~pasted].tobytes() == images[0][~pasted].tobytes()
    assert img[55:60, 0:8].tobytes() == images[0, 55:60, 0:8].tobytes()                            # the rejected instance
    # image 1: itself
    assert got["images"][1].tobytes() == images[1].tobytes() and got["gt_masks"][1].tobytes() == masks[1].tobytes()
    assert got["gt_ids"][1].tolist() == [5, 6, 7, 0] and got["gt_boxes"][1].tolist() == [[30, 5, 64, 35], [38, 38, 52, 52], [0, 55, 8, 60], [0, 0, 0, 0]]


def test_refusals_write_nothing():
    e = Entry(*_scene(3, 64, 64, 4, seed=1))
    X, s, o = e.X, e.src, e.out
    err = X.load().myolo_last_error_string
    for kw in (dict(images=None), dict(masks=None), dict(ids=None), dict(donor=None), dict(select=None), dict(out_images=None), dict(dropped=None),
               dict(y_true=None), dict(T=33), dict(T=0), dict(H=0), dict(ws_bytes=e.ws.numel() - 4), dict(ws_bytes=0),
               dict(out_images=X.ptr(s[0])), dict(out_ids=X.ptr(s[2])), dict(dropped=X.ptr(s[3])), dict(out_images=X.ptr(s[0]) + 64 * 64 * 12)):
        assert e.call(**kw) == -1, kw
        assert err().startswith(b"copy_paste_batch:"), (kw, err())
    assert b"T" in (e.call(T=33), err())[1] and b"workspace" in (e.call(ws_bytes=8), err())[1] and b"null" in (e.call(select=None), err())[1]
    assert b"lies over" in (e.call(out_ids=X.ptr(s[2])), err())[1]
    _assert_bit_equal(e.host(), e.untouched)
    assert e.call() == 0                                            # and the same operands, unrefused, run


def _small_cfg():
    from myolo.config import ShapesConfig, make_config
    return make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], ALPHA=0.5, BATCH_SIZE=4)


def _check_second_stage(db, cfg):
    """the batch the step received is the restatement's of the first stage's outputs and the tables that went up with them"""
    mid_images, mid_masks, _, mid_ids, donor, select = [t.cpu().numpy() for t in db["_paste_src"]]
    want = CP.copy_paste_batch(mid_images, mid_masks, mid_ids, donor, select, 64, 64, cfg.TRUE_BOX_BUFFER, cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES,
                               np.asarray(cfg.ANCHORS, np.float64))
    got = {k: db[k].cpu().numpy() for k in KEYS}
    got["dropped"] = db["paste_dropped"].cpu().numpy()
    _assert_bit_equal(got, want)
    return want, (mid_ids, donor, select)


def test_train_end_to_end_with_copy_paste():
    """train(copy_paste=CopyPaste(p=1.0)) on the dense route: finite losses, and the step received the restatement's boxes for the tables planned
    from the batch's image ids; CopyPaste(p=0.0) trains exactly as copy_paste=None does; one run with mosaic and augmentation as well"""
    from myolo.augment import Augmentation, CopyPaste, Mosaic
    from myolo.model import MaskYOLO
    from myolo.shapes import ShapesDataset
    cfg = _small_cfg()
    T = cfg.TRUE_BOX_BUFFER
    ds = ShapesDataset(1234)
    ds.load_shapes(8, 64, 64)
    ds.prepare()
    by_bytes = {ds.load_image(i).astype(np.uint8).tobytes(): int(i) for i in ds.image_ids}
    assert len(by_bytes) == 8

    def run(**kw):
        model = MaskYOLO(mode="training", config=cfg, seed=3)
        seen, outs = [], []
        step = model.train_on_batch

        def spy(db, *a, **k):
            seen.append(db)
            outs.append(step(db, *a, **k))
            return outs[-1]
        model.train_on_batch = spy
        hist = model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", max_samples=8, verbose=0, **kw)
        assert len(hist) == 1 and np.all(np.isfinite(hist)) and len(seen) == 2
        return model, seen, [o["loss"] for o in outs]

    paste = CopyPaste(p=1.0, instances=0.7, seed=5)
    model, seen, losses = run(copy_paste=paste)
    assert np.all(np.isfinite(losses))
    accepted = 0
    for db in seen:
        raw, masks, ids, rows = [t.cpu().numpy() for t in db["_src"]]
        image_ids = [by_bytes[raw[b].tobytes()] for b in range(4)]
        donor, select = model.paste_tables(paste, None, ds, 0, image_ids)
        assert np.array_equal(rows, np.tile([1., 0, 0, 0, 1, 0, 1, 0], (4, 1)))                 # no augmentation: identity rows
        assert (donor != np.arange(4)).all() and (select != 0).any()
        first = R.augment_batch(raw, masks, ids, rows, 0.0, 64, 64, T, cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES, np.asarray(cfg.ANCHORS, np.float64))
        want = CP.copy_paste_batch(first["images"], first["gt_masks"], first["gt_ids"], donor, select, 64, 64, T, cfg.GRID_W, cfg.N_BOX,
                                   cfg.NUM_CLASSES, np.asarray(cfg.ANCHORS, np.float64))
        got = {k: db[k].cpu().numpy() for k in KEYS}
        got["dropped"] = db["paste_dropped"].cpu().numpy()
        _assert_bit_equal(got, want)
        assert np.array_equal(db["_paste_src"][4].cpu().numpy(), donor) and np.array_equal(db["_paste_src"][5].cpu().numpy(), select)
        accepted += int((want["gt_ids"] != 0).sum() - (first["gt_ids"] != 0).sum())
    assert accepted > 0                                             # the pasted batches carry more instances than the plain ones

    aug = Augmentation(seed=1, **FULL)
    _, seen0, l0 = run(augmentation=aug, copy_paste=CopyPaste(p=0.0, seed=5))
    _, seen1, l1 = run(augmentation=aug)
    print("per-step losses with CopyPaste(p=0): %r, with copy_paste=None: %r, with CopyPaste(p=1): %r" % (l0, l1, losses))
    assert "paste_dropped" in seen0[0] and "paste_dropped" not in seen1[0] and "_paste_src" not in seen1[0]
    for a, b in zip(seen0, seen1):
        for k in KEYS:
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert l0 == l1

    _, seen2, l2 = run(augmentation=aug, mosaic=Mosaic(p=1.0, seed=5), copy_paste=paste)
    assert np.all(np.isfinite(l2))
    for db in seen2:
        assert "mosaic_dropped" in db and len(db["_src"]) == 7
        want, (mid_ids, donor, select) = _check_second_stage(db, cfg)
        assert (donor != np.arange(4)).all()
    with pytest.raises(TypeError, match="myolo.augment.CopyPaste"):
        model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", copy_paste=object(), verbose=0)


def test_polygon_and_segment_routes_give_the_dense_routes_paste():
    """outlines of the Shapes instances (the box of each mask with one corner cut off) as one-part segments through the device route, counted once as
    a load_polygons dataset's and once as a load_segments dataset's batch, and their host fill through the dense route: the same plan, the same
    pasted batch -- with mosaic and augmentation in front, and without"""
    import torch
    from myolo.augment import Augmentation, CopyPaste, Mosaic
    from myolo.model import MaskYOLO
    from myolo.myolo_utils import BatchGenerator
    from myolo.polygon import polygon_mask
    from myolo.shapes import make_shapes_samples
    cfg = _small_cfg()
    samples = make_shapes_samples(4, cfg, seed=1234)
    dense, poly, seg = [], [], []
    tables = (np.arange(64, dtype=np.int32), np.arange(64, dtype=np.int32))
    for k, (image, class_ids, boxes, _) in enumerate(samples):
        outlines = [np.array([[y1, x1], [y1, x2], [(y1 + y2) / 2., x2], [y2, (x1 + x2) / 2.], [y2, x1]], np.float64) for x1, y1, x2, y2 in boxes]
        filled = np.stack([polygon_mask(o[:, 0], o[:, 1], (64, 64)) for o in outlines], axis=-1)
        assert filled.any(axis=(0, 1)).all()
        dense.append([image, class_ids, boxes, filled, 40 + k])
        poly.append([image, np.asarray(class_ids, np.int32), [[o] for o in outlines], tables, 40 + k, 64])
        seg.append([image, np.asarray(class_ids, np.int32), [[o] for o in outlines], tables, 40 + k, 64])
    model = MaskYOLO(mode="training", config=cfg)
    paste = CopyPaste(p=1.0, instances=1.0, seed=6)
    gen_d = BatchGenerator(dense, cfg, 'training', shuffle=False, norm=True)
    gen_p = BatchGenerator(poly, cfg, 'training', shuffle=False, norm=True)
    gen_s = BatchGenerator(seg, cfg, 'training', shuffle=False, norm=True)
    donor, select = model.paste_tables(paste, None, None, 3, [40, 41, 42, 43])
    assert (donor != np.arange(4)).all() and (select == (1 << cfg.TRUE_BOX_BUFFER) - 1).all()
    for n, (aug, mosaic) in enumerate(((Augmentation(seed=2, **FULL), Mosaic(seed=6)), (None, None))):
        a = model._augmented_batches(aug, None, None, gen_d, 'training', mosaic, copy_paste=paste)((3, 0))
        b = model._segment_batches(aug, None, None, gen_p, 'training', mosaic, counter="polygon_batches", copy_paste=paste)((3, 0))
        c = model._segment_batches(aug, None, None, gen_s, 'training', mosaic, copy_paste=paste)((3, 0))
        torch.cuda.synchronize()
        assert model.host_times["polygon_batches"] == model.host_times["segment_batches"] == n + 1
        for route, other in (("polygon", b), ("segment", c)):
            for k in KEYS + ("paste_dropped",) + (("mosaic_dropped",) if mosaic else ()):
                x, y = a[k].cpu().numpy(), other[k].cpu().numpy()
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (route, k, int((x != y).sum()))
        want, (mid_ids, got_donor, got_select) = _check_second_stage(a, cfg)
        assert np.array_equal(got_donor, donor) and np.array_equal(got_select, select)
        assert (want["gt_ids"] != 0).sum() > (mid_ids != 0).sum() and a["gt_masks"].cpu().numpy().any()

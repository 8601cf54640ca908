"""Mosaic on the device (myolo_mosaic_batch, csrc/augment_kernels.hip): against myolo_augment_batch where the two must agree (all-self tables),
against the numpy restatement of the contract (tests/mosaic_ref.py) through the C-ABI, on hand-made tile cases, through its refusals, and
through MaskYOLO.train(mosaic=...) on the dense and on the polygon route.  Every comparison is bit for bit."""
import numpy as np
import pytest

import augment_ref as R
import mosaic_ref as M

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
    """myolo_mosaic_batch on one set of operands, outputs pre-filled with values the kernels never write"""

    def __init__(self, images, masks, ids, quad_src, quad_rows, centre, cval=37.0):
        import torch
        from myolo import _ext as X
        self.X, self.torch = X, torch
        self.B, self.H, self.W, self.T = masks.shape
        self.cval = cval
        dev = torch.device("cuda:0")
        self.src = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
                    (images, masks, ids, quad_src.astype(np.int32), quad_rows, centre.astype(np.int32), ANCHORS)]
        B, H, W, T = self.B, self.H, self.W, self.T
        self.out = dict(images=torch.full((B, H, W, 3), -1., device=dev), gt_masks=torch.full((B, H, W, T), 9, dtype=torch.uint8, device=dev),
                        gt_boxes=torch.full((B, T, 4), -1, dtype=torch.int32, device=dev), gt_ids=torch.full((B, T), -1, dtype=torch.int32, device=dev),
                        y_true=torch.full((B, G, G, A, 5 + C), -1., device=dev), true_boxes=torch.full((B, T, 4), -1., device=dev),
                        dropped=torch.full((B,), -7, dtype=torch.int32, device=dev))
        self.ws = torch.empty(X.mosaic_ws_bytes(B, T), dtype=torch.uint8, device=dev)
        self.untouched = {k: v.cpu().numpy() for k, v in self.out.items()}

    def call(self, **kw):
        X, o, s = self.X, self.out, self.src
        a = dict(images=X.ptr(s[0]), quad_src=X.ptr(s[3]), dropped=X.ptr(o["dropped"]), T=self.T, ws_bytes=self.ws.numel())
        a.update(kw)
        return X.load().myolo_mosaic_batch(a["images"], X.ptr(s[1]), X.ptr(s[2]), a["quad_src"], X.ptr(s[4]), X.ptr(s[5]), self.cval, X.ptr(s[6]),
                                           X.ptr(o["images"]), X.ptr(o["gt_masks"]), X.ptr(o["gt_boxes"]), X.ptr(o["gt_ids"]), X.ptr(o["y_true"]),
                                           X.ptr(o["true_boxes"]), a["dropped"], self.B, self.H, self.W, a["T"], G, A, C,
                                           self.ws.data_ptr(), a["ws_bytes"], X.stream())

    def host(self):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def want(self):
        s = [t.cpu().numpy() for t in self.src]
        return M.mosaic_batch(s[0], s[1], s[2], s[3], s[4], s[5], self.cval, self.H, self.W, self.T, G, A, C, ANCHORS)


def _scene(B, H, W, T, seed):
    """random bytes; per image up to T rectangles in random slots (class ids 1..7), and set pixels in one slot whose class id stays 0"""
    rs = np.random.RandomState(seed)
    images = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    masks = np.zeros((B, H, W, T), np.uint8)
    ids = np.zeros((B, T), np.int32)
    for b in range(B):
        for t in range(T):
            y0, x0 = rs.randint(0, H - 4), rs.randint(0, W - 4)
            h, w = rs.randint(3, H // 2 + 1), rs.randint(3, W // 2 + 1)
            masks[b, y0:y0 + h, x0:x0 + w, t] = 1
            ids[b, t] = 1 + rs.randint(0, 7)
        if T >= 3:
            ids[b, rs.randint(0, T)] = 0                        # set pixels, no instance
    return images, masks, ids


def _tables(B, H, W, seed):
    """plans with the centres this file is about -- image 0 cut at (1,1), image 1 at (W-1,H-1), image 2 mid-frame, the others where the draw puts
    them -- composed with rows that rotate, flip and change the gain"""
    from myolo.augment import Augmentation, Mosaic
    image_ids = [100 + 3 * b for b in range(B)]
    plans = [Mosaic(seed=seed, centre=c).plan(1, image_ids, H, W) for c in ((0., 0.), (1., 1.), (.5, .5), (.25, .75))]
    pick = [min(b, 3) for b in range(B)]
    src, tiles, centre = [np.stack([plans[pick[b]][k][b] for b in range(B)]) for k in range(3)]
    assert centre[0].tolist() == [1, 1] and centre[1].tolist() == [W - 1, H - 1] and centre[2].tolist() == [(W + 1) // 2, (H + 1) // 2]
    aug = Augmentation(seed=seed, **FULL)
    assert any(aug.draw(1, i)["flip"] for i in image_ids) and all(aug.draw(1, i)["theta"] != 0 and aug.draw(1, i)["gain"] != 1 for i in image_ids)
    rows = np.stack([aug.params(1, i, H, W) for i in image_ids])
    return src, Mosaic.compose(tiles, src, rows), centre, rows


def test_all_self_tables_equal_augment_batch():
    """the required property: quad_src[b] = [b,b,b,b], quad_rows[b,q] = rows[b], centre (W, H) -> myolo_augment_batch byte for byte, nothing dropped"""
    from myolo.augment import Augmentation, DeviceAugmenter, Mosaic
    from myolo.config import ShapesConfig, make_config
    from myolo.shapes import make_shapes_samples
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=3)
    samples = make_shapes_samples(3, cfg, seed=1234)
    aug = Augmentation(seed=4, **FULL)
    rows = np.stack([aug.params(0, i, 64, 64) for i in range(3)])
    images, masks, ids = R.pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    dev = DeviceAugmenter(cfg, cval=aug.cval)
    want = {k: v.cpu().numpy() for k, v in dev.apply(images, masks, ids, rows).items() if k in KEYS}
    src, tiles, centre = Mosaic(p=0.0).plan(0, [0, 1, 2], 64, 64)
    assert centre.tolist() == [[64, 64]] * 3
    d = dev.apply(images, masks, ids, rows, mosaic=(src, Mosaic.compose(tiles, src, rows), centre))
    got = {k: v.cpu().numpy() for k, v in d.items() if k in KEYS}
    assert (want["gt_ids"] != 0).sum() >= 3
    _assert_bit_equal(got, want, keys=KEYS)
    assert d["mosaic_dropped"].cpu().numpy().tolist() == [0, 0, 0]
    # and with the device arithmetic restated
    _assert_bit_equal(got, R.augment_cfg_batch(samples, rows, cfg, cval=aug.cval), keys=KEYS)


@pytest.mark.parametrize("H,W,B,T", [(64, 64, 3, 3), (96, 96, 5, 4), (37, 91, 3, 3), (64, 64, 3, 1), (64, 64, 5, 32), (37, 91, 5, 4), (96, 96, 3, 2)])
def test_entry_equals_the_restatement(H, W, B, T):
    """through the C-ABI: 64 x 64 and 96 x 96 (several workgroups per image), 37 x 91 (3367 pixels: a ragged last workgroup, mask bytes per image no
    multiple of four with T = 3), B = 3 (partners repeat) and 5, T = 1 / 3 (byte loads), 2 (two bytes), 4 / 32 (words); G = 2 independent of the frame.
    Two calls give the same bytes."""
    images, masks, ids = _scene(B, H, W, T, seed=H + T)
    src, quad_rows, centre, _ = _tables(B, H, W, seed=11)
    assert any(len(set(s.tolist())) < 4 for s in src)           # an image in two tiles of one sample
    e = Entry(images, masks, ids, src, quad_rows, centre)
    want = e.want()
    if T == 32:
        assert want["dropped"].max() > 0                        # more survivors than slots
    if T == 3:
        assert (want["gt_ids"] != 0).sum() >= B
    assert e.call() == 0
    got = e.host()
    _assert_bit_equal(got, want)
    for o in e.out.values():
        o.fill_(3)
    assert e.call() == 0
    _assert_bit_equal(e.host(), got)


def test_tile_cases_by_hand():
    """64 x 64, T = 4, the cut at (32, 32), pure translations as tile rows, so that every expected box can be written down:
    tile 0 shows image 0 shifted by (10, 10): its instance A is cut by both tile edges (box clipped at the cut), its instance B lies wholly outside;
    tiles 1 and 2 both show the top-left quadrant of image 1: its one instance comes out twice, as two distinct instances;
    tile 3 shows image 2 in place: one instance, and a slot with set pixels whose class id is 0."""
    H = W = 64
    T = 4
    rs = np.random.RandomState(3)
    images = rs.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    masks = np.zeros((3, H, W, T), np.uint8)
    ids = np.zeros((3, T), np.int32)
    masks[0, 20:50, 30:60, 0], ids[0, 0] = 1, 5                 # A
    masks[0, 50:60, 12:20, 1], ids[0, 1] = 1, 6                 # B: below the cut in tile 0's frame, where tile 2 shows image 1
    masks[1, 4:20, 6:28, 0], ids[1, 0] = 1, 2
    masks[2, 40:50, 40:56, 2], ids[2, 2] = 1, 3
    masks[2, 34:60, 34:60, 0] = 1                               # class id 0: no instance
    shift = lambda tx, ty: [1., 0., tx, 0., 1., ty, 1., 0.]     # noqa: E731
    quad_src = np.array([[0, 1, 1, 2], [1, 1, 1, 1], [2, 2, 2, 2]], np.int32)
    quad_rows = np.array([[shift(10, 10), shift(-32, 0), shift(0, -32), shift(0, 0)]] + [[shift(0, 0)] * 4] * 2, np.float64)
    centre = np.array([[32, 32], [64, 64], [64, 64]], np.int32)
    e = Entry(images, masks, ids, quad_src, quad_rows, centre)
    assert e.call() == 0
    got = e.host()
    _assert_bit_equal(got, e.want())
    assert got["gt_ids"][0].tolist() == [5, 2, 2, 3] and got["dropped"].tolist() == [0, 0, 0]
    assert got["gt_boxes"][0].tolist() == [[20, 10, 32, 32], [38, 4, 60, 20], [6, 36, 28, 52], [40, 40, 56, 50]]
    m = got["gt_masks"][0]
    assert m[:, :, 0].sum() == 12 * 22 and m[:, :, 1].sum() == m[:, :, 2].sum() == 16 * 22 and m[:, :, 3].sum() == 10 * 16
    assert not m[32:, :, 0].any() and not m[:, 32:, 0].any() and not m[32:, :, 1].any() and not m[:32, :, 2].any()
    # the image: each tile's bytes, from its own source
    img = got["images"][0]
    assert img[0:32, 0:32].tobytes() == (images[0, 10:42, 10:42] / 255.).astype(np.float32).tobytes()
    assert img[0:32, 32:64].tobytes() == (images[1, 0:32, 0:32] / 255.).astype(np.float32).tobytes()
    assert img[32:64, 0:32].tobytes() == (images[1, 0:32, 0:32] / 255.).astype(np.float32).tobytes()
    assert img[32:64, 32:64].tobytes() == (images[2, 32:64, 32:64] / 255.).astype(np.float32).tobytes()
    # images 1 and 2 are not mosaicked: themselves
    assert got["gt_ids"][1].tolist() == [2, 0, 0, 0] and got["gt_boxes"][1, 0].tolist() == [6, 4, 28, 20]
    assert got["gt_ids"][2].tolist() == [3, 0, 0, 0] and got["gt_boxes"][2, 0].tolist() == [40, 40, 56, 50]


def test_more_survivors_than_slots():
    """T = 4, four source images whose four instances each reach every tile (instance t = the pixels with (x + y) % 4 == t): 16 survivors, the
    four of tile 0 keep their order, 12 are counted, and no mask holds a pixel outside tile 0"""
    H = W = 64
    T = B = 4
    rs = np.random.RandomState(8)
    images = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.stack([np.stack([((xx + yy + b) % 4 == t) for t in range(T)], axis=-1) for b in range(B)]).astype(np.uint8)
    ids = np.array([[1 + (4 * b + t) % 7 for t in range(T)] for b in range(B)], np.int32)
    quad_src = np.array([[0, 1, 2, 3], [1, 1, 0, 2], [2, 3, 3, 0], [3, 3, 3, 3]], np.int32)
    quad_rows = np.tile(np.array([1., 0., 0., 0., 1., 0., 1., 0.]), (B, 4, 1))
    centre = np.array([[32, 32], [1, 1], [63, 63], [64, 64]], np.int32)
    e = Entry(images, masks, ids, quad_src, quad_rows, centre)
    assert e.call() == 0
    got = e.host()
    _assert_bit_equal(got, e.want())
    # image 1: tile 0 is the one pixel (0, 0), where only instance (0 + 0 + 1) % 4 = 1 of image 1 is set; tile 1 gives the next three slots
    # image 2: tile 3 is the one pixel (63, 63), where only instance (63 + 63 + 0) % 4 = 2 of image 0 is set: 4 + 4 + 4 + 1 survivors
    assert got["dropped"].tolist() == [12, 9, 9, 0]
    for b in (0, 2, 3):
        assert got["gt_ids"][b].tolist() == ids[quad_src[b, 0]].tolist()          # tile 0's candidates come first
    assert got["gt_ids"][1].tolist() == [ids[1, 1], ids[1, 0], ids[1, 1], ids[1, 2]]
    cx, cy = 32, 32
    assert got["gt_masks"][0][:cy, :cx].sum() == cx * cy and not got["gt_masks"][0][cy:].any() and not got["gt_masks"][0][:, cx:].any()
    assert got["gt_masks"][1][:, :, 0].sum() == 1 and got["gt_masks"][1][0, 0, 0] == 1 and not got["gt_masks"][1][1:].any()     # (tile 1 is row 0)
    assert got["gt_boxes"][0].tolist() == [[0, 0, 32, 32]] * 4


def test_refusals_write_nothing():
    images, masks, ids = _scene(3, 64, 64, 3, seed=1)
    src, quad_rows, centre, _ = _tables(3, 64, 64, seed=11)
    e = Entry(images, masks, ids, src, quad_rows, centre)
    err = e.X.load().myolo_last_error_string
    for kw in (dict(images=None), dict(quad_src=None), dict(dropped=None), dict(T=33), dict(ws_bytes=e.ws.numel() - 4), dict(ws_bytes=0)):
        assert e.call(**kw) == -1, kw
        assert err().startswith(b"mosaic_batch:"), (kw, err())
    assert b"T" in (e.call(T=33), err())[1] and b"workspace" in (e.call(ws_bytes=8), err())[1]
    _assert_bit_equal(e.host(), e.untouched)
    # sources outside the batch and centres outside the frame are refused before anything is uploaded
    from myolo.augment import DeviceAugmenter
    from myolo.config import ShapesConfig, make_config
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=3)
    T = cfg.TRUE_BOX_BUFFER
    dev = DeviceAugmenter(cfg)
    args = (images, np.zeros((3, 64, 64, T), np.uint8), np.zeros((3, T), np.int32), np.tile(np.array([1., 0, 0, 0, 1, 0, 1, 0]), (3, 1)))
    for bad_src, bad_centre in ((np.where(src == 2, 3, src), centre), (-src - 1, centre), (src, centre + 64), (src, -centre)):
        with pytest.raises(ValueError, match="mosaic tables"):
            dev.apply(*args, mosaic=(bad_src, quad_rows, bad_centre))


def _small_cfg():
    from myolo.config import ShapesConfig, make_config
    return make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], ALPHA=0.5, BATCH_SIZE=4)


def test_train_end_to_end_with_mosaic():
    """train(mosaic=Mosaic(p=1.0)) on the dense route: finite losses, and the step received the restatement's boxes for the tables planned from
    the batch's image ids; Mosaic(p=0.0) trains exactly as mosaic=None does under the same augmentation"""
    from myolo.augment import Augmentation, Mosaic
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

    mosaic = Mosaic(p=1.0, seed=5)
    model, seen, losses = run(mosaic=mosaic)
    assert np.all(np.isfinite(losses))
    mosaicked = 0
    for db in seen:
        raw, masks, ids, rows, quad_src, quad_rows, centre = [t.cpu().numpy() for t in db["_src"]]
        image_ids = [by_bytes[raw[b].tobytes()] for b in range(4)]
        src, tiles, cen = model.mosaic_tables(mosaic, None, ds, 0, image_ids)
        assert np.array_equal(rows, np.tile([1., 0, 0, 0, 1, 0, 1, 0], (4, 1)))                 # no augmentation: identity rows
        assert np.array_equal(quad_src, src) and np.array_equal(centre, cen) and quad_rows.tobytes() == Mosaic.compose(tiles, src, rows).tobytes()
        assert (cen != 64).all()
        want = M.mosaic_batch(raw, masks, ids, src, quad_rows, cen, 0.0, 64, 64, T, cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES,
                              np.asarray(cfg.ANCHORS, np.float64))
        got = {k: db[k].cpu().numpy() for k in KEYS}
        got["dropped"] = db["mosaic_dropped"].cpu().numpy()
        _assert_bit_equal(got, want)
        mosaicked += int((want["gt_ids"] != 0).sum())
    assert mosaicked >= 8

    aug = Augmentation(seed=1, **FULL)
    _, seen0, l0 = run(augmentation=aug, mosaic=Mosaic(p=0.0, seed=5))
    _, seen1, l1 = run(augmentation=aug)
    print("per-step losses with Mosaic(p=0): %r, with mosaic=None: %r, with Mosaic(p=1): %r" % (l0, l1, losses))
    assert "mosaic_dropped" in seen0[0] and "mosaic_dropped" not in seen1[0]
    for a, b in zip(seen0, seen1):
        for k in KEYS:
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert l0 == l1
    with pytest.raises(TypeError, match="myolo.augment.Mosaic"):
        model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", mosaic=object(), verbose=0)


def test_polygon_and_segment_routes_give_the_dense_routes_mosaic():
    """outlines of the Shapes instances (the box of each mask with one corner cut off) as one-part segments through the device route, counted once as
    a load_polygons dataset's and once as a load_segments dataset's batch, and their host fill through the dense route: the same plan, the same
    mosaicked batch"""
    import torch
    from myolo.augment import Augmentation, Mosaic
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
    aug, mosaic = Augmentation(seed=2, **FULL), Mosaic(seed=6)
    gen_d = BatchGenerator(dense, cfg, 'training', shuffle=False, norm=True)
    gen_p = BatchGenerator(poly, cfg, 'training', shuffle=False, norm=True)
    a = model._augmented_batches(aug, None, None, gen_d, 'training', mosaic)((3, 0))
    b = model._segment_batches(aug, None, None, gen_p, 'training', mosaic, counter="polygon_batches")((3, 0))
    c = model._segment_batches(aug, None, None, BatchGenerator(seg, cfg, 'training', shuffle=False, norm=True), 'training', mosaic)((3, 0))
    torch.cuda.synchronize()
    assert (a["_src"][6].cpu().numpy() != 64).all()             # every sample is mosaicked
    assert model.host_times["polygon_batches"] == model.host_times["segment_batches"] == 1
    for route, other in (("polygon", b), ("segment", c)):
        for k in KEYS + ("mosaic_dropped",):
            x, y = a[k].cpu().numpy(), other[k].cpu().numpy()
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (route, k, int((x != y).sum()))
    assert (a["gt_ids"].cpu().numpy() != 0).sum() >= 4 and a["gt_masks"].cpu().numpy().any()
    src, _, centre = model.mosaic_tables(mosaic, None, None, 3, [40, 41, 42, 43])
    assert np.array_equal(a["_src"][4].cpu().numpy(), src) and np.array_equal(a["_src"][6].cpu().numpy(), centre)

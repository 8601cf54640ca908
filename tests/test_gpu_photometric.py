"""Photometric augmentation on the device (myolo_photometric_batch, csrc/photometric_kernels.hip): against the numpy restatement of the contract
(tests/photometric_ref.py) through the C-ABI, on small frames where the reflection wraps, on identity rows, under the caller's radius bound, on
cases made by hand, through its refusals, behind each first stage of DeviceAugmenter.apply and through MaskYOLO.train(photometric=...) on the
dense, polygon and segment routes.  Every comparison is bit for bit unless it says otherwise."""
import numpy as np
import pytest

import augment_ref as R
import photometric_ref as PR

pytestmark = pytest.mark.gpu

FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))
WIDE = dict(hue=(-40, 40), saturation=(.5, 1.5), contrast=(.6, 1.4), blur=(0.4, 2.), noise=(0.01, .1))
KEYS = ("images", "true_boxes", "y_true", "gt_ids", "gt_boxes", "gt_masks")


def _row(hue=0., saturation=1., contrast=1., sigma=0., std=0., key=0):
    from myolo.augment import Photometric
    row = Photometric.identity()
    row[0:12] = Photometric.matrix(hue, saturation, contrast).reshape(-1)
    row[12], row[13] = std, key
    r, w = Photometric.kernel(sigma)
    row[14], row[16:32] = r, w
    return row


KINDS = ("identity", "colour only", "blur r = 1", "blur r = 15", "noise only", "everything at once")


def _kinds():
    kinds = [_row(), _row(hue=35., saturation=1.4, contrast=0.7), _row(sigma=0.3), _row(sigma=5.0), _row(std=0.08, key=12345),
             _row(hue=-100., saturation=0.3, contrast=1.5, sigma=1.7, std=0.05, key=2 ** 32 - 1)]
    assert [int(k[14]) for k in kinds] == [0, 0, 1, 15, 0, 6] and [k[12] > 0 for k in kinds] == [False] * 4 + [True] * 2
    assert (kinds[4][0:12] == kinds[0][0:12]).all() and kinds[4][16] == 1.0          # noise only: identity colour, no blur
    return kinds


def _row_sets(B):
    """-> (kind indices, rows [B,32]) for as many calls as it takes to show a shape of batch B all six KINDS: call n holds kinds n*B .. n*B+B-1
    (mod 6), so B = 3 makes two calls, B = 4 two (the second wraps to identity and colour only), B = 1 six"""
    kinds = _kinds()
    sets = []
    for n in range(-(-6 // B)):
        idx = [(n * B + b) % 6 for b in range(B)]
        sets.append((idx, np.stack([kinds[i] for i in idx])))
    assert sorted(set(i for idx, _ in sets for i in idx)) == list(range(6))
    return sets


def _rows(B):
    """the first B of KINDS, cycled"""
    kinds = _kinds()
    return np.stack([kinds[b % 6] for b in range(B)])


class Entry(object):
    """myolo_photometric_batch on one set of operands, the output pre-filled with a value the kernels never write"""

    def __init__(self, images, rows, max_radius=15):
        import torch
        from myolo import _ext as X
        self.X, self.torch = X, torch
        self.B, self.H, self.W = images.shape[:3]
        self.max_radius = max_radius
        dev = torch.device("cuda:0")
        self.host_src = (np.ascontiguousarray(images, np.float32), np.ascontiguousarray(rows, np.float64))
        self.src = [torch.from_numpy(a).to(dev) for a in self.host_src]
        self.out = torch.full((self.B, self.H, self.W, 3), -1., device=dev)
        self.ws = torch.empty(max(X.photometric_ws_bytes(self.B, self.H, self.W, max_radius), 8), dtype=torch.uint8, device=dev)
        self.ws_bytes = X.photometric_ws_bytes(self.B, self.H, self.W, max_radius)

    def call(self, **kw):
        X, s = self.X, self.src
        a = dict(src=X.ptr(s[0]), rows=X.ptr(s[1]), out=X.ptr(self.out), max_radius=self.max_radius, B=self.B, H=self.H, W=self.W,
                 ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(kw)
        return X.load().myolo_photometric_batch(a["src"], a["rows"], a["out"], a["max_radius"], a["B"], a["H"], a["W"], a["ws"], a["ws_bytes"],
                                                X.stream())

    def host(self):
        self.torch.cuda.synchronize()
        return self.out.cpu().numpy()

    def want(self, max_radius=None):
        return PR.photometric_batch(self.host_src[0], self.host_src[1], self.max_radius if max_radius is None else max_radius)


def _images(B, H, W, seed):
    """floats in [0, 1] as the earlier stages write them: random, with exact zeros and ones among them"""
    rs = np.random.RandomState(seed)
    images = rs.random_sample((B, H, W, 3)).astype(np.float32)
    images[rs.random_sample((B, H, W, 3)) < 0.05] = 0.0
    images[rs.random_sample((B, H, W, 3)) < 0.05] = 1.0
    return images


def _assert_same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want).max()))


@pytest.mark.parametrize("H,W,B", [(37, 29, 3), (64, 64, 1), (64, 64, 3), (224, 224, 4)])
def test_entry_equals_the_restatement(H, W, B):
    """through the C-ABI: 37 x 29 (1073 pixels, 3219 floats: a ragged last workgroup in both passes), 64 x 64 (several workgroups per image) with one
    image and three, 224 x 224 with four.  Every shape sees all six KINDS of row -- identity, colour only, blur with r = 1 and with r = 15, noise
    only, everything at once -- over as many calls as its batch needs (_row_sets).  Each call is repeated into an output pre-filled with 3 and
    over a workspace filled with ones: two calls give the same bytes."""
    images = _images(B, H, W, seed=1)
    seen = set()
    for idx, rows in _row_sets(B):
        e = Entry(images, rows)
        want = e.want()
        assert e.call() == 0
        got = e.host()
        _assert_same_bits(got, want, [KINDS[i] for i in idx])
        assert got.min() >= 0.0 and got.max() <= 1.0
        for b, i in enumerate(idx):                              # every kind but the identity changes its image
            assert np.array_equal(got[b], images[b]) == (i == 0), KINDS[i]
        e.out.fill_(3)
        e.ws.fill_(255)
        assert e.call() == 0
        _assert_same_bits(e.host(), got, "second call")
        seen.update(idx)
    assert seen == set(range(6))


@pytest.mark.parametrize("H,W", [(5, 3), (1, 1), (2, 1), (1, 2)])
def test_small_frames_where_the_reflection_wraps(H, W):
    """r = 15 on frames smaller than the radius: refl wraps several times (and is 0 on a side of one pixel)"""
    rows = np.stack([_row(sigma=5.0), _row(hue=20., contrast=1.2, sigma=5.0, std=0.02, key=7)])
    e = Entry(_images(2, H, W, seed=2), rows)
    assert e.call() == 0
    _assert_same_bits(e.host(), e.want())


@pytest.mark.parametrize("max_radius", [0, 15])
def test_identity_rows_return_the_inputs_bits(max_radius):
    from myolo.augment import Photometric
    images = _images(3, 37, 29, seed=3)
    images[0, 0, 0] = (0.0, 1.0, 1e-40)                         # a denormal too
    e = Entry(images, np.tile(Photometric.identity(), (3, 1)), max_radius=max_radius)
    assert e.ws_bytes == (0 if max_radius == 0 else 3 * 37 * 29 * 3 * 8)
    assert e.call(**(dict(ws=None) if max_radius == 0 else {})) == 0
    _assert_same_bits(e.host(), images)


def test_the_callers_bound_clamps_a_rows_radius():
    """a row with r = 15 under max_radius = 4: the loops stop at 4, the weights stay the row's"""
    rows = np.stack([_row(sigma=5.0), _row(sigma=0.6), _row(hue=10., sigma=5.0, std=0.01, key=3)])
    assert rows[:, 14].tolist() == [15, 2, 15]
    e = Entry(_images(3, 37, 29, seed=4), rows, max_radius=4)
    assert e.call() == 0
    got = e.host()
    clamped = rows.copy()
    clamped[:, 14] = np.minimum(clamped[:, 14], 4)
    _assert_same_bits(got, PR.photometric_batch(e.host_src[0], clamped, 15))
    _assert_same_bits(got, e.want())
    assert not np.array_equal(got, e.want(max_radius=15))
    # and with max_radius = 0 no blur at all: w_0 alone, twice
    e0 = Entry(e.host_src[0], rows, max_radius=0)
    assert e0.call(ws=None, ws_bytes=0) == 0
    _assert_same_bits(e0.host(), e0.want())


def test_cases_by_hand():
    from myolo.augment import Photometric
    # a single white pixel on black with r = 1 spreads as the outer product of (w1, w0, w1)
    r, w = Photometric.kernel(0.3)
    assert r == 1
    point = np.zeros((1, 9, 9, 3), np.float32)
    point[0, 4, 4] = 1.0
    e = Entry(point, _row(sigma=0.3)[None])
    assert e.call() == 0
    got = e.host()[0]
    k = np.array([w[1], w[0], w[1]])
    want = np.zeros((9, 9, 3), np.float32)
    want[3:6, 3:6] = np.outer(k, k).astype(np.float32)[:, :, None]
    _assert_same_bits(got, want)
    # a pure-red image under a hue of 120 degrees becomes pure green within 1 ulp of the float
    red = np.zeros((1, 8, 8, 3), np.float32)
    red[..., 0] = 1.0
    e = Entry(red, _row(hue=120.)[None])
    assert e.call() == 0
    got = e.host()[0]
    ulp = float(np.spacing(np.float32(1.0)))
    assert np.abs(got - np.array([0., 1., 0.], np.float32)).max() <= ulp, got[0, 0]


def test_refusals_write_nothing():
    e = Entry(_images(3, 64, 64, seed=5), _rows(3))
    X, s = e.X, e.src
    err = X.load().myolo_last_error_string
    n = 64 * 64 * 3 * 4
    for kw in (dict(src=None), dict(rows=None), dict(out=None), dict(ws=None), dict(B=0), dict(H=0), dict(W=-1), dict(max_radius=16), dict(max_radius=-1),
               dict(out=X.ptr(s[0])), dict(out=X.ptr(s[0]) + 2 * n), dict(out=X.ptr(s[0]) - n + 4, B=1), dict(ws_bytes=e.ws_bytes - 8), dict(ws_bytes=0)):
        assert e.call(**kw) == -1, kw
        assert err().startswith(b"photometric_batch:"), (kw, err())
    assert b"max_radius" in (e.call(max_radius=16), err())[1] and b"workspace" in (e.call(ws_bytes=8), err())[1]
    assert b"null" in (e.call(rows=None), err())[1] and b"lies over" in (e.call(out=X.ptr(s[0])), err())[1] and b"sizes" in (e.call(H=0), err())[1]
    got = e.host()
    assert (got == -1.0).all()
    assert e.call() == 0                                            # and the same operands, unrefused, run
    _assert_same_bits(e.host(), e.want())


def _small_cfg(B=4):
    from myolo.config import ShapesConfig, make_config
    return make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], ALPHA=0.5, BATCH_SIZE=B)


@pytest.mark.parametrize("first", ["warp", "mosaic", "warp+copy_paste"])
def test_apply_runs_the_stage_behind_each_first_stage(first):
    """DeviceAugmenter.apply(..., photometric=rows) at 64 x 64, B = 3: images are the restatement's of the same call's images without photometric,
    the other five arrays are that call's byte for byte"""
    from myolo.augment import Augmentation, DeviceAugmenter, Mosaic, Photometric
    from myolo.shapes import make_shapes_samples
    cfg = _small_cfg(3)
    samples = make_shapes_samples(3, cfg, seed=1234)
    aug = Augmentation(seed=4, **FULL)
    params = np.stack([aug.params(0, i, 64, 64) for i in range(3)])
    images, masks, ids = R.pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    kw = {}
    if first == "mosaic":
        src, tiles, centre = Mosaic(seed=2).plan(0, [0, 1, 2], 64, 64)
        kw["mosaic"] = (src, Mosaic.compose(tiles, src, params), centre)
    if first == "warp+copy_paste":
        kw["copy_paste"] = (np.array([1, 2, 0], np.int32), np.full(3, (1 << cfg.TRUE_BOX_BUFFER) - 1, np.int32))
    photo = Photometric(seed=9, **WIDE)
    rows = np.stack([photo.row(0, 0), Photometric.identity(), photo.row(0, 2)])
    dev = DeviceAugmenter(cfg, cval=aug.cval)
    plain = dev.apply(images, masks, ids, params, **kw)
    assert "_photo_src" not in plain
    want = {k: plain[k].cpu().numpy() for k in KEYS}
    for photometric in (rows, (rows, 15)):
        d = dev.apply(images, masks, ids, params, photometric=photometric, **kw)
        got = {k: d[k].cpu().numpy() for k in KEYS}
        _assert_same_bits(d["_photo_src"][0].cpu().numpy(), want["images"], "the stage's input")
        _assert_same_bits(got["images"], PR.photometric_batch(want["images"], rows), "images")
        _assert_same_bits(got["images"][1], want["images"][1], "identity row")
        assert not np.array_equal(got["images"][0], want["images"][0])
        for k in KEYS[1:]:
            _assert_same_bits(got[k], want[k], k)
    # the 'yolo' form of the dict carries the same image
    y = dev.apply(images, masks, ids, params, yolo=True, photometric=rows, **kw)
    _assert_same_bits(y["images"].cpu().numpy(), got["images"], "yolo")
    # rows are checked before anything is uploaded
    bad = rows.copy()
    bad[1, 14] = 16
    with pytest.raises(ValueError, match="photometric rows"):
        dev.apply(images, masks, ids, params, photometric=bad, **kw)
    with pytest.raises(ValueError, match="max_radius"):
        dev.apply(images, masks, ids, params, photometric=(rows, 16), **kw)


def test_train_end_to_end_with_photometric():
    """train(photometric=Photometric(...)) on the dense route of the 64 x 64 Shapes config: finite losses; the batches the steps consumed are the
    restatement's on photometric_rows of the batch's image ids, applied to the first stage's image, every other array the first stage's; samples of
    a no_augmentation_sources source are untouched: the run is the one without photometric, loss for loss; validation batches are the ones a run
    without photometric evaluates"""
    from myolo.augment import Augmentation, Photometric
    from myolo.model import MaskYOLO
    from myolo.shapes import ShapesDataset
    cfg = _small_cfg()
    T = cfg.TRUE_BOX_BUFFER
    ds = ShapesDataset(1234)
    ds.load_shapes(8, 64, 64)
    ds.prepare()
    val = ShapesDataset(99)
    val.load_shapes(4, 64, 64)
    val.prepare()
    by_bytes = {ds.load_image(i).astype(np.uint8).tobytes(): int(i) for i in ds.image_ids}
    assert len(by_bytes) == 8
    anchors = np.asarray(cfg.ANCHORS, np.float64)

    def run(**kw):
        model = MaskYOLO(mode="training", config=cfg, seed=3)
        seen, outs, vseen = [], [], []
        step, evaluate = model.train_on_batch, model.evaluate_on_batch

        def spy(db, *a, **k):
            seen.append(db)
            outs.append(step(db, *a, **k))
            return outs[-1]

        def vspy(batch, *a, **k):
            vseen.append([np.array(x, copy=True) for x in batch])
            return evaluate(batch, *a, **k)
        model.train_on_batch, model.evaluate_on_batch = spy, vspy
        hist = model.train(ds, val, learning_rate=1e-3, epochs=1, layers="all", max_samples=8, verbose=0, **kw)
        assert len(hist) == 1 and np.all(np.isfinite(hist)) and len(seen) == 2 and len(vseen) == 1
        assert np.all(np.isfinite(model.history["val_loss"]))
        return model, seen, [o["loss"] for o in outs], vseen[0]

    photo = Photometric(seed=5, **WIDE)
    assert photo.max_radius == 6
    model, seen, losses, vseen = run(photometric=photo)
    assert np.all(np.isfinite(losses))
    for db in seen:
        raw, masks, ids, params = [t.cpu().numpy() for t in db["_src"]]
        image_ids = [by_bytes[raw[b].tobytes()] for b in range(4)]
        rows = model.photometric_rows(photo, None, ds, 0, image_ids)
        assert np.array_equal(params, np.tile([1., 0, 0, 0, 1, 0, 1, 0], (4, 1)))               # no augmentation: identity warp rows
        assert np.array_equal(db["_photo_src"][1].cpu().numpy(), rows) and (rows[:, 14] >= 1).all() and (rows[:, 12] > 0).all()
        first = R.augment_batch(raw, masks, ids, params, 0.0, 64, 64, T, cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES, anchors)
        _assert_same_bits(db["images"].cpu().numpy(), PR.photometric_batch(first["images"], rows, photo.max_radius), "images")
        for k in KEYS[1:]:
            _assert_same_bits(db[k].cpu().numpy(), first[k], k)

    # samples of a listed source get the identity row and keep their pixels: behind an augmentation, the run without photometric
    skip = [ds.image_info[0]["source"]]
    assert all(ds.image_info[i]["source"] in skip for i in ds.image_ids)
    rows = model.photometric_rows(photo, skip, ds, 0, list(ds.image_ids))
    assert all(r.tobytes() == Photometric.identity().tobytes() for r in rows)
    aug = Augmentation(seed=1, **FULL)
    _, seen_skip, l_skip, v_skip = run(augmentation=aug, photometric=photo, no_augmentation_sources=skip)
    _, seen_none, l_none, v_none = run(augmentation=aug, no_augmentation_sources=skip)
    print("per-step losses with photometric %r; with every sample's source listed %r, without photometric %r" % (losses, l_skip, l_none))
    assert "_photo_src" in seen_skip[0] and "_photo_src" not in seen_none[0]
    for a, b in zip(seen_skip, seen_none):
        for k in KEYS:
            _assert_same_bits(a[k].cpu().numpy(), b[k].cpu().numpy(), k)
    assert l_skip == l_none

    # validation batches are never touched: array for array those of the run without photometric
    for other in (vseen, v_skip):
        assert len(other) == len(v_none)
        for x, y in zip(other, v_none):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()

    with pytest.raises(TypeError, match="myolo.augment.Photometric"):
        model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", photometric=object(), verbose=0)
    with pytest.raises(TypeError):
        model.train(ds, None, 1e-3, 1, "all", None, None, None, None, 0, 0, True, None, photo)      # keyword only


def test_polygon_and_segment_routes_give_the_dense_routes_images():
    """outlines of the Shapes instances as one-part segments through the device route, counted once as a load_polygons dataset's and once as a
    load_segments dataset's batch, and their host fill through the dense route: the same rows, the same batch -- with augmentation, mosaic and
    copy-paste in front, and with nothing in front"""
    import torch
    from myolo.augment import Augmentation, CopyPaste, Mosaic, Photometric
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
        dense.append([image, class_ids, boxes, filled, 40 + k])
        poly.append([image, np.asarray(class_ids, np.int32), [[o] for o in outlines], tables, 40 + k, 64])
        seg.append([image, np.asarray(class_ids, np.int32), [[o] for o in outlines], tables, 40 + k, 64])
    model = MaskYOLO(mode="training", config=cfg)
    photo = Photometric(seed=6, **WIDE)
    gen_d = BatchGenerator(dense, cfg, 'training', shuffle=False, norm=True)
    gen_p = BatchGenerator(poly, cfg, 'training', shuffle=False, norm=True)
    gen_s = BatchGenerator(seg, cfg, 'training', shuffle=False, norm=True)
    rows = model.photometric_rows(photo, None, None, 3, [40, 41, 42, 43])
    for n, (aug, mosaic, paste) in enumerate(((Augmentation(seed=2, **FULL), Mosaic(seed=6), CopyPaste(p=1.0, instances=1.0, seed=6)), (None, None, None))):
        a = model._augmented_batches(aug, None, None, gen_d, 'training', mosaic, copy_paste=paste, photometric=photo)((3, 0))
        b = model._segment_batches(aug, None, None, gen_p, 'training', mosaic, counter="polygon_batches", copy_paste=paste, photometric=photo)((3, 0))
        c = model._segment_batches(aug, None, None, gen_s, 'training', mosaic, copy_paste=paste, photometric=photo)((3, 0))
        torch.cuda.synchronize()
        assert model.host_times["polygon_batches"] == model.host_times["segment_batches"] == n + 1
        for route, other in (("polygon", b), ("segment", c)):
            for k in KEYS:
                _assert_same_bits(other[k].cpu().numpy(), a[k].cpu().numpy(), (route, k))
        assert np.array_equal(a["_photo_src"][1].cpu().numpy(), rows)
        _assert_same_bits(a["images"].cpu().numpy(), PR.photometric_batch(a["_photo_src"][0].cpu().numpy(), rows, photo.max_radius), "images")
        assert not np.array_equal(a["images"].cpu().numpy(), a["_photo_src"][0].cpu().numpy())

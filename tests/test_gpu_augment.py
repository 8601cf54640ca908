"""On-device augmentation (csrc/augment_kernels.hip through myolo.augment.DeviceAugmenter) against the host pipeline where the two must agree
(identity rows), against the reference's own flip output (tests/golden/ref_load_image_gt.npz), against the numpy restatement of the arithmetic
contract (tests/augment_ref.py) bit for bit on general transforms, and through the training step and MaskYOLO.train()."""
import os

import numpy as np
import pytest

import augment_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))
KEYS = ("images", "true_boxes", "y_true", "gt_ids", "gt_boxes", "gt_masks")


def _host(d):
    return {k: d[k].cpu().numpy() for k in KEYS if k in d}


def _assert_bit_equal(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))


def test_identity_rows_equal_the_host_pipeline():
    from myolo.augment import DeviceAugmenter, IDENTITY_ROW
    from myolo.config import ShapesConfig, make_config
    from myolo.myolo_utils import BatchGenerator
    from myolo.shapes import make_shapes_samples
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[96, 96, 3], BATCH_SIZE=8)
    assert cfg.GRID_W == 3
    samples = make_shapes_samples(8, cfg)
    want = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0][0]
    images, masks, ids = R.pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    got = _host(DeviceAugmenter(cfg).apply(images, masks, ids, np.tile(IDENTITY_ROW, (8, 1))))
    assert got["images"].dtype == np.float32 and got["images"].tobytes() == want[0].tobytes()
    np.testing.assert_array_equal(got["true_boxes"], want[1].reshape(8, -1, 4).astype(np.float32))
    np.testing.assert_array_equal(got["y_true"], want[2].astype(np.float32))
    np.testing.assert_array_equal(got["gt_ids"], want[3])
    np.testing.assert_array_equal(got["gt_boxes"], want[4])
    np.testing.assert_array_equal(got["gt_masks"], want[5].astype(np.uint8))


def test_flip_rows_equal_the_reference_output():
    """the reference's load_image_gt(augment=True) on 24 Shapes images at 224 x 224, 12 of them flipped: its image, masks, boxes and class ids."""
    from myolo.augment import Augmentation, DeviceAugmenter, IDENTITY_ROW
    from myolo.config import ShapesConfig
    from myolo.myolo_utils import load_image_gt
    from myolo.shapes import ShapesDataset
    fx = np.load(os.path.join(GOLDEN, "ref_load_image_gt.npz"), allow_pickle=False)
    h, w, start = [int(v) for v in fx["flip_hw_start"]]
    counts, drawn = fx["flip_counts"], fx["flip_drawn"]
    bits = np.unpackbits(fx["flip_mask_bits"])
    assert (h, w) == (224, 224) and len(counts) == 24 and 0 < drawn.sum() < 24
    cfg = ShapesConfig()
    T = cfg.TRUE_BOX_BUFFER
    ds = ShapesDataset(int(fx["seed"]))
    ds.load_shapes(len(counts), h, w, start_index=start)
    ds.prepare()
    samples = [list(load_image_gt(ds, cfg, g)) for g in range(len(counts))]
    flip = Augmentation(fliplr=1.0).params(0, 0, h, w)
    rows = np.stack([flip if drawn[g] else IDENTITY_ROW for g in range(len(counts))])
    images, masks, ids = R.pack_samples(samples, T)
    got = _host(DeviceAugmenter(cfg).apply(images, masks, ids, rows))
    assert got["images"].tobytes() == (fx["flip_images"] / 255.).astype(np.float32).tobytes()
    o_bit = o_box = 0
    for g in range(len(counts)):
        n = int(counts[g])
        want_m = np.zeros((h, w, T), np.uint8)
        want_m[:, :, :n] = bits[o_bit:o_bit + h * w * n].reshape(h, w, n)
        np.testing.assert_array_equal(got["gt_masks"][g], want_m)
        want_b, want_i = np.zeros((T, 4), np.int32), np.zeros(T, np.int32)
        want_b[:n], want_i[:n] = fx["flip_boxes"][o_box:o_box + n], fx["flip_class_ids"][o_box:o_box + n]
        np.testing.assert_array_equal(got["gt_boxes"][g], want_b)
        np.testing.assert_array_equal(got["gt_ids"][g], want_i)
        o_bit += h * w * n
        o_box += n
    assert o_box == len(fx["flip_boxes"])


def test_general_transforms_equal_the_restatement():
    from myolo.augment import Augmentation, DeviceAugmenter
    from myolo.config import ShapesConfig, make_config
    from myolo.shapes import make_shapes_samples
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[96, 96, 3], BATCH_SIZE=8)
    samples = make_shapes_samples(8, cfg, seed=1234)
    aug = Augmentation(**FULL)
    rows = np.stack([aug.params(0, i, 96, 96) for i in range(8)])
    rows[3] = [1, 0, -48, 0, 1, 0, 1, 0]            # image 3: its first instance leaves the frame, its second stays
    rows[5] = [1, 0, -96, 0, 1, 0, 1, 0]            # image 5: every instance leaves
    want = R.augment_cfg_batch(samples, rows, cfg, cval=aug.cval)
    # the inputs hold what this test is about
    assert list(samples[3][1]) == [1, 3] and list(want["gt_ids"][3][:2]) == [3, 0] and want["gt_masks"][3, :, :, 0].any()
    assert not want["gt_ids"][5].any() and not want["y_true"][5].any() and not want["true_boxes"][5].any() and not want["gt_masks"][5].any()
    touching = rotated_flipped = 0
    for b in range(8):
        for k in range(int((want["gt_ids"][b] != 0).sum())):
            x1, y1, x2, y2 = want["gt_boxes"][b, k]
            if x1 == 0 or y1 == 0 or x2 == 96 or y2 == 96:
                touching += 1
                d = aug.draw(0, b)
                rotated_flipped += b not in (3, 5) and d["flip"] and d["theta"] != 0.0
    assert touching >= 3 and rotated_flipped >= 1, (touching, rotated_flipped)
    images, masks, ids = R.pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    got = _host(DeviceAugmenter(cfg, cval=aug.cval).apply(images, masks, ids, rows))
    _assert_bit_equal(got, want)


@pytest.mark.parametrize("H,W,T,with_targets", [(40, 40, 3, True), (40, 40, 3, False), (40, 40, 4, True), (37, 41, 3, True)])
def test_c_abi_ragged_tail_and_other_slot_count(H, W, T, with_targets):
    """the entry point itself at 40 x 40 (1600 pixels: a ragged last workgroup), T = 3, G = 2, A = 2, C = 2, a non-zero cval, an empty slot in
    front of a live one; and its argument checks.  T = 4 takes the four-bytes-per-load form of the mask reads (T = 10: two, T = 3: one);
    37 x 41 x 3 mask bytes per image are no multiple of four, which takes the byte form of the mask stores."""
    import torch
    from myolo import _ext as X
    rs = np.random.RandomState(5)
    B, G, A, C = 3, 2, 2, 2
    images = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    masks = np.zeros((B, H, W, T), np.uint8)
    masks[0, 5:20, 8:30, 0] = 1
    masks[0, 25:40, 0:12, 2] = 1
    masks[1, 0:40, 0:40, 1] = 1                      # slot 0 empty, slot 1 live: compaction to slot 0
    masks[1, 10:12, 10:12, 2] = 1                    # set pixels in a slot whose class id is 0: not an instance
    masks[2, 30:36, 30:40, 0] = 1
    masks[2, 2:9, 3:7, 1] = 1
    masks[2, 18:22, 18:22, 2] = 1
    ids = np.zeros((B, T), np.int32)
    ids[:, :3] = [[1, 0, 1], [0, 1, 0], [1, 1, 1]]
    th = np.radians(20.)
    rows = np.array([[1, 0, 0, 0, 1, 0, 1, 0],
                     [np.cos(th) / .8, np.sin(th) / .8, 3.25, -np.sin(th) / .8, np.cos(th) / .8, -6.5, 1.1, -9.],
                     [-1.2, 0, 44.5, 0, 1.2, -4.75, .9, 12.]], np.float64)
    anchors = np.array([0.6, 0.7, 1.4, 1.2], np.float64)
    cval = 37.0
    want = R.augment_batch(images, masks, ids, rows, cval, H, W, T, G, A, C, anchors)
    assert list(want["gt_ids"][1][:3]) == [1, 0, 0] and (want["gt_ids"] != 0).sum() >= 5
    dev = torch.device("cuda:0")
    src = [torch.from_numpy(a).to(dev) for a in (images, masks, ids, rows, anchors)]
    out = dict(images=torch.full((B, H, W, 3), -1., device=dev), gt_masks=torch.full((B, H, W, T), 9, dtype=torch.uint8, device=dev),
               gt_boxes=torch.full((B, T, 4), -1, dtype=torch.int32, device=dev), gt_ids=torch.full((B, T), -1, dtype=torch.int32, device=dev),
               y_true=torch.full((B, G, G, A, 5 + C), -1., device=dev), true_boxes=torch.full((B, T, 4), -1., device=dev))
    ws = torch.empty(X.augment_ws_bytes(B, T), dtype=torch.uint8, device=dev)
    assert ws.numel() > 0

    def call(t=T, ws_bytes=ws.numel(), tb=X.ptr(out["true_boxes"]) if with_targets else None):
        return X.load().myolo_augment_batch(X.ptr(src[0]), X.ptr(src[1]), X.ptr(src[2]), X.ptr(src[3]), cval, X.ptr(src[4]),
                                            X.ptr(out["images"]), X.ptr(out["gt_masks"]), X.ptr(out["gt_boxes"]), X.ptr(out["gt_ids"]),
                                            X.ptr(out["y_true"]) if with_targets else None, tb, B, H, W, t, G, A, C,
                                            ws.data_ptr(), ws_bytes, X.stream())
    assert call(t=33) == -1 and b"T" in X.load().myolo_last_error_string()          # the slot bound of the LDS arrays
    assert call(ws_bytes=8) != 0
    if with_targets:
        assert call(tb=None) == -1                                                   # y_true without true_boxes
    assert call() == 0
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _assert_bit_equal(got, want, keys=KEYS if with_targets else ("images", "gt_ids", "gt_boxes", "gt_masks"))
    if not with_targets:
        assert (got["y_true"] == -1).all() and (got["true_boxes"] == -1).all()       # left alone


def _small_cfg():
    from myolo.config import ShapesConfig, make_config
    return make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], ALPHA=0.5, BATCH_SIZE=4)


def test_augmented_batch_plugs_into_the_step():
    import torch
    from myolo.augment import Augmentation, DeviceAugmenter
    from myolo.model import MaskYOLO
    from myolo.shapes import make_shapes_samples
    cfg = _small_cfg()
    samples = make_shapes_samples(4, cfg)
    aug = Augmentation(seed=2, **FULL)
    rows = np.stack([aug.params(0, i, 64, 64) for i in range(4)])
    want = R.augment_cfg_batch(samples, rows, cfg)
    assert (want["gt_ids"] != 0).sum() >= 3
    images, masks, ids = R.pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    model = MaskYOLO(mode="training", config=cfg)
    side = model.net._copy_stream
    db = DeviceAugmenter(cfg).apply(images, masks, ids, rows, stream=side, consumer=torch.cuda.current_stream())
    assert "_ready" in db
    model.net.seen = 0
    a = model.train_on_batch(db, learning_rate=0.0)
    la, ta = a["loss"], np.array(a["target_class_ids"])
    model.net.seen = 0
    b = model.train_on_batch([want[k] for k in KEYS], learning_rate=0.0)
    lb, tb = b["loss"], np.array(b["target_class_ids"])
    print("loss from the device batch %.9g, from the restated host batch %.9g" % (la, lb))
    assert np.array_equal(ta, tb)
    assert np.isfinite(la) and abs(la - lb) < 1e-3 * max(1.0, abs(lb)), (la, lb)


def test_train_end_to_end_with_augmentation():
    from myolo.augment import Augmentation, DeviceAugmenter, IDENTITY_ROW
    from myolo.model import MaskYOLO
    from myolo.myolo_utils import BatchGenerator, load_image_gt
    from myolo.shapes import ShapesDataset
    cfg = _small_cfg()
    ds = ShapesDataset(1234)
    ds.load_shapes(8, 64, 64)
    ds.prepare()

    def run(augmentation, **kw):
        model = MaskYOLO(mode="training", config=cfg)
        hist = model.train(ds, None, learning_rate=1e-3, epochs=2, layers="all", augmentation=augmentation, verbose=0, **kw)
        assert len(hist) == 2 and np.all(np.isfinite(hist)), hist
        return hist[0], model

    l1, _ = run(Augmentation(seed=1, **FULL))
    l2, _ = run(Augmentation(seed=1, **FULL))
    l3, _ = run(Augmentation(seed=2, **FULL))
    l0, model = run(None)
    print("first-epoch losses: seed 1 %.9g, seed 1 again %.9g, seed 2 %.9g, no augmentation %.9g" % (l1, l2, l3, l0))
    tol = 1e-3 * max(1.0, abs(l1))
    assert abs(l1 - l2) < tol, (l1, l2)
    assert abs(l1 - l3) > tol and abs(l1 - l0) > tol, (l1, l3, l0)
    with pytest.raises(TypeError, match="myolo.augment.Augmentation"):
        model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", augmentation=object(), verbose=0)

    # a sample whose source is in no_augmentation_sources reaches the step un-augmented: the rows train() builds, through the augmenter
    for i in (1, 4, 6):
        ds.image_info[i]["source"] = "plain"
    aug = Augmentation(seed=1, **FULL)
    idx = list(range(8))
    rows = model.augmentation_rows(aug, ["plain"], ds, 1, idx)
    for i in idx:
        if i in (1, 4, 6):
            assert rows[i].tobytes() == IDENTITY_ROW.tobytes()
        else:
            assert rows[i].tobytes() == aug.params(1, i, 64, 64).tobytes() != IDENTITY_ROW.tobytes()
    samples = [list(load_image_gt(ds, cfg, i)) for i in idx]
    images, masks, ids = R.pack_samples(samples, cfg.TRUE_BOX_BUFFER)
    got = _host(DeviceAugmenter(cfg).apply(images[:4], masks[:4], ids[:4], rows[:4]))
    plain = BatchGenerator(samples[:4], cfg, 'training', shuffle=False, norm=True)[0][0]
    assert got["images"][1].tobytes() == plain[0][1].tobytes() and got["images"][0].tobytes() != plain[0][0].tobytes()
    np.testing.assert_array_equal(got["gt_masks"][1], plain[5][1].astype(np.uint8))
    np.testing.assert_array_equal(got["gt_boxes"][1], plain[4][1])
    np.testing.assert_array_equal(got["y_true"][1], plain[2][1].astype(np.float32))
    assert np.array_equal(model.augmentation_rows(aug, None, ds, 1, idx), np.stack([aug.params(1, i, 64, 64) for i in idx]))

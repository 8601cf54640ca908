"""Detection on images of any size: myolo_resize_images_u8 against the host statement myolo_utils.resize_image bit for bit,
and MaskYOLO.detect / detect_many on images that are not at config.IMAGE_SHAPE, in both mask frames."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X                                            # noqa: E402
from myolo import myolo_utils as mutils                                # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.engine import pack_images, packed_bytes                     # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402

DEV = "cuda"
KEYS = ("bboxes", "class_ids", "confidence_scores", "full_masks")


# ------------------------------------------------------------------------------------------------ the kernel
def _sources():
    rng = np.random.default_rng(20)
    u8 = lambda h, w, lo=0, hi=256: rng.integers(lo, hi, (h, w, 3), dtype=np.uint8)           # noqa: E731
    return [
        u8(7, 5, 40, 251),                      # an upscale: the rim blends with the zero border and is clipped back to the minimum
        u8(53, 37),                             # a non-integer shrink
        u8(64, 96),                             # an exact 2 x shrink: weights of 1/2
        u8(32, 48),                             # already at the frame: must come back as it is
        u8(1, 1),
        np.full((19, 23, 3), 117, np.uint8),    # constant: every output is the constant
        u8(517, 1031),
    ]


def _resize_call(srcs, H, W, with_u8):
    n = len(srcs)
    host = np.zeros(packed_bytes(srcs), np.uint8)
    desc = pack_images(srcs, host)
    head = n * 24
    packed = torch.from_numpy(host).to(DEV)
    unit = torch.full((n, H, W, 3), -1.0, dtype=torch.float32, device=DEV)
    u8 = torch.full((n, H, W, 3), 99, dtype=torch.uint8, device=DEV) if with_u8 else None
    ws = torch.empty(2 * n, dtype=torch.int32, device=DEV)
    assert ws.numel() * 4 == X.resize_ws_bytes(n)
    X.call("myolo_resize_images_u8", packed.data_ptr() + head, host.size - head, packed.data_ptr(), desc.ctypes.data, X.ptr(u8), X.ptr(unit),
           n, H, W, ws.data_ptr(), ws.numel() * 4, X.stream())
    torch.cuda.synchronize()
    return desc, (None if u8 is None else u8.cpu().numpy()), unit.cpu().numpy(), ws.cpu().numpy()


def test_kernel_equals_resize_image_bit_for_bit():
    """one call, frame 32 x 48, seven sources of mixed sizes in one buffer (so the offsets are odd): out_u8 is resize_image's result with NO tolerance
    (the host function is the pinned statement of the reference's wrapper; the device adds nothing to its single-count difference from
    scikit-image), out_unit is its / 255. in float32, and a second call without out_u8 gives the same floats"""
    H, W = 32, 48
    srcs = _sources()
    desc, u8, unit, mm = _resize_call(srcs, H, W, True)
    assert any(int(o) % 2 for o in desc[:, 0]) and any((int(o) + 24 * len(srcs)) % 16 for o in desc[:, 0])      # unaligned starts
    n = len(srcs)
    for k, s in enumerate(srcs):
        assert (mm[k], mm[n + k]) == (s.min(), s.max()), (k, mm[k], mm[n + k], s.min(), s.max())
        want = mutils.resize_image(s, [H, W, 3])[0]
        assert want.dtype == np.uint8 and want.shape == (H, W, 3)
        bad = int((u8[k] != want).sum())
        print("image %d (%d x %d): %d of %d bytes differ" % (k, s.shape[0], s.shape[1], bad, want.size))
        assert u8[k].tobytes() == want.tobytes(), (k, s.shape, bad)
    assert u8[3].tobytes() == srcs[3].tobytes()                        # the image at frame size comes back as it is
    assert (u8[5] == 117).all()
    assert u8[0].min() == srcs[0].min() >= 40                          # the faded rim was clipped back up to the source's minimum
    assert unit.tobytes() == (u8 / 255.).astype(np.float32).tobytes()
    _, none, unit2, _ = _resize_call(srcs, H, W, False)
    assert none is None and unit2.tobytes() == unit.tobytes()


def test_kernel_minmax_head_body_and_tail():
    """the per-image extrema when the only extreme byte sits in the unaligned head, in the 16-byte body or in the tail of an image, and for images
    shorter than one 16-byte load; seen through the clip (a constant frame would hide it, so the frame is 1 x 1 and the workspace is read)"""
    rng = np.random.default_rng(5)
    srcs = []
    for h, w, where in ((1, 1, None), (1, 3, 0), (1, 3, 8), (9, 11, 0), (9, 11, 150), (9, 11, 296), (40, 57, 1), (40, 57, 3001), (40, 57, 6839)):
        s = rng.integers(100, 150, (h, w, 3), dtype=np.uint8)
        if where is not None:
            s.reshape(-1)[where] = 250
            s.reshape(-1)[(where + s.size // 2) % s.size] = 3
        srcs.append(s)
    _, _, _, mm = _resize_call(srcs, 1, 1, True)
    n = len(srcs)
    for k, s in enumerate(srcs):
        assert (mm[k], mm[n + k]) == (s.min(), s.max()), (k, s.shape)


def test_resize_to_frame_reuses_its_staging_buffer():
    cfg, m = _model()
    rng = np.random.default_rng(9)
    for rnd in range(2):                                               # the second round packs into the buffer the first one uploaded from
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((77, 130), (128, 128), (211, 64))]
        x, u8 = m.net.resize_to_frame(imgs, want_u8=True, n_slots=4)
        assert tuple(x.shape) == (4, 128, 128, 3) and x.dtype == torch.float32 and u8.dtype == torch.uint8
        u8 = u8.cpu().numpy()
        for k in range(4):
            assert u8[k].tobytes() == mutils.resize_image(imgs[min(k, 2)], cfg.IMAGE_SHAPE)[0].tobytes(), (rnd, k)
        assert x.cpu().numpy().tobytes() == (u8 / 255.).astype(np.float32).tobytes()
        assert m.net.resize_to_frame(imgs).cpu().numpy().tobytes() == x[:3].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------ the model
_MODEL = []


def _model():
    if not _MODEL:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4)
        _MODEL.append((cfg, MaskYOLO(mode="inference", config=cfg, seed=4)))
    return _MODEL[0]


def _shapes_like(h, w, seed):
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


def _same(a, b, what):
    for key in KEYS:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (what, key, a[key].shape, b[key].shape)
        assert np.array_equal(a[key], b[key]), (what, key)


def _forward(m, p):
    """the forward detect(p) runs, and its selection: -> det [R,6], masks [R,mh,mw,C] (host), the selected rows, their normalised corners"""
    x = m.net.resize_to_frame([p])
    _, det_d, mask_d = m.net.predict_graphed(x)
    det, masks = det_d[0].cpu().numpy(), mask_d[0].cpu().numpy()
    keep, nmb, boxes, scores, class_ids = m._select(det, 0.0)
    return det, masks, keep[nmb], boxes[nmb], scores[nmb], class_ids[nmb]


def test_network_frame_equals_detect_on_the_host_resized_image():
    cfg, m = _model()
    p = _shapes_like(200, 150, 1)
    got = m.detect(p, cs_threshold=0.0, mask_frame="network")[0]
    want = m.detect(mutils.resize_image(p, cfg.IMAGE_SHAPE)[0], cs_threshold=0.0)[0]
    assert len(got["class_ids"]) >= 1 and got["full_masks"].shape[:2] == (128, 128)
    _same(got, want, "network frame")


def test_image_frame_boxes_are_the_normalised_corners_in_the_images_pixels():
    cfg, m = _model()
    p = _shapes_like(200, 150, 1)
    got = m.detect(p, cs_threshold=0.0)[0]
    net = m.detect(p, cs_threshold=0.0, mask_frame="network")[0]
    assert len(got["class_ids"]) >= 1
    assert np.array_equal(got["class_ids"], net["class_ids"]) and np.array_equal(got["confidence_scores"], net["confidence_scores"])
    _, _, rows, corners, scores, class_ids = _forward(m, p)
    assert len(rows) == len(got["class_ids"]) and np.array_equal(scores, got["confidence_scores"]) and np.array_equal(class_ids, got["class_ids"])
    assert np.array_equal(got["bboxes"], corners * np.array([150, 200, 150, 200], dtype=corners.dtype))
    assert got["bboxes"].dtype == net["bboxes"].dtype
    assert got["full_masks"].shape == (200, 150, len(rows)) and got["full_masks"].dtype == net["full_masks"].dtype


def test_image_frame_masks_equal_a_host_paste():
    """full_masks of detect(p) against a paste written here: the mask rows of the same forward, each resized to its window of the 200 x 150 image
    by myolo_utils._resize_bilinear -- the window taken by the WIDTH for x and by the HEIGHT for y -- thresholded at 0.5"""
    cfg, m = _model()
    p = _shapes_like(200, 150, 1)
    h, w = p.shape[:2]
    got = m.detect(p, cs_threshold=0.0)[0]
    det, masks, rows, _, _, _ = _forward(m, p)
    assert len(rows) >= 1 and got["full_masks"].shape == (h, w, len(rows))
    f = np.float32
    some = 0
    for i, r in enumerate(rows):
        d = det[r]
        x1, x2 = min(max(0, int(f(d[0]) * f(w))), w), min(max(1, int(f(d[2]) * f(w))), w)
        y1, y2 = min(max(0, int(f(d[1]) * f(h))), h), min(max(1, int(f(d[3]) * f(h))), h)
        want = np.zeros((h, w), bool)
        if y2 > y1 and x2 > x1:
            want[y1:y2, x1:x2] = mutils._resize_bilinear(masks[r, :, :, int(d[5])], y2 - y1, x2 - x1) >= f(0.5)
        bad = int((got["full_masks"][:, :, i].astype(bool) != want).sum())
        print("detection %d: window x %d..%d y %d..%d, %d pixels set, %d differ" % (i, x1, x2, y1, y2, int(want.sum()), bad))
        assert bad == 0, (i, bad)
        some += int(want.sum())
    assert some > 0                                                    # not a comparison of empty masks


FIVE = ((128, 128), (200, 150), (61, 97), (128, 128), (300, 40))


def test_detect_many_mixed_sizes_equals_detect():
    """five images of mixed sizes in one call (batch 4: a mixed first batch, a short last one): every result equals detect(image)[0]"""
    cfg, m = _model()
    imgs = [_shapes_like(h, w, 10 + k) for k, (h, w) in enumerate(FIVE)]
    many = m.detect_many(imgs, cs_threshold=0.0)
    assert len(many) == 5 and sum(len(r["class_ids"]) for r in many) >= 5
    for k, im in enumerate(imgs):
        assert many[k]["full_masks"].shape[:2] == im.shape[:2]
        _same(many[k], m.detect(im, cs_threshold=0.0)[0], "image %d" % k)


@pytest.mark.parametrize("frame", ["image", "network"])
def test_detect_many_mixed_sizes_equals_the_forward_at_its_batch_shape(frame):
    """the same call, and one whose middle batch is all at network size (the byte path beside the resized batches), against the forward of each
    image at detect_many's own launch shape -- the image first in a batch padded with itself, as tests/test_gpu_step.py holds detect_many"""
    cfg, m = _model()
    sizes = FIVE[:4] + ((128, 128),) * 4 + FIVE[4:]
    imgs = [_shapes_like(h, w, 10 + k) for k, (h, w) in enumerate(sizes)]
    many = m.detect_many(imgs, cs_threshold=0.0, mask_frame=frame)
    assert len(many) == len(imgs)
    for k in (0, 1, 2, 5, 8):
        x = m.net.resize_to_frame([imgs[k]], n_slots=4)
        _, det_d, mask_d = m.net.predict_graphed(x)
        one = m._select_and_unmold(det_d[0], mask_d[0], imgs[k].shape if frame == "image" else cfg.IMAGE_SHAPE, 0.0)
        assert len(one["class_ids"]) >= 1
        _same(many[k], one, "image %d" % k)


def test_mask_frame_is_checked():
    cfg, m = _model()
    p = _shapes_like(40, 30, 2)
    with pytest.raises(ValueError):
        m.detect(p, mask_frame="photo")
    with pytest.raises(ValueError):
        m.detect_many([p], mask_frame="photo")
    with pytest.raises(AssertionError):
        m.detect(p.astype(np.float32))
    with pytest.raises(AssertionError):
        m.detect_many([p[:, :, 0]])


# ------------------------------------------------------------------------------------------------ the staging rings (myolo/detect.py Stager)
ELEVEN = ((128, 128), (128, 128), (200, 150), (300, 40), (61, 97), (1, 1), (128, 128), (128, 128), (128, 128), (128, 128), (77, 130))
_PAIRS = []


def _pairs():
    if not _PAIRS:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=2)
        _PAIRS.append((cfg, MaskYOLO(mode="inference", config=cfg, seed=4), [_shapes_like(h, w, 40 + k) for k, (h, w) in enumerate(ELEVEN)]))
    return _PAIRS[0]


def _same_results(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert list(a) == list(b), (what, k)
        for key in a:
            if key == "rle_masks":
                assert [x["size"] for x in a[key]] == [x["size"] for x in b[key]], (what, k)
                assert all(x["counts"].dtype == y["counts"].dtype and np.array_equal(x["counts"], y["counts"]) for x, y in zip(a[key], b[key])), (what, k)
            else:
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (what, k, key)


@pytest.mark.parametrize("fmt", ["dense", "rle"])
def test_a_wrapping_ring_gives_what_a_ring_that_never_wraps_gives(fmt):
    """eleven images in batches of two -- six batches, some at frame and some resized, a 1 x 1 image among them, a short last one -- with render:
    in_flight=1 stages through four slots, so batches 4 and 5 reuse the slots of batches 0 (at frame) and 1 (resized) while earlier batches are
    in flight; in_flight=3 has eight slots and reuses none.  predict_stream is held bit-identical across in_flight (tests/test_gpu_step.py), so
    every array of every result must be equal."""
    cfg, m, imgs = _pairs()
    stager = m._stager()
    groups = [imgs[lo:lo + 2] for lo in range(0, len(imgs), 2)]
    kinds = [stager.at_frame(g) for g in groups]
    assert len(groups) == 6 and len(groups[-1]) == 1
    assert kinds[0] and kinds[4] and not kinds[1] and not kinds[5]          # each ring has a slot that is used twice
    wrapped = m.detect_many(imgs, cs_threshold=0.0, in_flight=1, mask_format=fmt, render=True)
    assert stager.slots == 4 < len(groups)
    roomy = m.detect_many(imgs, cs_threshold=0.0, in_flight=3, mask_format=fmt, render=True)
    assert stager.slots == 8 > len(groups)
    assert sum(len(r["class_ids"]) for r in wrapped) >= len(imgs)
    for im, r in zip(imgs, wrapped):
        assert r["rendered"].shape == im.shape and r["rendered"].dtype == np.uint8
    _same_results(wrapped, roomy, fmt)


@pytest.mark.parametrize("k", [0, 2])
def test_detect_rle_with_render_equals_the_dense_call(k):
    """one image at IMAGE_SHAPE and one of another size through detect(render=True, mask_format="rle"): the overlay is detect(render=True)'s,
    and every run-length mask decodes to the dense plane"""
    from myolo import rle
    cfg, m, imgs = _pairs()
    im = imgs[k]
    dense = m.detect(im, cs_threshold=0.0, render=True, save_path=None)[0]
    coded = m.detect(im, cs_threshold=0.0, render=True, save_path=None, mask_format="rle")[0]
    n = len(dense["class_ids"])
    assert n >= 1 and list(coded) == ["bboxes", "class_ids", "confidence_scores", "rle_masks", "rendered"] and len(coded["rle_masks"]) == n
    for key in ("bboxes", "class_ids", "confidence_scores", "rendered"):
        assert coded[key].dtype == dense[key].dtype and np.array_equal(coded[key], dense[key]), key
    assert dense["rendered"].shape == im.shape and (dense["rendered"] != im).any()
    for i, code in enumerate(coded["rle_masks"]):
        assert code["size"] == list(im.shape[:2]) and np.array_equal(rle.decode(code), dense["full_masks"][:, :, i]), i
    assert dense["full_masks"].any()

"""Host side of the on-device augmentation (myolo/augment.py): the parameter rows, and the numpy restatement of the arithmetic contract
(tests/augment_ref.py) held against what the host pipeline itself gives where the two must agree -- identity rows against BatchGenerator,
flip rows against np.fliplr + load_image_gt's filter and boxes."""
import numpy as np
import pytest

import augment_ref as R
from myolo.augment import Augmentation, IDENTITY_ROW
from myolo.config import ShapesConfig, make_config
from myolo.myolo_utils import BatchGenerator, extract_bboxes
from myolo.shapes import make_shapes_samples

FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))


def test_params_are_a_pure_function_of_seed_epoch_and_image_id():
    a = Augmentation(seed=3, **FULL)
    base = a.params(2, 17, 96, 96)
    assert base.dtype == np.float64 and base.shape == (8,)
    np.testing.assert_array_equal(base, a.params(2, 17, 96, 96))
    np.testing.assert_array_equal(base, Augmentation(seed=3, **FULL).params(2, 17, 96, 96))       # no hidden state
    a.params(0, 1, 96, 96)                                                                         # other draws in between change nothing
    np.testing.assert_array_equal(base, a.params(2, 17, 96, 96))
    for other in (Augmentation(seed=4, **FULL).params(2, 17, 96, 96), a.params(3, 17, 96, 96), a.params(2, 18, 96, 96)):
        assert not np.array_equal(base, other)


def test_default_and_pure_flip_rows_are_exact():
    for h, w in ((64, 64), (96, 96), (224, 224), (40, 56)):
        for ep, i in ((0, 0), (3, 11)):
            row = Augmentation().params(ep, i, h, w)
            assert row.tobytes() == IDENTITY_ROW.tobytes()
            flip = Augmentation(fliplr=1.0).params(ep, i, h, w)
            assert flip.tobytes() == np.array([-1., 0., w - 1., 0., 1., 0., 1., 0.]).tobytes()


def test_draws_stay_inside_their_ranges_and_rows_invert_the_forward_map():
    a = Augmentation(seed=1, **FULL)
    flips = 0
    for i in range(200):
        d = a.draw(i % 5, i)
        flips += d["flip"]
        assert .7 <= d["scale"] <= 1.3 and -.3 <= d["tx"] <= .3 and -.3 <= d["ty"] <= .3
        assert -30 <= d["theta"] <= 30 and .8 <= d["gain"] <= 1.2 and -.1 <= d["bias"] <= .1
        # the row is the inverse of  out = c + t + s R(theta) F (src - c)
        H, W = 96, 128
        p = a.params(i % 5, i, H, W)
        c = np.array([(W - 1) / 2., (H - 1) / 2.])
        th = np.radians(d["theta"])
        Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        F = np.diag([-1. if d["flip"] else 1., 1.])
        src = np.array([13., 57.])
        out = c + np.array([d["tx"] * W, d["ty"] * H]) + d["scale"] * Rm @ F @ (src - c)
        back = np.array([p[0] * out[0] + p[1] * out[1] + p[2], p[3] * out[0] + p[4] * out[1] + p[5]])
        np.testing.assert_allclose(back, src, rtol=0, atol=1e-9)
        assert p[6] == d["gain"] and p[7] == d["bias"] * 255.0
    assert 60 <= flips <= 140


@pytest.mark.parametrize("kw", [dict(fliplr=1.5), dict(fliplr=-.1), dict(scale=(0., 1.)), dict(scale=(1.2, .8)), dict(scale=(1.,)),
                                dict(translate=(-2., 0.)), dict(translate=(.3, -.3)), dict(rotate=(0., 400.)), dict(rotate=(10., -10.)),
                                dict(brightness=(-.5, 1.)), dict(brightness=(1.2, .8)), dict(offset=(-.1, 1.5)), dict(offset=(.1, -.1)),
                                dict(cval=256), dict(cval=-1), dict(scale=(1., float("nan"))), dict(scale=1.0), dict(seed=-1)])
def test_bad_ranges_raise(kw):
    with pytest.raises(ValueError):
        Augmentation(**kw)


@pytest.mark.parametrize("size", [64, 96])
def test_restatement_reproduces_batch_generator_on_identity_rows(size):
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[size, size, 3], BATCH_SIZE=8)
    samples = make_shapes_samples(8, cfg)
    want = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0][0]
    got = R.augment_cfg_batch(samples, np.tile(IDENTITY_ROW, (8, 1)), cfg)
    assert got["images"].tobytes() == want[0].tobytes()
    np.testing.assert_array_equal(got["true_boxes"], want[1].reshape(8, -1, 4).astype(np.float32))
    np.testing.assert_array_equal(got["y_true"], want[2].astype(np.float32))
    np.testing.assert_array_equal(got["gt_ids"], want[3])
    np.testing.assert_array_equal(got["gt_boxes"], want[4])
    np.testing.assert_array_equal(got["gt_masks"], want[5].astype(np.uint8))
    assert (want[3] != 0).sum() >= 12 and want[2].sum() > 0


@pytest.mark.parametrize("size", [64, 96])
def test_restatement_reproduces_fliplr_on_flip_rows(size):
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[size, size, 3], BATCH_SIZE=8)
    T = cfg.TRUE_BOX_BUFFER
    samples = make_shapes_samples(8, cfg)
    rows = np.tile(Augmentation(fliplr=1.0).params(0, 0, size, size), (8, 1))
    got = R.augment_cfg_batch(samples, rows, cfg)
    flipped = []
    for image, ids, _, masks in samples:                       # load_image_gt's flip, filter and boxes (myolo_utils.py:306-311, 346-352)
        m = np.fliplr(masks)
        keep = np.sum(m, axis=(0, 1)) > 0
        flipped.append([np.fliplr(image), ids[keep], extract_bboxes(m[:, :, keep]), m[:, :, keep]])
    want = BatchGenerator(flipped, cfg, 'training', shuffle=False, norm=True)[0][0]
    assert got["images"].tobytes() == want[0].tobytes()
    np.testing.assert_array_equal(got["true_boxes"], want[1].reshape(8, T, 4).astype(np.float32))
    np.testing.assert_array_equal(got["y_true"], want[2].astype(np.float32))
    np.testing.assert_array_equal(got["gt_ids"], want[3])
    np.testing.assert_array_equal(got["gt_boxes"], want[4])
    np.testing.assert_array_equal(got["gt_masks"], want[5].astype(np.uint8))


def test_fill_raw_stages_the_unaugmented_sample_and_its_row():
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=4)
    T = cfg.TRUE_BOX_BUFFER
    samples = make_shapes_samples(6, cfg)
    for k, s in enumerate(samples):
        s.append(100 + k)
    gen = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)
    out = [np.full((4, 64, 64, 3), 7, np.uint8), np.full((4, 64, 64, T), 7, np.uint8), np.full((4, T), 7, np.int32), np.zeros((4, 8))]
    gen.fill_raw(1, out, lambda inst: np.arange(8.) + inst[4])
    images, masks, ids = R.pack_samples(samples[2:6], T)             # the wrapped last batch
    np.testing.assert_array_equal(out[0], images)
    np.testing.assert_array_equal(out[1], masks)
    np.testing.assert_array_equal(out[2], ids)
    np.testing.assert_array_equal(out[3][:, 0], [102., 103., 104., 105.])
    samples[3][0] = samples[3][0].astype(np.float32)
    with pytest.raises(ValueError):
        gen.fill_raw(0, out, lambda inst: np.zeros(8))

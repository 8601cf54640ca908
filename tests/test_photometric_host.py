"""Host side of the photometric augmentation (myolo.augment.Photometric, check_photo_rows) and the numpy restatement of its device contract
(tests/photometric_ref.py): no GPU."""
import math

import numpy as np
import pytest

import photometric_ref as PR
from myolo.augment import PHOTO_ROW, Photometric, check_photo_rows, photo_reflect

WIDE = dict(hue=(-40, 40), saturation=(.5, 1.5), contrast=(.6, 1.4), blur=(0., 5.), noise=(0., .1))


def test_row_is_pure_and_keyed_by_seed_epoch_and_image():
    p = Photometric(seed=7, **WIDE)
    a = p.row(2, 11)
    assert a.dtype == np.float64 and a.shape == (PHOTO_ROW,) and a.tobytes() == Photometric(seed=7, **WIDE).row(2, 11).tobytes()
    assert a.tobytes() == p.row(2, 11).tobytes()
    others = [Photometric(seed=8, **WIDE).row(2, 11), p.row(3, 11), p.row(2, 12)]
    assert all(o.tobytes() != a.tobytes() for o in others)
    # the draws are those of RandomState([seed, epoch, id, 1]) in a fixed order
    u = np.random.RandomState([7, 2, 11, 1]).random_sample(7)
    d = p.draw(2, 11)
    assert d["on"] and d["hue"] == -40 + 80 * u[1] and d["saturation"] == .5 + 1.0 * u[2] and d["contrast"] == .6 + (1.4 - .6) * u[3]
    assert d["sigma"] == 5.0 * u[4] and d["std"] == .1 * u[5] and d["key"] == int(u[6] * 2.0 ** 32)
    assert a[12] == d["std"] and a[13] == d["key"] and a[15] == 0.0
    # a generator of the caller's, re-seeded per sample, gives the same rows in any order; the object holds no state and copies like the others
    import copy
    import pickle
    rs = np.random.RandomState(123)
    for e, i in ((3, 11), (2, 11), (2, 12), (2, 11)):
        assert p.row(e, i, rs).tobytes() == p.row(e, i).tobytes() and p.draw(e, i, rs) == p.draw(e, i)
    assert pickle.loads(pickle.dumps(p)).row(2, 11).tobytes() == a.tobytes() and copy.deepcopy(p).row(2, 11).tobytes() == a.tobytes()


def test_a_draw_does_not_depend_on_which_other_ranges_are_open():
    """always the same draws in the same order: opening or closing one range leaves every other parameter's draw where it was"""
    full = Photometric(seed=3, **WIDE).draw(1, 5)
    for name in WIDE:
        only = Photometric(seed=3, **{name: WIDE[name]}).draw(1, 5)
        key = dict(blur="sigma", noise="std").get(name, name)
        assert only[key] == full[key] and only["key"] == full["key"], name
        neutral = Photometric().draw(1, 5)
        for other in ("hue", "saturation", "contrast", "sigma", "std"):
            if other != key:
                assert only[other] == neutral[other], (name, other)
    # and the stream is not Augmentation's under the same seed
    assert not np.array_equal(np.random.RandomState([3, 1, 5, 1]).random_sample(7), np.random.RandomState([3, 1, 5]).random_sample(7))


def test_defaults_and_p_zero_give_exactly_the_identity_row():
    ident = Photometric.identity()
    want = np.zeros(32)
    want[[0, 5, 10, 16]] = 1.0
    assert ident.tobytes() == want.tobytes()                     # [I|0], std 0, key 0, r 0, w_0 = 1 -- and no -0.0 anywhere
    p = Photometric(seed=5)
    assert all(p.row(0, i).tobytes() == ident.tobytes() for i in range(20))      # (without noise the drawn key is not stored)
    assert Photometric(noise=(.1, .1), seed=5).row(0, 3)[13] == p.draw(0, 3)["key"] > 0
    off = Photometric(p=0.0, seed=5, **WIDE)
    assert all(off.row(e, i).tobytes() == ident.tobytes() for e in range(3) for i in range(20))
    half = Photometric(p=0.5, seed=5, **WIDE)
    n = sum(half.row(0, i).tobytes() == ident.tobytes() for i in range(200))
    assert 60 < n < 140
    assert Photometric().max_radius == 0 and Photometric(blur=(0, 5)).max_radius == 15 and Photometric(blur=(0, 1.1)).max_radius == 4


@pytest.mark.parametrize("n", [2, 3, 7])
def test_refl_is_numpys_reflect_padding(n):
    a = np.arange(n)
    for pad in (1, n - 1):                                         # np.pad reflects once only
        want = np.pad(a, pad, mode="reflect")
        assert [PR.refl(i, n) for i in range(-pad, n + pad)] == want.tolist()
    # further out: the pattern has period 2 (n - 1), so that a radius beyond the side stays valid
    for i in range(-40, 40):
        assert PR.refl(i, n) == PR.refl(i + 2 * (n - 1), n) == photo_reflect(i, n) and 0 <= PR.refl(i, n) < n


def test_refl_of_a_single_pixel():
    assert all(PR.refl(i, 1) == 0 and photo_reflect(i, 1) == 0 for i in range(-16, 17))


def test_weights_sum_to_one_and_the_radius_follows_the_rule():
    for sigma in (1e-300, 1e-3, 0.2, 1 / 3., 0.34, 0.5, 1.0, 1.7, 2.0, 4.9, 5.0):
        r, w = Photometric.kernel(sigma)
        assert r == min(15, int(math.ceil(3 * sigma))) and w.shape == (16,)
        assert abs(w[0] + 2 * w[1:].sum() - 1.0) <= 1e-15 and (w >= 0).all() and (w[r + 1:] == 0).all()
        k = np.arange(1, r + 1)
        with np.errstate(divide="ignore"):                         # (1e-300 squared is 0: every weight beyond w_0 is exp(-inf))
            assert np.allclose(w[1:r + 1] / w[0], np.exp(-k * k / (2 * sigma * sigma)), rtol=1e-14, atol=0)
        assert (np.diff(w[:r + 1]) <= 0).all()
    r, w = Photometric.kernel(0.0)
    assert r == 0 and w[0] == 1.0 and (w[1:] == 0).all()
    assert Photometric.kernel(1 / 3.)[0] == 1 and Photometric.kernel(5.0)[0] == 15 and Photometric.kernel(4.7)[0] == 15
    # the row carries them
    p = Photometric(blur=(2.0, 2.0), seed=1)
    row = p.row(0, 0)
    assert row[14] == 6 and row[16:32].tobytes() == Photometric.kernel(2.0)[1].tobytes()


def test_colour_matrix():
    L = np.array([0.299, 0.587, 0.114])
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    assert Photometric.matrix(0, 1, 1).tobytes() == ident.tobytes()
    # saturation 0: every channel is the luma, three equal rows
    for h in (0.0, 25.0):
        A = Photometric.matrix(h, 0.0, 1.0)
        assert A[0].tobytes() == A[1].tobytes() == A[2].tobytes()
    assert np.allclose(Photometric.matrix(0, 0, 1)[0], np.append(L, 0), atol=0, rtol=0)
    # a full turn is the identity, a third of a turn moves red to green, green to blue
    assert np.abs(Photometric.matrix(360.0, 1, 1) - ident).max() < 1e-12
    assert np.abs(Photometric.matrix(120.0, 1, 1)[:, :3] - np.array([[0., 0, 1], [1, 0, 0], [0, 1, 0]])).max() < 1e-12
    # grey stays grey under hue and saturation, and contrast turns about mid-grey
    A = Photometric.matrix(33.0, 0.4, 1.0)
    assert np.abs(A[:, :3].dot(np.ones(3)) - 1).max() < 1e-15 and (A[:, 3] == 0).all()
    A = Photometric.matrix(33.0, 0.4, 1.3)
    assert np.abs(A[:, :3].dot(np.full(3, .5)) + A[:, 3] - .5).max() < 1e-15 and (A[:, 3] == 0.5 * (1 - 1.3)).all()
    # c * S * R
    co, si = math.cos(math.radians(33.0)), math.sin(math.radians(33.0))
    R = co * np.eye(3) + (1 - co) / 3 * np.ones((3, 3)) + si / math.sqrt(3) * np.array([[0., -1, 1], [1, 0, -1], [-1, 1, 0]])
    S = 0.4 * np.eye(3) + 0.6 * np.outer(np.ones(3), L)
    assert np.allclose(A[:, :3], 1.3 * S.dot(R), rtol=1e-14, atol=1e-16)
    # a hue rotation preserves the luma-free part's length: R is orthogonal
    assert np.abs(R.dot(R.T) - np.eye(3)).max() < 1e-15


def test_check_photo_rows_refusals():
    rows = np.stack([Photometric(seed=2, **WIDE).row(0, i) for i in range(4)])
    check_photo_rows(rows, 4)
    check_photo_rows(np.tile(Photometric.identity(), (2, 1)), 2)

    def bad(col, value, match):
        r = rows.copy()
        r[2, col] = value
        with pytest.raises(ValueError, match=match):
            check_photo_rows(r, 4)
    bad(3, np.nan, "finite")
    bad(20, np.inf, "finite")
    bad(14, 16.0, "radius")
    bad(14, -1.0, "radius")
    bad(14, 2.5, "radius")
    bad(18, -1e-9, "weight")
    bad(12, -0.01, "deviation")
    bad(13, -1.0, "key")
    bad(13, 2.0 ** 32, "key")
    bad(13, 0.5, "key")
    for shape in ((3, 32), (4, 31), (4 * 32,)):
        with pytest.raises(ValueError, match="photometric rows: expected"):
            check_photo_rows(np.zeros(shape), 4)
    with pytest.raises(ValueError, match="photometric rows: expected"):
        check_photo_rows(rows.astype(np.float32), 4)
    r = rows.copy()
    r[0, 13] = 2.0 ** 32 - 1
    r[0, 14] = 15.0
    check_photo_rows(r, 4)


@pytest.mark.parametrize("kw,match", [
    (dict(p=-0.1), "p is a probability"), (dict(p=1.5), "p is a probability"),
    (dict(hue=(-181, 0)), "hue: low must be >= -180"), (dict(hue=(0, 181)), "hue: high must be <= 180"), (dict(hue=(5, -5)), "hue must be a finite"),
    (dict(hue=3.0), "hue must be a \\(low, high\\) pair"), (dict(hue=(0, 1, 2)), "hue must be a finite"),
    (dict(saturation=(-0.1, 1)), "saturation: low must be >= 0"), (dict(saturation=(1, np.inf)), "saturation must be a finite"),
    (dict(contrast=(-1, 1)), "contrast: low must be >= 0"), (dict(contrast=(np.nan, 1)), "contrast must be a finite"),
    (dict(blur=(-1, 1)), "blur: low must be >= 0"), (dict(blur=(0, 5.1)), "blur: high must be <= 5"),
    (dict(noise=(-0.1, 0)), "noise: low must be >= 0"), (dict(noise=(0, 1.1)), "noise: high must be <= 1"),
    (dict(seed=-1), "seed must be in"), (dict(seed=2 ** 32), "seed must be in")])
def test_constructor_validation(kw, match):
    with pytest.raises(ValueError, match=match):
        Photometric(**kw)


def test_constructor_takes_the_edges_of_every_range():
    p = Photometric(p=0, hue=(-180, 180), saturation=(0, 3), contrast=(0, 2), blur=(0, 5), noise=(0, 1), seed=2 ** 32 - 1)
    assert "hue=(-180.0, 180.0)" in repr(p) and p.max_radius == 15


def test_hash_against_a_second_statement():
    z = np.array([0, 1, 12345, (1 << 64) - 1, (0xdeadbeef << 32) | 77], np.uint64)
    assert PR.splitmix64(z).tolist() == [PR.splitmix64_int(int(v)) for v in z]
    assert PR.splitmix64_int(0) == 0xE220A8397B1DCDAF              # the first output of SplitMix64 seeded with 0
    # j of (y, x, c) and the key's place
    f = PR.noise_field(12345, 4, 5)
    y, x, c = 2, 3, 1
    zz = PR.splitmix64_int((12345 << 32) | ((y * 5 + x) * 3 + c))
    S = (zz & 0xffff) + ((zz >> 16) & 0xffff) + ((zz >> 32) & 0xffff) + (zz >> 48)
    assert f[y, x, c] == (float(S) - 131070.0) * (1.7320508075688772 / 65536.0)


@pytest.mark.parametrize("key", [0, 1, 12345, 2 ** 32 - 1])
def test_noise_field_has_zero_mean_and_unit_deviation(key):
    """the sum of four uniform 16-bit fields, centred and scaled by sqrt(3) / 65536: mean 0, variance 4 * (65536^2 - 1) / 12 * 3 / 65536^2 = 1 (less
    2e-10).  Over 64 x 64 x 3 = 12288 samples the mean's standard error is 0.009 and the deviation's 0.0064; the definition gives at most 0.011
    and 0.012 for these keys."""
    f = PR.noise_field(key, 64, 64)
    print("key %d: mean %.5f, std %.5f, min %.3f, max %.3f" % (key, f.mean(), f.std(), f.min(), f.max()))
    assert abs(f.mean()) < 0.05 and abs(f.std() - 1.0) < 0.05
    assert np.abs(f).max() <= 131070 * 1.7320508075688772 / 65536.0
    if key:
        assert not np.array_equal(f, PR.noise_field(0, 64, 64))


def test_restatement_on_the_identity_row_returns_the_inputs_bits():
    rs = np.random.RandomState(0)
    src = rs.random_sample((2, 9, 7, 3)).astype(np.float32)
    src[0, 0, 0] = (0.0, 1.0, 1e-40)                             # zero, one and a denormal
    out = PR.photometric_batch(src, np.tile(Photometric.identity(), (2, 1)))
    assert out.dtype == np.float32 and out.tobytes() == src.tobytes()


def test_restatement_blur_preserves_a_constant_and_spreads_a_point():
    r, w = Photometric.kernel(1.5)
    row = Photometric.identity()
    row[14], row[16:32] = r, w
    flat = np.full((6, 4, 3), 0.25, np.float32)
    assert np.abs(PR.photometric_image(flat, row) - 0.25).max() < 1e-7          # r = 5 on a 6 x 4 frame: reflection wraps
    point = np.zeros((21, 21, 3), np.float32)
    point[10, 10] = 1.0
    out = PR.photometric_image(point, row).astype(np.float64)
    full = np.concatenate([w[r:0:-1], w[:r + 1]])
    assert np.allclose(out[5:16, 5:16, 0], np.outer(full, full), rtol=1e-6, atol=1e-12) and out[:5].max() == 0
    # the bound clamps the radius and leaves the weights as they are
    assert PR.photometric_image(point, row, max_radius=2)[10, 7:14, 0].tolist() == [0] + (w[0] * np.array([w[2], w[1], w[0], w[1], w[2]])).astype(np.float32).tolist() + [0]


def test_train_refuses_what_is_not_a_photometric_and_takes_it_by_keyword_only():
    import inspect
    from myolo.augment import Augmentation
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO
    par = inspect.signature(MaskYOLO.train).parameters
    assert par["photometric"].kind is inspect.Parameter.KEYWORD_ONLY and par["photometric"].default is None
    model = MaskYOLO.__new__(MaskYOLO)                          # the check comes before anything touches a dataset or a device
    model.config = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=4)
    model._resumed = False
    for bad in (Augmentation(), object(), 0.5):
        with pytest.raises(TypeError, match="myolo.augment.Photometric"):
            model.train(None, None, 1e-3, 1, "all", photometric=bad)


def test_photometric_rows_give_plain_sources_the_identity():
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO

    class DS(object):
        image_info = [{"source": "a"}, {"source": "b"}, {"source": "a"}]
    model = MaskYOLO.__new__(MaskYOLO)
    model.config = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=4)
    p = Photometric(seed=4, **WIDE)
    rows = model.photometric_rows(p, ["b"], DS, 2, [2, 1, 0])
    assert rows.shape == (3, 32) and rows[1].tobytes() == Photometric.identity().tobytes()
    assert rows[0].tobytes() == p.row(2, 2).tobytes() and rows[2].tobytes() == p.row(2, 0).tobytes()
    assert model.photometric_rows(p, None, DS, 2, [1])[0].tobytes() == p.row(2, 1).tobytes()
    check_photo_rows(rows, 3)
    a = Photometric.around(hue=10, saturation=.3, contrast=2, blur=1.5, noise=.02, seed=3)
    assert (a.hue, a.saturation, a.contrast, a.blur, a.noise, a.seed) == ((-10, 10), (.7, 1.3), (0, 3), (0, 1.5), (0, .02), 3)


def test_build_list_compiles_the_unit_without_contraction():
    import __graft_entry__ as G
    assert ("photometric_kernels.hip", ["-ffp-contract=off"]) in G.UNITS

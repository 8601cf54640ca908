"""Host side of the mosaic augmentation (myolo.augment.Mosaic): the plan, the tile geometry, the composed rows against their restatement
(tests/mosaic_ref.py), the argument checks and the C-ABI declaration."""
import os
import re

import numpy as np
import pytest

import mosaic_ref as M
from myolo.augment import Augmentation, IDENTITY_TILE, Mosaic, check_mosaic_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_plan_is_a_pure_function_of_seed_epoch_and_image_ids():
    m = Mosaic(seed=3)
    ids = [17, 4, 9, 30, 2]
    base = m.plan(2, ids, 96, 64)
    src, tiles, centre = base
    assert src.dtype == np.int32 and src.shape == (5, 4) and tiles.dtype == np.float64 and tiles.shape == (5, 4, 6)
    assert centre.dtype == np.int32 and centre.shape == (5, 2)
    assert _same(base, m.plan(2, ids, 96, 64)) and _same(base, Mosaic(seed=3).plan(2, ids, 96, 64))      # no hidden state
    m.plan(0, [1, 2], 96, 64)                                                                        # other plans in between change nothing
    assert _same(base, m.plan(2, ids, 96, 64))
    for other in (Mosaic(seed=4).plan(2, ids, 96, 64), m.plan(3, ids, 96, 64), m.plan(2, [18] + ids[1:], 96, 64)):
        assert not _same(base, other)
    # a sample's own draws do not depend on its neighbours: position 1 keeps its centre and zooms when another image id changes
    other = m.plan(2, [18] + ids[1:], 96, 64)
    assert other[2][1].tolist() == centre[1].tolist() and other[1][1, :, 0].tolist() == tiles[1, :, 0].tolist()
    # tile 0 is the sample itself, partners are batch positions, centres leave every tile a pixel, zooms are inside their range
    assert src[:, 0].tolist() == [0, 1, 2, 3, 4] and ((src >= 0) & (src < 5)).all()
    assert (centre[:, 0] >= 1).all() and (centre[:, 0] <= 63).all() and (centre[:, 1] >= 1).all() and (centre[:, 1] <= 95).all()
    assert (tiles[:, :, 0] >= 1.0).all() and (tiles[:, :, 0] <= 2.0).all() and (tiles[:, :, 0] == tiles[:, :, 4]).all()
    assert (tiles[:, :, 1] == 0).all() and (tiles[:, :, 3] == 0).all()


def test_the_ranges_do_not_change_the_draws():
    """the same number of draws in the same order whatever the ranges: fixing the zoom leaves centres and partners where they were"""
    a = Mosaic(seed=5).plan(1, list(range(8)), 64, 64)
    b = Mosaic(seed=5, zoom=(1., 1.)).plan(1, list(range(8)), 64, 64)
    assert _same((a[0], a[2]), (b[0], b[2])) and not _same((a[1],), (b[1],))
    c = Mosaic(seed=5, centre=(.5, .5)).plan(1, list(range(8)), 64, 64)
    assert c[2].tolist() == [[32, 32]] * 8 and _same((a[0],), (c[0],)) and (a[1][:, :, 0] == c[1][:, :, 0]).all()


def test_p_zero_is_all_self_and_compose_returns_the_rows():
    src, tiles, centre = Mosaic(p=0.0, seed=1).plan(0, [5, 6, 7], 48, 80)
    assert src.tolist() == [[0] * 4, [1] * 4, [2] * 4] and centre.tolist() == [[80, 48]] * 3
    assert tiles.tobytes() == np.tile(IDENTITY_TILE, (3, 4, 1)).tobytes()
    aug = Augmentation(seed=2, **FULL)
    rows = np.stack([aug.params(0, i, 48, 80) for i in (5, 6, 7)])
    rows[1, 0] = -0.0                                           # the bit pattern is kept, not only the value
    got = Mosaic.compose(tiles, src, rows)
    assert got.shape == (3, 4, 8) and got.tobytes() == np.repeat(rows[:, None, :], 4, axis=1).tobytes()


def test_compose_equals_its_restatement_and_inverts_both_maps():
    H, W = 64, 96
    m = Mosaic(seed=7)
    src, tiles, centre = m.plan(4, [3, 1, 4, 1, 5], H, W)
    aug = Augmentation(seed=2, **FULL)
    rows = np.stack([aug.params(4, i, H, W) for i in (3, 1, 4, 1, 5)])
    got = Mosaic.compose(tiles, src, rows)
    assert got.tobytes() == M.compose(tiles, src, rows).tobytes()
    for b in range(5):
        for q in range(4):
            r, a = rows[src[b, q]], tiles[b, q]
            out = np.array([13., 29.])
            u = np.array([a[0] * out[0] + a[1] * out[1] + a[2], a[3] * out[0] + a[4] * out[1] + a[5]])        # position in the tile image's frame
            want = np.array([r[0] * u[0] + r[1] * u[1] + r[2], r[3] * u[0] + r[4] * u[1] + r[5]])
            p = got[b, q]
            np.testing.assert_allclose([p[0] * out[0] + p[1] * out[1] + p[2], p[3] * out[0] + p[4] * out[1] + p[5]], want, rtol=0, atol=1e-9)
            assert p[6] == r[6] and p[7] == r[7]


@pytest.mark.parametrize("B", [1, 3])
def test_small_batches_give_valid_plans(B):
    src, tiles, centre = Mosaic(seed=2).plan(0, list(range(10, 10 + B)), 64, 64)
    assert src.shape == (B, 4) and ((src >= 0) & (src < B)).all() and src[:, 0].tolist() == list(range(B))
    assert ((centre >= 1) & (centre <= 63)).all()
    check_mosaic_tables(src, centre, B, 64, 64)
    if B == 1:
        assert src.tolist() == [[0, 0, 0, 0]]                       # the sample is its own partner three times


def test_eligible_positions():
    m = Mosaic(seed=9)
    ids = list(range(40, 48))
    src, tiles, centre = m.plan(0, ids, 64, 64, eligible=[1, 2, 5, 6])
    for b in range(8):
        if b in (1, 2, 5, 6):
            assert centre[b].tolist() != [64, 64] and set(src[b, 1:].tolist()) <= {1, 2, 5, 6} and src[b, 0] == b
        else:                                                   # not eligible: not mosaicked, and nobody's partner
            assert src[b].tolist() == [b] * 4 and centre[b].tolist() == [64, 64] and tiles[b].tobytes() == np.tile(IDENTITY_TILE, (4, 1)).tobytes()
    # the partner is eligible[floor(u * len(eligible))]: the draws of the all-positions plan, re-indexed
    full = m.plan(0, ids, 64, 64)
    for b in (1, 2, 5, 6):
        for q in (1, 2, 3):
            u = np.random.RandomState([9, 0, ids[b]]).random_sample(Mosaic.DRAWS)[2 + q]
            assert full[0][b, q] == int(u * 8) and src[b, q] == [1, 2, 5, 6][int(u * 4)]
        assert full[2][b].tolist() == centre[b].tolist()
    none = m.plan(0, ids, 64, 64, eligible=[])
    assert none[0].tolist() == [[b] * 4 for b in range(8)] and none[2].tolist() == [[64, 64]] * 8
    with pytest.raises(ValueError):
        m.plan(0, ids, 64, 64, eligible=[8])


def test_centre_clamp():
    lo = Mosaic(centre=(0., 0.)).plan(0, [1, 2, 3], 40, 56)[2]
    hi = Mosaic(centre=(1., 1.)).plan(0, [1, 2, 3], 40, 56)[2]
    assert lo.tolist() == [[1, 1]] * 3 and hi.tolist() == [[55, 39]] * 3


def test_known_answer_tiles():
    """zoom 1, the cut at mid-frame: every tile pins its image's facing corner pixel to the cut, exactly"""
    H, W = 48, 64
    src, tiles, centre = Mosaic(centre=(.5, .5), zoom=(1., 1.)).plan(0, [0, 1, 2, 3], H, W)
    cx, cy = centre[0]
    assert (cx, cy) == (W // 2, H // 2)

    def at(q, x, y):
        a = tiles[0, q]
        return ((a[0] * x + a[1] * y) + a[2], (a[3] * x + a[4] * y) + a[5])
    assert at(0, cx - 1, cy - 1) == (W - 1, H - 1)              # tile 0 shows its image's bottom-right corner
    assert at(1, cx, cy - 1) == (0, H - 1)                      # tile 1 its bottom-left
    assert at(2, cx - 1, cy) == (W - 1, 0)                      # tile 2 its top-right
    assert at(3, cx, cy) == (0, 0)                              # tile 3 its top-left
    # zoom 0.5: the image shrinks, so a step of one output pixel is two source pixels, about the same pinned corner
    t = Mosaic(centre=(.5, .5), zoom=(.5, .5)).plan(0, [0], H, W)[1][0, 0]
    assert t[0] == 2.0 and (t[0] * (cx - 0.5) + t[2], t[4] * (cy - 0.5) + t[5]) == (W - 0.5, H - 0.5)


@pytest.mark.parametrize("kw", [dict(p=1.5), dict(p=-.1), dict(centre=(-.1, .5)), dict(centre=(.5, 1.1)), dict(centre=(.7, .3)), dict(centre=.5),
                                dict(zoom=(0., 1.)), dict(zoom=(1.2, .8)), dict(zoom=(1.,)), dict(zoom=(1., float("nan"))), dict(seed=-1)])
def test_bad_ranges_raise(kw):
    with pytest.raises(ValueError):
        Mosaic(**kw)


def test_table_check_refuses_bad_sources_and_centres():
    src, centre = np.zeros((2, 4), np.int32), np.array([[3, 3], [8, 6]], np.int32)
    check_mosaic_tables(src, centre, 2, 6, 8)                   # (W, H) itself is allowed: "not mosaicked"
    for bad_src, bad_centre in ((np.full((2, 4), 2), centre), (np.full((2, 4), -1), centre), (src, np.array([[3, 3], [9, 6]])),
                                (src, np.array([[3, 7], [8, 6]])), (src, np.array([[-1, 3], [8, 6]])), (src[:1], centre)):
        with pytest.raises(ValueError, match="mosaic tables"):
            check_mosaic_tables(bad_src, bad_centre, 2, 6, 8)


def test_train_refuses_what_is_not_a_mosaic():
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO
    assert MaskYOLO.train.__code__.co_varnames[:MaskYOLO.train.__code__.co_argcount][-1] == "mosaic"      # the new keyword comes last
    model = MaskYOLO.__new__(MaskYOLO)                          # the check comes before anything touches a dataset or a device
    model.config = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=4)
    with pytest.raises(TypeError, match="myolo.augment.Mosaic"):
        model.train(None, None, 1e-3, 1, "all", mosaic=Augmentation())


def test_mosaic_tables_skip_plain_sources():
    """MaskYOLO.mosaic_tables: the plan of the batch's image ids; a sample from no_augmentation_sources is neither mosaicked nor a partner"""
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO

    class DS(object):
        image_info = [dict(source="plain" if i in (1, 4) else "shapes") for i in range(6)]
    model = MaskYOLO.__new__(MaskYOLO)
    model.config = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=4)
    m = Mosaic(seed=1)
    ids = [5, 4, 0, 1]
    got = model.mosaic_tables(m, ["plain"], DS, 2, ids)
    assert _same(got, m.plan(2, ids, 64, 64, eligible=[0, 2]))
    assert got[0][1].tolist() == [1] * 4 and got[0][3].tolist() == [3] * 4 and set(got[0][[0, 2], 1:].ravel().tolist()) <= {0, 2}
    assert _same(model.mosaic_tables(m, None, DS, 2, ids), m.plan(2, ids, 64, 64))


def test_symbol_is_declared_bound_and_exported():
    from myolo import _ext as X
    txt = open(os.path.join(ROOT, "include", "myolo_hip_internal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = dict(re.findall(r"\b(?:int|size_t)\s+(myolo_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S))
    assert len(X.SIGS["myolo_mosaic_batch"]) == decl["myolo_mosaic_batch"].count(",") + 1 == 25
    assert decl["myolo_mosaic_batch_ws_bytes"].count(",") + 1 == 2
    ops = open(os.path.join(ROOT, "include", "myolo_hip.h")).read()
    assert "myolo_mosaic_batch" not in ops                      # the operator header is full
    lib = X.load()
    assert hasattr(lib, "myolo_mosaic_batch") and "myolo_mosaic_batch_ws_bytes" in X.exported_symbols()
    # four candidates per slot: five statistics and a slot index each
    assert X.mosaic_ws_bytes(3, 5) == 3 * 4 * 5 * 6 * 4 == 4 * X.augment_ws_bytes(3, 5) and X.mosaic_ws_bytes(0, 5) == 0
    assert lib.myolo_mosaic_batch(*[None if t is X.P else 0 for t in X.SIGS["myolo_mosaic_batch"]]) == -1
    assert lib.myolo_last_error_string().startswith(b"mosaic_batch:")

"""Host side of the copy-paste augmentation (myolo.augment.CopyPaste): the plan and its draws, the table check, train()'s keyword, the C-ABI
declaration, and the numpy restatement of the device contract (tests/copy_paste_ref.py) on cases made by hand."""
import inspect
import os
import re

import numpy as np
import pytest

import copy_paste_ref as CP
from myolo.augment import CopyPaste, Mosaic, check_paste_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHORS = np.array([0.6, 0.7, 1.4, 1.2], np.float64)


def _same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _draws(seed, epoch, image_id):
    return np.random.RandomState([seed, epoch, image_id, 2]).random_sample(CopyPaste.DRAWS)


@pytest.mark.parametrize("kw", [dict(p=1.5), dict(p=-.1), dict(instances=1.01), dict(instances=-1e-9), dict(seed=-1), dict(seed=2 ** 32),
                                dict(p=float("nan"))])
def test_bad_arguments_raise(kw):
    with pytest.raises(ValueError):
        CopyPaste(**kw)


def test_defaults_and_repr():
    c = CopyPaste()
    assert (c.p, c.instances, c.seed) == (0.5, 0.5, 0) and repr(c) == "CopyPaste(p=0.5, instances=0.5, seed=0)"
    assert CopyPaste.DRAWS == 34
    for T in (0, 33):
        with pytest.raises(ValueError):
            c.plan(0, [1, 2], T)


def test_plan_is_a_pure_function_of_its_arguments():
    c = CopyPaste(p=1.0, seed=3)
    ids = [17, 4, 9, 30, 2]
    base = c.plan(2, ids, 10)
    donor, select = base
    assert donor.dtype == np.int32 and donor.shape == (5,) and select.dtype == np.int32 and select.shape == (5,)
    assert _same(base, c.plan(2, ids, 10)) and _same(base, CopyPaste(p=1.0, seed=3).plan(2, ids, 10))     # no hidden state
    c.plan(0, [1, 2], 4)
    assert _same(base, c.plan(2, ids, 10))
    for other in (CopyPaste(p=1.0, seed=4).plan(2, ids, 10), c.plan(3, ids, 10), c.plan(2, [18] + ids[1:], 10)):
        assert not _same(base, other)
    assert ((donor >= 0) & (donor < 5)).all() and (donor != np.arange(5)).all()                     # p = 1: everyone takes, never from itself
    check_paste_tables(donor, select, 5, 10)
    # the stated draws: u0 turns the paste on, u1 picks among the others in batch order, u[2+t] < instances sets bit t
    for b, i in enumerate(ids):
        u = _draws(3, 2, i)
        others = [e for e in range(5) if e != b]
        assert donor[b] == others[int(u[1] * 4)]
        assert int(select[b]) == sum(1 << t for t in range(10) if u[2 + t] < 0.5)
    # the stream is not Augmentation's or Mosaic's: their first draws come from RandomState([seed, epoch, id])
    assert _draws(3, 2, 17)[0] != np.random.RandomState([3, 2, 17]).random_sample(1)[0]


def test_p_and_instances_do_not_move_another_samples_draws():
    """always 34 draws per sample, each from its own stream: the ranges change what a draw means, never which draw a sample gets"""
    ids = list(range(40, 48))
    a = CopyPaste(p=1.0, instances=0.5, seed=5).plan(1, ids, 8)
    b = CopyPaste(p=1.0, instances=0.9, seed=5).plan(1, ids, 8)
    assert _same((a[0],), (b[0],)) and not _same((a[1],), (b[1],))
    assert all(int(x) & int(y) == int(x) for x, y in zip(a[1], b[1]))                               # a higher probability only adds bits
    c = CopyPaste(p=0.5, instances=0.5, seed=5).plan(1, ids, 8)
    on = [_draws(5, 1, i)[0] < 0.5 for i in ids]
    assert any(on) and not all(on)
    for k in range(8):
        if on[k]:
            assert c[0][k] == a[0][k] and c[1][k] == a[1][k]
        else:
            assert c[0][k] == k and c[1][k] == 0
    # T only cuts the pattern; T = 32 reaches the sign bit for some sample
    t4 = CopyPaste(p=1.0, seed=5).plan(1, ids, 4)
    assert _same((t4[0],), (a[0],)) and [int(s) for s in t4[1]] == [int(s) & 15 for s in a[1]]
    t32 = CopyPaste(p=1.0, instances=1.0, seed=5).plan(1, ids, 32)
    assert (t32[1] == -1).all()
    check_paste_tables(t32[0], t32[1], 8, 32)
    zero = CopyPaste(p=1.0, instances=0.0, seed=5).plan(1, ids, 8)
    assert _same((zero[0],), (a[0],)) and (zero[1] == 0).all()


def test_eligible_positions():
    c = CopyPaste(p=1.0, instances=1.0, seed=9)
    ids = list(range(40, 48))
    donor, select = c.plan(0, ids, 6, eligible=[1, 2, 5, 6])
    for b in range(8):
        if b in (1, 2, 5, 6):
            others = [e for e in (1, 2, 5, 6) if e != b]
            assert donor[b] == others[int(_draws(9, 0, ids[b])[1] * 3)] and select[b] == 63
        else:                                                   # not eligible: receives nothing, and nobody takes from it
            assert donor[b] == b and select[b] == 0
    assert set(donor[[1, 2, 5, 6]].tolist()) <= {1, 2, 5, 6}
    none = c.plan(0, ids, 6, eligible=[])
    assert none[0].tolist() == list(range(8)) and (none[1] == 0).all()
    with pytest.raises(ValueError):
        c.plan(0, ids, 6, eligible=[8])


def test_a_single_eligible_position_gives_identity_tables():
    c = CopyPaste(p=1.0, instances=1.0, seed=1)
    for got in (c.plan(0, [7], 5), c.plan(0, [7, 8, 9], 5, eligible=[1])):
        assert got[0].tolist() == list(range(len(got[0]))) and (got[1] == 0).all()
    assert CopyPaste(p=0.0).plan(0, [1, 2, 3], 5)[0].tolist() == [0, 1, 2] and (CopyPaste(p=0.0).plan(0, [1, 2, 3], 5)[1] == 0).all()


def test_table_check_refusals():
    donor, select = np.array([1, 0, 1], np.int32), np.array([0, 7, 4], np.int32)
    check_paste_tables(donor, select, 3, 3)
    check_paste_tables(np.array([0], np.int32), np.array([-1], np.int32), 1, 32)                   # bit 31 with T = 32
    bad = ((np.array([1, 0, 3], np.int32), select, 3, 3), (np.array([1, 0, -1], np.int32), select, 3, 3), (donor, np.array([0, 8, 4], np.int32), 3, 3),
           (donor, np.array([0, -1, 4], np.int32), 3, 31), (donor[:2], select, 3, 3), (donor, select[:2], 3, 3), (donor[:, None], select, 3, 3),
           (donor, select, 4, 3), (donor.astype(np.float64), select, 3, 3))
    for d, s, B, T in bad:
        with pytest.raises(ValueError, match="copy-paste tables: "):
            check_paste_tables(d, s, B, T)


def test_train_refuses_what_is_not_a_copy_paste_and_takes_it_by_keyword_only():
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO
    par = inspect.signature(MaskYOLO.train).parameters
    assert par["copy_paste"].kind is inspect.Parameter.KEYWORD_ONLY and par["copy_paste"].default is None
    assert list(par)[-1] == "copy_paste" and par["mosaic"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    model = MaskYOLO.__new__(MaskYOLO)                          # the check comes before anything touches a dataset or a device
    model.config = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=4)
    for bad in (Mosaic(), object(), 0.5):
        with pytest.raises(TypeError, match="myolo.augment.CopyPaste"):
            model.train(None, None, 1e-3, 1, "all", copy_paste=bad)
    with pytest.raises(TypeError):
        model.train(None, None, 1e-3, 1, "all", None, None, None, None, 1, 0, True, None, CopyPaste())      # not positional


def test_paste_tables_skip_plain_sources():
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO

    class DS(object):
        image_info = [dict(source="plain" if i in (1, 4) else "shapes") for i in range(6)]
    model = MaskYOLO.__new__(MaskYOLO)
    model.config = make_config(ShapesConfig, IMAGE_SHAPE=[64, 64, 3], BATCH_SIZE=4)
    T = model.config.TRUE_BOX_BUFFER
    c = CopyPaste(p=1.0, instances=1.0, seed=1)
    ids = [5, 4, 0, 1]
    got = model.paste_tables(c, ["plain"], DS, 2, ids)
    assert _same(got, c.plan(2, ids, T, eligible=[0, 2]))
    assert got[0].tolist() == [2, 1, 0, 3] and got[1][1] == 0 and got[1][3] == 0 and got[1][0] != 0
    assert _same(model.paste_tables(c, None, DS, 2, ids), c.plan(2, ids, T))


def test_symbol_is_declared_bound_and_exported():
    from myolo import _ext as X
    txt = open(os.path.join(ROOT, "include", "myolo_hip_internal.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = dict(re.findall(r"\b(?:int|size_t)\s+(myolo_\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S))
    assert len(X.SIGS["myolo_copy_paste_batch"]) == decl["myolo_copy_paste_batch"].count(",") + 1 == 23
    assert decl["myolo_copy_paste_batch_ws_bytes"].count(",") + 1 == 2
    assert "myolo_copy_paste_batch" not in open(os.path.join(ROOT, "include", "myolo_hip.h")).read()      # the operator header stays as it is
    lib = X.load()
    assert hasattr(lib, "myolo_copy_paste_batch") and "myolo_copy_paste_batch_ws_bytes" in X.exported_symbols()
    # two candidates per slot: five statistics and a slot index each
    assert X.copy_paste_ws_bytes(3, 5) == 3 * 2 * 5 * 6 * 4 == 2 * X.augment_ws_bytes(3, 5) and X.copy_paste_ws_bytes(0, 5) == 0
    assert lib.myolo_copy_paste_batch(*[None if t is X.P else 0 for t in X.SIGS["myolo_copy_paste_batch"]]) == -1
    assert lib.myolo_last_error_string() == b"copy_paste_batch: null pointer"


# ---------------------------------------------------------------- the restatement, on cases made by hand
def _rect_scene(T, rects):
    """8 x 8 images, image i a constant i + 1; rects: {(image, slot): (y0, y1, x0, x1, class id)}"""
    B = 1 + max(i for i, _ in rects)
    images = np.stack([np.full((8, 8, 3), i + 1, np.float32) for i in range(B)])
    masks, ids = np.zeros((B, 8, 8, T), np.uint8), np.zeros((B, T), np.int32)
    for (i, t), (y0, y1, x0, x1, cls) in rects.items():
        masks[i, y0:y1, x0:x1, t], ids[i, t] = 1, cls
    return images, masks, ids


def _run(images, masks, ids, donor, select):
    T = masks.shape[-1]
    return CP.copy_paste_batch(images, masks, ids, np.asarray(donor, np.int32), np.asarray(select, np.int32), 8, 8, T, 2, 2, 8, ANCHORS)


def test_restatement_full_receiver():
    """F = 0: every selected live instance is counted, none is pasted, and the image and its labels stay what they were"""
    images, masks, ids = _rect_scene(2, {(0, 0): (0, 3, 0, 3, 1), (0, 1): (4, 8, 4, 8, 2), (1, 0): (1, 6, 1, 6, 3), (1, 1): (0, 8, 0, 2, 4)})
    out = _run(images, masks, ids, [1, 1], [3, 0])
    assert out["dropped"].tolist() == [2, 0]
    assert out["images"].tobytes() == images.tobytes() and out["gt_masks"].tobytes() == masks.tobytes() and out["gt_ids"].tobytes() == ids.tobytes()
    assert out["gt_boxes"][0].tolist() == [[0, 0, 3, 3], [4, 4, 8, 8]]
    assert out["true_boxes"][0, 0].tolist() == [0.375, 0.375, 0.75, 0.75]


def test_restatement_partially_free_receiver():
    """T = 4, two own instances: of the donor's selected live slots 0, 2, 3 the first two are accepted, in ascending slot order; slot 3 is counted and
    its pixels stay out of the image"""
    images, masks, ids = _rect_scene(4, {(0, 0): (0, 2, 0, 2, 1), (0, 1): (6, 8, 0, 2, 2),
                                         (1, 0): (0, 2, 6, 8, 3), (1, 1): (3, 4, 3, 4, 4), (1, 2): (3, 5, 6, 8, 5), (1, 3): (6, 8, 6, 8, 6)})
    out = _run(images, masks, ids, [1, 1], [0b1101, 0])
    assert out["dropped"].tolist() == [1, 0]
    assert out["gt_ids"][0].tolist() == [1, 2, 3, 5]
    assert out["gt_boxes"][0].tolist() == [[0, 0, 2, 2], [0, 6, 2, 8], [6, 0, 8, 2], [6, 3, 8, 5]]
    img = out["images"][0, :, :, 0]
    assert (img[0:2, 6:8] == 2).all() and (img[3:5, 6:8] == 2).all() and (img[6:8, 6:8] == 1).all() and (img[3, 3] == 1)
    assert (img == 2).sum() == 8
    assert out["gt_masks"][0].sum(axis=(0, 1)).tolist() == [4, 4, 4, 4]
    assert out["gt_ids"][1].tolist() == [3, 4, 5, 6] and out["images"][1].tobytes() == images[1].tobytes()


def test_restatement_covered_own_instance_and_dead_donor_slots():
    """an own instance wholly under the paste is dropped, the later slots move up, and it is not counted; another loses part of its box; selected
    donor slots whose class id is 0 are ignored though their mask has pixels"""
    images, masks, ids = _rect_scene(4, {(0, 0): (2, 4, 2, 4, 1), (0, 1): (0, 8, 6, 8, 2), (0, 2): (6, 8, 0, 2, 7),
                                         (1, 0): (1, 5, 1, 7, 3)})
    masks[1, :, :, 2] = 1                                       # dead: set pixels, class id 0
    out = _run(images, masks, ids, [1, 0], [0b0101, 0b1000])
    assert out["dropped"].tolist() == [0, 0]
    assert out["gt_ids"][0].tolist() == [2, 7, 3, 0]
    assert out["gt_boxes"][0].tolist() == [[6, 0, 8, 8], [0, 6, 2, 8], [1, 1, 7, 5], [0, 0, 0, 0]]         # the strip keeps its box: rows 0 and 5..7 remain
    assert out["gt_masks"][0].sum(axis=(0, 1)).tolist() == [16 - 4, 4, 24, 0]
    assert (out["images"][0, :, :, 1] == 2).sum() == 24
    # image 1 selected slot 3 of image 0, which is dead: nothing happens to it -- its own dead slot stays out of the labels as before
    assert out["gt_ids"][1].tolist() == [3, 0, 0, 0] and out["gt_masks"][1, :, :, 1:].sum() == 0 and out["images"][1].tobytes() == images[1].tobytes()
    # a donor outside the batch is nobody
    out = _run(images, masks, ids, [2, -1], [0b0101, 0b0001])
    assert out["dropped"].tolist() == [0, 0] and out["images"].tobytes() == images.tobytes() and out["gt_ids"][0].tolist() == [1, 2, 7, 0]

"""detect()'s selection on the device: myolo_select_detections against the numpy restatement of its contract
(tests/select_ref.py) -- sel and count integer for integer, picked bit for bit -- on the cases a selection can get wrong, its refusals, and
Net.select_detections at K = 10 against the host's detect.Selection."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X                                            # noqa: E402
from myolo import detect as D                                          # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.engine import Net                                           # noqa: E402
from select_ref import clustered_det, select_ref                       # noqa: E402

DEV = "cuda"
SENTINEL = 0x5A5A5A5A
KS = (1, 10, 16, 17, 40, 128)


def _run(det, n_live, K, cs_threshold, shape, nms_threshold=0.7):
    """the entry itself, through ctypes (no engine), on outputs pre-filled with SENTINEL -> sel, picked, count (numpy)"""
    B, R = det.shape[:2]
    dd = torch.as_tensor(np.ascontiguousarray(det), device=DEV)
    sel = torch.full((B, K), SENTINEL, dtype=torch.int32, device=DEV)
    picked = torch.full((B, K, 6), SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    X.call("myolo_select_detections", X.ptr(dd), B, R, n_live, K, float(cs_threshold), float(nms_threshold), int(shape[0]), int(shape[1]),
           X.ptr(sel), X.ptr(picked), X.ptr(count), X.stream())
    torch.cuda.synchronize()
    return sel.cpu().numpy(), picked.cpu().numpy().view(np.float32), count.cpu().numpy()


def _check(det, n_live, K, cs_threshold, shape, nms_threshold=0.7):
    want = select_ref(det, n_live, K, cs_threshold, shape, nms_threshold)
    got = _run(det, n_live, K, cs_threshold, shape, nms_threshold)
    what = (det.shape, n_live, K, cs_threshold, tuple(shape), nms_threshold)
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what
    return got


@pytest.mark.parametrize("R", [1, 7, 147, 845, 1280])
def test_sizes_equal_the_reference(R):
    """B in {1, 3} x every K (K > R included), two thresholds: one workgroup per image, 2 .. 2048 keys in the sort, rows without area and rows
    with both extents negative among them"""
    rng = np.random.default_rng(9000 + R)
    suppressed = under = 0
    for B in (1, 3):
        det = clustered_det(rng, B, R)
        live = ((det[:, :, 2] - det[:, :, 0]) * (det[:, :, 3] - det[:, :, 1]) > 0).sum(axis=1)
        area = (det[:, :, 2] - det[:, :, 0]) * (det[:, :, 3] - det[:, :, 1]) > 0
        ranked = np.sort(det[0, area[0], 4])[::-1] if area[0].any() else np.zeros(1, np.float32)
        for K in KS:
            _, _, c0 = _check(det, B, K, 0.0, [224, 224, 3])
            # ... and a threshold that IS a score (the >= at equality), halfway down image 0's first K
            _, _, c5 = _check(det, B, K, float(ranked[min(K, len(ranked)) // 2]), [224, 224, 3])
            suppressed += int((np.minimum(live, K) - c0).sum())
            under += int((c0 - c5).sum())
    if R >= 147:
        assert suppressed > 0 and under > 0                              # NMB and the threshold both had rows to drop


def test_the_largest_call():
    """R = 4096 and K = 128: every key slot and every candidate slot in use"""
    det = clustered_det(np.random.default_rng(4096), 2, 4096, dead=0.05)
    _, _, count = _check(det, 2, 128, 0.25, [416, 416, 3])
    assert 16 < count.max() <= 128


def test_padding_images_get_only_their_empty_slots():
    det = clustered_det(np.random.default_rng(1), 3, 147)
    for n_live in (0, 1, 2):
        sel, picked, count = _check(det, n_live, 40, 0.0, [224, 224, 3])
        assert (sel[n_live:] == -1).all() and not picked[n_live:].view(np.uint32).any() and not count[n_live:].any()
        assert (count[:n_live] > 0).all()


def test_a_non_square_image_shape():
    """image_shape (96, 64) and (64, 96): x scales by image_shape[0] and y by image_shape[1].  (An IoU does not change when an axis is scaled, and
    with float32 corners and small integer factors every product and difference up to the two areas is exact in binary64, so both orders give
    the same doubles: the case holds the kernel to the reference at a shape whose factors differ, it cannot tell the orders apart.)"""
    det = clustered_det(np.random.default_rng(2), 3, 147)
    for shape in ((96, 64), (64, 96), (97, 61)):
        for K in (10, 40):
            _, _, count = _check(det, 3, K, 0.0, shape)
            assert (count < np.minimum(K, 100)).any()


def test_rows_without_area_and_with_negative_extents():
    det = np.zeros((1, 7, 6), np.float32)
    det[0, 0] = (0.1, 0.1, 0.1, 0.5, 0.99, 1)          # zero width
    det[0, 1] = (0.1, 0.1, 0.5, 0.1, 0.98, 1)          # zero height
    det[0, 2] = (0.5, 0.1, 0.1, 0.5, 0.97, 1)          # one negative extent
    det[0, 3] = (0.9, 0.9, 0.6, 0.7, 0.96, 1)          # both negative: live
    det[0, 4] = (0.0, 0.0, 0.0, 0.0, 0.95, 1)          # the zero row the forward leaves for a cell under its threshold
    det[0, 5] = (0.2, 0.2, 0.4, 0.4, 0.10, 1)
    det[0, 6] = (0.6, 0.1, 0.8, 0.3, 0.20, 0)
    sel, _, count = _check(det, 1, 10, 0.0, [224, 224, 3])
    assert sel[0, :3].tolist() == [3, 6, 5] and count[0] == 3
    dead = det.copy()
    dead[0, [3, 5, 6], 2] = dead[0, [3, 5, 6], 0]
    assert _check(dead, 1, 10, 0.0, [224, 224, 3])[2].tolist() == [0]    # no live row at all


def test_every_score_under_the_threshold():
    det = clustered_det(np.random.default_rng(3), 2, 147)
    sel, picked, count = _check(det, 2, 40, 1.5, [224, 224, 3])
    assert (sel == -1).all() and not count.any() and not picked.view(np.uint32).any()


def test_one_class_one_box_keeps_the_first():
    det = np.zeros((2, 50, 6), np.float32)
    det[:, :, :4] = (0.25, 0.25, 0.75, 0.5)
    det[:, :, 4] = np.linspace(0.1, 0.9, 50, dtype=np.float32)
    det[:, :, 5] = 2
    for K in (1, 17, 128):
        sel, _, count = _check(det, 2, K, 0.0, [224, 224, 3])
        assert count.tolist() == [1, 1] and sel[:, 0].tolist() == [49, 49]


def test_the_chain_is_not_greedy():
    """A suppresses B; B and C overlap at 0.739; A and C at 0.538: a greedy suppression would keep C, NMB drops it (B, though dropped, still
    suppresses)"""
    det = np.zeros((1, 3, 6), np.float32)
    det[0, 0] = (0.000, 0.0, 0.500, 0.5, 0.9, 1)
    det[0, 1] = (0.075, 0.0, 0.575, 0.5, 0.8, 1)
    det[0, 2] = (0.150, 0.0, 0.650, 0.5, 0.7, 1)
    sel, _, count = _check(det, 1, 10, 0.0, [224, 224, 3])
    assert sel[0, :2].tolist() == [0, -1] and count[0] == 1
    other = det.copy()
    other[0, 1, 5] = 3                                                  # B of another class: nothing suppresses C
    assert _check(other, 1, 10, 0.0, [224, 224, 3])[0][0, :4].tolist() == [0, 1, 2, -1]


def test_equal_scores_take_the_higher_row_first():
    rng = np.random.default_rng(4)
    det = clustered_det(rng, 2, 147)
    det[:, :, 4] = rng.integers(1, 6, (2, 147)).astype(np.float32) / 8            # five score values: long runs of ties
    det[1, ::3, 4] = 0.0
    det[1, 1::6, 4] = -0.0                                                         # -0 ties with +0
    for K in (10, 40, 128):
        sel, _, count = _check(det, 2, K, 0.0, [224, 224, 3])
    five = np.zeros((1, 5, 6), np.float32)
    for r in range(5):
        five[0, r] = (0.18 * r, 0.0, 0.18 * r + 0.1, 0.1, 0.5, 1)
    assert _check(five, 1, 8, 0.0, [64, 64, 3])[0][0].tolist() == [4, 3, 2, 1, 0, -1, -1, -1]
    assert _check(five, 1, 3, 0.0, [64, 64, 3])[0][0].tolist() == [4, 3, 2]


def test_an_iou_that_equals_the_threshold():
    """[0,0,.5,1] and [0,0,.5,.75]: IoU = 0.75 exactly -- suppressed at nms_threshold 0.75 (>=), kept at the next double above it"""
    det = np.zeros((1, 2, 6), np.float32)
    det[0, 0] = (0.0, 0.0, 0.5, 1.0, 0.9, 1)
    det[0, 1] = (0.0, 0.0, 0.5, 0.75, 0.8, 1)
    for shape in ([64, 64, 3], [96, 64, 3], [224, 224, 3]):
        assert _check(det, 1, 10, 0.0, shape, nms_threshold=0.75)[2].tolist() == [1]
        assert _check(det, 1, 10, 0.0, shape, nms_threshold=float(np.nextafter(0.75, 1.0)))[2].tolist() == [2]
    # ... and a score that equals the threshold is kept, one a float32 step under it is not
    det[0, 1, :4] = (0.6, 0.0, 0.9, 0.5)
    det[0, 1, 4] = 0.35                                                 # float32(0.35) = 0.3499999940...
    assert _check(det, 1, 10, float(np.float32(0.35)), [64, 64, 3])[2].tolist() == [2]
    assert _check(det, 1, 10, 0.35, [64, 64, 3])[2].tolist() == [1]


def test_class_ids():
    """ids 0, 1 and 80, and the truncation of a fractional id: 1.9 is class 1"""
    det = np.zeros((1, 6, 6), np.float32)
    det[0, :, :4] = (0.25, 0.25, 0.75, 0.5)
    det[0, :, 4] = (0.9, 0.8, 0.7, 0.6, 0.5, 0.4)
    det[0, :, 5] = (0, 1, 80, 80, 1.9, 0)
    sel, picked, count = _check(det, 1, 10, 0.0, [224, 224, 3])
    assert sel[0, :4].tolist() == [0, 1, 2, -1] and picked[0, :3, 5].tolist() == [0.0, 1.0, 80.0]


def test_two_runs_bit_identical():
    det = clustered_det(np.random.default_rng(6), 3, 845)
    a, b = _run(det, 3, 128, 0.1, [416, 416, 3]), _run(det, 3, 128, 0.1, [416, 416, 3])
    assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def test_refusals():
    lib = X.load()
    det = torch.as_tensor(clustered_det(np.random.default_rng(7), 2, 4097), device=DEV)
    sel = torch.full((2, 129), SENTINEL, dtype=torch.int32, device=DEV)
    picked = torch.full((2, 129, 6), SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    null = ctypes.c_void_p(None)

    def call(**kw):
        a = dict(det=X.ptr(det), B=2, R=147, n_live=2, K=10, cs=0.0, nms=0.7, s0=224, s1=224, sel=X.ptr(sel), picked=X.ptr(picked),
                 count=X.ptr(count), stream=X.stream())
        a.update(kw)
        return lib.myolo_select_detections(*a.values())
    for kw in (dict(K=0), dict(K=129), dict(K=-1), dict(R=4097), dict(R=0), dict(n_live=3), dict(n_live=-1), dict(B=0, n_live=0), dict(det=null),
               dict(sel=null), dict(picked=null), dict(count=null)):
        assert call(**kw) == -1, kw
        assert lib.myolo_last_error_string().startswith(b"select_detections:"), (kw, lib.myolo_last_error_string())
    torch.cuda.synchronize()
    assert (sel == SENTINEL).all() and (picked == SENTINEL).all() and (count == SENTINEL).all()      # nothing was launched
    assert call(K=128, R=4096) == 0
    torch.cuda.synchronize()
    assert (sel.reshape(-1)[2 * 128:] == SENTINEL).all() and (picked.reshape(-1)[2 * 128 * 6:] == SENTINEL).all()      # K = 128 wrote [2,128]


# ------------------------------------------------------------------------------------------------ the engine
def test_net_select_detections_equals_the_host_selection():
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4)
    net = Net(cfg)
    det = clustered_det(np.random.default_rng(8), 4, 147)
    dd = torch.as_tensor(det, device=DEV)
    for shape, thr in (([128, 128, 3], 0.0), ([96, 64, 3], 0.5)):
        host = D.Selection(det, 3, thr, shape)
        sel, picked = net.select_detections(dd, 3, 10, thr, shape)
        assert sel.dtype == np.int32 and picked.dtype == np.float32 and sel.shape == (4, 10) and picked.shape == (4, 10, 6)
        dev = D.Selection.from_device(sel, picked, 3)
        assert np.array_equal(dev.sel, host.sel) and dev.n == host.n
        for k in range(3):
            for a, b in zip(dev.picked[k], host.picked[k]):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    # the pinned buffer is the Net's and is reused; the arrays handed out are copies
    first = net.select_detections(dd, 4, 40, 0.0, [128, 128, 3])
    keep = [a.copy() for a in first]
    pin = net._select_pin
    net.select_detections(dd, 4, 16, 0.9, [128, 128, 3])
    assert net._select_pin is pin and pin.is_pinned() and all(np.array_equal(a, b) for a, b in zip(first, keep))
    want = select_ref(det, 4, 40, 0.0, [128, 128, 3])
    assert np.array_equal(first[0], want[0]) and np.array_equal(first[1].view(np.uint32), want[1].view(np.uint32))
    assert (want[2] > 16).any()
    with pytest.raises(RuntimeError, match="select_detections: need 1 <= K <= 128"):
        net.select_detections(dd, 4, 129, 0.0, [128, 128, 3])
    with pytest.raises(ValueError):
        net.select_detections(dd[0], 1, 10, 0.0, [128, 128, 3])

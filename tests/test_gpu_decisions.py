"""The decision kernels of csrc/exact_kernels.hip against the oracle on the edge tables of tests/decision_cases.py ("Edge tables of the
exact kernels"; tests/test_decision_cases_host.py proves that every case sits on its edge).  Integer decisions and the floats that feed them are
compared with np.array_equal / ==; only the float loss terms and gradient carry the project's 1e-4 bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decision_cases as DC                         # noqa: E402
from myolo import _ext as X                         # noqa: E402

DEV = "cuda:0"
_KEEP = []   # device tensors must outlive the asynchronous kernel that reads them


@pytest.fixture(autouse=True)
def _keepalive():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dt(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device=DEV)                 # a copy: the tables are read-only
    t = t if dtype is None else t.to(dtype)
    _KEEP.append(t)
    return t


def new(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=DEV)


def _same_bits(a, b):
    """equal as float32 bit patterns: tells -0 from +0 and a subnormal from 0"""
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


# ------------------------------------------------------------------------------------------------------------------------------------------
# targets
# ------------------------------------------------------------------------------------------------------------------------------------------
def _run_targets(c):
    B, R, T, size = c["B"], c["R"], c["T"], c["size"]
    rois, tcls = new(B, R, 4), new(B, R, dtype=torch.int32)
    tmask, npos = new(B, R, DC.MASK, DC.MASK), new(B, dtype=torch.int32)
    X.call("myolo_mask_targets", X.ptr(dt(c["prop"])), X.ptr(dt(c["gt_ids"])), X.ptr(dt(c["gt_boxes"])), X.ptr(dt(c["gt_masks"].view(np.uint8))),
           X.ptr(rois), X.ptr(tcls), X.ptr(tmask), X.ptr(npos), B, R, T, size, size, DC.MASK, DC.MASK, X.stream())
    return rois.cpu().numpy(), tcls.cpu().numpy(), tmask.cpu().numpy(), npos.cpu().numpy()


@pytest.mark.parametrize("name", DC.TARGET_NAMES)
def test_mask_targets_edge_case(name):
    c = DC.target_case(name)
    want = DC.target_reference(name)
    got = _run_targets(c)
    for what, g, w in zip(("rois", "target_class_ids", "target_masks", "n_pos"), got, want):
        print("%s %s: %d of %d entries differ" % (name, what, int((g != w).sum()) if g.shape == w.shape else -1, w.size))
    assert np.array_equal(got[3], want[3]), "n_pos: %s, oracle %s (%s)" % (got[3], want[3], c["edge"])
    assert np.array_equal(got[0], want[0]), "rois (%s)" % c["edge"]
    assert np.array_equal(got[1], want[1]), "target_class_ids (%s)" % c["edge"]
    assert np.array_equal(got[2], want[2]), "target_masks (%s)" % c["edge"]
    again = _run_targets(c)
    assert all(_same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(got, again)), "two runs differ"


# ------------------------------------------------------------------------------------------------------------------------------------------
# decode and detections
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in DC.DECODE_SHAPES])
def test_yolo_decode_edge_case(name):
    c = DC.decode_case(name)
    B, G, A, C = c["B"], c["G"], c["A"], c["C"]
    want_prop, want_det = DC.decode_reference(name)
    prop, det = new(B, G * G * A, 4), new(B, G * G * A, 6)
    yp, anchors = dt(c["y_pred"]), dt(c["anchors"])
    X.call("myolo_yolo_decode", X.ptr(yp), X.ptr(anchors), X.ptr(prop), B, G, A, C, X.stream())
    X.call("myolo_yolo_detections", X.ptr(yp), X.ptr(anchors), X.ptr(det), B, G, A, C, X.stream())
    prop, det = prop.cpu().numpy(), det.cpu().numpy()
    bad = prop != want_prop
    print("%s proposals: %d of %d differ" % (name, int(bad.sum()), bad.size))
    bad = det != want_det
    print("%s detections: %d of %d differ; by column %s" % (name, int(bad.sum()), bad.size, bad.reshape(-1, 6).sum(0).tolist()))
    conf, wconf = det[..., 4], want_det[..., 4]
    tiny = np.finfo(np.float32).tiny
    print("%s subnormal confidences: %d, oracle %d" % (name, int(((conf > 0) & (conf < tiny)).sum()), int(((wconf > 0) & (wconf < tiny)).sum())))
    assert np.array_equal(prop, want_prop), "proposals not bit-exact"
    assert np.array_equal(det, want_det), "detections not bit-exact"
    assert np.array_equal(det[..., :4], prop)
    assert np.array_equal(det[..., 5].astype(np.int64), np.argmax(c["y_pred"][..., 5:], -1).reshape(B, -1)), "class column is not np.argmax"


# ------------------------------------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------------------------------------
TERMS = ("loss", "loss_xy", "loss_wh", "loss_conf", "loss_class", "recall", "n_coord", "n_conf")
LOSS_NAMES = tuple(s[0] for s in DC.LOSS_SHAPES)


def _run_loss(c, warm, loss_weight=1.0, entry="myolo_yolo_loss_warmup"):
    cfg, B, G, A, C, T = c["cfg"], c["B"], c["G"], c["A"], c["C"], c["T"]
    terms, grad = new(8), new(*c["y_pred"].shape)
    args = (X.ptr(dt(c["y_true"])), X.ptr(dt(c["y_pred"])), X.ptr(dt(c["true_boxes"].reshape(B, T, 4))), X.ptr(dt(np.asarray(cfg.ANCHORS, np.float32))),
            X.ptr(dt(np.asarray(cfg.CLASS_WEIGHTS, np.float32))), cfg.OBJECT_SCALE, cfg.NO_OBJECT_SCALE, cfg.COORD_SCALE, cfg.CLASS_SCALE, loss_weight)
    flag = (int(warm),) if entry == "myolo_yolo_loss_warmup" else ()
    X.call(entry, *args, *flag, X.ptr(terms), X.ptr(grad), B, G, A, C, T, 0, 0, X.stream())
    return terms.cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize("name", LOSS_NAMES)
@pytest.mark.parametrize("warm", [0, 1])
def test_yolo_loss_edge_case(name, warm):
    c, ref = DC.loss_case(name), DC.loss_reference(name, warm)
    t, grad = _run_loss(c, warm)
    for i, k in enumerate(TERMS):
        print("%s warm %d %-10s %.9g oracle %.9g" % (name, warm, k, t[i], float(ref[k])))
    gmax = max(1.0, float(np.abs(ref["grad"]).max()))
    gerr = float(np.abs(grad.astype(np.float64) - ref["grad"]).max()) / gmax
    print("%s warm %d gradient: rel err %.3e of max %.3e" % (name, warm, gerr, gmax))
    # the counts are integer decisions: exact
    assert t[6] == float(ref["n_coord"]), ("n_coord", t[6], ref["n_coord"])
    assert t[7] == float(ref["n_conf"]), ("n_conf", t[7], ref["n_conf"])
    assert abs(float(t[5]) - float(ref["recall"])) <= 1e-6, ("recall", t[5], ref["recall"])
    for i, k in enumerate(TERMS[:5]):
        assert abs(t[i] - float(ref[k])) <= 1e-4 * max(1.0, abs(float(ref[k]))), (k, t[i], ref[k])
    assert np.isfinite(grad).all() and gerr <= 1e-4, "gradient: rel err %.3e" % gerr
    if name == "no_object":
        assert (grad[..., 5:] == 0).all(), "class gradients without an object must be exactly 0"
        if not warm:
            assert (grad[..., 0:4] == 0).all(), "coordinate gradients without an object must be exactly 0 outside warm-up"


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_yolo_loss_weight_and_entries(name):
    """loss_weight = 0.5 halves the gradient bit for bit (a power of two) and leaves the terms; warmup=0 is myolo_yolo_loss bit for bit"""
    c = DC.loss_case(name)
    for warm in (0, 1):
        t1, g1 = _run_loss(c, warm, 1.0)
        th, gh = _run_loss(c, warm, 0.5)
        assert _same_bits(th, t1), "the terms depend on loss_weight"
        assert _same_bits(gh, g1 * np.float32(0.5)), "gradient at 0.5 is not half the gradient at 1.0"
    t0, g0 = _run_loss(c, 0, 1.0)
    tp, gp = _run_loss(c, 0, 1.0, entry="myolo_yolo_loss")
    assert _same_bits(t0, tp) and _same_bits(g0, gp), "myolo_yolo_loss_warmup(warmup=0) != myolo_yolo_loss"

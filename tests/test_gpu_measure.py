"""Measurements of the detected instances, taken on the device: myolo_measure_masks against measure.measure_dense of the
bytes the existing paste (myolo_unmold_masks) writes for the same rows -- integer for integer, no tolerance -- over the crafted rows of
tests/test_gpu_rle.py, degenerate and mixed frames, every K up to 128 and the frames at which 32-bit sums wrap and the coordinates reach their
limit; its buffer and refusal contracts; and detect / detect_many(measure=True) against their own dense masks.  The only comparison with a
tolerance is that of the float64 fields of "measurements" with properties(measure_dense(...)), at rtol 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X                                            # noqa: E402
from myolo import measure as M                                         # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402
from test_gpu_rle import R, _case, _paste, _picture                    # noqa: E402  (the crafted rows and the paste oracle of the run-length tests)

DEV = "cuda"
MH = MW = 28
WORDS = 13
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64                  # words behind out that must come back untouched
FLOAT_FIELDS = ("centroid", "major_axis_length", "minor_axis_length", "orientation", "eccentricity")


# ------------------------------------------------------------------------------------------------ the entry against the existing paste
def _measure_case(B, K, C, frames, seed):
    """test_gpu_rle's case (every fourth slot empty, the middle image of three without a live slot) with one row repeated: the last live slot of
    image 0 takes the row of its first (visible_area 0 there)"""
    masks, det, sel, frames = _case(B, K, C, frames, seed)
    live = np.flatnonzero(sel[0] >= 0)
    if live.size >= 2:
        sel[0, live[-1]] = sel[0, live[0]]
    return masks, det, sel, frames


class Call(object):
    """one myolo_measure_masks call through ctypes (no engine) on buffers this object owns: out [B*K*13 + GUARD] int64 pre-filled with SENTINEL,
    the workspace carved out of a larger allocation (ws_fill, the bytes behind ws_bytes a guard of 0xA5)."""

    def __init__(self, masks, det, sel, frames, ws_bytes=None, ws_fill=0xFF):
        self.B, self.K = sel.shape
        self.R, self.C = masks.shape[1], masks.shape[4]
        self.frames_h, self.sel_h = np.ascontiguousarray(frames, np.int32), np.ascontiguousarray(sel, np.int32)
        self.md, self.dd, self.sd, self.fd = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (masks, det, self.sel_h, self.frames_h))
        self.n = self.B * self.K * WORDS
        self.out_d = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
        self.need = X.measure_masks_ws_bytes(self.B, self.K)
        self.ws_bytes = self.need if ws_bytes is None else int(ws_bytes)
        self.ws = torch.full((self.ws_bytes + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ws[:self.ws_bytes] = ws_fill

    def args(self, **kw):
        a = dict(masks=X.ptr(self.md), det=X.ptr(self.dd), sel=X.ptr(self.sd), sel_host=self.sel_h.ctypes.data, frames=X.ptr(self.fd),
                 frames_host=self.frames_h.ctypes.data, out=X.ptr(self.out_d), B=self.B, R=self.R, K=self.K, mh=MH, mw=MW, C=self.C,
                 ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes, stream=X.stream())
        a.update(kw)
        return list(a.values())

    def run(self):
        X.call("myolo_measure_masks", *self.args())
        return self.out()

    def out(self):
        """-> the records [B,K,13]; the words behind them are checked here"""
        torch.cuda.synchronize()
        flat = self.out_d.cpu().numpy()
        assert (flat[self.n:] == SENTINEL).all(), "words behind out were written"
        return flat[:self.n].reshape(self.B, self.K, WORDS)

    def guard_intact(self):
        return bool((self.ws[self.ws_bytes:] == 0xA5).all())


def _check(masks, det, sel, frames, got):
    """every slot against measure_dense of the dense paste of the image's live rows, in slot order; -> the number of live slots"""
    B, K = sel.shape
    assert got.shape == (B, K, WORDS) and got.dtype == np.int64
    n = 0
    for b in range(B):
        H, W = int(frames[b, 0]), int(frames[b, 1])
        live = [k for k in range(K) if sel[b, k] >= 0]
        assert not got[b][[k for k in range(K) if sel[b, k] < 0]].any(), b
        if not live:
            continue
        want = M.measure_dense(_paste(masks[b], det[b], [sel[b, k] for k in live], H, W))
        for i, k in enumerate(live):
            assert got[b, k].tolist() == want[i].tolist(), (b, k, int(sel[b, k]), (H, W), dict(zip(M.FIELDS, zip(got[b, k], want[i]))))
        n += len(live)
    return n


def _crafted(got, sel, frames):
    """the crafted rows give what they were crafted for (so the case holds what it is meant to hold); -> the rows seen"""
    seen = set()
    B, K = sel.shape
    for b in range(B):
        H, W = int(frames[b, 0]), int(frames[b, 1])
        first = {}
        for k in range(K):
            r = int(sel[b, k])
            if r < 0:
                continue
            g = dict(zip(M.FIELDS, got[b, k].tolist()))
            seen.add(r)
            if r in first:
                assert g["visible_area"] == 0 and got[b, k, 2:].tolist() == got[b, first[r], 2:].tolist(), (b, k)       # a repeated row
            first.setdefault(r, k)
            if r == 0:                                                 # the full frame
                assert g["area"] == H * W and g["perimeter"] == 2 * (H + W) and g["quads"] == (H - 1) * (W - 1)
                assert [g[c] for c in ("x1", "y1", "x2", "y2")] == [0, 0, W, H]
                assert g["sxx"] == H * ((W - 1) * W * (2 * W - 1) // 6) and g["sxy"] == (W * (W - 1) // 2) * (H * (H - 1) // 2)
            elif r in (2, 6):
                assert not got[b, k].any()
            elif r == 3:
                assert got[b, k].tolist() == [1, g["visible_area"], 0, 0, 0, 0, 0, 4, 0, 0, 0, 1, 1]
            elif r == 4:
                assert g["area"] == 1 and [g[c] for c in ("x1", "y1", "x2", "y2")] == [W - 1, H - 1, W, H] and g["sxy"] == (W - 1) * (H - 1)
    return seen


FRAMES = [(70, 70), (1, 1), (1, 97), (97, 1), (33, 129)]


@pytest.mark.parametrize("frame", FRAMES, ids=["%dx%d" % f for f in FRAMES])
def test_frames_equal_the_paste(frame):
    """partial tiles; joints of 64 columns (33 x 129: two) and of 32 rows (70, 97, 33: the 33rd row alone in its tile) inside windows;
    degenerate frames of one row, one column, one pixel"""
    masks, det, sel, frames = _measure_case(2, 20, 4, [frame, frame], seed=sum(frame))           # 15 live slots an image: every row in each
    got = Call(masks, det, sel, frames).run()
    assert _check(masks, det, sel, frames, got) == 30
    assert _crafted(got, sel, frames) == set(range(R))


def test_mixed_frames_in_one_batch():
    frames = FRAMES + [(64, 128), (65, 65)]
    masks, det, sel, fr = _measure_case(len(frames), 10, 4, frames, seed=21)
    c = Call(masks, det, sel, fr)
    got = c.run()
    _check(masks, det, sel, fr, got)
    _crafted(got, sel, fr)
    assert c.guard_intact()


@pytest.mark.parametrize("C", [1, 4, 81])
@pytest.mark.parametrize("K", [1, 10, 16, 17, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_sizes_equal_the_paste(B, K, C):
    frames = [(70, 70), (33, 129), (97, 1)][:B]
    masks, det, sel, frames = _measure_case(B, K, C, frames, seed=100 * B + 10 * K + C)
    c = Call(masks, det, sel, frames)
    got = c.run()
    _check(masks, det, sel, frames, got)
    _crafted(got, sel, frames)
    assert c.guard_intact()
    if B == 3:
        assert not got[1].any()                                         # the image without a live slot
    if K >= 16:
        assert (got[0, :, 1] < got[0, :, 0]).any() and got[0, :, 1].sum() > 0          # slots hidden in part under earlier ones


@pytest.mark.parametrize("side", [416, 2048])
def test_sums_beyond_32_bits(side):
    """a full-frame all-high slot: sxx = side * sum x^2 and sxy = (sum x)^2 leave 32 bits (416: 1.0e10, 2048: 5.9e12 and 4.4e12)"""
    masks, det, _, frames = _case(1, 1, 4, [(side, side)], seed=side)
    sel = np.array([[0, 9, -1, 1, 0]], np.int32)                       # the full frame, a window partly outside, the bands, the full frame again
    got = Call(masks, det, sel, frames).run()
    _check(masks, det, sel, frames, got)
    _crafted(got, sel, frames)
    assert got[0, 0, 4] > 2 ** 32 and got[0, 0, 6] > 2 ** 32 and got[0, 4, 1] == 0


@pytest.mark.parametrize("frame", [(1, 32768), (32768, 1)], ids=["1x32768", "32768x1"])
def test_the_coordinate_limit(frame):
    masks, det, sel, frames = _measure_case(1, 10, 4, [frame], seed=9)
    got = Call(masks, det, sel, frames).run()
    _check(masks, det, sel, frames, got)
    assert 0 in _crafted(got, sel, frames)
    assert got[0, 0, 0] == 32768 and got[0, 0, 11:].tolist() == [frame[1], frame[0]] and got[0, 0, 4] + got[0, 0, 5] == 32767 * 32768 * 65535 // 6


def test_buffer_discipline():
    masks, det, sel, frames = _measure_case(2, 17, 4, [(33, 129), (70, 70)], seed=17)
    outs = []
    for fill in (0x00, 0xFF, 0xFF):
        c = Call(masks, det, sel, frames, ws_fill=fill)
        assert c.ws_bytes == X.measure_masks_ws_bytes(2, 17) >= 2 * 17 * 4
        outs.append(c.run())                                            # (out() checks the words behind out)
        assert (outs[-1] != SENTINEL).all() and c.guard_intact(), fill
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], outs[2])          # whatever the workspace held; two runs bit-identical
    _check(masks, det, sel, frames, outs[0])
    c = Call(masks, det, sel, frames)
    c.run()
    again = c.run()                                                     # onto the previous result: every word is written anew
    assert np.array_equal(again, outs[0])


def test_refusals():
    lib = X.load()
    masks, det, sel, frames = _measure_case(1, 10, 4, [(70, 70)], seed=3)
    c = Call(masks, det, sel, frames)
    assert getattr(lib, "myolo_measure_masks")(*c.args()) == 0
    torch.cuda.synchronize()
    c.out_d.fill_(SENTINEL)
    c.ws[:c.ws_bytes] = 0xFF                                            # (the accepted call has used its workspace)
    null = ctypes.c_void_p(None)
    bad_sel = c.sel_h.copy()
    bad_sel[0, 3] = R
    sel129 = np.full((1, 129), -1, np.int32)
    bad_frames = [np.array([hw], np.int32) for hw in ((0, 70), (70, 0), (32769, 70), (70, 32769), (-1, 5))]          # (the arrays outlive the calls)
    cases = [dict(masks=null), dict(det=null), dict(sel=null), dict(sel_host=null), dict(frames=null), dict(frames_host=null), dict(out=null),
             dict(ws=null), dict(B=0), dict(B=-1), dict(K=0), dict(K=129, sel_host=sel129.ctypes.data), dict(sel_host=bad_sel.ctypes.data),
             dict(ws_bytes=c.need - 1), dict(ws_bytes=0)] + [dict(frames_host=f.ctypes.data) for f in bad_frames]
    for kw in cases:
        assert getattr(lib, "myolo_measure_masks")(*c.args(**kw)) == -1, kw
        assert lib.myolo_last_error_string().startswith(b"measure_masks:"), (kw, lib.myolo_last_error_string())
    torch.cuda.synchronize()
    assert bool((c.out_d == SENTINEL).all()) and c.guard_intact() and bool((c.ws[:c.ws_bytes] == 0xFF).all())


# ------------------------------------------------------------------------------------------------ the public path
SEED = 4                    # of the random weights: with it image 0 below reports more than sixteen instances at max_detections=40 (asserted)
SIZES = ((224, 224), (224, 224), (200, 150), (224, 224), (61, 97), (224, 224))      # batch 2: whole batches at the frame and mixed ones
_STATE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the model this file shares is destroyed HERE, with the device idle -- not by a collection that happens to start inside a later test"""
    yield
    import gc
    _STATE.clear()
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _model():
    if "model" not in _STATE:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], ALPHA=0.5, BATCH_SIZE=2)
        _STATE["model"] = (cfg, MaskYOLO(mode="inference", config=cfg, seed=SEED))
    return _STATE["model"]


def _images():
    return [_picture(h, w, 30 + k) for k, (h, w) in enumerate(SIZES)]


def _results(**kw):
    """detect_many over the six images at cs_threshold 0, computed once per set of arguments and left unchanged"""
    key = tuple(sorted(kw.items()))
    if key not in _STATE:
        _STATE[key] = _model()[1].detect_many(_images(), cs_threshold=0.0, **kw)
    return _STATE[key]


def _equals_its_dense_masks(r, what):
    """the "measurements" of one result dict against the full_masks beside them"""
    p, n = r["measurements"], len(r["class_ids"])
    raw = M.measure_dense(r["full_masks"])
    assert p["raw"].dtype == np.int64 and p["raw"].shape == (n, WORDS) and np.array_equal(p["raw"], raw), what
    want = M.properties(raw)
    assert set(p) == set(want), what
    for key in ("area", "visible_area", "perimeter", "euler_number", "bbox"):
        assert p[key].dtype == want[key].dtype and np.array_equal(p[key], want[key]), (what, key)
    for key in FLOAT_FIELDS:
        np.testing.assert_allclose(p[key], want[key], rtol=1e-12, atol=0, equal_nan=True, err_msg="%s %s" % (what, key))
    return int(raw[:, 0].sum())


@pytest.mark.parametrize("frame", ["image", "network"])
def test_detect_many_measure_equals_the_dense_masks(frame):
    cfg, m = _model()
    imgs, got = _images(), _results(mask_frame=frame, measure=True)
    plain = _results(mask_frame=frame)
    assert len(got) == len(imgs) and sum(len(r["class_ids"]) for r in got) >= len(imgs)
    pixels = 0
    for k, (r, d) in enumerate(zip(got, plain)):
        assert set(r) == set(d) | {"measurements"} and "measurements" not in d, k             # measure=False: no such key
        for key in d:
            assert np.array_equal(r[key], d[key]), (k, key)
        size = imgs[k].shape[:2] if frame == "image" else tuple(cfg.IMAGE_SHAPE[:2])
        assert r["full_masks"].shape[:2] == size
        pixels += _equals_its_dense_masks(r, "image %d" % k)
    assert pixels > 0                                                   # not a comparison of empty masks


def _loop_length(loop):
    q = np.asarray(loop, np.int64)
    return int(np.abs(q - np.roll(q, -1, axis=0)).sum())


def test_rle_and_polygon_runs_give_the_same_records():
    dense = _results(mask_frame="image", measure=True)
    runs = _results(mask_format="rle", measure=True)
    polys = _results(mask_format="polygon", measure=True)
    plain = _results(mask_format="rle")
    for k, (d, r, p) in enumerate(zip(dense, runs, polys)):
        assert "full_masks" not in r and "full_masks" not in p and "measurements" not in plain[k]
        assert set(r) == set(plain[k]) | {"measurements"}, k
        for q in (r, p):
            assert np.array_equal(q["class_ids"], d["class_ids"]), k
            assert np.array_equal(q["measurements"]["raw"], d["measurements"]["raw"]), k
            for key in FLOAT_FIELDS:
                assert np.array_equal(q["measurements"][key], d["measurements"][key], equal_nan=True), (k, key)
        lengths = [sum(_loop_length(l) for l in loops) for loops in p["polygons"]]
        assert lengths == p["measurements"]["perimeter"].tolist(), k


def test_forty_detections_cross_the_blocks_of_sixteen():
    """the other consumers take 40 slots in column blocks of 16; visible_area ranks a slot against ALL earlier ones, across the blocks"""
    got = _results(max_detections=40, measure=True)
    assert len(got[0]["class_ids"]) > 16
    for k, r in enumerate(got):
        _equals_its_dense_masks(r, "image %d" % k)
    v, a = got[0]["measurements"]["visible_area"], got[0]["measurements"]["area"]
    assert (v[16:] < a[16:]).any()                                      # an instance behind the first block is hidden in part
    assert v.sum() == got[0]["full_masks"].any(axis=2).sum()
    runs = _results(max_detections=40, mask_format="rle", measure=True)
    for r, d in zip(runs, got):
        assert np.array_equal(r["measurements"]["raw"], d["measurements"]["raw"])


def test_detect_measure_and_render():
    cfg, m = _model()
    imgs = _images()
    for k in (0, 2, 4):
        one = m.detect(imgs[k], cs_threshold=0.0, measure=True)
        assert len(one) == 1 and "measurements" in one[0]
        _equals_its_dense_masks(one[0], "detect %d" % k)
        assert "measurements" not in m.detect(imgs[k], cs_threshold=0.0)[0]
    net = m.detect(imgs[2], cs_threshold=0.0, mask_frame="network", measure=True)[0]
    assert net["full_masks"].shape[:2] == tuple(cfg.IMAGE_SHAPE[:2])
    _equals_its_dense_masks(net, "network frame")
    drawn = m.detect(imgs[2], cs_threshold=0.0, render=True, save_path=None, mask_format="rle", measure=True)[0]
    ref = m.detect(imgs[2], cs_threshold=0.0, measure=True)[0]
    assert "rendered" in drawn and np.array_equal(drawn["measurements"]["raw"], ref["measurements"]["raw"])
    rows = M.table([ref], names=["p.png"], scale=0.5)
    assert len(rows) == len(ref["class_ids"]) and rows[0]["area"] == int(ref["measurements"]["area"][0]) * 0.25


def test_net_measure_masks_checks_its_arguments():
    cfg, m = _model()
    masks, det, sel, frames = _measure_case(2, 40, 4, [(70, 70), (33, 129)], seed=5)
    md, dd = torch.as_tensor(masks, device=DEV), torch.as_tensor(det, device=DEV)
    got = m.net.measure_masks(dd, md, sel, frames)
    assert got.dtype == np.int64 and got.shape == (2, 40, WORDS)
    _check(masks, det, sel, frames, got)
    with pytest.raises(ValueError):
        m.net.measure_masks(dd, md, sel.astype(np.int64), frames)
    with pytest.raises(ValueError):
        m.net.measure_masks(dd, md, sel, frames[:1])
    with pytest.raises(ValueError):
        m.net.measure_masks(dd, md, np.full((2, 129), -1, np.int32), frames)
    bad = sel.copy()
    bad[1, 0] = R
    with pytest.raises(RuntimeError, match="measure_masks: sel"):
        m.net.measure_masks(dd, md, bad, frames)
    cfg2 = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    m2 = MaskYOLO(mode="inference", config=cfg2, seed=4)
    with pytest.raises(ValueError):
        m2.detect(_picture(40, 30, 2), measure=True)
    with pytest.raises(ValueError):
        m2.detect_many([_picture(40, 30, 2)], measure=True)

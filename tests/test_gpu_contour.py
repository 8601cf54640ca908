"""Detection masks as polygons, traced on the device: myolo_contour_masks against contour.trace of the bytes of the existing
paste (myolo_unmold_masks), integer for integer -- vert_off, verts, loop_id -- its capacity, workspace and refusal contracts, and
detect / detect_many(mask_format="polygon") against their dense results."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_rle as RL                                              # noqa: E402  (the crafted detection rows, the paste oracle, the pictures)
from myolo import _ext as X                                            # noqa: E402
from myolo import contour                                              # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402

DEV = "cuda"
MH = MW = RL.MH
R = RL.R
SENTINEL = 0x5A5A5A5A
GUARD = 64                  # vertices behind cap that must come back untouched
RING, BLOBS = 11, 12        # rows of RL._rows replaced here (they are random there)
CAP = 1 << 14               # the capacity of the workspace tests: above their totals (a few thousand vertices), below the default


def _case(B, K, C, frames, seed):
    """RL._case (rows 0-10: the full window all-high / banded / all-low / as a checkerboard, one-pixel windows at either corner, an empty window,
    windows outside the frame and partly outside, an all-high window in the middle; every fourth slot empty) with two rows more: 11 a ring -- a
    mask with a hole -- and 12 two blobs in one mask, both in windows inside the frame."""
    masks, det, sel, frames = RL._case(B, K, C, frames, seed)
    yy, xx = np.mgrid[0:MH, 0:MW]
    rr = (yy - 13.5) ** 2 + (xx - 13.5) ** 2
    ring = ((rr <= 12.0 ** 2) & (rr >= 5.0 ** 2)).astype(np.float32)
    blobs = (((yy >= 3) & (yy < 12) & (xx >= 2) & (xx < 10)) | ((yy >= 15) & (yy < 26) & (xx >= 14) & (xx < 25))).astype(np.float32)
    for b in range(B):
        det[b, RING, :4] = (0.1, 0.1, 0.9, 0.9)
        det[b, BLOBS, :4] = (0.05, 0.1, 0.95, 0.8)
        masks[b, RING, :, :, int(det[b, RING, 5])] = ring
        masks[b, BLOBS, :, :, int(det[b, BLOBS, 5])] = blobs
    return masks, det, sel, frames


class Call(object):
    """one myolo_contour_masks call through ctypes (no engine) on buffers this object owns: vert_off [B*K+1], verts [cap + GUARD, 2] and loop_id
    [cap + GUARD] pre-filled with SENTINEL, the workspace carved out of a larger allocation (ws_fill, the bytes behind ws_bytes a guard of 0xA5)."""

    def __init__(self, masks, det, sel, frames, cap=1 << 16, ws_bytes=None, ws_fill=0xFF):
        self.B, self.K = sel.shape
        self.C = masks.shape[4]
        self.frames_h, self.sel_h = np.ascontiguousarray(frames, np.int32), np.ascontiguousarray(sel, np.int32)
        self.md, self.dd, self.sd, self.fd = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (masks, det, self.sel_h, self.frames_h))
        self.cap = int(cap)
        self.vert_off = torch.full((self.B * self.K + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        self.verts = torch.full((self.cap + GUARD, 2), SENTINEL, dtype=torch.int32, device=DEV)
        self.loop_id = torch.full((self.cap + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.need = X.contour_masks_ws_bytes(self.B, self.K, int(self.frames_h[:, 0].max()), int(self.frames_h[:, 1].max()), self.cap)
        self.ws_bytes = self.need if ws_bytes is None else int(ws_bytes)
        self.ws = torch.full((self.ws_bytes + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ws[:self.ws_bytes] = ws_fill

    def args(self, **kw):
        a = dict(masks=X.ptr(self.md), det=X.ptr(self.dd), sel=X.ptr(self.sd), sel_host=self.sel_h.ctypes.data, frames=X.ptr(self.fd),
                 frames_host=self.frames_h.ctypes.data, vert_off=X.ptr(self.vert_off), verts=X.ptr(self.verts), loop_id=X.ptr(self.loop_id),
                 cap=self.cap, B=self.B, R=R, K=self.K, mh=MH, mw=MW, C=self.C, ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes, stream=X.stream())
        a.update(kw)
        return list(a.values())

    def run(self):
        X.call("myolo_contour_masks", *self.args())
        return self.out()

    def out(self):
        torch.cuda.synchronize()
        return self.vert_off.cpu().numpy(), self.verts.cpu().numpy(), self.loop_id.cpu().numpy()

    def untouched(self):
        vert_off, verts, loop_id = self.out()
        return bool((vert_off == SENTINEL).all() and (verts == SENTINEL).all() and (loop_id == SENTINEL).all())

    def guard_intact(self):
        return bool((self.ws[self.ws_bytes:] == 0xA5).all())


def _check(masks, det, sel, frames, vert_off, verts, loop_id):
    """every slot against contour.trace of the dense paste, integer for integer; -> {(b, k): (loops, dense plane)}"""
    B, K = sel.shape
    assert vert_off[0] == 0 and (np.diff(vert_off.astype(np.int64)) >= 0).all()
    got = {}
    for b in range(B):
        H, W = int(frames[b, 0]), int(frames[b, 1])
        live = [k for k in range(K) if sel[b, k] >= 0]
        dense = RL._paste(masks[b], det[b], [sel[b, k] for k in live], H, W) if live else None
        for k in range(K):
            s = b * K + k
            lo, hi = int(vert_off[s]), int(vert_off[s + 1])
            if sel[b, k] < 0:
                assert hi == lo, (b, k)
                continue
            plane = dense[:, :, live.index(k)]
            want = contour.trace(plane)
            what = (b, k, int(sel[b, k]), (H, W))
            assert hi - lo == sum(len(l) for l in want), what
            if want:
                assert np.array_equal(verts[lo:hi], np.concatenate(want)), what
                assert np.array_equal(loop_id[lo:hi], np.repeat(np.arange(len(want)), [len(l) for l in want])), what
            got[(b, k)] = (want, plane)
    return got


def _crafted(got, sel, frames):
    """the crafted rows give what they were crafted for (so the case holds what it is meant to hold); -> the rows seen"""
    seen = set()
    for (b, k), (loops, plane) in got.items():
        r, H, W = int(sel[b, k]), int(frames[b, 0]), int(frames[b, 1])
        ll = [l.tolist() for l in loops]
        seen.add(r)
        if r == 0:
            assert ll == [[[0, 0], [W, 0], [W, H], [0, H]]]                   # touches all four edges of the frame
        elif r in (2, 6):
            assert ll == []
        elif r == 3:
            assert ll == [[[0, 0], [1, 0], [1, 1], [0, 1]]]
        elif r == 4:
            assert ll == [[[W - 1, H - 1], [W, H - 1], [W, H], [W - 1, H]]]
        elif r == 10:
            assert len(ll) == 1 and len(ll[0]) == 4 and ll[0][0][1] == 0 and ll[0][2][1] == H
        elif r == RING and min(H, W) >= 37:
            areas = [contour.signed_area(l) for l in loops]
            assert len(loops) == 2 and areas[0] > 0 > areas[1]
            assert loops[1][1][0] == loops[1][0][0] and loops[1][1][1] > loops[1][0][1]           # the hole leaves its first corner heading south
        elif r == BLOBS and min(H, W) >= 37:
            assert len(loops) == 2 and all(contour.signed_area(l) > 0 for l in loops)
    return seen


FRAMES = [(70, 70), (37, 91), (91, 37), (64, 5), (65, 5), (129, 3)]


@pytest.mark.parametrize("frame", FRAMES, ids=["%dx%d" % f for f in FRAMES])
def test_frames_equal_the_traced_paste(frame):
    """h x w frames: neither side a multiple of 64 / windows of exactly 64 and 65 rows / 129 rows by 3 columns (4 corner columns: one group of lanes
    barely used); 37 x 91 beside 91 x 37 catches a row / column swap and holds window rows of more than 64 corners (two groups of lanes, the carry)"""
    masks, det, sel, frames = _case(2, 10, 4, [frame, frame], seed=sum(frame))
    vert_off, verts, loop_id = Call(masks, det, sel, frames).run()
    seen = _crafted(_check(masks, det, sel, frames, vert_off, verts, loop_id), sel, frames)
    assert seen == set(range(R))


def test_mixed_frames_in_one_batch():
    frames = FRAMES + [(28, 28), (84, 56)]
    masks, det, sel, fr = _case(len(frames), 10, 4, frames, seed=21)
    c = Call(masks, det, sel, fr)
    vert_off, verts, loop_id = c.run()
    _crafted(_check(masks, det, sel, fr, vert_off, verts, loop_id), sel, fr)
    total = int(vert_off[-1])
    assert c.guard_intact() and (verts[total:] == SENTINEL).all() and (loop_id[total:] == SENTINEL).all()


def test_checkerboard_holds_the_most_vertices():
    """the 28 x 28 checkerboard pasted at scale 1 into a 28 x 28 frame: every set pixel is a loop of its own, four vertices each, two vertex edges at
    every inner corner; with an empty slot between two live ones"""
    rng = np.random.default_rng(2)
    masks, det = RL._rows(4, 28, 28, rng)
    sel = np.array([[8, -1, 8]], np.int32)
    frames = np.array([[28, 28]], np.int32)
    vert_off, verts, loop_id = Call(masks[None], det[None], sel, frames).run()
    got = _check(masks[None], det[None], sel, frames, vert_off, verts, loop_id)
    assert vert_off.tolist() == [0, 1568, 1568, 3136]
    loops, plane = got[(0, 0)]
    assert len(loops) == 392 == plane.sum() and all(len(l) == 4 for l in loops)
    assert loop_id[:1568].tolist() == np.repeat(np.arange(392), 4).tolist()


def test_ring_and_two_blobs_wide_frame():
    """a frame of 300 columns: window rows of five groups of 64 corners, straight stretches of more than 64 steps for the link pass"""
    masks, det, sel, frames = _case(1, 4, 4, [(45, 300)], seed=9)
    sel[0] = (RING, -1, BLOBS, 0)
    vert_off, verts, loop_id = Call(masks, det, sel, frames).run()
    got = _check(masks, det, sel, frames, vert_off, verts, loop_id)
    _crafted(got, sel, frames)
    assert len(got[(0, 0)][0]) == 2 and len(got[(0, 2)][0]) == 2 and got[(0, 3)][0][0].tolist() == [[0, 0], [300, 0], [300, 45], [0, 45]]


@pytest.mark.parametrize("C", [1, 81])
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_sizes_equal_the_traced_paste_70x70(B, K, C):
    masks, det, sel, frames = _case(B, K, C, [(70, 70)] * B, seed=100 * B + 10 * K + C)
    vert_off, verts, loop_id = Call(masks, det, sel, frames).run()
    _crafted(_check(masks, det, sel, frames, vert_off, verts, loop_id), sel, frames)
    if B == 3:
        assert vert_off[K] == vert_off[2 * K]                          # the image without a live slot


def test_two_runs_bit_identical():
    masks, det, sel, frames = _case(3, 10, 4, [(70, 70), (37, 91), (129, 3)], seed=11)
    a, b = Call(masks, det, sel, frames).run(), Call(masks, det, sel, frames, ws_fill=0x00).run()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_capacity_below_the_total():
    """cap smaller than the total: vert_off is complete and correct and no vertex is written anywhere; cap equal to the total: everything is there"""
    masks, det, sel, frames = _case(2, 10, 4, [(70, 70), (91, 37)], seed=13)
    full_off, full_v, full_l = Call(masks, det, sel, frames).run()
    total = int(full_off[-1])
    assert total > 400
    for cap in (total - 1, total // 2, 1, 0):
        c = Call(masks, det, sel, frames, cap=cap)
        vert_off, verts, loop_id = c.run()
        assert np.array_equal(vert_off, full_off), cap
        assert (verts == SENTINEL).all() and (loop_id == SENTINEL).all() and c.guard_intact(), cap
    c = Call(masks, det, sel, frames, cap=total)
    vert_off, verts, loop_id = c.run()
    assert np.array_equal(vert_off, full_off) and np.array_equal(verts[:total], full_v[:total]) and np.array_equal(loop_id[:total], full_l[:total])
    assert (verts[total:] == SENTINEL).all() and (loop_id[total:] == SENTINEL).all() and c.guard_intact()


def test_workspace_at_the_planner_figure():
    masks, det, sel, frames = _case(2, 10, 4, [(37, 91), (70, 70)], seed=17)
    outs = []
    for fill in (0x00, 0xFF):
        c = Call(masks, det, sel, frames, cap=CAP, ws_fill=fill)
        assert c.ws_bytes == X.contour_masks_ws_bytes(2, 10, 70, 91, CAP)
        outs.append(c.run())
        assert c.guard_intact(), fill
    assert all(np.array_equal(x, y) for x, y in zip(*outs))
    _check(masks, det, sel, frames, *outs[0])
    # the growth condition: at a fixed cap at most 64 * B * K bytes per extra row or column of the frame, so a 4000 x 3000 frame needs no dense plane
    base = X.contour_masks_ws_bytes(2, 10, 70, 91, CAP)
    for h, w in ((71, 91), (70, 92), (3000, 4000), (4000, 3000)):
        assert X.contour_masks_ws_bytes(2, 10, h, w, CAP) - base <= 64 * 2 * 10 * ((h - 70) + (w - 91)), (h, w)
    assert X.contour_masks_ws_bytes(2, 10, 3000, 4000, CAP) < 3000 * 4000
    # 16 bytes less, and a workspace planned for lower frames than the call's tallest: the error, no output written, the workspace as it was
    for short in (c.need - 16, X.contour_masks_ws_bytes(2, 10, 37, 91, CAP)):
        c = Call(masks, det, sel, frames, cap=CAP, ws_bytes=short)
        with pytest.raises(RuntimeError, match=r"contour_masks: workspace too small"):
            c.run()
        assert c.untouched() and c.guard_intact() and bool((c.ws[:c.ws_bytes] == 0xFF).all())


def test_refusals():
    lib = X.load()
    masks, det, sel, frames = _case(1, 10, 4, [(70, 70)], seed=3)
    c = Call(masks, det, sel, frames)
    assert getattr(lib, "myolo_contour_masks")(*c.args()) == 0
    torch.cuda.synchronize()
    c.vert_off.fill_(SENTINEL)
    c.verts.fill_(SENTINEL)
    c.loop_id.fill_(SENTINEL)
    null = ctypes.c_void_p(None)
    bad_sel = c.sel_h.copy()
    bad_sel[0, 3] = R
    sel17 = np.full((1, 17), -1, np.int32)
    # frames the entry must refuse: h < 1, w < 1, 2^31 pixels, and one taller than the workspace was planned for (the arrays outlive the calls)
    bad_frames = [np.array([hw], np.int32) for hw in ((0, 70), (70, 0), (65536, 32768), (200, 70))]
    cases = [dict(masks=null), dict(det=null), dict(sel=null), dict(sel_host=null), dict(frames=null), dict(frames_host=null), dict(vert_off=null),
             dict(verts=null), dict(loop_id=null), dict(ws=null), dict(K=17, sel_host=sel17.ctypes.data), dict(K=0),
             dict(sel_host=bad_sel.ctypes.data), dict(ws_bytes=c.need - 1), dict(cap=-1)] + [dict(frames_host=f.ctypes.data) for f in bad_frames]
    for kw in cases:
        assert getattr(lib, "myolo_contour_masks")(*c.args(**kw)) == -1, kw
        assert lib.myolo_last_error_string().startswith(b"contour_masks:"), (kw, lib.myolo_last_error_string())
    assert c.untouched()


# ------------------------------------------------------------------------------------------------ the public path
_MODELS = {}
_DENSE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the models this file shares are destroyed HERE, with the device idle -- not by a collection that happens to start inside a later test"""
    yield
    import gc
    _MODELS.clear()
    _DENSE.clear()
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _model(dtype):
    if dtype not in _MODELS:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4, INFERENCE_DTYPE=dtype)
        _MODELS[dtype] = (cfg, MaskYOLO(mode="inference", config=cfg, seed=4))
    return _MODELS[dtype]


def _dense(dtype, frame):
    """detect_many's dense results with the overlays, computed once per (dtype, frame) and left unchanged.  In the network frame render takes
    only images at IMAGE_SHAPE: those results carry no overlay."""
    if (dtype, frame) not in _DENSE:
        _DENSE[(dtype, frame)] = _model(dtype)[1].detect_many(RL._images(), cs_threshold=0.0, mask_frame=frame, render=frame == "image")
    return _DENSE[(dtype, frame)]


def _same_as_dense(r, d, what, rendered=False):
    assert set(r) == {"bboxes", "class_ids", "confidence_scores", "polygons"} | ({"rendered"} if rendered else set()), what
    for key in ("bboxes", "class_ids", "confidence_scores") + (("rendered",) if rendered else ()):
        assert r[key].shape == d[key].shape and r[key].dtype == d[key].dtype and np.array_equal(r[key], d[key]), (what, key)
    n = len(d["class_ids"])
    assert len(r["polygons"]) == n == d["full_masks"].shape[2], what
    for i, loops in enumerate(r["polygons"]):
        want = contour.trace(d["full_masks"][:, :, i])
        assert len(loops) == len(want), (what, i)
        for a, b in zip(loops, want):
            assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (what, i)


@pytest.mark.parametrize("frame", ["image", "network"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_detect_many_polygon_equals_dense(dtype, frame):
    cfg, m = _model(dtype)
    imgs, dense = RL._images(), _dense(dtype, frame)                    # six pictures, three of them not at IMAGE_SHAPE; a short last batch
    got = m.detect_many(imgs, cs_threshold=0.0, mask_frame=frame, mask_format="polygon")
    assert len(got) == len(imgs) == len(dense) and sum(len(r["class_ids"]) for r in got) >= len(imgs)
    for k, (r, d) in enumerate(zip(got, dense)):
        _same_as_dense(r, d, "image %d" % k)
    assert sum(len(l) for r in got for loops in r["polygons"] for l in loops) > 0          # not a comparison of empty masks
    if frame == "image":
        drawn = m.detect_many(imgs, cs_threshold=0.0, mask_format="polygon", render=True)
        for k, (r, d) in enumerate(zip(drawn, dense)):
            _same_as_dense(r, d, "rendered image %d" % k, rendered=True)
    # detect() itself: its dense result, and detect_many's entry
    for k in (0, 1, 5):
        one = m.detect(imgs[k], cs_threshold=0.0, mask_frame=frame, mask_format="polygon")
        assert len(one) == 1
        _same_as_dense(one[0], m.detect(imgs[k], cs_threshold=0.0, mask_frame=frame)[0], "detect %d" % k)
        _same_as_dense(one[0], dict(dense[k], **{key: got[k][key] for key in ("bboxes", "class_ids", "confidence_scores")}), "detect / many %d" % k)
    if frame == "image":
        one = m.detect(imgs[1], cs_threshold=0.0, mask_format="polygon", render=True, save_path=None)[0]
        _same_as_dense(one, m.detect(imgs[1], cs_threshold=0.0, render=True, save_path=None)[0], "detect rendered", rendered=True)


def test_forced_regrow_gives_the_same_result():
    """a Net whose vertex buffer starts at ONE element: the first call finds the total above the capacity, enlarges the buffer and calls again"""
    cfg, m = _model("fp32")
    imgs = RL._images()
    want = m.detect_many(imgs, cs_threshold=0.0, mask_format="polygon")
    m.net._contour_verts = torch.empty(3, dtype=torch.int32, device=m.net.dev)
    m.net._contour_ws = None
    got = m.detect_many(imgs, cs_threshold=0.0, mask_format="polygon")
    assert m.net._contour_verts.numel() > 3
    for k, (a, b) in enumerate(zip(got, want)):
        for key in ("bboxes", "class_ids", "confidence_scores"):
            assert np.array_equal(a[key], b[key]), (k, key)
        assert [[l.tolist() for l in loops] for loops in a["polygons"]] == [[l.tolist() for l in loops] for loops in b["polygons"]], k
    _same_as_dense(got[1], _dense("fp32", "image")[1], "regrown")


def test_mask_format_is_checked():
    cfg, m = _model("fp32")
    p = RL._picture(40, 30, 2)
    with pytest.raises(ValueError):
        m.detect(p, mask_format="png")
    assert "polygons" in m.detect(p, cs_threshold=0.0, mask_format="polygon")[0]
    cfg2 = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    m2 = MaskYOLO(mode="inference", config=cfg2, seed=4)
    with pytest.raises(ValueError, match="DETECT_MASKS_FOR_SELECTED_ONLY"):
        m2.detect(p, mask_format="polygon")
    with pytest.raises(ValueError, match="DETECT_MASKS_FOR_SELECTED_ONLY"):
        m2.detect_many([p], mask_format="polygon")


def test_net_contour_masks_checks_its_arguments():
    cfg, m = _model("fp32")
    masks, det, sel, frames = _case(2, 10, 4, [(70, 70), (37, 91)], seed=5)
    md, dd = torch.as_tensor(masks, device=DEV), torch.as_tensor(det, device=DEV)
    slots = m.net.contour_masks(dd, md, sel, frames)
    assert len(slots) == 20
    for b in range(2):
        live = [k for k in range(10) if sel[b, k] >= 0]
        dense = RL._paste(masks[b], det[b], [sel[b, k] for k in live], int(frames[b, 0]), int(frames[b, 1]))
        for k in range(10):
            want = contour.trace(dense[:, :, live.index(k)]) if k in live else []
            assert [l.tolist() for l in slots[b * 10 + k]] == [l.tolist() for l in want], (b, k)
    with pytest.raises(ValueError):
        m.net.contour_masks(dd, md, sel.astype(np.int64), frames)
    with pytest.raises(ValueError):
        m.net.contour_masks(dd, md, sel, frames[:1])
    bad = sel.copy()
    bad[1, 0] = R
    with pytest.raises(RuntimeError, match="contour_masks: sel"):
        m.net.contour_masks(dd, md, bad, frames)

"""Detection masks as COCO run-length codes, encoded on the device: myolo_rle_masks against the bytes of the existing paste
(myolo_unmold_masks) -- rle.decode(device) equals the dense paste bit for bit and the device's counts equal rle.encode(dense) integer for integer --
its capacity, workspace and refusal contracts, and detect / detect_many(mask_format="rle") against their dense results."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X                                            # noqa: E402
from myolo import rle                                                  # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402

DEV = "cuda"
MH = MW = 28
R = 14                      # detection rows per image in the kernel cases: 11 crafted ones (below) + 3 random
SENTINEL = 0x5A5A5A5A
GUARD = 64                  # words behind bounds + cap that must come back untouched


# ------------------------------------------------------------------------------------------------ the entry against the existing paste
def _rows(C, H, W, rng):
    """masks [R,28,28,C], det [R,6] of one image with an H x W frame.  Rows 0-10 are what a run-length walk can get wrong:
    0 the full-image window with an all-high mask (ONE run across every column joint: counts [0, N]); 1 a full-height window whose mask is high in
    its top and bottom bands only (runs that continue over the joints, with boundaries inside the columns); 2 the full window with an all-low mask
    ([N]); 3 a one-pixel window at pixel 0, 4 one at pixel N - 1 (all-high masks); 5 a zero-width window; 6 a window wholly outside the frame
    (beyond 1); 7 one wholly below 0 (the clamps leave pixel 0); 8 the full window with a 28 x 28 checkerboard; 9 a window partly outside the
    frame, random mask; 10 a full-height all-high window in the middle columns (one run over its joints); 11-13 random boxes and masks."""
    masks = rng.random((R, MH, MW, C), dtype=np.float32)
    det = np.zeros((R, 6), np.float32)
    lo = rng.random((R, 2)) * 0.7
    det[:, 0:2] = lo
    det[:, 2:4] = lo + 0.05 + rng.random((R, 2)) * 0.5
    det[:, 4] = rng.random(R)
    det[:, 5] = rng.integers(0, C, R)
    det[0, :4] = (0.0, 0.0, 1.0, 1.0)
    det[1, :4] = (0.2, 0.0, 0.9, 1.0)
    det[2, :4] = (0.0, 0.0, 1.0, 1.0)
    det[3, :4] = (0.0, 0.0, 1.2 / W, 1.2 / H)
    det[4, :4] = ((W - 0.8) / W, (H - 0.8) / H, 1.0, 1.0)
    det[5, :4] = (0.3, 0.2, 0.3, 0.8)
    det[6, :4] = (1.2, 1.1, 1.5, 1.6)
    det[7, :4] = (-0.5, -0.6, -0.2, -0.1)
    det[8, :4] = (0.0, 0.0, 1.0, 1.0)
    det[9, :4] = (-0.2, 0.4, 0.6, 1.3)
    det[10, :4] = (0.3, 0.0, 0.7, 1.0)
    yy, xx = np.mgrid[0:MH, 0:MW]
    bands = np.where((yy < 10) | (yy >= 18), 1.0, 0.0)
    for r, m in ((0, 0.5 + 0.5 * rng.random((MH, MW))), (1, bands), (2, 0.499 * rng.random((MH, MW))), (3, np.ones((MH, MW))),
                 (4, np.full((MH, MW), 0.5)), (8, (yy + xx) % 2), (10, 0.5 + 0.5 * rng.random((MH, MW)))):
        masks[r, :, :, int(det[r, 5])] = np.asarray(m, np.float32)
    return masks, det


def _case(B, K, C, frames, seed):
    """-> masks [B,R,28,28,C], det [B,R,6], sel [B,K] (-1 = empty), frames [B,2].  The live slots walk through the rows in an order that starts with
    the crafted ones; every fourth slot is empty (between live ones), and with B == 3 the middle image has no live slot at all."""
    rng = np.random.default_rng(seed)
    frames = np.asarray(frames, np.int32).reshape(B, 2)
    both = [_rows(C, int(h), int(w), rng) for h, w in frames]
    masks, det = np.stack([m for m, _ in both]), np.stack([d for _, d in both])
    sel = np.full((B, K), -1, np.int32)
    order = list(range(R))
    i = 0
    for b in range(B):
        if B == 3 and b == 1:
            continue
        for k in range(K):
            if K > 1 and k % 4 == 2:
                continue
            sel[b, k] = order[(i + seed) % R] if K == 1 else order[i % R]
            i += 1
    return masks, det, sel, frames


def _paste(masks_b, det_b, rows, H, W):
    """myolo_unmold_masks on the chosen rows of one image -> [H,W,n] bool: the oracle"""
    idx = torch.as_tensor(np.asarray(rows, np.int64), device=DEV)
    m = torch.as_tensor(masks_b, device=DEV).index_select(0, idx).contiguous()
    d = torch.as_tensor(det_b, device=DEV).index_select(0, idx).contiguous()
    n = len(rows)
    full = torch.empty(H, W, n, dtype=torch.uint8, device=DEV)
    ws = torch.empty(n, dtype=torch.int32, device=DEV)
    X.call("myolo_unmold_masks", X.ptr(m), X.ptr(d), X.ptr(full), n, MH, MW, int(m.shape[3]), H, W, ws.data_ptr(), ws.numel() * 4, X.stream())
    return full.cpu().numpy().astype(bool)


class Call(object):
    """one myolo_rle_masks call through ctypes (no engine) on buffers this object owns: run_off [B*K+1] and bounds [cap + GUARD] pre-filled with
    SENTINEL, the workspace carved out of a larger allocation (ws_fill, the bytes behind ws_bytes a guard of 0xA5)."""

    def __init__(self, masks, det, sel, frames, cap=1 << 16, ws_bytes=None, ws_fill=0xFF):
        self.B, self.K = sel.shape
        self.C = masks.shape[4]
        self.frames_h, self.sel_h = np.ascontiguousarray(frames, np.int32), np.ascontiguousarray(sel, np.int32)
        self.md, self.dd, self.sd, self.fd = (torch.as_tensor(np.ascontiguousarray(a), device=DEV) for a in (masks, det, self.sel_h, self.frames_h))
        self.cap = int(cap)
        self.run_off = torch.full((self.B * self.K + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        self.bounds = torch.full((self.cap + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.need = X.rle_masks_ws_bytes(self.B, self.K, int(self.frames_h[:, 1].max()))
        self.ws_bytes = self.need if ws_bytes is None else int(ws_bytes)
        self.ws = torch.full((self.ws_bytes + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
        self.ws[:self.ws_bytes] = ws_fill

    def args(self, **kw):
        a = dict(masks=X.ptr(self.md), det=X.ptr(self.dd), sel=X.ptr(self.sd), sel_host=self.sel_h.ctypes.data, frames=X.ptr(self.fd),
                 frames_host=self.frames_h.ctypes.data, run_off=X.ptr(self.run_off), bounds=X.ptr(self.bounds), cap=self.cap, B=self.B, R=R,
                 K=self.K, mh=MH, mw=MW, C=self.C, ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes, stream=X.stream())
        a.update(kw)
        return list(a.values())

    def run(self):
        X.call("myolo_rle_masks", *self.args())
        return self.out()

    def out(self):
        torch.cuda.synchronize()
        return self.run_off.cpu().numpy(), self.bounds.cpu().numpy().view(np.uint32)

    def guard_intact(self):
        return bool((self.ws[self.ws_bytes:] == 0xA5).all())


def _check(masks, det, sel, frames, run_off, bounds):
    """the two checks of every slot against the dense paste; -> {(b, k): counts}"""
    B, K = sel.shape
    assert run_off[0] == 0 and (np.diff(run_off.astype(np.int64)) >= 0).all()
    got = {}
    for b in range(B):
        H, W = int(frames[b, 0]), int(frames[b, 1])
        live = [k for k in range(K) if sel[b, k] >= 0]
        dense = _paste(masks[b], det[b], [sel[b, k] for k in live], H, W) if live else None
        for k in range(K):
            s = b * K + k
            mine = bounds[run_off[s]:run_off[s + 1]]
            if sel[b, k] < 0:
                assert mine.size == 0, (b, k)
                continue
            want = dense[:, :, live.index(k)]
            assert (np.diff(mine.astype(np.int64)) > 0).all() and (mine.size == 0 or int(mine[-1]) < H * W), (b, k)
            counts = rle.counts_from_boundaries(mine, H * W)
            ref = rle.encode(want)["counts"]
            assert counts.tolist() == ref.tolist(), (b, k, int(sel[b, k]), (H, W), counts[:8], ref[:8])
            assert np.array_equal(rle.decode({"size": [H, W], "counts": counts}), want), (b, k)
            got[(b, k)] = counts
    return got


def _crafted(got, sel, frames):
    """the crafted rows give what they were crafted for (so the case holds what it is meant to hold)"""
    seen = set()
    for (b, k), counts in got.items():
        r, H, W = int(sel[b, k]), int(frames[b, 0]), int(frames[b, 1])
        N = H * W
        c = counts.tolist()
        seen.add(r)
        if r == 0:
            assert c == [0, N]
        elif r == 1:
            end = np.cumsum(counts)
            start = end - counts
            assert ((start[1::2] // H) != ((end[1::2] - 1) // H)).any() and len(c) > W          # runs over joints, boundaries inside columns
        elif r in (2, 6):
            assert c == [N]
        elif r == 5:
            # x1 == x2 wherever 0.3 W >= 1; in a narrower frame the clamp x2 >= 1 leaves the window one column
            assert c == [N] or int(np.float32(0.3) * np.float32(W)) < 1
        elif r == 3:
            assert c == [0, 1, N - 1]
        elif r == 7:
            assert c in ([N], [0, 1, N - 1])                            # (a random mask: the one pixel is set or it is not)
        elif r == 4:
            assert c == [N - 1, 1]
        elif r == 10:
            x1, x2 = min(max(0, int(np.float32(0.3) * np.float32(W))), W), min(max(1, int(np.float32(0.7) * np.float32(W))), W)
            assert x1 < x2 and c == [x1 * H, (x2 - x1) * H] + ([(W - x2) * H] if x2 < W else [])
    return seen


FRAMES = [(70, 70), (37, 91), (91, 37), (64, 5), (65, 5), (129, 3)]


@pytest.mark.parametrize("frame", FRAMES, ids=["%dx%d" % f for f in FRAMES])
def test_frames_equal_the_paste(frame):
    """h x w frames: neither side a multiple of 64 / exactly 64 rows / 65 (one row into the second group of lanes) / 129 rows by 3 columns (a
    full-height run ends exactly on a 64-lane joint); 37 x 91 beside 91 x 37 catches a row / column swap"""
    masks, det, sel, frames = _case(2, 10, 4, [frame, frame], seed=sum(frame))
    run_off, bounds = Call(masks, det, sel, frames).run()
    seen = _crafted(_check(masks, det, sel, frames, run_off, bounds), sel, frames)
    assert seen == set(range(R))


def test_mixed_frames_in_one_batch():
    frames = FRAMES + [(28, 28), (84, 56)]
    masks, det, sel, fr = _case(len(frames), 10, 4, frames, seed=21)
    c = Call(masks, det, sel, fr)
    run_off, bounds = c.run()
    _crafted(_check(masks, det, sel, fr, run_off, bounds), sel, fr)
    assert c.guard_intact() and (bounds[c.cap:] == SENTINEL).all()


def test_checkerboard_holds_the_most_boundaries():
    """the 28 x 28 checkerboard pasted at scale 1 into a 28 x 28 frame: every pixel differs from the one above it, and -- 28 being even -- the last
    pixel of a column equals the first of the next, so the runs go on over every joint: 28 * 27 boundaries (pixel 0 is clear)"""
    rng = np.random.default_rng(2)
    masks, det = _rows(4, 28, 28, rng)
    sel = np.array([[8, -1, 8]], np.int32)
    frames = np.array([[28, 28]], np.int32)
    run_off, bounds = Call(masks[None], det[None], sel, frames).run()
    got = _check(masks[None], det[None], sel, frames, run_off, bounds)
    assert run_off.tolist() == [0, 756, 756, 1512]
    c = got[(0, 0)].tolist()
    assert len(c) == 757 and c[:27] == [1] * 27 and c[27] == 2 and sorted(set(c)) == [1, 2] and c.count(2) == 27


@pytest.mark.parametrize("C", [1, 4, 81])
@pytest.mark.parametrize("K", [1, 10])
@pytest.mark.parametrize("B", [1, 3])
def test_sizes_equal_the_paste_70x70(B, K, C):
    masks, det, sel, frames = _case(B, K, C, [(70, 70)] * B, seed=100 * B + 10 * K + C)
    run_off, bounds = Call(masks, det, sel, frames).run()
    _crafted(_check(masks, det, sel, frames, run_off, bounds), sel, frames)
    if B == 3:
        assert run_off[K] == run_off[2 * K]                            # the image without a live slot


def test_two_runs_bit_identical():
    masks, det, sel, frames = _case(3, 10, 4, [(70, 70), (37, 91), (129, 3)], seed=11)
    a, b = Call(masks, det, sel, frames).run(), Call(masks, det, sel, frames).run()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_capacity_below_the_total():
    """cap smaller than the total: run_off is complete and correct, the first cap boundaries are the full run's, nothing at or behind bounds + cap"""
    masks, det, sel, frames = _case(2, 10, 4, [(70, 70), (91, 37)], seed=13)
    full_off, full = Call(masks, det, sel, frames).run()
    total = int(full_off[-1])
    assert total > 400
    for cap in (total - 1, total // 2, 1, 0):
        run_off, bounds = Call(masks, det, sel, frames, cap=cap).run()
        assert np.array_equal(run_off, full_off), cap
        assert np.array_equal(bounds[:cap], full[:cap]), cap
        assert (bounds[cap:] == SENTINEL).all(), cap
    run_off, bounds = Call(masks, det, sel, frames, cap=total).run()
    assert np.array_equal(bounds[:total], full[:total]) and (bounds[total:] == SENTINEL).all()


def test_workspace_at_the_planner_figure():
    masks, det, sel, frames = _case(2, 10, 4, [(37, 91), (70, 70)], seed=17)
    outs = []
    for fill in (0x00, 0xFF):
        c = Call(masks, det, sel, frames, ws_fill=fill)
        assert c.ws_bytes == X.rle_masks_ws_bytes(2, 10, 91) >= (2 * 10 * (91 + 1)) * 4
        outs.append(c.run())
        assert c.guard_intact(), fill
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    _check(masks, det, sel, frames, *outs[0])
    # 256 bytes less: the workspace error, no output written, the guard alone
    for short in (c.need - 256, X.rle_masks_ws_bytes(2, 10, 70)):          # ... and a workspace planned for narrower frames than the call's widest
        c = Call(masks, det, sel, frames, ws_bytes=short)
        with pytest.raises(RuntimeError, match=r"rle_masks: workspace too small"):
            c.run()
        run_off, bounds = c.out()
        assert (run_off == SENTINEL).all() and (bounds == SENTINEL).all() and c.guard_intact()
        assert bool((c.ws[:c.ws_bytes] == 0xFF).all())


def test_refusals():
    lib = X.load()
    masks, det, sel, frames = _case(1, 10, 4, [(70, 70)], seed=3)
    c = Call(masks, det, sel, frames)
    assert getattr(lib, "myolo_rle_masks")(*c.args()) == 0
    torch.cuda.synchronize()
    c.run_off.fill_(SENTINEL)
    c.bounds.fill_(SENTINEL)
    null = ctypes.c_void_p(None)
    bad_sel = c.sel_h.copy()
    bad_sel[0, 3] = R
    sel17 = np.full((1, 17), -1, np.int32)

    # frames the entry must refuse: h < 1, w < 1, 2^31 pixels, and one wider than the workspace was planned for (the arrays outlive the calls)
    bad_frames = [np.array([hw], np.int32) for hw in ((0, 70), (70, 0), (65536, 32768), (70, 200))]
    cases = [dict(masks=null), dict(det=null), dict(sel=null), dict(sel_host=null), dict(frames=null), dict(frames_host=null), dict(run_off=null),
             dict(bounds=null), dict(ws=null), dict(K=17, sel_host=sel17.ctypes.data), dict(K=0), dict(sel_host=bad_sel.ctypes.data),
             dict(ws_bytes=c.need - 1), dict(cap=-1)] + [dict(frames_host=f.ctypes.data) for f in bad_frames]
    for kw in cases:
        assert getattr(lib, "myolo_rle_masks")(*c.args(**kw)) == -1, kw
        assert lib.myolo_last_error_string().startswith(b"rle_masks:"), (kw, lib.myolo_last_error_string())
    run_off, bounds = c.out()
    assert (run_off == SENTINEL).all() and (bounds == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the public path
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """the models this file shares are destroyed HERE, with the device idle -- not by a collection that happens to start inside a later test"""
    yield
    import gc
    _MODELS.clear()
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _model(dtype):
    if dtype not in _MODELS:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4, INFERENCE_DTYPE=dtype)
        _MODELS[dtype] = (cfg, MaskYOLO(mode="inference", config=cfg, seed=4))
    return _MODELS[dtype]


def _picture(h, w, seed):
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


SIX = ((128, 128), (200, 150), (61, 97), (128, 128), (128, 128), (200, 150))        # batch 4: a mixed first batch, a short last one
_DENSE = {}


def _images():
    return [_picture(h, w, 30 + k) for k, (h, w) in enumerate(SIX)]


def _dense(dtype, frame):
    """detect_many's dense results, computed once per (dtype, frame) and left unchanged"""
    if (dtype, frame) not in _DENSE:
        _DENSE[(dtype, frame)] = _model(dtype)[1].detect_many(_images(), cs_threshold=0.0, mask_frame=frame)
    return _DENSE[(dtype, frame)]


def _same_as_dense(r, d, size, what):
    assert set(r) == {"bboxes", "class_ids", "confidence_scores", "rle_masks"}, what
    for key in ("bboxes", "class_ids", "confidence_scores"):
        assert r[key].shape == d[key].shape and r[key].dtype == d[key].dtype and np.array_equal(r[key], d[key]), (what, key)
    n = len(d["class_ids"])
    assert len(r["rle_masks"]) == n == d["full_masks"].shape[2], what
    for i, m in enumerate(r["rle_masks"]):
        assert m["size"] == list(size) and m["counts"].dtype == np.int64, (what, i)
        assert (m["counts"][1:] > 0).all(), (what, i)
        assert np.array_equal(rle.decode(m), d["full_masks"][:, :, i].astype(bool)), (what, i)
        assert m["counts"].tolist() == rle.encode(d["full_masks"][:, :, i])["counts"].tolist(), (what, i)


@pytest.mark.parametrize("frame", ["image", "network"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_detect_many_rle_equals_dense(dtype, frame):
    cfg, m = _model(dtype)
    imgs, dense = _images(), _dense(dtype, frame)
    got = m.detect_many(imgs, cs_threshold=0.0, mask_frame=frame, mask_format="rle")
    assert len(got) == len(imgs) == len(dense) and sum(len(r["class_ids"]) for r in got) >= len(imgs)
    set_pixels = 0
    for k, (r, d) in enumerate(zip(got, dense)):
        size = imgs[k].shape[:2] if frame == "image" else tuple(cfg.IMAGE_SHAPE[:2])
        _same_as_dense(r, d, size, "image %d" % k)
        set_pixels += sum(rle.area(x) for x in r["rle_masks"])
    assert set_pixels > 0                                               # not a comparison of empty masks
    # detect() itself: its dense result, and detect_many's entry
    for k in (0, 1, 5):
        one = m.detect(imgs[k], cs_threshold=0.0, mask_frame=frame, mask_format="rle")
        assert len(one) == 1
        size = imgs[k].shape[:2] if frame == "image" else tuple(cfg.IMAGE_SHAPE[:2])
        _same_as_dense(one[0], m.detect(imgs[k], cs_threshold=0.0, mask_frame=frame)[0], size, "detect %d" % k)
        for key in ("bboxes", "class_ids", "confidence_scores"):
            assert np.array_equal(one[0][key], got[k][key]), (k, key)
        assert [x["counts"].tolist() for x in one[0]["rle_masks"]] == [x["counts"].tolist() for x in got[k]["rle_masks"]], k
    # the results go through coco_results like the dense ones
    ids = list(range(len(imgs)))
    assert rle.coco_results(got, ids) == rle.coco_results(dense, ids)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forced_regrow_gives_the_same_result(dtype):
    """a Net whose boundary buffer starts at ONE element: the first call finds the total above the capacity, enlarges the buffer and calls again"""
    cfg, m = _model(dtype)
    imgs = _images()
    want = m.detect_many(imgs, cs_threshold=0.0, mask_format="rle")
    m.net._rle_bounds = torch.empty(1, dtype=torch.int32, device=m.net.dev)
    got = m.detect_many(imgs, cs_threshold=0.0, mask_format="rle")
    assert m.net._rle_bounds.numel() > 1
    for k, (a, b) in enumerate(zip(got, want)):
        for key in ("bboxes", "class_ids", "confidence_scores"):
            assert np.array_equal(a[key], b[key]), (k, key)
        assert [x["counts"].tolist() for x in a["rle_masks"]] == [x["counts"].tolist() for x in b["rle_masks"]], k
        assert [x["size"] for x in a["rle_masks"]] == [x["size"] for x in b["rle_masks"]], k
    _same_as_dense(got[1], _dense(dtype, "image")[1], imgs[1].shape[:2], "regrown")


def test_mask_format_is_checked():
    cfg, m = _model("fp32")
    p = _picture(40, 30, 2)
    with pytest.raises(ValueError):
        m.detect(p, mask_format="png")
    with pytest.raises(ValueError):
        m.detect_many([p], mask_format="png")
    assert "full_masks" in m.detect(p, cs_threshold=0.0)[0] and "full_masks" in m.detect_many([p], cs_threshold=0.0, mask_format="dense")[0]
    cfg2 = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    m2 = MaskYOLO(mode="inference", config=cfg2, seed=4)
    with pytest.raises(ValueError):
        m2.detect(p, mask_format="rle")
    with pytest.raises(ValueError):
        m2.detect_many([p], mask_format="rle")


def test_net_rle_masks_checks_its_arguments():
    cfg, m = _model("fp32")
    masks, det, sel, frames = _case(2, 10, 4, [(70, 70), (37, 91)], seed=5)
    md, dd = torch.as_tensor(masks, device=DEV), torch.as_tensor(det, device=DEV)
    run_off, bounds = m.net.rle_masks(dd, md, sel, frames)
    assert run_off.dtype == np.int32 and bounds.dtype == np.uint32 and bounds.size == run_off[-1]
    _check(masks, det, sel, frames, run_off, bounds)
    with pytest.raises(ValueError):
        m.net.rle_masks(dd, md, sel.astype(np.int64), frames)
    with pytest.raises(ValueError):
        m.net.rle_masks(dd, md, sel, frames[:1])
    bad = sel.copy()
    bad[1, 0] = R
    with pytest.raises(RuntimeError, match="rle_masks: sel"):
        m.net.rle_masks(dd, md, bad, frames)

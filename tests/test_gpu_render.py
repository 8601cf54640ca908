"""The overlay drawn on the device: myolo_render_instances against render.render_instances (the host statement of the picture)
over the bytes of the existing paste (myolo_unmold_masks), byte for byte; its refusals; and detect / detect_many(render=True) against the host render
of the same call's masks and boxes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X                                            # noqa: E402
from myolo import render, rle                                          # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.engine import pack_images, packed_bytes                     # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402

DEV = "cuda"
R = 12                      # detection rows per image in the kernel cases: 7 crafted ones (below) + 5 random
K = 10
TILE_H, TILE_W = 8, 128     # the kernel's tile (csrc/exact_kernels.hip: RN_TH, RN_TW)
# h x w: one pixel; smaller than a tile; odd sizes over several tile rows; one pixel more than a tile in each direction; several tiles with a partial
# last one both ways; and a width that is a multiple of 4 over more than one tile (every row 4-byte aligned: the 12-byte loads and stores)
FRAMES = ((1, 1), (3, 5), (37, 53), (TILE_H + 1, TILE_W + 1), (130, 70), (20, 136))
SEL = np.array([0, 1, 2, -1, 3, 4, 6, -1, 5, 8], np.int32)              # the crafted rows in an order of their own, two empty slots between live ones

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


def _model():
    if "m" not in _MODELS:
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4, INFERENCE_DTYPE="fp32")
        _MODELS["m"] = (cfg, MaskYOLO(mode="inference", config=cfg, seed=4))
    return _MODELS["m"]


# ------------------------------------------------------------------------------------------------ the entry against the host render of the paste
def _rows(mh, C, rng):
    """masks [R,mh,mh,C], det [R,6] of one image.  0 the full-image window with an all-high mask (the allhigh flag; touches all four frame borders);
    1 and 2 one window with two high masks (the same pixels under two instances: order, and a truncation between the two blends); 3 a window that
    the frame's far corner clamps; 4 a zero-area window; 5 a window wholly outside the frame; 6 the full window with a random mask (holes: outline
    pixels inside, and on the borders); 7-11 random boxes and masks."""
    masks = rng.random((R, mh, mh, C), dtype=np.float32)
    det = np.zeros((R, 6), np.float32)
    lo = rng.random((R, 2)) * 0.7
    det[:, 0:2] = lo
    det[:, 2:4] = lo + 0.05 + rng.random((R, 2)) * 0.5
    det[:, 4] = rng.random(R)
    det[:, 5] = rng.integers(0, C, R)
    det[0, :4] = (0.0, 0.0, 1.0, 1.0)
    det[1, :4] = det[2, :4] = (0.1, 0.2, 0.8, 0.9)
    det[3, :4] = (0.6, 0.7, 1.3, 1.4)
    det[4, :4] = (0.3, 0.2, 0.3, 0.8)
    det[5, :4] = (1.2, 1.1, 1.5, 1.6)
    det[6, :4] = (0.0, 0.0, 1.0, 1.0)
    for r in (0, 1, 2):
        masks[r, :, :, int(det[r, 5])] = (0.5 + 0.5 * rng.random((mh, mh))).astype(np.float32)
    return masks, det


def _window(d, H, W):
    """unmold_kernel's window (csrc/exact_kernels.hip, unmold_window) restated in numpy float32"""
    f = np.float32
    x1 = min(max(0, int(f(d[0]) * f(W))), W)
    x2 = min(max(1, int(f(d[2]) * f(W))), W)
    y1 = min(max(0, int(f(d[1]) * f(H))), H)
    y2 = min(max(1, int(f(d[3]) * f(H))), H)
    return [x1, y1, x2, y2]


def _paste(masks_b, det_b, rows, H, W):
    """myolo_unmold_masks on the chosen rows of one image -> [H,W,n] bool: the oracle of the paste"""
    n = len(rows)
    if n == 0:
        return np.zeros((H, W, 0), bool)
    idx = torch.as_tensor(np.asarray(rows, np.int64), device=DEV)
    m = torch.as_tensor(masks_b, device=DEV).index_select(0, idx).contiguous()
    d = torch.as_tensor(det_b, device=DEV).index_select(0, idx).contiguous()
    full = torch.empty(H, W, n, dtype=torch.uint8, device=DEV)
    ws = torch.empty(n, dtype=torch.int32, device=DEV)
    X.call("myolo_unmold_masks", X.ptr(m), X.ptr(d), X.ptr(full), n, int(m.shape[1]), int(m.shape[2]), int(m.shape[3]), H, W, ws.data_ptr(),
           ws.numel() * 4, X.stream())
    return full.cpu().numpy().astype(bool)


def _case(frames, mh, C, seed, sels=None):
    """-> images (list of uint8 [h,w,3]), masks [B,R,mh,mh,C], det [B,R,6], sel [B,K], colors [B,K,3] (with exact 0s and 1s among them)"""
    rng = np.random.default_rng(seed)
    B = len(frames)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in frames]
    both = [_rows(mh, C, rng) for _ in frames]
    masks, det = np.stack([m for m, _ in both]), np.stack([d for _, d in both])
    sel = np.stack([SEL if sels is None else sels[b] for b in range(B)]).astype(np.int32)
    colors = rng.random((B, K, 3))
    colors[:, 0] = (1.0, 0.0, 0.0)
    colors[:, 1] = (0.0, 1.0, 1.0)
    return images, masks, det, sel, colors


def _expect(image, masks_b, det_b, sel_b, colors_b, **kw):
    H, W = image.shape[:2]
    live = [k for k in range(len(sel_b)) if sel_b[k] >= 0]
    rows = [int(sel_b[k]) for k in live]
    dense = _paste(masks_b, det_b, rows, H, W)
    return render.render_instances(image, [_window(det_b[r], H, W) for r in rows], dense, np.asarray(colors_b)[live].reshape(-1, 3), **kw), dense


def _upload(images):
    """the images in the pack_images layout on the device -> (the flat uint8 tensor of their bytes, the host descriptor)"""
    buf = np.zeros(packed_bytes(images), np.uint8)
    desc = pack_images(images, buf)
    return torch.as_tensor(buf[len(images) * 24:], device=DEV), desc


def _device(images, masks, det, sel, colors, **kw):
    bytes_d, desc = _upload(images)
    got = _model()[1].net.render_instances(bytes_d, desc, torch.as_tensor(det, device=DEV), torch.as_tensor(masks, device=DEV), sel, colors, **kw)
    assert len(got) == len(images)
    for g, im in zip(got, images):
        assert g.dtype == np.uint8 and g.shape == im.shape and g.flags["OWNDATA"]
    return got


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mh", [4, 28])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_device_overlay_is_the_host_render_of_the_paste(frame, mh, C):
    images, masks, det, sel, colors = _case([frame], mh, C, seed=7 + mh + C)
    got = _device(images, masks, det, sel, colors)[0]
    want, dense = _expect(images[0], masks[0], det[0], sel[0], colors[0])
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:8]
    assert dense[:, :, 0].all() and np.array_equal(dense[:, :, 1], dense[:, :, 2])        # the all-high full window; two instances on the same pixels
    if frame[0] * frame[1] > 1:
        assert not np.array_equal(got, images[0])


def test_three_sizes_in_one_call_and_other_alphas():
    frames = [(37, 53), (TILE_H + 1, TILE_W + 1), (130, 70)]
    sels = [SEL, np.full(K, -1, np.int32), SEL[::-1].copy()]           # the middle image has no live slot at all: its bytes come back as they went up
    images, masks, det, sel, colors = _case(frames, 28, 3, seed=11, sels=sels)
    for kw in ({}, {"alpha": 0.3, "box_alpha": 0.45}, {"alpha": 1.0, "box_alpha": 0.0}):
        got = _device(images, masks, det, sel, colors, **kw)
        for b in range(3):
            want, _ = _expect(images[b], masks[b], det[b], sel[b], colors[b], **kw)
            assert np.array_equal(got[b], want), (kw, b)
        assert np.array_equal(got[1], images[1])
    # colors=None: render.instance_colors over the live slots of each image, in slot order
    got = _device(images, masks, det, sel, None)
    for b in (0, 2):
        live = np.flatnonzero(sel[b] >= 0)
        cols = np.zeros((K, 3))
        cols[live] = render.instance_colors(len(live))
        assert np.array_equal(got[b], _expect(images[b], masks[b], det[b], sel[b], cols)[0]), b
    # a batch at one size needs no descriptor: [B,H,W,3]
    same = [images[0], images[0][::-1].copy()]
    got = _model()[1].net.render_instances(torch.as_tensor(np.stack(same), device=DEV), None, torch.as_tensor(det[:2], device=DEV),
                                           torch.as_tensor(masks[:2], device=DEV), sel[[0, 2]], colors[:2])
    for b in range(2):
        assert np.array_equal(got[b], _expect(same[b], masks[b], det[b], sel[[0, 2]][b], colors[b])[0]), b


@pytest.mark.parametrize("off", ["show_mask", "show_outline", "show_bbox"])
def test_each_layer_switched_off(off):
    images, masks, det, sel, colors = _case([(37, 53)], 28, 3, seed=13)
    everything = _device(images, masks, det, sel, colors)[0]
    got = _device(images, masks, det, sel, colors, **{off: False})[0]
    want, _ = _expect(images[0], masks[0], det[0], sel[0], colors[0], **{off: False})
    assert np.array_equal(got, want)
    assert not np.array_equal(got, everything)                          # the layer was in the picture


# ------------------------------------------------------------------------------------------------ refusals
SENTINEL = 0x5A


class Call(object):
    """one myolo_render_instances call through ctypes (no engine) on buffers this object owns; out is pre-filled with SENTINEL"""

    def __init__(self):
        images, masks, det, sel, colors = _case([(37, 53), (9, 20)], 4, 3, seed=17)
        self.images = images
        self.bytes_d, desc = _upload(images)
        self.desc_h, self.sel_h = np.ascontiguousarray(desc, np.int64), np.ascontiguousarray(sel, np.int32)
        self.md, self.dd, self.sd, self.cd, self.descd = (torch.as_tensor(np.ascontiguousarray(a), device=DEV)
                                                          for a in (masks, det, self.sel_h, colors, self.desc_h))
        self.out = torch.full_like(self.bytes_d, SENTINEL)
        self.ws = torch.zeros(2 * K, dtype=torch.int32, device=DEV)
        self.case = (images, masks, det, sel, colors)

    def args(self, **kw):
        a = dict(images=X.ptr(self.bytes_d), out=X.ptr(self.out), nbytes=self.bytes_d.numel(), desc=X.ptr(self.descd), desc_host=self.desc_h.ctypes.data,
                 masks=X.ptr(self.md), det=X.ptr(self.dd), sel=X.ptr(self.sd), sel_host=self.sel_h.ctypes.data, colors=X.ptr(self.cd), alpha=0.5,
                 box_alpha=0.7, flags=7, B=2, R=R, K=K, mh=4, mw=4, C=3, ws=self.ws.data_ptr(), ws_bytes=self.ws.numel() * 4, stream=X.stream())
        a.update(kw)
        return list(a.values())


def test_refusals_come_back_before_any_launch():
    lib = X.load()
    c = Call()
    images, masks, det, sel, colors = c.case

    def refused(message, **kw):
        assert lib.myolo_render_instances(*c.args(**kw)) == -1, kw
        err = lib.myolo_last_error_string().decode()
        assert err.startswith("render_instances: " + message), (kw, err)

    for name in ("images", "out", "desc", "desc_host", "masks", "det", "sel", "sel_host", "colors", "ws"):
        refused("null pointer", **{name: None})
    refused("need 1 <= K <= 16 (got K=0)", K=0)
    refused("need 1 <= K <= 16 (got K=17)", K=17)
    bad_sel = c.sel_h.copy()
    bad_sel[1, 4] = R
    refused("sel[14] = %d is not a row of the %d detections" % (R, R), sel_host=bad_sel.ctypes.data)
    for col, what in ((1, "0 x 20"), (2, "9 x 0")):
        bad = c.desc_h.copy()
        bad[1, col] = 0
        refused("frame 1 is %s (h, w >= 1 needed)" % what, desc_host=bad.ctypes.data)
    bad = c.desc_h.copy()
    bad[0, 1] = -3
    refused("frame 0 is -3 x 53", desc_host=bad.ctypes.data)
    refused("a batch of 2147483648 bytes, 2^31 or more", nbytes=1 << 31)
    refused("workspace too small (80 needed, 76 given)", ws_bytes=76)
    # an image that leaves the batch's bytes: by its offset, by its size, by a negative offset
    for row, col, val in ((1, 0, int(c.desc_h[1, 0]) + 1), (1, 1, 10), (0, 0, -1)):
        bad = c.desc_h.copy()
        bad[row, col] = val
        refused("image %d (offset" % row, desc_host=bad.ctypes.data)
    refused("alpha and box_alpha must lie in [0, 1]", alpha=1.5)
    refused("alpha and box_alpha must lie in [0, 1]", box_alpha=float("nan"))
    refused("alpha and box_alpha must lie in [0, 1]", flags=8)
    torch.cuda.synchronize()
    assert bool((c.out == SENTINEL).all())                              # nothing was launched
    # the same arguments, untouched, are accepted and give the picture
    assert lib.myolo_render_instances(*c.args()) == 0
    torch.cuda.synchronize()
    flat = c.out.cpu().numpy()
    for b, im in enumerate(images):
        o = int(c.desc_h[b, 0])
        want, _ = _expect(im, masks[b], det[b], sel[b], colors[b])
        assert np.array_equal(flat[o:o + im.size].reshape(im.shape), want), b


def test_net_render_instances_checks_its_arguments():
    net = _model()[1].net
    images, masks, det, sel, colors = _case([(37, 53), (9, 20)], 4, 3, seed=17)
    bytes_d, desc = _upload(images)
    md, dd = torch.as_tensor(masks, device=DEV), torch.as_tensor(det, device=DEV)
    with pytest.raises(ValueError, match="sel"):
        net.render_instances(bytes_d, desc, dd, md, sel.astype(np.int64), colors)
    with pytest.raises(ValueError, match="expected"):
        net.render_instances(bytes_d, desc[:1], dd, md, sel, colors)
    with pytest.raises(ValueError, match="colors"):
        net.render_instances(bytes_d, desc, dd, md, sel, colors * 2.0)
    with pytest.raises(ValueError, match="uint8 device"):
        net.render_instances(bytes_d.cpu(), desc, dd, md, sel, colors)
    bad = sel.copy()
    bad[1, 0] = R
    with pytest.raises(RuntimeError, match="render_instances: sel"):
        net.render_instances(bytes_d, desc, dd, md, bad, colors)


# ------------------------------------------------------------------------------------------------ the public path
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
DENSE_KEYS = {"bboxes", "class_ids", "confidence_scores", "full_masks"}
RLE_KEYS = {"bboxes", "class_ids", "confidence_scores", "rle_masks"}


def _images():
    return [_picture(h, w, 30 + k) for k, (h, w) in enumerate(SIX)]


def _host_render(image, r):
    """the host render of one result dict: its masks (dense, or decoded from their run-length form), the windows its pixel boxes clamp to (a box
    corner is the float32 product unmold_window truncates), the palette of its instance count"""
    H, W = image.shape[:2]
    n = len(r["class_ids"])
    if "full_masks" in r:
        dense = np.asarray(r["full_masks"]).astype(bool)
    else:
        dense = np.stack([rle.decode(m) for m in r["rle_masks"]], axis=2) if n else np.zeros((H, W, 0), bool)
    assert dense.shape == (H, W, n)
    wins = [[min(max(0, int(b[0])), W), min(max(0, int(b[1])), H), min(max(1, int(b[2])), W), min(max(1, int(b[3])), H)] for b in r["bboxes"]]
    return render.render_instances(image, wins, dense, render.instance_colors(n) if n else np.zeros((0, 3)))


def _same_results(a, b, keys):
    for key in keys:
        if key == "rle_masks":
            assert [m["counts"].tolist() for m in a[key]] == [m["counts"].tolist() for m in b[key]]
        else:
            assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key


def test_detect_render_equals_the_host_render(tmp_path):
    cfg, m = _model()
    imgs = _images()
    drawn = 0
    for k in (0, 1, 2):                                                 # at IMAGE_SHAPE, larger, smaller
        plain = m.detect(imgs[k], cs_threshold=0.0)
        assert len(plain) == 1 and set(plain[0]) == DENSE_KEYS         # render=False: today's keys
        got = m.detect(imgs[k], cs_threshold=0.0, render=True, save_path=None)
        assert len(got) == 1 and set(got[0]) == DENSE_KEYS | {"rendered"}
        _same_results(got[0], plain[0], DENSE_KEYS)
        pic = got[0]["rendered"]
        assert pic.dtype == np.uint8 and pic.shape == imgs[k].shape
        assert np.array_equal(pic, _host_render(imgs[k], got[0])), k
        drawn += int(not np.array_equal(pic, imgs[k]))
        # run-length masks: the same picture, from the decoded masks
        as_rle = m.detect(imgs[k], cs_threshold=0.0, render=True, mask_format="rle", save_path=None)
        assert set(as_rle[0]) == RLE_KEYS | {"rendered"}
        assert np.array_equal(as_rle[0]["rendered"], pic) and np.array_equal(as_rle[0]["rendered"], _host_render(imgs[k], as_rle[0])), k
        assert set(m.detect(imgs[k], cs_threshold=0.0, mask_format="rle")[0]) == RLE_KEYS
    assert drawn >= 1                                                   # not a comparison of untouched images
    # the file under save_path
    where = str(tmp_path / "results" / "deeper")
    got = m.detect(imgs[1], cs_threshold=0.0, render=True, save_path=where)
    assert os.listdir(where) == ["InferMaskYOLO-0.png"]
    assert np.array_equal(render.read_png(os.path.join(where, "InferMaskYOLO-0.png")), got[0]["rendered"])
    # without render, save_path stays ignored
    other = str(tmp_path / "untouched")
    m.detect(imgs[1], cs_threshold=0.0, save_path=other)
    assert not os.path.exists(other)


@pytest.mark.parametrize("mask_format", ["dense", "rle"])
def test_detect_many_render_over_mixed_sizes(mask_format):
    cfg, m = _model()
    imgs = _images()
    keys = DENSE_KEYS if mask_format == "dense" else RLE_KEYS
    plain = m.detect_many(imgs, cs_threshold=0.0, mask_format=mask_format)
    got = m.detect_many(imgs, cs_threshold=0.0, mask_format=mask_format, render=True)
    assert len(got) == len(plain) == len(imgs) and sum(len(r["class_ids"]) for r in got) >= len(imgs)
    for k, (r, p) in enumerate(zip(got, plain)):
        assert set(p) == keys and set(r) == keys | {"rendered"}, k
        _same_results(r, p, keys)
        assert np.array_equal(r["rendered"], _host_render(imgs[k], r)), k
    # a batch whose images are all at IMAGE_SHAPE, short: the bytes go up as they are
    at_frame = [imgs[0], imgs[3], imgs[4], imgs[0], imgs[3]]
    for frame in ("image", "network"):
        got = m.detect_many(at_frame, cs_threshold=0.0, mask_format=mask_format, mask_frame=frame, render=True)
        for k, r in enumerate(got):
            assert np.array_equal(r["rendered"], _host_render(at_frame[k], r)), (frame, k)
    # detect() gives detect_many's picture
    one = m.detect(imgs[5], cs_threshold=0.0, render=True, save_path=None, mask_format=mask_format)[0]
    many = m.detect_many(imgs, cs_threshold=0.0, mask_format=mask_format, render=True)[5]
    assert np.array_equal(one["rendered"], many["rendered"])


def test_render_refuses_what_it_cannot_draw():
    cfg, m = _model()
    p, at = _picture(40, 30, 2), _picture(128, 128, 3)
    with pytest.raises(ValueError, match="mask_frame"):
        m.detect(p, render=True, mask_frame="network", save_path=None)
    with pytest.raises(ValueError, match="mask_frame"):
        m.detect_many([at, p], render=True, mask_frame="network")
    assert "rendered" in m.detect(at, cs_threshold=0.0, render=True, mask_frame="network", save_path=None)[0]
    cfg2 = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=1, DETECT_MASKS_FOR_SELECTED_ONLY=True)
    m2 = MaskYOLO(mode="inference", config=cfg2, seed=4)
    with pytest.raises(ValueError, match="DETECT_MASKS_FOR_SELECTED_ONLY"):
        m2.detect(p, render=True, save_path=None)
    with pytest.raises(ValueError, match="DETECT_MASKS_FOR_SELECTED_ONLY"):
        m2.detect_many([p], render=True)
    assert set(m2.detect(p, cs_threshold=0.0)[0]) == DENSE_KEYS        # without render that configuration detects as before

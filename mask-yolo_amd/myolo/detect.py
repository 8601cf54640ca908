"""
``myolo.detect`` -- the one detection pipeline under MaskYOLO.detect / detect_many / evaluate / evaluate_shapes_stream:
uint8 images are staged to the device (Stager), run through the forward, up to SLOTS rows per image are selected on the host from the one
detection download of a batch (Selection), and the selection is handed to a mask consumer: dense_masks, rle_masks, polygon_masks, overlap_counts,
measurements, render.  With max_detections=K the same record is filled on the device instead, K <= MAX_SLOTS rows per image (Selection.from_device, DESIGN.md
section 23); no consumer learns where a selection came from.
"""
import numpy as np
import torch

from . import _ext as X
from . import myolo_utils as mutils
from .engine import packed_bytes

SLOTS = 10            # detect() keeps at most the top 10 detections of an image


MAX_SLOTS = 128       # ... or, with max_detections=K, at most K <= 128, selected on the device
RENDER_SLOTS = 16     # the instances of an image myolo_render_instances draws in its one pass


def check_max_detections(cfg, max_detections, render=False):
    """the max_detections argument of detect / detect_many / evaluate / evaluate_shapes_stream: None (the host selection of SLOTS rows) or an int
    in 1 .. MAX_SLOTS"""
    if max_detections is None:
        return
    if isinstance(max_detections, (bool, np.bool_)) or not isinstance(max_detections, (int, np.integer)) or not 1 <= max_detections <= MAX_SLOTS:
        raise ValueError("max_detections must be None or an int in 1 .. %d (got %r)" % (MAX_SLOTS, max_detections))
    if bool(getattr(cfg, "DETECT_MASKS_FOR_SELECTED_ONLY", False)):
        raise ValueError("max_detections is not supported with config.DETECT_MASKS_FOR_SELECTED_ONLY")
    if render and max_detections > RENDER_SLOTS:
        raise ValueError("render=True draws at most %d instances per image: the overlay kernel blends, outlines and boxes all instances of an "
                         "image in one pass and its layers cannot be split into blocks (got max_detections=%d); rendering more is out of scope"
                         % (RENDER_SLOTS, max_detections))


def check_args(cfg, images, mask_frame, mask_format, render, max_detections=None, measure=False):
    """detect() / detect_many()'s argument checks, before anything is uploaded"""
    selected_only = bool(getattr(cfg, "DETECT_MASKS_FOR_SELECTED_ONLY", False))
    check_max_detections(cfg, max_detections, render)
    if mask_frame not in ("image", "network"):
        raise ValueError("mask_frame must be 'image' or 'network' (got %r)" % (mask_frame,))
    if mask_format not in ("dense", "rle", "polygon"):
        raise ValueError("mask_format must be 'dense', 'rle' or 'polygon' (got %r)" % (mask_format,))
    if mask_format in ("rle", "polygon") and selected_only:
        raise ValueError("mask_format=%r is not supported with config.DETECT_MASKS_FOR_SELECTED_ONLY" % (mask_format,))
    for im in images:
        assert im.dtype == 'uint8' and im.ndim == 3 and im.shape[2] == 3 and im.shape[0] >= 1 and im.shape[1] >= 1, \
            "a uint8 [h,w,3] image is expected (got %s %s)" % (im.dtype, tuple(im.shape))
    if render and selected_only:
        raise ValueError("render=True is not supported with config.DETECT_MASKS_FOR_SELECTED_ONLY")
    if measure and selected_only:
        raise ValueError("measure=True is not supported with config.DETECT_MASKS_FOR_SELECTED_ONLY")
    if render and mask_frame == "network" and any(list(im.shape) != list(cfg.IMAGE_SHAPE) for im in images):
        raise ValueError("render=True draws on the image given: mask_frame='network' needs every image at config.IMAGE_SHAPE")


# ------------------------------------------------------------------------------------------------ 1. the stager
class Stager(object):
    """uint8 [h,w,3] host images -> (x, canvas): x the float32 [n,H,W,3] device batch the forward takes, canvas what render draws on -- (the image
    bytes on the device, their host descriptor, or None for a [n,H,W,3] tensor) -- or None when no render was asked for.  One per model: it owns
    the pinned host buffers of the pipeline (pinning costs ~5 ms per buffer: once per model, not once per call)."""

    def __init__(self, net):
        self.net, self.slots, self._flat, self._pins = net, 0, None, {}

    def pinned(self, name, n, shape, dtype=torch.uint8):
        """n pinned host tensors of `shape`, kept under `name` until another count or a larger size is asked for"""
        have = self._pins.get(name)
        if have is None or len(have) != n or have[0].numel() < int(np.prod(shape)):
            have = self._pins[name] = [torch.empty(shape, dtype=dtype).pin_memory() for _ in range(n)]
        return have

    def at_frame(self, grp):
        return all(list(im.shape) == list(self.net.cfg.IMAGE_SHAPE) for im in grp)

    def reserve(self, in_flight, groups=()):
        """Open a streamed call of Net.predict_stream(..., in_flight): batch bi stages through slot bi % slots of every ring.  -> slots.
        predict_stream takes batch i from its source BEFORE it waits for a result, with up to 2 * in_flight batches submitted and not waited for:
        their uploads may still be reading their buffers while batch i is packed, so a ring needs 2 * in_flight + 1 slots; one to spare.
        groups: the call's batches -- the flat ring of the resized ones is sized once, here, to the largest of them packed."""
        self.slots = 2 * in_flight + 2
        B = int(self.net.cfg.BATCH_SIZE)
        need = max([packed_bytes(grp, B) for grp in groups if not self.at_frame(grp)], default=0)
        self._flat = self.pinned("flat", self.slots, (need,)) if need else None
        return self.slots

    def _unit(self, raw, shape):
        # (image / 255.).astype(float32) formed on the device from the uploaded bytes (myolo_u8_to_unit_f32: the float32 of the float64 quotient, as numpy
        # forms it on the host) -- bit-identical, a quarter of the bytes over PCIe and no float64 temporary on the host (the host normalisation + pageable
        # upload of 8 MB per batch of four 416 x 416 images cost 2.3 ms per batch, more than half the forward; three float64 torch kernels 0.37 ms)
        x = torch.empty(shape, dtype=torch.float32, device=raw.device)
        X.call("myolo_u8_to_unit_f32", X.ptr(raw), X.ptr(x), raw.numel(), X.stream())
        return x

    def stage(self, bi, grp, render=False):
        """batch bi of a reserved call, len(grp) <= BATCH_SIZE images: all at IMAGE_SHAPE, their bytes go up from the [B,H,W,3] ring (a short group
        repeats its last image: the captured graph has one shape); else the group is resized on the device from the flat ring (n_slots=B: a
        descriptor, not a copy)."""
        cfg, B = self.net.cfg, int(self.net.cfg.BATCH_SIZE)
        if not self.at_frame(grp):
            out = self.net.resize_to_frame(grp, n_slots=B, stage=self._flat[bi % self.slots], want_packed=render)
            return out if render else (out, None)
        buf = self.pinned("frame", self.slots, (B,) + tuple(cfg.IMAGE_SHAPE))[bi % self.slots]
        np.stack(list(grp) + [grp[-1]] * (B - len(grp)), out=buf.numpy())
        raw = buf.to(self.net.dev, non_blocking=True)
        return self._unit(raw, raw.shape), ((raw, None) if render else None)

    def stage_one(self, image, render=False):
        """detect()'s form: ONE image per launch (its fp32 sums differ in the last bits from a padded batch's), and nothing pinned per call -- the
        bytes go up pageable, or through the Net's own grow-only buffer (Net.resize_to_frame)"""
        if self.at_frame([image]):
            raw = torch.from_numpy(np.ascontiguousarray(image)).to(self.net.dev)
            return self._unit(raw, (1,) + tuple(raw.shape)), ((raw.unsqueeze(0), None) if render else None)
        out = self.net.resize_to_frame([image], want_packed=render)
        return out if render else (out, None)


# ------------------------------------------------------------------------------------------------ 2. the selection of a batch
def select(det_h, cs_threshold, image_shape):
    """detect()'s selection on the host copy det_h [R,6] of one image's detections (model.py:1290-1304, 1373-1380): drop the zero-area boxes,
    take the top 10 by score, drop those under cs_threshold, NMB at 0.7.  -> keep (rows of det_h with area), nmb (the survivors, indices
    into keep, in the order detect() reports them), and boxes / scores / class_ids of the keep rows.  The selected rows of det_h are keep[nmb]."""
    boxes, scores, class_ids = det_h[:, :4], det_h[:, 4], det_h[:, 5].astype(np.int32)
    keep = np.where((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) > 0)[0]     # model.py:1373-1380
    boxes, scores, class_ids = boxes[keep], scores[keep], class_ids[keep]
    top10 = np.argsort(scores)[::-1][:SLOTS]
    kept = np.array([i for i in top10 if scores[i] >= cs_threshold], dtype=np.int64)
    nmb = mutils.NMB(boxes[kept], class_ids[kept], kept, image_shape, nms_threshold=0.7) if len(kept) else kept
    return keep, np.asarray(nmb, dtype=np.int64), boxes, scores, class_ids


class Selection(object):
    """What the images of one batch report, from the batch's one detection download det_all [B,R,6] (host): sel [B,SLOTS] int32 = the rows of
    det_all[k] image k reports, in reporting order, -1 in the empty slots and for the padding images k >= n (= n_live); picked[k] = (boxes
    [m,4] normalised corners, class_ids [m], scores [m]) of those rows.  Every consumer below reads this record."""

    def __init__(self, det_all, n_live, cs_threshold, image_shape):
        self.n = int(n_live)
        self.sel = np.full((det_all.shape[0], SLOTS), -1, np.int32)
        self.picked = []
        for k in range(self.n):
            keep, nmb, boxes, scores, class_ids = select(det_all[k], cs_threshold, image_shape)
            self.sel[k, :len(nmb)] = keep[nmb]
            self.picked.append((boxes[nmb], class_ids[nmb], scores[nmb]))

    @classmethod
    def from_device(cls, sel, picked, n_live):
        """the same record from Net.select_detections' (sel [B,K] int32, picked [B,K,6] float32): any K, nothing selected on the host"""
        self = cls.__new__(cls)
        self.n, self.sel, self.picked = int(n_live), sel, []
        for k in range(self.n):
            m = int((sel[k] >= 0).sum())                         # (the survivors fill the leading slots)
            self.picked.append((picked[k, :m, :4].copy(), picked[k, :m, 5].astype(np.int32), picked[k, :m, 4].copy()))
        return self

    @classmethod
    def of_batch(cls, net, det_d, n_live, cs_threshold, image_shape, max_detections=None):
        """the selection of one batch's det_d [B,R,6] (device): max_detections None -- the host selection of SLOTS rows from the batch's one
        detection download; an int -- K = max_detections slots filled on the device (Net.select_detections), det_d stays there"""
        if max_detections is None:
            return cls(det_d.cpu().numpy(), n_live, cs_threshold, image_shape)
        return cls.from_device(*net.select_detections(det_d, n_live, max_detections, cs_threshold, image_shape), n_live=n_live)

    def rows(self, k):
        return self.sel[k, :len(self.picked[k][1])]

    def result(self, k, frame):
        """the part of image k's result dict every mask form shares, its boxes in pixels of the frame (h, w, ...) (model.py:1307)"""
        boxes, class_ids, scores = self.picked[k]
        h, w = float(frame[0]), float(frame[1])
        return {"bboxes": boxes * np.array([w, h, w, h], dtype=boxes.dtype), "class_ids": class_ids, "confidence_scores": scores}


# ------------------------------------------------------------------------------------------------ 3. the consumers
def paste(det, masks, frame):
    """myolo_unmold_masks: det [N,6], masks [N,mh,mw,C] device rows of one image, N >= 1 boxes with area -> bool [h,w,N] on the host"""
    N, H, W = int(det.shape[0]), int(frame[0]), int(frame[1])
    mh, mw, C = int(masks.shape[1]), int(masks.shape[2]), int(masks.shape[3])
    full = torch.empty(H, W, N, dtype=torch.uint8, device=det.device)
    ws = torch.empty(N, dtype=torch.int32, device=det.device)
    X.call("myolo_unmold_masks", X.ptr(masks.contiguous()), X.ptr(det.contiguous()), X.ptr(full), N, mh, mw, C, H, W,
           ws.data_ptr(), ws.numel() * 4, X.stream())
    # (a pinned staging buffer for this download was measured slower: the host's astype() then reads uncached memory)
    return full.view(torch.bool).cpu().numpy()        # (the kernel writes 0 / 1 bytes: the bool view saves the host's astype pass)


def dense_masks(stager, det_img, mask_img, rows, frame, feature=None):
    """full_masks [h,w,n] of ONE image: det_img [R,6], mask_img [R,mh,mw,C] device tensors, rows = Selection.rows(k).  mask_img None
    (DETECT_MASKS_FOR_SELECTED_ONLY): the mask head runs here, on the survivors, over the image's `feature`.
    decode_masks (model.py:1330-1391) unmolds every box and the caller then keeps <= 10 of them (model.py:1290-1304); the selection needs only
    boxes / scores / classes, so it ran first and only the survivors are unmolded (same output: full_masks[:, :, nmb] of the all-box result).
    Per image on purpose: one unmold launch and one download per BATCH was measured at 514 img/s against 865 -- a pageable 6.9 MB download runs
    at 2 GB/s where four of 1.7 MB do not, and cutting the H x W x 40 block into per-image H x W x n arrays costs the host another 0.5 ms per image."""
    if not len(rows):
        return np.empty((int(frame[0]), int(frame[1]), 0), dtype=bool)
    # (the few indices go up from a pinned buffer without blocking; the download of the pasted masks ends every image with a synchronisation, so
    # the buffer is free again by the next one)
    pin = stager.pinned("rows", 1, (MAX_SLOTS,), torch.int64)[0][:len(rows)]
    pin.copy_(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)))
    idx = pin.to(det_img.device, non_blocking=True)
    det_s = det_img.index_select(0, idx).contiguous()
    if mask_img is None:
        mask_s = stager.net.predict_masks(feature, det_s[:, :4].unsqueeze(0))[0]
    else:
        mask_s = mask_img.index_select(0, idx).contiguous()
    return paste(det_s, mask_s, frame)


def rle_masks(net, det_d, mask_d, selection, frames):
    """rle_masks of the live images of a batch, one Net.rle_masks call: frames[k] = (h, w, ...) of the frame image k's masks are pasted into"""
    from .rle import counts_from_boundaries
    K = selection.sel.shape[1]
    fr = np.ones(selection.sel.shape[:1] + (2,), np.int32)                 # (padding: no slot, a 1 x 1 frame)
    for k, f in enumerate(frames):
        fr[k] = (int(f[0]), int(f[1]))
    run_off, bounds = net.rle_masks(det_d, mask_d, selection.sel, fr)
    return [[{"size": [h, w], "counts": counts_from_boundaries(bounds[run_off[s]:run_off[s + 1]], h * w)}
             for s in range(k * K, k * K + len(selection.rows(k)))] for k, (h, w) in enumerate(fr[:selection.n].tolist())]


def polygon_masks(net, det_d, mask_d, selection, frames):
    """polygons of the live images of a batch, one Net.contour_masks call: per image the list, in class_ids order, of each instance's loops (int32
    [n,2] (X, Y) corner coordinates of the frame frames[k] = (h, w, ...), contour.trace's order)"""
    K = selection.sel.shape[1]
    fr = np.ones(selection.sel.shape[:1] + (2,), np.int32)                 # (padding: no slot, a 1 x 1 frame)
    for k, f in enumerate(frames):
        fr[k] = (int(f[0]), int(f[1]))
    loops = net.contour_masks(det_d, mask_d, selection.sel, fr)
    return [loops[k * K:k * K + len(selection.rows(k))] for k in range(selection.n)]


def measurements(net, det_d, mask_d, selection, frames):
    """measure.properties of the instances of the live images of a batch, one Net.measure_masks call over all the slots of every image: per
    image the dict of arrays over its instances, in class_ids order, taken in the frame frames[k] = (h, w, ...) its masks are pasted into"""
    from .measure import properties
    fr = np.ones(selection.sel.shape[:1] + (2,), np.int32)                 # (padding: no slot, a 1 x 1 frame)
    for k, f in enumerate(frames):
        fr[k] = (int(f[0]), int(f[1]))
    raw = net.measure_masks(det_d, mask_d, selection.sel, fr)
    return [properties(raw[k, :len(selection.rows(k))]) for k in range(selection.n)]


def overlap_counts(stager, det_d, mask_d, selection, gt_d):
    """(inter [B,K,T], area_pred [B,K], area_gt [B,T], win [B,K,4]) on the host: one Net.overlap_counts call against gt_d [B,H,W,T]"""
    # (the table goes up from a pinned buffer without blocking; free again by the next batch: the downloads here end with a synchronisation)
    # (kept flat: K differs between calls with and without max_detections)
    pin = stager.pinned("sel", 1, (selection.sel.size,), torch.int32)[0][:selection.sel.size].view(selection.sel.shape)
    pin.numpy()[:] = selection.sel
    return [t.cpu().numpy() for t in stager.net.overlap_counts(det_d, mask_d, pin, gt_d)]


def render(net, canvas, det_d, mask_d, selection):
    """the overlays of the live images of a batch on its Stager canvas, instance i of an image in colour i: one Net.render_instances call"""
    n = selection.n
    images_d, desc = canvas
    if desc is None:
        images_d = images_d[:n]                              # (a short last batch is padded with copies of its last image)
    else:
        desc = desc[:n]
    return net.render_instances(images_d, desc, det_d[:n], mask_d[:n], selection.sel[:n])


def batch_results(stager, det_d, mask_d, selection, frames, mask_format="dense", canvas=None, feature=None, measure=False):
    """detect()'s result dicts of the live images of one batch: det_d [B,R,6], mask_d [B,R,mh,mw,C] (None: see dense_masks) device tensors,
    frames[k] the frame image k reports in; with a canvas the dicts gain "rendered", drawn from the same selection after either mask form, and
    with measure "measurements" (measure.properties of the image's instances), taken from the same selection in the same frame."""
    out = [selection.result(k, frames[k]) for k in range(selection.n)]
    if mask_format == "rle":
        for r, codes in zip(out, rle_masks(stager.net, det_d, mask_d, selection, frames)):
            r["rle_masks"] = codes
    elif mask_format == "polygon":
        for r, loops in zip(out, polygon_masks(stager.net, det_d, mask_d, selection, frames)):
            r["polygons"] = loops
    else:
        for k, r in enumerate(out):
            r["full_masks"] = dense_masks(stager, det_d[k], None if mask_d is None else mask_d[k], selection.rows(k), frames[k], feature)
    if measure:
        for r, props in zip(out, measurements(stager.net, det_d, mask_d, selection, frames)):
            r["measurements"] = props
    if canvas is not None:
        for r, pic in zip(out, render(stager.net, canvas, det_d, mask_d, selection)):
            r["rendered"] = pic
    return out

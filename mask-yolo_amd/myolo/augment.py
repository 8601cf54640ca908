"""
Training augmentation on the device: random horizontal flip, scale, translation, rotation, brightness gain and offset.

The reference augments on the host through imgaug (model.py:943-1060 `augmentation=`, myolo_utils.py:313-343).  Here the host only
draws one row of eight doubles per image -- Augmentation.params() -- and the warp itself is one more device producer of the six training
inputs (DeviceAugmenter -> myolo_augment_batch, csrc/augment_kernels.hip): bilinear image, nearest-neighbour masks, empty instances
dropped, boxes re-derived from the warped masks, YOLO targets encoded from those boxes.  The arithmetic is a bit-exact contract, stated
in DESIGN.md ("On-device augmentation") and restated in numpy by tests/augment_ref.py.
"""
import math

import numpy as np

IDENTITY_ROW = np.array([1., 0., 0., 0., 1., 0., 1., 0.], dtype=np.float64)


def _pair(name, v, lo=None, hi=None, lo_open=False):
    try:
        a, b = float(v[0]), float(v[1])
        n = len(v)
    except (TypeError, IndexError, ValueError):
        raise ValueError("%s must be a (low, high) pair, got %r" % (name, v))
    if n != 2 or not (math.isfinite(a) and math.isfinite(b)) or a > b:
        raise ValueError("%s must be a finite (low, high) pair with low <= high, got %r" % (name, v))
    if lo is not None and (a <= lo if lo_open else a < lo):
        raise ValueError("%s: low must be %s %g, got %r" % (name, ">" if lo_open else ">=", lo, v))
    if hi is not None and b > hi:
        raise ValueError("%s: high must be <= %g, got %r" % (name, hi, v))
    return a, b


class Augmentation(object):
    """What MaskYOLO.train(augmentation=...) takes.

    fliplr      probability of a horizontal flip
    scale       (low, high) zoom factor about the image centre, > 0
    translate   (low, high) shift as a fraction of the side, drawn independently for x and y, within [-1, 1]
    rotate      (low, high) rotation in degrees, within [-360, 360]
    brightness  (low, high) gain of the byte values, >= 0
    offset      (low, high) bias of the byte values as a fraction of 255, within [-1, 1]
    cval        byte value (0..255) read outside the source frame
    seed        params() is a pure function of (seed, epoch, image_id)

    Forward map about the centre c = ((W-1)/2, (H-1)/2): out = c + t + s * R(theta) * F * (src - c), F the flip; a row holds its inverse."""

    def __init__(self, fliplr=0.0, scale=(1., 1.), translate=(0., 0.), rotate=(0., 0.), brightness=(1., 1.), offset=(0., 0.), cval=0, seed=0):
        fliplr = float(fliplr)
        if not 0.0 <= fliplr <= 1.0:
            raise ValueError("fliplr is a probability in [0, 1], got %r" % (fliplr,))
        self.fliplr = fliplr
        self.scale = _pair("scale", scale, lo=0.0, lo_open=True)
        self.translate = _pair("translate", translate, lo=-1.0, hi=1.0)
        self.rotate = _pair("rotate", rotate, lo=-360.0, hi=360.0)
        self.brightness = _pair("brightness", brightness, lo=0.0)
        self.offset = _pair("offset", offset, lo=-1.0, hi=1.0)
        cval = float(cval)
        if not 0.0 <= cval <= 255.0:
            raise ValueError("cval is a byte value in [0, 255], got %r" % (cval,))
        self.cval = cval
        seed = int(seed)
        if not 0 <= seed < 2 ** 32:
            raise ValueError("seed must be in [0, 2**32), got %r" % (seed,))
        self.seed = seed

    def draw(self, epoch, image_id):
        """-> dict(flip, scale, tx, ty, theta, gain, bias): the raw draws (translations as fractions, theta in degrees, bias as a fraction).
        Always the same seven draws in the same order from RandomState([seed, epoch, image_id]), whatever the ranges."""
        rs = np.random.RandomState([self.seed, int(epoch), int(image_id)])
        u = rs.random_sample(7)

        def between(r, x):
            return r[0] + (r[1] - r[0]) * x if r[1] > r[0] else r[0]
        return dict(flip=bool(u[0] < self.fliplr), scale=between(self.scale, u[1]), tx=between(self.translate, u[2]),
                    ty=between(self.translate, u[3]), theta=between(self.rotate, u[4]), gain=between(self.brightness, u[5]),
                    bias=between(self.offset, u[6]))

    def params(self, epoch, image_id, H, W):
        """-> float64[8]: m00 m01 m02 m10 m11 m12 (output pixel -> source position, pixel centres baked in), gain, bias (in byte units)."""
        d = self.draw(epoch, image_id)
        f = -1.0 if d["flip"] else 1.0
        s, th = d["scale"], d["theta"]
        co, si = (1.0, 0.0) if th == 0.0 else (math.cos(math.radians(th)), math.sin(math.radians(th)))
        inv = 1.0 if s == 1.0 else 1.0 / s
        # inverse of s * R(theta) * F:  F * R(-theta) / s  (F is its own inverse and only negates the first row)
        m00, m01 = f * (co * inv), f * (si * inv)
        m10, m11 = -si * inv, co * inv
        cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
        ox, oy = cx + d["tx"] * W, cy + d["ty"] * H                 # c + t
        row = np.array([m00, m01, cx - (m00 * ox + m01 * oy), m10, m11, cy - (m10 * ox + m11 * oy), d["gain"], d["bias"] * 255.0],
                       dtype=np.float64)
        return row + 0.0                                            # (-0.0 -> 0.0)

    @staticmethod
    def identity():
        return IDENTITY_ROW.copy()

    def __repr__(self):
        return ("Augmentation(fliplr=%r, scale=%r, translate=%r, rotate=%r, brightness=%r, offset=%r, cval=%r, seed=%r)" %
                (self.fliplr, self.scale, self.translate, self.rotate, self.brightness, self.offset, self.cval, self.seed))


class DeviceAugmenter(object):
    """Runs myolo_augment_batch: raw bytes, un-augmented instance masks and class ids, one parameter row per image -> the device batch dict
    Net.forward_backward consumes.  T = cfg.TRUE_BOX_BUFFER (= cfg.MAX_GT_INSTANCES) slots per image; a class id of 0 marks an empty slot."""

    def __init__(self, cfg, device="cuda:0", cval=0.0):
        import torch
        from . import _ext as X
        X.load()
        self.cfg = cfg
        self.dev = torch.device(device)
        self.cval = float(cval)
        self.anchors = torch.tensor(np.asarray(cfg.ANCHORS, np.float64).reshape(-1), device=self.dev)
        self._ws = None

    def _dev(self, a, dtype, shape):
        import torch
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(
                {torch.uint8: np.uint8, torch.int32: np.int32, torch.float64: np.float64}[dtype], copy=False)))
        if a.dtype != dtype:
            raise ValueError("DeviceAugmenter: expected %s, got %s" % (dtype, a.dtype))
        if tuple(a.shape) != tuple(shape):
            raise ValueError("DeviceAugmenter: expected shape %s, got %s" % (tuple(shape), tuple(a.shape)))
        return a.to(self.dev).contiguous()

    def apply(self, raw_images, gt_masks, gt_ids, params, yolo=False, stream=None, consumer=None):
        """raw_images [B,H,W,3] uint8, gt_masks [B,H,W,T] uint8 / bool 0-1, gt_ids [B,T] int32 (0 = empty slot), params [B,8] float64 --
        numpy arrays (uploaded here) or device tensors.  -> dict(images, true_boxes, y_true, gt_ids, gt_boxes, gt_masks), the first three
        with yolo=True.  stream / consumer: as ShapesProducer.batch -- produce on `stream`, the dict carries the event `_ready` and its
        tensors are registered with the stream that will read them."""
        import torch
        from . import _ext as X
        if stream is not None:
            with torch.cuda.stream(stream):
                d = self.apply(raw_images, gt_masks, gt_ids, params, yolo=yolo)
                ev = torch.cuda.Event()
                ev.record(stream)
            if consumer is not None:
                for t in d.values():
                    if isinstance(t, torch.Tensor):
                        t.record_stream(consumer)
            d["_ready"] = ev
            return d
        cfg = self.cfg
        H, W = cfg.IMAGE_SHAPE[0], cfg.IMAGE_SHAPE[1]
        G, A, C, T = cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES, cfg.TRUE_BOX_BUFFER
        if cfg.GRID_H != G or cfg.MAX_GT_INSTANCES != T:
            raise ValueError("DeviceAugmenter needs a square grid and MAX_GT_INSTANCES == TRUE_BOX_BUFFER")
        B = int(raw_images.shape[0])
        if isinstance(gt_masks, np.ndarray) and gt_masks.dtype == bool:
            gt_masks = gt_masks.view(np.uint8)
        if isinstance(raw_images, np.ndarray) and raw_images.dtype != np.uint8:
            raise ValueError("DeviceAugmenter needs uint8 images, got %s" % raw_images.dtype)
        src = (self._dev(raw_images, torch.uint8, (B, H, W, 3)), self._dev(gt_masks, torch.uint8, (B, H, W, T)),
               self._dev(gt_ids, torch.int32, (B, T)), self._dev(params, torch.float64, (B, 8)))
        need = X.augment_ws_bytes(B, T)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.dev)
        d = dict(images=torch.empty(B, H, W, 3, device=self.dev),
                 true_boxes=torch.empty(B, T, 4, device=self.dev),
                 y_true=torch.empty(B, G, G, A, 5 + C, device=self.dev),
                 gt_ids=torch.empty(B, T, dtype=torch.int32, device=self.dev),
                 gt_boxes=torch.empty(B, T, 4, dtype=torch.int32, device=self.dev),
                 gt_masks=torch.empty(B, H, W, T, dtype=torch.uint8, device=self.dev))
        X.call("myolo_augment_batch", X.ptr(src[0]), X.ptr(src[1]), X.ptr(src[2]), X.ptr(src[3]), self.cval, X.ptr(self.anchors),
               X.ptr(d["images"]), X.ptr(d["gt_masks"]), X.ptr(d["gt_boxes"]), X.ptr(d["gt_ids"]), X.ptr(d["y_true"]), X.ptr(d["true_boxes"]),
               B, H, W, T, G, A, C, self._ws.data_ptr(), self._ws.numel(), X.stream())
        if yolo:
            # the step reads three arrays; the other three stay on the dict's side until the kernels that wrote them have run
            d = dict(images=d["images"], true_boxes=d["true_boxes"], y_true=d["y_true"], _gt=(d["gt_ids"], d["gt_boxes"], d["gt_masks"]))
        d["_src"] = src            # the kernels read them asynchronously
        return d

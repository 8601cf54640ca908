"""
Training augmentation on the device: random horizontal flip, scale, translation, rotation, brightness gain and offset.

The reference augments on the host through imgaug (model.py:943-1060 `augmentation=`, myolo_utils.py:313-343).  Here the host only
draws one row of eight doubles per image -- Augmentation.params() -- and the warp itself is one more device producer of the six training
inputs (DeviceAugmenter -> myolo_augment_batch, csrc/augment_kernels.hip): bilinear image, nearest-neighbour masks, empty instances
dropped, boxes re-derived from the warped masks, YOLO targets encoded from those boxes.  The arithmetic is a bit-exact contract, stated
in DESIGN.md ("On-device augmentation") and restated in numpy by tests/augment_ref.py.

Mosaic (MaskYOLO.train(mosaic=Mosaic(...))) composes every sample from four images of its batch: the host plans three small tables per batch
(Mosaic.plan, Mosaic.compose) and the same augmenter runs myolo_mosaic_batch on them -- DESIGN.md ("Mosaic"), tests/mosaic_ref.py.

Copy-paste (MaskYOLO.train(copy_paste=CopyPaste(...))) pastes instances of one augmented sample of the batch into another: the host plans two
small tables per batch (CopyPaste.plan) and the augmenter runs myolo_copy_paste_batch behind either entry -- DESIGN.md ("Copy-paste"),
tests/copy_paste_ref.py.
"""
import math

import numpy as np

IDENTITY_ROW = np.array([1., 0., 0., 0., 1., 0., 1., 0.], dtype=np.float64)
IDENTITY_TILE = np.array([1., 0., 0., 0., 1., 0.], dtype=np.float64)


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


class Mosaic(object):
    """What MaskYOLO.train(mosaic=...) takes: a sample is cut at a random point into four tiles, tile 0 (top left) showing the sample itself and
    the others three images of the same batch, each zoomed about the frame corner that faces the cut.

    p       probability that a sample is mosaicked
    centre  (low, high) cut point as a fraction of each side, drawn independently for x and y, within [0, 1]
    zoom    (low, high) zoom factor of a tile's image, drawn per tile, > 0
    seed    plan() is a pure function of (seed, epoch, image ids, eligible)

    Tile q = (x >= cx) + 2 * (y >= cy).  With integer pixel positions at pixel centres the frame is [-0.5, W-0.5] x [-0.5, H-0.5] and the cut lies at
    (cx-0.5, cy-0.5); tile q pins the corner k_q of its image's frame to the cut -- k_0 = (W-0.5, H-0.5), k_1 = (-0.5, H-0.5), k_2 = (W-0.5, -0.5),
    k_3 = (-0.5, -0.5) -- so its map from an output pixel to a position in its image's own frame is  u = k_q + (out - cut) / z_q."""

    DRAWS = 10           # per sample: mosaicked?, centre x, centre y, three partners, four zooms

    def __init__(self, p=1.0, centre=(0.25, 0.75), zoom=(0.5, 1.0), seed=0):
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError("p is a probability in [0, 1], got %r" % (p,))
        self.p = p
        self.centre = _pair("centre", centre, lo=0.0, hi=1.0)
        self.zoom = _pair("zoom", zoom, lo=0.0, lo_open=True)
        seed = int(seed)
        if not 0 <= seed < 2 ** 32:
            raise ValueError("seed must be in [0, 2**32), got %r" % (seed,))
        self.seed = seed

    def plan(self, epoch, image_ids, H, W, eligible=None):
        """-> (src int32 [B,4], tiles float64 [B,4,6], centre int32 [B,2]) for a batch whose position b holds dataset image image_ids[b].
        src[b,q]: the batch position tile q shows (src[b,0] = b); tiles[b,q]: m00 m01 m02 m10 m11 m12, output pixel -> position in that image's own
        frame; centre[b] = (cx, cy).  eligible: the batch positions that may be mosaicked and used as partners, in batch order (default: all; a
        partner may repeat and may be b itself).  Position b always takes the same DRAWS draws in the same order from
        RandomState([seed, epoch, image_ids[b]]), whatever the ranges: u0 < p mosaics it, u1 / u2 place the cut (round(fraction x side), clamped to
        [1, side-1]), u3..u5 pick the partners eligible[floor(u * len(eligible))] of tiles 1..3, u6..u9 are the zooms of tiles 0..3.  A sample that
        is not mosaicked (u0 >= p, or b not eligible) gets src = [b,b,b,b], identity tiles and the centre (W, H): every pixel in tile 0."""
        B = len(image_ids)
        eligible = list(range(B)) if eligible is None else [int(e) for e in eligible]
        if any(not 0 <= e < B for e in eligible):
            raise ValueError("eligible holds batch positions in [0, %d), got %r" % (B, eligible))
        src = np.repeat(np.arange(B, dtype=np.int32)[:, None], 4, axis=1)
        tiles = np.tile(IDENTITY_TILE, (B, 4, 1))
        centre = np.tile(np.array([W, H], np.int32), (B, 1))
        u = np.empty((B, self.DRAWS))
        rs = np.random.RandomState(0)          # re-seeded per sample: the draws of a fresh RandomState([seed, epoch, id]) at a tenth of its cost
        for b in range(B):
            rs.seed([self.seed, int(epoch), int(image_ids[b])])
            u[b] = rs.random_sample(self.DRAWS)
        on = u[:, 0] < self.p
        on &= np.isin(np.arange(B), eligible)
        if not on.any():
            return src, tiles, centre

        def between(r, x):
            return r[0] + (r[1] - r[0]) * x if r[1] > r[0] else np.full_like(x, r[0])
        cx = np.clip(np.floor(between(self.centre, u[:, 1]) * W + 0.5).astype(np.int64), 1, W - 1)
        cy = np.clip(np.floor(between(self.centre, u[:, 2]) * H + 0.5).astype(np.int64), 1, H - 1)
        partner = np.minimum((u[:, 3:6] * len(eligible)).astype(np.int64), len(eligible) - 1)
        a = 1.0 / between(self.zoom, u[:, 6:10])                                          # [B,4]; zoom 1 gives exactly 1
        kx, ky = np.array([W - 0.5, -0.5, W - 0.5, -0.5]), np.array([H - 0.5, H - 0.5, -0.5, -0.5])
        zero = np.zeros_like(a)
        drawn = np.stack([a, zero, kx - a * (cx[:, None] - 0.5), zero, a, ky - a * (cy[:, None] - 0.5)], axis=-1)
        src[on, 1:] = np.asarray(eligible, np.int32)[partner[on]]
        tiles[on] = drawn[on]
        centre[on] = np.stack([cx, cy], axis=-1)[on]
        return src, tiles, centre

    @staticmethod
    def compose(tiles, src, rows):
        """-> float64 [B,4,8], the rows myolo_mosaic_batch reads: tile (b,q)'s map followed by the Augmentation row r = rows[src[b,q]] of the image it
        shows -- output pixel -> source position in image src[b,q]; gain and bias are r's.  With the tile a = tiles[b,q], each entry is these binary64
        operations in this order:
            m00 = r0*a0 + r1*a3        m01 = r0*a1 + r1*a4        m02 = (r0*a2 + r1*a5) + r2
            m10 = r3*a0 + r4*a3        m11 = r3*a1 + r4*a4        m12 = (r3*a2 + r4*a5) + r5
        A tile that is exactly the identity [1,0,0, 0,1,0] copies r instead, so that it leaves the row unchanged to the bit."""
        tiles, src, rows = np.asarray(tiles, np.float64), np.asarray(src), np.asarray(rows, np.float64)
        r = rows[src]                                              # [B,4,8]
        a = tiles
        out = r.copy()
        out[..., 0] = r[..., 0] * a[..., 0] + r[..., 1] * a[..., 3]
        out[..., 1] = r[..., 0] * a[..., 1] + r[..., 1] * a[..., 4]
        out[..., 2] = (r[..., 0] * a[..., 2] + r[..., 1] * a[..., 5]) + r[..., 2]
        out[..., 3] = r[..., 3] * a[..., 0] + r[..., 4] * a[..., 3]
        out[..., 4] = r[..., 3] * a[..., 1] + r[..., 4] * a[..., 4]
        out[..., 5] = (r[..., 3] * a[..., 2] + r[..., 4] * a[..., 5]) + r[..., 5]
        same = (a == IDENTITY_TILE).all(axis=-1)
        out[same] = r[same]
        return out

    def __repr__(self):
        return "Mosaic(p=%r, centre=%r, zoom=%r, seed=%r)" % (self.p, self.centre, self.zoom, self.seed)


def check_mosaic_tables(quad_src, centre, B, H, W):
    """myolo_mosaic_batch does not read its tables on the host, so they are checked here, on the host arrays, before they are uploaded: sources in
    [0, B), centres in [0, W] x [0, H]."""
    quad_src, centre = np.asarray(quad_src), np.asarray(centre)
    if quad_src.shape != (B, 4) or centre.shape != (B, 2):
        raise ValueError("mosaic tables: expected quad_src [%d,4] and centre [%d,2], got %s and %s" % (B, B, quad_src.shape, centre.shape))
    if ((quad_src < 0) | (quad_src >= B)).any():
        raise ValueError("mosaic tables: quad_src holds batch positions in [0, %d)" % B)
    if ((centre < 0) | (centre > np.array([W, H]))).any():
        raise ValueError("mosaic tables: a centre lies in [0, %d] x [0, %d]" % (W, H))


class CopyPaste(object):
    """What MaskYOLO.train(copy_paste=...) takes: a sample receives instances of another sample of its batch -- their pixels replace its own, their
    masks occlude its instances -- after both have been augmented ("Copy-paste").

    p          probability that a sample receives a paste
    instances  probability that each instance slot of the donor is selected
    seed       plan() is a pure function of (seed, epoch, image ids, eligible, T)"""

    DRAWS = 34           # per sample: pasted?, the donor, one per instance slot (32 at the most)

    def __init__(self, p=0.5, instances=0.5, seed=0):
        p, instances = float(p), float(instances)
        if not 0.0 <= p <= 1.0:
            raise ValueError("p is a probability in [0, 1], got %r" % (p,))
        if not 0.0 <= instances <= 1.0:
            raise ValueError("instances is a probability in [0, 1], got %r" % (instances,))
        self.p, self.instances = p, instances
        seed = int(seed)
        if not 0 <= seed < 2 ** 32:
            raise ValueError("seed must be in [0, 2**32), got %r" % (seed,))
        self.seed = seed

    def plan(self, epoch, image_ids, T, eligible=None):
        """-> (donor int32 [B], select int32 [B]) for a batch whose position b holds dataset image image_ids[b] in T instance slots.
        donor[b]: the batch position whose instances b receives; bit t of select[b]: the donor's slot t is selected (a bit pattern: bit 31 is the
        sign bit when T = 32).  The slots are those of the donor AFTER the first stage -- the host cannot know which survive the warp -- and the
        device ignores selected slots that are empty.  eligible: the batch positions that may receive and donate, in batch order (default: all).
        Position b always takes the same DRAWS draws in the same order from RandomState([seed, epoch, image_ids[b], 2]) -- the fourth element keeps
        the stream apart from Augmentation's and Mosaic's: u0 < p turns the paste on, u1 picks the donor others[floor(u1 * len(others))], others =
        eligible without b, and bit t < T is set iff u[2+t] < instances.  A sample that is not eligible, did not draw u0 < p or has nobody else to
        take from gets donor[b] = b, select[b] = 0."""
        B, T = len(image_ids), int(T)
        if not 1 <= T <= 32:
            raise ValueError("T is the number of instance slots, 1..32, got %r" % (T,))
        eligible = list(range(B)) if eligible is None else [int(e) for e in eligible]
        if any(not 0 <= e < B for e in eligible):
            raise ValueError("eligible holds batch positions in [0, %d), got %r" % (B, eligible))
        donor = np.arange(B, dtype=np.int32)
        select = np.zeros(B, np.uint32)
        rs = np.random.RandomState(0)          # re-seeded per sample, as in Mosaic.plan
        for b in range(B):
            rs.seed([self.seed, int(epoch), int(image_ids[b]), 2])
            u = rs.random_sample(self.DRAWS)
            others = [e for e in eligible if e != b]
            if b not in eligible or not u[0] < self.p or not others:
                continue
            donor[b] = others[min(int(u[1] * len(others)), len(others) - 1)]
            select[b] = sum(1 << t for t in range(T) if u[2 + t] < self.instances)
        return donor, select.view(np.int32)

    def __repr__(self):
        return "CopyPaste(p=%r, instances=%r, seed=%r)" % (self.p, self.instances, self.seed)


def check_paste_tables(donor, select, B, T):
    """myolo_copy_paste_batch does not read its tables on the host, so they are checked here, on the host arrays, before they are uploaded: donors in
    [0, B), no selected slot at or above T."""
    donor, select = np.asarray(donor), np.asarray(select)
    if donor.shape != (B,) or select.shape != (B,):
        raise ValueError("copy-paste tables: expected donor [%d] and select [%d], got %s and %s" % (B, B, donor.shape, select.shape))
    if donor.dtype.kind not in "iu" or select.dtype.kind not in "iu":
        raise ValueError("copy-paste tables: integer arrays, got %s and %s" % (donor.dtype, select.dtype))
    if ((donor < 0) | (donor >= B)).any():
        raise ValueError("copy-paste tables: donor holds batch positions in [0, %d)" % B)
    if select.dtype.itemsize > 4 and ((select < -(1 << 31)) | (select >= (1 << 32))).any():
        raise ValueError("copy-paste tables: select holds 32-bit patterns")
    if (((select.astype(np.int64) & 0xffffffff) >> T) != 0).any():
        raise ValueError("copy-paste tables: select names a slot at or above T = %d" % T)


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

    def apply(self, raw_images, gt_masks, gt_ids, params, yolo=False, stream=None, consumer=None, mosaic=None, copy_paste=None):
        """raw_images [B,H,W,3] uint8, gt_masks [B,H,W,T] uint8 / bool 0-1, gt_ids [B,T] int32 (0 = empty slot), params [B,8] float64 --
        numpy arrays (uploaded here) or device tensors.  -> dict(images, true_boxes, y_true, gt_ids, gt_boxes, gt_masks), the first three
        with yolo=True.  stream / consumer: as ShapesProducer.batch -- produce on `stream`, the dict carries the event `_ready` and its
        tensors are registered with the stream that will read them.
        mosaic = (quad_src int32 [B,4], quad_rows float64 [B,4,8], centre int32 [B,2]) (Mosaic.plan / Mosaic.compose): myolo_mosaic_batch instead,
        which reads quad_rows in place of params; the dict gains "mosaic_dropped" int32 [B], the survivors beyond T that were discarded.  Tables
        given as numpy arrays are checked here (check_mosaic_tables); device tensors must have been checked before their upload, as
        MaskYOLO.train() does.
        copy_paste = (donor int32 [B], select int32 [B]) (CopyPaste.plan): myolo_copy_paste_batch runs behind either entry on the same stream, on
        that entry's images, masks and class ids (its targets are not encoded), and its outputs are the dict's, which gains "paste_dropped" int32
        [B], the selected instances that found no free slot.  Numpy tables are checked here (check_paste_tables); device tensors as above."""
        import torch
        from . import _ext as X
        if stream is not None:
            with torch.cuda.stream(stream):
                d = self.apply(raw_images, gt_masks, gt_ids, params, yolo=yolo, mosaic=mosaic, copy_paste=copy_paste)
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
        if mosaic is not None and not (isinstance(mosaic[0], torch.Tensor) and isinstance(mosaic[2], torch.Tensor)):
            check_mosaic_tables(mosaic[0], mosaic[2], B, H, W)
        if copy_paste is not None and not (isinstance(copy_paste[0], torch.Tensor) and isinstance(copy_paste[1], torch.Tensor)):
            check_paste_tables(copy_paste[0], copy_paste[1], B, T)
        src = (self._dev(raw_images, torch.uint8, (B, H, W, 3)), self._dev(gt_masks, torch.uint8, (B, H, W, T)),
               self._dev(gt_ids, torch.int32, (B, T)), self._dev(params, torch.float64, (B, 8)))
        if mosaic is not None:
            src += (self._dev(mosaic[0], torch.int32, (B, 4)), self._dev(mosaic[1], torch.float64, (B, 4, 8)),
                    self._dev(mosaic[2], torch.int32, (B, 2)))
        need = X.augment_ws_bytes(B, T) if mosaic is None else X.mosaic_ws_bytes(B, T)
        if copy_paste is not None:
            need = max(need, X.copy_paste_ws_bytes(B, T))      # (one workspace: the second stage runs behind the first on the same stream)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.dev)
        d = dict(images=torch.empty(B, H, W, 3, device=self.dev),
                 true_boxes=torch.empty(B, T, 4, device=self.dev),
                 y_true=torch.empty(B, G, G, A, 5 + C, device=self.dev),
                 gt_ids=torch.empty(B, T, dtype=torch.int32, device=self.dev),
                 gt_boxes=torch.empty(B, T, 4, dtype=torch.int32, device=self.dev),
                 gt_masks=torch.empty(B, H, W, T, dtype=torch.uint8, device=self.dev))
        outs = (X.ptr(d["images"]), X.ptr(d["gt_masks"]), X.ptr(d["gt_boxes"]), X.ptr(d["gt_ids"]), X.ptr(d["y_true"]), X.ptr(d["true_boxes"]))
        if copy_paste is not None:
            # the first stage writes four intermediate arrays and encodes no target; the second stage writes the dict's six
            final = outs
            mid = (torch.empty_like(d["images"]), torch.empty_like(d["gt_masks"]), torch.empty_like(d["gt_boxes"]), torch.empty_like(d["gt_ids"]))
            outs = tuple(X.ptr(t) for t in mid) + (None, None)
        if mosaic is None:
            X.call("myolo_augment_batch", X.ptr(src[0]), X.ptr(src[1]), X.ptr(src[2]), X.ptr(src[3]), self.cval, X.ptr(self.anchors), *outs,
                   B, H, W, T, G, A, C, self._ws.data_ptr(), self._ws.numel(), X.stream())
        else:
            dropped = torch.empty(B, dtype=torch.int32, device=self.dev)
            X.call("myolo_mosaic_batch", X.ptr(src[0]), X.ptr(src[1]), X.ptr(src[2]), X.ptr(src[4]), X.ptr(src[5]), X.ptr(src[6]), self.cval,
                   X.ptr(self.anchors), *outs, X.ptr(dropped), B, H, W, T, G, A, C, self._ws.data_ptr(), self._ws.numel(), X.stream())
        if copy_paste is not None:
            tables = (self._dev(copy_paste[0], torch.int32, (B,)), self._dev(copy_paste[1], torch.int32, (B,)))
            paste_dropped = torch.empty(B, dtype=torch.int32, device=self.dev)
            X.call("myolo_copy_paste_batch", X.ptr(mid[0]), X.ptr(mid[1]), X.ptr(mid[3]), X.ptr(tables[0]), X.ptr(tables[1]), X.ptr(self.anchors),
                   *final, X.ptr(paste_dropped), B, H, W, T, G, A, C, self._ws.data_ptr(), self._ws.numel(), X.stream())
        if yolo:
            # the step reads three arrays; the other three stay on the dict's side until the kernels that wrote them have run
            d = dict(images=d["images"], true_boxes=d["true_boxes"], y_true=d["y_true"], _gt=(d["gt_ids"], d["gt_boxes"], d["gt_masks"]))
        if mosaic is not None:
            d["mosaic_dropped"] = dropped
        if copy_paste is not None:
            d["paste_dropped"] = paste_dropped
            d["_paste_src"] = mid + tables      # the first stage's images, masks, boxes and ids, then donor and select: read asynchronously too
        d["_src"] = src            # the kernels read them asynchronously
        return d

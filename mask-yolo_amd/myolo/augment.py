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

Photometric (MaskYOLO.train(photometric=Photometric(...))) changes the pixels only -- hue, saturation, contrast, Gaussian blur, noise: the host
draws one row of 32 doubles per image (Photometric.row) and the augmenter runs myolo_photometric_batch (csrc/photometric_kernels.hip) last of
all -- DESIGN.md ("Photometric augmentation"), tests/photometric_ref.py.
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


PHOTO_ROW = 32           # doubles per image: A [0:12], noise deviation [12], noise key [13], blur radius [14], 0 [15], blur weights [16:32]
PHOTO_MAX_RADIUS = 15
_HUE_K = np.array([[0., -1., 1.], [1., 0., -1.], [-1., 1., 0.]])
_LUMA = np.array([0.299, 0.587, 0.114])


def photo_reflect(i, n):
    """reflect-101 index of the blur: ... 2 1 | 0 1 .. n-1 | n-2 ...; valid however far i lies outside [0, n)"""
    if n == 1:
        return 0
    P = 2 * (n - 1)
    m = ((i % P) + P) % P
    return m if m < n else P - m


class Photometric(object):
    """What MaskYOLO.train(photometric=...) takes: colour, blur and noise applied to a training image on the device, after every geometric stage
    ("Photometric augmentation").

    p           probability that a sample is touched at all
    hue         (low, high) rotation of the colour about the grey axis in degrees, within [-180, 180]
    saturation  (low, high) gain, >= 0
    contrast    (low, high) gain about mid-grey, >= 0
    blur        (low, high) Gaussian sigma in pixels, within [0, 5]
    noise       (low, high) standard deviation of additive noise as a fraction of full scale, within [0, 1]
    seed        row() is a pure function of (seed, epoch, image_id)"""

    DRAWS = 7            # per sample: touched?, hue, saturation, contrast, sigma, noise deviation, noise key

    def __init__(self, p=1.0, hue=(0., 0.), saturation=(1., 1.), contrast=(1., 1.), blur=(0., 0.), noise=(0., 0.), seed=0):
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError("p is a probability in [0, 1], got %r" % (p,))
        self.p = p
        self.hue = _pair("hue", hue, lo=-180.0, hi=180.0)
        self.saturation = _pair("saturation", saturation, lo=0.0)
        self.contrast = _pair("contrast", contrast, lo=0.0)
        self.blur = _pair("blur", blur, lo=0.0, hi=5.0)
        self.noise = _pair("noise", noise, lo=0.0, hi=1.0)
        seed = int(seed)
        if not 0 <= seed < 2 ** 32:
            raise ValueError("seed must be in [0, 2**32), got %r" % (seed,))
        self.seed = seed

    @classmethod
    def around(cls, hue=0.0, saturation=0.0, contrast=0.0, blur=0.0, noise=0.0, p=1.0, seed=0):
        """the ranges the example scripts' flags name: symmetric about the neutral value -- hue (-hue, hue) degrees, saturation and contrast
        (max(0, 1 - f), 1 + f) -- and from zero for blur (0, sigma) and noise (0, deviation)"""
        return cls(p=p, hue=(-hue, hue), saturation=(max(0.0, 1.0 - saturation), 1.0 + saturation), contrast=(max(0.0, 1.0 - contrast), 1.0 + contrast),
                   blur=(0.0, blur), noise=(0.0, noise), seed=seed)

    @property
    def max_radius(self):
        """the largest blur radius a row of this object can hold: what myolo_photometric_batch takes as its bound"""
        return self.kernel(self.blur[1])[0]

    def draw(self, epoch, image_id, rs=None):
        """-> dict(on, hue, saturation, contrast, sigma, std, key): the raw draws.  Always the same seven draws in the same order from
        RandomState([seed, epoch, image_id, 1]), whatever the ranges -- the fourth element keeps the stream apart from Augmentation's.
        rs: a RandomState of the caller's to re-seed instead (its state is lost): the same draws at a fraction of a fresh generator's cost, as
        in Mosaic.plan."""
        key = [self.seed, int(epoch), int(image_id), 1]
        if rs is None:
            rs = np.random.RandomState(key)
        else:
            rs.seed(key)
        u = rs.random_sample(self.DRAWS)

        def between(r, x):
            return r[0] + (r[1] - r[0]) * x if r[1] > r[0] else r[0]
        return dict(on=bool(u[0] < self.p), hue=between(self.hue, u[1]), saturation=between(self.saturation, u[2]),
                    contrast=between(self.contrast, u[3]), sigma=between(self.blur, u[4]), std=between(self.noise, u[5]),
                    key=min(int(u[6] * 4294967296.0), 2 ** 32 - 1))

    @staticmethod
    def matrix(hue, saturation, contrast):
        """-> float64 [3,4], the colour transform [c * S * R | 0.5 * (1 - c)] of a hue rotation in degrees, a saturation and a contrast gain:
        R = cos h * I + (1 - cos h)/3 * J + (sin h / sqrt 3) * K, S = s * I + (1 - s) * 1 L^T.  h = 0, s = 1 and c = 1 are taken without arithmetic."""
        h, s, c = float(hue), float(saturation), float(contrast)
        eye = np.eye(3)
        if h == 0.0:
            R = eye
        else:
            co, si = math.cos(math.radians(h)), math.sin(math.radians(h))
            R = co * eye + (1.0 - co) / 3.0 * np.ones((3, 3)) + (si / math.sqrt(3.0)) * _HUE_K
        S = eye if s == 1.0 else s * eye + (1.0 - s) * np.tile(_LUMA, (3, 1))
        M = R if s == 1.0 else (S if h == 0.0 else S.dot(R))
        A = np.zeros((3, 4))
        A[:, :3] = M if c == 1.0 else c * M
        A[:, 3] = 0.0 if c == 1.0 else 0.5 * (1.0 - c)
        return A + 0.0                                             # (-0.0 -> 0.0)

    @staticmethod
    def kernel(sigma):
        """-> (r, w float64 [16]): r = min(15, ceil(3 sigma)); w_k proportional to exp(-k^2 / (2 sigma^2)) for k <= r and 0 beyond, normalised to
        w_0 + 2 * sum_{k>=1} w_k = 1.  sigma = 0 gives r = 0, and r = 0 gives exactly w_0 = 1."""
        sigma = float(sigma)
        w = np.zeros(PHOTO_MAX_RADIUS + 1)
        r = min(PHOTO_MAX_RADIUS, int(math.ceil(3.0 * sigma))) if sigma > 0.0 else 0
        if r == 0:
            w[0] = 1.0
            return 0, w
        k = np.arange(r + 1, dtype=np.float64)
        with np.errstate(all="ignore"):                            # (a sigma whose square underflows: every w_k beyond w_0 is 0)
            g = np.exp(-(k * k) / (2.0 * sigma * sigma))
        g[0] = 1.0
        w[:r + 1] = g / (g[0] + 2.0 * g[1:].sum())
        return r, w

    def row(self, epoch, image_id, rs=None):
        """-> float64[32], the row myolo_photometric_batch reads (layout: PHOTO_ROW); identity() for a sample that is not picked.  rs: as draw."""
        d = self.draw(epoch, image_id, rs)
        if not d["on"]:
            return self.identity()
        row = np.zeros(PHOTO_ROW)
        row[0:12] = self.matrix(d["hue"], d["saturation"], d["contrast"]).reshape(-1)
        row[12], row[13] = d["std"], (float(d["key"]) if d["std"] > 0.0 else 0.0)      # (no noise: the key is not used, and the defaults give identity())
        r, w = self.kernel(d["sigma"])
        row[14], row[16:32] = float(r), w
        return row

    @staticmethod
    def identity():
        row = np.zeros(PHOTO_ROW)
        row[0] = row[5] = row[10] = row[16] = 1.0
        return row

    def __repr__(self):
        return ("Photometric(p=%r, hue=%r, saturation=%r, contrast=%r, blur=%r, noise=%r, seed=%r)" %
                (self.p, self.hue, self.saturation, self.contrast, self.blur, self.noise, self.seed))


def check_photo_rows(rows, B):
    """myolo_photometric_batch does not read its rows on the host, so they are checked here, on the host array, before they are uploaded: finite
    entries, a radius that is an integer in 0..15, weights >= 0, a deviation >= 0, a key that is an integer in [0, 2**32)."""
    rows = np.asarray(rows)
    if rows.shape != (B, PHOTO_ROW) or rows.dtype != np.float64:
        raise ValueError("photometric rows: expected float64 [%d,%d], got %s %s" % (B, PHOTO_ROW, rows.dtype, rows.shape))
    if not np.isfinite(rows).all():
        raise ValueError("photometric rows: every entry is finite")
    r = rows[:, 14]
    if ((r != np.floor(r)) | (r < 0) | (r > PHOTO_MAX_RADIUS)).any():
        raise ValueError("photometric rows: the blur radius is an integer in 0..%d" % PHOTO_MAX_RADIUS)
    if (rows[:, 16:32] < 0).any():
        raise ValueError("photometric rows: a blur weight is >= 0")
    if (rows[:, 12] < 0).any():
        raise ValueError("photometric rows: the noise deviation is >= 0")
    k = rows[:, 13]
    if ((k != np.floor(k)) | (k < 0) | (k >= 4294967296.0)).any():
        raise ValueError("photometric rows: the noise key is an integer in [0, 2**32)")


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

    def apply(self, raw_images, gt_masks, gt_ids, params, yolo=False, stream=None, consumer=None, mosaic=None, copy_paste=None, photometric=None):
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
        [B], the selected instances that found no free slot.  Numpy tables are checked here (check_paste_tables); device tensors as above.
        photometric = rows float64 [B,32] (Photometric.row), or (rows, max_radius): myolo_photometric_batch runs last of all on the same stream, on
        the image of the stage before it, into the dict's images; masks, boxes, ids and targets are that stage's.  max_radius is the host-known
        bound on the rows' blur radius (default: the largest radius of numpy rows, 15 for a device tensor).  Numpy rows are checked here
        (check_photo_rows); a device tensor as above."""
        import torch
        from . import _ext as X
        if stream is not None:
            with torch.cuda.stream(stream):
                d = self.apply(raw_images, gt_masks, gt_ids, params, yolo=yolo, mosaic=mosaic, copy_paste=copy_paste, photometric=photometric)
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
        if photometric is not None:
            photo_rows, photo_radius = photometric if isinstance(photometric, tuple) else (photometric, None)
            if not isinstance(photo_rows, torch.Tensor):
                photo_rows = np.ascontiguousarray(photo_rows, dtype=np.float64)
                check_photo_rows(photo_rows, B)
                if photo_radius is None:
                    photo_radius = int(photo_rows[:, 14].max())
            photo_radius = PHOTO_MAX_RADIUS if photo_radius is None else int(photo_radius)
            if not 0 <= photo_radius <= PHOTO_MAX_RADIUS:
                raise ValueError("photometric: max_radius is in 0..%d, got %r" % (PHOTO_MAX_RADIUS, photo_radius))
        src = (self._dev(raw_images, torch.uint8, (B, H, W, 3)), self._dev(gt_masks, torch.uint8, (B, H, W, T)),
               self._dev(gt_ids, torch.int32, (B, T)), self._dev(params, torch.float64, (B, 8)))
        if mosaic is not None:
            src += (self._dev(mosaic[0], torch.int32, (B, 4)), self._dev(mosaic[1], torch.float64, (B, 4, 8)),
                    self._dev(mosaic[2], torch.int32, (B, 2)))
        need = X.augment_ws_bytes(B, T) if mosaic is None else X.mosaic_ws_bytes(B, T)
        if copy_paste is not None:
            need = max(need, X.copy_paste_ws_bytes(B, T))      # (one workspace: the second stage runs behind the first on the same stream)
        if photometric is not None:
            need = max(need, X.photometric_ws_bytes(B, H, W, photo_radius))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.dev)
        d = dict(images=torch.empty(B, H, W, 3, device=self.dev),
                 true_boxes=torch.empty(B, T, 4, device=self.dev),
                 y_true=torch.empty(B, G, G, A, 5 + C, device=self.dev),
                 gt_ids=torch.empty(B, T, dtype=torch.int32, device=self.dev),
                 gt_boxes=torch.empty(B, T, 4, dtype=torch.int32, device=self.dev),
                 gt_masks=torch.empty(B, H, W, T, dtype=torch.uint8, device=self.dev))
        outs = (X.ptr(d["images"]), X.ptr(d["gt_masks"]), X.ptr(d["gt_boxes"]), X.ptr(d["gt_ids"]), X.ptr(d["y_true"]), X.ptr(d["true_boxes"]))
        if photometric is not None:
            # the stage before the last writes its image to an intermediate tensor; the photometric stage writes the dict's
            photo_src = torch.empty_like(d["images"])
            outs = (X.ptr(photo_src),) + outs[1:]
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
        if photometric is not None:
            photo_rows = self._dev(photo_rows, torch.float64, (B, PHOTO_ROW))
            X.call("myolo_photometric_batch", X.ptr(photo_src), X.ptr(photo_rows), X.ptr(d["images"]), photo_radius, B, H, W,
                   self._ws.data_ptr(), self._ws.numel(), X.stream())
        if yolo:
            # the step reads three arrays; the other three stay on the dict's side until the kernels that wrote them have run
            d = dict(images=d["images"], true_boxes=d["true_boxes"], y_true=d["y_true"], _gt=(d["gt_ids"], d["gt_boxes"], d["gt_masks"]))
        if mosaic is not None:
            d["mosaic_dropped"] = dropped
        if copy_paste is not None:
            d["paste_dropped"] = paste_dropped
            d["_paste_src"] = mid + tables      # the first stage's images, masks, boxes and ids, then donor and select: read asynchronously too
        if photometric is not None:
            d["_photo_src"] = (photo_src, photo_rows)      # the image of the stage before and the rows: read asynchronously too
        d["_src"] = src            # the kernels read them asynchronously
        return d

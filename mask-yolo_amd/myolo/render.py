"""The overlay of a detection result: what the reference's visualize.display_instances draws over the image -- every mask blended in
(apply_mask), the mask outlines, the dashed boxes -- stated in numpy.  This is the specification the device renderer is held to
(myolo_render_instances): Net.render_instances gives these bytes.  Captions are left out: they need a font, and the class
and the score of every instance are in the result dict.

write_png / read_png: 8-bit RGB PNG files with the standard library alone."""
import colorsys
import struct
import zlib

import numpy as np

BOX_RING = 2        # the box is drawn this many pixels wide (the reference's linewidth=2) ...
BOX_DASH = 6        # ... in dashes of this many pixels, a gap of as many between two


def instance_colors(n):
    """the reference's random_colors(n, bright=True) before its shuffle: n hues around the circle at full saturation and value, as [(r, g, b)]
    of Python floats in [0, 1], in slot order"""
    return [colorsys.hsv_to_rgb(i / n, 1, 1.0) for i in range(n)]


def blend(canvas, where, color, alpha):
    """the reference's apply_mask on a uint32 [h,w,3] canvas, in place: where `where` holds, channel c becomes
    canvas * (1 - alpha) + alpha * color[c] * 255, formed in float64 in this order and truncated by the store into the canvas"""
    for c in range(3):
        canvas[:, :, c] = np.where(where, canvas[:, :, c] * (1 - alpha) + alpha * color[c] * 255, canvas[:, :, c])
    return canvas


def outline(mask):
    """the set pixels of a bool [h,w] mask that lie on the frame's border or have a 4-neighbour that is not set: the one-pixel stand-in for the
    find_contours polygon of the zero-padded mask"""
    p = np.zeros((mask.shape[0] + 2, mask.shape[1] + 2), dtype=bool)
    p[1:-1, 1:-1] = mask
    return p[1:-1, 1:-1] & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def box_ring(h, w, window):
    """the drawn pixels (bool [h,w]) of the dashed ring of the pixel window [x1,y1,x2,y2): every window pixel within BOX_RING px of one of the
    window's edges, dashed along x in the top and bottom bands and along y elsewhere.  An empty window draws nothing."""
    x1, y1, x2, y2 = (int(v) for v in window)
    out = np.zeros((h, w), dtype=bool)
    if x2 <= x1 or y2 <= y1:
        return out
    y, x = np.mgrid[0:h, 0:w]
    inside = (x >= x1) & (x < x2) & (y >= y1) & (y < y2)
    band = (y - y1 < BOX_RING) | (y2 - 1 - y < BOX_RING)
    side = (x - x1 < BOX_RING) | (x2 - 1 - x < BOX_RING)
    dash = np.where(band, ((x - x1) // BOX_DASH) % 2 == 0, ((y - y1) // BOX_DASH) % 2 == 0)
    return inside & (band | side) & dash


def render_instances(image, windows, masks, colors, alpha=0.5, box_alpha=0.7, show_mask=True, show_outline=True, show_bbox=True):
    """image uint8 [h,w,3], windows int [n,4] = the [x1,y1,x2,y2) pixel window of every instance's paste, masks bool or 0/1 [h,w,n],
    colors float [n,3] in [0,1] -> the overlay, uint8 [h,w,3].  Three layers, each over all instances in slot order, each on top of the one
    before (as matplotlib stacks its patches over imshow): the masks blended in with alpha, the mask outlines in the instance's colour, the
    dashed box rings blended in with box_alpha."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("render_instances: image must be uint8 [h,w,3] (got %s %s)" % (image.dtype, tuple(image.shape)))
    h, w = image.shape[:2]
    masks = np.asarray(masks)
    n = int(masks.shape[2]) if masks.ndim == 3 else -1
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 4)
    colors = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    if n < 0 or tuple(masks.shape[:2]) != (h, w) or windows.shape[0] != n or colors.shape[0] != n:
        raise ValueError("render_instances: masks [h,w,n], windows [n,4] and colors [n,3] expected for an image of %d x %d" % (h, w))
    masks = masks != 0
    canvas = image.astype(np.uint32)
    if show_mask:
        for i in range(n):
            blend(canvas, masks[:, :, i], colors[i], alpha)
    if show_outline:
        for i in range(n):
            canvas[outline(masks[:, :, i])] = (colors[i] * 255).astype(np.uint32)
    if show_bbox:
        for i in range(n):
            blend(canvas, box_ring(h, w, windows[i]), colors[i], box_alpha)
    return canvas.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- PNG
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, rgb):
    """rgb uint8 [h,w,3] -> an 8-bit RGB PNG at path (every row with filter type 0, one IDAT chunk)"""
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("write_png: uint8 [h,w,3] expected (got %s %s)" % (rgb.dtype, tuple(rgb.shape)))
    h, w = rgb.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)               # a filter byte (0: none) in front of every row
    rows[:, 1:] = rgb.reshape(h, 3 * w)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))


def read_png(path):
    """the inverse of write_png, for the same restricted form: 8-bit RGB, not interlaced, filter type 0 on every row -> uint8 [h,w,3]"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError("read_png: %s is not a PNG file" % path)
    at, head, idat = 8, None, []
    while at + 8 <= len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if len(body) != n or struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(kind + body) & 0xffffffff):
            raise ValueError("read_png: %s: damaged %r chunk" % (path, kind))
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        at += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError("read_png: %s: only 8-bit RGB without interlacing is read" % path)
    w, h = head[0], head[1]
    rows = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if rows.size != h * (1 + 3 * w):
        raise ValueError("read_png: %s: %d bytes of pixel data for %d x %d" % (path, rows.size, h, w))
    rows = rows.reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError("read_png: %s: only rows of filter type 0 are read" % path)
    return rows[:, 1:].reshape(h, w, 3).copy()

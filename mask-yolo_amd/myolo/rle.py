"""COCO run-length masks on the host (numpy only): the form MaskYOLO.detect(..., mask_format="rle") returns and every COCO tool reads.

The format.  A mask m[h, w] of 0 / 1 is read in COLUMN-MAJOR order, p = x * h + y, N = h * w.  With v[-1] = 0 a boundary is
every p in [0, N) with v[p] != v[p-1], and counts = diff([0, boundaries..., N]): run lengths that alternate and start with the zeros, so counts[0]
is 0 exactly when pixel 0 is set and no other count is 0; an all-zero mask is [N]; sum(counts) = N and the area is sum(counts[1::2]).  An RLE is
{"size": [h, w], "counts": a 1-D integer array} -- or, compressed, the string of to_string(counts) in its place (pycocotools' rleToString).

The compressed string: the i-th count goes out as x = counts[i], less counts[i-2] when i > 2, in groups of five bits from the low end --
c = x & 0x1f, x >>= 5 (arithmetic), more follows unless the rest is the sign extension of bit 4 of c (x == 0 for a clear bit, x == -1 for a set one),
c |= 0x20 when more follows, chr(c + 48).  from_string reverses it."""
import numpy as np


def counts_from_boundaries(bounds, n_pixels):
    """the run lengths of a mask of n_pixels pixels whose boundaries (ascending positions, see above) are `bounds`"""
    b = np.asarray(bounds, dtype=np.int64).reshape(-1)
    edges = np.empty(b.size + 2, np.int64)
    edges[0], edges[-1] = 0, int(n_pixels)
    edges[1:-1] = b
    return np.diff(edges)


def encode(mask):
    """a 2-D mask (anything numpy reads as [h, w]; non-zero = set) -> {"size": [h, w], "counts": int64 array}"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("encode: a 2-D mask is expected (got shape %s)" % (tuple(m.shape),))
    h, w = int(m.shape[0]), int(m.shape[1])
    v = (m != 0).reshape(-1, order="F")
    prev = np.empty_like(v)
    prev[:1] = False
    prev[1:] = v[:-1]
    return {"size": [h, w], "counts": counts_from_boundaries(np.flatnonzero(v != prev), h * w)}


def _counts(rle):
    c = rle["counts"]
    if isinstance(c, (str, bytes)):
        return from_string(c)
    c = np.asarray(c)
    if c.ndim != 1 or (c.size and not np.issubdtype(c.dtype, np.integer)):
        raise ValueError("an RLE's counts are a 1-D integer array or a compressed string")
    return c.astype(np.int64)


def decode(rle):
    """{"size": [h, w], "counts": array or compressed string} -> the bool [h, w] mask"""
    h, w = int(rle["size"][0]), int(rle["size"][1])
    counts = _counts(rle)
    if (counts < 0).any() or int(counts.sum()) != h * w:
        raise ValueError("decode: the counts sum to %d, the size %s holds %d pixels" % (int(counts.sum()), [h, w], h * w))
    ones = (np.arange(counts.size) & 1).astype(bool)
    return np.repeat(ones, counts).reshape((h, w), order="F")


def area(rle):
    """the number of set pixels"""
    return int(_counts(rle)[1::2].sum())


def bbox(rle):
    """[x, y, w, h] of the set pixels (the smallest box that holds them; [0, 0, 0, 0] for an empty mask), from the runs alone"""
    h = int(rle["size"][0])
    counts = _counts(rle)
    end = np.cumsum(counts)
    start = end - counts
    on = (np.arange(counts.size) & 1).astype(bool) & (counts > 0)
    if not on.any():
        return [0, 0, 0, 0]
    first, last = start[on], end[on] - 1
    xa, xb = first // h, last // h
    ya, yb = first % h, last % h
    spans = xa != xb                                   # a run that goes on into the next column touches row h - 1 and row 0
    y0 = 0 if spans.any() else int(ya.min())
    y1 = h - 1 if spans.any() else int(yb.max())
    if spans.any() and (~spans).any():
        y0, y1 = min(y0, int(ya[~spans].min())), max(y1, int(yb[~spans].max()))
    x0, x1 = int(xa.min()), int(xb.max())
    return [x0, y0, x1 - x0 + 1, y1 - y0 + 1]


def to_string(counts):
    """run lengths -> the compressed string (pycocotools' rleToString)"""
    counts = [int(c) for c in np.asarray(counts).reshape(-1)]
    out = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def from_string(s):
    """the compressed string (str or bytes) -> int64 run lengths (pycocotools' rleFrString)"""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError("from_string: the string ends inside a count")
            c = ord(s[p]) - 48
            if not 0 <= c < 64:
                raise ValueError("from_string: %r is no character of a compressed RLE" % s[p])
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return np.array(counts, dtype=np.int64)


def coco_results(results, image_ids, category_ids=None):
    """detect() / detect_many() result dicts of either mask format -> the list of COCO result dicts
    {"image_id", "category_id", "segmentation": {"size": [h, w], "counts": <compressed string>}, "bbox": [x, y, w, h], "score"}, ready for json.dump.
    image_ids: one id per result dict.  category_ids (None: the class id itself): a mapping or sequence, class id -> COCO category id.  bbox is the
    detection's box (bboxes, [x1, y1, x2, y2] pixels of the masks' frame) as COCO writes it.
    Results of mask_format="polygon" (they carry "polygons") give COCO's polygon form instead: segmentation = the list of the instance's OUTER loops
    (myolo/contour.py; holes are dropped), each flat [x1, y1, x2, y2, ...] in corner coordinates, which are COCO's; bbox = the loops' own extent and
    "area" = the pixels they enclose."""
    results, image_ids = list(results), list(image_ids)
    if len(results) != len(image_ids):
        raise ValueError("coco_results: %d results but %d image ids" % (len(results), len(image_ids)))
    out = []
    for r, image_id in zip(results, image_ids):
        n = len(r["class_ids"])
        for i in range(n):
            if "polygons" in r:
                from .contour import outer_loops, signed_area
                loops = outer_loops(r["polygons"][i])
                cls = int(r["class_ids"][i])
                pts = np.concatenate(loops) if loops else np.zeros((1, 2), np.int32)
                x1, y1, x2, y2 = (float(t) for t in (pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()))
                out.append({
                    "image_id": image_id.item() if isinstance(image_id, np.generic) else image_id,
                    "category_id": cls if category_ids is None else int(category_ids[cls]),
                    "segmentation": [[int(v) for v in np.asarray(l).reshape(-1)] for l in loops],
                    "bbox": [x1, y1, x2 - x1, y2 - y1],
                    "area": float(sum(signed_area(l) for l in loops)),
                    "score": float(r["confidence_scores"][i]),
                })
                continue
            m = r["rle_masks"][i] if "rle_masks" in r else encode(np.asarray(r["full_masks"])[:, :, i])
            cls = int(r["class_ids"][i])
            x1, y1, x2, y2 = (float(t) for t in r["bboxes"][i])
            out.append({
                "image_id": image_id.item() if isinstance(image_id, np.generic) else image_id,
                "category_id": cls if category_ids is None else int(category_ids[cls]),
                "segmentation": {"size": [int(m["size"][0]), int(m["size"][1])], "counts": to_string(_counts(m))},
                "bbox": [x1, y1, x2 - x1, y2 - y1],
                "score": float(r["confidence_scores"][i]),
            })
    return out

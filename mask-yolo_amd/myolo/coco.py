"""
Datasets annotated in the COCO instance format (``instances_*.json``): the ground-truth side of the protocol whose detection side
myolo.rle.coco_results writes.  numpy, json and PIL only (no pycocotools).

COCODataset has VIADataset's duck-typed surface, so load_image_gt and the host routes of MaskYOLO.train() / evaluate() take it as it is.  It also
has load_segments, and that is what keeps the masks off the host: train() and evaluate() send the segments to the device and decode them there
(myolo_segment_masks).  It deliberately has NO load_polygons: train() routes on that attribute.

The contract.  An annotation's segmentation becomes one *segment*, in one of two forms:

* a list of parts, each a float64 [k,2] array of (row, col) vertices taken from COCO's flat [x0, y0, x1, y1, ...].  Every part is filled by THIS
  project's polygon rule (myolo.polygon, DESIGN.md section 13: scikit-image's), and the instance is the UNION of its parts (as COCO defines it) -- not
  even-odd over the concatenated outlines.  pycocotools fills a polygon with its own rule (frPoly: the outline upsampled by 5 and traced); the two
  can differ at boundary pixels, and nothing here pins that difference;
* a run-length code {"size": [h, w], "counts": int64 array} (iscrowd regions, datasets exported from masks): column-major runs that start with the
  zeros (myolo.rle).  Compressed string counts are expanded when the file is read.  A run-length code is exact by definition.

Classes: class id = position + 1 in the ascending list of the kept category ids (``category_ids=`` restricts and orders it); ds.category_ids is that
list with a leading 0 for the background, so that ``rle.coco_results(results, image_ids, category_ids=ds.category_ids)`` maps a class id back to its
COCO category.  The image size comes from the image record's height / width.
"""
import json
import os

import numpy as np

from . import rle as _rle
from .polygon import polygon_mask, polygon_mask_sampled


def is_rle(segment):
    return isinstance(segment, dict)


def rle_bounds(segment):
    """a run-length segment -> int64 boundaries: the running sums of its counts without the final total (ascending; equal ones where a run has
    length 0).  Pixel p = col * h + row is set when the number of boundaries <= p is odd -- what myolo_segment_masks is handed."""
    return np.cumsum(np.asarray(segment["counts"], np.int64))[:-1]


def segment_mask(segment, shape):
    """-> bool [h,w]: a segment at full resolution (the OR of polygon_mask over the parts; rle.decode of a run-length code)."""
    h, w = int(shape[0]), int(shape[1])
    if is_rle(segment):
        return _rle.decode(segment)
    m = np.zeros((h, w), bool)
    for p in segment:
        m |= polygon_mask(p[:, 0], p[:, 1], (h, w))
    return m


def segment_mask_sampled(segment, src_row, src_col):
    """-> bool [len(src_row), len(src_col)]: the segment evaluated ONLY at the source pixels (src_row[i], src_col[j]) -- the host restatement of
    myolo_segment_masks.  Parts: polygon_mask_sampled of each, OR-ed.  A run-length code: pixel (r, c) sits at p = c * h + r and is set when the
    number of i with counts[0] + ... + counts[i] <= p is odd (runs of length 0 anywhere change nothing)."""
    rows = np.asarray(src_row, np.int64).reshape(-1)
    cols = np.asarray(src_col, np.int64).reshape(-1)
    if is_rle(segment):
        h = int(segment["size"][0])
        p = cols[None, :] * h + rows[:, None]
        return (np.searchsorted(rle_bounds(segment), p, side="right") & 1).astype(bool)
    m = np.zeros((rows.shape[0], cols.shape[0]), bool)
    for part in segment:
        m |= polygon_mask_sampled(part[:, 0], part[:, 1], rows, cols)
    return m


class COCODataset(object):
    SOURCE = "coco"

    def __init__(self):
        self.image_info = []
        self.class_info = [{"source": "", "id": 0, "name": "BG"}]
        self.image_ids = []
        self.class_names = []
        self.source_class_ids = {}
        self.category_ids = [0]

    # ---- mrcnn.utils.Dataset surface (as myolo.via.VIADataset)
    def add_class(self, source, class_id, class_name):
        self.class_info.append({"source": source, "id": class_id, "name": class_name})

    def add_image(self, source, image_id, path, **kwargs):
        info = {"id": image_id, "source": source, "path": path}
        info.update(kwargs)
        self.image_info.append(info)

    def prepare(self):
        self.num_classes = len(self.class_info)
        self.class_ids = np.arange(self.num_classes)
        self.class_names = [c["name"] for c in self.class_info]
        self.num_images = len(self.image_info)
        self.image_ids = np.arange(self.num_images)
        self.source_class_ids = {self.SOURCE: list(range(self.num_classes)), "": [0]}

    def load_image(self, image_id):
        from PIL import Image
        with Image.open(self.image_info[image_id]["path"]) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    def load_segments(self, image_id):
        """-> (list of segments -- a list of float64 [k,2] (row, col) parts, or {"size": [h,w], "counts": int64 array} --, int32 [n] class ids)."""
        info = self.image_info[image_id]
        return info["segments"], info["segment_class_ids"]

    def load_mask(self, image_id):
        """-> (bool [h,w,n], int32 [n]): every segment at full resolution (segment_mask)."""
        info = self.image_info[image_id]
        segments, ids = self.load_segments(image_id)
        mask = np.zeros([info["height"], info["width"], len(segments)], dtype=bool)
        for i, s in enumerate(segments):
            mask[:, :, i] = segment_mask(s, (info["height"], info["width"]))
        return mask, ids.copy()

    def image_reference(self, image_id):
        return self.image_info[image_id]["path"]


def _segment(seg, ann_id, h, w, path):
    """an annotation's `segmentation` -> a segment (None when it is empty)"""
    where = "%s: annotation %r" % (path, ann_id)
    if not seg:
        return None
    if isinstance(seg, dict):
        size = [int(v) for v in seg.get("size", [])]
        if size != [h, w]:
            raise ValueError("%s has a run-length code of size %s, its image is %s" % (where, size, [h, w]))
        if h * w >= 1 << 31:
            raise ValueError("%s: a run-length code of %d x %d pixels is beyond 2^31" % (where, h, w))
        counts = seg.get("counts")
        try:
            counts = _rle.from_string(counts) if isinstance(counts, (str, bytes)) else np.asarray(counts)
            if counts.ndim != 1 or counts.size == 0 or not np.issubdtype(counts.dtype, np.integer):
                raise ValueError("counts are a non-empty list of integers or a compressed string")
            counts = counts.astype(np.int64)
            if (counts < 0).any() or int(counts.sum()) != h * w:
                raise ValueError("counts %s, which sum to %d for %d pixels" %
                                 ("hold a negative run" if (counts < 0).any() else "are all >= 0", int(counts.sum()), h * w))
        except ValueError as e:
            raise ValueError("%s: bad run-length code: %s" % (where, e))
        return {"size": [h, w], "counts": counts}
    parts = []
    for k, flat in enumerate(seg):
        try:
            a = np.asarray(flat, np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("%s: part %d is no list of numbers" % (where, k))
        if a.size % 2 or a.size < 2 or not np.isfinite(a).all():
            raise ValueError("%s: part %d has %d values; an even number (>= 2) of finite x, y is needed" % (where, k, a.size))
        parts.append(np.ascontiguousarray(a.reshape(-1, 2)[:, ::-1]))            # (x, y) -> (row, col)
    return parts


def load_coco(annotation_file, image_dir, category_ids=None, crowd="skip"):
    """-> a prepared COCODataset of the instance annotations in `annotation_file`, its images under `image_dir`.
    category_ids None: every category of the file, ascending; else the categories kept, in this order -- class id = position + 1, annotations of other
    categories are dropped.  crowd "skip": iscrowd == 1 annotations are dropped; "keep": they are ordinary instances.  Annotations with an empty
    segmentation, and images left without an annotation, are skipped (as load_via skips images without regions)."""
    if crowd not in ("skip", "keep"):
        raise ValueError("load_coco: crowd=%r; 'skip' or 'keep'" % (crowd,))
    with open(annotation_file) as f:
        data = json.load(f)
    cats = {int(c["id"]): c.get("name", str(c["id"])) for c in data.get("categories", [])}
    if category_ids is None:
        kept = sorted(cats)
    else:
        kept = [int(c) for c in category_ids]
        missing = [c for c in kept if c not in cats]
        if missing or len(set(kept)) != len(kept):
            raise ValueError("load_coco: category_ids %r: %s" % (list(category_ids), "not in the file: %r" % missing if missing else "repeated ids"))
    class_of = {c: k + 1 for k, c in enumerate(kept)}
    ds = COCODataset()
    ds.category_ids = [0] + kept
    for c in kept:
        ds.add_class(ds.SOURCE, class_of[c], cats[c])
    by_image = {}
    for a in data.get("annotations", []):
        by_image.setdefault(a["image_id"], []).append(a)
    for im in data.get("images", []):
        h, w = int(im["height"]), int(im["width"])
        segments, ids, ann_ids = [], [], []
        for a in by_image.get(im["id"], []):
            if int(a["category_id"]) not in class_of or (crowd == "skip" and int(a.get("iscrowd", 0)) == 1):
                continue
            s = _segment(a.get("segmentation"), a.get("id"), h, w, annotation_file)
            if s is None:
                continue
            segments.append(s)
            ids.append(class_of[int(a["category_id"])])
            ann_ids.append(a.get("id"))
        if not segments:
            continue
        ds.add_image(ds.SOURCE, image_id=im["id"], path=os.path.join(image_dir, im["file_name"]), width=w, height=h,
                     segments=segments, segment_class_ids=np.asarray(ids, np.int32), annotation_ids=ann_ids)
    ds.prepare()
    return ds

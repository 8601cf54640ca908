"""
Datasets annotated with the VGG Image Annotator (``via_*_annotation.json``): the working counterpart of the reference's rice / food example
datasets (example/rice/rice_dataset.py:89-167, RiceDataset.load_rice / load_mask), without scikit-image.

VIADataset has ShapesDataset's duck-typed surface, so load_image_gt, the host route of MaskYOLO.train() and evaluate() take it as it is:
load_mask fills every outline with myolo.polygon.polygon_mask (skimage.draw.polygon restated bit for bit).  It also has load_polygons, and
that is what lets train() keep the masks off the host altogether: the outlines go to the device and are rasterised there
as one-part segments (myolo_segment_masks, DESIGN.md sections 13 and 18).

Differences from the reference: the image size is read from the file header (PIL, no decode) where the reference decodes every image to
learn it; a region may be mapped to a class by one of its region attributes (the reference has one class); a region that is not a polygon
is an error rather than a KeyError in load_mask.
"""
import glob
import json
import os

import numpy as np

from .polygon import polygon_mask


class VIADataset(object):
    SOURCE = "via"

    def __init__(self):
        self.image_info = []
        self.class_info = [{"source": "", "id": 0, "name": "BG"}]
        self.image_ids = []
        self.class_names = []
        self.source_class_ids = {}

    # ---- mrcnn.utils.Dataset surface (as myolo.shapes.ShapesDataset)
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

    def load_polygons(self, image_id):
        """-> (list of float64 [k,2] (row, col) vertex arrays in source-image pixels, int32 [n] class ids)."""
        info = self.image_info[image_id]
        return info["polygons"], info["polygon_class_ids"]

    def load_mask(self, image_id):
        """-> (bool [h,w,n], int32 [n]): every outline filled as skimage.draw.polygon fills it, clipped to the image frame."""
        info = self.image_info[image_id]
        polygons, ids = self.load_polygons(image_id)
        mask = np.zeros([info["height"], info["width"], len(polygons)], dtype=bool)
        for i, p in enumerate(polygons):
            mask[:, :, i] = polygon_mask(p[:, 0], p[:, 1], (info["height"], info["width"]))
        return mask, ids.copy()

    def image_reference(self, image_id):
        return self.image_info[image_id]["path"]


def via_annotations(results, filenames, class_names=None, tolerance=0.0):
    """detect() / detect_many(mask_format="polygon") result dicts -> the VIA 2.x annotation dict, ready for json.dump and for load_via: one entry
    per image (filenames: one per result dict), one `polygon` region per OUTER loop of every instance -- VIA has no holes, so they are dropped; an
    instance of several pieces gives several regions.  all_points_x / all_points_y = X - 0.5, Y - 0.5: the pixel-centre convention load_via's
    fill reads, under which the outline of a hole-free piece fills to exactly its pixels.  region_attributes carries "class" (class_names[class
    id], a sequence indexed by class id as VIADataset.class_names is; None: the id as a string), "score" and "instance" (the position in
    class_ids).  tolerance > 0: every loop goes through contour.simplify first (in pixels)."""
    from .contour import outer_loops, simplify
    results, filenames = list(results), list(filenames)
    if len(results) != len(filenames):
        raise ValueError("via_annotations: %d results but %d filenames" % (len(results), len(filenames)))
    out = {}
    for r, name in zip(results, filenames):
        if "polygons" not in r:
            raise ValueError("via_annotations: results of mask_format='polygon' are expected (no 'polygons' in the result of %r)" % (name,))
        regions = []
        for i, loops in enumerate(r["polygons"]):
            cid = int(r["class_ids"][i])
            label = str(cid) if class_names is None else str(class_names[cid])
            for loop in outer_loops(loops):
                pts = np.asarray(simplify(loop, tolerance), np.float64) - 0.5
                regions.append({"shape_attributes": {"name": "polygon", "all_points_x": pts[:, 0].tolist(), "all_points_y": pts[:, 1].tolist()},
                                "region_attributes": {"class": label, "score": float(r["confidence_scores"][i]), "instance": i}})
        out["%s-1" % name] = {"filename": str(name), "size": -1, "regions": regions, "file_attributes": {}}
    return out


def load_via(dataset_dir, subset, annotation=None, class_attribute=None, class_names=None):
    """-> a prepared VIADataset of <dataset_dir>/<subset>/<annotation> (default: the one via_*.json there), VIA 1.x (`regions` a dict) or 2.x
    (a list); images without regions are skipped.
    class_attribute None: every region is class 1 (named class_names[0], or "object").  Otherwise region_attributes[class_attribute]
    is looked up in class_names (class id = position + 1)."""
    from PIL import Image
    ds = VIADataset()
    folder = os.path.join(dataset_dir, subset)
    if annotation is None:
        found = sorted(glob.glob(os.path.join(folder, "via_*.json")))
        if len(found) != 1:
            raise ValueError("load_via: expected one via_*.json in %s, found %d; name it with annotation=" % (folder, len(found)))
        path = found[0]
    else:
        path = os.path.join(folder, annotation)
    if class_attribute is not None and not class_names:
        raise ValueError("load_via: class_attribute=%r needs class_names" % (class_attribute,))
    names = list(class_names) if class_names else ["object"]
    if class_attribute is None:
        names = names[:1]
    for k, name in enumerate(names):
        ds.add_class(ds.SOURCE, k + 1, name)
    with open(path) as f:
        entries = list(json.load(f).values())
    for a in entries:
        regions = a.get("regions")
        if not regions:                          # VIA lists images that carry no annotation
            continue
        regions = list(regions.values()) if isinstance(regions, dict) else list(regions)
        polygons, ids = [], []
        for k, reg in enumerate(regions):
            sh = reg["shape_attributes"]
            if sh.get("name") != "polygon":
                raise ValueError("%s: region %d of %r has shape %r; only 'polygon' regions are handled" %
                                 (path, k, a.get("filename"), sh.get("name")))
            pts = np.stack([np.asarray(sh["all_points_y"], np.float64), np.asarray(sh["all_points_x"], np.float64)], axis=1)
            if pts.ndim != 2 or pts.shape[0] == 0 or not np.isfinite(pts).all():
                raise ValueError("%s: region %d of %r has no usable vertices" % (path, k, a.get("filename")))
            if class_attribute is None:
                cid = 1
            else:
                value = (reg.get("region_attributes") or {}).get(class_attribute)
                if value not in names:
                    raise ValueError("%s: region %d of %r has %s=%r, which is not one of class_names %r" %
                                     (path, k, a.get("filename"), class_attribute, value, names))
                cid = names.index(value) + 1
            polygons.append(pts)
            ids.append(cid)
        image_path = os.path.join(folder, a["filename"])
        with Image.open(image_path) as im:       # the header only: nothing is decoded
            width, height = im.size
        ds.add_image(ds.SOURCE, image_id=a["filename"], path=image_path, width=width, height=height,
                     polygons=polygons, polygon_class_ids=np.asarray(ids, np.int32))
    ds.prepare()
    return ds

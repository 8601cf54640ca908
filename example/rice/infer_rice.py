#!/usr/bin/env python
"""Run a trained Mask-YOLO over a folder of photographs on one MI355X -- the inference counterpart of train_rice.py.  The photographs go to
MaskYOLO.detect_many as they are, whatever their sizes: they are resized to the network frame on the device and the boxes and masks come back
in each photograph's own frame.  With --coco-json the masks are asked for as COCO run-length codes (encoded on the device,
DESIGN section 15: no dense mask is written or downloaded) and every detection goes into one COCO results file.  With --render-dir every
photograph's overlay -- masks, outlines and boxes drawn over it on the device -- is written there as <name>.png.  With
--via-json the masks are asked for as polygons (traced on the device) and written as a VIA 2.x annotation file: load it in the
VGG Image Annotator beside the photographs to correct the predictions, or read it back with myolo.via.load_via.  With --max-detections N up to
N instances (1 .. 128) are reported per photograph instead of ten, selected on the device; an overlay holds at most 16.
With --measure-csv every grain's measurements -- area, the area no other grain hides, length and width, orientation, perimeter, Euler number,
box and centroid, taken on the device -- are written as one CSV row per grain, in pixels or, with --units-per-pixel S,
in units (lengths times S, areas times S * S); it goes with every other output.

  python example/rice/infer_rice.py WEIGHTS.npz IMAGE_DIR [--size 224] [--batch 8] [--threshold 0.35] [--network-frame] [--coco-json PATH]
                                    [--render-dir DIR] [--via-json PATH] [--polygon-tolerance T] [--max-detections N]
                                    [--measure-csv PATH] [--units-per-pixel S]
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                   # noqa: E402
from myolo.config import RiceConfig, make_config     # noqa: E402
from myolo.model import MaskYOLO                     # noqa: E402
from myolo import measure, render, rle, via          # noqa: E402


def load_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("weights", help="weights saved by train_rice.py (mask_yolo_rice_final.npz)")
    ap.add_argument("images", help="directory of .jpg / .jpeg / .png photographs, of any sizes")
    ap.add_argument("--size", type=int, default=224, help="the network frame the weights were trained at")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=0.35)
    ap.add_argument("--network-frame", action="store_true", help="report boxes and masks in the network frame (cheap for large photographs)")
    ap.add_argument("--coco-json", metavar="PATH", help="write the detections as a COCO results file (image_id = the file's name without extension)")
    ap.add_argument("--render-dir", metavar="DIR", help="write every photograph's overlay (masks, outlines, boxes) as DIR/<name>.png")
    ap.add_argument("--via-json", metavar="PATH", help="write the detections as a VIA 2.x annotation file (one polygon region per outer outline)")
    ap.add_argument("--polygon-tolerance", metavar="T", type=float, default=0.0,
                    help="with --via-json: simplify every outline (Douglas-Peucker), dropping vertices within T pixels of it; 0 keeps every corner")
    ap.add_argument("--max-detections", metavar="N", type=int, default=None,
                    help="report up to N instances per photograph (1 .. 128), selected on the device; default: the ten of the host selection")
    ap.add_argument("--measure-csv", metavar="PATH", help="write one row of measurements per detected grain (myolo.measure.table)")
    ap.add_argument("--units-per-pixel", metavar="S", type=float, default=1.0,
                    help="with --measure-csv: the length of a pixel's side in the unit wanted (say mm); lengths are multiplied by S, areas by S * S")
    a = ap.parse_args()
    if a.max_detections is not None and not 1 <= a.max_detections <= 128:
        ap.error("--max-detections must be in 1 .. 128")
    if a.render_dir and a.max_detections is not None and a.max_detections > 16:
        ap.error("--render-dir draws at most 16 instances per photograph: it does not go with --max-detections above 16")
    if a.render_dir and a.network_frame:
        ap.error("--render-dir draws on the photograph given: it does not go with --network-frame")
    if a.via_json and a.network_frame:
        ap.error("--via-json outlines the photograph given: it does not go with --network-frame")
    if a.polygon_tolerance < 0:
        ap.error("--polygon-tolerance must be >= 0")
    if not a.units_per_pixel > 0:
        ap.error("--units-per-pixel must be > 0")
    mask_format = "polygon" if a.via_json else ("rle" if a.coco_json or a.render_dir else "dense")

    paths = sorted(p for ext in ("jpg", "jpeg", "png", "JPG", "JPEG", "PNG") for p in glob.glob(os.path.join(a.images, "*." + ext)))
    if not paths:
        raise SystemExit("no .jpg / .jpeg / .png file in %s" % a.images)
    config = make_config(RiceConfig, IMAGE_SHAPE=[a.size, a.size, 3], BATCH_SIZE=a.batch)
    model = MaskYOLO(mode="inference", config=config)
    model.load_weights(a.weights)
    total, coco, annotations, rows = 0, [], {}, []
    for lo in range(0, len(paths), 8 * a.batch):                  # a few batches at a time: the photographs of one call are held in memory
        chunk = paths[lo:lo + 8 * a.batch]
        photos = [load_rgb(p) for p in chunk]
        results = model.detect_many(photos, cs_threshold=a.threshold, mask_frame="network" if a.network_frame else "image",
                                    mask_format=mask_format, render=bool(a.render_dir), max_detections=a.max_detections,
                                    measure=bool(a.measure_csv))
        if a.measure_csv:
            rows += measure.table(results, names=[os.path.basename(p) for p in chunk], scale=a.units_per_pixel)
        if a.via_json:
            annotations.update(via.via_annotations(results, [os.path.basename(p) for p in chunk], class_names=["BG", "rice"],
                                                   tolerance=a.polygon_tolerance))
        if a.coco_json:
            coco += rle.coco_results(results, [os.path.splitext(os.path.basename(p))[0] for p in chunk])
        for p, r, photo in zip(chunk, results, photos):
            n = len(r["class_ids"])
            total += n
            if a.render_dir:
                os.makedirs(a.render_dir, exist_ok=True)
                render.write_png(os.path.join(a.render_dir, os.path.splitext(os.path.basename(p))[0] + ".png"), r["rendered"])
            if "full_masks" in r:
                fh, fw = r["full_masks"].shape[:2]
            elif "polygons" in r:
                fh, fw = photo.shape[:2]
            else:
                fh, fw = r["rle_masks"][0]["size"] if n else (0, 0)
            print("%s: %d (mask frame %d x %d%s)" % (os.path.basename(p), n, fh, fw, "".join(", %.2f" % s for s in r["confidence_scores"])))
    print("%d detections in %d images" % (total, len(paths)))
    if a.coco_json:
        with open(a.coco_json, "w") as f:
            json.dump(coco, f)
        print("wrote %s" % a.coco_json)
    if a.via_json:
        with open(a.via_json, "w") as f:
            json.dump(annotations, f)
        print("wrote %s" % a.via_json)
    if a.measure_csv:
        measure.write_csv(a.measure_csv, rows)
        print("wrote %s" % a.measure_csv)


if __name__ == "__main__":
    main()

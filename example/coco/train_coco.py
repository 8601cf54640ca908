#!/usr/bin/env python
"""Train and evaluate Mask-YOLO on a dataset in the COCO instance format (an instances_*.json and a folder of images) on one MI355X.  The
segmentations -- polygon parts and run-length codes -- are decoded on the device, for the training batches and for evaluate()'s ground truth
(DESIGN section 18): no mask is built on the host.  After training the validation set is scored (MaskYOLO.evaluate) and its detections are
written as a COCO results file, category ids mapped back through the dataset.

  python example/coco/train_coco.py TRAIN_JSON TRAIN_IMAGES [--val-json PATH --val-images DIR] [--categories 1,3,17] [--keep-crowd]
                                    [--epochs 30] [--size 224] [--batch 8] [--no-augment] [--host-masks] [--results PATH]
                                    [--fit-anchors K] [--mosaic P] [--copy-paste P] [--max-detections N]
                                    [--hue DEG] [--saturation F] [--contrast F] [--blur SIGMA] [--noise F]

--fit-anchors K fits K anchors to the training set's boxes first (myolo.anchors) and trains with them; without it the anchors are
Config's, which were fitted to UECFOOD100 at 224 x 224.  --max-detections N scores and writes up to N detections per validation image (1 .. 128,
selected on the device: DESIGN section 23) instead of ten -- on pictures with more than ten objects recall, and every AP, stops at 10 / n without it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "mask-yolo_amd")]
from myolo import rle                                # noqa: E402
from myolo.anchors import fit_anchors                # noqa: E402
from myolo.augment import Augmentation, CopyPaste, Mosaic, Photometric       # noqa: E402
from myolo.coco import load_coco                     # noqa: E402
from myolo.config import Config, make_config         # noqa: E402
from myolo.model import MaskYOLO                     # noqa: E402
from myolo.optim import Recipe, Schedule             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("train_json", help="COCO instance annotations of the training images")
    ap.add_argument("train_images", help="the directory their file_name entries are relative to")
    ap.add_argument("--val-json")
    ap.add_argument("--val-images")
    ap.add_argument("--categories", help="comma-separated COCO category ids to keep, in class order (default: all of the file, ascending)")
    ap.add_argument("--keep-crowd", action="store_true", help="keep iscrowd annotations as ordinary instances (default: skip them)")
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--logs", default="./logs")
    ap.add_argument("--no-augment", action="store_true")
    ap.add_argument("--mosaic", type=float, default=0.0, metavar="P", help="mosaic a training sample with probability P: four images of the batch "
                                                                            "per sample, on the device (default: 0, off)")
    ap.add_argument("--copy-paste", type=float, default=0.0, metavar="P", help="paste instances of another sample of the batch into a training "
                                                                                "sample with probability P, on the device (default: 0, off)")
    ap.add_argument("--hue", type=float, default=0.0, metavar="DEG", help="rotate a training sample's colours by up to DEG degrees either way, on "
                                                                         "the device (photometric augmentation, DESIGN section 26; default: 0, off)")
    ap.add_argument("--saturation", type=float, default=0.0, metavar="F", help="saturation gain in [1 - F, 1 + F] (default: 0, off)")
    ap.add_argument("--contrast", type=float, default=0.0, metavar="F", help="contrast gain about mid-grey in [1 - F, 1 + F] (default: 0, off)")
    ap.add_argument("--blur", type=float, default=0.0, metavar="SIGMA", help="Gaussian blur with a sigma in [0, SIGMA] pixels, at most 5 (default: 0, off)")
    ap.add_argument("--noise", type=float, default=0.0, metavar="F", help="additive noise with a deviation in [0, F] of full scale (default: 0, off)")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="C", help="scale the whole gradient down to Euclidean norm C when it is longer "
                    "(the reference config's GRADIENT_CLIP_NORM is 5.0; default: no clipping)")
    ap.add_argument("--weight-decay", type=float, default=0.0, metavar="W", help="decoupled (AdamW) weight decay on the convolution kernels "
                    "(the reference config's WEIGHT_DECAY is 0.0001; default: none)")
    ap.add_argument("--ema", type=float, default=None, metavar="D", help="keep an exponential moving average of the weights with decay D in (0, 1), "
                    "saved as saved_model_<stamp>_ema.npz beside every epoch's checkpoint (default: none)")
    ap.add_argument("--lr-schedule", choices=Schedule.KINDS, default=None, help="learning-rate schedule over the whole run (default: constant)")
    ap.add_argument("--warmup-steps", type=int, default=0, metavar="N", help="linear warm-up over the first N optimiser steps")
    ap.add_argument("--host-masks", action="store_true", help="decode the segmentations on the host (load_mask) for the training batches")
    ap.add_argument("--fit-anchors", type=int, default=0, metavar="K", help="fit K anchors to the training set first (default: Config's anchors)")
    ap.add_argument("--results", default=None, help="where the validation detections go as a COCO results file (default: LOGS/coco_results.json)")
    ap.add_argument("--max-detections", metavar="N", type=int, default=None,
                    help="evaluate and write up to N detections per validation image (1 .. 128), selected on the device (default: ten, on the host)")
    a = ap.parse_args()
    if a.max_detections is not None and not 1 <= a.max_detections <= 128:
        ap.error("--max-detections must be in 1 .. 128")

    cats = [int(c) for c in a.categories.split(",")] if a.categories else None
    crowd = "keep" if a.keep_crowd else "skip"
    train = load_coco(a.train_json, a.train_images, category_ids=cats, crowd=crowd)
    val = load_coco(a.val_json, a.val_images or a.train_images, category_ids=train.category_ids[1:], crowd=crowd) if a.val_json else None
    print("train: %d images, classes %s" % (len(train.image_ids), train.class_names))
    overrides = dict(IMAGE_SHAPE=[a.size, a.size, 3], BATCH_SIZE=a.batch, NUM_CLASSES=train.num_classes, LABELS=train.class_names)
    if a.fit_anchors:
        fitted = fit_anchors(train, make_config(Config, **overrides), a.fit_anchors)
        print("anchors fitted to the training set (mean IoU %.4f): %s" % (fitted.mean_iou[fitted.best], ["%.2f" % v for v in fitted.anchors]))
        overrides.update(fitted.overrides())
    config = make_config(Config, **overrides)
    augmentation = None if a.no_augment else Augmentation(fliplr=.5, scale=(.8, 1.2), translate=(-.1, .1), rotate=(-15, 15),
                                                          brightness=(.8, 1.2))
    model = MaskYOLO(mode="training", config=config, model_dir=a.logs, yolo_pretrain_dir=None, yolo_trainable=True)
    recipe = None                                   # any of the five flags: the optimiser pass with the recipe on the device
    if a.clip_norm is not None or a.weight_decay > 0 or a.ema is not None or a.lr_schedule is not None or a.warmup_steps > 0:
        recipe = Recipe(clip_norm=a.clip_norm, weight_decay=a.weight_decay, ema=a.ema,
                        schedule=Schedule(a.lr_schedule or "constant", warmup_steps=a.warmup_steps))
    photometric = None                              # any of the five flags: colour, blur and noise as the augmenter's last stage on the device
    if a.hue > 0 or a.saturation > 0 or a.contrast > 0 or a.blur > 0 or a.noise > 0:
        photometric = Photometric.around(hue=a.hue, saturation=a.saturation, contrast=a.contrast, blur=a.blur, noise=a.noise)
    hist = model.train(train, val, learning_rate=config.LEARNING_RATE, epochs=a.epochs, layers='all', augmentation=augmentation,
                       device_polygons=not a.host_masks, mosaic=Mosaic(p=a.mosaic) if a.mosaic > 0 else None,
                       copy_paste=CopyPaste(p=a.copy_paste) if a.copy_paste > 0 else None, recipe=recipe, photometric=photometric)
    print("epoch losses:", ["%.4f" % h for h in hist])
    print("batches decoded on the device: %d of %d" % (model.host_times["segment_batches"], model.host_times["steps"]))
    os.makedirs(a.logs, exist_ok=True)
    weights = os.path.join(a.logs, "mask_yolo_coco_final.npz")
    model.save_weights(weights)

    if val is not None:
        infer = MaskYOLO(mode="inference", config=config)
        infer.load_weights(weights)
        r = infer.evaluate(val, max_detections=a.max_detections)
        print("validation: mask AP50 %.4f, mask AP %.4f, box AP50 %.4f, box AP %.4f over %d images (%d instances, %d detections)" %
              (r["mask_ap50"], r["mask_ap"], r["box_ap50"], r["box_ap"], r["n_images"], r["n_gt"], r["n_det"]))
        out, ids = [], list(val.image_ids)
        for lo in range(0, len(ids), 8 * a.batch):                  # a few batches at a time: the photographs of one call are held in memory
            chunk = ids[lo:lo + 8 * a.batch]
            results = infer.detect_many([val.load_image(i) for i in chunk], mask_format="rle", max_detections=a.max_detections)
            out += rle.coco_results(results, [val.image_info[i]["id"] for i in chunk], category_ids=val.category_ids)
        path = a.results or os.path.join(a.logs, "coco_results.json")
        with open(path, "w") as f:
            json.dump(out, f)
        print("wrote %d detections to %s" % (len(out), path))


if __name__ == "__main__":
    main()

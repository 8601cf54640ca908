#!/usr/bin/env python
"""Train Mask-YOLO on a dataset annotated with the VGG Image Annotator on one MI355X -- the working counterpart of the reference's
example/rice/train_rice.py and rice_dataset.py (RiceConfig, a dataset of <dir>/train and <dir>/val, each with its images and one
via_*_annotation.json, MaskYOLO(mode="training"), model.train(...)).  The outlines are rasterised on the device: no mask
is built on the host.

  python example/rice/train_rice.py DATASET_DIR [--epochs 30] [--size 224] [--batch 8] [--no-augment] [--host-masks] [--fit-anchors K]
                                             [--mosaic P] [--copy-paste P]
                                             [--hue DEG] [--saturation F] [--contrast F] [--blur SIGMA] [--noise F]

--fit-anchors K fits K anchors to the training set's boxes first (myolo.anchors) and trains with them; without it the anchors are
RiceConfig's.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "mask-yolo_amd")]
from myolo.anchors import fit_anchors                # noqa: E402
from myolo.augment import Augmentation, CopyPaste, Mosaic, Photometric       # noqa: E402
from myolo.config import RiceConfig, make_config     # noqa: E402
from myolo.model import MaskYOLO                     # noqa: E402
from myolo.optim import Recipe, Schedule             # noqa: E402
from myolo.via import load_via                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dataset", help="directory with train/ and val/, each holding the images and one via_*_annotation.json")
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
    ap.add_argument("--host-masks", action="store_true", help="fill the outlines on the host (load_mask) instead of on the device")
    ap.add_argument("--fit-anchors", type=int, default=0, metavar="K", help="fit K anchors to the training set first (default: RiceConfig's anchors)")
    a = ap.parse_args()

    config = make_config(RiceConfig, IMAGE_SHAPE=[a.size, a.size, 3], BATCH_SIZE=a.batch)
    dataset_train = load_via(a.dataset, "train")
    if a.fit_anchors:
        fitted = fit_anchors(dataset_train, config, a.fit_anchors)
        print("anchors fitted to the training set (mean IoU %.4f): %s" % (fitted.mean_iou[fitted.best], ["%.2f" % v for v in fitted.anchors]))
        config = make_config(RiceConfig, IMAGE_SHAPE=[a.size, a.size, 3], BATCH_SIZE=a.batch, **fitted.overrides())
    dataset_val = load_via(a.dataset, "val") if os.path.isdir(os.path.join(a.dataset, "val")) else None
    print("train: %d images, classes %s" % (len(dataset_train.image_ids), dataset_train.class_names))
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
    hist = model.train(dataset_train, dataset_val, learning_rate=config.LEARNING_RATE, epochs=a.epochs, layers='all',
                       augmentation=augmentation, device_polygons=not a.host_masks,
                       mosaic=Mosaic(p=a.mosaic) if a.mosaic > 0 else None,
                       copy_paste=CopyPaste(p=a.copy_paste) if a.copy_paste > 0 else None, recipe=recipe, photometric=photometric)
    print("epoch losses:", ["%.4f" % h for h in hist])
    print("batches rasterised on the device: %d of %d" % (model.host_times["polygon_batches"], model.host_times["steps"]))
    os.makedirs(a.logs, exist_ok=True)
    model.save_weights(os.path.join(a.logs, "mask_yolo_rice_final.npz"))


if __name__ == "__main__":
    main()

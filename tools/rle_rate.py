#!/usr/bin/env python
"""Images per second of MaskYOLO.detect_many with its two mask formats, at one config (Rice 416 x 416, batch 4, bf16 mask head, random weights,
cs_threshold 0 so that every image carries its ten masks):
  dense  mask_format="dense": one paste launch and one download of the [h, w, n] bytes per IMAGE (the code path as it was before the run-length
         form existed: the baseline);
  rle    mask_format="rle": the masks encoded on the device (myolo_rle_masks), one launch set and two small downloads per BATCH.
Each is warmed up (graphs captured, staging rings pinned, clocks up) and then timed with a host clock around calls that end in a download, REPS
times alternating on the same images in the same process; the medians, the ratio rle / dense and the mask bytes each form brings down per image
(beside the detection rows both download) are printed as one JSON line (DESIGN.md section 15 and profiles/rle_notes.md record a run).
  python tools/rle_rate.py [N=images per call, default 256] [REPS=default 5]
"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo.config import make_config, RiceConfig               # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402

over = dict(a.split("=", 1) for a in sys.argv[1:])
N, REPS = int(over.get("N", 256)), int(over.get("REPS", 5))
assert torch.cuda.is_available(), "rle_rate needs a GPU: a rate measured anywhere else says nothing"
cfg = make_config(RiceConfig, BATCH_SIZE=4, INFERENCE_DTYPE="bf16")
m = MaskYOLO(mode="inference", config=cfg, seed=4)
rng = np.random.default_rng(3)
images = [(rng.random(tuple(cfg.IMAGE_SHAPE)) * 255).astype(np.uint8) for _ in range(N)]
B, K = int(cfg.BATCH_SIZE), m.EVAL_SLOTS


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


ways = {
    "dense": lambda: m.detect_many(images, cs_threshold=0.0),
    "rle": lambda: m.detect_many(images, cs_threshold=0.0, mask_format="rle"),
}
last = {}
for k, fn in ways.items():                                     # warm-up: every shape the timed window uses
    fn()
    last[k] = fn()
times = {k: [] for k in ways}
for _ in range(REPS):                                          # alternating, so that a drifting clock or a busy host meets both
    for k, fn in ways.items():
        times[k].append(timed(fn))
rate = {k: N / float(np.median(v)) for k, v in times.items()}
masks = sum(len(r["class_ids"]) for r in last["rle"])
assert masks == sum(r["full_masks"].shape[2] for r in last["dense"])
dense_bytes = sum(r["full_masks"].nbytes for r in last["dense"]) / N
# a mask of c counts has c - 1 boundaries of 4 bytes; every batch also brings its B * K + 1 offsets down
rle_bytes = (sum(4 * (len(x["counts"]) - 1) for r in last["rle"] for x in r["rle_masks"]) + 4 * (B * K + 1) * ((N + B - 1) // B)) / N
out = {"config": "Rice 416x416 batch 4 bf16 head, random weights, cs_threshold 0", "images_per_call": N, "reps": REPS,
       "masks_per_image": round(masks / N, 2),
       "images_per_sec": {k: round(v, 1) for k, v in rate.items()},
       "spread_images_per_sec": {k: [round(N / max(v), 1), round(N / min(v), 1)] for k, v in times.items()},
       "rle_over_dense": round(rate["rle"] / rate["dense"], 3),
       "mask_bytes_downloaded_per_image": {"dense": round(dense_bytes), "rle": round(rle_bytes)}}
print(json.dumps(out))

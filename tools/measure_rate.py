#!/usr/bin/env python
"""Images per second of MaskYOLO.detect_many with and without the per-instance measurements, at one config (Rice 416 x 416, batch 4, bf16 mask
head, random weights, cs_threshold 0 so that every image carries its ten masks):
  dense        mask_format="dense": one paste launch and one download of the [h, w, n] bytes per IMAGE, nothing measured (the download a host
               measurement needs, alone);
  dense_host   the same, then measure.properties(measure.measure_dense(full_masks)) on the host for every image: what a user did before
               measure=True existed (with numpy in regionprops' place);
  rle_measure  mask_format="rle", measure=True: masks encoded and measured on the device (myolo_rle_masks, myolo_measure_masks), per BATCH one
               launch set each and the small downloads (104 bytes per slot for the records); properties on the host, no pixel work there.
Each is warmed up (graphs captured, staging rings pinned, clocks up) and then timed with a host clock around calls that end in a download, REPS
times alternating on the same images in the same process; the medians, the ratios and the mask bytes each route brings down per image are
printed as one JSON line, after the records of the two measuring routes were compared integer for integer (DESIGN.md section 25 records a run).
  python tools/measure_rate.py [N=images per call, default 256] [REPS=default 5]
"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import measure                                      # noqa: E402
from myolo.config import make_config, RiceConfig               # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402

over = dict(a.split("=", 1) for a in sys.argv[1:])
N, REPS = int(over.get("N", 256)), int(over.get("REPS", 5))
assert torch.cuda.is_available(), "measure_rate needs a GPU: a rate measured anywhere else says nothing"
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


def dense_host():
    out = m.detect_many(images, cs_threshold=0.0)
    for r in out:
        r["measurements"] = measure.properties(measure.measure_dense(r["full_masks"]))
    return out


ways = {
    "dense": lambda: m.detect_many(images, cs_threshold=0.0),
    "dense_host": dense_host,
    "rle_measure": lambda: m.detect_many(images, cs_threshold=0.0, mask_format="rle", measure=True),
}
last = {}
for k, fn in ways.items():                                     # warm-up: every shape the timed window uses
    fn()
    last[k] = fn()
masks = sum(len(r["class_ids"]) for r in last["rle_measure"])
assert masks == sum(r["full_masks"].shape[2] for r in last["dense_host"])
for a, b in zip(last["dense_host"], last["rle_measure"]):       # faster and different is not faster
    assert np.array_equal(a["measurements"]["raw"], b["measurements"]["raw"])
times = {k: [] for k in ways}
for _ in range(REPS):                                          # alternating, so that a drifting clock or a busy host meets all three
    for k, fn in ways.items():
        times[k].append(timed(fn))
rate = {k: N / float(np.median(v)) for k, v in times.items()}
dense_bytes = sum(r["full_masks"].nbytes for r in last["dense"]) / N
# a mask of c counts has c - 1 boundaries of 4 bytes; every batch also brings its B * K + 1 offsets and its B * K records of 104 bytes down
batches = (N + B - 1) // B
device_bytes = (sum(4 * (len(x["counts"]) - 1) for r in last["rle_measure"] for x in r["rle_masks"])
                + (4 * (B * K + 1) + 8 * measure.WORDS * B * K) * batches) / N
out = {"config": "Rice 416x416 batch 4 bf16 head, random weights, cs_threshold 0", "images_per_call": N, "reps": REPS,
       "masks_per_image": round(masks / N, 2),
       "images_per_sec": {k: round(v, 1) for k, v in rate.items()},
       "spread_images_per_sec": {k: [round(N / max(v), 1), round(N / min(v), 1)] for k, v in times.items()},
       "rle_measure_over_dense_host": round(rate["rle_measure"] / rate["dense_host"], 3),
       "rle_measure_over_dense": round(rate["rle_measure"] / rate["dense"], 3),
       "mask_bytes_downloaded_per_image": {"dense": round(dense_bytes), "dense_host": round(dense_bytes), "rle_measure": round(device_bytes)}}
print(json.dumps(out))

#!/usr/bin/env python
"""Images per second of MaskYOLO.detect_many(mask_format="rle") with the selection made on the host and on the device, at one config (Rice
416 x 416, batch 4, bf16 mask head, random weights, cs_threshold 0 so that every slot a selection may fill is filled):
  none   max_detections=None: the [B,R,6] detections come down per batch and every image is selected on the host (argsort, NMB in Python) --
         the code path of the parent commit, the baseline;
  10     max_detections=10: myolo_select_detections, one launch and B * K * 7 words down per batch;
  40     max_detections=40: 16 + 16 + 8 slots through myolo_rle_masks;
  100    max_detections=100: seven column blocks.
Each is warmed up (graphs captured, staging rings pinned, clocks up) and then timed with a host clock around calls that end in a download, REPS
times alternating on the same images in the same process; the medians, the spread of the repetitions and the ratios to `none` are printed as one
JSON line (DESIGN.md section 23 records a run), with the number of images on which `10` reports exactly what `none` reports.
  python tools/select_rate.py [N=images per call, default 256] [REPS=default 5]
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
assert torch.cuda.is_available(), "select_rate needs a GPU: a rate measured anywhere else says nothing"
cfg = make_config(RiceConfig, BATCH_SIZE=4, INFERENCE_DTYPE="bf16")
m = MaskYOLO(mode="inference", config=cfg, seed=4)
rng = np.random.default_rng(3)
images = [(rng.random(tuple(cfg.IMAGE_SHAPE)) * 255).astype(np.uint8) for _ in range(N)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def way(k):
    return lambda: m.detect_many(images, cs_threshold=0.0, mask_format="rle", max_detections=k)


ways = {"none": way(None), "10": way(10), "40": way(40), "100": way(100)}
last = {}
for k, fn in ways.items():                                     # warm-up: every shape the timed window uses
    fn()
    last[k] = fn()


def same(a, b):
    return (all(np.array_equal(a[key], b[key]) for key in ("bboxes", "class_ids", "confidence_scores"))
            and [x["counts"].tolist() for x in a["rle_masks"]] == [x["counts"].tolist() for x in b["rle_masks"]])


# faster and different is not faster: the images on which `10` reports what `none` reports.  They differ only where candidates TIE in score: the
# device breaks ties by the higher row (a stable argsort reversed), the host's default argsort is not stable.  Random weights on noise give every
# row of an image the same score, so here that is most images; tests/test_gpu_max_detections.py holds the equality on inputs without ties.
equal_images = sum(same(a, b) for a, b in zip(last["none"], last["10"]))
tied_images = sum(len(np.unique(r["confidence_scores"])) < len(r["confidence_scores"]) for r in last["none"])
times = {k: [] for k in ways}
for _ in range(REPS):                                          # alternating, so that a drifting clock or a busy host meets all four
    for k, fn in ways.items():
        times[k].append(timed(fn))
rate = {k: N / float(np.median(v)) for k, v in times.items()}
out = {"config": "Rice 416x416 batch 4 bf16 head, random weights, cs_threshold 0, mask_format rle", "images_per_call": N, "reps": REPS,
       "images_where_10_equals_none": equal_images, "images_with_tied_scores": tied_images,
       "masks_per_image": {k: round(sum(len(r["class_ids"]) for r in v) / N, 2) for k, v in last.items()},
       "images_per_sec": {k: round(v, 1) for k, v in rate.items()},
       "spread_images_per_sec": {k: [round(N / max(v), 1), round(N / min(v), 1)] for k, v in times.items()},
       "over_none": {k: round(rate[k] / rate["none"], 3) for k in ("10", "40", "100")}}
print(json.dumps(out))

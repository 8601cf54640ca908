#!/usr/bin/env python
"""Images per second of scoring a model on a validation stream, two ways, at one config (Shapes 224 x 224, batch 4, bf16 mask head):
  evaluate     MaskYOLO.evaluate_shapes_stream: inputs and ground truth produced on the device, overlaps counted on the device
               (myolo_mask_overlap_counts), K x T integers per image come down;
  detect_many  what had to be done before: MaskYOLO.detect_many on the same images (host uint8 in, pasted H x W x n masks out) followed by a
               numpy IoU loop against the ground-truth masks.  detect_many alone is reported too.
Each is warmed up (graphs captured, staging rings pinned, clocks up) and then timed with a host clock around calls that end in a download,
REPS times alternating; the medians and the ratio evaluate / detect_many are printed as one JSON line (DESIGN.md section 11 records a run).
  python tools/eval_rate.py [N=images per call, default 256] [REPS=default 5]
"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo.config import make_config, ShapesConfig             # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402
from myolo.shapes import make_shapes_samples                   # noqa: E402

over = dict(a.split("=", 1) for a in sys.argv[1:])
N, REPS = int(over.get("N", 256)), int(over.get("REPS", 5))
assert torch.cuda.is_available(), "eval_rate needs a GPU: a rate measured anywhere else says nothing"
cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], BATCH_SIZE=4, INFERENCE_DTYPE="bf16")
m = MaskYOLO(mode="inference", config=cfg, seed=4)
samples = make_shapes_samples(N, cfg, seed=0)                  # the images evaluate_shapes_stream(N, seed=0) produces on the device
images = [s[0] for s in samples]


def numpy_iou_loop(results):
    """every pasted mask against every ground-truth mask of its image, as tools/overfit_check.py used to do it"""
    best = []
    for (_, _, _, gt), res in zip(samples, results):
        for j in range(res["full_masks"].shape[2]):
            pm = res["full_masks"][:, :, j]
            best.append(max([np.logical_and(pm, gt[:, :, g]).sum() / max(1, np.logical_or(pm, gt[:, :, g]).sum()) for g in range(gt.shape[2])] or [0.0]))
    return best


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


ways = {
    "evaluate_shapes_stream": lambda: m.evaluate_shapes_stream(N, seed=0, cs_threshold=0.0),
    "detect_many": lambda: m.detect_many(images, cs_threshold=0.0),
    "detect_many_plus_numpy_iou": lambda: numpy_iou_loop(m.detect_many(images, cs_threshold=0.0)),
}
for fn in ways.values():                                       # warm-up: every shape the timed window uses
    fn()
    fn()
times = {k: [] for k in ways}
for _ in range(REPS):                                          # alternating, so that a drifting clock or a busy host meets all three
    for k, fn in ways.items():
        times[k].append(timed(fn))
rate = {k: N / float(np.median(v)) for k, v in times.items()}
out = {"config": "Shapes 224x224 batch 4 bf16 head, random weights, cs_threshold 0", "images_per_call": N, "reps": REPS,
       "images_per_sec": {k: round(v, 1) for k, v in rate.items()},
       "spread_images_per_sec": {k: [round(N / max(v), 1), round(N / min(v), 1)] for k, v in times.items()},
       "evaluate_over_detect_many": round(rate["evaluate_shapes_stream"] / rate["detect_many"], 3),
       "evaluate_over_detect_many_plus_numpy_iou": round(rate["evaluate_shapes_stream"] / rate["detect_many_plus_numpy_iou"], 3)}
print(json.dumps(out))

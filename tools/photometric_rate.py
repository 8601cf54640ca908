#!/usr/bin/env python
"""What the photometric stage costs on one MI355X (profiles/augment_notes.md records a run), one JSON line:
  kernel   device microseconds per call of myolo_photometric_batch on a resident batch of random floats -- Shapes 224 x 224, batch 32, and Rice
           416 x 416, batch 4 -- with max_radius 0 (colour and noise only), 6 and 15 (every row blurs at that radius): HIP events around LAUNCHES
           back-to-back calls, the cases alternating REPS times in this one process; the median and the extremes of each; the bytes the stage has to
           move (12 read and 12 written per pixel, whatever the radius), the time they would take at HBM_TBS TB/s, and measured over that.
           The batch is called on again and again and fits the Infinity Cache: these are warm-cache times, the case train() meets (the stage
           before has just written the input), set against an HBM rate;
  train    MaskYOLO.train() images/s on a ShapesDataset of N images, timed between the on_epoch_end callbacks of epochs 2..E as bench.py's
           train_api does, `augmentation` without and with `photometric`, alternating RUNS times in this one process -- at 224 x 224 / batch 32,
           and at the Rice geometry (416 x 416, batch 4, five anchors) on N416 Shapes images; and the launch thread's host milliseconds per step.
  python tools/photometric_rate.py [KERNEL=1] [TRAIN=1] [PHOTO=1] [N=512] [N416=64] [EPOCHS=4] [RUNS=3] [LAUNCHES=100] [REPS=7] [HBM_TBS=5.2]
PHOTO=0 times `augmentation` alone and imports nothing this stage added: the form that runs on a commit without it.
"""
import json
import os
import sys
import time

over = dict(a.split("=", 1) for a in sys.argv[1:])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import _ext as X                                    # noqa: E402
from myolo.augment import Augmentation                         # noqa: E402
from myolo.config import make_config, RiceConfig, ShapesConfig  # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402
from myolo.shapes import ShapesDataset                         # noqa: E402

PHOTO = int(over.get("PHOTO", 1))
KERNEL, TRAIN = int(over.get("KERNEL", 1)) and PHOTO, int(over.get("TRAIN", 1))
N, N416, EPOCHS, RUNS = int(over.get("N", 512)), int(over.get("N416", 64)), int(over.get("EPOCHS", 4)), int(over.get("RUNS", 3))
LAUNCHES, REPS = int(over.get("LAUNCHES", 100)), int(over.get("REPS", 7))
HBM_TBS = float(over.get("HBM_TBS", 5.2))                      # the plain-copy rate profiles/r6_notes.md records: 5.2-5.5 TB/s
assert torch.cuda.is_available(), "photometric_rate needs a GPU: a rate measured anywhere else says nothing"
FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))
WIDE = dict(hue=(-20, 20), saturation=(.6, 1.4), contrast=(.7, 1.3), blur=(0., 2.), noise=(0., .05))
SHAPES = {"shapes224_b32": (32, 224, 224), "rice416_b4": (4, 416, 416)}
res = {}


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


if KERNEL:
    from myolo.augment import Photometric
    dev = torch.device("cuda:0")
    res["kernel"] = {}
    for name, (B, H, W) in SHAPES.items():
        src = torch.rand(B, H, W, 3, device=dev)
        out = torch.empty_like(src)
        ws = torch.empty(max(X.photometric_ws_bytes(B, H, W, 15), 8), dtype=torch.uint8, device=dev)
        calls = {}
        for radius in (0, 6, 15):
            rows = np.empty((B, 32))
            for b in range(B):
                rows[b] = Photometric.identity()
                rows[b, 0:12] = Photometric.matrix(10.0 + b, 1.2, 0.9).reshape(-1)
                rows[b, 12], rows[b, 13] = 0.03, 1000 + b
                rows[b, 14], rows[b, 16:32] = Photometric.kernel(radius / 3.0)
            assert (rows[:, 14] == radius).all()
            drows = torch.from_numpy(rows).to(dev)

            def call(drows=drows, radius=radius):
                X.call("myolo_photometric_batch", X.ptr(src), X.ptr(drows), X.ptr(out), radius, B, H, W, ws.data_ptr(), ws.numel(), X.stream())
            calls["max_radius_%d" % radius] = call

        def timed(fn):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return 1e3 * e0.elapsed_time(e1) / LAUNCHES
        us = {k: [] for k in calls}
        for fn in calls.values():
            timed(fn)                                           # warm-up: code objects, caches
        for _ in range(REPS):
            for k, fn in calls.items():
                us[k].append(timed(fn))
        nbytes = B * H * W * 24
        bound = nbytes / (HBM_TBS * 1e12) * 1e6
        res["kernel"][name] = {"algorithmic_bytes": nbytes, "us_at_hbm_rate": bound, "us_per_call": {k: spread(v) for k, v in us.items()},
                               "measured_over_bound": {k: float(np.median(v)) / bound for k, v in us.items()}}
        print("kernel %s: %r (bound %.1f us)" % (name, {k: round(float(np.median(v)), 1) for k, v in us.items()}, bound), file=sys.stderr, flush=True)

if TRAIN:
    names = ["augmentation"] + (["augmentation+photometric"] if PHOTO else [])
    res["train"] = {}
    for shape, (B, H, W) in SHAPES.items():
        n = N if H == 224 else N416
        cfg = make_config(ShapesConfig, IMAGE_SHAPE=[H, W, 3], BATCH_SIZE=B) if H == 224 else \
            make_config(ShapesConfig, IMAGE_SHAPE=[H, W, 3], BATCH_SIZE=B, N_BOX=RiceConfig.N_BOX, ANCHORS=RiceConfig.ANCHORS)
        try:
            ds = ShapesDataset(1234)
            ds.load_shapes(n, H, W)
            ds.prepare()
            rates = {k: [] for k in names}
            waits, launches = {k: [] for k in names}, {k: [] for k in names}
            for r in range(RUNS):
                for name in names:
                    model = MaskYOLO(mode="training", config=cfg)
                    stamps = []

                    def cb(ep, logs):
                        torch.cuda.synchronize()
                        stamps.append(time.perf_counter())
                    kw = {"augmentation": Augmentation(seed=r, **FULL)}
                    if name.endswith("photometric"):
                        from myolo.augment import Photometric
                        kw["photometric"] = Photometric(seed=r, **WIDE)
                    model.train(ds, None, 1e-4, epochs=EPOCHS, layers="all", verbose=0, custom_callbacks=[cb], **kw)
                    steps = (n + B - 1) // B
                    rates[name].append(B * steps * (len(stamps) - 1) / (stamps[-1] - stamps[0]))
                    ht = model.host_times
                    waits[name].append(1e3 * ht["wait_for_batch_s"] / max(1, ht["steps"]))
                    launches[name].append(1e3 * ht["launch_step_s"] / max(1, ht["steps"]))
                    print("train %s run %d, %s: %.1f img/s" % (shape, r, name, rates[name][-1]), file=sys.stderr, flush=True)
                    del model
            res["train"][shape] = {"images": n, "img_per_s": {k: spread(v) for k, v in rates.items()},
                                   "wait_for_batch_ms_per_step": {k: spread(v) for k, v in waits.items()},
                                   "launch_step_ms_per_step": {k: spread(v) for k, v in launches.items()}}
        except Exception as e:                                  # (recorded with what was measured before it; nothing more is started on the device)
            res["train"][shape] = {"error": "%s: %s" % (type(e).__name__, e)}
            print("train %s failed: %r" % (shape, e), file=sys.stderr, flush=True)
            break
print(json.dumps(res))

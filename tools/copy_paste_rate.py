#!/usr/bin/env python
"""What copy-paste costs on one MI355X (profiles/copy_paste_notes.md records a run), one JSON line:
  kernel   device microseconds per call of myolo_copy_paste_batch -- with select all zero and with planned tables -- and of myolo_augment_batch,
           whose outputs it reads, on the same resident batch (224 x 224, batch 32, Shapes, T slots, drawn rows): HIP events around LAUNCHES
           back-to-back calls, the entries alternating REPS times in this one process; the median and the extremes of each; and the bytes the
           second stage has to move (computed from the shapes and the plan), with the time they would take at COPY_TBS TB/s;
  train    MaskYOLO.train() images/s on a ShapesDataset of N images at 224 x 224 / batch 32, timed between the on_epoch_end callbacks of epochs
           2..E as bench.py's train_api does, `augmentation` + `mosaic` without and with `copy_paste`, alternating RUNS times in this one process;
           and the launch thread's host milliseconds per step: waiting for the prefetched batch, and launching the step.
  python tools/copy_paste_rate.py [KERNEL=1] [TRAIN=1] [N=512] [EPOCHS=4] [RUNS=3] [LAUNCHES=100] [REPS=7] [COPY_TBS=5.2]
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
from myolo.augment import Augmentation, CopyPaste, DeviceAugmenter, Mosaic  # noqa: E402
from myolo.config import make_config, ShapesConfig             # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402
from myolo.shapes import ShapesDataset, make_shapes_samples    # noqa: E402

KERNEL, TRAIN = int(over.get("KERNEL", 1)), int(over.get("TRAIN", 1))
N, EPOCHS, RUNS = int(over.get("N", 512)), int(over.get("EPOCHS", 4)), int(over.get("RUNS", 3))
LAUNCHES, REPS = int(over.get("LAUNCHES", 100)), int(over.get("REPS", 7))
COPY_TBS = float(over.get("COPY_TBS", 5.2))                    # the plain-copy rate profiles/r6_notes.md records: 5.2-5.5 TB/s
assert torch.cuda.is_available(), "copy_paste_rate needs a GPU: a rate measured anywhere else says nothing"
FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))
cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], BATCH_SIZE=32)
B, H, W, T = cfg.BATCH_SIZE, 224, 224, cfg.TRUE_BOX_BUFFER
res = {"T": T}


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def algorithmic_bytes(ids, donor, select):
    """what the second stage cannot avoid moving: render reads an image's floats and its live own mask bytes, the accepted donor mask bytes of a
    receiver, and writes floats and T mask bytes per pixel; stats reads the live own and the accepted donor mask bytes once more.  Mask bytes are
    counted in the units the kernels load: T bytes per pixel and side that has anything to read."""
    px = H * W
    render = stats = 0
    for b in range(B):
        own = int((ids[b] != 0).any())
        room = T - int((ids[b] != 0).sum())
        sel = [t for t in range(T) if (int(select[b]) >> t) & 1 and ids[donor[b]][t] != 0][:room]
        sides = own + int(bool(sel))
        render += px * (12 + 12 + T + sides * T)
        stats += px * sides * T
    return {"render": render, "stats": stats}


if KERNEL:
    samples = make_shapes_samples(B, cfg)
    images = np.stack([s[0] for s in samples])
    masks, ids = np.zeros((B, H, W, T), np.uint8), np.zeros((B, T), np.int32)
    for b, s in enumerate(samples):
        ids[b, :len(s[1])] = s[1]
        masks[b, :, :, :len(s[1])] = s[3]
    dev = torch.device("cuda:0")
    aug = DeviceAugmenter(cfg, dev)
    rows = np.stack([Augmentation(**FULL).params(0, i, H, W) for i in range(B)])
    src = [torch.from_numpy(a).to(dev) for a in (images, masks, ids, rows)]
    donor, select = CopyPaste(p=1.0).plan(0, list(range(B)), T)
    out = aug.apply(*src, copy_paste=(donor, select))            # the outputs every timed call writes again, and the first stage's (its inputs)
    mid = out["_paste_src"]
    first_ids = mid[3].cpu().numpy()
    res["instances_per_batch"] = {"first_stage": int((first_ids != 0).sum()), "pasted": int((out["gt_ids"] != 0).sum()),
                                  "paste_dropped": int(out["paste_dropped"].sum())}
    res["algorithmic_bytes"] = {"planned": algorithmic_bytes(first_ids, donor, select),
                                "zero_select": algorithmic_bytes(first_ids, donor, np.zeros(B, np.int32))}
    for v in res["algorithmic_bytes"].values():
        v["us_at_copy_rate"] = (v["render"] + v["stats"]) / (COPY_TBS * 1e12) * 1e6
    outs = [X.ptr(out[k]) for k in ("images", "gt_masks", "gt_boxes", "gt_ids", "y_true", "true_boxes")]
    G, A, C = cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES
    ws = torch.empty(max(X.copy_paste_ws_bytes(B, T), X.augment_ws_bytes(B, T)), dtype=torch.uint8, device=dev)
    first = [torch.empty_like(t) for t in mid[:4]]               # the timed first stage writes its own buffers: the second stage's inputs stay put
    zero = torch.zeros(B, dtype=torch.int32, device=dev)

    def augment():
        X.call("myolo_augment_batch", X.ptr(src[0]), X.ptr(src[1]), X.ptr(src[2]), X.ptr(src[3]), 0.0, X.ptr(aug.anchors), X.ptr(first[0]),
               X.ptr(first[1]), X.ptr(first[2]), X.ptr(first[3]), outs[4], outs[5], B, H, W, T, G, A, C, ws.data_ptr(), ws.numel(), X.stream())

    def paste_with(sel):
        def call():
            X.call("myolo_copy_paste_batch", X.ptr(mid[0]), X.ptr(mid[1]), X.ptr(mid[3]), X.ptr(mid[4]), X.ptr(sel), X.ptr(aug.anchors), *outs,
                   X.ptr(out["paste_dropped"]), B, H, W, T, G, A, C, ws.data_ptr(), ws.numel(), X.stream())
        return call

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / LAUNCHES
    calls = {"augment_batch": augment, "copy_paste_batch": paste_with(mid[5]), "copy_paste_batch_zero_select": paste_with(zero)}
    us = {k: [] for k in calls}
    for fn in calls.values():
        timed(fn)                                               # warm-up: code objects, caches
    for _ in range(REPS):
        for k, fn in calls.items():
            us[k].append(timed(fn))
    res["kernel_us_per_call"] = {k: spread(v) for k, v in us.items()}
    res["measured_over_bound"] = {"planned": res["kernel_us_per_call"]["copy_paste_batch"]["median"] / res["algorithmic_bytes"]["planned"]["us_at_copy_rate"],
                                  "zero_select": res["kernel_us_per_call"]["copy_paste_batch_zero_select"]["median"] /
                                  res["algorithmic_bytes"]["zero_select"]["us_at_copy_rate"]}
    print("kernel: %r" % {k: round(v["median"], 1) for k, v in res["kernel_us_per_call"].items()}, file=sys.stderr, flush=True)

if TRAIN:
    ds = ShapesDataset(1234)
    ds.load_shapes(N, H, W)
    ds.prepare()
    rates = {"augmentation+mosaic": [], "augmentation+mosaic+copy_paste": []}
    waits, launches = {k: [] for k in rates}, {k: [] for k in rates}
    for r in range(RUNS):
        for name in rates:
            model = MaskYOLO(mode="training", config=cfg)
            stamps = []

            def cb(ep, logs):
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
            kw = {"augmentation": Augmentation(seed=r, **FULL), "mosaic": Mosaic(seed=r)}
            if name.endswith("copy_paste"):
                kw["copy_paste"] = CopyPaste(seed=r)
            model.train(ds, None, 1e-4, epochs=EPOCHS, layers="all", verbose=0, custom_callbacks=[cb], **kw)
            steps = (N + B - 1) // B
            rates[name].append(B * steps * (len(stamps) - 1) / (stamps[-1] - stamps[0]))
            ht = model.host_times
            waits[name].append(1e3 * ht["wait_for_batch_s"] / max(1, ht["steps"]))
            launches[name].append(1e3 * ht["launch_step_s"] / max(1, ht["steps"]))
            print("train run %d, %s: %.1f img/s" % (r, name, rates[name][-1]), file=sys.stderr, flush=True)
            del model
    res["train_img_per_s"] = {k: spread(v) for k, v in rates.items()}
    res["wait_for_batch_ms_per_step"] = {k: spread(v) for k, v in waits.items()}
    res["launch_step_ms_per_step"] = {k: spread(v) for k, v in launches.items()}
print(json.dumps(res))

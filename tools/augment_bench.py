#!/usr/bin/env python
"""What the on-device augmentation costs (profiles/augment_notes.md records a run), one JSON line:
  kernel   microseconds per myolo_augment_batch at 224 x 224 / batch 32 / T 10 (identity rows and drawn rows; HIP events around LAUNCHES
           back-to-back calls on resident inputs, and around the same calls replayed as a captured graph), its algorithmic bytes over that time -- source bytes and masks read once, the float image,
           the masks and the small target arrays written once -- and that rate as a fraction of the copy bandwidth bench.py --full reports
           (_ext.measure_hbm_copy_gbs, "float4", measured here in the same process);
  train    MaskYOLO.train() images/sec on a ShapesDataset of N images at 224 x 224 / batch 32, timed between the on_epoch_end callbacks of
           epochs 2..E as bench.py's train_api does, RUNS times, with a full Augmentation (AUG=1) or without (AUG=0).
AUG=0 with KERNEL=0 touches nothing this feature added, so the same file measures the parent commit: ROOT=<its built checkout>.
  python tools/augment_bench.py [AUG=1] [KERNEL=1] [N=512] [EPOCHS=4] [RUNS=3] [LAUNCHES=200] [ROOT=checkout]
"""
import json
import os
import sys
import time

over = dict(a.split("=", 1) for a in sys.argv[1:])
ROOT = os.path.abspath(over.get("ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import _ext as X                                    # noqa: E402
from myolo.config import make_config, ShapesConfig             # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402
from myolo.shapes import ShapesDataset, make_shapes_samples    # noqa: E402

AUG, KERNEL = int(over.get("AUG", 1)), int(over.get("KERNEL", 1))
N, EPOCHS, RUNS, LAUNCHES = int(over.get("N", 512)), int(over.get("EPOCHS", 4)), int(over.get("RUNS", 3)), int(over.get("LAUNCHES", 200))
assert torch.cuda.is_available(), "augment_bench needs a GPU: a rate measured anywhere else says nothing"
FULL = dict(fliplr=.5, scale=(.7, 1.3), translate=(-.3, .3), rotate=(-30, 30), brightness=(.8, 1.2), offset=(-.1, .1))
cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], BATCH_SIZE=32)
B, H, W, T = cfg.BATCH_SIZE, 224, 224, cfg.TRUE_BOX_BUFFER
res = {"root": os.path.relpath(ROOT), "augmentation": bool(AUG)}

if KERNEL:
    from myolo.augment import Augmentation, DeviceAugmenter, IDENTITY_ROW
    samples = make_shapes_samples(B, cfg)
    images = np.stack([s[0] for s in samples])
    masks, ids = np.zeros((B, H, W, T), np.uint8), np.zeros((B, T), np.int32)
    for b, s in enumerate(samples):
        ids[b, :len(s[1])] = s[1]
        masks[b, :, :, :len(s[1])] = s[3]
    dev = torch.device("cuda:0")
    aug = DeviceAugmenter(cfg, dev)
    src = [torch.from_numpy(a).to(dev) for a in (images, masks, ids)]
    G, A, C = cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES
    alg_bytes = B * H * W * (3 + T) + B * H * W * (12 + T) + B * T * 4 * 6 + B * G * G * A * (5 + C) * 4
    res["kernel"] = {"algorithmic_bytes": alg_bytes}
    for name, rows in (("identity", np.tile(IDENTITY_ROW, (B, 1))),
                       ("drawn", np.stack([Augmentation(**FULL).params(0, i, H, W) for i in range(B)]))):
        p = torch.from_numpy(rows).to(dev)
        out = aug.apply(src[0], src[1], src[2], p)                 # the outputs every timed call below writes again

        def call():
            X.call("myolo_augment_batch", X.ptr(src[0]), X.ptr(src[1]), X.ptr(src[2]), X.ptr(p), 0.0, X.ptr(aug.anchors), X.ptr(out["images"]),
                   X.ptr(out["gt_masks"]), X.ptr(out["gt_boxes"]), X.ptr(out["gt_ids"]), X.ptr(out["y_true"]), X.ptr(out["true_boxes"]),
                   B, H, W, T, G, A, C, aug._ws.data_ptr(), aug._ws.numel(), X.stream())

        def timed(fn, n):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        timed(call, 20)
        # five memsets and three launches per call: issued one by one the host's enqueue rate can be the limit, so the same calls are also
        # timed as one captured graph of 20 (the device's own time)
        us_host = 1e3 * timed(call, LAUNCHES) / LAUNCHES
        entry = {"us_per_call_enqueued": us_host}
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                call()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    for _ in range(20):
                        call()
            torch.cuda.current_stream().wait_stream(side)
            timed(g.replay, 3)
            entry["us_per_call_graph"] = 1e3 * timed(g.replay, max(1, LAUNCHES // 20)) / (20 * max(1, LAUNCHES // 20))
        except Exception as e:
            entry["us_per_call_graph"] = None
            entry["graph_error"] = "%s: %s" % (type(e).__name__, e)
        us = entry["us_per_call_graph"] or us_host
        entry["us_per_call"] = us
        entry["algorithmic_gbs"] = alg_bytes / us / 1e3
        res["kernel"][name] = entry
    copy = X.measure_hbm_copy_gbs(device="cuda:0")
    res["kernel"]["hbm_copy_float4_gbs"] = copy["float4"]
    for name in ("identity", "drawn"):
        res["kernel"][name]["fraction_of_copy"] = res["kernel"][name]["algorithmic_gbs"] / copy["float4"]

ds = ShapesDataset(1234)
ds.load_shapes(N, H, W)
ds.prepare()
rates = []
for r in range(RUNS):
    model = MaskYOLO(mode="training", config=cfg)
    stamps = []

    def cb(ep, logs):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    kw = {}
    if AUG:
        from myolo.augment import Augmentation
        kw["augmentation"] = Augmentation(seed=r, **FULL)
    model.train(ds, None, 1e-4, epochs=EPOCHS, layers="all", verbose=0, custom_callbacks=[cb], **kw)
    steps = (N + B - 1) // B
    rates.append(B * steps * (len(stamps) - 1) / (stamps[-1] - stamps[0]))
    ht = model.host_times
    res.setdefault("wait_for_batch_ms_per_step", []).append(1e3 * ht["wait_for_batch_s"] / max(1, ht["steps"]))
    del model
res["train_img_per_s"] = rates
print(json.dumps(res))

#!/usr/bin/env python
"""Time the ResNet-50 training step (Net.train_step: forward, both losses, backward, Adam) with HIP events: warm-up, then --steps steps.
Prints img/s, the step time and, per step, the compute stream's time inside the trunk forward, the trunk backward (stages 3-2, the max-pool
and conv1, after the YOLO branch's backward has joined) and the mask head (forward + backward).  Shapes scenes, class ids remapped into 1..80
at 81 classes (BASELINE configs[4]'s data).  The default batch, 6 images of 512^2, is the largest the engine accepts at 512^2
(engine.RESNET_MAX_MASK_ROIS); configs[4]'s 16 is refused until its launches have been audited.
  python tools/resnet50_step.py [--batch 6] [--size 512] [--classes 81] [--steps 20] [--warmup 5] [--fp32-matmul bf16x6|native]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

from myolo.config import make_config, ShapesConfig     # noqa: E402
from myolo.model import MaskYOLO                        # noqa: E402
from myolo.shapes import make_shapes_samples            # noqa: E402
from myolo.myolo_utils import BatchGenerator            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--classes", type=int, default=81)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fp32-matmul", default="bf16x6")
    a = ap.parse_args()
    nc = a.classes
    cfg = make_config(ShapesConfig, BACKBONE="resnet50", IMAGE_SHAPE=[a.size, a.size, 3], BATCH_SIZE=a.batch, NUM_CLASSES=nc,
                      LABELS=["background"] + ["class%d" % i for i in range(1, nc)], FP32_MATMUL=a.fp32_matmul)
    samples = make_shapes_samples(a.batch, cfg, start_index=0)
    if nc > 4:
        remap = {1: 17 % nc or 1, 2: 45 % nc or 2, 3: nc - 1}
        for s in samples:
            s[1] = np.asarray([remap[int(c)] for c in s[1]], dtype=np.asarray(s[1]).dtype)
    batch, _ = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0]
    net = MaskYOLO(mode="training", config=cfg).net

    spans = {"trunk_fwd": [], "trunk_bwd": [], "mask_head": []}

    def timed(name, tag):
        fn = getattr(net, name)

        def wrap(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args, **kw)
            e1.record()
            spans[tag].append((e0, e1))
            return r
        setattr(net, name, wrap)
    timed("trunk_fwd", "trunk_fwd")
    timed("trunk_bwd", "trunk_bwd")
    for name in ("mask_head_fwd", "mask_head_fwd_positives", "mask_head_bwd", "mask_head_bwd_sparse"):
        timed(name, "mask_head")

    for _ in range(a.warmup):
        net.train_step(net.to_device_batch(batch), 1e-4)
    torch.cuda.synchronize()
    for v in spans.values():
        del v[:]
    dbs = [net.to_device_batch(batch) for _ in range(a.steps)]
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for db in dbs:
        net.train_step(db, 1e-4)
    s1.record()
    torch.cuda.synchronize()
    ms = s0.elapsed_time(s1) / a.steps
    per = {k: sum(e0.elapsed_time(e1) for e0, e1 in v) / a.steps for k, v in spans.items()}
    print("resnet50 train_step: batch %d x %d^2, %d classes, FP32_MATMUL=%s, %d steps after %d warm-up" % (a.batch, a.size, nc, a.fp32_matmul,
                                                                                                       a.steps, a.warmup))
    print("  %.1f img/s   %.2f ms/step" % (a.batch * 1000.0 / ms, ms))
    print("  trunk forward %.2f ms   trunk backward %.2f ms   mask head (fwd + bwd) %.2f ms   (compute stream, per step)" %
          (per["trunk_fwd"], per["trunk_bwd"], per["mask_head"]))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What the on-device polygon rasteriser costs and saves (profiles/polygon_notes.md records a run), one JSON line:
  kernel   microseconds per myolo_segment_masks at 224 x 224 / batch 32 / T 10 on the food outlines of tests/golden/via as single-part segments
           with boxes = NULL, as Net.stage_segments calls it (cycled to fill the batch, each image sampled from its own frame), HIP events
           around LAUNCHES back-to-back calls; the 16 MB it writes over that time as a
           fraction of the copy bandwidth (_ext.measure_hbm_copy_gbs, "float4", same process); and the time of the H2D copy of those 16 MB of
           masks from pinned memory, which is what the host-mask route pays instead;
  train    per step of MaskYOLO.train() over the same VIADataset (N images written as PNGs into a temporary directory), device_polygons True
           against False, RUNS runs of EPOCHS epochs each, alternating: wait_for_batch_s and launch_step_s of every epoch after a run's first
           (the per-epoch values, their median and range),
           images/sec between the epoch-end callbacks; bytes staged per step (from the staging specs) and host bytes held by the sample lists.
  python tools/polygon_bench.py [KERNEL=1] [TRAIN=1] [N=128] [EPOCHS=4] [RUNS=2] [LAUNCHES=200]
"""
import json
import os
import shutil
import sys
import tempfile
import time

over = dict(a.split("=", 1) for a in sys.argv[1:])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import _ext as X                                    # noqa: E402
from myolo import myolo_utils as mutils                        # noqa: E402
from myolo.config import make_config, ShapesConfig             # noqa: E402
from myolo.engine import Net                                   # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402
from myolo.via import load_via                                 # noqa: E402

KERNEL, TRAIN = int(over.get("KERNEL", 1)), int(over.get("TRAIN", 1))
N, EPOCHS, LAUNCHES, RUNS = int(over.get("N", 128)), int(over.get("EPOCHS", 4)), int(over.get("LAUNCHES", 200)), int(over.get("RUNS", 2))
assert torch.cuda.is_available(), "polygon_bench needs a GPU: a rate measured anywhere else says nothing"
cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], BATCH_SIZE=32)
B, H, W, T = cfg.BATCH_SIZE, 224, 224, cfg.TRUE_BOX_BUFFER
VIA = os.path.join(ROOT, "tests", "golden", "via", "food")
res = {}


def food_images():
    """-> [(h, w, [outline [k,2] (row, col), ...]), ...]: the annotated images of food/train and food/val; the JSON carries no image size, so
    the frame is the one the test fixture uses: (max y + 7, max x + 5) over the image's regions"""
    out = []
    for subset in ("train", "val"):
        d = json.load(open(os.path.join(VIA, subset, "via_food_annotation.json")))
        for a in d.values():
            regs = list(a["regions"].values()) if isinstance(a["regions"], dict) else a["regions"]
            if not regs:
                continue
            sh = [g["shape_attributes"] for g in regs]
            polys = [np.stack([np.asarray(s["all_points_y"], np.float64), np.asarray(s["all_points_x"], np.float64)], 1) for s in sh]
            out.append((int(max(p[:, 0].max() for p in polys)) + 7, int(max(p[:, 1].max() for p in polys)) + 5, polys, a))
    return out


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


imgs = food_images()
if KERNEL:
    dev = torch.device("cuda:0")
    group = []
    for b in range(B):
        h, w, polys, _ = imgs[b % len(imgs)]
        r, c = mutils.mask_index_tables(h, w, [H / h, W / w])
        group.append(([[p] for p in polys[:T]], (r.astype(np.int32), c.astype(np.int32)), h))
    n_verts, n_outlines, _ = mutils.segment_sizes([g[0] for g in group])
    d = [torch.from_numpy(a).to(dev) for a in mutils.segment_tables(group, B, T, H, W)]
    masks = torch.empty((B, H, W, T), dtype=torch.uint8, device=dev)

    def call():
        Net.segment_masks(d, masks)
    timed(call, 20)
    us = sorted(1e3 * timed(call, LAUNCHES) / LAUNCHES for _ in range(5))
    pinned = torch.empty((B, H, W, T), dtype=torch.uint8, pin_memory=True)
    pinned.copy_(masks)
    timed(lambda: masks.copy_(pinned, non_blocking=True), 5)
    h2d = sorted(1e3 * timed(lambda: masks.copy_(pinned, non_blocking=True), 20) / 20 for _ in range(5))
    copy = X.measure_hbm_copy_gbs(device="cuda:0")
    nbytes = B * H * W * T
    res["kernel"] = {"outlines": n_outlines, "vertices": n_verts, "set_fraction": float(masks.float().mean().item()),
                     "us_per_launch_runs": us, "us_per_launch": us[2], "bytes_written": nbytes,
                     "write_gbs": nbytes / us[2] / 1e3, "hbm_copy_float4_gbs": copy["float4"],
                     "fraction_of_copy": nbytes / us[2] / 1e3 / copy["float4"],
                     "h2d_us_of_the_same_bytes_runs": h2d, "h2d_us_of_the_same_bytes": h2d[2], "h2d_gbs": nbytes / h2d[2] / 1e3}

if TRAIN:
    from PIL import Image
    tmp = tempfile.mkdtemp(prefix="polygon_bench_")
    try:
        folder = os.path.join(tmp, "train")
        os.makedirs(folder)
        ann = {}
        yy, xx = np.mgrid[0:1024, 0:1024]
        for i in range(N):
            h, w, polys, a = imgs[i % len(imgs)]
            a = json.loads(json.dumps(a))
            a["filename"] = "img_%04d.png" % i
            img = np.stack([(yy[:h, :w] + 3 * i) % 256, (xx[:h, :w] * 2) % 256, (yy[:h, :w] + xx[:h, :w]) % 256], -1).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(folder, a["filename"]), compress_level=1)
            ann[a["filename"]] = a
        json.dump(ann, open(os.path.join(folder, "via_food_annotation.json"), "w"))
        ds = load_via(tmp, "train")

        def held(v):
            if isinstance(v, (list, tuple)):
                return sum(held(a) for a in v)
            return v.nbytes if isinstance(v, np.ndarray) else 0
        probe = MaskYOLO(mode="training", config=cfg)
        t0 = time.perf_counter()
        host_info = [list(mutils.load_image_gt(ds, cfg, i)) for i in ds.image_ids]
        t1 = time.perf_counter()
        poly_info = probe._collect_segments(ds, load="load_polygons")
        t2 = time.perf_counter()
        G, A, C = cfg.GRID_W, cfg.N_BOX, cfg.NUM_CLASSES

        def cap(need, least):                                                           # Net.stage_segments' staging shapes
            while least < need:
                least *= 2
            return least
        nv, npart, nb = mutils.segment_sizes([inst[2][:T] for inst in poly_info[:B]])
        res["train"] = {
            "images": N, "steps_per_epoch": (N + B - 1) // B,
            "collect_seconds": {"host_masks": t1 - t0, "polygons": t2 - t1},
            "host_bytes_held": {"host_masks": held(host_info), "polygons": held(poly_info), "of_which_images_on_either": N * H * W * 3},
            "bytes_staged_per_step": {
                "host_masks": B * H * W * 3 + B * T * 4 * 4 + B * G * G * A * (5 + C) * 4 + B * T * 4 + B * T * 4 * 4 + B * H * W * T,
                "host_masks_augmented": B * H * W * 3 + B * H * W * T + B * T * 4 + B * 8 * 8,
                "polygons": B * H * W * 3 + cap(nv, 1024) * 16 + (cap(npart, 64) + 1) * 4 + 2 * (B * T + 1) * 4 + (cap(nb, 1024) * 4 if nb else 0) + B * 4 +
                B * T * 4 + B * H * 4 + B * W * 4 + B * 8 * 8}}
        del probe, host_info, poly_info
        for name, flag in (("polygons", True), ("host_masks", False)) * RUNS:           # alternating: other work shares the host
            model = MaskYOLO(mode="training", config=cfg)
            snaps = []

            def cb(ep, logs):
                torch.cuda.synchronize()
                snaps.append((time.perf_counter(), dict(model.host_times)))
            model.train(ds, None, 1e-4, epochs=EPOCHS, layers="all", verbose=0, custom_callbacks=[cb], device_polygons=flag)
            wait, launch, ips = [], [], []
            for (ta, a), (tb, b) in zip(snaps[:-1], snaps[1:]):                     # every epoch after the first
                n = b["steps"] - a["steps"]
                wait.append(1e3 * (b["wait_for_batch_s"] - a["wait_for_batch_s"]) / n)
                launch.append(1e3 * (b["launch_step_s"] - a["launch_step_s"]) / n)
                ips.append(B * n / (tb - ta))
            e = res["train"].setdefault(name, {"polygon_batches": 0, "steps": 0, "wait_for_batch_ms_per_step": [],
                                                "launch_step_ms_per_step": [], "img_per_s": []})
            e["polygon_batches"] += model.host_times["polygon_batches"]
            e["steps"] += model.host_times["steps"]
            e["wait_for_batch_ms_per_step"] += wait
            e["launch_step_ms_per_step"] += launch
            e["img_per_s"] += ips
            del model
        for name in ("polygons", "host_masks"):
            e = res["train"][name]
            e["median"] = {k: float(np.median(e[k])) for k in ("wait_for_batch_ms_per_step", "launch_step_ms_per_step", "img_per_s")}
            e["range"] = {k: [float(np.min(e[k])), float(np.max(e[k]))] for k in ("wait_for_batch_ms_per_step", "launch_step_ms_per_step", "img_per_s")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(res))

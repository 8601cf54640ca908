#!/usr/bin/env python
"""Images per second of MaskYOLO.detect_many with and without the overlay, at one config (Rice 416 x 416, batch 4, bf16 mask head, random weights,
cs_threshold 0 so that every image carries its ten masks):
  dense        mask_format="dense": one paste launch and one download of the [h, w, n] bytes per IMAGE;
  dense+host   the same, then render.render_instances of every result on the host: what an overlay cost before the device renderer existed;
  rle          mask_format="rle": the counterpart of the next line without the overlay;
  rle+render   render=True, mask_format="rle": the overlay drawn on the device (myolo_render_instances), one launch set and one download of
               h * w * 3 bytes per image per BATCH, no dense mask anywhere.
Each is warmed up (graphs captured, staging rings pinned, clocks up) and then timed with a host clock around calls that end in a download, REPS
times alternating on the same images in the same process.  Then the renderer's own launches (the all-high flags and the overlay kernel) on one
batch of B images with ten live slots each, timed with device events over LAUNCHES back-to-back calls, beside a plain device copy of the same
bytes timed the same way in the same run.  One JSON line (DESIGN.md section 16 and profiles/render_notes.md record a run).
  python tools/render_rate.py [N=images per call, default 256] [REPS=default 5] [LAUNCHES=default 200]
"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import _ext as X                                    # noqa: E402
from myolo import render                                       # noqa: E402
from myolo.config import make_config, RiceConfig               # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402

over = dict(a.split("=", 1) for a in sys.argv[1:])
N, REPS, LAUNCHES = int(over.get("N", 256)), int(over.get("REPS", 5)), int(over.get("LAUNCHES", 200))
assert torch.cuda.is_available(), "render_rate needs a GPU: a rate measured anywhere else says nothing"
cfg = make_config(RiceConfig, BATCH_SIZE=4, INFERENCE_DTYPE="bf16")
m = MaskYOLO(mode="inference", config=cfg, seed=4)
rng = np.random.default_rng(3)
images = [(rng.random(tuple(cfg.IMAGE_SHAPE)) * 255).astype(np.uint8) for _ in range(N)]
B, K = int(cfg.BATCH_SIZE), m.EVAL_SLOTS
H, W = int(cfg.IMAGE_SHAPE[0]), int(cfg.IMAGE_SHAPE[1])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def windows(r):
    return [[min(max(0, int(b[0])), W), min(max(0, int(b[1])), H), min(max(1, int(b[2])), W), min(max(1, int(b[3])), H)] for b in r["bboxes"]]


def dense_then_host():
    out = m.detect_many(images, cs_threshold=0.0)
    for im, r in zip(images, out):
        n = len(r["class_ids"])
        r["rendered"] = render.render_instances(im, windows(r), r["full_masks"], render.instance_colors(n) if n else np.zeros((0, 3)))
    return out


ways = {
    "dense": lambda: m.detect_many(images, cs_threshold=0.0),
    "dense+host": dense_then_host,
    "rle": lambda: m.detect_many(images, cs_threshold=0.0, mask_format="rle"),
    "rle+render": lambda: m.detect_many(images, cs_threshold=0.0, mask_format="rle", render=True),
}
last = {}
for k, fn in ways.items():                                     # warm-up: every shape the timed window uses
    fn()
    last[k] = fn()
same = all(np.array_equal(a["rendered"], b["rendered"]) for a, b in zip(last["dense+host"], last["rle+render"]))
times = {k: [] for k in ways}
for _ in range(REPS):                                          # alternating, so that a drifting clock or a busy host meets all of them
    for k, fn in ways.items():
        times[k].append(timed(fn))
rate = {k: N / float(np.median(v)) for k, v in times.items()}

# the renderer's launches alone, on the detections of the first batch, beside a copy of the same bytes
dev = m.net.dev
x = torch.as_tensor(np.stack(images[:B]), device=dev)
_, det_d, mask_d = m.net.predict(x.float() / 255.0)
det_d, mask_d = det_d.contiguous(), mask_d.contiguous()
det_h = det_d.cpu().numpy()
sel = np.full((B, K), -1, np.int32)
for b in range(B):
    keep, nmb = m._select(det_h[b], 0.0)[:2]
    sel[b, :len(nmb)] = keep[nmb]
desc = np.array([[b * H * W * 3, H, W] for b in range(B)], np.int64)
col = np.zeros((B, K, 3))
col[:] = np.asarray(render.instance_colors(K))
sel_d, desc_d, col_d = (torch.as_tensor(a, device=dev) for a in (sel, desc, col))
out_d, ws = torch.empty_like(x), torch.empty(B * K, dtype=torch.int32, device=dev)
R, (mh, mw, C) = int(det_d.shape[1]), (int(v) for v in mask_d.shape[2:])


def launch_render():
    X.call("myolo_render_instances", X.ptr(x), X.ptr(out_d), x.numel(), X.ptr(desc_d), desc.ctypes.data, X.ptr(mask_d), X.ptr(det_d), X.ptr(sel_d),
           sel.ctypes.data, X.ptr(col_d), 0.5, 0.7, 7, B, R, K, mh, mw, C, ws.data_ptr(), ws.numel() * 4, X.stream())


def events_ms(fn):
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / LAUNCHES


pairs = [(events_ms(launch_render), events_ms(lambda: out_d.copy_(x))) for _ in range(3)]      # alternating
render_ms, copy_ms = (float(np.median([p[i] for p in pairs])) for i in (0, 1))
out = {"config": "Rice 416x416 batch 4 bf16 head, random weights, cs_threshold 0", "images_per_call": N, "reps": REPS,
       "masks_per_image": round(sum(len(r["class_ids"]) for r in last["rle+render"]) / N, 2),
       "device_overlay_equals_host_overlay": bool(same),
       "images_per_sec": {k: round(v, 1) for k, v in rate.items()},
       "spread_images_per_sec": {k: [round(N / max(v), 1), round(N / min(v), 1)] for k, v in times.items()},
       "render_over_dense_host": round(rate["rle+render"] / rate["dense+host"], 3),
       "render_over_rle": round(rate["rle+render"] / rate["rle"], 3),
       "renderer_batch": {"images": B, "live_slots": int((sel >= 0).sum()), "bytes": int(x.numel()), "launches_timed": LAUNCHES,
                          "render_us": round(render_ms * 1e3, 2), "plain_copy_us": round(copy_ms * 1e3, 2),
                          "render_over_copy": round(render_ms / copy_ms, 2)}}
print(json.dumps(out))

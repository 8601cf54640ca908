#!/usr/bin/env python
"""Images per second of MaskYOLO.detect_many with its three mask formats, at one config (Rice 416 x 416, batch 4, bf16 mask head, random weights,
cs_threshold 0 so that every image carries its ten masks):
  dense    mask_format="dense": one paste launch and one download of the [h, w, n] bytes per IMAGE;
  rle      mask_format="rle": the masks encoded on the device (myolo_rle_masks), one launch set and two small downloads per BATCH;
  polygon  mask_format="polygon": the masks traced on the device (myolo_contour_masks), one launch set and three small downloads per BATCH.
Each is warmed up (graphs captured, staging rings pinned, buffers grown, clocks up) and then timed with a host clock around calls that end in a
download, REPS times alternating on the same images in the same process.  Printed as one JSON line: the medians with their spread, the ratios to
"rle", the mask bytes each form brings down per image (beside the detection rows all three download) and the time a batch spends in
detect.batch_results -- everything behind the detection download: the consumer's launches, its downloads and the host's share (the split into
loops, the counts from the boundaries, the bool planes).  Random weights paste filled windows, so the two device entries are also timed by
themselves on crafted masks (entry_times below), at 416 x 416 and at 3000 x 4000.  DESIGN.md section 21 and profiles/contour_notes.md record a run.
  python tools/contour_rate.py [N=images per call, default 256] [REPS=default 5]
"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import detect as D                                  # noqa: E402
from myolo.config import make_config, RiceConfig               # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402

over = dict(a.split("=", 1) for a in sys.argv[1:])
N, REPS = int(over.get("N", 256)), int(over.get("REPS", 5))
assert torch.cuda.is_available(), "contour_rate needs a GPU: a rate measured anywhere else says nothing"
cfg = make_config(RiceConfig, BATCH_SIZE=4, INFERENCE_DTYPE="bf16")
m = MaskYOLO(mode="inference", config=cfg, seed=4)
rng = np.random.default_rng(3)
images = [(rng.random(tuple(cfg.IMAGE_SHAPE)) * 255).astype(np.uint8) for _ in range(N)]
B, K = int(cfg.BATCH_SIZE), D.SLOTS

post = []                                                      # seconds of every detect.batch_results call of the run in progress
_batch_results = D.batch_results


def _timed_batch_results(*a, **kw):
    t0 = time.perf_counter()
    out = _batch_results(*a, **kw)
    post.append(time.perf_counter() - t0)
    return out


D.batch_results = _timed_batch_results


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


ways = {
    "dense": lambda: m.detect_many(images, cs_threshold=0.0),
    "rle": lambda: m.detect_many(images, cs_threshold=0.0, mask_format="rle"),
    "polygon": lambda: m.detect_many(images, cs_threshold=0.0, mask_format="polygon"),
}
last = {}
for k, fn in ways.items():                                     # warm-up: every shape the timed window uses
    fn()
    last[k] = fn()
times = {k: [] for k in ways}
post_ms = {k: [] for k in ways}
for _ in range(REPS):                                          # alternating, so that a drifting clock or a busy host meets all three
    for k, fn in ways.items():
        del post[:]
        times[k].append(timed(fn))
        post_ms[k].append(1e3 * float(np.median(post)))
rate = {k: N / float(np.median(v)) for k, v in times.items()}
masks = sum(len(r["class_ids"]) for r in last["rle"])
assert masks == sum(r["full_masks"].shape[2] for r in last["dense"]) == sum(len(r["polygons"]) for r in last["polygon"])
batches = (N + B - 1) // B
dense_bytes = sum(r["full_masks"].nbytes for r in last["dense"]) / N
# a mask of c counts has c - 1 boundaries of 4 bytes, a vertex is 8 bytes and 4 of loop ordinal; every batch also brings its B * K + 1 offsets down
rle_bytes = (sum(4 * (len(x["counts"]) - 1) for r in last["rle"] for x in r["rle_masks"]) + 4 * (B * K + 1) * batches) / N
vertices = sum(len(l) for r in last["polygon"] for loops in r["polygons"] for l in loops)
polygon_bytes = (12 * vertices + 4 * (B * K + 1) * batches) / N


def entry_times(frame, kind, calls=20):
    """Random weights paste filled windows (four vertices a mask), which says nothing about ragged outlines: the two entries by themselves, HIP
    events round one call, on B x K crafted 28 x 28 masks in full-frame windows -- "window" all-high, "disc" a disc with a hole, "noise" thresholded
    noise (the most vertices a 28 x 28 mask gives, every stretch one mask cell long).  -> (us rle, us polygon, vertices per mask)"""
    from myolo import _ext as X
    g = np.random.default_rng(5)
    yy, xx = np.mgrid[0:28, 0:28]
    rr = (yy - 13.5) ** 2 + (xx - 13.5) ** 2
    plane = {"window": np.ones((28, 28)), "disc": (rr <= 144) & (rr >= 25), "noise": g.random((28, 28)) < 0.5}[kind].astype(np.float32)
    masks = torch.as_tensor(np.broadcast_to(plane[None, None, :, :, None], (B, K, 28, 28, 1)).copy(), device="cuda")
    det = torch.as_tensor(np.tile(np.array([0, 0, 1, 1, 0.9, 0], np.float32), (B, K, 1)), device="cuda")
    sel_h = np.tile(np.arange(K, dtype=np.int32), (B, 1))
    frames_h = np.tile(np.array(frame, np.int32), (B, 1))
    sel_d, frames_d = torch.as_tensor(sel_h, device="cuda"), torch.as_tensor(frames_h, device="cuda")
    cap = 1 << 22
    off = torch.empty(B * K + 1, dtype=torch.int32, device="cuda")
    buf = torch.empty(3 * cap, dtype=torch.int32, device="cuda")
    ws_r = torch.empty(X.rle_masks_ws_bytes(B, K, frame[1]) // 8 + 1, dtype=torch.int64, device="cuda")
    ws_c = torch.empty(X.contour_masks_ws_bytes(B, K, frame[0], frame[1], cap) // 8 + 1, dtype=torch.int64, device="cuda")
    head = (X.ptr(masks), X.ptr(det), X.ptr(sel_d), sel_h.ctypes.data, X.ptr(frames_d), frames_h.ctypes.data, X.ptr(off))
    tail = (B, K, K, 28, 28, 1)
    runs = {"rle": lambda: X.call("myolo_rle_masks", *head, X.ptr(buf), 3 * cap, *tail, ws_r.data_ptr(), ws_r.numel() * 8, X.stream()),
            "polygon": lambda: X.call("myolo_contour_masks", *head, X.ptr(buf), buf.data_ptr() + 8 * cap, cap, *tail, ws_c.data_ptr(),
                                      ws_c.numel() * 8, X.stream())}
    us = {}
    for name, fn in runs.items():
        fn()
        torch.cuda.synchronize()
        total = int(off[-1])
        assert total <= (3 * cap if name == "rle" else cap), (name, total)
        ts = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        us[name] = float(np.median(ts))
    return round(us["rle"], 1), round(us["polygon"], 1), round(total / (B * K), 1)


entries = {"%dx%d %s" % (f[0], f[1], kind): entry_times(f, kind) for f in ((416, 416), (3000, 4000)) for kind in ("window", "disc", "noise")}
out = {"config": "Rice 416x416 batch 4 bf16 head, random weights, cs_threshold 0", "images_per_call": N, "reps": REPS,
       "masks_per_image": round(masks / N, 2), "vertices_per_mask": round(vertices / max(masks, 1), 1),
       "images_per_sec": {k: round(v, 1) for k, v in rate.items()},
       "spread_images_per_sec": {k: [round(N / max(v), 1), round(N / min(v), 1)] for k, v in times.items()},
       "over_rle": {k: round(rate[k] / rate["rle"], 3) for k in ways},
       "mask_bytes_downloaded_per_image": {"dense": round(dense_bytes), "rle": round(rle_bytes), "polygon": round(polygon_bytes)},
       "batch_results_ms_per_batch": {k: round(float(np.median(v)), 3) for k, v in post_ms.items()},
       "entry_us_rle_polygon_vertices_per_mask": entries}
print(json.dumps(out))

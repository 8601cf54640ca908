#!/usr/bin/env python
"""What detection on photographs costs by the device resize (profiles/resize_notes.md records a run), one JSON line:
  kernel   myolo_resize_images_u8 on 4 x (768 x 1024) and 4 x (3000 x 4000) random uint8 sources into 416 x 416, HIP events around LAUNCHES
           back-to-back calls: `call_us` is the whole call (two fills of the workspace, the min/max launch, the sampling launch); `minmax_us` is the
           same call into a 1 x 1 frame (the min/max launch with a sampling launch of four threads: the closest an event timing gets to the first
           launch alone); `sample_us` their difference.  GB/s: the source bytes (every one is read once by the min/max pass) over minmax_us, and
           source + output bytes over call_us -- beside the copy bandwidth of _ext.measure_hbm_copy_gbs ("float4", same process).
  detect   MaskYOLO.detect_many (Rice 416, batch 4, bf16 mask head, seeded random weights, cs_threshold 0 so that every image keeps detections)
           on N photographs of each size, host clock around the call (it ends with the download of the last masks), RUNS runs of each route,
           alternating:  new_network / new_image = the photographs handed to detect_many as they are, mask_frame "network" / "image";
           host_resize = the route without the device resize: myolo_utils.resize_image per photograph on the host, then detect_many on the
           416 x 416 results (its output is the "network" frame's); host_resize_only_s is the resize_image part of it.
  python tools/resize_probe.py [KERNEL=1] [DETECT=1] [N=64] [RUNS=2] [LAUNCHES=200]
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
from myolo import myolo_utils as mutils                        # noqa: E402
from myolo.config import make_config, RiceConfig               # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402

KERNEL, DETECT = int(over.get("KERNEL", 1)), int(over.get("DETECT", 1))
N, RUNS, LAUNCHES = int(over.get("N", 64)), int(over.get("RUNS", 2)), int(over.get("LAUNCHES", 200))
assert torch.cuda.is_available(), "resize_probe needs a GPU: a rate measured anywhere else says nothing"
SIZES = ((768, 1024), (3000, 4000))
B, H, W = 4, 416, 416
dev = torch.device("cuda:0")
res = {}


def timed(fn, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if KERNEL:
    res["kernel"] = {"copy_gbs_float4": X.measure_hbm_copy_gbs(nbytes=1 << 30, iters=3)["float4"]}
    for h, w in SIZES:
        per = h * w * 3
        # the packed batch made on the device: descriptor, then the images back to back -- the second starts on an odd byte when per is odd
        desc = np.array([[k * per, h, w] for k in range(B)], np.int64)
        packed = torch.randint(0, 256, (B * 24 + B * per,), dtype=torch.uint8, device=dev)
        packed[:B * 24] = torch.from_numpy(desc.reshape(-1).view(np.uint8).copy()).to(dev)
        ws = torch.empty(2 * B, dtype=torch.int32, device=dev)
        out = {}
        for name, (fh, fw) in (("call", (H, W)), ("minmax", (1, 1))):
            x = torch.empty((B, fh, fw, 3), dtype=torch.float32, device=dev)

            def call():
                X.call("myolo_resize_images_u8", packed.data_ptr() + B * 24, B * per, packed.data_ptr(), desc.ctypes.data, None, X.ptr(x),
                       B, fh, fw, ws.data_ptr(), ws.numel() * 4, X.stream())
            timed(call, 20)                                     # warm-up: code objects, clocks
            reps = [timed(call, LAUNCHES) * 1e3 / LAUNCHES for _ in range(3)]
            out[name + "_us"] = float(np.median(reps))
            out[name + "_us_runs"] = reps
        out["sample_us"] = out["call_us"] - out["minmax_us"]
        out["source_bytes"] = B * per
        out["minmax_gbs"] = B * per / (out["minmax_us"] * 1e-6) / 1e9
        out["call_gbs"] = (B * per + B * H * W * 3 * 4) / (out["call_us"] * 1e-6) / 1e9
        res["kernel"]["%dx%d" % (h, w)] = out
        del packed

if DETECT:
    cfg = make_config(RiceConfig, BATCH_SIZE=B, INFERENCE_DTYPE="bf16")
    m = MaskYOLO(mode="inference", config=cfg, seed=4)
    rng = np.random.default_rng(0)
    res["detect"] = {"images": N, "runs": RUNS}
    for h, w in SIZES:
        distinct = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(8)]       # N photographs: eight distinct ones in turn
        photos = [distinct[k % 8] for k in range(N)]

        def new_route(frame):
            return m.detect_many(photos, cs_threshold=0.0, mask_frame=frame)

        def host_route():
            t0 = time.perf_counter()
            small = [mutils.resize_image(p, cfg.IMAGE_SHAPE)[0] for p in photos]
            t1 = time.perf_counter()
            return m.detect_many(small, cs_threshold=0.0), t1 - t0
        m.detect_many(photos[:2 * B], cs_threshold=0.0)                                       # warm-up: graphs, staging rings, lanes
        m.detect_many([mutils.resize_image(p, cfg.IMAGE_SHAPE)[0] for p in photos[:2 * B]], cs_threshold=0.0)
        out = {"new_network_s": [], "new_image_s": [], "host_resize_s": [], "host_resize_only_s": []}
        for _ in range(RUNS):
            for key, fn in (("new_network_s", lambda: new_route("network")), ("new_image_s", lambda: new_route("image")), ("host_resize_s", host_route)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                out[key].append(time.perf_counter() - t0)
                if key == "host_resize_s":
                    out["host_resize_only_s"].append(r[1])
                    r = r[0]
                out["kept_per_image"] = float(np.mean([len(d["class_ids"]) for d in r]))
        for key in ("new_network", "new_image", "host_resize"):
            out[key + "_images_per_sec"] = N / min(out[key + "_s"])
        res["detect"]["%dx%d" % (h, w)] = out
        del photos, distinct

print(json.dumps(res))

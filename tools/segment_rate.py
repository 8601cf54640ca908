#!/usr/bin/env python
"""What the on-device segment rasteriser costs (profiles/segment_notes.md records a run), one JSON line.  224 x 224, batch 32, T 10, on the food
outlines of tests/golden/via (cycled to fill the batch, each image sampled from its own frame), two cases, microseconds per launch:
  segment_parts  myolo_segment_masks on the outlines as single-part segments (boxes = NULL, as Net.stage_segments calls it);
  segment_rle    myolo_segment_masks on the same masks, each filled at full resolution on the host and handed over as a run-length code.
After a warm-up the two cases run REPS = 5 repetitions of LAUNCHES back-to-back launches each, alternating case by case (so that a drift of the
clock falls on both alike), HIP events around every repetition; reported: every repetition, the median, and the ratio of the medians with the
spread (max / min) of the repetitions beside them.  The two outputs are compared byte for byte before anything is timed.  (The recorded run had a
third case, the polygon kernel that has since been retired: the same outlines took 0.994 of its time as single-part segments.)
  python tools/segment_rate.py [LAUNCHES=200] [REPS=5]
"""
import json
import os
import sys

over = dict(a.split("=", 1) for a in sys.argv[1:])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo import myolo_utils as mutils                        # noqa: E402
from myolo import rle                                          # noqa: E402
from myolo.engine import Net                                   # noqa: E402
from myolo.polygon import polygon_mask                         # noqa: E402

LAUNCHES, REPS = int(over.get("LAUNCHES", 200)), int(over.get("REPS", 5))
assert torch.cuda.is_available(), "segment_rate needs a GPU: a rate measured anywhere else says nothing"
B, H, W, T = 32, 224, 224, 10
VIA = os.path.join(ROOT, "tests", "golden", "via", "food")
dev = torch.device("cuda:0")


def food_images():
    """-> [(h, w, [outline [k,2] (row, col), ...]), ...] as tools/polygon_bench.py takes them: the frame is (max y + 7, max x + 5) over the regions"""
    out = []
    for subset in ("train", "val"):
        d = json.load(open(os.path.join(VIA, subset, "via_food_annotation.json")))
        for a in d.values():
            regs = list(a["regions"].values()) if isinstance(a["regions"], dict) else a["regions"]
            if not regs:
                continue
            sh = [g["shape_attributes"] for g in regs]
            polys = [np.stack([np.asarray(s["all_points_y"], np.float64), np.asarray(s["all_points_x"], np.float64)], 1) for s in sh]
            out.append((int(max(p[:, 0].max() for p in polys)) + 7, int(max(p[:, 1].max() for p in polys)) + 5, polys))
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
group_parts, group_codes = [], []
codes_of = {}
for b in range(B):
    k = b % len(imgs)
    h, w, polys = imgs[k]
    polys = polys[:T]
    r, c = mutils.mask_index_tables(h, w, [H / h, W / w])
    if k not in codes_of:
        codes_of[k] = [rle.encode(polygon_mask(p[:, 0], p[:, 1], (h, w))) for p in polys]
    index = (r.astype(np.int32), c.astype(np.int32))
    group_parts.append(([[p] for p in polys], index, h))
    group_codes.append((codes_of[k], index, h))
sizes = {"segment_parts": mutils.segment_sizes([g[0] for g in group_parts]), "segment_rle": mutils.segment_sizes([g[0] for g in group_codes])}
d_parts = [torch.from_numpy(a).to(dev) for a in mutils.segment_tables(group_parts, B, T, H, W)]
d_codes = [torch.from_numpy(a).to(dev) for a in mutils.segment_tables(group_codes, B, T, H, W)]
out = {name: torch.full((B, H, W, T), 9, dtype=torch.uint8, device=dev) for name in ("segment_parts", "segment_rle")}
calls = {"segment_parts": lambda: Net.segment_masks(d_parts, out["segment_parts"]),
         "segment_rle": lambda: Net.segment_masks(d_codes, out["segment_rle"])}
for fn in calls.values():
    fn()
torch.cuda.synchronize()
ref = out["segment_parts"].cpu().numpy()
same = {name: bool(np.array_equal(out[name].cpu().numpy(), ref)) for name in out}
assert all(same.values()), same
for fn in calls.values():                                      # warm-up: clocks, caches, code objects
    timed(fn, 50)
us = {name: [] for name in calls}
for _ in range(REPS):
    for name, fn in calls.items():                             # alternating
        us[name].append(1e3 * timed(fn, LAUNCHES) / LAUNCHES)
med = {name: float(np.median(v)) for name, v in us.items()}
res = {"shape": {"B": B, "H": H, "W": W, "T": T}, "outlines": sizes["segment_parts"][1], "vertices": sizes["segment_parts"][0],
       "rle_boundaries": sizes["segment_rle"][2],
       "set_fraction": float(ref.mean()), "launches_per_repetition": LAUNCHES, "us_per_launch_repetitions": us, "us_per_launch_median": med,
       "spread_max_over_min": {name: float(max(v) / min(v)) for name, v in us.items()},
       "segment_rle_over_segment_parts": med["segment_rle"] / med["segment_parts"], "outputs_equal": same}
print(json.dumps(res))

#!/usr/bin/env python
"""What the training recipe costs per step, at the benchmark's configuration (Shapes 224 x 224, batch 32, alpha 1, bf16x6 products):
  optimiser   Net.adam_step (one launch) against Net.recipe_step with everything on -- clipping, decoupled weight decay, EMA, and a flags byte
              that freezes nothing (the gradient-norm reduction, its finish and the fused update: three launches) -- on the gradient a real step
              left in flat_g, REPS_INNER calls back to back between two device events;
  step        the whole training step, Net.forward_backward + either optimiser, STEPS steps between two device events.
Each way is warmed up first, then timed REPS times alternating (a drifting clock or a busy chip meets both); the medians and the spreads are
printed as one JSON line and written to profiles/optim_notes.md (DESIGN.md section 24 records a run).
  python tools/optim_rate.py [REPS=5] [STEPS=20] [REPS_INNER=50] [NOTES=profiles/optim_notes.md]
"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np                                             # noqa: E402
import torch                                                   # noqa: E402
from myolo.config import make_config, ShapesConfig             # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402
from myolo.myolo_utils import BatchGenerator                   # noqa: E402
from myolo.optim import Recipe                                 # noqa: E402
from myolo.shapes import make_shapes_samples                   # noqa: E402

over = dict(a.split("=", 1) for a in sys.argv[1:])
REPS, STEPS, INNER = int(over.get("REPS", 5)), int(over.get("STEPS", 20)), int(over.get("REPS_INNER", 50))
NOTES = over.get("NOTES", os.path.join(ROOT, "profiles", "optim_notes.md"))
assert torch.cuda.is_available(), "optim_rate needs a GPU: a time measured anywhere else says nothing"
cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], ALPHA=1.0, BATCH_SIZE=32, FP32_MATMUL="bf16x6")
LR = 0.0          # both ways keep the seed's weights, so every step of either does the same work (the positive ROIs depend on the weights); the kernels' arithmetic does not depend on the rate
recipe = Recipe(clip_norm=cfg.GRADIENT_CLIP_NORM, weight_decay=cfg.WEIGHT_DECAY, ema=0.999)


def make():
    m = MaskYOLO(mode="training", config=cfg, seed=0)
    m.set_trainable(".*")
    m.compile(LR, 0.9)
    return m


# one model per way, the same seed and batches: neither way trains on the other's weights
models = {"adam": make(), "recipe": make()}
dbs = None
for m in models.values():
    if dbs is None:
        host = [BatchGenerator(make_shapes_samples(32, cfg, start_index=32 * i), cfg, 'training', shuffle=False, norm=True)[0][0] for i in range(2)]
        dbs = [m.net.to_device_batch(b) for b in host]
torch.cuda.synchronize()


def optimiser(name):
    m = models[name]
    return (lambda: m.net.adam_step(LR)) if name == "adam" else (lambda: m.net.recipe_step(LR, recipe, m._recipe_flags()))


def events(fn, n):
    """ms per call of n calls of fn between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def step(name, k):
    m = models[name]
    m.net.forward_backward(dbs[k % len(dbs)])
    optimiser(name)()


ways = {}
for name in models:
    ways["optimiser_" + name] = (optimiser(name), INNER)
    count = {"k": 0}

    def one(name=name, count=count):
        step(name, count["k"])
        count["k"] += 1
    ways["step_" + name] = (one, STEPS)
for fn, n in ways.values():                                    # warm-up: scratch sized, allocator settled, clocks up
    events(fn, n)
    events(fn, n)
times = {k: [] for k in ways}
for _ in range(REPS):
    for k, (fn, n) in ways.items():
        times[k].append(events(fn, n))
med = {k: float(np.median(v)) for k, v in times.items()}
nparam = models["adam"].net.nparam
stats = models["recipe"].optimizer_stats()
out = {"config": "Shapes 224x224 batch 32 alpha 1 bf16x6, seed 0, lr 0 (weights held), Recipe(clip_norm=%g, weight_decay=%g, ema=0.999), all layers trainable" %
                 (recipe.clip_norm, recipe.weight_decay),
       "nparam": nparam, "buffer_mb": round(nparam * 4 / 1e6, 2), "reps": REPS, "steps_per_rep": STEPS, "optimiser_calls_per_rep": INNER,
       "ms_median": {k: round(v, 4) for k, v in med.items()},
       "ms_spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
       "optimiser_recipe_minus_adam_ms": round(med["optimiser_recipe"] - med["optimiser_adam"], 4),
       "step_recipe_over_adam": round(med["step_recipe"] / med["step_adam"], 4),
       "recipe_stats_after": stats}
print(json.dumps(out))

adam_bytes, recipe_bytes = 7 * nparam * 4, 10 * nparam * 4 + 2 * (nparam // 4)
with open(NOTES, "w") as f:
    f.write("# The training recipe's optimiser pass: what it costs (tools/optim_rate.py)\n\n")
    f.write("%s; nparam = %d (%.2f MB per flat buffer). Warm-up, then the median of %d alternating repetitions, device events around %d optimiser "
            "calls / %d whole steps. One MI355X.\n\n" % (out["config"], nparam, nparam * 4 / 1e6, REPS, INNER, STEPS))
    f.write("| what | ms (median) | fastest .. slowest repetition |\n|---|---|---|\n")
    for k in ways:
        f.write("| `%s` | %.4f | %.4f .. %.4f |\n" % (k, med[k], min(times[k]), max(times[k])))
    f.write("\nThe recipe's optimiser takes %.4f ms more than `Net.adam_step` (%.2f against %.2f MB moved: %.0f and %.0f GB/s); the whole step with "
            "the recipe takes %.4f times the plain step (%+.2f %%).\n" %
            (out["optimiser_recipe_minus_adam_ms"], recipe_bytes / 1e6, adam_bytes / 1e6, recipe_bytes / 1e6 / med["optimiser_recipe"],
             adam_bytes / 1e6 / med["optimiser_adam"], out["step_recipe_over_adam"], 100.0 * (out["step_recipe_over_adam"] - 1.0)))
    f.write("\nThe optimiser rows run back to back on the same buffers, %.0f MB (Adam) and %.0f MB (recipe) of distinct data against a 256 MB last-level "
            "cache, so they flatter both; the step rows are the ones that meet the buffers cold, behind a backward pass.\n" %
            (4 * nparam * 4 / 1e6, 5 * nparam * 4 / 1e6))
    f.write("\nThe record after the run: `%s`.\n\n```json\n%s\n```\n" % (json.dumps(stats), json.dumps(out)))

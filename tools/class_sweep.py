#!/usr/bin/env python
"""Cost of the class count: prints one JSON object with
  - the configs[1] training step (Shapes 224x224, alpha 1.0, batch 32, N_BOX 3) at NUM_CLASSES 4, 9, 16 and 81, the Shapes class
    ids remapped into the range (so the positives spread over classes like a real data set's would);
  - the Rice 416x416 bf16 inference forward (batch 4, hipGraph replay) at NUM_CLASSES 2 and 81;
  - the mask conv 1x1 kernels of more than 8 classes alone at configs[1]'s row count (32 x 147 ROIs x 784 rows, Cin 256, C 81),
    each with its roofline fraction: the fp32 forward against the 155 TF/s fp32 matrix rate (useful FLOPs, C not padded), the bf16
    forward against its bytes at 8 TB/s, the selected-class loss and backward against their bytes at 8 TB/s.
  python tools/class_sweep.py [--steps N] [--warmup W] [--skip-steps] [--skip-infer]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mask-yolo_amd")]
import numpy as np   # noqa: E402
import torch         # noqa: E402

FP32_MATRIX_TFS = 155.0     # measured fp32 matrix rate (v_mfma_f32_32x32x2_f32)
HBM_TBS = 8.0


def _labels(n):
    return ["background"] + ["class%d" % i for i in range(1, n)]


def _remap(C):
    """Shapes ids 1..3 -> three classes spread over 1..C-1 (identity at C = 4)"""
    if C <= 4:
        return {1: 1, 2: 2, 3: 3}
    return {1: max(1, C // 5), 2: max(2, C // 2), 3: C - 1}


def time_events(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def train_step_ms(C, steps, warmup):
    from myolo.config import make_config, ShapesConfig
    from myolo.model import MaskYOLO
    from myolo.shapes import make_shapes_samples
    from myolo.myolo_utils import BatchGenerator
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[224, 224, 3], ALPHA=1.0, BATCH_SIZE=32, NUM_CLASSES=C, LABELS=_labels(C))
    model = MaskYOLO(mode="training", config=cfg, seed=0)
    net = model.net
    rm = _remap(C)
    dbs = []
    for k in range(2):
        samples = make_shapes_samples(32, cfg, start_index=32 * k)
        for s in samples:
            s[1] = np.asarray([rm[int(c)] for c in s[1]], dtype=np.asarray(s[1]).dtype)
        batch, _ = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0]
        dbs.append(net.to_device_batch(batch))
    i = [0]

    def step():
        net.train_step(dbs[i[0] % 2], 1e-4)
        i[0] += 1
    ms = time_events(step, steps, warmup)
    del model, net, dbs
    torch.cuda.empty_cache()
    return ms


def infer_ms(C, steps, warmup):
    from myolo.config import make_config, RiceConfig
    from myolo.engine import Net
    cfg = make_config(RiceConfig, BATCH_SIZE=4, INFERENCE_DTYPE="bf16", NUM_CLASSES=C, LABELS=_labels(C))
    net = Net(cfg, device="cuda:0", seed=0)
    x = torch.rand(4, 416, 416, 3, device="cuda:0")
    ms = time_events(lambda: net.predict_graphed(x), steps, warmup)
    del net
    torch.cuda.empty_cache()
    return ms


def kernels(iters):
    from myolo import _ext as X
    X.load()
    NR, hw, Cin, C = 32 * 147, 784, 256, 81
    M = NR * hw
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.relu(torch.randn(M, Cin, device="cuda", generator=g))
    w = torch.randn(Cin, C, device="cuda", generator=g) * 0.05
    b = torch.randn(C, device="cuda", generator=g) * 0.1
    p = torch.empty(M, C, device="cuda")
    out = {}
    t = time_events(lambda: X.call("myolo_mask_head_out_fwd", X.ptr(x), X.ptr(w), X.ptr(b), X.ptr(p), M, Cin, C, X.stream()), iters, 2)
    fl = 2.0 * M * Cin * C
    out["mask_head_out_fwd_fp32"] = dict(ms=round(t, 4), tflops=round(fl / t / 1e9, 1), frac_fp32_matrix_peak=round(fl / t / 1e9 / FP32_MATRIX_TFS, 3),
                                         gbytes=round((M * Cin + M * C) * 4 / 1e9, 2))
    xb = x.to(torch.bfloat16)
    t = time_events(lambda: X.call("myolo_mask_head_out_bf16_fwd", X.ptr(xb), X.ptr(w), X.ptr(b), X.ptr(p), M, Cin, C, X.stream()), iters, 2)
    by = M * Cin * 2 + M * C * 4
    out["mask_head_out_fwd_bf16"] = dict(ms=round(t, 4), frac_hbm_8tbs=round(by / t / 1e9 / HBM_TBS, 3), gbytes=round(by / 1e9, 2))
    del xb
    ids = torch.randint(0, C, (NR,), device="cuda", dtype=torch.int32, generator=g)
    tm = (torch.rand(M, device="cuda", generator=g) > 0.5).float()
    ws = torch.empty(max(64 << 20, X.mask_bwd_sel_ws_bytes(NR, Cin)), dtype=torch.uint8, device="cuda")
    terms = torch.empty(2, device="cuda")
    dz = torch.empty(M, device="cuda")
    t = time_events(lambda: X.call("myolo_mask_bce_sel", X.ptr(tm), X.ptr(ids), X.ptr(p), 1.0, X.ptr(terms), X.ptr(dz), NR, 28, 28, C,
                                   X.ptr(ws), ws.numel(), X.stream()), iters, 2)
    by = M * 4 * 3 + M * 4        # target, the selected probability (a 4-byte read per row; the lines of p it touches), dz_sel; ids
    out["mask_bce_sel"] = dict(ms=round(t, 4), frac_hbm_8tbs=round(by / t / 1e9 / HBM_TBS, 3), gbytes=round(by / 1e9, 2))
    dx = torch.empty_like(x)
    dw, db = torch.empty(Cin, C, device="cuda"), torch.empty(C, device="cuda")
    t = time_events(lambda: X.call("myolo_mask_head_out_bwd_sel", X.ptr(x), X.ptr(w), X.ptr(dz), X.ptr(ids), X.ptr(dx), X.ptr(dw), X.ptr(db), M, Cin,
                                   C, hw, X.ptr(ws), ws.numel(), X.stream()), iters, 2)
    by = 2 * M * Cin * 4 + M * 4
    out["mask_head_out_bwd_sel"] = dict(ms=round(t, 4), frac_hbm_8tbs=round(by / t / 1e9 / HBM_TBS, 3), gbytes=round(by / 1e9, 2))
    out["shape"] = dict(M=M, Cin=Cin, C=C)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=10)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--skip-infer", action="store_true")
    args = ap.parse_args()
    t0 = time.time()
    res = {"kernels_configs1_rows": kernels(args.kernel_iters)}
    torch.cuda.empty_cache()
    if not args.skip_steps:
        res["train_step_ms_shapes224_b32"] = {str(C): round(train_step_ms(C, args.steps, args.warmup), 3) for C in (4, 9, 16, 81)}
    if not args.skip_infer:
        res["infer_ms_rice416_bf16_b4"] = {str(C): round(infer_ms(C, args.steps, args.warmup), 3) for C in (2, 81)}
    res["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

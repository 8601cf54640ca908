"""Data-parallel step on real kernels: 2 / 4 / 5 processes share cuda:0, rendezvous over gloo (it accepts
device tensors), each runs the REAL engine (myolo.engine.Net) on its own shard with the bucketed, overlapped GradReducer.
  * the all-reduced, 1/world-scaled gradient equals the mean of the `world` single-rank gradients (<= 1e-5 relative) -- SURVEY
    8(e)'s "8-rank averaged gradient == mean of 8 single-GPU gradients on the same shards" at up to 5 ranks (with the test process
    itself, six processes hold the GPU: the most a shared GPU takes);
  * after Adam every rank holds bit-identical weights;
  * with frozen layers (set_trainable / the yolo_trainable=False recipe) the frozen weights stay bit-identical -- the
    reducer is joined before the freeze mask is applied (round-1 advisor finding).
RCCL itself needs one GPU per rank; on a 1-GPU box it is exercised as a 1-rank communicator through the C-ABI
(myolo_comm_*), which checks the dlopen'ed librccl, the stream plumbing and the timing instrumentation; on a box with >= 2 GPUs
test_two_rank_step_over_rccl runs the same parity check over real RCCL, through torch.distributed (nccl) and through the C-ABI."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case(world=2):
    from myolo.config import make_config, ShapesConfig
    from myolo.shapes import make_shapes_samples
    from myolo.myolo_utils import BatchGenerator
    from myolo.engine import init_state_dict
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4)
    P = init_state_dict(cfg, seed=5)
    batches = []
    for r in range(world):
        samples = make_shapes_samples(4, cfg, start_index=40 + 4 * r)
        batches.append(BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0][0])
    return cfg, P, batches


def _force_positives(net, cfg, k=3):
    """the first k proposals of every image are replaced by a ground-truth box (IoU 1 -> positive): the compacted mask-head backward, conv1's
    dense backward on its side stream and the release of the mask-head bucket BEHIND that stream's work all run under the reducer"""
    def hook(proposals, db):
        gt = db["gt_boxes"].to(torch.float32)                       # [B,T,4] px, x1 y1 x2 y2
        H, W = float(cfg.IMAGE_SHAPE[0]), float(cfg.IMAGE_SHAPE[1])
        norm = (gt - torch.tensor([0., 0., 1., 1.], device=gt.device)) / torch.tensor([W - 1, H - 1, W - 1, H - 1], device=gt.device)
        proposals[:, :k, :] = norm[:, :1, :].expand(-1, k, -1)
    net.proposals_hook = hook


def _worker(rank, world, port, q, freeze, backend="gloo", reducer="torch", positives=False):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = "cuda:%d" % rank if backend == "nccl" else "cuda:0"       # RCCL: one GPU per rank; gloo: every rank on cuda:0
    if backend == "nccl":
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from myolo.model import MaskYOLO
        from myolo.dist import GradReducer
        cfg, P, batches = _case(world)
        # ---- single-rank gradients of EVERY shard (no communication) -> their mean is the expected exchanged gradient
        solo = MaskYOLO(mode="training", config=cfg, device=dev)
        if positives:
            _force_positives(solo.net, cfg)
        expect = None
        npos_seen = 0
        for b in batches:
            solo.load_state_dict(P)
            out = solo.net.forward_backward(solo.net.to_device_batch(b))
            npos_seen += int(out["n_pos"].sum())
            solo.net.join_conv1_wgrad()
            torch.cuda.synchronize()
            expect = solo.net.flat_g.double() if expect is None else expect + solo.net.flat_g.double()
        expect = (expect / world).float()
        del solo
        # ---- the data-parallel step: own shard, bucketed overlapped all-reduce, 1/world inside Adam
        model = MaskYOLO(mode="training", config=cfg, device=dev)
        model.load_state_dict(P)
        if positives:
            _force_positives(model.net, cfg)
            assert npos_seen >= 3 * len(batches), "forcing positives did not produce positives (%d)" % npos_seen
        model._reducer = GradReducer(model.net.flat_g, model.net.bucket_ranges, timing=True, backend=reducer).attach(model.net)
        assert model._reducer.world == world and model._reducer.ranks_seen() == world
        if freeze:
            model.set_trainable(r"(myolo_mask.*)|(feature_map)|(conv_23)|(conv_.w_1[0-4].*)")   # the mask side has no gradient when a random-init batch has no positive ROI
        else:
            model.set_trainable(".*")
        model.compile(1e-3, 0.9)
        before = model.net.flat_p.clone()
        model.train_on_batch(batches[rank])
        torch.cuda.synchronize()
        got = model.net.flat_g * model.net.grad_scale
        if freeze:
            m = model._train_mask
            err = float(((got - expect * m).abs().max() / expect.abs().max()).item())
        else:
            err = float(((got - expect).abs().max() / expect.abs().max()).item())
        after = model.net.flat_p.clone()
        if backend == "nccl":
            gathered = [torch.zeros_like(after) for _ in range(world)]
            dist.all_gather(gathered, after)
            gathered = [t.cpu() for t in gathered]
        else:
            gathered = [torch.zeros(after.numel()) for _ in range(world)]
            dist.all_gather(gathered, after.cpu())
        same = all(torch.equal(gathered[0], t) for t in gathered)
        frozen_ok = "ok"
        if freeze:
            fz = model._train_mask == 0
            if not torch.equal(after[fz], before[fz]):
                frozen_ok = "frozen weights moved: %d entries, max %g" % (int((after[fz] != before[fz]).sum()), float((after[fz] - before[fz]).abs().max()))
            elif not bool((after[~fz] != before[~fz]).any()):
                frozen_ok = "trainable weights did not move"
        ms = model._reducer.bucket_ms()
        q.put((rank, err, same, frozen_ok, str(ms) if not (ms is not None and len(ms) == 5 and all(v >= 0 for v in ms)) else "ok"))
        if model._reducer.backend == "capi":
            model._reducer.close()
    finally:
        dist.destroy_process_group()


def _run_ranks(world, freeze, backend="gloo", reducer="torch", positives=False):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, freeze, backend, reducer, positives)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert [r[0] for r in res] == list(range(world))
    for rank, err, same, frozen_ok, timed in res:
        assert err < 1e-5, (rank, err)                # averaged gradient == mean of the single-rank gradients
        assert same, "ranks hold different weights after Adam"
        assert frozen_ok == "ok", frozen_ok
        assert timed == "ok", timed


@pytest.mark.parametrize("world,freeze", [(2, False), (2, True), (4, False), (5, False)])
def test_n_rank_step_real_engine_gloo_on_one_gpu(world, freeze):
    """SURVEY 8(e)'s parity test for 2 / 4 / 5 ranks (the ranks share the one GPU of the box; the transport is gloo; five ranks plus the test
    process are the most processes a shared GPU takes, and an odd world checks the 1/world scaling where it is not a power of two)."""
    _run_ranks(world, freeze)


@pytest.mark.parametrize("world", [2, 4])
def test_n_rank_step_with_positive_rois(world):
    """the same parity check with positive ROIs in every image (a random-init net proposes almost none): the mask-head bucket is then complete
    only behind the side stream that carries the compacted weight gradients and conv1's dense weight gradient, and is released there."""
    _run_ranks(world, False, positives=True)


@pytest.mark.parametrize("reducer", ["torch", "capi"])
def test_two_rank_step_over_rccl(reducer):
    """The same check over real RCCL, one GPU per rank: through torch.distributed's nccl backend and through the library's own
    myolo_comm_* entry points.  Needs >= 2 visible GPUs (the driver's 1-GPU test box skips it; an 8-GPU node runs it)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL has one device per rank)")
    _run_ranks(2, False, backend="nccl", reducer=reducer)


def test_rccl_through_the_c_abi_one_rank():
    """myolo_comm_unique_id / comm_init / comm_size / allreduce_sum_f32 / comm_destroy on a 1-rank RCCL communicator, driven
    by GradReducer(backend='capi'): sum over one rank is the identity, on the reducer's side stream, with event timing."""
    from myolo.dist import GradReducer
    g = torch.randn(1 << 20, device="cuda:0")
    g0 = g.clone()
    red = GradReducer(g, [(0, 300000), (300000, 700000), (700000, 1 << 20)], always=True, backend="capi", timing=True)
    try:
        assert red.active and red.comm is not None and red.ranks_seen() == 1
        for _ in range(2):
            for i in (2, 1, 0):
                red.bucket_ready(i)
            red.wait()
        torch.cuda.synchronize()
        assert torch.equal(g, g0)
        ms = red.bucket_ms()
        assert len(ms) == 3 and all(v > 0 for v in ms)
        rel = red.release_ms_before_wait()
        assert len(rel) == 3 and all(v >= 0 for v in rel)
    finally:
        red.close()


def test_engine_releases_buckets_where_backward_finishes_them():
    """SURVEY 8(e) "each bucket launched when its last dW kernel completes": with a (1-rank, C-ABI) reducer attached, every one of the five buckets is
    released exactly once per step, the YOLO-head bucket FIRST (its backward runs on a side stream under the mask head) and the backbone LAST, and the
    YOLO-head and mask-head-rest buckets are released EARLIER (relative to the end of backward) than conv1's and the backbone's."""
    from myolo.model import MaskYOLO
    from myolo.dist import GradReducer
    from myolo import engine as E
    cfg, P, batches = _case()
    model = MaskYOLO(mode="training", config=cfg, device="cuda:0")
    model.load_state_dict(P)
    red = GradReducer(model.net.flat_g, model.net.bucket_ranges, always=True, backend="capi", timing=True).attach(model.net)
    assert model.net.exchange_active and model.net.yolo_bwd_early == -1      # an active exchange: the YOLO head's backward goes under the mask head's forward
    order = []
    inner = model.net.on_bucket_ready
    model.net.on_bucket_ready = lambda i: (order.append(i), inner(i))[1]
    try:
        model.set_trainable(".*")
        model.compile(1e-3, 0.9)
        for k in range(3):
            del order[:]
            model.train_on_batch(batches[k % len(batches)])
            assert sorted(order) == list(range(E.N_BUCKETS)), order
            assert order[0] == E.BUCKET_YOLO and order[-1] == E.BUCKET_BACKBONE, order
            assert order.index(E.BUCKET_MASK_REST) < order.index(E.BUCKET_MASK_CONV1), order
        rel = red.release_ms_before_wait()
        assert len(rel) == E.N_BUCKETS and all(v >= 0 for v in rel)
        assert rel[E.BUCKET_YOLO] > rel[E.BUCKET_BACKBONE] and rel[E.BUCKET_MASK_REST] >= rel[E.BUCKET_MASK_CONV1] - 0.05, rel
    finally:
        model.net.on_bucket_ready = inner
        red.close()


def test_engine_step_with_capi_reducer_is_bit_identical_to_no_reducer():
    from myolo.model import MaskYOLO
    from myolo.dist import GradReducer
    cfg, P, batches = _case()
    outs = []
    for use in (False, True):
        model = MaskYOLO(mode="training", config=cfg, device="cuda:0")
        model.load_state_dict(P)
        red = None
        if use:
            red = GradReducer(model.net.flat_g, model.net.bucket_ranges, always=True, backend="capi").attach(model.net)
        model.set_trainable(".*")
        model.compile(1e-3, 0.9)
        model.train_on_batch(batches[0])
        torch.cuda.synchronize()
        outs.append(model.net.flat_p.clone())
        if red:
            red.close()
    assert torch.equal(outs[0], outs[1])


def test_bench_plain_run_measures_only_the_headline(tmp_path):
    """`python bench.py` without --full on one GPU: set-up, warm-up, the timed steps, --dump-outputs and the ONE line -- no CPU baseline, no
    variants, no second per-kernel pass, probes or secondary configurations.  The dominant kernel's roofline, timed inside the region, stays."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    detail = os.path.join(root, "plain_bench_detail.json")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4", "--size", "128", "--alpha", "0.5",
                        "--detail-name", os.path.basename(detail), "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) < 6000, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-5 * d["value"]
    assert d["cpu_baseline"] is None and d["roofline"]["avg_launch_ms"] > 0 and "depthwise" not in d["roofline"]
    full = json.load(open(detail))
    os.remove(detail)
    for k in ("variants", "train_api", "hbm_copy_measured_gbs", "power_limit_probe", "secondary_nbox5", "inference_rice416_bf16", "comm"):
        assert k not in full, k
    assert "trunk_layers" not in full["roofline"] and "traffic_live" not in full["roofline"]
    assert len(os.listdir(str(tmp_path / "out"))) == 12                          # what the last timed step returned + the weights after it


def test_bench_multi_rank_path_on_one_gpu(tmp_path):
    """`python bench.py --gpus 2` end to end on this one-GPU box: the script re-launches itself under torch.distributed.run, two ranks
    build the engine, exchange gradients every step (gloo instead of RCCL: --share-gpu puts both ranks on cuda:0), take the MAX over
    ranks of the timed region, and rank 0 prints ONE JSON line on stdout with n_gpus = 2, the comm object (two ranks seen, five
    bucket timings) and weak-scaling semantics (global batch = 2 x per-GPU batch).  What the driver's 8-GPU command runs, minus the wire."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--share-gpu", "--steps", "3", "--warmup", "1", "--batch", "4",
                        "--size", "128", "--alpha", "0.5", "--cpu-images", "0", "--full", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                                   # stdout carries exactly the JSON line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert d["config"]["global_batch"] == 8 and d["config"]["parallelism"] == "dp2" and d["config"]["share_gpu"] is True
    assert d["comm"]["rccl_ranks_seen"] == 2 and len(d["comm"]["bucket_allreduce_ms"]) == 5 and all(v > 0 for v in d["comm"]["bucket_allreduce_ms"])
    assert d["value"] > 0 and abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) < 1e-5 * d["value"]      # (both are printed rounded to four decimals)
    assert d["dense_mask_backward_ms_per_step"] > 0                               # the variants ran in lockstep on both ranks
    assert len(lines[0]) < 6000 and d["detail"] == "bench_detail.json"            # the compact line; the full object is beside it
    full = json.load(open(os.path.join(root, "bench_detail.json")))
    assert "variants" in full and "dense_mask_backward" in full["variants"] and "trunk_layers" in full["roofline"]
    # --dump-outputs: rank 0's last timed step, as its caller received it, plus the weights after its update
    got = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in os.listdir(str(tmp_path / "out"))}
    assert set(got) == {"yolo_output", "yolo_proposals", "output_rois", "myolo_mask", "target_class_ids", "target_mask", "n_pos", "yolo_terms",
                        "mask_terms", "feature_map", "loss_weights", "weights_after_step"}, sorted(got)
    assert all(a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)) for a in got.values())
    assert got["yolo_output"].shape[0] == 4 and got["myolo_mask"].shape[:2] == got["target_class_ids"].shape == got["output_rois"].shape[:2]
    assert got["n_pos"].shape == (4,) and sum(a.nbytes for a in got.values()) <= 64 << 20


def test_bench_four_ranks_at_full_config2_size_on_one_gpu():
    """BASELINE configs[2] minus the wire: `bench.py --gpus 4` at the FULL per-GPU size (224 x 224, batch 32 per rank, alpha 1, R = 147) with
    the four ranks sharing this box's one GPU (gloo transport; RCCL needs a device per rank; more ranks plus the test process would exceed the
    six processes a shared GPU takes).  Four ranks are seen by the reducer, the global batch is 128, every rank holds bit-identical weights after
    the averaged updates, the line is well-formed.  Not a throughput claim."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4", "--share-gpu", "--steps", "3", "--warmup", "1", "--cpu-images", "0",
                        "--full", "--no-variant", "--no-extras"], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) < 6000, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["config"]["global_batch"] == 128 and d["config"]["parallelism"] == "dp4" and d["config"]["share_gpu"] is True
    assert d["comm"]["rccl_ranks_seen"] == 4 and len(d["comm"]["bucket_allreduce_ms"]) == 5
    assert d["comm"]["weights_identical_across_ranks"] is True
    assert "224x224" in d["config"]["workload"] and "batch 32/GPU" in d["config"]["workload"] and np.isfinite(d["config"]["final_loss"])

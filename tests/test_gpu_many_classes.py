"""More than eight mask classes (the reference builds its mask head for any NUM_CLASSES, model.py:668-754): the matrix-pipe
forms of the mask conv 1x1 (myolo_mask_head_out_fwd / _bf16_fwd above 8 classes), the selected-channel loss and backward
(myolo_mask_bce_sel, myolo_mask_head_out_bwd_sel), and the training step, inference and post-processing at 81 classes
against the oracle.  Shapes class ids are remapped to {17, 45, 80} so that a kernel that ignores the class index fails."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_model, np_ops as O                      # noqa: E402
from myolo.config import make_config, ShapesConfig, ShapesHeadConfig  # noqa: E402
from myolo.model import MaskYOLO                               # noqa: E402
from myolo.shapes import make_shapes_samples                   # noqa: E402
from myolo.myolo_utils import BatchGenerator                   # noqa: E402
from test_gpu_step import TOL, rel, decision_margins, compare_step, make_case   # noqa: E402

NC = 81
REMAP = {1: 17, 2: 45, 3: 80}
U = 2.0 ** -24


def _labels(n):
    return ["background"] + ["class%d" % i for i in range(1, n)]


def _cfg(base=ShapesConfig, **kw):
    return make_config(base, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4, NUM_CLASSES=NC, LABELS=_labels(NC), **kw)


_CASES = {}


def many_class_case(base=ShapesConfig, seed=0, need_pos=2, min_margin=1e-3, min_roi_px=4e-3):
    """test_gpu_step._make_case with NUM_CLASSES = 81 and the Shapes class ids remapped into the range"""
    key = (base, seed)
    if key in _CASES:
        return _CASES[key]
    cfg = _cfg(base)
    P = np_model.init_params(cfg, seed=seed, bias_scale=0.05)
    B = cfg.BATCH_SIZE
    for start in range(0, 400 * B, B):
        samples = make_shapes_samples(B, cfg, start_index=start)
        for s in samples:
            s[1] = np.asarray([REMAP[int(c)] for c in s[1]], dtype=np.asarray(s[1]).dtype)
        batch, _ = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0]
        T = np_model.Tape(P, cfg, training=True)
        C4, Fm, yo = T.trunk(batch[0])
        prop = O.yolo_decode(yo, cfg.ANCHORS, cfg.GRID_W)
        rois, tcls, tmask, npos = O.mask_targets(prop, batch[3], batch[4], batch[5], cfg)
        if npos.sum() < need_pos:
            continue
        mg = decision_margins(cfg, batch, yo, prop, rois, Fm.shape[1])
        if min(mg["partition"], mg["noobj"]) > min_margin and mg["roi_px"] > min_roi_px:
            ref = np_model.train_step_fwd_bwd(P, batch, cfg)
            assert set(np.unique(ref["target_class_ids"])) - {0} <= set(REMAP.values())
            _CASES[key] = (cfg, P, batch, ref)
            return _CASES[key]
    raise RuntimeError("no batch with positive ROIs and safe decision margins found")


def _X():
    from myolo import _ext as X
    X.load()
    return X


def _ws(nbytes=64 << 20):
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def _fwd(x, w, b, C):
    X = _X()
    M, Cin = x.shape
    p = torch.empty(M, C, device="cuda")
    name = "myolo_mask_head_out_bf16_fwd" if x.dtype == torch.bfloat16 else "myolo_mask_head_out_fwd"
    X.call(name, X.ptr(x), X.ptr(w), X.ptr(b), X.ptr(p), M, Cin, C, X.stream())
    torch.cuda.synchronize()
    return p


def _sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-z))


# ---------------------------------------------------------------------------------------------------------------- 1, 2: forward
@pytest.mark.parametrize("C", [9, 16, 33, 81, 128])
def test_mask_out_fwd_many_classes_vs_float64(C):
    """p = sigmoid(x w + b) on the fp32 matrix pipe: per element within the fp32 product bound of the logit, carried through the
    sigmoid, plus the sigmoid's own rounding; a ragged row count; two runs give the same bits."""
    g = torch.Generator().manual_seed(C)
    M, Cin = 3 * 784 + 45, 256
    x = torch.relu(torch.randn(M, Cin, generator=g)).cuda()
    w = (torch.randn(Cin, C, generator=g) * 0.08).cuda()
    b = (torch.randn(C, generator=g) * 0.3).cuda()
    p = _fwd(x, w, b, C).cpu().numpy().astype(np.float64)
    x64, w64, b64 = (t.cpu().numpy().astype(np.float64) for t in (x, w, b))
    z = x64 @ w64 + b64
    zb = 4 * Cin * U * (np.abs(x64) @ np.abs(w64)) + 2 * U * (np.abs(z) + np.abs(b64))
    s = _sigmoid64(z)
    err = np.abs(p - s)
    bound = s * (1 - s) * zb * 1.01 + 4 * U
    assert np.all(err <= bound), (float((err / bound).max()), float(err.max()))
    assert np.isfinite(p).all() and p.shape == (M, C)
    p2 = _fwd(x, w, b, C).cpu().numpy().astype(np.float64)
    assert np.array_equal(p, p2), "two runs differ"


def test_mask_out_bf16_fwd_81_classes():
    """bf16 activations: against the fp32 kernel on the same bf16-rounded activations, max abs <= 8e-3 (the fused bf16 path's bound)"""
    g = torch.Generator().manual_seed(7)
    M, Cin, C = 2 * 784 + 19, 256, NC
    xb = torch.relu(torch.randn(M, Cin, generator=g)).to(torch.bfloat16).cuda()
    w = (torch.randn(Cin, C, generator=g) * 0.08).cuda()
    b = (torch.randn(C, generator=g) * 0.3).cuda()
    pb = _fwd(xb, w, b, C)
    pf = _fwd(xb.float().contiguous(), w, b, C)
    d = float((pb - pf).abs().max())
    assert d <= 8e-3, d
    assert d > 0, "bf16 path gave the fp32 bits: the weights were not rounded"
    assert torch.equal(pb, _fwd(xb, w, b, C))


# ---------------------------------------------------------------------------------------------------------------- 3: the loss
def _bce(tm, ids, pred, C, sel):
    X = _X()
    NR = ids.numel()
    terms = torch.empty(2, device="cuda")
    dz = torch.empty(pred.shape[0], 1 if sel else C, device="cuda")
    ws = _ws(1 << 20)
    X.call("myolo_mask_bce_sel" if sel else "myolo_mask_bce", X.ptr(tm), X.ptr(ids), X.ptr(pred), 0.7, X.ptr(terms), X.ptr(dz), NR, 28, 28, C,
           X.ptr(ws), ws.numel(), X.stream())
    torch.cuda.synchronize()
    return terms.cpu().numpy(), dz


@pytest.mark.parametrize("C,ids", [(4, [0, 3, 1, 0, 2, 3, 0]), (NC, [0, 80, 17, 1, 0, 45, 80]), (NC, [0, 0, 0])])
def test_mask_bce_sel_equals_dense(C, ids):
    g = torch.Generator().manual_seed(C + len(ids))
    NR = len(ids)
    idt = torch.tensor(ids, dtype=torch.int32).cuda()
    tm = (torch.rand(NR * 784, generator=g) > 0.5).float().cuda()
    pred = torch.rand(NR * 784, C, generator=g)
    pred[::97] = 0.0                      # outside [eps, 1 - eps]: zero gradient
    pred[1::89] = 1.0
    pred = pred.cuda()
    t_d, dz = _bce(tm, idt, pred, C, False)
    t_s, dz_sel = _bce(tm, idt, pred, C, True)
    assert np.array_equal(t_d.view(np.uint32), t_s.view(np.uint32)), (t_d, t_s)
    rows = torch.arange(NR * 784, device="cuda")
    want = dz[rows, idt.long().repeat_interleave(784)]
    assert torch.equal(dz_sel.view(-1).view(torch.int32), want.view(torch.int32))
    if max(ids) == 0:
        assert t_s[0] == 0 and t_s[1] == 0 and not dz_sel.any()
    else:
        assert dz_sel.abs().sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 4: the backward
def _bwd_dense(x, w, dz, C):
    X = _X()
    M, Cin = x.shape
    dx, dw, db = torch.empty_like(x), torch.empty(Cin, C, device="cuda"), torch.empty(C, device="cuda")
    ws = _ws(256 << 20)
    X.call("myolo_mask_head_out_bwd", X.ptr(x), X.ptr(w), X.ptr(dz), X.ptr(dx), X.ptr(dw), X.ptr(db), M, Cin, C, X.ptr(ws), ws.numel(), X.stream())
    torch.cuda.synchronize()
    return dx, dw, db


def _bwd_sel(x, w, dz_sel, ids, C, hw=784):
    X = _X()
    M, Cin = x.shape
    dx = torch.full_like(x, float("nan"))
    dw, db = torch.full((Cin, C), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    ws = _ws(X.mask_bwd_sel_ws_bytes(M // hw, Cin))
    X.call("myolo_mask_head_out_bwd_sel", X.ptr(x), X.ptr(w), X.ptr(dz_sel), X.ptr(ids), X.ptr(dx), X.ptr(dw), X.ptr(db), M, Cin, C, hw,
           X.ptr(ws), ws.numel(), X.stream())
    torch.cuda.synchronize()
    return dx, dw, db


def _sel_inputs(C, ids, seed):
    g = torch.Generator().manual_seed(seed)
    NR, Cin = len(ids), 256
    x = torch.randn(NR * 784, Cin, generator=g)             # both signs: the ReLU mask matters
    w = torch.randn(Cin, C, generator=g) * 0.1
    idt = torch.tensor(ids, dtype=torch.int32)
    g_rows = torch.randn(NR * 784, generator=g) * 1e-3
    valid = ((idt > 0) & (idt < C)).repeat_interleave(784)
    dz_sel = torch.where(valid, g_rows, torch.zeros_like(g_rows))
    return x.cuda(), w.cuda(), idt.cuda(), dz_sel.cuda()


@pytest.mark.parametrize("C", [4, 8])
def test_mask_out_bwd_sel_equals_dense_on_one_hot(C):
    ids = [0, 1, C - 1, 2, 0, C - 1]
    x, w, idt, dz_sel = _sel_inputs(C, ids, C)
    M = x.shape[0]
    dz = torch.zeros(M, C, device="cuda")
    rows = torch.arange(M, device="cuda")
    dz[rows, idt.long().repeat_interleave(784)] = dz_sel
    dx_d, dw_d, db_d = _bwd_dense(x, w, dz, C)
    dx_s, dw_s, db_s = _bwd_sel(x, w, dz_sel, idt, C)
    assert torch.equal(dx_s.view(torch.int32), dx_d.view(torch.int32)), "dx differs from the dense kernel"
    S = (x.abs().double().t() @ dz.abs().double()).cpu().numpy()
    assert np.all(np.abs(dw_s.double().cpu().numpy() - dw_d.double().cpu().numpy()) <= 256 * U * S + 1e-30)
    Sb = dz.abs().double().sum(0).cpu().numpy()
    assert np.all(np.abs(db_s.double().cpu().numpy() - db_d.double().cpu().numpy()) <= 256 * U * Sb + 1e-30)


def test_mask_out_bwd_sel_81_classes_vs_float64():
    ids = [0, 17, 80, 45, 1, 17, 0, 80]
    x, w, idt, dz_sel = _sel_inputs(NC, ids, 81)
    dx, dw, db = _bwd_sel(x, w, dz_sel, idt, NC)
    x64, w64, g64 = x.double().cpu().numpy(), w.double().cpu().numpy(), dz_sel.double().cpu().numpy()
    cls = np.repeat(np.asarray(ids), 784)
    dx_ref = np.where(x64 > 0, g64[:, None] * w64.T[cls], 0.0)
    assert np.all(np.abs(dx.double().cpu().numpy() - dx_ref) <= U * np.abs(dx_ref))
    dw_ref, db_ref = np.zeros((256, NC)), np.zeros(NC)
    S = np.zeros((256, NC))
    for k in set(ids) - {0}:
        m = cls == k
        dw_ref[:, k] = x64[m].T @ g64[m]
        S[:, k] = np.abs(x64[m]).T @ np.abs(g64[m])
        db_ref[k] = g64[m].sum()
    dw_h, db_h = dw.double().cpu().numpy(), db.double().cpu().numpy()
    assert np.all(np.abs(dw_h - dw_ref) <= 2 * U * np.abs(dw_ref) + 1e-12 * S)
    assert np.all(np.abs(db_h - db_ref) <= 2 * U * np.abs(db_ref) + 1e-15)
    absent = [k for k in range(NC) if k not in ids or k == 0]
    assert np.all(dw_h[:, absent] == 0) and np.all(db_h[absent] == 0)
    dx2, dw2, db2 = _bwd_sel(x, w, dz_sel, idt, NC)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)


# ---------------------------------------------------------------------------------------------------------------- 5: teacher-forced head
@pytest.mark.parametrize("sparse", [False, True])
def test_mask_head_teacher_forced_81_classes(sparse):
    """test_gpu_step.test_mask_head_teacher_forced at 81 classes: the oracle's feature map and ROIs in, the selected-channel loss and
    backward, every mask-head gradient and dF within 5e-3 relative L2 / 5e-2 max-norm of the oracle's tape"""
    cfg, P, batch, ref = many_class_case()
    model = MaskYOLO(mode="training", config=cfg)
    model.load_state_dict(P)
    net = model.net
    net.sparse_mask_bwd = sparse
    net.tape = {}
    Fm = torch.as_tensor(ref["feature_map"], device=net.dev).contiguous()
    n, h, w, cf = Fm.shape
    rois = torch.as_tensor(ref["output_rois"], device=net.dev).contiguous()
    tcls = torch.as_tensor(ref["target_class_ids"], device=net.dev).contiguous()
    tmask = torch.as_tensor(ref["target_mask"], device=net.dev).contiguous()
    B, R = rois.shape[:2]
    pred = net.mask_head_fwd(Fm.view(n * h * w, cf), (n, h, w, cf), rois, True)
    assert pred.shape[1] == NC
    assert rel(pred.cpu().numpy().reshape(ref["myolo_mask"].shape), ref["myolo_mask"]) < 1e-4
    mterms, dz = net.mask_bce(tmask, tcls, pred, 1.0, B * R)
    assert dz.shape == (pred.shape[0], 1)
    if sparse:
        net._start_npos_copy(torch.as_tensor(ref["n_pos"].astype(np.int32), device=net.dev))
        dF = net.mask_head_bwd_sparse(dz, B, R, tcls)
    else:
        dF = net.mask_head_bwd(dz, tcls)
    grads = net.grads_dict()
    T = ref["tape"]
    G = {}
    ml, dpred = O.mask_bce(ref["target_mask"], ref["target_class_ids"], ref["myolo_mask"], want_grad=True)
    dF_ref = T.mask_head_bwd(dpred, G)
    assert abs(float(mterms.cpu().numpy()[0]) - float(ml)) < 1e-5

    def l2(a, b):
        return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(1e-30, np.linalg.norm(b)))
    worst_l2 = l2(dF.cpu().numpy().reshape(dF_ref.shape), dF_ref)
    worst_max = rel(dF.cpu().numpy().reshape(dF_ref.shape), dF_ref)
    for k, g in G.items():
        if k == "myolo_mask_conv1/bias":
            continue
        worst_l2 = max(worst_l2, l2(grads[k], g))
        worst_max = max(worst_max, rel(grads[k], g))
    assert worst_l2 < 5e-3 and worst_max < 5e-2, (worst_l2, worst_max)
    # the classes no positive ROI has get exact zeros
    used = set(np.unique(ref["target_class_ids"][ref["target_class_ids"] > 0]).tolist())
    absent = [k for k in range(NC) if k not in used]
    gk = grads["myolo_mask/kernel"].reshape(-1, NC)
    assert np.all(gk[:, absent] == 0) and np.all(grads["myolo_mask/bias"][absent] == 0)
    assert all(np.abs(gk[:, k]).max() > 0 for k in used)


# ---------------------------------------------------------------------------------------------------------------- 6: the training step
@pytest.mark.parametrize("base", [ShapesConfig, ShapesHeadConfig], ids=["nbox3", "nbox5"])
def test_train_step_81_classes_matches_oracle(base):
    """Shapes 128x128, alpha 0.5, batch 4, NUM_CLASSES 81 (YOLO head output 3 * 86 = 258 / 5 * 86 = 430 channels): integer outputs
    bit-exact, activations / losses / gradients within test_gpu_step's bounds; two steps give the same bits"""
    cfg, P, batch, ref = many_class_case(base, seed=0 if base is ShapesConfig else 1, need_pos=2 if base is ShapesConfig else 1)
    assert cfg.N_BOX * (5 + NC) in (258, 430)
    rows = compare_step(cfg, P, batch, ref)
    bad = [r for r in rows if r[1] > TOL]
    assert not bad, bad
    outs, grads = [], []
    for _ in range(2):
        model = MaskYOLO(mode="training", config=cfg)
        model.load_state_dict(P)
        outs.append(model.train_on_batch(batch, learning_rate=0.0))
        grads.append(model.net.grads_dict())
    assert outs[0]["myolo_mask"].shape[-1] == NC
    assert outs[0]["loss"] == outs[1]["loss"] and np.array_equal(outs[0]["myolo_mask"], outs[1]["myolo_mask"])
    for k in grads[0]:
        assert np.array_equal(grads[0][k], grads[1][k]), k


def test_sparse_and_positives_only_paths_at_81_classes():
    """the sparse backward equals the dense one, and the positives-only forward the full one on the positives (to the bounds of
    test_gpu_step's tests of the same eliminations: fp32 summation-order noise plus at most a ReLU flip)"""
    cfg, P, batch, ref = many_class_case()
    res = []
    for sparse, rois in ((False, "all"), (True, "all"), (True, "positives")):
        c = _cfg(TRAIN_MASK_HEAD_ROIS=rois)
        model = MaskYOLO(mode="training", config=c)
        model.load_state_dict(P)
        model.net.sparse_mask_bwd = sparse
        out = model.train_on_batch(batch, learning_rate=0.0)
        res.append((out, model.net.grads_dict()))
    (od, gd), (os_, gs), (op, gp) = res
    for k in ("yolo_sum_loss", "mask_loss", "loss"):
        assert abs(od[k] - os_[k]) <= 1e-6 * max(1.0, abs(od[k])) and abs(od[k] - op[k]) <= 1e-6 * max(1.0, abs(od[k])), k
    R = od["myolo_mask"].shape[1]
    pos = np.concatenate([np.arange(b * R, b * R + n) for b, n in enumerate(od["n_pos"])])
    full = od["myolo_mask"].reshape((-1,) + od["myolo_mask"].shape[2:])
    assert op["myolo_mask"].shape == (len(pos),) + full.shape[1:] and full.shape[-1] == NC
    assert np.abs(op["myolo_mask"] - full[pos]).max() < 1e-5
    for g in (gs, gp):
        worst = 0.0
        for k in gd:
            if np.abs(gd[k]).max() < 1e-12 or k == "myolo_mask_conv1/bias":
                continue
            worst = max(worst, rel(g[k], gd[k]))
        assert worst < 3e-2, worst
    assert np.array_equal(gs["myolo_mask/kernel"] == 0, gd["myolo_mask/kernel"] == 0) and np.array_equal(gp["myolo_mask/kernel"] == 0, gd["myolo_mask/kernel"] == 0)


# ---------------------------------------------------------------------------------------------------------------- 7: inference
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_inference_81_classes(dtype):
    """predict keeps all 81 channels; detect_many (hipGraph replay) equals predict_graphed + unmold image by image and detect() in shapes"""
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=2, NUM_CLASSES=NC, LABELS=_labels(NC),
                      INFERENCE_DTYPE=dtype)
    m = MaskYOLO(mode="inference", config=cfg, seed=4)
    rng = np.random.default_rng(5)
    imgs = [(rng.random((128, 128, 3)) * 255).astype(np.uint8) for _ in range(3)]
    x = np.stack(imgs[:2]).astype(np.float32) / 255.
    yo, det, mask = m.keras_model.predict([x])
    R = cfg.GRID_H * cfg.GRID_W * cfg.N_BOX
    assert yo.shape[-1] == 5 + NC and det.shape == (2, R, 6) and mask.shape == (2, R, 28, 28, NC)
    assert np.isfinite(mask).all()
    many = m.detect_many(imgs, cs_threshold=0.0)
    assert len(many) == 3 and sum(r["full_masks"].shape[2] for r in many) >= 1
    for k in (0, 2):
        xx = torch.as_tensor(np.ascontiguousarray((np.stack([imgs[k]] * 2) / 255.).astype(np.float32)), device=m.net.dev)
        _, det_d, mask_d = m.net.predict_graphed(xx)
        one = m._select_and_unmold(det_d[0], mask_d[0], imgs[k].shape, 0.0)
        for key in ("bboxes", "class_ids", "confidence_scores", "full_masks"):
            assert np.array_equal(one[key], many[k][key]), (k, key)
    d0 = m.detect(imgs[0], cs_threshold=0.0)[0]
    assert d0["full_masks"].shape[:2] == (128, 128) and d0["full_masks"].shape[2] == len(d0["class_ids"])


def test_unmold_picks_the_detected_class_channel_at_81_classes():
    """myolo_unmold_masks at 81 classes: each detection's mask is the channel of its class (all other channels are zero)"""
    X = _X()
    N, C, H, W = 3, NC, 96, 80
    cls = [17, 45, 80]
    masks = torch.zeros(N, 28, 28, C, device="cuda")
    for i, c in enumerate(cls):
        masks[i, :, :, c] = 1.0
    det = torch.tensor([[0.1, 0.1, 0.5, 0.6, 0.9, cls[0]], [0.4, 0.3, 0.9, 0.8, 0.8, cls[1]], [0.0, 0.5, 0.3, 1.0, 0.7, cls[2]]],
                       dtype=torch.float32, device="cuda")
    full = torch.zeros(H, W, N, dtype=torch.uint8, device="cuda")
    ws = _ws(1 << 16)
    X.call("myolo_unmold_masks", X.ptr(masks), X.ptr(det), X.ptr(full), N, 28, 28, C, H, W, X.ptr(ws), ws.numel(), X.stream())
    torch.cuda.synchronize()
    f = full.cpu().numpy()
    for i in range(N):
        assert f[..., i].sum() > 0.5 * (det[i, 2] - det[i, 0]).item() * W * (det[i, 3] - det[i, 1]).item() * H, i


# ---------------------------------------------------------------------------------------------------------------- 8: C <= 8 unchanged
def test_four_class_step_still_uses_the_dense_mask_kernels():
    """Shapes C = 4, dense backward (the unfused deconv + 1x1 forward): the step's myolo_mask is myolo_mask_head_out_fwd of the taped
    deconv output, and its myolo_mask gradients are myolo_mask_head_out_bwd's on the dense dz of myolo_mask_bce, bit for bit"""
    from myolo.engine import MASK_DENSE_MAX_CLASSES
    X = _X()
    cfg, P, batch, ref = make_case(ShapesConfig, 128, 0.5, 4)
    assert cfg.NUM_CLASSES == 4 <= MASK_DENSE_MAX_CLASSES and ref["n_pos"].sum() > 0
    model = MaskYOLO(mode="training", config=cfg)
    model.load_state_dict(P)
    net = model.net
    net.sparse_mask_bwd = False
    cap = {}

    def hook(n):
        cap["d"] = n.tape["mask"].deconv.t.detach().clone()
    net.tape_hook = hook
    out = model.train_on_batch(batch, learning_rate=0.0)
    grads = net.grads_dict()
    d = cap["d"]
    C = 4
    w = torch.as_tensor(P["myolo_mask/kernel"], device="cuda").contiguous()
    b = torch.as_tensor(P["myolo_mask/bias"], device="cuda").contiguous()
    p = _fwd(d, w, b, C)
    assert np.array_equal(p.cpu().numpy().reshape(out["myolo_mask"].shape), out["myolo_mask"])
    tm = torch.as_tensor(out["target_mask"], device="cuda").contiguous()
    tc = torch.as_tensor(out["target_class_ids"].astype(np.int32), device="cuda").contiguous()
    w2 = float(cfg.LOSS_WEIGHTS.get("myolo_mask_loss", 1.))
    terms = torch.empty(2, device="cuda")
    dz = torch.empty(p.shape[0], C, device="cuda")
    ws = _ws(256 << 20)
    X.call("myolo_mask_bce", X.ptr(tm), X.ptr(tc), X.ptr(p), w2, X.ptr(terms), X.ptr(dz), tc.numel(), 28, 28, C, X.ptr(ws), ws.numel(), X.stream())
    _, dw, db = _bwd_dense(d, w, dz, C)
    gk = grads["myolo_mask/kernel"].reshape(-1, C)
    assert np.abs(gk).max() > 0
    assert np.array_equal(dw.cpu().numpy(), gk) and np.array_equal(db.cpu().numpy(), grads["myolo_mask/bias"])

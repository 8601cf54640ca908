"""ResNet-50 backbone (cfg.BACKBONE = "resnet50"): the new operators against float64 (conv1 7x7/s2, the max-pool, the stride-2 gather /
scatter, the residual join), and the training step / inference forward against a float64 autograd oracle -- oracle.torch_ref.TorchRef with
its trunk restated as keras_applications ResNet50 v1 (the reference builds no ResNet graph of its own: model.py:62 asserts mobilenet)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from oracle import np_ops as O                                         # noqa: E402
from oracle.torch_ref import TorchRef, _t, _conv, _bn                   # noqa: E402
from myolo import _ext as X                                            # noqa: E402
from myolo.config import make_config, ShapesConfig                     # noqa: E402
from myolo.engine import RESNET_STAGES, RESNET_C4_STAGE, resnet_block_names, init_state_dict   # noqa: E402
from myolo.model import MaskYOLO                                       # noqa: E402
from myolo.shapes import make_shapes_samples                           # noqa: E402
from myolo.myolo_utils import BatchGenerator                           # noqa: E402
from test_gpu_step import TOL, rel, decision_margins                   # noqa: E402

DEV = "cuda"
REMAP = {1: 17, 2: 45, 3: 80}


_KEEP = []


@pytest.fixture(autouse=True)
def _keepalive():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dt(a):
    """device copy, kept alive until the test ends (a temporary handed to X.call as a raw pointer would go back to the allocator at once)"""
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    _KEEP.append(t)
    return t


def ws(nbytes):
    buf = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr(), buf.numel()


def maxnorm(got, ref):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2)


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


# ------------------------------------------------------------------------------------------------ operators
def _stem_ref(x, w, b):
    return Fn.conv2d(Fn.pad(nchw(x), (3, 3, 3, 3)), torch.from_numpy(w.astype(np.float64)).permute(3, 2, 0, 1),
                     bias=torch.from_numpy(b.astype(np.float64)), stride=2)


@pytest.mark.parametrize("fp32_matmul", ["bf16x6", "native"])
@pytest.mark.parametrize("N,H,W", [(2, 33, 37), (1, 64, 64), (3, 128, 96), (2, 512, 512)])
def test_conv7x7s2_forward_and_weight_gradient(N, H, W, fp32_matmul):
    rng = np.random.default_rng(1)
    Co = 64
    x = rng.random((N, H, W, 3), dtype=np.float32)
    w = (rng.standard_normal((7, 7, 3, Co)) * 0.1).astype(np.float32)
    b = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    with X.option("wino_x6", 1 if fp32_matmul == "bf16x6" else 0):
        _buf, p, n = ws(X.conv7x7s2_ws_bytes(N, H, W, Co))
        y = torch.empty(N, Ho, Wo, Co, device=DEV)
        X.call("myolo_conv7x7s2_c3_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(b)), X.ptr(y), N, H, W, Co, p, n, X.stream())
        wt = torch.from_numpy(w.astype(np.float64)).requires_grad_(True)
        ref = Fn.conv2d(Fn.pad(nchw(x), (3, 3, 3, 3)), wt.permute(3, 2, 0, 1), bias=torch.from_numpy(b.astype(np.float64)), stride=2)
        assert maxnorm(y, nhwc(ref)) < TOL
        dy = (rng.standard_normal((N, Ho, Wo, Co))).astype(np.float32)
        dw, db = torch.empty(7, 7, 3, Co, device=DEV), torch.empty(Co, device=DEV)
        X.call("myolo_conv7x7s2_c3_bwd_weight", X.ptr(dt(x)), X.ptr(dt(dy)), X.ptr(dw), X.ptr(db), N, H, W, Co, p, n, X.stream())
        (ref * nchw(dy)).sum().backward()
        assert maxnorm(dw, wt.grad.numpy()) < TOL
        assert maxnorm(db, dy.astype(np.float64).sum((0, 1, 2))) < TOL
        # training form: batch statistics of y (the bias included) from the GEMM's epilogue, as myolo_bn_stats gives them on y itself
        r = ref.detach()
        mean, var = r.mean((0, 2, 3)).numpy(), r.var((0, 2, 3), unbiased=False).numpy()
        g = (1 + rng.random(Co)).astype(np.float32)
        be = (rng.standard_normal(Co) * 0.1).astype(np.float32)
        stats = [torch.zeros(Co, device=DEV) for _ in range(4)]
        mov = [dt(np.zeros(Co, np.float32)), dt(np.ones(Co, np.float32))]
        y2 = torch.empty(N, Ho, Wo, Co, device=DEV)
        X.call("myolo_conv7x7s2_c3_bnstats_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(b)), X.ptr(y2), X.ptr(dt(g)), X.ptr(dt(be)),
               *[X.ptr(t) for t in stats], *[X.ptr(t) for t in mov], N, H, W, Co, p, n, X.stream())
        assert maxnorm(y2, nhwc(r)) < TOL
        assert maxnorm(stats[0], mean) < TOL and maxnorm(stats[1], var) < TOL
        sc_ref = g / np.sqrt(var + 1e-3)
        assert maxnorm(stats[2], sc_ref) < TOL and maxnorm(stats[3], be - mean * sc_ref) < TOL
        assert maxnorm(mov[0], 0.01 * mean) < TOL
        # inference form: ReLU((conv + bias) * scale + shift) in the GEMM's store
        y3 = torch.empty(N, Ho, Wo, Co, device=DEV)
        X.call("myolo_conv7x7s2_c3_affine_act_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(b)), X.ptr(dt(g)), X.ptr(dt(be)), 1, X.ptr(y3),
               N, H, W, Co, p, n, X.stream())
        assert maxnorm(y3, np.maximum(nhwc(r) * g + be, 0)) < TOL
        torch.cuda.synchronize()


def test_conv7x7s2_adjointness_at_full_size():
    """<Y, f(X, W)> = <W, f_bwd_weight(X, Y)> at the BASELINE configs[4] stem (16 x 512 x 512 -> 256 x 256 x 64), bias 0"""
    N, H, W, Co = 16, 512, 512, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.rand(N, H, W, 3, device=DEV, generator=g)
    w = torch.randn(7, 7, 3, Co, device=DEV, generator=g) * 0.1
    yb = torch.randn(N, 256, 256, Co, device=DEV, generator=g)
    zero = torch.zeros(Co, device=DEV)
    _buf, p, n = ws(X.conv7x7s2_ws_bytes(N, H, W, Co))
    y = torch.empty(N, 256, 256, Co, device=DEV)
    X.call("myolo_conv7x7s2_c3_fwd", X.ptr(x), X.ptr(w), X.ptr(zero), X.ptr(y), N, H, W, Co, p, n, X.stream())
    dw = torch.empty(7, 7, 3, Co, device=DEV)
    X.call("myolo_conv7x7s2_c3_bwd_weight", X.ptr(x), X.ptr(yb), X.ptr(dw), None, N, H, W, Co, p, n, X.stream())
    lhs = float((yb.double() * y.double()).sum())
    rhs = float((w.double() * dw.double()).sum())
    scale = float((yb.double().abs() * y.double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)


def _pool_ref(a):
    """ZeroPadding2D(1) + MaxPool2D 3x3/s2 in float64 autograd (first maximum wins, as the kernel's argmax)"""
    t = nchw(a).requires_grad_(True)
    return t, Fn.max_pool2d(Fn.pad(t, (1, 1, 1, 1)), 3, 2)


@pytest.mark.parametrize("N,H,W,C,affine", [(2, 16, 16, 64, False), (1, 15, 17, 8, False), (2, 256, 256, 64, True), (1, 9, 11, 4, True)])
def test_maxpool_forward_backward(N, H, W, C, affine):
    rng = np.random.default_rng(2)
    x = rng.integers(-6, 6, size=(N, H, W, C)).astype(np.float32) / 4         # many exact ties
    x[0, :4, :4, :] = -1.0                                                     # all-negative windows: the padding (0) wins at the corner
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if affine:      # bn_conv1's apply + ReLU on the pool's load: scale / shift powers of two keep the fp32 activations exact
        sc = (2.0 ** rng.integers(-1, 2, size=C)).astype(np.float32)
        sh = (rng.integers(-2, 3, size=C) / 4).astype(np.float32)
        act = np.maximum(x * sc + sh, 0).astype(np.float32)
        args = (X.ptr(dt(sc)), X.ptr(dt(sh)), 1)
    else:
        act = x
        args = (None, None, 0)
    y = torch.empty(N, Ho, Wo, C, device=DEV)
    arg = torch.empty(N, Ho, Wo, C, dtype=torch.uint8, device=DEV)
    X.call("myolo_maxpool3x3s2_fwd", X.ptr(dt(x)), *args, X.ptr(y), X.ptr(arg), N, H, W, C, X.stream())
    t, ref = _pool_ref(act)
    assert np.array_equal(y.cpu().numpy(), nhwc(ref).astype(np.float32))
    a = arg.cpu().numpy()
    assert a.max() <= 8
    # the argmax is the FIRST maximum of the zero-padded window in row-major order
    pad = np.pad(act, ((0, 0), (1, 1), (1, 1), (0, 0)))
    win = np.stack([pad[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :] for kh in range(3) for kw in range(3)], 0)
    assert np.array_equal(a, np.argmax(win, 0))
    if not affine:
        assert (a[0, 0, 0, :] == 0).all()          # the padding cell wins the all-negative corner window
    dy = rng.standard_normal((N, Ho, Wo, C)).astype(np.float32)
    dx = torch.empty(N, H, W, C, device=DEV)
    X.call("myolo_maxpool3x3s2_bwd", X.ptr(dt(dy)), X.ptr(arg), X.ptr(dx), N, H, W, C, X.stream())
    (ref * nchw(dy)).sum().backward()
    assert maxnorm(dx, nhwc(t.grad)) < TOL


@pytest.mark.parametrize("N,H,W,C", [(2, 16, 16, 256), (1, 9, 7, 64), (2, 64, 64, 512)])
def test_gather_and_scatter_s2(N, H, W, C):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xs = torch.empty(N, Ho, Wo, C, device=DEV)
    X.call("myolo_gather_s2", X.ptr(dt(x)), X.ptr(xs), N, H, W, C, X.stream())
    assert np.array_equal(xs.cpu().numpy(), x[:, ::2, ::2, :])
    a = rng.standard_normal((N, Ho, Wo, C)).astype(np.float32)
    b = rng.standard_normal((N, Ho, Wo, C)).astype(np.float32)
    for bb in (b, None):
        dx = torch.full((N, H, W, C), float("nan"), device=DEV)
        X.call("myolo_scatter_s2", X.ptr(dt(a)), None if bb is None else X.ptr(dt(bb)), X.ptr(dx), N, H, W, C, X.stream())
        ref = np.zeros((N, H, W, C), np.float32)
        ref[:, ::2, ::2, :] = a if bb is None else a + bb
        assert np.array_equal(dx.cpu().numpy(), ref)
    # the adjoint of the strided 1x1 conv's gather, as a float64 autograd pins it
    t = nchw(x).requires_grad_(True)
    (Fn.conv2d(t, torch.eye(C, dtype=torch.float64).view(C, C, 1, 1), stride=2) * nchw(a)).sum().backward()
    dx = torch.empty(N, H, W, C, device=DEV)
    X.call("myolo_scatter_s2", X.ptr(dt(a)), None, X.ptr(dx), N, H, W, C, X.stream())
    assert maxnorm(dx, nhwc(t.grad)) < TOL


@pytest.mark.parametrize("M,C,proj", [(512, 256, False), (512, 256, True), (4099, 64, True), (128, 2048, False)])
def test_residual_join(M, C, proj):
    rng = np.random.default_rng(4)
    y, sc = rng.standard_normal((M, C)).astype(np.float32), rng.standard_normal((M, C)).astype(np.float32)
    s, t = rng.random(C).astype(np.float32) + 0.5, rng.standard_normal(C).astype(np.float32) * 0.3
    s1, t1 = rng.random(C).astype(np.float32) + 0.5, rng.standard_normal(C).astype(np.float32) * 0.3
    out = torch.empty(M, C, device=DEV)
    X.call("myolo_residual_fwd", X.ptr(dt(y)), X.ptr(dt(s)), X.ptr(dt(t)), X.ptr(dt(sc)), X.ptr(dt(s1)) if proj else None,
           X.ptr(dt(t1)) if proj else None, X.ptr(out), M, C, X.stream())
    yt = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
    st = torch.from_numpy(sc.astype(np.float64)).requires_grad_(True)
    r = st * torch.from_numpy(s1.astype(np.float64)) + torch.from_numpy(t1.astype(np.float64)) if proj else st
    ref = torch.relu(yt * torch.from_numpy(s.astype(np.float64)) + torch.from_numpy(t.astype(np.float64)) + r)
    assert maxnorm(out, ref.detach().numpy()) < TOL
    dout = rng.standard_normal((M, C)).astype(np.float32)
    g = torch.empty(M, C, device=DEV)
    X.call("myolo_residual_bwd", X.ptr(dt(dout)), X.ptr(out), X.ptr(g), M * C, X.stream())
    # g = dout * [out > 0]: the gradient of the pre-activation sum, i.e. of y*s + t and of the shortcut term
    (ref * torch.from_numpy(dout.astype(np.float64))).sum().backward()
    assert maxnorm(g * dt(s), yt.grad.numpy()) < TOL
    assert maxnorm(g * dt(s1) if proj else g, st.grad.numpy()) < TOL


# ------------------------------------------------------------------------------------------------ the net against the oracle
class ResNetRef(TorchRef):
    """TorchRef with keras_applications ResNet50 v1 as its trunk (float64 autograd); the heads, losses and targets are TorchRef's.
    self.bn_batch: BatchNorm name -> (batch mean, biased variance, rows) of the last training forward (moving-statistics check).
    forced: {ReLU name: 0/1 mask (NHWC), "pool": argmax (NHWC)} -- the trunk's activation decisions taken as given (the GPU's, see
    gpu_decisions) instead of re-taken on the float64 values; without it every ReLU and the max-pool decide for themselves."""

    def __init__(self, P_np, cfg, forced=None, **kw):
        super().__init__(P_np, cfg, **kw)
        self.forced = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (forced or {}).items()}

    def _relu(self, name, x):
        m = self.forced.get(name)
        return torch.relu(x) if m is None else x * m.permute(0, 3, 1, 2).to(x.dtype)

    def _pool(self, x):
        xp = Fn.pad(x, (1, 1, 1, 1))
        a = self.forced.get("pool")
        if a is None:
            return Fn.max_pool2d(xp, 3, 2)
        Ho, Wo = a.shape[1], a.shape[2]
        win = torch.stack([xp[:, :, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2] for kh in range(3) for kw in range(3)], 0)
        return win.gather(0, a.permute(0, 3, 1, 2).long().unsqueeze(0)).squeeze(0)

    def _bnl(self, name, x, train):
        P = self.P
        if train:
            with torch.no_grad():
                self.bn_batch[name] = (x.mean((0, 2, 3)).numpy(), x.var((0, 2, 3), unbiased=False).numpy(), x.numel() // x.shape[1])
        return _bn(x, P[name + "/gamma"], P[name + "/beta"], P[name + "/moving_mean"], P[name + "/moving_variance"], train)

    def _bottleneck(self, x, st, b, stride, train):
        P = self.P
        cb, bb = resnet_block_names(st, b)
        y = self._relu(cb + "2a", self._bnl(bb + "2a", _conv(x, P[cb + "2a/kernel"], stride=stride, bias=P[cb + "2a/bias"]), train))
        y = self._relu(cb + "2b", self._bnl(bb + "2b", _conv(y, P[cb + "2b/kernel"], pad=(1, 1, 1, 1), bias=P[cb + "2b/bias"]), train))
        y = self._bnl(bb + "2c", _conv(y, P[cb + "2c/kernel"], bias=P[cb + "2c/bias"]), train)
        sc = self._bnl(bb + "1", _conv(x, P[cb + "1/kernel"], stride=stride, bias=P[cb + "1/bias"]), train) if b == "a" else x
        return self._relu(cb + "out", y + sc)

    def trunk(self, images, train):
        P, cfg = self.P, self.cfg
        self.bn_batch = {}
        x = _t(images, self.dtype).permute(0, 3, 1, 2)
        x = _conv(x, P["conv1/kernel"], stride=2, pad=(3, 3, 3, 3), bias=P["conv1/bias"])
        x = self._pool(self._relu("bn_conv1", self._bnl("bn_conv1", x, train)))
        for st, blocks, _, stride in RESNET_STAGES:
            for i, b in enumerate(blocks):
                x = self._bottleneck(x, st, b, stride if i == 0 else 1, train)
            if st == RESNET_C4_STAGE:
                C4 = x
                Fm = _conv(C4, P["feature_map/kernel"], pad=(1, 1, 1, 1), bias=P["feature_map/bias"])
        y = _conv(x, P["conv_23/kernel"], bias=P["conv_23/bias"])
        B = y.shape[0]
        return C4, Fm, y.permute(0, 2, 3, 1).reshape(B, cfg.GRID_H, cfg.GRID_W, cfg.N_BOX, 5 + cfg.NUM_CLASSES)


def gpu_decisions(net):
    """the activation decisions of the Net's last training forward: every trunk ReLU's mask and the max-pool's argmax, NHWC (for ResNetRef)"""
    t, out = net.tape, {}
    y0, _, _ = t["bn_conv1"]
    images, (N, Hs, Ws, C0), arg = t["stem"]
    buf = net.bnbuf["bn_conv1"]
    out["bn_conv1"] = ((y0 * buf[2]) + buf[3] > 0).reshape(N, Hs, Ws, C0).cpu().numpy()      # the pool's load: product and sum rounded apart
    out["pool"] = arg.reshape(N, (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1, C0).cpu().numpy()
    for st, blocks, _, _ in RESNET_STAGES:
        for b in blocks:
            cb, _ = resnet_block_names(st, b)
            shape, stride, xs, a2a, a2b, o = t[cb]
            n, h, w = shape[0], shape[1], shape[2]
            if stride == 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            for key, v in (("2a", a2a), ("2b", a2b), ("out", o)):
                out[cb + key] = (v > 0).reshape(n, h, w, -1).cpu().numpy()
    return out


def _cfg(nc, B=2, size=128, **kw):
    labels = ["background"] + ["class%d" % i for i in range(1, nc)]
    return make_config(ShapesConfig, BACKBONE="resnet50", IMAGE_SHAPE=[size, size, 3], BATCH_SIZE=B, NUM_CLASSES=nc, LABELS=labels, **kw)


def _params(cfg, seed):
    """the Keras initialisation, with non-zero biases, BN affines and moving statistics so that every term is exercised"""
    P = init_state_dict(cfg, seed=seed)
    rng = np.random.default_rng(seed + 100)
    for k, v in P.items():
        if k.endswith("/bias") or k.endswith("/beta") or k.endswith("/moving_mean"):
            P[k] = (rng.standard_normal(v.shape) * 0.05).astype(np.float32)
        elif k.endswith("/gamma") or k.endswith("/moving_variance"):
            P[k] = (1 + np.abs(rng.standard_normal(v.shape)) * 0.05).astype(np.float32)
    # res5c's output (a sum of 16 residual branches over 2048 channels) puts a glorot conv_23 at |yolo_output| ~ 10, where exp(w, h) leaves no
    # proposal near a ground-truth box: scaled down, as a trained head would be, so that the step has positive ROIs
    P["conv_23/kernel"] *= np.float32(0.05)
    return P


_CASES = {}


def resnet_case(nc, seed=0, need_pos=2, min_margin=1e-3, min_roi_px=4e-3, size=128, batch=2, oracle=None):
    """first seeded Shapes batch (class ids remapped into 1..80 at nc = 81) with positives and safe decision margins (test_gpu_step._make_case)
    -> (cfg, P, batch, unforced oracle's results).  size, batch: image side and images per step.  oracle(ref, batch): what to run on the screened
    batch instead of the whole unforced train_step (the full-size tests take a forward only: tests/test_gpu_resnet50_fullsize.py)."""
    key = (nc, size, batch)
    if key in _CASES:
        return _CASES[key]
    cfg = _cfg(nc, B=batch, size=size)
    P = _params(cfg, seed)
    B = cfg.BATCH_SIZE
    for start in range(0, 200 * B, B):
        samples = make_shapes_samples(B, cfg, start_index=start)
        if nc > 4:
            for s in samples:
                s[1] = np.asarray([REMAP[int(c)] for c in s[1]], dtype=np.asarray(s[1]).dtype)
        batch, _ = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0]
        ref = ResNetRef(P, cfg)
        with torch.no_grad():
            C4, Fm, yo = ref.trunk(batch[0], True)
        yo = yo.numpy().astype(np.float32)
        prop = O.yolo_decode(yo, cfg.ANCHORS, cfg.GRID_W)
        rois, tcls, tmask, npos = O.mask_targets(prop, batch[3], batch[4], batch[5], cfg)
        if npos.sum() < need_pos:
            continue
        mg = decision_margins(cfg, batch, yo, prop, rois, Fm.shape[2])
        if min(mg["partition"], mg["noobj"]) > min_margin and mg["roi_px"] > min_roi_px:
            out = ref.train_step(batch) if oracle is None else oracle(ref, batch)
            out.update(target_mask=tmask, n_pos=npos, bn_batch=dict(ref.bn_batch))
            _CASES[key] = (cfg, P, batch, out)
            return _CASES[key]
    raise RuntimeError("no batch with positive ROIs and safe decision margins found")


def _bn_of_bias(k):
    """the training-mode BatchNorm a trunk conv's bias feeds (conv1 -> bn_conv1, res3a_branch2b -> bn3a_branch2b), else None"""
    layer = k.split("/")[0]
    if layer == "conv1":
        return "bn_conv1"
    return "bn" + layer[3:] if layer.startswith("res") else None


def step_against_oracle(case, fp32_matmul, forced_oracle=lambda P, cfg, seen, batch, out: ResNetRef(P, cfg, forced=seen).train_step(batch)):
    """one training step of the engine on `case` (resnet_case) against the float64 oracle run with the GPU's trunk decisions; forced_oracle(P, cfg,
    decisions, batch, the engine's results) runs that oracle.  -> {gradient key: relative L2 error}"""
    cfg, P, batch, screen = case
    cfg = make_config(type(cfg), FP32_MATMUL=fp32_matmul)
    model = MaskYOLO(mode="training", config=cfg)
    assert model.net.resnet and model.net.fp32_matmul == fp32_matmul
    model.load_state_dict(P)
    seen = {}
    model.net.tape_hook = lambda net: seen.update(gpu_decisions(net))
    out = model.train_on_batch(batch, learning_rate=0.0)
    grads = model.net.grads_dict()
    torch.cuda.synchronize()
    # the shared decisions differ from the oracle's own in a handful of elements at most
    ref = forced_oracle(P, cfg, seen, batch, out)
    assert np.array_equal(out["target_class_ids"], ref["target_class_ids"])
    assert np.array_equal(out["n_pos"], screen["n_pos"])
    assert np.array_equal(out["target_mask"], screen["target_mask"])
    assert np.array_equal(ref["target_class_ids"], screen["target_class_ids"])
    for k in ("yolo_output", "feature_map", "myolo_mask"):
        got = np.asarray(out[k]).reshape(np.shape(ref[k]))          # (the oracle's mask rows are [B*R, h, w, C])
        assert rel(got, ref[k]) < TOL, (k, rel(got, ref[k]))
        assert rel(got, screen[k]) < TOL, (k, "unforced oracle", rel(got, screen[k]))
    for k in ("yolo_sum_loss", "mask_loss", "loss"):
        assert abs(out[k] - ref[k]) / max(1.0, abs(ref[k])) < TOL, k
    assert set(ref["grads"]) == set(grads)
    worst = {}
    for k, g in ref["grads"].items():
        bn = _bn_of_bias(k) if k.endswith("/bias") else None
        if bn is not None:
            # a conv bias in front of a training-mode BatchNorm cancels in its output: the oracle's gradient (the column sum of the BatchNorm
            # input's gradient) is 0, the GPU's is that column sum in fp32 -- held to rounding against the size of the BatchNorm's own beta gradient
            assert np.abs(g).max() < 1e-9 * max(1.0, np.abs(ref["grads"][bn + "/beta"]).max()), k
            assert np.abs(grads[k]).max() <= 1e-3 * np.abs(ref["grads"][bn + "/beta"]).max(), (k, np.abs(grads[k]).max())
            continue
        if k == "myolo_mask_conv1/bias":
            continue          # the same cancellation in front of myolo_mask_bn1; its noise is the MobileNet path's (test_gpu_step.compare_step)
        worst[k] = float(np.linalg.norm(grads[k].astype(np.float64) - g) / max(1e-30, np.linalg.norm(g)))
    bad = {k: e for k, e in worst.items() if e > 0.02}
    assert not bad, bad
    # the trunk, where no mask-head branch decision is left to move anything (the shared decisions cover all of its own)
    trunk = {k: e for k, e in worst.items() if not (k.startswith("myolo_mask") or k.startswith("feature_map"))}
    assert max(trunk.values()) < 0.02, max(trunk.items(), key=lambda kv: kv[1])
    return worst


@pytest.mark.parametrize("fp32_matmul", ["bf16x6", "native"])
@pytest.mark.parametrize("nc", [4, 81])
def test_train_step_matches_oracle(nc, fp32_matmul):
    """One step against the float64 oracle.  The oracle takes the trunk's activation decisions (ReLU masks, max-pool argmax) from the GPU's
    forward: every ReLU is a hard branch on an activation with ~1e-5 fp32 noise, and at 128^2 stage 5 normalises 32 rows per channel, so a
    single branch taken the other way behind one BatchNorm moves every gradient below it by a few percent (measured: 1.5-2.9 % relative L2 from
    one flip behind bn5c_branch2a).  Screening the case for trunk margins is no way out: stages 4-5 alone hold ~1.5 M pre-ReLU values, ~10 of
    them within fp32 noise of 0 in any batch.  With the decisions shared, the backward's arithmetic is held to the 2 % bound."""
    step_against_oracle(resnet_case(nc), fp32_matmul)


def test_adam_update_and_moving_statistics_match_oracle():
    cfg, P, batch, ref = resnet_case(4)
    model = MaskYOLO(mode="training", config=cfg)
    model.load_state_dict(P)
    model.train_on_batch(batch, learning_rate=1e-3)
    sd = model.state_dict()
    from oracle import np_model
    # Keras Adam on the step's own gradients (their agreement with the oracle is test_train_step_matches_oracle's; Adam's first step is
    # lr * sign(g), which a ReLU flip turns for entries near 0)
    G = model.net.grads_dict()
    P2, _ = np_model.adam_update({k: v.copy() for k, v in P.items()}, {k: G[k].astype(np.float64) for k in ref["grads"]}, {}, 1, 1e-3)
    worst = max(float(np.abs(sd[k] - P2[k]).max()) for k in ref["grads"])
    assert worst < 2e-6, worst
    # every trunk BatchNorm: batch mean (the conv bias included) and the Keras / TF moving-variance update
    assert len(ref["bn_batch"]) == 53
    for name, (mean, var, n) in ref["bn_batch"].items():
        mm, mv = O.bn_moving_update(P[name + "/moving_mean"], P[name + "/moving_variance"], mean.astype(np.float32), var.astype(np.float32), n)
        assert np.abs(sd[name + "/moving_mean"] - mm).max() < 1e-4 * max(1.0, np.abs(mm).max()), name
        assert rel(sd[name + "/moving_variance"], mv) < 1e-4, name


@pytest.mark.parametrize("early", [-1, 1])
def test_two_runs_bit_identical(early):
    """determinism, also with the YOLO branch's backward launched early on its side stream, under the mask head's forward (yolo_bwd_early = 1):
    its tensors come from the compute stream's forward and must stay alive while that stream allocates for the mask head"""
    cfg, P, batch, _ = resnet_case(4)
    outs, gs = [], []
    for _ in range(2):
        model = MaskYOLO(mode="training", config=cfg)
        model.net.yolo_bwd_early = early
        model.load_state_dict(P)
        outs.append(model.train_on_batch(batch, learning_rate=0.0))
        gs.append(model.net.flat_g.clone())
    assert outs[0]["loss"] == outs[1]["loss"]
    assert np.array_equal(outs[0]["yolo_output"], outs[1]["yolo_output"])
    assert torch.equal(gs[0], gs[1])


def _infer_model(B=2, **kw):
    cfg = _cfg(4, B=B, **kw)
    model = MaskYOLO(mode="inference", config=cfg)
    model.load_state_dict(_params(cfg, 5))
    return cfg, model


def test_inference_forward_matches_oracle():
    cfg, model = _infer_model()
    samples = make_shapes_samples(2, cfg)
    images = np.stack([s[0] for s in samples]).astype(np.float32) / 255.
    yo, det, mask = model.keras_model.predict([images])
    ref = ResNetRef(model.state_dict(), cfg)
    with torch.no_grad():
        C4, Fm, ryo = ref.trunk(images, False)
        assert rel(yo, ryo.numpy()) < TOL
        rdet = O.yolo_detections(ryo.numpy().astype(np.float32), cfg.ANCHORS, cfg.GRID_W)
        assert np.array_equal(det[..., 5], rdet[..., 5]), "class ids differ"
        assert rel(det[..., :5], rdet[..., :5]) < TOL
        pred = ref.mask_head(Fm, rdet[..., :4], False)
    assert rel(mask, pred.permute(0, 2, 3, 1).numpy().reshape(mask.shape)) < TOL


def test_inference_folded_frozen_bn_equals_unfolded():
    cfg, model = _infer_model()
    x = torch.as_tensor(np.random.default_rng(6).random((2, 128, 128, 3), dtype=np.float32), device=DEV)
    a = [t.clone() for t in model.net.predict(x)]
    model.net.fold_frozen_bn = False
    b = model.net.predict(x)
    # (bn_conv1 + ReLU in the conv's GEMM epilogue against the same affine on the max-pool's load: equal up to the epilogue's fma)
    assert rel(a[0].cpu().numpy(), b[0].cpu().numpy()) < 1e-5
    assert torch.equal(a[1][..., 5], b[1][..., 5]) and rel(a[1].cpu().numpy(), b[1].cpu().numpy()) < 1e-5
    assert rel(a[2].cpu().numpy(), b[2].cpu().numpy()) < 1e-4


def test_inference_hip_graph_replay_equals_eager():
    cfg, model = _infer_model()
    net = model.net
    rng = np.random.default_rng(8)
    for _ in range(2):
        x = torch.as_tensor(rng.random((2, 128, 128, 3), dtype=np.float32), device=net.dev)
        g = [t.clone() for t in net.predict_graphed(x)]
        e = net.predict(x)
        assert all(torch.equal(u, v) for u, v in zip(g, e))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_detect_many_equals_detect_per_image(dtype):
    cfg, m = _infer_model(B=2, INFERENCE_DTYPE=dtype)
    rng = np.random.default_rng(3)
    imgs = [(rng.random((128, 128, 3)) * 255).astype(np.uint8) for _ in range(3)]
    many = m.detect_many(imgs, cs_threshold=0.0)
    assert len(many) == 3
    for k in range(3):
        x = torch.as_tensor(np.ascontiguousarray((np.stack([imgs[k]] * 2) / 255.).astype(np.float32)), device=m.net.dev)
        _, det_d, mask_d = m.net.predict_graphed(x)
        one = m._select_and_unmold(det_d[0], mask_d[0], imgs[k].shape, 0.0)
        for key in ("bboxes", "class_ids", "confidence_scores", "full_masks"):
            assert np.array_equal(one[key], many[k][key]), (k, key)
    res = m.detect(imgs[0], cs_threshold=0.0)
    assert set(res[0]) == {"bboxes", "class_ids", "confidence_scores", "full_masks"}

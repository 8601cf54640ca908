"""The ResNet-50 path at the size the engine ships at -- 6 images of 512 x 512, 81 classes, N_BOX 3 (resnet50_launches) -- where the library's row
counts pick other kernels than at test_gpu_resnet50's 2 x 128 x 128: Winograd F(4,3) on 128 x 128 and 64 x 64 maps, the thin data / weight
gradient kernels at 98 304 rows, pw_smallm_kernel<2> and the big-tile GEMMs in stage 4, K = 2048 in stage 5.

  test_census_*       the launches a real step / forward issues are exactly resnet50_launches.LAUNCHES (both directions, both FP32_MATMUL modes)
  test_launch_*       every row of that table as an operator case against float64, at the bounds the suite already holds the entry to
  test_train_step_full_size_matches_oracle    one step against the float64 autograd oracle with the engine's trunk decisions and ROIs
  test_full_size_*    the inference forward against the oracle, two steps bit-identical, graph replay equal to the eager forward

Cost of the oracle (FullSizeRef, float64 autograd on the CPU): with the whole mask head taped over 4 608 ROIs one train_step took 331 s and
64 GB on 8 cores.  FullSizeRef tapes the head only where a gradient flows; measured on the GPU host's 16 CPUs, test_train_step_full_size_
matches_oracle[bf16x6] -- screening, the unforced forward, the engine's step and one forced train_step -- takes 103 s in all with a peak
resident set of 47 GB."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

import resnet50_launches as L                                                      # noqa: E402
from oracle import np_ops as O                                                     # noqa: E402
from myolo import _ext as X                                                        # noqa: E402
from myolo.model import MaskYOLO                                                   # noqa: E402
from test_gpu_fp32_products import check_a, check_c, seq_matmul, errs, U24         # noqa: E402
from test_gpu_ops import TOL                                                       # noqa: E402
from oracle.torch_ref import _t, _conv, _bn, crop_and_resize_t, yolo_loss_t, mask_bce_t      # noqa: E402
from test_gpu_resnet50 import (ResNetRef, resnet_case, step_against_oracle, _cfg, _params, REMAP, nchw, nhwc, maxnorm)      # noqa: E402
from myolo.shapes import make_shapes_samples                                       # noqa: E402
from myolo.myolo_utils import BatchGenerator                                       # noqa: E402

DEV = "cuda"
MODES = ["bf16x6", "native"]
W43_TOL = 5e-5          # test_winograd_error_is_at_fp32_level's bound on the F(4,3) form (K = 9 * 256, the same operand statistics)

_KEEP = []


@pytest.fixture(autouse=True)
def _keepalive():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dt(a):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    _KEEP.append(t)
    return t


def new(*shape, dtype=torch.float32):
    t = torch.full(shape, float("nan") if dtype == torch.float32 else 0, dtype=dtype, device=DEV)
    _KEEP.append(t)
    return t


def wsbuf(nbytes=None):
    """(pointer, size) of a workspace of exactly nbytes -- what the size function the engine relies on returned, so that a size that is too small
    for the shape fails the call (MYOLO_NEED_WS) or misses its kernel; None: 768 MB, for the entries whose scratch the engine does not size"""
    need = (768 << 20) if nbytes is None else int(nbytes)
    if getattr(wsbuf, "buf", None) is None or wsbuf.buf.numel() < need:
        wsbuf.buf = None
        wsbuf.buf = torch.empty(max(need, 768 << 20), dtype=torch.uint8, device=DEV)
    return wsbuf.buf.data_ptr(), need


def mode_option(mode):
    return X.option("wino_x6", 1 if mode == "bf16x6" else 0)


# ------------------------------------------------------------------------------------------------ operands as in the network
def act_in(rng, *shape):
    """post-ReLU O(1) activations"""
    return np.maximum(rng.standard_normal(shape), 0).astype(np.float32)


def he(rng, *shape):
    """he-normal weights: std sqrt(2 / fan_in), fan_in = every axis but the last"""
    return (rng.standard_normal(shape) * np.sqrt(2.0 / np.prod(shape[:-1]))).astype(np.float32)


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def mm64(a, b):
    """float64 product on the CPU (torch: threaded)"""
    return (t64(a) @ t64(b)).numpy()


def seed_of(entry, args):
    return (sum(map(ord, entry)) * 7919 + hash(tuple(args))) % (1 << 31)


# ------------------------------------------------------------------------------------------------ 1. census
def _scene(size, B, mode):
    cfg = _cfg(L.NUM_CLASSES, B=B, size=size, FP32_MATMUL=mode)
    samples = make_shapes_samples(B, cfg, start_index=0)
    for s in samples:
        s[1] = np.asarray([REMAP[int(c)] for c in s[1]], dtype=np.asarray(s[1]).dtype)
    batch, _ = BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0]
    return cfg, _params(cfg, 0), batch


def _census(monkeypatch, size, B, mode):
    """{phase: set of (entry, integer arguments)} of one train_on_batch and one predict"""
    cfg, P, batch = _scene(size, B, mode)
    assert cfg.N_BOX == L.N_BOX
    out = {}
    for phase, mname in ((L.TRAIN, "training"), (L.INFER, "inference")):
        model = MaskYOLO(mode=mname, config=cfg)
        assert model.net.resnet and model.net.fp32_matmul == mode
        model.load_state_dict(P)
        seen = set()
        with L.recording(monkeypatch, model.net, seen):
            if phase == L.TRAIN:
                model.train_on_batch(batch, learning_rate=0.0)
            else:
                model.keras_model.predict([batch[0]])
        torch.cuda.synchronize()
        out[phase] = seen
        del model
    return out


@pytest.mark.parametrize("mode", MODES)
def test_census_full_size_launches_are_the_table(monkeypatch, mode):
    """every launch of the trunk at 6 x 512^2 is a row of resnet50_launches.LAUNCHES (a new shape in the engine fails here until it has an
    operator case below), and every row was launched (the table cannot rot)"""
    seen = _census(monkeypatch, L.SIZE, L.B, mode)
    for phase in (L.TRAIN, L.INFER):
        table = set(L.rows(phase))
        assert not seen[phase] - table, ("launched, not in the table", phase, sorted(seen[phase] - table))
        assert not table - seen[phase], ("in the table, never launched", phase, sorted(table - seen[phase]))


def test_census_small_step_does_not_reach_the_full_size_rows(monkeypatch, capsys):
    """what test_gpu_resnet50's 2 x 128^2 step launches against the table: other shapes throughout, and other ENTRIES for the 3x3 convs of stages
    2-3 and feature_map (direct at 128^2, Winograd F(4,3) at 512^2).  Printed once, for the record."""
    small = _census(monkeypatch, 128, 2, "bf16x6")
    table = set(L.rows())
    got = small[L.TRAIN] | small[L.INFER]
    assert not (got & table) - {("myolo_bn_frozen_coeffs_batched", (53,))}, "a 128^2 launch has a full-size shape"
    e_small, e_full = {e for e, _ in got}, {e for e, _ in table}
    with capsys.disabled():
        print("\n2 x 128^2 against 6 x 512^2: %d launches, none with a full-size shape (%d rows in the table)" % (len(got), len(table)))
        print("  entries only the full size reaches: %s" % sorted(e_full - e_small))
        print("  entries only the small step reaches: %s" % sorted(e_small - e_full))
        for e in ("myolo_conv3x3_fwd", "myolo_pwconv1x1_bwd_data", "myolo_bn_stats"):
            print("  %s: 128^2 %s | 512^2 %s" % (e, sorted(a for n, a in got if n == e), sorted(a for n, a in table if n == e)))
    assert {"myolo_wino_multiply_w", "myolo_conv3x3_wino_bwd_data", "myolo_conv3x3_wino_bwd_weight"} <= e_full - e_small


# ------------------------------------------------------------------------------------------------ 2. every row against float64
def _ids(rows):
    return ["%s-%s" % (e.replace("myolo_", ""), "x".join(map(str, a))) for e, a in rows]


def _rows_of(*entries):
    return [(e, a) for e, a in L.rows() if e in entries]


def _gemm_case(got_by_mode, ref, absdot, K, what, seq, extra=0.0):
    """(a) in both modes; (c) where the bf16x6 call did not run the native kernel (entry and shape decide that inside the library)"""
    for mode in MODES:
        w = check_a(got_by_mode[mode], ref, absdot, K, extra=extra, what="%s %s" % (what, mode))
        print("%s %s: worst err / componentwise bound %.3g" % (what, mode, w))
    if not torch.equal(got_by_mode["bf16x6"], got_by_mode["native"]):
        check_c(got_by_mode["bf16x6"], got_by_mode["native"], ref, what, seq=seq())
        return True
    return False


PW_ROWS = _rows_of("myolo_pwconv1x1_fwd", "myolo_pwconv1x1_bwd_data", "myolo_pwconv1x1_bwd_weight")


@pytest.mark.parametrize("entry,args", PW_ROWS, ids=_ids(PW_ROWS))
def test_launch_pointwise(entry, args):
    """the 1x1 convs with bias as the engine calls them (Net._rn_pw_fwd / _rn_pw_bwd_data / _rn_pw_wgrad): the componentwise fp32 bound of
    test_gpu_fp32_products (check_a; the bias adds one term to the dot product) in both modes, check_c where bf16x6 ran another kernel.
    The library sends the data gradient to the bf16x6 kernel for Cin % 256 == 0 (Cin not 32 / 64), the weight gradient for Cin % 256 == 0 and
    Cout % 256 == 0, both from 4096 rows: those rows must not be bit-identical to native."""
    M, Cin, Cout = args
    rng = np.random.default_rng(seed_of(entry, args))
    x, w, b, dy = act_in(rng, M, Cin), he(rng, Cin, Cout), rnd(rng, Cout, scale=0.1), rnd(rng, M, Cout)
    got = {}
    if entry == "myolo_pwconv1x1_fwd":
        ref, absdot, K = mm64(x, w) + b.astype(np.float64), mm64(np.abs(x), np.abs(w)) + np.abs(b).astype(np.float64), Cin + 1
        seq, want_x6 = (lambda: seq_matmul(x, w) + b.astype(np.float64)), False
        for mode in MODES:
            with mode_option(mode):
                got[mode] = new(M, Cout)
                X.call(entry, X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(b)), X.ptr(got[mode]), M, Cin, Cout, *wsbuf(X.workspace_bytes(M, Cin, Cout)), X.stream())
    elif entry == "myolo_pwconv1x1_bwd_data":
        ref, absdot, K = mm64(dy, w.T), mm64(np.abs(dy), np.abs(w.T)), Cout
        seq, want_x6 = (lambda: seq_matmul(dy, np.ascontiguousarray(w.T))), Cin % 256 == 0 and Cout % 16 == 0 and M >= 4096
        for mode in MODES:
            with mode_option(mode):
                got[mode] = new(M, Cin)
                X.call(entry, X.ptr(dt(dy)), X.ptr(dt(w)), X.ptr(got[mode]), M, Cin, Cout, *wsbuf(X.workspace_bytes(M, Cin, Cout)), X.stream())
    else:
        ref, absdot, K = mm64(x.T, dy), mm64(np.abs(x.T), np.abs(dy)), M
        seq, want_x6 = (lambda: seq_matmul(np.ascontiguousarray(x.T), dy)), Cin % 256 == 0 and Cout % 256 == 0 and M >= 4096
        for mode in MODES:
            with mode_option(mode):
                got[mode] = new(Cin, Cout)
                X.call(entry, X.ptr(dt(x)), X.ptr(dt(dy)), X.ptr(got[mode]), M, Cin, Cout, *wsbuf(X.workspace_bytes(M, Cin, Cout)), X.stream())
    torch.cuda.synchronize()
    split = _gemm_case(got, ref, absdot, K, "%s %s" % (entry, args), seq)
    assert split or not want_x6, "%s %s: bit-identical to native -- did not reach the bf16x6 kernel" % (entry, args)


COLSUM_ROWS = _rows_of("myolo_colsum")


@pytest.mark.parametrize("entry,args", COLSUM_ROWS, ids=_ids(COLSUM_ROWS))
def test_launch_colsum(entry, args):
    """bias gradients: a dot product of M ones with a column -- check_a with K = M"""
    M, C = args
    rng = np.random.default_rng(seed_of(entry, args))
    dy = rnd(rng, M, C)
    out = new(C)
    X.call(entry, X.ptr(dt(dy)), X.ptr(out), M, C, *wsbuf(X.workspace_bytes(M, C, C)), X.stream())
    d64 = dy.astype(np.float64)
    check_a(out, d64.sum(0), np.abs(d64).sum(0), M, what="colsum %s" % (args,))


# ---- 3x3 convs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _conv_case(N, H, W, Cin, Cout):
    """operands and float64 results (torch on the CPU) of a 3x3 / s1 / SAME conv and its gradients, plus torch's own CPU float32 forward error"""
    rng = np.random.default_rng(N * 1000003 + H * 1009 + W * 101 + Cin * 7 + Cout)
    x, w, b, dy = act_in(rng, N, H, W, Cin), he(rng, 3, 3, Cin, Cout), rnd(rng, Cout, scale=0.1), rnd(rng, N, H, W, Cout)
    xt, wt = nchw(x).requires_grad_(True), t64(w).requires_grad_(True)
    y = Fn.conv2d(xt, wt.permute(3, 2, 0, 1), bias=t64(b), padding=1)
    (y * nchw(dy)).sum().backward()
    y32 = Fn.conv2d(nchw(x).float(), torch.from_numpy(w).permute(3, 2, 0, 1), bias=torch.from_numpy(b), padding=1)
    ref = dict(y=nhwc(y), dx=nhwc(xt.grad), dw=wt.grad.numpy())
    cpu32 = float((y32.double() - y.detach()).abs().max() / y.detach().abs().max())
    return x, w, b, dy, ref, cpu32


def normwise(got, ref):
    """max|err| / max|ref| (test_gpu_fp32_products' (b)); the suite's TOL form (test_gpu_ops.relerr) divides by max(1, max|ref|)"""
    return errs(got, ref)[0], maxnorm(got, ref)


CIN512_TOL = 2.2e-5


def wino_bound(Cin):
    """the F(4,3) normwise bound of a case.  Cin <= 256: W43_TOL.  Cin = 512 (feature_map on res3d, K = 9 * 512: the project had no number): 10 x
    the float64 error of torch's CPU float32 convolution on the same operands, 10 being the ratio between the project's own direct (5e-6) and
    Winograd (5e-5) bounds.  Measured: 2.209e-6 on 6 x 64 x 64, 512 -> 256 (2.199e-6 on the ragged 3 x 61 x 66), hence CIN512_TOL = 2.2e-5 --
    tighter than W43_TOL, with 7 % of headroom on the ragged map: a miss after a change of seed or summation order is to be read against the
    printed CPU float32 figure of that run before a kernel is suspected.  The kernels' own figures there: forward 1.36e-5 (bf16x6) / 1.51e-5 (native), data gradient 1.43e-5 / 1.56e-5,
    weight gradient 5.0e-6 / 1.03e-5; on the ragged map up to 2.06e-5 (native forward).  Each run prints the CPU convolution's error again."""
    return W43_TOL if Cin <= 256 else CIN512_TOL


WINO_SHAPES = sorted({a for e, a in L.rows() if e == "myolo_wino_multiply_w"})
# ragged edges next to the census shapes: one map that is no multiple of 4 per Winograd channel pair (extra operator rows, not table rows)
WINO_RAGGED = [(2, 126, 130, 64, 64), (2, 62, 67, 128, 128), (3, 61, 66, 512, 256)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,H,W,Cin,Cout", WINO_SHAPES + WINO_RAGGED, ids=["x".join(map(str, s)) for s in WINO_SHAPES + WINO_RAGGED])
def test_launch_winograd(N, H, W, Cin, Cout, mode):
    """F(4,3) as the engine runs it at full size (Net.conv3x3_fwd / conv3x3_bwd_weight / conv3x3_bwd_data): the forward as input transform +
    multiply_w + output transform with the bias (the rows myolo_wino_input_transform / _multiply_w / _output_transform of the table) and as the
    one-call myolo_conv3x3_wino_fwd with V kept; the data gradient; the weight gradient from x (the engine's form) and from the saved V.
    Gate: the suite's TOL; bound: wino_bound (fp32 level)."""
    case = _conv_case(N, H, W, Cin, Cout)
    x, w, b, dy, ref, cpu32 = case
    bound = wino_bound(Cin)
    with mode_option(mode):
        xt, wt, bt, dyt = dt(x), dt(w), dt(b), dt(dy)
        T = N * ((H + 3) // 4) * ((W + 3) // 4)
        U, V, Mm = new(X.wino_u_elems(Cin, Cout)), new(36, T, Cin), new(36, T, Cout)
        y = new(N, H, W, Cout)
        X.call("myolo_wino_input_transform", X.ptr(xt), X.ptr(V), N, H, W, Cin, X.stream())
        X.call("myolo_wino_multiply_w", X.ptr(V), X.ptr(wt), X.ptr(U), X.ptr(Mm), N, H, W, Cin, Cout, X.stream())
        X.call("myolo_wino_output_transform", X.ptr(Mm), X.ptr(bt), None, None, X.ptr(y), N, H, W, Cout, 0, X.stream())
        wsa = wsbuf(max(X.wino_ws_bytes(N, H, W, Cin, Cout, k) for k in (0, 1, 2)))
        y2, vk = new(N, H, W, Cout), new(36, T, Cin)
        X.call("myolo_conv3x3_wino_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), None, None, X.ptr(y2), N, H, W, Cin, Cout, 0, X.ptr(vk), *wsa, X.stream())
        dx, dw, dw2 = new(N, H, W, Cin), new(3, 3, Cin, Cout), new(3, 3, Cin, Cout)
        X.call("myolo_conv3x3_wino_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(dx), N, H, W, Cin, Cout, *wsa, X.stream())
        X.call("myolo_conv3x3_wino_bwd_weight", X.ptr(xt), None, X.ptr(dyt), X.ptr(dw), N, H, W, Cin, Cout, *wsa, X.stream())
        X.call("myolo_conv3x3_wino_bwd_weight", None, X.ptr(vk), X.ptr(dyt), X.ptr(dw2), N, H, W, Cin, Cout, *wsa, X.stream())
        torch.cuda.synchronize()
    print("F(4,3) %dx%dx%d %d->%d %s: torch CPU float32 forward error %.3e, bound %.3e" % (N, H, W, Cin, Cout, mode, cpu32, bound))
    fails = []
    for name, got, r in (("y (three launches)", y, ref["y"]), ("y (one call)", y2, ref["y"]), ("dx", dx, ref["dx"]), ("dw (from x)", dw, ref["dw"]),
                         ("dw (saved V)", dw2, ref["dw"])):
        e, e_tol = normwise(got, r)
        print("  %-20s normwise %.3e" % (name, e))
        assert e_tol <= TOL, (name, e_tol)
        if e > bound:
            fails.append((name, e, bound))
    assert not fails, fails


@pytest.mark.parametrize("N,H,W,Cin,Cout", WINO_SHAPES, ids=["x".join(map(str, s)) for s in WINO_SHAPES])
def test_launch_winograd_bf16x6_against_native(N, H, W, Cin, Cout):
    """check_c on the forward and both gradients where the bf16x6 multiply applies (its result differs from the native one); the 64 -> 64 and
    128 -> 128 pairs have no 256-column tile: there the two modes must agree with each other at fp32 level whatever kernel ran"""
    x, w, b, dy, ref, _ = _conv_case(N, H, W, Cin, Cout)
    out = {}
    for mode in MODES:
        with mode_option(mode):
            xt, wt, bt, dyt = dt(x), dt(w), dt(b), dt(dy)
            wsa = wsbuf(max(X.wino_ws_bytes(N, H, W, Cin, Cout, k) for k in (0, 1, 2)))
            y, dx, dw = new(N, H, W, Cout), new(N, H, W, Cin), new(3, 3, Cin, Cout)
            X.call("myolo_conv3x3_wino_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), None, None, X.ptr(y), N, H, W, Cin, Cout, 0, None, *wsa, X.stream())
            X.call("myolo_conv3x3_wino_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(dx), N, H, W, Cin, Cout, *wsa, X.stream())
            X.call("myolo_conv3x3_wino_bwd_weight", X.ptr(xt), None, X.ptr(dyt), X.ptr(dw), N, H, W, Cin, Cout, *wsa, X.stream())
            torch.cuda.synchronize()
            out[mode] = (y, dx, dw)
    for i, name in enumerate(("y", "dx", "dw")):
        a, n = out["bf16x6"][i], out["native"][i]
        if not torch.equal(a, n):
            check_c(a, n, ref[name], "F(4,3) %s %dx%dx%d %d->%d" % (name, N, H, W, Cin, Cout))
    if Cout % 256 == 0:
        assert not torch.equal(out["bf16x6"][0], out["native"][0]), "the 256-column forward did not reach the bf16x6 multiply"


DIRECT_SHAPES = sorted({a for e, a in L.rows() if e == "myolo_conv3x3_fwd"})


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,H,W,Cin,Cout", DIRECT_SHAPES, ids=["x".join(map(str, s)) for s in DIRECT_SHAPES])
def test_launch_direct_conv3x3(N, H, W, Cin, Cout, mode):
    """stages 4-5 stay on the direct implicit GEMM (6 144 / 1 536 rows < WINO_MIN_ROWS): forward with bias, data and weight gradient at the
    componentwise bound, K = 9 Cin (+ 1 for the bias), 9 Cout, N H W"""
    x, w, b, dy, ref, _ = _conv_case(N, H, W, Cin, Cout)
    ax, aw, ady = np.abs(x), np.abs(w), np.abs(dy)
    one = lambda a, k, **kw: nhwc(Fn.conv2d(nchw(a), t64(k).permute(3, 2, 0, 1), padding=1, **kw))      # noqa: E731
    abs_y = one(ax, aw, bias=t64(np.abs(b)))
    abs_dx = one(ady, np.ascontiguousarray(aw[::-1, ::-1].transpose(0, 1, 3, 2)))
    xp = np.pad(ax.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    abs_dw = np.stack([np.stack([mm64(xp[:, ky:ky + H, kx:kx + W].reshape(-1, Cin).T, ady.reshape(-1, Cout)) for kx in range(3)]) for ky in range(3)])
    with mode_option(mode):
        xt, wt, bt, dyt = dt(x), dt(w), dt(b), dt(dy)
        wsa = wsbuf(X.workspace_bytes(N * H * W, 4 * Cin, 4 * Cout))          # Net._rn_block_fwd's: (M, max(C, f2), max(f1, f3)), C = f3 = 4 f
        y, dx, dw = new(N, H, W, Cout), new(N, H, W, Cin), new(3, 3, Cin, Cout)
        X.call("myolo_conv3x3_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), X.ptr(y), N, H, W, Cin, Cout, *wsa, X.stream())
        X.call("myolo_conv3x3_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(dx), N, H, W, Cin, Cout, *wsa, X.stream())
        X.call("myolo_conv3x3_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(dw), N, H, W, Cin, Cout, *wsa, X.stream())
        torch.cuda.synchronize()
    check_a(y, ref["y"], abs_y, 9 * Cin + 1, what="conv3x3 fwd %s" % mode)
    check_a(dx, ref["dx"], abs_dx, 9 * Cout, what="conv3x3 dx %s" % mode)
    check_a(dw, ref["dw"], abs_dw, N * H * W, what="conv3x3 dw %s" % mode)
    assert normwise(y, ref["y"])[0] < 5e-6          # the direct kernel's fp32 level (test_winograd_error_is_at_fp32_level)


def test_winograd_and_direct_rows_cover_the_table():
    """the 3x3 cases above are built from the multiply_w / conv3x3_fwd rows: every other 3x3 row of the table has one of those shapes"""
    for e, a in L.rows():
        if e in ("myolo_conv3x3_wino_bwd_data", "myolo_conv3x3_wino_bwd_weight"):
            assert a in WINO_SHAPES
        elif e == "myolo_wino_input_transform":
            assert a in {s[:4] for s in WINO_SHAPES}
        elif e == "myolo_wino_output_transform":
            assert a in {s[:3] + (s[4], 0) for s in WINO_SHAPES}
        elif e in ("myolo_conv3x3_bwd_data", "myolo_conv3x3_bwd_weight"):
            assert a in DIRECT_SHAPES


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------------------
BN_SHAPES = sorted({a[:2] for e, a in L.rows() if e in ("myolo_bn_stats", "myolo_bn_apply_act", "myolo_bn_act_bwd")})


@pytest.mark.parametrize("M,C", BN_SHAPES, ids=["%dx%d" % s for s in BN_SHAPES])
def test_launch_batchnorm(M, C):
    """myolo_bn_stats / bn_apply_act / bn_act_bwd (batch statistics) at every (rows, channels) of the table, with the activation codes the table
    holds for that shape: test_gpu_ops.test_batchnorm's bounds, unchanged (mean 1e-5, variance 1e-4, moving statistics 1e-5, the rest TOL).  The
    statistics are accumulated in double on the device: 393 216 rows need no more room than 2 048."""
    rows = L.rows()
    acts = sorted({a[2] for e, a in rows if e == "myolo_bn_act_bwd" and a[:2] == (M, C)})
    has_stats = ("myolo_bn_stats", (M, C)) in rows
    rng = np.random.default_rng(M + C)
    x = rnd(rng, M, C, scale=2.0) + rnd(rng, 1, C)
    g, b = 1 + rnd(rng, C, scale=0.2), rnd(rng, C, scale=0.3)
    mm, mv = rnd(rng, C, scale=0.1), 1 + np.abs(rnd(rng, C, scale=0.1))
    dy = rnd(rng, M, C)
    xt = t64(x).requires_grad_(True)
    gt, bt = t64(g).requires_grad_(True), t64(b).requires_grad_(True)
    mean_r, var_r = xt.detach().mean(0), xt.detach().var(0, unbiased=False)
    mean, var, scale, shift = new(C), new(C), new(C), new(C)
    tmm, tmv = dt(mm), dt(mv)
    xd = dt(x)
    X.call("myolo_bn_stats", X.ptr(xd), X.ptr(dt(g)), X.ptr(dt(b)), X.ptr(mean), X.ptr(var), X.ptr(scale), X.ptr(shift), X.ptr(tmm), X.ptr(tmv),
           M, C, *wsbuf(), X.stream())
    # (393 216 x 64 is bn_conv1, whose statistics the step takes from the stem conv's epilogue: myolo_bn_stats makes them for its backward here)
    assert has_stats or (M, C) == (L.B * (L.SIZE // 2) ** 2, 64)
    assert maxnorm(mean, mean_r.numpy()) <= 1e-5 and maxnorm(var, var_r.numpy()) <= 1e-4
    rmm, rmv = O.bn_moving_update(mm, mv, mean_r.numpy().astype(np.float32), var_r.numpy().astype(np.float32), M)
    assert maxnorm(tmm, rmm) <= 1e-5 and maxnorm(tmv, rmv) <= 1e-5
    y_r = (xt - xt.mean(0)) / torch.sqrt(xt.var(0, unbiased=False) + 1e-3) * gt + bt
    for act in acts:
        a_r = torch.relu(y_r) if act == 1 else y_r
        if ("myolo_bn_apply_act", (M, C, act)) in rows:
            a = new(M, C)
            X.call("myolo_bn_apply_act", X.ptr(xd), X.ptr(scale), X.ptr(shift), X.ptr(a), M, C, act, X.stream())
            assert maxnorm(a, a_r.detach().numpy()) <= TOL, "bn apply"
        for t in (xt, gt, bt):
            t.grad = None
        (a_r * t64(dy)).sum().backward(retain_graph=True)
        dx, dg, db = new(M, C), new(C), new(C)
        X.call("myolo_bn_act_bwd", X.ptr(dt(dy)), X.ptr(xd), X.ptr(dt(g)), X.ptr(mean), X.ptr(var), X.ptr(scale), X.ptr(shift),
               X.ptr(dx), X.ptr(dg), X.ptr(db), M, C, act, 1, *wsbuf(), X.stream())
        assert maxnorm(dx, xt.grad.numpy()) <= TOL, ("bn dx", act)
        assert maxnorm(dg, gt.grad.numpy()) <= TOL, ("bn dgamma", act)
        assert maxnorm(db, bt.grad.numpy()) <= TOL, ("bn dbeta", act)


def test_launch_bn_frozen_coeffs_batched():
    """the inference forward's one launch for all 53 trunk BatchNorms: scale = gamma / sqrt(moving_variance + eps), shift = beta - moving_mean * scale"""
    (n,), = [a for e, a in L.rows() if e == "myolo_bn_frozen_coeffs_batched"]
    rng = np.random.default_rng(53)
    C = [int(c) for c in rng.choice([64, 128, 256, 512, 1024, 2048], size=n)]
    tot = sum(C)
    p = np.concatenate([1 + rnd(rng, tot, scale=0.2), rnd(rng, tot, scale=0.3)])          # gammas, then betas
    s = np.concatenate([rnd(rng, tot, scale=0.1), 1 + np.abs(rnd(rng, tot, scale=0.1))])   # moving means, then variances
    table, off = [], 0
    for c in C:
        table.append([off, tot + off, off, tot + off, 2 * off, c])
        off += c
    out = new(2 * tot)
    X.call("myolo_bn_frozen_coeffs_batched", X.ptr(dt(p)), X.ptr(dt(s)), dt(np.asarray(table, np.int64)).data_ptr(), n, X.ptr(out), X.stream())
    got = out.cpu().numpy()
    for g_off, b_off, m_off, v_off, o, c in table:
        sc = p[g_off:g_off + c].astype(np.float64) / np.sqrt(s[v_off:v_off + c].astype(np.float64) + 1e-3)
        sh = p[b_off:b_off + c] - s[m_off:m_off + c].astype(np.float64) * sc
        assert maxnorm(got[o:o + c], sc) <= 1e-5 and maxnorm(got[o + c:o + 2 * c], sh) <= 1e-5


# ---- residual join, gather / scatter, max-pool, the stem -----------------------------------------------------------------------------------------
RES_ROWS = _rows_of("myolo_residual_fwd")


@pytest.mark.parametrize("entry,args", RES_ROWS, ids=_ids(RES_ROWS))
def test_launch_residual_join(entry, args):
    """test_gpu_resnet50.test_residual_join at the table's sizes (projection and identity shortcut), its bounds; the backward at M * C elements
    (the myolo_residual_bwd rows) and the identity shortcut's myolo_add_inplace at the block input's size"""
    M, C = args
    rows = L.rows()
    assert ("myolo_residual_bwd", (M * C,)) in rows
    rng = np.random.default_rng(M + C)
    y, sc = rnd(rng, M, C), rnd(rng, M, C)
    s, t = rng.random(C).astype(np.float32) + 0.5, rnd(rng, C, scale=0.3)
    s1, t1 = rng.random(C).astype(np.float32) + 0.5, rnd(rng, C, scale=0.3)
    dout = rnd(rng, M, C)
    y64, sc64 = y.astype(np.float64), sc.astype(np.float64)
    for proj in (True, False):
        out = new(M, C)
        X.call(entry, X.ptr(dt(y)), X.ptr(dt(s)), X.ptr(dt(t)), X.ptr(dt(sc)), X.ptr(dt(s1)) if proj else None, X.ptr(dt(t1)) if proj else None,
               X.ptr(out), M, C, X.stream())
        ref = np.maximum(y64 * s + t + (sc64 * s1 + t1 if proj else sc64), 0)
        assert maxnorm(out, ref) < TOL
        g = new(M, C)
        X.call("myolo_residual_bwd", X.ptr(dt(dout)), X.ptr(out), X.ptr(g), M * C, X.stream())
        # g = dout * [out > 0], on the forward's own decision (a pre-activation within rounding of 0 falls either way)
        assert np.array_equal(g.cpu().numpy(), dout * (out.cpu().numpy() > 0))
    acc = dt(y)
    X.call("myolo_add_inplace", X.ptr(acc), X.ptr(dt(sc)), M * C, X.stream())
    assert np.array_equal(acc.cpu().numpy(), y + sc)


def test_launch_add_inplace_rows_are_block_inputs():
    """every myolo_add_inplace row has the element count of a residual row (run there) or of a block input of the same stage"""
    sizes = {a[0] * a[1] for e, a in L.rows() if e == "myolo_residual_fwd"}
    for e, a in L.rows():
        if e == "myolo_add_inplace":
            assert a[0] in sizes or 4 * a[0] in sizes, a


def test_launch_add_inplace():
    for (n,) in sorted({a for e, a in L.rows() if e == "myolo_add_inplace"}):
        rng = np.random.default_rng(n % 1000)
        a, b = rnd(rng, n), rnd(rng, n)
        acc = dt(a)
        X.call("myolo_add_inplace", X.ptr(acc), X.ptr(dt(b)), n, X.stream())
        assert np.array_equal(acc.cpu().numpy(), a + b), n
        del _KEEP[:]


GS_ROWS = _rows_of("myolo_gather_s2")


@pytest.mark.parametrize("entry,args", GS_ROWS, ids=_ids(GS_ROWS))
def test_launch_gather_and_scatter_s2(entry, args):
    """test_gpu_resnet50.test_gather_and_scatter_s2 at the table's sizes: exact"""
    N, H, W, C = args
    assert ("myolo_scatter_s2", args) in L.rows()
    rng = np.random.default_rng(H + C)
    x = rnd(rng, N, H, W, C)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xs = new(N, Ho, Wo, C)
    X.call("myolo_gather_s2", X.ptr(dt(x)), X.ptr(xs), N, H, W, C, X.stream())
    assert np.array_equal(xs.cpu().numpy(), x[:, ::2, ::2, :])
    a, b = rnd(rng, N, Ho, Wo, C), rnd(rng, N, Ho, Wo, C)
    dx = new(N, H, W, C)
    X.call("myolo_scatter_s2", X.ptr(dt(a)), X.ptr(dt(b)), X.ptr(dx), N, H, W, C, X.stream())       # the engine's form: both branches' gradients
    ref = np.zeros((N, H, W, C), np.float32)
    ref[:, ::2, ::2, :] = a + b
    assert np.array_equal(dx.cpu().numpy(), ref)


STEM_ROWS = _rows_of("myolo_conv7x7s2_c3_bnstats_fwd", "myolo_conv7x7s2_c3_affine_act_fwd", "myolo_conv7x7s2_c3_bwd_weight")


@functools.lru_cache(maxsize=1)
def _stem_case():
    rng = np.random.default_rng(12)
    N, H, W, Co = L.B, L.SIZE, L.SIZE, 64
    x, w, b = rng.random((N, H, W, 3), dtype=np.float32), rnd(rng, 7, 7, 3, Co, scale=0.1), rnd(rng, Co, scale=0.1)
    dy = rnd(rng, N, H // 2, W // 2, Co)
    wt = t64(w).requires_grad_(True)
    ref = Fn.conv2d(Fn.pad(nchw(x), (3, 3, 3, 3)), wt.permute(3, 2, 0, 1), bias=t64(b), stride=2)
    (ref * nchw(dy)).sum().backward()
    g, be = (1 + rng.random(Co)).astype(np.float32), rnd(rng, Co, scale=0.1)
    return x, w, b, dy, g, be, nhwc(ref), wt.grad.numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry,args", STEM_ROWS, ids=_ids(STEM_ROWS))
def test_launch_stem(entry, args, mode):
    """the 7x7 / s2 stem at 6 x 512^2 in the three forms the table holds (test_gpu_resnet50.test_conv7x7s2_forward_and_weight_gradient's bounds)"""
    N, H, W, Co = args[-4:]
    assert (N, H, W, Co) == (L.B, L.SIZE, L.SIZE, 64)
    x, w, b, dy, g, be, r, dw_ref = _stem_case()
    Hs = H // 2
    with mode_option(mode):
        p, n = wsbuf(X.conv7x7s2_ws_bytes(N, H, W, Co))
        if entry == "myolo_conv7x7s2_c3_bnstats_fwd":
            mean, var = r.mean((0, 1, 2)), r.var((0, 1, 2))
            stats = [new(Co) for _ in range(4)]
            mov = [dt(np.zeros(Co, np.float32)), dt(np.ones(Co, np.float32))]
            y = new(N, Hs, Hs, Co)
            X.call(entry, X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(b)), X.ptr(y), X.ptr(dt(g)), X.ptr(dt(be)),
                   *[X.ptr(t) for t in stats], *[X.ptr(t) for t in mov], N, H, W, Co, p, n, X.stream())
            assert maxnorm(y, r) < TOL
            assert maxnorm(stats[0], mean) < TOL and maxnorm(stats[1], var) < TOL
            sc_ref = g / np.sqrt(var + 1e-3)
            assert maxnorm(stats[2], sc_ref) < TOL and maxnorm(stats[3], be - mean * sc_ref) < TOL
        elif entry == "myolo_conv7x7s2_c3_affine_act_fwd":
            assert args[0] == 1
            y3 = new(N, Hs, Hs, Co)
            X.call(entry, X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(b)), X.ptr(dt(g)), X.ptr(dt(be)), 1, X.ptr(y3), N, H, W, Co, p, n, X.stream())
            assert maxnorm(y3, np.maximum(r * g + be, 0)) < TOL
        else:
            dw, db = new(7, 7, 3, Co), new(Co)
            X.call(entry, X.ptr(dt(x)), X.ptr(dt(dy)), X.ptr(dw), X.ptr(db), N, H, W, Co, p, n, X.stream())
            assert maxnorm(dw, dw_ref) < TOL and maxnorm(db, dy.astype(np.float64).sum((0, 1, 2))) < TOL
        torch.cuda.synchronize()


POOL_ROWS = _rows_of("myolo_maxpool3x3s2_fwd")


@pytest.mark.parametrize("entry,args", POOL_ROWS, ids=_ids(POOL_ROWS))
def test_launch_maxpool(entry, args):
    """the max-pool on the stem's map, with bn_conv1 + ReLU on its load (training) and plain (inference): exact values and first-maximum
    argmax (test_gpu_resnet50.test_maxpool_forward_backward); the backward (the myolo_maxpool3x3s2_bwd row) on the forward's argmax"""
    affine, N, H, W, C = args
    assert ("myolo_maxpool3x3s2_bwd", (N, H, W, C)) in L.rows()
    rng = np.random.default_rng(13)
    xq = rng.integers(-6, 6, size=(N, H, W, C)).astype(np.float32) / 4
    sc = (2.0 ** rng.integers(-1, 2, size=C)).astype(np.float32)
    sh = (rng.integers(-2, 3, size=C) / 4).astype(np.float32)
    act = np.maximum(xq * sc + sh, 0).astype(np.float32) if affine else xq
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y, arg = new(N, Ho, Wo, C), new(N, Ho, Wo, C, dtype=torch.uint8)
    X.call(entry, X.ptr(dt(xq)), X.ptr(dt(sc)) if affine else None, X.ptr(dt(sh)) if affine else None, affine, X.ptr(y), X.ptr(arg), N, H, W, C, X.stream())
    t = nchw(act).requires_grad_(True)
    pr = Fn.max_pool2d(Fn.pad(t, (1, 1, 1, 1)), 3, 2)
    assert np.array_equal(y.cpu().numpy(), nhwc(pr).astype(np.float32))
    pad = np.pad(act, ((0, 0), (1, 1), (1, 1), (0, 0)))
    win = np.stack([pad[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :] for kh in range(3) for kw in range(3)], 0)
    assert np.array_equal(arg.cpu().numpy(), np.argmax(win, 0))
    dy = rnd(rng, N, Ho, Wo, C)
    dx = new(N, H, W, C)
    X.call("myolo_maxpool3x3s2_bwd", X.ptr(dt(dy)), X.ptr(arg), X.ptr(dx), N, H, W, C, X.stream())
    (pr * nchw(dy)).sum().backward()
    assert maxnorm(dx, nhwc(t.grad)) < TOL


def test_every_entry_of_the_table_has_an_operator_case():
    covered = {"myolo_pwconv1x1_fwd", "myolo_pwconv1x1_bwd_data", "myolo_pwconv1x1_bwd_weight", "myolo_colsum", "myolo_wino_input_transform",
               "myolo_wino_multiply_w", "myolo_wino_output_transform", "myolo_conv3x3_wino_bwd_data", "myolo_conv3x3_wino_bwd_weight",
               "myolo_conv3x3_fwd", "myolo_conv3x3_bwd_data", "myolo_conv3x3_bwd_weight", "myolo_bn_stats", "myolo_bn_apply_act", "myolo_bn_act_bwd",
               "myolo_bn_frozen_coeffs_batched", "myolo_residual_fwd", "myolo_residual_bwd", "myolo_add_inplace", "myolo_gather_s2",
               "myolo_scatter_s2", "myolo_maxpool3x3s2_fwd", "myolo_maxpool3x3s2_bwd", "myolo_conv7x7s2_c3_bnstats_fwd",
               "myolo_conv7x7s2_c3_affine_act_fwd", "myolo_conv7x7s2_c3_bwd_weight"}
    assert set(L.LAUNCHES) == covered


# ------------------------------------------------------------------------------------------------ 3. the whole step and forward at full size
class FullSizeRef(ResNetRef):
    """ResNetRef whose train_step fits the full size: the same float64 operations, with the mask head's tape kept only where a gradient flows.
    The mask loss reads the positive ROIs alone, and behind myolo_mask_bn1 (the one BatchNorm of the head on batch statistics) every ROI is
    independent of the others: conv1 + bn1 + ReLU run taped over all ROIs, the rest of the head runs without a tape in chunks of ROIS_PER_CHUNK
    (the predictions) and with one on the positive ROIs (the loss), whose gradient enters bn1's output at the positives' rows.  Same sums in
    another order (against TorchRef.train_step at 2 x 128^2: every gradient within 5e-16 relative L2, the masks equal); train_step(batch, backward=False) is the forward alone, without any tape."""
    ROIS_PER_CHUNK = 256

    def __init__(self, P_np, cfg, forced=None, rois=None, **kw):
        """rois [B, R, 4]: the mask head's ROIs taken as given (the engine's output_rois) instead of the oracle's own"""
        super().__init__(P_np, cfg, forced=forced, **kw)
        self.rois = rois

    def _head_front(self, Fm, rois):
        """ROIAlign + conv1 + bn1 (batch statistics) + ReLU over all ROIs"""
        P, cfg = self.P, self.cfg
        Bn, R = rois.shape[:2]
        boxes = O.roi_boxes_to_crop_order(rois.reshape(-1, 4), cfg.ROI_BOX_ORDER)
        x = crop_and_resize_t(Fm, boxes, np.repeat(np.arange(Bn), R), cfg.MASK_POOL_SIZE, cfg.MASK_POOL_SIZE)
        x = _conv(x, P["myolo_mask_conv1/kernel"], pad=(1, 1, 1, 1), bias=P["myolo_mask_conv1/bias"])
        b = "myolo_mask_bn1"
        return torch.relu(_bn(x, P[b + "/gamma"], P[b + "/beta"], P[b + "/moving_mean"], P[b + "/moving_variance"], True))

    def _head_back(self, x):
        """conv2-4 with their frozen BatchNorms, the deconv and the class masks (TorchRef.mask_head behind bn1)"""
        P = self.P
        for i in range(2, 5):
            n, b = "myolo_mask_conv%d" % i, "myolo_mask_bn%d" % i
            x = _conv(x, P[n + "/kernel"], pad=(1, 1, 1, 1), bias=P[n + "/bias"])
            x = torch.relu(_bn(x, P[b + "/gamma"], P[b + "/beta"], P[b + "/moving_mean"], P[b + "/moving_variance"], False))
        x = torch.relu(Fn.conv_transpose2d(x, P["myolo_mask_deconv/kernel"].permute(3, 2, 0, 1), bias=P["myolo_mask_deconv/bias"], stride=2))
        return torch.sigmoid(_conv(x, P["myolo_mask/kernel"], bias=P["myolo_mask/bias"]))

    def train_step(self, batch, backward=True):
        cfg = self.cfg
        images, true_boxes, y_true, gt_ids, gt_boxes, gt_masks = batch
        for k in self.train_names:
            self.P[k].grad = None
        with torch.set_grad_enabled(backward):
            C4, Fm, yolo_out = self.trunk(images, True)
            del C4
            yo_np = yolo_out.detach().to(torch.float32).numpy()
            proposals = O.yolo_decode(yo_np, cfg.ANCHORS, cfg.GRID_W)
            rois, tcls, tmask, npos = O.mask_targets(proposals, gt_ids, gt_boxes, gt_masks, cfg)
            if self.rois is not None:
                assert self.rois.shape == rois.shape
                rois = np.asarray(self.rois, rois.dtype)
            a1 = self._head_front(Fm, rois)
            with torch.no_grad():
                pred = torch.cat([self._head_back(a1[i:i + self.ROIS_PER_CHUNK]) for i in range(0, a1.shape[0], self.ROIS_PER_CHUNK)])
            tc = tcls.reshape(-1)
            pos = np.where(tc > 0)[0]
            a1p = a1.detach()[torch.from_numpy(pos)].requires_grad_(backward)
            ml = mask_bce_t(tmask.reshape((-1,) + tmask.shape[2:])[pos], tc[pos], self._head_back(a1p))
            yl, _ = yolo_loss_t(_t(y_true, self.dtype), yolo_out, _t(true_boxes, self.dtype), cfg)
            w1, w2 = cfg.LOSS_WEIGHTS.get("yolo_sum_loss", 1.), cfg.LOSS_WEIGHTS.get("myolo_mask_loss", 1.)
            out = dict(loss=float((yl * w1 + ml * w2).detach()), yolo_sum_loss=float(yl.detach()), mask_loss=float(ml.detach()),
                       yolo_output=yo_np, output_rois=rois, target_class_ids=tcls, myolo_mask=pred.permute(0, 2, 3, 1).numpy(),
                       feature_map=Fm.detach().permute(0, 2, 3, 1).numpy())
            if backward:
                (ml * w2).backward()                       # the head behind bn1: its parameters and the positives' rows of bn1's output
                da1 = torch.zeros_like(a1)
                da1[torch.from_numpy(pos)] = a1p.grad
                torch.autograd.backward([a1, yl * w1], [da1, None])
                out["grads"] = {k: self.P[k].grad.detach().numpy() for k in self.train_names if self.P[k].grad is not None}
        return out

# Screening at full size.  decision_margins' roi_px is the distance of every ROIAlign sample coordinate from the edge of the sampled map, where
# crop_and_resize switches to extrapolation.  The small test asks for 4e-3 px because oracle and engine there compute their ROI corners from their
# own yolo_output (fp32 noise ~3e-5 -> ~1e-3 px).  Among 4 608 ROIs x 28 coordinates on a 64 x 64 map no batch leaves that much (seen: 4e-5 .. 3e-4
# px).  Here the forced oracle takes the ROIs themselves from the engine (FullSizeRef(rois=output_rois)), as it takes the ReLU masks: both sides
# then start from the same fp32 corners, and what is left is the rounding of the coordinate arithmetic itself -- y1 (H - 1) + i (y2 - y1) (H - 1) /
# (crop - 1), three fp32 operations on values up to ~1.2 x 63 px, i.e. 3 x 76 x 2^-24 = 1.4e-5 px.  FULL_MIN_ROI_PX is 7 x that.  The partition and
# no-object margins keep the small test's 1e-3 (min_margin).
FULL_MIN_ROI_PX = 1e-4


def _case_params(ref):
    return {k: v.detach().numpy() for k, v in ref.P.items()}


def full_case():
    """the screened 6 x 512^2 batch; its unforced oracle is a forward without a tape (the step's comparisons against it are forward values)"""
    return resnet_case(L.NUM_CLASSES, size=L.SIZE, batch=L.B, min_roi_px=FULL_MIN_ROI_PX,
                       oracle=lambda ref, batch: FullSizeRef(_case_params(ref), ref.cfg).train_step(batch, backward=False))


@pytest.mark.parametrize("fp32_matmul", MODES)
def test_train_step_full_size_matches_oracle(fp32_matmul):
    """test_gpu_resnet50.test_train_step_matches_oracle's recipe, assertions and bounds (step_against_oracle) at 6 x 512^2, 81 classes: the
    workspace regrows between stages, the side streams overlap far longer launches, and every kernel is the full-size choice.  Stage 5
    normalises 1 536 rows per channel here instead of 32: the five worst gradient keys are printed for the record of the headroom under 2 %."""
    import resource
    import time
    t0 = time.time()
    worst = step_against_oracle(full_case(), fp32_matmul, forced_oracle=lambda P, cfg, seen, batch, out: FullSizeRef(
        P, cfg, forced=seen, rois=np.asarray(out["output_rois"])).train_step(batch))
    print("full size %s: %.0f s in all, peak resident set %.1f GB" % (fp32_matmul, time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6))
    for k, e in sorted(worst.items(), key=lambda kv: -kv[1])[:5]:
        print("full size %s: %-40s relative L2 %.3e" % (fp32_matmul, k, e))


@pytest.mark.parametrize("early", [-1, 1])
def test_full_size_two_runs_bit_identical(early):
    """test_gpu_resnet50.test_two_runs_bit_identical at full size, where the YOLO branch's early backward overlaps the mask head's longest launches"""
    cfg, P, batch = _scene(L.SIZE, L.B, "bf16x6")
    outs, gs = [], []
    for _ in range(2):
        model = MaskYOLO(mode="training", config=cfg)
        model.net.yolo_bwd_early = early
        model.load_state_dict(P)
        outs.append(model.train_on_batch(batch, learning_rate=0.0))
        gs.append(model.net.flat_g.clone())
        del model
    assert outs[0]["loss"] == outs[1]["loss"]
    assert np.array_equal(outs[0]["yolo_output"], outs[1]["yolo_output"])
    assert torch.equal(gs[0], gs[1])


def test_full_size_inference_forward_matches_oracle():
    """test_gpu_resnet50.test_inference_forward_matches_oracle at 6 x 512^2: frozen BatchNorms do not cancel a conv bias, so a bias lost on the way
    to a full-size kernel shows here (the training step's batch statistics would hide it)"""
    from test_gpu_step import rel
    cfg = _cfg(L.NUM_CLASSES, B=L.B, size=L.SIZE)
    model = MaskYOLO(mode="inference", config=cfg)
    model.load_state_dict(_params(cfg, 5))
    samples = make_shapes_samples(L.B, cfg)
    images = np.stack([s[0] for s in samples]).astype(np.float32) / 255.
    yo, det, mask = model.keras_model.predict([images])
    ref = ResNetRef(model.state_dict(), cfg)
    with torch.no_grad():
        C4, Fm, ryo = ref.trunk(images, False)
        assert rel(yo, ryo.numpy()) < TOL
        rdet = O.yolo_detections(ryo.numpy().astype(np.float32), cfg.ANCHORS, cfg.GRID_W)
        assert np.array_equal(det[..., 5], rdet[..., 5]), "class ids differ"
        assert rel(det[..., :5], rdet[..., :5]) < TOL
        for i in range(L.B):          # (image by image: the head's float64 activations of 768 ROIs at a time)
            pred = ref.mask_head(Fm[i:i + 1], rdet[i:i + 1, ..., :4], False)
            assert rel(mask[i], pred.permute(0, 2, 3, 1).numpy().reshape(mask[i].shape)) < TOL, i


def test_full_size_hip_graph_replay_equals_eager():
    cfg = _cfg(L.NUM_CLASSES, B=L.B, size=L.SIZE)
    model = MaskYOLO(mode="inference", config=cfg)
    model.load_state_dict(_params(cfg, 5))
    net = model.net
    rng = np.random.default_rng(8)
    for _ in range(2):
        x = torch.as_tensor(rng.random((L.B, L.SIZE, L.SIZE, 3), dtype=np.float32), device=net.dev)
        g = [t.clone() for t in net.predict_graphed(x)]
        e = net.predict(x)
        assert all(torch.equal(u, v) for u, v in zip(g, e))


# ------------------------------------------------------------------------------------------------ 4. alignment of the on-load BatchNorm's coefficients
@pytest.mark.parametrize("mode", MODES)
def test_pw_bnstats_fwd_with_unaligned_scale_and_shift(mode):
    """every kernel behind myolo_pwconv1x1_bnstats_fwd reads in_scale / in_shift as float4 beside the A operand (pw_smallm_kernel, gemm_nn_fast,
    the thin and the bf16x6 kernels).  A C-ABI caller whose coefficient vectors sit 4 bytes off a 16-byte boundary gets them copied to the
    aligned end of the workspace first, and the float64 result at the componentwise bound -- at a small-M shape (pw_smallm_kernel, whose
    pw_smallm_ok also checks the two pointers) and at one the big-tile kernels take.  myolo_pwconv1x1_bwd_weight_affine_in refuses such a pair."""
    rng = np.random.default_rng(77)
    for M, Cin, Cout in ((1568, 512, 256), (6144, 256, 1024)):
        x, w = rnd(rng, M, Cin, scale=2.0), he(rng, Cin, Cout)
        isc, ish = 1 + rnd(rng, Cin, scale=0.3), rnd(rng, Cin, scale=1.0)
        a64 = np.maximum((x.astype(np.float64) * isc + ish).astype(np.float32), 0).astype(np.float64)
        ref, absdot = mm64(a64, w), mm64(np.abs(a64), np.abs(w))
        g, b = 1 + rnd(rng, Cout, scale=0.2), rnd(rng, Cout, scale=0.3)
        with mode_option(mode):
            for off in (1, 0):
                sbuf, tbuf = new(Cin + 4), new(Cin + 4)
                sc, sh = sbuf[off:off + Cin], tbuf[off:off + Cin]
                sc.copy_(torch.from_numpy(isc))
                sh.copy_(torch.from_numpy(ish))
                assert sc.data_ptr() % 16 == 4 * off and sh.data_ptr() % 16 == 4 * off
                y = new(M, Cout)
                mean, var, scale, shift = new(Cout), new(Cout), new(Cout), new(Cout)
                X.call("myolo_pwconv1x1_bnstats_fwd", X.ptr(dt(x)), sc.data_ptr(), sh.data_ptr(), 1, X.ptr(dt(w)), X.ptr(y), X.ptr(dt(g)), X.ptr(dt(b)),
                       X.ptr(mean), X.ptr(var), X.ptr(scale), X.ptr(shift), X.ptr(dt(np.zeros(Cout, np.float32))), X.ptr(dt(np.ones(Cout, np.float32))),
                       M, Cin, Cout, 3, *wsbuf(), X.stream())
                torch.cuda.synchronize()
                check_a(y, ref, absdot, Cin, extra=U24 * absdot, what="pw bnstats %s, coefficients %d bytes off" % ((M, Cin, Cout), 4 * off))
                assert maxnorm(mean, ref.mean(0)) <= 1e-5 and maxnorm(var, ref.var(0)) <= 1e-4
                if off:
                    with pytest.raises(RuntimeError, match="aligned"):
                        X.call("myolo_pwconv1x1_bwd_weight_affine_in", X.ptr(dt(x)), sc.data_ptr(), sh.data_ptr(), 1, X.ptr(y), X.ptr(new(Cin, Cout)),
                               M, Cin, Cout, *wsbuf(), X.stream())

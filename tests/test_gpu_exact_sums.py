"""The reductions and stencils of the training step held to EXACT sums on integer operands.

Operands are small integers or integer multiples of one power of two (`unit`).  Where sum|terms| < 2^24 units for an output, every partial sum
of it is exactly representable in fp32 in EVERY summation order (per-thread fp32 accumulators, fp32 atomics, fmaf, double partials), so the
float64 reference is the exact answer and the kernel must equal it bit for bit: one element dropped, duplicated or misplaced anywhere turns
the case red whatever its magnitude.  `assert_exact` asserts that precondition first (a case that could round is a test error, not a silent
pass), then np.array_equal, and reports the indices that differ -- they say which strip, chunk or border is wrong.

The producing layer's affine + ReLU / ReLU6 on load stays exact with per-channel scale in {1/2, 1, 2} and shift in multiples of 1/4, and hits
0 and 6 exactly in a good share of elements (asserted), where the backward mask's strict inequalities decide.  ROIAlign boxes have corners
in multiples of 1/8, so a good share of the samples falls exactly on a pixel centre (floor == ceil).

Every case id names the kernel / path of csrc/mem_kernels.hip it reaches; for the row-sliding depthwise kernels the geometry that the id
claims (channel block, strips, row chunks, tiles) is re-derived and asserted by `dw_rows_geom` below.

The only bounds in this file are the ulp-derived ones on BatchNorm statistics (`check_stats`): mean / var / scale within 1 fp32 ulp of the
float64 value formed from the exact sums, shift within 2^-22 (|beta| + |mean scale|) (three fp32 roundings)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_ops as O                      # noqa: E402
from myolo import _ext as X                         # noqa: E402

DEV = "cuda:0"
_KEEP = []   # device tensors must outlive the asynchronous kernel that reads them


@pytest.fixture(autouse=True)
def _keepalive():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dt(a, dtype=None):
    a = np.ascontiguousarray(a)
    t = torch.as_tensor(a if a.flags.writeable else a.copy(), device=DEV)          # (the shared references are read-only)
    t = t if dtype is None else t.to(dtype)
    _KEEP.append(t)
    return t


def new(*shape, dtype=torch.float32):
    t = torch.full(shape, float("nan") if dtype == torch.float32 else 0, dtype=dtype, device=DEV)
    _KEEP.append(t)
    return t


def ws():
    if not hasattr(ws, "buf"):
        ws.buf = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    return ws.buf.data_ptr(), ws.buf.numel()


def host(t):
    if torch.is_tensor(t):
        torch.cuda.synchronize()
        t = t.detach().cpu().numpy()
    return np.asarray(t)


# ---- the two helpers every case uses -------------------------------------------------------------------------------------------------------
def ints(rng, shape, lo, hi):
    """integers lo..hi (inclusive) as float32"""
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def act_np(v, act):
    return np.clip(v, 0, 6) if act == 2 else (np.maximum(v, 0) if act == 1 else v)


def pass_np(v, act):
    """1 where the activation passes gradient: strict inequalities (tf.nn.relu / relu6 gradients)"""
    return ((v > 0) & (v < 6)) if act == 2 else ((v > 0) if act == 1 else np.ones(v.shape, bool))


def pre_activation_operands(rng, shape, act):
    """A pre-BN tensor x (integers -4..12 for ReLU6, -4..2 otherwise; last axis = channels) with the producing layer's folded BatchNorm: per-channel scale in {1/2, 1, 2} and
    shift in multiples of 1/4, such that pre = x * scale + shift is exact in fp32 (a multiple of 1/4) and equals 0 -- and 6 -- exactly in a good
    share of elements.  Three channels in four have shift = -scale * t0 with t0 in -2..0 (ties at x = t0 and x = t0 + 6 / scale),
    the fourth is a quarter off (no ties, non-integer activations).  Asserts that >= 1 % of pre-activations equal 0 and, for ReLU6, >= 1 % equal 6.
    Returns x, scale, shift, pre (float64), a = act(pre) (float32, exact)."""
    C = shape[-1]
    x = ints(rng, shape, -4, 12 if act == 2 else 2)
    scale = np.array([0.5, 1.0, 2.0], np.float32)[rng.integers(0, 3, C)]
    shift = (-scale * rng.integers(-2, 1, C)).astype(np.float32)
    shift[3::4] += np.float32(0.25) * rng.integers(1, 4, shift[3::4].shape)
    pre = x.astype(np.float64) * scale + shift
    assert np.array_equal(pre, np.round(pre * 4) / 4) and np.abs(pre).max() < 64
    if x.size >= 1000:
        assert (pre == 0).mean() >= 0.01, "operand maker: only %.2f %% of pre-activations are exactly 0" % (100 * (pre == 0).mean())
        if act == 2:
            assert (pre == 6).mean() >= 0.01, "operand maker: only %.2f %% of pre-activations are exactly 6" % (100 * (pre == 6).mean())
    return x, scale, shift, pre, act_np(pre, act).astype(np.float32)


def assert_exact(got, ref64, abs_terms, unit, what=""):
    """got == ref64 bit for bit, behind the precondition that makes ref64 THE answer in every summation order: every operand product is a multiple of
    `unit` and sum|terms| (abs_terms: the same operation on |operands|) stays below 2^24 units for every output."""
    got, ref64, abs_terms = host(got), np.asarray(ref64, np.float64), np.asarray(abs_terms, np.float64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    top = float(abs_terms.max()) / unit if abs_terms.size else 0.0
    assert top < 2.0 ** 24, "%s: test error: sum|terms| reaches %.4g units of %g (>= 2^24): the sums could round" % (what, top, unit)
    assert np.array_equal(ref64 / unit, np.round(ref64 / unit)), "%s: test error: the reference is not a multiple of the unit %g" % (what, unit)
    want = ref64.astype(np.float32)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    first = "; ".join("%s got %r want %r" % (tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6])
    raise AssertionError("%s: %d of %d elements differ from the exact result; first: %s" % (what, len(bad), want.size, first))


def check_stats(what, y2d, gamma, beta, mean, var, scale, shift):
    """BatchNorm statistics of y2d [M, C] (whose sums are exact in fp32: asserted): the kernel forms mean = sum / M and var = sumsq / M - mean^2 in
    double from exact sums and rounds once.  mean, var, scale (gamma a power of two) within 1 fp32 ulp of the float64 value; shift within
    2^-22 (|beta| + |mean scale|)."""
    y = np.asarray(y2d, np.float64)
    assert np.array_equal(y * 4, np.round(y * 4))
    assert float((y * y).sum(0).max()) * 16 < 2.0 ** 24, "%s: test error: the sum of squares reaches %.4g units of 1/16" % (what, float((y * y).sum(0).max()) * 16)
    m, v = y.mean(0), y.var(0)
    sc = gamma.astype(np.float64) / np.sqrt(v + float(O.BN_EPS))
    sh = beta.astype(np.float64) - m * sc

    def ulp(r):
        return np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
    for name, got, ref, tol in (("mean", mean, m, ulp(m)), ("var", var, v, ulp(v)), ("scale", scale, sc, ulp(sc)),
                                ("shift", shift, sh, 2.0 ** -22 * (np.abs(beta) + np.abs(m * sc)))):
        err = np.abs(host(got).astype(np.float64) - ref)
        bad = np.argwhere(err > tol)
        print("%s %s: worst err / bound %.3f" % (what, name, float((err / np.maximum(tol, 1e-300)).max())))
        assert not len(bad), "%s %s: %d channels beyond the bound, first %d: got %r want %r (bound %.3g)" % (
            what, name, len(bad), bad[0][0], float(host(got)[bad[0][0]]), float(ref[bad[0][0]]), float(tol[bad[0][0]]))


def bn_params(rng, C):
    """gamma a power of two (either sign), beta in multiples of 1/4; moving averages for the entry points that update them"""
    gamma = (np.array([0.5, 1.0, 2.0], np.float32)[rng.integers(0, 3, C)] * np.where(rng.random(C) < 0.2, -1, 1)).astype(np.float32)
    beta = (np.float32(0.25) * rng.integers(-8, 9, C)).astype(np.float32)
    return gamma, beta, dt(np.zeros(C, np.float32)), dt(np.ones(C, np.float32))


# ============================================================================================================================================
# A. depthwise 3x3
# ============================================================================================================================================
def dw_rows_geom(N, H, W, C, S):
    """restates dw_rows_geom of csrc/mem_kernels.hip: channel-quad block, strip widths, row-chunk heights, workgroups"""
    Ho, Wo, cq = H // S, W // S, C // 4
    cqb = 32 if (Wo <= 7 and cq % 32 == 0) else (16 if cq % 16 == 0 else 8)
    px = 224 // cqb
    strips = -(-Wo // px)
    base, chunks = N * (cq // cqb) * strips, 1
    while base * chunks < 1024 and Ho // (chunks * 2) >= 7:
        chunks *= 2
    rc = -(-Ho // chunks)
    chunks = -(-Ho // rc)
    return dict(cqb=cqb, ncb=cq // cqb, strips=[min(px, Wo - i * px) for i in range(strips)], chunks=[min(rc, Ho - i * rc) for i in range(chunks)],
                tiles=base * chunks)


def dw_fwd_which(N, H, W, C, S):
    """restates dw_fwd_grid for the shapes the row-sliding kernels do not take (C % 32 != 0): the dw_fwd_kernel<S, TW, TH> instance"""
    Ho, Wo = H // S, W // S
    if S == 1:
        wg4 = -(-(-(-Wo // 4) * (C // 4)) // 256) * -(-Ho // 4) * N
        return "1,4,4" if (Ho >= 4 and wg4 >= 400) else ("1,4,2" if Ho >= 2 else "1,4,1")
    wg2 = -(-(-(-Wo // 2) * (C // 4)) // 256) * -(-Ho // 2) * N
    return "2,2,2" if (Ho >= 2 and wg2 >= 400) else "2,2,1"


# (id, (N, H, W, C, stride), what the dispatch must give)
DW_ROWS = [
    ("dw_rows<1,8>-5cb-strips28+28+2", (2, 30, 58, 160, 1), dict(cqb=8, ncb=5, strips=[28, 28, 2], chunks=[8, 8, 8, 6])),
    ("dw_rows<2,8>-3cb-chunks12+11", (2, 46, 40, 96, 2), dict(cqb=8, ncb=3, strips=[20], chunks=[12, 11])),
    ("dw_rows<1,16>-strips14+14+12-chunks12+12+12+10", (2, 46, 40, 64, 1), dict(cqb=16, strips=[14, 14, 12], chunks=[12, 12, 12, 10])),
    ("dw_rows<1,32>-9x7", (4, 9, 7, 1024, 1), dict(cqb=32, ncb=8, strips=[7], chunks=[9])),
    ("dw_rows<1,32>-5x3", (3, 5, 3, 128, 1), dict(cqb=32, ncb=1, strips=[3], chunks=[5])),
    ("dw_rows<2,32>", (2, 18, 14, 1024, 2), dict(cqb=32, ncb=8, strips=[7], chunks=[9])),
    ("dw_rows<1,16>-xcd_remap-64tiles", (8, 28, 28, 64, 1), dict(cqb=16, strips=[14, 14], chunks=[7, 7, 7, 7], tiles=64)),
    ("dw_rows<1,8>-xcd_remap-160tiles-31360px", (40, 28, 28, 32, 1), dict(cqb=8, ncb=1, strips=[28], chunks=[7, 7, 7, 7], tiles=160)),
]
# the generic kernels (C % 32 != 0): forward instance | data gradient | weight gradient
DW_GENERIC = [
    ("dw_fwd<1,4,4>+dw_bwd_data<1>+dw_wgrad_tiled", (25, 64, 5, 16, 1), "1,4,4"),
    ("dw_fwd<1,4,2>+dw_bwd_data<1>+dw_wgrad_tiled", (2, 9, 13, 16, 1), "1,4,2"),
    ("dw_fwd<1,4,1>+dw_bwd_data<1>+dw_wgrad_tiled", (1, 1, 5, 8, 1), "1,4,1"),
    ("dw_fwd<2,2,2>+dw_bwd_data_s2+dw_wgrad_tiled", (25, 64, 8, 16, 2), "2,2,2"),
    ("dw_fwd<2,2,1>+dw_bwd_data_s2+dw_wgrad_tiled", (1, 6, 10, 8, 2), "2,2,1"),
    ("dw_fwd<1,4,2>+dw_bwd_data<1>+OpDwDw_colreduce-C24", (2, 7, 6, 24, 1), "1,4,2"),
    ("dw_fwd<2,2,1>+dw_bwd_data_s2+OpDwDw_colreduce-C48", (3, 10, 6, 48, 2), "2,2,1"),
]
DW_CASES = [pytest.param(shape, id=i) for i, shape, _ in DW_ROWS + DW_GENERIC]


@pytest.mark.parametrize("cid,shape,want", DW_ROWS + DW_GENERIC, ids=[c[0] for c in DW_ROWS + DW_GENERIC])
def test_dw_case_ids_name_the_dispatch(cid, shape, want):
    """the geometry / kernel instance a case id claims is what the dispatch of csrc/mem_kernels.hip gives for its shape (host arithmetic only)"""
    N, H, W, C, S = shape
    if isinstance(want, dict):
        assert C % 32 == 0 and H * W * C * 4 < (1 << 30)                    # dw_rows_ok
        g = dw_rows_geom(*shape)
        assert {k: g[k] for k in want} == want, (cid, g)
        if "xcd_remap" in cid:
            assert g["tiles"] % 8 == 0 and g["tiles"] >= 64                 # the weight gradient's XCD-contiguous remap
    else:
        assert C % 32 != 0 and dw_fwd_which(*shape) == want
        assert ("colreduce" in cid) == (256 % (C // 4) != 0)                # the tiled weight gradient needs C/4 to divide 256


def _dw_abs(x, w, dy, S):
    """sum|terms| of y, dx, dw: the same operations on |operands|"""
    ay = O.dwconv3x3(np.abs(x), np.abs(w), S)
    adx, adw = O.dwconv3x3_bwd(np.abs(x), np.abs(w), np.abs(dy), S)
    return ay, adx, adw


@functools.lru_cache(maxsize=None)
def dw_plain_case(shape):
    """integer operands and the exact results of one depthwise shape, computed once"""
    N, H, W, C, S = shape
    rng = np.random.default_rng(101)
    x, w = ints(rng, (N, H, W, C), -3, 3), ints(rng, (3, 3, C), -2, 2)
    y = O.dwconv3x3(x, w, S)
    dy = ints(rng, y.shape, -3, 3)
    dx, dw = O.dwconv3x3_bwd(x, w, dy, S)
    for a in (x, w, dy, y, dx, dw):
        a.setflags(write=False)
    return dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw, abs=_dw_abs(x, w, dy, S))


@pytest.mark.parametrize("shape", DW_CASES)
def test_dwconv3x3_plain_exact(shape):
    """myolo_dwconv3x3_fwd / _bwd_data / _bwd_weight on x, dy in -3..3, w in -2..2"""
    N, H, W, C, S = shape
    k = dw_plain_case(shape)
    Ho, Wo = k["y"].shape[1:3]
    x, w, dy = dt(k["x"]), dt(k["w"]), dt(k["dy"])
    y, dx, dw = new(N, Ho, Wo, C), new(N, H, W, C), new(3, 3, C)
    X.call("myolo_dwconv3x3_fwd", X.ptr(x), X.ptr(w), X.ptr(y), N, H, W, C, S, X.stream())
    X.call("myolo_dwconv3x3_bwd_data", X.ptr(dy), X.ptr(w), X.ptr(dx), N, H, W, C, S, X.stream())
    X.call("myolo_dwconv3x3_bwd_weight", X.ptr(x), X.ptr(dy), X.ptr(dw), N, H, W, C, S, *ws(), X.stream())
    ay, adx, adw = k["abs"]
    assert_exact(y, k["y"], ay, 1.0, "dw y")
    assert_exact(dx, k["dx"], adx, 1.0, "dw dx")
    assert_exact(dw, k["dw"], adw, 1.0, "dw dw")


def two_tap_filters(rng, C):
    """w [3, 3, C] with two taps of +-1 per channel, at positions drawn per channel: over the channels every tap is used, while |y| stays small enough for
    the sum of y^2 over a whole layer to stay below 2^24 units (the statistics' precondition)"""
    w = np.zeros((9, C), np.float32)
    for j in range(2):
        w[rng.integers(0, 9, C), np.arange(C)] = rng.choice(np.array([-1, 1], np.float32), C)
    return w.reshape(3, 3, C)


# (40, 28, 28, 32, 1) stays with the plain entries: the sum of y^2 over its 31 360 pixels passes 2^24 units
DW_CASES_STATS = [pytest.param(shape, id=i) for i, shape, _ in DW_ROWS[:-1] + DW_GENERIC]


@pytest.mark.parametrize("act", [2, 1], ids=["relu6", "relu"])
@pytest.mark.parametrize("shape", DW_CASES_STATS)
def test_dwconv3x3_input_formed_on_load_exact(shape, act):
    """myolo_dwconv3x3_bnstats_fwd (fused statistics and no_trunk_fusion = 1) and myolo_dwconv3x3_bwd_weight_affine_in (the R6 template flag: ReLU6 and
    ReLU) with the input act(x * in_scale + in_shift) formed on load, ties at 0 and 6 included.  y and its statistics (check_stats) on two-tap filters,
    y once more on full filters, dw (which no filter enters) on the full sum."""
    N, H, W, C, S = shape
    rng = np.random.default_rng(102)
    x, isc, ish, _, a = pre_activation_operands(rng, (N, H, W, C), act)
    g, b, tmm, tmv = bn_params(rng, C)
    wsb = torch.empty(X.dw_bnstats_ws_bytes(N, H, W, C, S), dtype=torch.uint8, device=DEV)
    Ho, Wo = H // S, W // S
    for w, nofuse in ((two_tap_filters(rng, C), 0), (two_tap_filters(rng, C), 1), (ints(rng, (3, 3, C), -2, 2), 0)):
        yref = O.dwconv3x3(a, w, S)
        y, mean, var, scale, shift = new(N, Ho, Wo, C), new(C), new(C), new(C), new(C)
        with X.option("no_trunk_fusion", nofuse):
            X.call("myolo_dwconv3x3_bnstats_fwd", X.ptr(dt(x)), X.ptr(dt(isc)), X.ptr(dt(ish)), act, X.ptr(dt(w)), X.ptr(y), X.ptr(dt(g)), X.ptr(dt(b)),
                   X.ptr(mean), X.ptr(var), X.ptr(scale), X.ptr(shift), X.ptr(tmm), X.ptr(tmv), N, H, W, C, S, 3, wsb.data_ptr(), wsb.numel(), X.stream())
        assert_exact(y, yref, O.dwconv3x3(a, np.abs(w), S), 0.25, "dw y, input formed on load (no_trunk_fusion=%d)" % nofuse)
        if np.abs(w).sum(0).max() <= 2:
            check_stats("dw bnstats (no_trunk_fusion=%d)" % nofuse, yref.reshape(-1, C), g, b, mean, var, scale, shift)
    dy = ints(rng, (N, Ho, Wo, C), -3, 3)
    _, dwref = O.dwconv3x3_bwd(a, w, dy, S)
    _, adw = O.dwconv3x3_bwd(a, w, np.abs(dy), S)
    dw = new(3, 3, C)
    X.call("myolo_dwconv3x3_bwd_weight_affine_in", X.ptr(dt(x)), X.ptr(dt(isc)), X.ptr(dt(ish)), act, X.ptr(dt(dy)), X.ptr(dw), N, H, W, C, S, *ws(), X.stream())
    assert_exact(dw, dwref, adw, 0.25, "dw dw, input formed on load")


@pytest.mark.parametrize("shape", DW_CASES)
def test_dwconv3x3_affine_act_fwd_exact(shape):
    """myolo_dwconv3x3_affine_act_fwd: y = relu6(dwconv(x) * scale + shift), the inference fold, with scale in {1/2, 1, 2} and shift in multiples of 1/4"""
    N, H, W, C, S = shape
    k = dw_plain_case(shape)
    rng = np.random.default_rng(103)
    sc = np.array([0.5, 1.0, 2.0], np.float32)[rng.integers(0, 3, C)]
    sh = (np.float32(0.25) * rng.integers(-8, 9, C)).astype(np.float32)
    ref = act_np(k["y"].astype(np.float64) * sc + sh, 2)
    y = new(*k["y"].shape)
    X.call("myolo_dwconv3x3_affine_act_fwd", X.ptr(dt(k["x"])), X.ptr(dt(k["w"])), X.ptr(dt(sc)), X.ptr(dt(sh)), 2, X.ptr(y), N, H, W, C, S, X.stream())
    assert_exact(y, ref, k["abs"][0] * 2 + 2, 0.25, "dw affine_act y")


@pytest.mark.parametrize("act", [2, 1, 0], ids=["relu6", "relu", "none"])
@pytest.mark.parametrize("shape", DW_CASES)
def test_dwconv3x3_bwd_data_bnsums_exact(shape, act):
    """myolo_dwconv3x3_bwd_data_bnsums + myolo_bn_act_bwd_from_partials (dw_rows_kernel MODE 3 for stride 1, dw_bwd_data_s2_kernel<true> for stride 2 with
    C / 4 <= 64): the conv's dx exact, and dbeta = sum dx * [the BatchNorm's activation passes] exact with the pass decided right at the ties."""
    N, H, W, C, S = shape
    rows = X.dw_bwd_data_bnsums_rows(N, H, W, C, S)
    want_rows = (C % 32 == 0) if S == 1 else (C // 4 <= 64 and 256 % (C // 4) == 0)
    assert (rows > 0) == want_rows
    if not rows:
        return                                  # sizes the fused kernels do not take (the caller runs the two plain calls, covered above and in C)
    k = dw_plain_case(shape)
    rng = np.random.default_rng(104)
    xbn, sc, sh, pre, _ = pre_activation_operands(rng, (N, H, W, C), act)
    mean, var = ints(rng, (C,), -2, 2), ints(rng, (C,), 1, 4)
    M = N * H * W
    part = torch.full((rows * 2 * C,), float("nan"), dtype=torch.float64, device=DEV)
    dx, dbn, dg, db = new(N, H, W, C), new(M, C), new(C), new(C)
    X.call("myolo_dwconv3x3_bwd_data_bnsums", X.ptr(dt(k["dy"])), X.ptr(dt(k["w"])), X.ptr(dx), N, H, W, C, S, X.ptr(dt(xbn)), X.ptr(dt(sc)), X.ptr(dt(sh)),
           X.ptr(dt(mean)), X.ptr(dt(var)), act, X.ptr(part), rows, X.stream())
    X.call("myolo_bn_act_bwd_from_partials", X.ptr(dx), X.ptr(dt(xbn)), X.ptr(dt(mean)), X.ptr(dt(var)), X.ptr(dt(sc)), X.ptr(dt(sh)), X.ptr(dbn), X.ptr(dg), X.ptr(db),
           M, C, act, X.ptr(part), rows, *ws(), X.stream())
    assert_exact(dx, k["dx"], k["abs"][1], 1.0, "dw dx (bnsums)")
    p = pass_np(pre, act)
    assert_exact(db, (k["dx"].astype(np.float64) * p).sum((0, 1, 2)), k["abs"][1].astype(np.float64).sum((0, 1, 2)), 1.0, "dbeta from the conv's partials")


# ============================================================================================================================================
# B. conv1 (3x3 stride 2 on three channels)
# ============================================================================================================================================
def conv1_fwd_rows_ok(H, W, Co):
    cq = Co // 4
    return H % 2 == 0 and W % 4 == 0 and 5 * 3 * W // 4 <= 8 * 256 and 1 <= cq <= 64 and cq & (cq - 1) == 0


def conv1_wgrad_lds_ok(H, W, Co):
    cq = Co // 4
    return 1 <= cq <= 64 and cq & (cq - 1) == 0 and H % 2 == 0 and W % 2 == 0 and W <= 340


# (id, (N, H, W, Cout), forward is the rows kernel, weight gradient is the LDS kernel)
CONV1 = [
    ("conv1_fwd_rows+conv1_wgrad_lds-32x32", (2, 32, 32, 16), True, True),
    ("conv1_fwd_generic-2x2+conv1_wgrad_lds", (1, 2, 2, 4), False, True),
    ("conv1_fwd_rows-wide+OpConv1Dw_colreduce-W400", (1, 6, 400, 256), True, False),
    ("conv1_fwd_rows-widest+OpConv1Dw_colreduce-W544", (1, 4, 544, 8), True, False),
    ("conv1_fwd_generic-W548+OpConv1Dw_colreduce", (1, 4, 548, 8), False, False),
    ("conv1_fwd_generic-W26+conv1_wgrad_lds", (1, 30, 26, 32), False, True),
    ("conv1_fwd_rows+conv1_wgrad_lds-14x16", (2, 14, 16, 8), True, True),
    ("conv1_fwd_rows+conv1_wgrad_lds-3chunks", (3, 36, 20, 64), True, True),
    ("conv1_fwd_generic+OpConv1Dw_colreduce-Cout24", (2, 6, 10, 24), False, False),
]


@pytest.mark.parametrize("cid,shape,rows,lds", CONV1, ids=[c[0] for c in CONV1])
def test_conv1_exact(cid, shape, rows, lds):
    """myolo_conv3x3s2_c3_fwd / _affine_act_fwd / _bnstats_fwd (fused and no_trunk_fusion = 1) / _bwd_weight on x in 0..3 and integer w, dy"""
    N, H, W, Co = shape
    assert conv1_fwd_rows_ok(H, W, Co) == rows and conv1_wgrad_lds_ok(H, W, Co) == lds, "the case id does not name the dispatch"
    rng = np.random.default_rng(105)
    x, w = ints(rng, (N, H, W, 3), 0, 3), ints(rng, (3, 3, 3, Co), -2, 2)
    pads = O.conv1_pads()
    yref = O.conv2d(x, w, stride=2, pads=pads, acc=np.float64)
    ay = O.conv2d(x, np.abs(w), stride=2, pads=pads, acc=np.float64)
    Ho, Wo = H // 2, W // 2
    dy = ints(rng, (N, Ho, Wo, Co), -3, 3)
    _, dwref, _ = O.conv2d_bwd(x, w, dy, stride=2, pads=pads, acc=np.float64, need_dx=False)
    _, adw, _ = O.conv2d_bwd(x, w, np.abs(dy), stride=2, pads=pads, acc=np.float64, need_dx=False)
    y = new(N, Ho, Wo, Co)
    X.call("myolo_conv3x3s2_c3_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(y), N, H, W, Co, X.stream())
    assert_exact(y, yref, ay, 1.0, "conv1 y")
    sc = np.array([0.5, 1.0, 2.0], np.float32)[rng.integers(0, 3, Co)]
    sh = (np.float32(0.25) * rng.integers(-8, 9, Co)).astype(np.float32)
    for act in (2, 1):
        y = new(N, Ho, Wo, Co)
        X.call("myolo_conv3x3s2_c3_affine_act_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(sc)), X.ptr(dt(sh)), act, X.ptr(y), N, H, W, Co, X.stream())
        assert_exact(y, act_np(yref.astype(np.float64) * sc + sh, act), ay * 2 + 2, 0.25, "conv1 affine_act y (act %d)" % act)
    g, b, tmm, tmv = bn_params(rng, Co)
    wsb = torch.empty(X.conv1_bnstats_ws_bytes(N, H, W, Co), dtype=torch.uint8, device=DEV)
    for nofuse in (0, 1):
        y, mean, var, scale, shift = new(N, Ho, Wo, Co), new(Co), new(Co), new(Co), new(Co)
        with X.option("no_trunk_fusion", nofuse):
            X.call("myolo_conv3x3s2_c3_bnstats_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(y), X.ptr(dt(g)), X.ptr(dt(b)), X.ptr(mean), X.ptr(var),
                   X.ptr(scale), X.ptr(shift), X.ptr(tmm), X.ptr(tmv), N, H, W, Co, 3, wsb.data_ptr(), wsb.numel(), X.stream())
        assert_exact(y, yref, ay, 1.0, "conv1 bnstats y (no_trunk_fusion=%d)" % nofuse)
        check_stats("conv1 bnstats (no_trunk_fusion=%d)" % nofuse, yref.reshape(-1, Co), g, b, mean, var, scale, shift)
    dw = new(3, 3, 3, Co)
    X.call("myolo_conv3x3s2_c3_bwd_weight", X.ptr(dt(x)), X.ptr(dt(dy)), X.ptr(dw), N, H, W, Co, *ws(), X.stream())
    assert_exact(dw, dwref, adw, 1.0, "conv1 dw")


# ============================================================================================================================================
# C. column reductions (run_colreduce: colreduce_kernel + colreduce_finish carry every BatchNorm and bias gradient)
# ============================================================================================================================================
def col_geom(M, C):
    """restates col_geom: channel-quad lanes, row lanes, channel groups, rows per slab"""
    q = C // 4
    cl = 1
    while cl * 2 <= q and cl * 2 <= 64:
        cl *= 2
    pl, cgroups = 256 // cl, -(-q // cl)
    rpb = max(-(-M // max(1024 // cgroups, 1)), max(pl * 4, 32))
    return cl, pl, cgroups, rpb


COL_M = [1, 31, 33, 1000, 4099]       # below / above the 32-row slab floor; tails that are no multiple of four rows per lane
COL_C = [4, 12, 24, 40, 256, 1024]    # one quad; quads that are no power of two (cl = 2, 4, 8 of 3, 6, 10); four channel groups


def _col_id(M, C):
    if C % 4:
        return "small_colsum-M%d-C%d" % (M, C)
    cl, pl, cg, rpb = col_geom(M, C)
    return "colreduce-M%d-C%d-cl%d-pl%d-cgroups%d-slab%d" % (M, C, cl, pl, cg, rpb)


def test_colreduce_case_ids_cover_the_paths():
    """the (M, C) grid reaches: lanes beyond the channel count (cl does not divide C/4), several channel groups, several row slabs, a slab whose rows per
    lane are no multiple of four (the tail loop), and a single partial slab"""
    geoms = {(M, C): col_geom(M, C) for M in COL_M for C in COL_C}
    assert any((C // 4) % cl for (M, C), (cl, pl, cg, rpb) in geoms.items())
    assert any(cg == 4 for cl, pl, cg, rpb in geoms.values())
    assert any(M > rpb and M % rpb for (M, C), (cl, pl, cg, rpb) in geoms.items())
    assert any((min(M, rpb) // pl) % 4 or min(M, rpb) % pl for (M, C), (cl, pl, cg, rpb) in geoms.items())
    assert any(min(M, rpb) >= 4 * pl for (M, C), (cl, pl, cg, rpb) in geoms.items())


@pytest.mark.parametrize("M,C", [pytest.param(M, C, id=_col_id(M, C)) for C in COL_C + [27, 35] for M in COL_M])
def test_colsum_exact(M, C):
    x = ints(np.random.default_rng(106), (M, C), -8, 8)
    out = new(C)
    X.call("myolo_colsum", X.ptr(dt(x)), X.ptr(out), M, C, *ws(), X.stream())
    assert_exact(out, x.astype(np.float64).sum(0), np.abs(x).astype(np.float64).sum(0), 1.0, "colsum")


@pytest.mark.parametrize("M,C", [pytest.param(M, C, id=_col_id(M, C)) for C in COL_C for M in COL_M])
def test_bn_stats_from_exact_sums(M, C):
    rng = np.random.default_rng(107)
    x = (ints(rng, (M, C), -8, 8) + ints(rng, (1, C), -4, 4)) * np.float32(0.25)
    g, b, tmm, tmv = bn_params(rng, C)
    mean, var, scale, shift = new(C), new(C), new(C), new(C)
    X.call("myolo_bn_stats", X.ptr(dt(x)), X.ptr(dt(g)), X.ptr(dt(b)), X.ptr(mean), X.ptr(var), X.ptr(scale), X.ptr(shift), X.ptr(tmm), X.ptr(tmv),
           M, C, *ws(), X.stream())
    check_stats("bn_stats", x, g, b, mean, var, scale, shift)


BN_BWD_SHAPES = [(4099, 24), (1000, 256), (33, 1024), (31, 4)]


def _bn_bwd_operands(M, C, act):
    rng = np.random.default_rng(108)
    x, sc, sh, pre, a = pre_activation_operands(rng, (M, C), act)
    sc = (sc * np.where(rng.random(C) < 0.2, -1, 1)).astype(np.float32)        # a negative scale: the pass follows the pre-activation, not x
    pre = x.astype(np.float64) * sc + sh
    dy = ints(rng, (M, C), -3, 3)
    return x, sc, sh, pre, dy, ints(rng, (C,), -2, 2), ints(rng, (C,), 1, 4)


@pytest.mark.parametrize("act", [2, 1, 0], ids=["relu6", "relu", "none"])
@pytest.mark.parametrize("M,C", [pytest.param(M, C, id=_col_id(M, C)) for M, C in BN_BWD_SHAPES])
def test_bn_act_bwd_dbeta_exact_and_pass_mask_at_the_ties(M, C, act):
    """myolo_bn_act_bwd, batch statistics (OpBnBwd) and frozen (OpBnBwdFrozenDx): dbeta = sum dy [pass] exact; the frozen form's dx = scale dy [pass]
    exact, its pass mask compared where dy != 0"""
    x, sc, sh, pre, dy, mean, var = _bn_bwd_operands(M, C, act)
    p = pass_np(pre, act)
    dbref, adb = (dy.astype(np.float64) * p).sum(0), np.abs(dy).astype(np.float64).sum(0)
    for batch in (1, 0):
        dx, dg, db = new(M, C), new(C), new(C)
        X.call("myolo_bn_act_bwd", X.ptr(dt(dy)), X.ptr(dt(x)), X.ptr(dt(sc)), X.ptr(dt(mean)), X.ptr(dt(var)), X.ptr(dt(sc)), X.ptr(dt(sh)),
               X.ptr(dx), X.ptr(dg), X.ptr(db), M, C, act, batch, *ws(), X.stream())
        assert_exact(db, dbref, adb, 1.0, "bn_act_bwd dbeta (batch_stats=%d)" % batch)
        if not batch:
            got = host(dx)
            assert np.array_equal((got != 0)[dy != 0], p[dy != 0]), "the pass mask differs at %s" % np.argwhere(((got != 0) != p) & (dy != 0))[:6].tolist()
            assert_exact(dx, dy.astype(np.float64) * sc * p, np.abs(dy) * 2.0, 0.5, "frozen dx")


@pytest.mark.parametrize("act", [2, 1], ids=["relu6", "relu"])
@pytest.mark.parametrize("M,C", [pytest.param(M, C, id=_col_id(M, C)) for M, C in BN_BWD_SHAPES])
def test_bn_act_bwd_frozen_post_dbeta_exact_and_pass_mask_at_the_ties(M, C, act):
    """myolo_bn_act_bwd_frozen_post (OpBnBwdPost + bn_bwd_dx_post_kernel; the entry point takes ReLU and ReLU6 only): the mask is read off the
    post-activation tensor, which equals 0 and 6 exactly at the ties"""
    x, sc, sh, pre, dy, _, _ = _bn_bwd_operands(M, C, act)
    a = act_np(pre, act).astype(np.float32)
    p = pass_np(pre, act)
    g, b = sc, sh                                           # gamma / beta of xhat = (a - beta) / gamma: only dgamma reads them
    dx, dg, db = new(M, C), new(C), new(C)
    X.call("myolo_bn_act_bwd_frozen_post", X.ptr(dt(dy)), X.ptr(dt(a)), X.ptr(dt(g)), X.ptr(dt(b)), X.ptr(dt(sc)), X.ptr(dx), X.ptr(dg), X.ptr(db),
           M, C, act, *ws(), X.stream())
    assert_exact(db, (dy.astype(np.float64) * p).sum(0), np.abs(dy).astype(np.float64).sum(0), 1.0, "frozen_post dbeta")
    got = host(dx)
    assert np.array_equal((got != 0)[dy != 0], p[dy != 0]), "the pass mask differs at %s" % np.argwhere(((got != 0) != p) & (dy != 0))[:6].tolist()
    assert_exact(dx, dy.astype(np.float64) * sc * p, np.abs(dy) * 2.0, 0.5, "frozen_post dx")


@pytest.mark.parametrize("act", [2, 1, 0], ids=["relu6", "relu", "none"])
@pytest.mark.parametrize("groups,grows,C", [(9, 196, 256), (5, 33, 24), (7, 196, 1024)], ids=["OpBnBwdSparse-9x196-C256", "OpBnBwdSparse-5x33-C24", "OpBnBwdSparse-7x196-C1024"])
def test_bn_bwd_rowsparse_dbeta_exact(groups, grows, C, act):
    """myolo_bn_act_bwd_rowsparse and myolo_bn_bwd_rowsparse_coeffs: dbeta over the compacted row groups (OpBnBwdSparse reads x through idx)"""
    rng = np.random.default_rng(109)
    M = groups * grows
    x, sc, sh, pre, _ = pre_activation_operands(rng, (M, C), act)
    idx = np.sort(rng.choice(groups, size=max(1, groups // 2), replace=False)).astype(np.int32)
    n = len(idx)
    inv = np.full(groups, -1, np.int32)
    inv[idx] = np.arange(n, dtype=np.int32)
    dyc = ints(rng, (n * grows, C), -3, 3)
    rows = (idx[:, None].astype(np.int64) * grows + np.arange(grows)).reshape(-1)
    dbref = (dyc.astype(np.float64) * pass_np(pre[rows], act)).sum(0)
    adb = np.abs(dyc).astype(np.float64).sum(0)
    mean, var = ints(rng, (C,), -2, 2), ints(rng, (C,), 1, 4)
    dx, dg, db = new(M, C), new(C), new(C)
    X.call("myolo_bn_act_bwd_rowsparse", X.ptr(dt(dyc)), X.ptr(dt(x)), X.ptr(dt(idx)), X.ptr(dt(inv)), X.ptr(dt(mean)), X.ptr(dt(var)), X.ptr(dt(sc)), X.ptr(dt(sh)),
           X.ptr(dx), X.ptr(dg), X.ptr(db), M, C, n, grows, act, *ws(), X.stream())
    assert_exact(db, dbref, adb, 1.0, "rowsparse dbeta")
    dg2, db2, ka, kb = new(C), new(C), new(C), new(C)
    X.call("myolo_bn_bwd_rowsparse_coeffs", X.ptr(dt(dyc)), X.ptr(dt(x)), X.ptr(dt(idx)), X.ptr(dt(mean)), X.ptr(dt(var)), X.ptr(dt(sc)), X.ptr(dt(sh)),
           X.ptr(dg2), X.ptr(db2), X.ptr(ka), X.ptr(kb), M, C, n, grows, act, *ws(), X.stream())
    assert_exact(db2, dbref, adb, 1.0, "rowsparse_coeffs dbeta")


# ============================================================================================================================================
# D. ROIAlign
# ============================================================================================================================================
def roi_boxes(rng, B, R):
    """B * R boxes (y1, x1, y2, x2), corners in multiples of 1/8, grouped by image; the last image holds R copies of one box.  oracle._crop_coords and the
    kernels' crop_coord are the same fp32 expression lo (size-1) + idx ((hi-lo) (size-1) / (crop-1)) whatever the sign of hi - lo, so a flipped
    box (y2 < y1: the samples walk upwards) is included."""
    lo = rng.integers(-2, 8, (B * R, 2)) * (rng.random((B * R, 2)) > 0.4)          # four in ten start on pixel 0: every 8 / gcd-th sample of theirs is a tie
    hi = lo + rng.integers(0, 7, (B * R, 2))
    b = (np.concatenate([lo, hi], 1) / 8.0).astype(np.float32)
    fixed = [[0, 0, 1, 1],                      # every sample on a pixel centre, the last ones exactly at size - 1
             [0.375, 0.625, 0.375, 0.625],      # zero size: every sample on one point
             [0.5, 0.125, 0.5, 0.875],          # zero height only
             [0.75, 0.25, 0.25, 0.5],           # flipped: y2 < y1
             [-0.25, -0.25, 1.25, 1.25],        # extrapolation on every side
             [0.5, -0.25, 1.25, 0.75],
             [0, 0, 1, 1]]                      # the full box once more beyond the first 64 boxes (second trip of the ballot loop)
    b[:6] = fixed[:6]
    if R > 64:
        b[R - 1] = fixed[6]
    b[(B - 1) * R:] = [0.125, 0.25, 0.5, 0.875]
    return b


# (id, (B, H, W, C, R, crop), unit of the bilinear weights' products, least share of the valid row samples that must fall exactly on a pixel row: the
# row coordinates are multiples of 1/8 (14 rows, crop 14), 1/4 (9 rows, crop 5), 3/16 (7 rows, crop 5) and 15/64 (16 rows, crop 9: ties are rare))
ROI = [
    ("crop_bwd_grouped_lds-quad1-R70", (2, 14, 14, 256, 70, 14), 2.0 ** -6, 0.1),
    ("crop_bwd_grouped_lds-quad0-R70", (2, 9, 12, 256, 70, 5), 2.0 ** -7, 0.1),
    ("crop_bwd_grouped_lds-quad1-xcd_remap-128wg-R72", (2, 16, 16, 256, 72, 9), 2.0 ** -12, 0.02),
    ("crop_bwd_grouped_generic-C16", (3, 7, 9, 16, 5, 5), 2.0 ** -6, 0.1),
]


@pytest.mark.parametrize("cid,shape,unit,ties", ROI, ids=[c[0] for c in ROI])
def test_roialign_exact(cid, shape, unit, ties):
    """myolo_crop_and_resize_fwd, _bwd_image (fp32 atomics: exact, hence order-free) and myolo_roialign_bwd_grouped on integer features / gradients and boxes
    whose samples fall exactly on pixel centres in a good share; the two backward forms equal each other bit for bit"""
    B, H, W, C, R, crop = shape
    lds = C == 256 and (H * W) % 4 == 0 and R <= 1536
    assert lds == ("lds" in cid) and (not lds or ("quad1" in cid) == (H % 2 == 0 and W % 2 == 0))
    wgs = B * H * W * (C // 4) // 256
    assert ("xcd_remap" in cid) == (lds and wgs % 8 == 0 and wgs >= 64)
    rng = np.random.default_rng(110)
    boxes = roi_boxes(rng, B, R)
    bind = np.repeat(np.arange(B), R).astype(np.int32)
    iny = O._crop_coords(boxes[:, 0], boxes[:, 2], H, crop)
    valid = ~((iny < 0) | (iny > H - 1))
    assert (np.floor(iny) == np.ceil(iny))[valid].mean() >= ties, "too few samples on a pixel row"
    img = ints(rng, (B, H, W, C), -3, 3)
    dout = ints(rng, (B * R, crop, crop, C), -3, 3)
    out = new(B * R, crop, crop, C)
    X.call("myolo_crop_and_resize_fwd", X.ptr(dt(img)), X.ptr(dt(boxes)), X.ptr(dt(bind)), X.ptr(out), B, H, W, C, B * R, crop, crop, X.stream())
    assert_exact(out, O.crop_and_resize(img, boxes, bind, (crop, crop)), np.array([4.0 * np.abs(img).max()]), unit, "crop fwd")
    ref = O.crop_and_resize_bwd_image(dout, boxes, bind, (B, H, W, C))
    aref = O.crop_and_resize_bwd_image(np.abs(dout), boxes, bind, (B, H, W, C))
    d1, d2 = new(B, H, W, C), new(B, H, W, C)
    X.call("myolo_crop_and_resize_bwd_image", X.ptr(dt(dout)), X.ptr(dt(boxes)), X.ptr(dt(bind)), X.ptr(d1), B, H, W, C, B * R, crop, crop, X.stream())
    X.call("myolo_roialign_bwd_grouped", X.ptr(dt(dout)), X.ptr(dt(boxes)), X.ptr(d2), B, H, W, C, R, crop, crop, X.stream())
    assert_exact(d1, ref, aref, unit, "crop bwd_image")
    assert_exact(d2, ref, aref, unit, "roialign bwd grouped")
    assert torch.equal(d1, d2)


@pytest.mark.parametrize("C", [256, 16], ids=["crop_bwd_grouped_lds-tiny_box", "crop_bwd_grouped_generic-tiny_box"])
def test_roialign_tiny_box_exact(C):
    """a box 2^-10 tall and wide (1 / step = 1024: a live window, above the kernels' 1e-6 degeneracy threshold) next to a zero-size one.  Its weights
    are multiples of 2^-10, their products of 2^-20: exact while sum|terms| < 16, so its gradient crop is sparse (one sample in sixteen)."""
    B, H, W, R, crop = 1, 14, 14, 3, 14
    t = 2.0 ** -10
    boxes = np.array([[0.375, 0.5, 0.375 + t, 0.5 + t], [0.375, 0.5, 0.375, 0.5], [0.625 + t, 0.25 + t, 0.625, 0.25]], np.float32)
    bind = np.zeros(R, np.int32)
    rng = np.random.default_rng(111)
    img = ints(rng, (B, H, W, C), -3, 3)
    dout = ints(rng, (R, crop, crop, C), -1, 1) * (rng.random((R, crop, crop, 1)) < 0.0625)
    dout[1] = 0
    dout[1, 3, 5] = 1
    dout = dout.astype(np.float32)
    out = new(R, crop, crop, C)
    X.call("myolo_crop_and_resize_fwd", X.ptr(dt(img)), X.ptr(dt(boxes)), X.ptr(dt(bind)), X.ptr(out), B, H, W, C, R, crop, crop, X.stream())
    assert_exact(out, O.crop_and_resize(img, boxes, bind, (crop, crop)), np.array([4.0 * np.abs(img).max()]), t * t, "crop fwd")
    ref = O.crop_and_resize_bwd_image(dout, boxes, bind, (B, H, W, C))
    aref = O.crop_and_resize_bwd_image(np.abs(dout), boxes, bind, (B, H, W, C))
    d1, d2 = new(B, H, W, C), new(B, H, W, C)
    X.call("myolo_crop_and_resize_bwd_image", X.ptr(dt(dout)), X.ptr(dt(boxes)), X.ptr(dt(bind)), X.ptr(d1), B, H, W, C, R, crop, crop, X.stream())
    X.call("myolo_roialign_bwd_grouped", X.ptr(dt(dout)), X.ptr(dt(boxes)), X.ptr(d2), B, H, W, C, R, crop, crop, X.stream())
    assert_exact(d1, ref, aref, t * t, "crop bwd_image")
    assert_exact(d2, ref, aref, t * t, "roialign bwd grouped")


# ============================================================================================================================================
# E. the mask head's 1x1 conv, backward
# ============================================================================================================================================
@pytest.mark.parametrize("C", [1, 3, 4, 8], ids=lambda c: "OpMaskOutBwd<%d>_colreduce" % c)
def test_mask_head_out_bwd_exact(C):
    """myolo_mask_head_out_bwd: dx = (dz w^T) [x > 0], dw = x^T dz, db = sum dz on integer x >= 0 with exact zeros, integer w and dz"""
    rng = np.random.default_rng(112)
    M, Cin = 6 * 784, 256
    x = np.maximum(ints(rng, (M, Cin), -3, 3), 0)
    assert (x == 0).mean() >= 0.1
    w, dz = ints(rng, (Cin, C), -2, 2), ints(rng, (M, C), -2, 2)
    dx, dw, db = new(M, Cin), new(Cin, C), new(C)
    X.call("myolo_mask_head_out_bwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(dz)), X.ptr(dx), X.ptr(dw), X.ptr(db), M, Cin, C, *ws(), X.stream())
    x64, w64, dz64 = x.astype(np.float64), w.astype(np.float64), dz.astype(np.float64)
    assert_exact(dx, (dz64 @ w64.T) * (x > 0), np.abs(dz64) @ np.abs(w64).T, 1.0, "mask out dx")
    assert_exact(dw, x64.T @ dz64, x64.T @ np.abs(dz64), 1.0, "mask out dw")
    assert_exact(db, dz64.sum(0), np.abs(dz64).sum(0), 1.0, "mask out db")


@pytest.mark.parametrize("C,ids", [(81, [2, 0, 80, 2, 5, 0]), (8, [2, 0, 7, 2, 5, 0])], ids=["mask_out_bwd_sel-C81", "mask_out_bwd_sel-C8+OpMaskOutBwd<8>"])
def test_mask_head_out_bwd_sel_exact(C, ids):
    """myolo_mask_head_out_bwd_sel: the gradient of the selected class's logit only; ids include 0 (background: no gradient) and leave classes without a
    ROI, whose columns of dw / db must be exactly zero.  At C = 8 the dense entry on the one-hot dz must agree bit for bit."""
    rng = np.random.default_rng(113)
    hw, Cin = 784, 256
    NR = len(ids)
    M = NR * hw
    ids = np.array(ids, np.int32)
    x = np.maximum(ints(rng, (M, Cin), -3, 3), 0)
    w = ints(rng, (Cin, C), -2, 2)
    dzs = ints(rng, (M,), -2, 2) * np.repeat(ids > 0, hw)
    dz = np.zeros((M, C), np.float64)
    dz[np.arange(M), np.repeat(ids, hw)] = dzs
    dz[:, 0] = 0
    dx, dw, db = new(M, Cin), new(Cin, C), new(C)
    wsb = torch.empty(max(X.mask_bwd_sel_ws_bytes(NR, Cin), 256), dtype=torch.uint8, device=DEV)
    X.call("myolo_mask_head_out_bwd_sel", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(dzs.astype(np.float32))), X.ptr(dt(ids)), X.ptr(dx), X.ptr(dw), X.ptr(db),
           M, Cin, C, hw, wsb.data_ptr(), wsb.numel(), X.stream())
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    assert_exact(dx, (dz @ w64.T) * (x > 0), np.abs(dz) @ np.abs(w64).T, 1.0, "mask sel dx")
    assert_exact(dw, x64.T @ dz, x64.T @ np.abs(dz), 1.0, "mask sel dw")
    assert_exact(db, dz.sum(0), np.abs(dz).sum(0), 1.0, "mask sel db")
    absent = np.setdiff1d(np.arange(C), ids[ids > 0])
    assert not host(dw)[:, absent].any() and not host(db)[absent].any()
    if C <= 8:
        dx2, dw2, db2 = new(M, Cin), new(Cin, C), new(C)
        X.call("myolo_mask_head_out_bwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(dz.astype(np.float32))), X.ptr(dx2), X.ptr(dw2), X.ptr(db2), M, Cin, C, *ws(), X.stream())
        torch.cuda.synchronize()
        assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)

"""Every fp32 matrix product of the training step held to an fp32 error bound against a float64 reference of the SAME fp32 operands.

FP32_MATMUL = "bf16x6" (library switch wino_x6, csrc/wino_mm.hip) forms each fp32 product from six exact bf16 piece products accumulated in
fp32 on the bf16 matrix pipe; the native kernels use the fp32 matrix pipe or VALU fma.  Three checks, each written once below:

  (a) componentwise: |got - ref| <= 4 K 2^-24 (|A| |B|) per output element, K = reduction depth, |A| |B| in float64, plus the rounding terms
      of the epilogue (bias / affine / sigmoid) and of an A operand formed on load (BatchNorm affine + activation);
  (b) normwise: max|err| / max|ref| <= 2e-6 sqrt(K / 256) for GEMM-shaped products; 5e-5 for the F(4,3) operators; a measured bound for F(6,3);
  (c) bf16x6 against its native twin (the same call with the split path switched off): rms error <= 1.05 x, max error <= 1.25 x the native
      one, and the two results are not bit-identical (the case did reach the split kernel).

The library options force each kernel onto small shapes (pw_x6_min_rows, x6_no_half_tiles, tn_wgs, pw_no_smallm, gemm_generic, no_splitk)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from myolo import _ext as X      # noqa: E402

DEV = "cuda:0"
U24 = 2.0 ** -24
_KEEP = []


@pytest.fixture(autouse=True)
def _keepalive():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dt(a):
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
    _KEEP.append(t)
    return t


def new(*shape):
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    _KEEP.append(t)
    return t


def wsbuf(nbytes=512 << 20):
    """a workspace of at least nbytes (one shared buffer: every call here runs on the one stream)"""
    if getattr(wsbuf, "buf", None) is None or wsbuf.buf.numel() < nbytes:
        wsbuf.buf = torch.empty(max(int(nbytes), 512 << 20), dtype=torch.uint8, device=DEV)
    return wsbuf.buf.data_ptr(), wsbuf.buf.numel()


def f64(t):
    if torch.is_tensor(t):
        torch.cuda.synchronize()
        t = t.detach().cpu().numpy()
    return np.asarray(t, np.float64)


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


@contextlib.contextmanager
def options(**kv):
    """library switches for the block, the previous values restored on exit (also when the block raises)"""
    with contextlib.ExitStack() as st:
        for k, v in kv.items():
            st.enter_context(X.option(k, v))
        yield


def act_np(v, act):
    return np.clip(v, 0, 6) if act == 2 else (np.maximum(v, 0) if act == 1 else v)


def formed_on_load(x, sc, sh, act):
    """the A operand the kernels form on load: mm_act(fmaf(x, sc, sh)) -- one rounding of the exact float64 value to fp32, then the activation"""
    return act_np((x.astype(np.float64) * sc + sh).astype(np.float32), act)


# ---- the three checks ----------------------------------------------------------------------------------------------------------------------
def check_a(got, ref, absdot, K, extra=0.0, what=""):
    """(a) |got - ref| <= 4 K 2^-24 absdot + extra, element by element (extra: the epilogue's / prologue's rounding terms)"""
    got = f64(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite output" % what
    err = np.abs(got - ref)
    bound = 4.0 * K * U24 * absdot + extra
    bad = err > bound
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert not bad.any(), "%s: %d of %d elements beyond the componentwise fp32 bound (worst err / bound %.3g, first at %s)" % (
        what, int(bad.sum()), bad.size, worst, np.argwhere(bad)[0].tolist())
    return worst


def errs(got, ref):
    """max and rms of |got - ref|, both relative to max|ref|"""
    e = np.abs(f64(got) - ref)
    s = float(np.abs(ref).max())
    return float(e.max()) / s, float(np.sqrt(np.mean(e ** 2))) / s


def gemm_tol(K):
    return 2e-6 * (K / 256.0) ** 0.5


def check_b(got, ref, tol, what=""):
    """(b) max|err| / max|ref| <= tol"""
    mx, rms = errs(got, ref)
    assert mx <= tol, "%s: normwise error %.3e > %.3e" % (what, mx, tol)
    return mx, rms


C_MIN_VALUES = 1024     # (c)'s rms / max ratios need this many outputs: on 60-840 values the rms of two sets of roundings differs by 5-11 % by chance


def check_c(x6, nat, ref, what="", seq=None):
    """(c) the bf16x6 result against the native one of the same call on the same operands: not bit-identical (the call did reach the split kernel);
    rms <= 1.05 x and max <= 1.25 x the native error.  seq: where the switched-off call runs a kernel that sums K in another order (pw_smallm_kernel's
    four K slices, split-K gemm_nn_fast, gemm_tn_fast's row split), the ratios are taken against the fp32 kernel with the split kernel's summation
    order instead -- myolo_matmul_f32's native product (wino_mm_kernel: the same 128-row tiles, the same 16-deep K steps in one chain) on the same
    fp32 operands.  Measured: against a K-splitting twin a single chain is 1.1-3x its rms by design, at the fp32 level of (a) and (b) all the same."""
    (mx6, r6), (mxn, rn) = errs(x6, ref), errs(nat, ref)
    line = "%s: native max %.3e rms %.3e | bf16x6 max %.3e rms %.3e" % (what, mxn, rn, mx6, r6)
    if seq is not None:
        mxn, rn = errs(seq, ref)
        line += " | fp32 same order max %.3e rms %.3e" % (mxn, rn)
    print(line)
    assert not torch.equal(x6, nat), "%s: bit-identical to the native kernel -- the case did not reach the bf16x6 kernel" % what
    if ref.size < C_MIN_VALUES:
        return
    assert r6 <= 1.05 * rn, "%s: bf16x6 rms %.3e > 1.05 x native %.3e" % (what, r6, rn)
    assert mx6 <= 1.25 * mxn, "%s: bf16x6 max %.3e > 1.25 x native %.3e" % (what, mx6, mxn)


def seq_matmul(A, B):
    """C = A B with myolo_matmul_f32's fp32 kernel (the same-order twin of check_c); K padded with zero columns / rows to a multiple of 16 (exact)"""
    M, K = A.shape
    Kp = (K + 15) // 16 * 16
    Ap, Bp = np.zeros((M, Kp), np.float32), np.zeros((Kp, B.shape[1]), np.float32)
    Ap[:, :K], Bp[:K] = A, B
    return f64(_matmul(dt(Ap), dt(Bp), X.PRODUCTS_NATIVE, 0))


def adversarial(rng, m, K, n):
    """P [m][K], Q [K][n] for C = P Q: magnitudes 2^-20 .. 2^20 inside one dot product, all-zero row 1 / column 2, row 3 x column 4 cancels
    pairwise (exact sum 0), row 5 = 1 + 2^-23 against column 6 = 1 - 2^-24 (the third bf16 piece of both operands matters)"""
    assert K % 2 == 0 and m >= 6 and n >= 7
    P = (rng.standard_normal((m, K)) * 2.0 ** rng.integers(-20, 21, size=(m, K))).astype(np.float32)
    Q = (rng.standard_normal((K, n)) * 2.0 ** rng.integers(-20, 21, size=(K, n))).astype(np.float32)
    P[1] = 0
    Q[:, 2] = 0
    P[3, 1::2] = -P[3, 0::2]
    Q[1::2, 4] = Q[0::2, 4]
    P[5] = np.float32(1.0) + np.float32(2.0 ** -23)
    Q[:, 6] = np.float32(1.0) - np.float32(2.0 ** -24)
    return P, Q


def check_adversarial(C, P, Q, what):
    """(a) on an adversarial() product; zero rows / columns exactly 0, the cancelling pair and the 1 +- ulp pair inside the bound"""
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    ref, absdot = P64 @ Q64, np.abs(P64) @ np.abs(Q64)
    K = P.shape[1]
    check_a(C, ref, absdot, K, what=what)
    c = f64(C)
    assert (c[1] == 0).all() and (c[:, 2] == 0).all(), "%s: zero row / column not exactly 0" % what
    assert abs(c[3, 4]) <= 4 * K * U24 * absdot[3, 4], what
    assert abs(c[5, 6] - ref[5, 6]) <= 4 * K * U24 * absdot[5, 6], what


# ---- plain products: myolo_matmul_f32 ------------------------------------------------------------------------------------------------------
def _matmul(A, B, products, b_is_nk):
    M, K = A.shape
    N = B.shape[0] if b_is_nk else B.shape[1]
    C = new(M, N)
    X.call("myolo_matmul_f32", X.ptr(A), X.ptr(B), X.ptr(C), M, K, N, b_is_nk, products, *wsbuf(max(256, X.matmul_ws_bytes(K, N, b_is_nk, products))),
           X.stream())
    torch.cuda.synchronize()
    return C


@pytest.mark.parametrize("M,K,N,b_is_nk,full", [(1, 16, 256, 1, 0), (129, 272, 512, 0, 0), (129, 16, 768, 1, 1), (300, 272, 768, 0, 1),
                                                (8193, 256, 1024, 1, 0)])       # the last: 260 tiles, the full-tile kernel by itself
def test_matmul_f32(M, K, N, b_is_nk, full):
    """wino_mm_x6_kernel<PLAIN>: the 128 x 128 half tiles (fewer than 256 tiles) and the 128 x 256 full tiles (x6_no_half_tiles = 1, or >= 256
    tiles); M = 1 and ragged row tiles, K = 16 and K % 256 != 0, B given as [N][K] and as [K][N]; against float64 and the native kernel"""
    rng = np.random.default_rng(M + K + N)
    A, Bnk = rnd(rng, M, K, scale=2.0), rnd(rng, N, K, scale=0.05)
    A64, B64 = A.astype(np.float64), Bnk.astype(np.float64).T
    ref, absdot = A64 @ B64, np.abs(A64) @ np.abs(B64)
    At, Bt = dt(A), dt(Bnk if b_is_nk else Bnk.T)
    out = {}
    with options(x6_no_half_tiles=full):
        for prod in (X.PRODUCTS_NATIVE, X.PRODUCTS_BF16X6):
            out[prod] = _matmul(At, Bt, prod, b_is_nk)
            check_a(out[prod], ref, absdot, K, what="matmul products=%d" % prod)
            check_b(out[prod], ref, gemm_tol(K), what="matmul products=%d" % prod)
    check_c(out[X.PRODUCTS_BF16X6], out[X.PRODUCTS_NATIVE], ref, "matmul M=%d K=%d N=%d b_is_nk=%d full=%d" % (M, K, N, b_is_nk, full))


@pytest.mark.parametrize("b_is_nk,full", [(1, 0), (0, 1)])
def test_matmul_f32_adversarial(b_is_nk, full):
    rng = np.random.default_rng(7 + b_is_nk)
    M, K, N = 129, 272, 512
    P, Q = adversarial(rng, M, K, N)
    At, Bt = dt(P), dt(Q.T if b_is_nk else Q)
    with options(x6_no_half_tiles=full):
        for prod in (X.PRODUCTS_NATIVE, X.PRODUCTS_BF16X6):
            check_adversarial(_matmul(At, Bt, prod, b_is_nk), P, Q, "adversarial matmul products=%d" % prod)


# ---- pointwise forward with BatchNorm applied on load and statistics in the epilogue (wino_mm_x6_kernel<PLAIN, true>) ------------------------
def _pw_bnstats(x, sc, sh, act, w, M, Cin, Cout):
    y = new(M, Cout)
    g, b = dt(np.ones(Cout)), dt(np.zeros(Cout))
    mean, var, scale, shift, mm, mv = new(Cout), new(Cout), new(Cout), new(Cout), dt(np.zeros(Cout)), dt(np.ones(Cout))
    X.call("myolo_pwconv1x1_bnstats_fwd", X.ptr(x), X.ptr(sc) if sc is not None else None, X.ptr(sh) if sh is not None else None, act, X.ptr(w),
           X.ptr(y), X.ptr(g), X.ptr(b), X.ptr(mean), X.ptr(var), X.ptr(scale), X.ptr(shift), X.ptr(mm), X.ptr(mv), M, Cin, Cout, 3,
           *wsbuf(X.pw_bnstats_ws_bytes(M, Cin, Cout)), X.stream())
    torch.cuda.synchronize()
    return y, mean, var


def _check_stats(y, mean, var, what):
    """the epilogue's statistics against float64 of the kernel's own y (fp32 partial sums of <= 128 rows per tile, then double)"""
    y64 = f64(y)
    mu, v = y64.mean(0), y64.var(0)
    assert np.all(np.abs(f64(mean) - mu) <= 256 * U24 * np.abs(y64).mean(0) + 1e-30), what + ": batch mean"
    assert np.all(np.abs(f64(var) - v) <= 1024 * U24 * (y64 ** 2).mean(0) + U24 * v), what + ": batch variance"


@pytest.mark.parametrize("M,Cin,Cout,act,full", [(1000, 256, 256, 2, 0), (1000, 272, 512, 1, 1), (300, 256, 768, 0, 0), (129, 512, 256, 2, 1),
                                                 (8193, 256, 1024, 2, 0)])
def test_pw_bnstats_fwd_x6(M, Cin, Cout, act, full):
    """myolo_pwconv1x1_bnstats_fwd under "wino_x6": A = act(fmaf(x, in_scale, in_shift)) formed on load with inputs straddling 0 and 6, NU = 2
    (half tiles) and NU = 4, ragged M; y to (a) / (b) / (c) (native twin: pw_no_x6 = 1), the batch statistics against the kernel's own y"""
    rng = np.random.default_rng(M * 7 + Cout)
    x = rnd(rng, M, Cin, scale=3.0)
    isc, ish = 1 + rnd(rng, Cin, scale=0.3), 3 + rnd(rng, Cin, scale=1.0)
    w = rnd(rng, Cin, Cout, scale=0.1)
    a = formed_on_load(x, isc, ish, act).astype(np.float64)
    assert (a <= 0).any() and (act != 2 or (a >= 6).any())
    w64 = w.astype(np.float64)
    ref, absdot = a @ w64, np.abs(a) @ np.abs(w64)
    xt, sct, sht, wt = dt(x), dt(isc), dt(ish), dt(w)
    out = {}
    for no in (1, 0):
        with options(wino_x6=1, pw_x6_min_rows=1, x6_no_half_tiles=full, pw_no_x6=no):
            y, mean, var = _pw_bnstats(xt, sct, sht, act, wt, M, Cin, Cout)
        what = "pw bnstats fwd %s M=%d act=%d" % ("native" if no else "bf16x6", M, act)
        check_a(y, ref, absdot, Cin, extra=U24 * absdot, what=what)
        check_b(y, ref, gemm_tol(Cin), what=what)
        _check_stats(y, mean, var, what)
        out[no] = y
    check_c(out[0], out[1], ref, "pw bnstats fwd M=%d Cin=%d Cout=%d act=%d full=%d" % (M, Cin, Cout, act, full), seq=seq_matmul(a.astype(np.float32), w))


def test_pw_bnstats_fwd_x6_adversarial():
    rng = np.random.default_rng(17)
    M, Cin, Cout = 1000, 272, 512
    P, Q = adversarial(rng, M, Cin, Cout)
    for full in (0, 1):
        with options(wino_x6=1, pw_x6_min_rows=1, x6_no_half_tiles=full):
            y, _, _ = _pw_bnstats(dt(P), None, None, 0, dt(Q), M, Cin, Cout)
        check_adversarial(y, P, Q, "adversarial pw bnstats fwd full=%d" % full)


# ---- pointwise data gradient on wino_mm_x6_kernel (w is the [N][K] operand) ----------------------------------------------------------------
@pytest.mark.parametrize("M,Cin,Cout", [(4097, 256, 48), (4100, 512, 272), (4099, 768, 16)])
def test_pw_bwd_data_x6(M, Cin, Cout):
    rng = np.random.default_rng(M + Cin)
    dy, w = rnd(rng, M, Cout), rnd(rng, Cin, Cout, scale=0.1)
    d64, w64 = dy.astype(np.float64), w.astype(np.float64)
    ref, absdot = d64 @ w64.T, np.abs(d64) @ np.abs(w64).T
    dyt, wt = dt(dy), dt(w)
    out = {}
    for no in (1, 0):
        dx = new(M, Cin)
        with options(wino_x6=1, pw_no_x6=no):
            X.call("myolo_pwconv1x1_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(dx), M, Cin, Cout, *wsbuf(), X.stream())
        what = "pw dx %s M=%d Cin=%d Cout=%d" % ("native" if no else "bf16x6", M, Cin, Cout)
        check_a(dx, ref, absdot, Cout, what=what)
        check_b(dx, ref, gemm_tol(Cout), what=what)
        out[no] = dx
    check_c(out[0], out[1], ref, "pw dx M=%d Cin=%d Cout=%d" % (M, Cin, Cout), seq=seq_matmul(dy, w.T))


def test_pw_bwd_data_x6_adversarial():
    rng = np.random.default_rng(19)
    M, Cin, Cout = 4097, 256, 272
    P, Q = adversarial(rng, M, Cout, Cin)                 # dx = dy w^T: P = dy, Q = w^T
    dx = new(M, Cin)
    with options(wino_x6=1):
        X.call("myolo_pwconv1x1_bwd_data", X.ptr(dt(P)), X.ptr(dt(Q.T)), X.ptr(dx), M, Cin, Cout, *wsbuf(), X.stream())
    check_adversarial(dx, P, Q, "adversarial pw dx")


# ---- weight gradients on wino_tn_x6_kernel<false> + tn_x6_reduce_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("M,Cin,Cout,act,wgs", [(4097, 256, 256, None, None), (25101, 512, 256, 2, None), (4097, 256, 512, 1, 8), (25, 256, 256, 0, 0),
                                                (1000, 256, 256, 2, 3)])
def test_pw_bwd_weight_x6(M, Cin, Cout, act, wgs):
    """dw = A^T dy, K = M rows: rows not a multiple of 16 nor of the split, several split-K slices, tn_wgs small enough for several launches
    (unit_base != 0) and 0 (one launch); act: myolo_pwconv1x1_bwd_weight_affine_in with A = act(fmaf(x, sc, sh)) formed on load"""
    rng = np.random.default_rng(M + Cout)
    x, dy = rnd(rng, M, Cin, scale=2.0), rnd(rng, M, Cout)
    if act is None:
        a = x.astype(np.float64)
    else:
        isc, ish = 1 + rnd(rng, Cin, scale=0.3), 3 + rnd(rng, Cin, scale=1.0)
        a = formed_on_load(x, isc, ish, act).astype(np.float64)
        sct, sht = dt(isc), dt(ish)
    d64 = dy.astype(np.float64)
    ref, absdot = a.T @ d64, np.abs(a).T @ np.abs(d64)
    xt, dyt = dt(x), dt(dy)
    out = {}
    for no in (1, 0):
        dw = new(Cin, Cout)
        opts = dict(wino_x6=1, pw_x6_min_rows=1, pw_no_x6=no)
        if wgs is not None:
            opts["tn_wgs"] = wgs
        with options(**opts):
            if act is None:
                X.call("myolo_pwconv1x1_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(dw), M, Cin, Cout, *wsbuf(), X.stream())
            else:
                X.call("myolo_pwconv1x1_bwd_weight_affine_in", X.ptr(xt), X.ptr(sct), X.ptr(sht), act, X.ptr(dyt), X.ptr(dw), M, Cin, Cout, *wsbuf(),
                       X.stream())
        what = "pw dw %s M=%d Cin=%d Cout=%d act=%s" % ("native" if no else "bf16x6", M, Cin, Cout, act)
        check_a(dw, ref, absdot, M, extra=0 if act is None else U24 * absdot, what=what)
        check_b(dw, ref, gemm_tol(M), what=what)
        out[no] = dw
    check_c(out[0], out[1], ref, "pw dw M=%d Cin=%d Cout=%d act=%s tn_wgs=%s" % (M, Cin, Cout, act, wgs), seq=seq_matmul(a.T.astype(np.float32), dy))


def test_pw_bwd_weight_x6_adversarial():
    rng = np.random.default_rng(23)
    M, Cin, Cout = 4098, 256, 256
    P, Q = adversarial(rng, Cin, M, Cout)                 # dw = x^T dy: P = x^T, Q = dy
    dw = new(Cin, Cout)
    with options(wino_x6=1, tn_wgs=8):
        X.call("myolo_pwconv1x1_bwd_weight", X.ptr(dt(P.T)), X.ptr(dt(Q)), X.ptr(dw), M, Cin, Cout, *wsbuf(), X.stream())
    check_adversarial(dw, P, Q, "adversarial pw dw")


# ---- Winograd multiply stages: V[q] U[q] on plain operands -------------------------------------------------------------------------------------
def _wino43_runs(N, H, W):
    """(row offset, rows, first plane, planes) of the plane groups of the F(4,3) tiling with F(2,3) on a ragged last tile row / column
    (csrc/wino_kernels.hip geom(): 16 / 8 / 8 / 4 points with all / fewer columns / fewer rows / both)"""
    TH, TW = (H + 3) // 4, (W + 3) // 4
    redv = 1 if TH > 1 and H - 4 * (TH - 1) <= 2 else 0
    redh = 1 if TW > 1 and W - 4 * (TW - 1) <= 2 else 0
    out, at, q = [], 0, 0
    for k, cnt in enumerate((16, 8, 8, 4)):
        rows = N * (TH - (redv if k & 2 else 0)) * (TW - (redh if k & 1 else 0))
        out.append((at, rows, q, cnt))
        at += rows * cnt
        q += cnt
    assert at == X.wino_plane_elems(N, H, W, 1)
    return out


def _wino63_runs(N):
    return [(0, 9 * N, 0, 36), (36 * 9 * N, 3 * N, 36, 24), (36 * 9 * N + 24 * 3 * N, N, 60, 4)]


def _planes_ref(V, U, runs):
    """M = V[q] U[q] plane by plane in float64, and |V| |U|"""
    V64, U64 = V.astype(np.float64), U.astype(np.float64)
    ref = np.zeros((V.shape[0], U.shape[2]))
    absdot = np.zeros_like(ref)
    for r0, rows, q0, nq in runs:
        for j in range(nq):
            sl = slice(r0 + j * rows, r0 + (j + 1) * rows)
            ref[sl] = V64[sl] @ U64[q0 + j]
            absdot[sl] = np.abs(V64[sl]) @ np.abs(U64[q0 + j])
    return ref, absdot


def _adversarial_planes(rng, V, w):
    """adversarial operands for a multiply stage: V rows spanning 2^-20 .. 2^20, an all-zero row, 1 + 2^-23 rows, rows cancelling pairwise against
    output column 4 (filters of input channels 2j and 2j+1 equal there: so are their transformed values); output column 2 all zero"""
    V *= (2.0 ** rng.integers(-20, 21, size=V.shape)).astype(np.float32)
    V[1] = 0
    V[5] = np.float32(1.0) + np.float32(2.0 ** -23)
    V[3, 1::2] = -V[3, 0::2]
    w *= (2.0 ** rng.integers(-10, 11, size=(1, 1, w.shape[2], 1))).astype(np.float32)
    w[..., 2] = 0
    w[:, :, 1::2, 4] = w[:, :, 0::2, 4]


@pytest.mark.parametrize("N,H,W,Cin,Cout,adv", [(5, 14, 14, 256, 256, False), (4, 13, 11, 272, 256, False), (3, 14, 14, 256, 512, True)])
def test_wino43_multiply(N, H, W, Cin, Cout, adv):
    """myolo_wino_multiply: the 36 planes of a mixed tiling (14 x 14: three runs of plane heights in one gemm_nt_batched_runs launch; 13 x 11: two)
    against float64 of the plain [36][K][N] operands (wino_no_bt = 1 gives them), x6 against the fp32-MFMA kernel (wino_x6 = 0)"""
    rng = np.random.default_rng(N * H + Cin)
    runs = _wino43_runs(N, H, W)
    V = rnd(rng, runs[-1][0] + runs[-1][1] * runs[-1][3], Cin, scale=3.0)
    w = rnd(rng, 3, 3, Cin, Cout, scale=0.05)
    if adv:
        _adversarial_planes(rng, V, w)
    wt, Vt = dt(w), dt(V)
    st = X.stream()
    with options(wino_x6=0, wino_no_bt=1):
        Up = new(X.wino_u_elems(Cin, Cout))
        X.call("myolo_wino_weight_transform", X.ptr(wt), X.ptr(Up), Cin, Cout, 0, st)
    U = f64(Up)[:36 * Cin * Cout].reshape(36, Cin, Cout)
    ref, absdot = _planes_ref(V, U, runs)
    out = {}
    for x6 in (0, 1):
        with options(wino_x6=x6):
            Ut, Mt = new(X.wino_u_elems(Cin, Cout)), new(V.shape[0], Cout)
            X.call("myolo_wino_weight_transform", X.ptr(wt), X.ptr(Ut), Cin, Cout, 0, st)
            X.call("myolo_wino_multiply", X.ptr(Vt), X.ptr(Ut), X.ptr(Mt), N, H, W, Cin, Cout, st)
            if x6 == 0:        # the transposed fp32 layout holds the same values
                assert np.array_equal(f64(Ut)[:36 * Cin * Cout].reshape(36, Cout, Cin).transpose(0, 2, 1), U)
        what = "F(4,3) multiply %s" % ("bf16x6" if x6 else "native")
        if adv:
            check_a(Mt, ref, absdot, Cin, what="adversarial " + what)
            m = f64(Mt)
            assert (m[1] == 0).all() and (m[:, 2] == 0).all()
        else:
            check_a(Mt, ref, absdot, Cin, what=what)
            check_b(Mt, ref, gemm_tol(Cin), what=what)
        out[x6] = Mt
    if not adv:
        check_c(out[1], out[0], ref, "F(4,3) multiply N=%d %dx%d Cin=%d Cout=%d" % (N, H, W, Cin, Cout))


@pytest.mark.parametrize("N,Cin,Cout,adv", [(5, 256, 256, False), (3, 320, 512, False), (2, 256, 256, True)])
def test_wino63_multiply(N, Cin, Cout, adv):
    """myolo_wino63_multiply: 64 planes in three runs (9N / 3N / N rows: ragged row tiles) against float64 of the plain operands (the fp32
    transposed layout of wino_x6 = 0, read back), x6 against the fp32-MFMA kernel"""
    rng = np.random.default_rng(N * 3 + Cin)
    runs = _wino63_runs(N)
    V = rnd(rng, X.wino63_plane_elems(N, 1), Cin, scale=3.0)
    w = rnd(rng, 3, 3, Cin, Cout, scale=0.05)
    if adv:
        _adversarial_planes(rng, V, w)
    wt, Vt = dt(w), dt(V)
    st = X.stream()
    out, U = {}, None
    for x6 in (0, 1):
        with options(wino_x6=x6):
            Ut, Mt = new(X.wino63_u_elems(Cin, Cout)), new(V.shape[0], Cout)
            X.call("myolo_wino63_weight_transform", X.ptr(wt), X.ptr(Ut), Cin, Cout, st)
            X.call("myolo_wino63_multiply", X.ptr(Vt), X.ptr(Ut), X.ptr(Mt), N, Cin, Cout, st)
        if x6 == 0:
            U = f64(Ut)[:64 * Cin * Cout].reshape(64, Cout, Cin).transpose(0, 2, 1)
            ref, absdot = _planes_ref(V, U, runs)
        what = "F(6,3) multiply %s" % ("bf16x6" if x6 else "native")
        if adv:
            check_a(Mt, ref, absdot, Cin, what="adversarial " + what)
            m = f64(Mt)
            assert (m[1] == 0).all() and (m[:, 2] == 0).all()
        else:
            check_a(Mt, ref, absdot, Cin, what=what)
            check_b(Mt, ref, gemm_tol(Cin), what=what)
        out[x6] = Mt
    if not adv:
        check_c(out[1], out[0], ref, "F(6,3) multiply N=%d Cin=%d Cout=%d" % (N, Cin, Cout))


# ---- the full Winograd operators: (b) and (c) ------------------------------------------------------------------------------------------------
W43_TOL = 5e-5
# F(6,3)/F(4,3) tiling, measured on an MI355X with the operands below (native fp32 kernels, max error / max|ref|): forward 1.5e-5, data gradient
# 1.6e-5 / 2.6e-5, weight gradient 5.5e-6 / 4.5e-6 (bf16x6: 1.4e-5, 2.1e-5, 5.4e-6).  Bound: about 2x the worst native figure.
W63_TOL = 5e-5


def _conv_refs64(x, w, b, dy):
    """float64 results of conv2d / its gradients (the oracle's, without its final fp32 rounding)"""
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    N, H, W, Ci = x.shape
    Co = w.shape[3]
    xp = np.pad(x64, ((0, 0), (1, 1), (1, 1), (0, 0)))
    P = np.stack([xp[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)], axis=3).reshape(N * H * W, 9 * Ci)
    y = (P @ w64.reshape(9 * Ci, Co) + b).reshape(N, H, W, Co)
    dw = (P.T @ dy64.reshape(-1, Co)).reshape(3, 3, Ci, Co)
    dyp = np.pad(dy64, ((0, 0), (1, 1), (1, 1), (0, 0)))
    Pd = np.stack([dyp[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)], axis=3).reshape(N * H * W, 9 * Co)
    wf = w64[::-1, ::-1].transpose(0, 1, 3, 2).reshape(9 * Co, Ci)
    dx = (Pd @ wf).reshape(N, H, W, Ci)
    return y, dx, dw


@pytest.mark.parametrize("N,H,W,C", [(6, 14, 14, 256), (4, 13, 11, 256)])
def test_wino43_operators(N, H, W, C):
    """myolo_conv3x3_wino_{fwd,bwd_data,bwd_weight}: forward and data gradient on wino_mm_x6_kernel, weight gradient on wino_tn_x6_kernel (all 36
    planes in one launch over the runs of the mixed tiling) -- (b) at 5e-5 against float64, (c) against wino_x6 = 0"""
    rng = np.random.default_rng(N * H * W)
    x, w, b, dy = rnd(rng, N, H, W, C), rnd(rng, 3, 3, C, C, scale=0.03), rnd(rng, C, scale=0.1), rnd(rng, N, H, W, C)
    refs = _conv_refs64(x, w, b, dy)
    xt, wt, bt, dyt = dt(x), dt(w), dt(b), dt(dy)
    wsa = wsbuf(max(X.wino_ws_bytes(N, H, W, C, C, k) for k in (0, 1, 2)))
    out = {}
    for x6 in (0, 1):
        with options(wino_x6=x6):
            y, dx, dw = new(N, H, W, C), new(N, H, W, C), new(3, 3, C, C)
            X.call("myolo_conv3x3_wino_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), None, None, X.ptr(y), N, H, W, C, C, 0, None, *wsa, X.stream())
            X.call("myolo_conv3x3_wino_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(dx), N, H, W, C, C, *wsa, X.stream())
            X.call("myolo_conv3x3_wino_bwd_weight", X.ptr(xt), None, X.ptr(dyt), X.ptr(dw), N, H, W, C, C, *wsa, X.stream())
            torch.cuda.synchronize()
        out[x6] = (y, dx, dw)
        for got, ref, name in zip(out[x6], refs, ("y", "dx", "dw")):
            check_b(got, ref, W43_TOL, "F(4,3) %s x6=%d" % (name, x6))
    for i, name in enumerate(("y", "dx", "dw")):
        check_c(out[1][i], out[0][i], refs[i], "F(4,3) %s N=%d %dx%d C=%d" % (name, N, H, W, C))


@pytest.mark.parametrize("N,Cin,Cout", [(6, 256, 256), (3, 256, 512)])
def test_wino63_operators(N, Cin, Cout):
    """myolo_conv3x3_wino63_{fwd,bwd_data,bwd_weight} on 14 x 14 maps: (b) at W63_TOL against float64, (c) against wino_x6 = 0"""
    rng = np.random.default_rng(N * Cout)
    H = W = 14
    x, w, b, dy = rnd(rng, N, H, W, Cin), rnd(rng, 3, 3, Cin, Cout, scale=0.03), rnd(rng, Cout, scale=0.1), rnd(rng, N, H, W, Cout)
    refs = _conv_refs64(x, w, b, dy)
    xt, wt, bt, dyt = dt(x), dt(w), dt(b), dt(dy)
    wsa = wsbuf(max(X.wino63_ws_bytes(N, Cin, Cout, k) for k in (0, 1, 2)))
    has_dx = X.wino63_ok(14, 14, Cout, Cin)
    out = {}
    for x6 in (0, 1):
        with options(wino_x6=x6):
            y, dx, dw, vk = new(N, H, W, Cout), new(N, H, W, Cin), new(3, 3, Cin, Cout), new(X.wino63_plane_elems(N, Cin))
            X.call("myolo_conv3x3_wino63_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), None, None, X.ptr(y), N, Cin, Cout, 0, X.ptr(vk), *wsa, X.stream())
            if has_dx:
                X.call("myolo_conv3x3_wino63_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(dx), N, Cin, Cout, *wsa, X.stream())
            X.call("myolo_conv3x3_wino63_bwd_weight", X.ptr(xt), None, X.ptr(dyt), X.ptr(dw), N, Cin, Cout, *wsa, X.stream())
            torch.cuda.synchronize()
        out[x6] = (y, dx, dw)
        for got, ref, name in zip(out[x6], refs, ("y", "dx", "dw")):
            if name == "dx" and not has_dx:
                continue
            mx, rms = check_b(got, ref, W63_TOL, "F(6,3) %s x6=%d" % (name, x6))
            print("F(6,3) %s x6=%d N=%d Cin=%d Cout=%d: max %.3e rms %.3e" % (name, x6, N, Cin, Cout, mx, rms))
    for i, name in enumerate(("y", "dx", "dw")):
        if name == "dx" and not has_dx:
            continue
        check_c(out[1][i], out[0][i], refs[i], "F(6,3) %s N=%d Cin=%d Cout=%d" % (name, N, Cin, Cout))


# ---- Conv2DTranspose 2x2 / s2 -----------------------------------------------------------------------------------------------------------------
def _deconv_refs(x, w, b, dy):
    """float64: y = relu(deconv(x) + b) with |x| |w| + |b|, dx / dw with their |A| |B| (w [2,2,Co,Ci]; dy None: forward only)"""
    N, H, W, Ci = x.shape
    Co = w.shape[2]
    x2, w64 = x.reshape(-1, Ci).astype(np.float64), w.astype(np.float64)
    pre, pabs = np.zeros((N, 2 * H, 2 * W, Co)), np.zeros((N, 2 * H, 2 * W, Co))
    dx, dxa = np.zeros_like(x2), np.zeros_like(x2)
    dw, dwa = np.zeros(w.shape), np.zeros(w.shape)
    for ky in range(2):
        for kx in range(2):
            pre[:, ky::2, kx::2] = (x2 @ w64[ky, kx].T).reshape(N, H, W, Co) + b
            pabs[:, ky::2, kx::2] = (np.abs(x2) @ np.abs(w64[ky, kx]).T).reshape(N, H, W, Co) + np.abs(b)
            if dy is None:
                continue
            d = dy[:, ky::2, kx::2, :].reshape(-1, Co).astype(np.float64)
            dx += d @ w64[ky, kx]
            dxa += np.abs(d) @ np.abs(w64[ky, kx])
            dw[ky, kx] = d.T @ x2
            dwa[ky, kx] = np.abs(d).T @ np.abs(x2)
    return (np.maximum(pre, 0), pabs), (dx.reshape(x.shape), dxa.reshape(x.shape)), (dw, dwa), pre


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(16, 16, 16, 256, 256), (1, 17, 241, 256, 256), (3, 37, 37, 256, 512)])
def test_deconv_x6(N, H, W, Cin, Cout):
    """myolo_deconv2x2s2_{fwd (bias + ReLU, scatter epilogue), bwd_data (four taps gathered into A), bwd_weight (wino_tn_x6_kernel<true>)}
    from 4096 input pixels: 4096, 4097 (odd H / W), 4107; (a) / (b) / (c) against deconv_no_x6 = 1"""
    rng = np.random.default_rng(N * H * W)
    x, w, b = rnd(rng, N, H, W, Cin), rnd(rng, 2, 2, Cout, Cin, scale=0.05), rnd(rng, Cout)
    dy = rnd(rng, N, 2 * H, 2 * W, Cout)
    (ry, ya), (rdx, dxa), (rdw, dwa), _ = _deconv_refs(x, w, b, dy)
    xt, wt, bt, dyt = dt(x), dt(w), dt(b), dt(dy)
    M = N * H * W
    out = {}
    for no in (1, 0):
        y, dx, dw = new(N, 2 * H, 2 * W, Cout), new(N, H, W, Cin), new(2, 2, Cout, Cin)
        with options(wino_x6=1, deconv_no_x6=no):
            X.call("myolo_deconv2x2s2_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), X.ptr(y), N, H, W, Cin, Cout, 1, *wsbuf(), X.stream())
            X.call("myolo_deconv2x2s2_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(dx), N, H, W, Cin, Cout, *wsbuf(), X.stream())
            X.call("myolo_deconv2x2s2_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(dw), N, H, W, Cin, Cout, *wsbuf(), X.stream())
            torch.cuda.synchronize()
        tag = "native" if no else "bf16x6"
        check_a(y, ry, ya, Cin + 1, what="deconv y " + tag)            # (the bias: one more term of the sum)
        check_a(dx, rdx, dxa, 4 * Cout, what="deconv dx " + tag)
        check_a(dw, rdw, dwa, M, what="deconv dw " + tag)
        check_b(y, ry, gemm_tol(Cin), "deconv y " + tag)
        check_b(dx, rdx, gemm_tol(4 * Cout), "deconv dx " + tag)
        check_b(dw, rdw, gemm_tol(M), "deconv dw " + tag)
        out[no] = (y, dx, dw)
    # the same-order twins: the three products as plain matrices (A of the data / weight gradient = dy's four taps gathered, k = (tap, co))
    taps = np.concatenate([dy[:, ky::2, kx::2, :].reshape(M, Cout) for ky in range(2) for kx in range(2)], axis=1)
    acc = seq_matmul(x.reshape(M, Cin), w.reshape(4 * Cout, Cin).T).reshape(N, H, W, 2, 2, Cout).transpose(0, 1, 3, 2, 4, 5)
    seq = (np.maximum((acc.reshape(N, 2 * H, 2 * W, Cout).astype(np.float32) + b).astype(np.float64), 0),
           seq_matmul(taps, w.reshape(4 * Cout, Cin)).reshape(N, H, W, Cin), seq_matmul(taps.T, x.reshape(M, Cin)).reshape(2, 2, Cout, Cin))
    for i, (name, ref) in enumerate(zip(("y", "dx", "dw"), (ry, rdx, rdw))):
        check_c(out[0][i], out[1][i], ref, "deconv %s N=%d %dx%d Cin=%d Cout=%d" % (name, N, H, W, Cin, Cout), seq=seq[i])


# ---- fused deconv + ReLU + 1x1 + sigmoid (MM_EP_DECONV_MASK_T / MM_EP_DECONV_MASK) -----------------------------------------------------------
def _mask_refs(x, w, b, w2, b2):
    (d, dabs), _, _, pre = _deconv_refs(x, w, b, None)
    Cin, Cout = x.shape[3], w.shape[2]
    w2a = np.abs(w2.astype(np.float64))
    logit = d @ w2.astype(np.float64) + b2
    # |d logit| <= sum_c |w2_c| |d d_c| + fp32 rounding of the 1x1 conv (with b2 as one more term); |d p| <= |d logit| / 4; + the sigmoid's own
    dlog = (4 * (Cin + 1) * U24 * dabs) @ w2a + 4 * (Cout + 1) * U24 * (np.abs(d) @ w2a + np.abs(b2))
    return 1 / (1 + np.exp(-logit)), logit, dlog / 4 + 16 * U24, d, dabs


@pytest.mark.parametrize("N,H,W,Cin,Cout,C,legacy", [(3, 14, 14, 256, 256, 4, 0), (1, 3, 5, 256, 256, 1, 0), (2, 5, 7, 64, 512, 3, 0),
                                                      (3, 14, 14, 256, 256, 2, 1), (1, 2, 3, 48, 256, 3, 1)])
def test_deconv_mask_fused_x6(N, H, W, Cin, Cout, C, legacy):
    """myolo_deconv2x2s2_mask_fwd: MM_EP_DECONV_MASK_T (the default bf16x6 tile; 256 channels: the sigmoid stored by the kernel, 512: partial
    logits + finish) and MM_EP_DECONV_MASK (deconv_mask_legacy = 1), 1-4 classes, row tiles with a handful of valid rows; native twin: wino_x6 = 0.
    (b) at the sigmoid's image of the GEMM bound: max|dp| <= tol(Cin) + tol(Cout) times max|logit| / 4"""
    rng = np.random.default_rng(N * H * W * C)
    x, w, b = rnd(rng, N, H, W, Cin), rnd(rng, 2, 2, Cout, Cin, scale=0.05), rnd(rng, Cout)
    w2, b2 = rnd(rng, Cout, C, scale=0.1), rnd(rng, C)
    ref, logit, pbound, _, _ = _mask_refs(x, w, b, w2, b2)
    args = [X.ptr(dt(a)) for a in (x, w, b, w2, b2)]
    wsa = wsbuf(X.deconv_mask_ws_bytes(N, H, W, Cin, Cout, C))
    out = {}
    for x6 in (0, 1):
        p = new(N, 2 * H, 2 * W, C)
        with options(wino_x6=x6, deconv_mask_legacy=legacy):
            X.call("myolo_deconv2x2s2_mask_fwd", *args, X.ptr(p), N, H, W, Cin, Cout, C, *wsa, X.stream())
        tag = "deconv+mask %s legacy=%d" % ("bf16x6" if x6 else "native", legacy)
        check_a(p, ref, np.zeros_like(ref), 0, extra=pbound, what=tag)
        mx = float(np.abs(f64(p) - ref).max())
        tol = (gemm_tol(Cin) + gemm_tol(Cout)) * float(np.abs(logit).max()) / 4
        assert mx <= tol, "%s: max |dp| %.3e > %.3e" % (tag, mx, tol)
        out[x6] = p
    check_c(out[1], out[0], ref, "deconv+mask N=%d %dx%d Cin=%d Cout=%d C=%d legacy=%d" % (N, H, W, Cin, Cout, C, legacy))


@pytest.mark.parametrize("N,H,W", [(9, 14, 14), (66, 14, 14)])
def test_deconv_mask_fused_keep_x6(N, H, W):
    """myolo_deconv2x2s2_mask_fwd_keep: the kept deconv rows of the positives (ReLU(deconv + bias)) to (a) and (b), the probabilities to (a)"""
    Cin = Cout = 256
    C = 4
    rng = np.random.default_rng(N)
    x, w, b = rnd(rng, N, H, W, Cin), rnd(rng, 2, 2, Cout, Cin, scale=0.05), rnd(rng, Cout)
    w2, b2 = rnd(rng, Cout, C, scale=0.1), rnd(rng, C)
    ref, _, pbound, d, dabs = _mask_refs(x, w, b, w2, b2)
    chosen = np.sort(rng.choice(N, size=max(2, N // 3), replace=False)).astype(np.int32)
    inv = np.full(N, -1, np.int32)
    inv[chosen] = np.arange(len(chosen), dtype=np.int32)
    cap = len(chosen) - 1
    inv_t = torch.as_tensor(inv, device=DEV)
    _KEEP.append(inv_t)
    args = [X.ptr(dt(a)) for a in (x, w, b, w2, b2)]
    wsa = wsbuf(X.deconv_mask_ws_bytes(N, H, W, Cin, Cout, C))
    out = {}
    for x6 in (0, 1):
        p, dk = new(N, 2 * H, 2 * W, C), new(len(chosen), 2 * H, 2 * W, Cout)
        with options(wino_x6=x6):
            X.call("myolo_deconv2x2s2_mask_fwd_keep", *args, X.ptr(p), N, H, W, Cin, Cout, C, X.ptr(inv_t), X.ptr(dk), cap, *wsa, X.stream())
        tag = "deconv+mask keep %s" % ("bf16x6" if x6 else "native")
        check_a(p, ref, np.zeros_like(ref), 0, extra=pbound, what=tag + " p")
        kept = dk[:cap]
        check_a(kept, d[chosen[:cap]], dabs[chosen[:cap]], Cin + 1, what=tag + " kept rows")
        check_b(kept, d[chosen[:cap]], gemm_tol(Cin), tag + " kept rows")
        assert bool(torch.isnan(dk[cap:]).all()), "a slot at / beyond the cap was written"
        out[x6] = kept
    check_c(out[1], out[0], d[chosen[:cap]], "deconv+mask keep rows N=%d" % N)


# ---- the native fp32 pointwise family: (a) and (b) --------------------------------------------------------------------------------------------
# (entry, M, Cin, Cout, options): which kernel each reaches is named beside it (csrc/gemm_kernels.hip)
NATIVE_PW = [
    ("fwd", 8197, 64, 64, {}),                                      # pw_fwd_thin_kernel (no bias, ragged last row block)
    ("fwd", 33, 288, 256, {}),                                      # pw_smallm_kernel
    ("fwd", 1571, 1024, 35, {}),                                    # pw_skinny_fwd_kernel<16>
    ("fwd", 677, 256, 27, {}),                                      # pw_skinny_fwd_kernel<4>
    ("fwd", 10, 16, 63, {}),                                        # pw_skinny_fwd_kernel<4>, one row block
    ("fwd", 1568, 1024, 24, {}),                                    # gemm_nn_fast (Cout % 4 == 0: not the skinny kernel)
    ("fwd", 1568, 1024, 256, {"pw_no_smallm": 1}),                  # gemm_nn_fast, split-K
    ("fwd", 1568, 1024, 256, {"pw_no_smallm": 1, "no_splitk": 1}),  # gemm_nn_fast, one pass
    ("fwd", 1003, 96, 80, {"gemm_generic": 1}),                     # the generic kernel
    ("affine", 33, 288, 256, {}),                                   # pw_smallm_kernel, affine + ReLU6 epilogue
    ("affine", 1003, 96, 80, {}),                                   # gemm_nn_fast, affine + ReLU6 epilogue
    ("bnstats", 9001, 32, 64, {}),                                  # pw_fwd_thin_kernel with the BatchNorm on load
    ("bnstats", 1568, 512, 256, {"pw_no_smallm": 1}),               # gemm_nn_fast with the BatchNorm on load
    ("dx", 8195, 32, 136, {}),                                      # pw_bwd_data_thin_kernel<1>
    ("dx", 8200, 64, 256, {}),                                      # pw_bwd_data_thin_kernel<2>
    ("dx", 1568, 1024, 512, {}),                                    # pw_smallm_kernel
    ("dw", 16387, 64, 128, {}),                                     # pw_wgrad_thin
    ("dw", 16390, 32, 64, {}),                                      # pw_wgrad_thin
    ("dw", 1003, 96, 80, {}),                                       # gemm_tn_fast
    ("dw_affine", 1003, 256, 256, {}),                              # gemm_tn_fast with the BatchNorm on load
]


@pytest.mark.parametrize("entry,M,Cin,Cout,opts", NATIVE_PW, ids=["%s-%d-%d-%d%s" % (e, m, ci, co, "".join("-" + k for k in o)) for e, m, ci, co, o in NATIVE_PW])
def test_native_pointwise(entry, M, Cin, Cout, opts):
    rng = np.random.default_rng(M + Cin * 3 + Cout)
    x, w, b = rnd(rng, M, Cin, scale=2.0), rnd(rng, Cin, Cout, scale=0.1), rnd(rng, Cout)
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    st = X.stream()
    extra = 0.0
    with options(wino_x6=0, **opts):
        if entry in ("fwd", "affine", "bnstats"):
            K = Cin
            if entry == "bnstats":
                isc, ish = 1 + rnd(rng, Cin, scale=0.3), 3 + rnd(rng, Cin, scale=1.0)
                x64 = formed_on_load(x, isc, ish, 2).astype(np.float64)
                got, mean, var = _pw_bnstats(dt(x), dt(isc), dt(ish), 2, dt(w), M, Cin, Cout)
                _check_stats(got, mean, var, "native bnstats")
            acc, absdot = x64 @ w64, np.abs(x64) @ np.abs(w64)
            if entry == "bnstats":
                ref, extra = acc, U24 * absdot
            elif entry == "fwd":
                bias = b if Cout % 4 else None             # (the thin kernel takes no bias; the skinny kernels are the bias users)
                ref = acc + (bias if bias is not None else 0)
                absdot = absdot + (np.abs(bias) if bias is not None else 0)
                K = Cin + 1
                got = new(M, Cout)
                X.call("myolo_pwconv1x1_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(bias)) if bias is not None else None, X.ptr(got), M, Cin, Cout,
                       *wsbuf(), st)
            else:
                sc, sh = 1 + rnd(rng, Cout, scale=0.2), rnd(rng, Cout, scale=0.5)
                ref = np.clip(acc * sc + sh, 0, 6)
                # y = act(fmaf(acc, sc, sh)): |sc| x the product's bound + one rounding of the affine
                extra = U24 * (np.abs(acc * sc) + np.abs(sh)) * 2
                absdot = absdot * np.abs(sc)
                got = new(M, Cout)
                X.call("myolo_pwconv1x1_affine_act_fwd", X.ptr(dt(x)), X.ptr(dt(w)), X.ptr(dt(sc)), X.ptr(dt(sh)), 2, X.ptr(got), M, Cin, Cout, *wsbuf(), st)
        elif entry == "dx":
            K = Cout
            dy = rnd(rng, M, Cout).astype(np.float64)
            ref, absdot = dy @ w64.T, np.abs(dy) @ np.abs(w64).T
            got = new(M, Cin)
            X.call("myolo_pwconv1x1_bwd_data", X.ptr(dt(dy)), X.ptr(dt(w)), X.ptr(got), M, Cin, Cout, *wsbuf(), st)
        else:
            K = M
            dy = rnd(rng, M, Cout)
            got = new(Cin, Cout)
            if entry == "dw_affine":
                isc, ish = 1 + rnd(rng, Cin, scale=0.3), 3 + rnd(rng, Cin, scale=1.0)
                x64 = formed_on_load(x, isc, ish, 2).astype(np.float64)
                extra = None
                X.call("myolo_pwconv1x1_bwd_weight_affine_in", X.ptr(dt(x)), X.ptr(dt(isc)), X.ptr(dt(ish)), 2, X.ptr(dt(dy)), X.ptr(got), M, Cin, Cout,
                       *wsbuf(), st)
            else:
                X.call("myolo_pwconv1x1_bwd_weight", X.ptr(dt(x)), X.ptr(dt(dy)), X.ptr(got), M, Cin, Cout, *wsbuf(), st)
            d64 = dy.astype(np.float64)
            ref, absdot = x64.T @ d64, np.abs(x64).T @ np.abs(d64)
            if extra is None:
                extra = U24 * absdot
        torch.cuda.synchronize()
    what = "native %s M=%d Cin=%d Cout=%d %s" % (entry, M, Cin, Cout, opts)
    check_a(got, ref, absdot, K, extra=extra, what=what)
    mx, rms = check_b(got, ref, gemm_tol(K), what=what)
    print("%s: max %.3e rms %.3e" % (what, mx, rms))


def test_native_pointwise_adversarial():
    """the adversarial operand set through the native forward (gemm_nn_fast), data gradient and weight gradient (gemm_tn_fast)"""
    rng = np.random.default_rng(29)
    M, Cin, Cout = 1000, 96, 80
    st = X.stream()
    with options(wino_x6=0):
        P, Q = adversarial(rng, M, Cin, Cout)
        y = new(M, Cout)
        X.call("myolo_pwconv1x1_fwd", X.ptr(dt(P)), X.ptr(dt(Q)), None, X.ptr(y), M, Cin, Cout, *wsbuf(), st)
        check_adversarial(y, P, Q, "adversarial native pw fwd")
        P, Q = adversarial(rng, M, Cout, Cin)
        dx = new(M, Cin)
        X.call("myolo_pwconv1x1_bwd_data", X.ptr(dt(P)), X.ptr(dt(Q.T)), X.ptr(dx), M, Cin, Cout, *wsbuf(), st)
        check_adversarial(dx, P, Q, "adversarial native pw dx")
        P, Q = adversarial(rng, Cin, M, Cout)
        dw = new(Cin, Cout)
        X.call("myolo_pwconv1x1_bwd_weight", X.ptr(dt(P.T)), X.ptr(dt(Q)), X.ptr(dw), M, Cin, Cout, *wsbuf(), st)
        check_adversarial(dw, P, Q, "adversarial native pw dw")

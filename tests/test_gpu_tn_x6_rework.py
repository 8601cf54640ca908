"""The bf16x6 weight-gradient product C[plane] = A[plane]^T B[plane] (csrc/wino_mm.hip, wino_tn_x6_kernel) with the loader's operand index as a
wave-uniform value (scalar load offsets, uniform branches) against the kernel as it was (library option "tn_x6_legacy": every operand load in a
waterfall loop): the same split plan, chunk order, piece-product order and fixed-order reduce, so every case asks for np.array_equal between the
two, and holds the result to the bounds tests/test_gpu_fp32_products.py uses for this kernel against a float64 product of the same fp32 operands:

  (a) |got - ref| <= 4 K 2^-24 (|A|^T |B|) per element, K = rows (+ 2^-24 |A|^T |B| where A is formed on load);   (b) max|err| / max|ref| <= 2e-6 sqrt(K / 256).

The shapes are the smallest that reach each path: fewer rows than a chunk, a ragged last chunk, several splits of unequal length, several runs of
planes in one call (one of them empty), more than one tile per (plane, split), a dozen units in one launch and in launches of three (tn_wgs),
the on-load affine and the gathered A operand of the deconv weight gradient."""
import contextlib
import ctypes

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


def wsbuf(nbytes=64 << 20):
    if getattr(wsbuf, "buf", None) is None:
        wsbuf.buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    return wsbuf.buf.data_ptr(), wsbuf.buf.numel()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


@contextlib.contextmanager
def options(**kv):
    with contextlib.ExitStack() as st:
        for k, v in kv.items():
            st.enter_context(X.option(k, v))
        yield


def both(fn, shape, **opts):
    """fn(out) under tn_x6_legacy = 1 and 0: the two outputs (numpy), asserted bit-identical"""
    out = {}
    for legacy in (1, 0):
        c = new(*shape)
        with options(wino_x6=1, tn_x6_legacy=legacy, **opts):
            fn(c)
        out[legacy] = host(c)
    assert np.isfinite(out[0]).all(), "non-finite output"
    assert np.array_equal(out[0], out[1]), "differs from the legacy kernel in %d of %d elements" % (int((out[0] != out[1]).sum()), out[0].size)
    return out[0]


def check(got, ref, absdot, K, extra=0.0, what=""):
    err = np.abs(got.astype(np.float64) - ref)
    bound = 4.0 * K * U24 * absdot + extra
    worst = float((err / np.maximum(bound, 1e-300)).max())
    mx = float(err.max()) / float(np.abs(ref).max())
    tol = 2e-6 * (max(K, 1) / 256.0) ** 0.5
    print("%s: worst err / componentwise bound %.3g, normwise %.3e (tol %.3e)" % (what, worst, mx, tol))
    assert not (err > bound).any(), "%s: %d elements beyond the componentwise fp32 bound (worst %.3g)" % (what, int((err > bound).sum()), worst)
    assert mx <= tol, "%s: normwise error %.3e > %.3e" % (what, mx, tol)


def act_np(v, act):
    return np.clip(v, 0, 6) if act == 2 else (np.maximum(v, 0) if act == 1 else v)


# ---- one plane through the pointwise weight gradient: dw [Ka][N] = x^T dy ------------------------------------------------------------------
@pytest.mark.parametrize("rows,Ka,N,wgs", [(5, 256, 256, None), (16, 256, 256, None), (133, 256, 256, None), (300, 256, 256, None),
                                           (300, 512, 256, None), (300, 256, 512, None), (300, 512, 512, 0), (1500, 256, 256, 0), (1500, 256, 256, 3)])
def test_one_plane(rows, Ka, N, wgs):
    """rows below one chunk, one chunk, a ragged last chunk, three splits of unequal length (112 / 112 / 76); two tiles per (plane, split) along
    Ka and along N; 12 units in one launch (tn_wgs = 0: 12 splits of one tile, or three splits of four tiles); tn_wgs = 3, which also sets the
    split plan's target: nine splits of 176 rows in launches of three units.  Both kernels get the same plan."""
    rng = np.random.default_rng(rows + Ka + 3 * N)
    x, dy = rnd(rng, rows, Ka, scale=2.0), rnd(rng, rows, N)
    xt, dyt = dt(x), dt(dy)
    opts = dict(pw_x6_min_rows=1)
    if wgs is not None:
        opts["tn_wgs"] = wgs
    got = both(lambda c: X.call("myolo_pwconv1x1_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(c), rows, Ka, N, *wsbuf(), X.stream()), (Ka, N), **opts)
    x64, d64 = x.astype(np.float64), dy.astype(np.float64)
    check(got, x64.T @ d64, np.abs(x64).T @ np.abs(d64), rows, what="rows=%d Ka=%d N=%d tn_wgs=%s" % (rows, Ka, N, wgs))
    with options(wino_x6=1, pw_x6_min_rows=1, pw_no_x6=1):          # the case did reach the bf16x6 kernel
        nat = new(Ka, N)
        X.call("myolo_pwconv1x1_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(nat), rows, Ka, N, *wsbuf(), X.stream())
    assert rows < 16 or not np.array_equal(host(nat), got)


def test_affine_on_load():
    """A = relu6(fmaf(x, scale, shift)) formed on load, scales of both signs, 133 rows: two splits of 80 and 53 rows, so the padding rows of the
    last chunk of both (which would become relu6(shift) != 0) must stay 0"""
    rng = np.random.default_rng(133)
    rows, Ka, N = 133, 256, 256
    x, dy = rnd(rng, rows, Ka, scale=3.0), rnd(rng, rows, N)
    sc, sh = rnd(rng, Ka, scale=1.0), 3 + rnd(rng, Ka, scale=1.0)
    assert (sc < 0).any() and (sc > 0).any() and (sh > 0).all()
    a = act_np((x.astype(np.float64) * sc + sh).astype(np.float32), 2).astype(np.float64)
    assert (a == 0).any() and (a == 6).any()
    xt, dyt, sct, sht = dt(x), dt(dy), dt(sc), dt(sh)
    got = both(lambda c: X.call("myolo_pwconv1x1_bwd_weight_affine_in", X.ptr(xt), X.ptr(sct), X.ptr(sht), 2, X.ptr(dyt), X.ptr(c), rows, Ka, N,
                                *wsbuf(), X.stream()), (Ka, N), pw_x6_min_rows=1)
    d64 = dy.astype(np.float64)
    absdot = np.abs(a).T @ np.abs(d64)
    check(got, a.T @ d64, absdot, rows, extra=U24 * absdot, what="affine on load")


# ---- several runs of planes in one call ----------------------------------------------------------------------------------------------------
def _planes(A, B, C, rows, nq, Ka, N):
    r = (ctypes.c_int64 * 4)(*rows)
    q = (ctypes.c_int32 * 4)(*nq)
    X.call("myolo_gemm_tn_bf16x6_planes", X.ptr(A), X.ptr(B), X.ptr(C), 4, ctypes.cast(r, ctypes.c_void_p), ctypes.cast(q, ctypes.c_void_p), Ka, N,
           *wsbuf(), X.stream())


@pytest.mark.parametrize("rows", [(48, 96, 96, 208), (48, 0, 96, 208)])
def test_four_runs(rows):
    """2 / 1 / 1 / 3 planes of 48 / 96 / 96 / 208 rows (the last run in two splits of 112 and 96 rows); then with the second run empty (it is
    skipped: its plane is not in C)"""
    nq = (2, 1, 1, 3)
    Ka = N = 256
    rng = np.random.default_rng(sum(rows))
    total = sum(r * q for r, q in zip(rows, nq))
    A, B = rnd(rng, total, Ka, scale=2.0), rnd(rng, total, N)
    At, Bt = dt(A), dt(B)
    planes = sum(q for r, q in zip(rows, nq) if r > 0)
    got = both(lambda c: _planes(At, Bt, c, rows, nq, Ka, N), (planes, Ka, N))
    at, z = 0, 0
    for r, q in zip(rows, nq):
        for _ in range(q if r > 0 else 0):
            a64, b64 = A[at:at + r].astype(np.float64), B[at:at + r].astype(np.float64)
            check(got[z], a64.T @ b64, np.abs(a64).T @ np.abs(b64), r, what="rows %s plane %d" % (rows, z))
            at += r
            z += 1
    assert z == planes and at == total


# ---- the gathered A operand: deconv 2x2 / s2 weight gradient -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_img", [2, 20])
def test_deconv_gather(n_img):
    """Co = 64 (Ka = 4 Co = 256), Cin = 256 on a 3 x 5 grid: 2 images (30 rows: chunks straddle the image boundary), 20 images (300 rows in
    three splits of 112: rows straddle image and split boundaries)"""
    H, W, Cin, Co = 3, 5, 256, 64
    rng = np.random.default_rng(n_img)
    x, dy = rnd(rng, n_img, H, W, Cin), rnd(rng, n_img, 2 * H, 2 * W, Co)
    xt, dyt = dt(x), dt(dy)
    M = n_img * H * W
    got = both(lambda c: X.call("myolo_deconv2x2s2_bwd_weight_bf16x6", X.ptr(xt), X.ptr(dyt), X.ptr(c), n_img, H, W, Cin, Co, *wsbuf(), X.stream()),
               (2, 2, Co, Cin))
    x2 = x.reshape(M, Cin).astype(np.float64)
    for ky in range(2):
        for kx in range(2):
            d = dy[:, ky::2, kx::2, :].reshape(M, Co).astype(np.float64)
            check(got[ky, kx], d.T @ x2, np.abs(d).T @ np.abs(x2), M, what="deconv dw images=%d tap (%d, %d)" % (n_img, ky, kx))


def test_repeatable():
    """two consecutive calls on the same inputs give the same bits"""
    rng = np.random.default_rng(7)
    rows, Ka, N = 300, 256, 512
    xt, dyt = dt(rnd(rng, rows, Ka)), dt(rnd(rng, rows, N))
    out = []
    with options(wino_x6=1, pw_x6_min_rows=1):
        for _ in range(2):
            c = new(Ka, N)
            X.call("myolo_pwconv1x1_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(c), rows, Ka, N, *wsbuf(), X.stream())
            out.append(host(c))
    assert np.array_equal(out[0], out[1])

"""Every scratch-taking entry held to its planner, at any scratch size.

The entries that take a `(ws, ws_bytes)` pair are called here on a workspace CARVED out of a larger allocation (`scratch`): the call is told
`ws_bytes = nbytes`, the bytes behind it are a guard that must come back byte-identical, and the scratch itself is pre-filled with 0x00 or with
0xFF (every fp32 / fp64 word of which is a NaN).  The guard is at least as large as the largest planner figure of the shape, so an entry that
forgets to look at `ws_bytes` writes into memory the test owns and is reported; it cannot write outside the allocation.

  Part 1  every planner the binding exports: its entry at exactly the planner's bytes -- succeeds, guard intact, same bits on 0xFF scratch as on
          0x00 scratch, correct result (exact sums on integer operands; the Winograd entries through the op tests' own check functions and bounds,
          imported from test_gpu_ops); 256 bytes below a
          documented hard minimum the entry raises the workspace error, writes no output and leaves the guard alone.
  Part 2  the entries that READ ws_bytes to choose a kernel or a split count, swept over sizes.  All operands are integers, so every size gives the
          same, exact result.  The path a call took is read off the poisoned scratch (`words`: the 4-byte words it overwrote) -- no threshold of
          csrc/ is restated here (the one restated line of the split rule is marked at `ragged`); thresholds are FOUND by bisection over the size (`find_paths`), which by construction makes one call
          just below each threshold and one at it.
  Part 3  one training step (both FP32_MATMUL modes) and one inference forward (fp32, bf16) of the engine with every scratch buffer it owns
          filled with 0xFF, against the same run on zero-filled buffers.

Each sweep prints one line naming the paths it reached (split counts seen, or words written per path and the size each path starts at)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_ops as O                      # noqa: E402
from myolo import _ext as X                         # noqa: E402
from test_gpu_ops import (check, TOL, check_stats_agree, check_mean_var_float64, check_f63_equals_f43,      # noqa: E402  (the op tests' check functions
                          _check_bn_outputs)                                                            # and bounds, unchanged)
from test_gpu_step import TOL as STEP_TOL           # noqa: E402
from test_gpu_exact_sums import ints, assert_exact, check_stats, pre_activation_operands, two_tap_filters      # noqa: E402

DEV = "cuda:0"
GUARD_BYTE = 0xA5
_KEEP = []   # device tensors must outlive the asynchronous kernel that reads them


@pytest.fixture(autouse=True)
def _keepalive():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


# ============================================================================================================================================
# the harness
# ============================================================================================================================================
def scratch(nbytes, guard, fill):
    """A workspace of `nbytes` carved out of an allocation of nbytes + guard: the first nbytes filled with `fill` (0x00 or 0xFF), the guard behind it
    with GUARD_BYTE.  -> (pointer, nbytes, report); report() -> (guard intact, number of 4-byte scratch words that no longer hold the fill)."""
    nbytes, guard = int(nbytes), int(guard)
    assert fill in (0x00, 0xFF) and nbytes >= 0 and guard >= 256
    buf = torch.empty(nbytes + guard, dtype=torch.uint8, device=DEV)
    buf[:nbytes].fill_(fill)
    buf[nbytes:].fill_(GUARD_BYTE)
    torch.cuda.synchronize()
    _KEEP.append(buf)

    def report():
        torch.cuda.synchronize()
        intact = bool((buf[nbytes:] == GUARD_BYTE).all())
        words = buf[:nbytes // 4 * 4].view(torch.int32)
        return intact, int((words != (-1 if fill == 0xFF else 0)).sum())
    return buf.data_ptr(), nbytes, report


def test_the_harness_reports_what_a_kernel_wrote():
    """myolo_fill on a carved workspace: the words it wrote are counted on either fill (a written zero is not told from a 0x00 fill: that run counts the
    scratch the kernel did NOT zero), one float past ws_bytes is reported as a damaged guard"""
    for fill, value, want in ((0xFF, 0.0, 100), (0xFF, 1.0, 100), (0x00, 1.0, 100), (0x00, 0.0, 0)):
        p, n, report = scratch(1024, 256, fill)
        X.call("myolo_fill", p, value, 100, X.stream())
        assert report() == (True, want), (fill, value)
    p, n, report = scratch(1024, 256, 0xFF)
    X.call("myolo_fill", p, 1.0, 257, X.stream())
    assert report() == (False, 256)
    p, n, report = scratch(0, 256, 0xFF)
    assert report() == (True, 0)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def exact(got, ref64, bound, unit, what):
    """assert_exact of test_gpu_exact_sums with a scalar bound on sum|terms|"""
    assert_exact(got, ref64, np.array([float(bound)]), unit, what)


class Case(object):
    """One entry on one set of operands.  outs() -> fresh NaN-filled outputs; call(ptr, nbytes, outs) runs the entry; verify(outs) asserts the result;
    guard: bytes of guard behind the scratch (>= every planner figure of the shape); options: library switches held while the entry runs."""

    def __init__(self, name, outs, call, verify, guard, options=None):
        self.name, self.outs, self._call, self.verify, self.guard, self.options = name, outs, call, verify, int(max(guard, 256)), dict(options or {})

    def call(self, ptr, nbytes, outs):
        old = {k: X.set_option(k, v) for k, v in self.options.items()}
        try:
            self._call(ptr, nbytes, outs)
            torch.cuda.synchronize()
        finally:
            for k, v in old.items():
                X.set_option(k, v)


def run_at(case, nbytes, fill):
    """the entry on `nbytes` of `fill` scratch -> (outputs, words overwritten); the guard must be intact"""
    p, n, report = scratch(nbytes, case.guard, fill)
    outs = case.outs()
    case.call(p, n, outs)
    intact, words = report()
    assert intact, "%s: wrote past ws_bytes = %d (guard of %d bytes damaged)" % (case.name, n, case.guard)
    return outs, words


def both_fills(case, nbytes):
    """(a) succeeds, (b) guard intact, (c) 0xFF scratch gives the bits of 0x00 scratch, (d) correct.  -> (outputs, words overwritten)"""
    o0, _ = run_at(case, nbytes, 0x00)
    o1, words = run_at(case, nbytes, 0xFF)
    for i, (a, b) in enumerate(zip(o0, o1)):
        assert torch.equal(a, b), "%s: output %d on 0xFF scratch differs from 0x00 scratch at ws_bytes = %d (scratch read before written)" % (case.name, i, nbytes)
    case.verify(o1)
    return o1, words


def touched(outs, before):
    """the outputs that no longer hold the bits they had before the call: the NaN pre-fill (a sentinel for the integer outputs), or for the moving averages
    (in / out) their starting values"""
    return [i for i, (t, b) in enumerate(zip(outs, before)) if not torch.equal(t.view(torch.uint8), b.view(torch.uint8))]


def expect_ws_error(case, nbytes):
    """the workspace error; no output written (the NaN pre-fill is still there); guard intact"""
    p, n, report = scratch(nbytes, case.guard, 0xFF)
    outs = case.outs()
    before = [t.clone() for t in outs]
    with pytest.raises(RuntimeError, match=r"\(-2\).*workspace too small"):
        case.call(p, n, outs)
    intact, _ = report()
    assert intact, "%s: the refused call (ws_bytes = %d) damaged the guard" % (case.name, n)
    assert not touched(outs, before), "%s: the refused call wrote outputs %s" % (case.name, touched(outs, before))


def probe(case, nbytes):
    """one call on 0xFF scratch: "error" (checked as expect_ws_error does), or the number of scratch words it overwrote (result verified)"""
    p, n, report = scratch(nbytes, case.guard, 0xFF)
    outs = case.outs()
    before = [t.clone() for t in outs]
    try:
        case.call(p, n, outs)
    except RuntimeError as e:
        assert "(-2)" in str(e) and "workspace too small" in str(e), e
        intact, _ = report()
        assert intact, "%s: the refused call (ws_bytes = %d) damaged the guard" % (case.name, n)
        assert not touched(outs, before), "%s: the refused call wrote outputs %s" % (case.name, touched(outs, before))
        return "error", None
    intact, words = report()
    assert intact, "%s: wrote past ws_bytes = %d (guard of %d bytes damaged)" % (case.name, n, case.guard)
    case.verify(outs)
    return words, outs


def find_paths(case, lo, hi):
    """The paths the entry takes for ws_bytes in [lo, hi] (multiples of 256), found by bisection on what the call leaves in the scratch: wherever two
    sizes leave different amounts, the interval between them is halved down to 256 bytes -- one call just below each threshold, one at it.  Every call
    is checked (probe).  -> [(first size of the path, "error" | words overwritten)], ascending; and {size: outputs} of the calls that succeeded."""
    lo, hi = lo // 256 * 256, -(-hi // 256) * 256
    seen = {}

    def sig(n):
        if n not in seen:
            seen[n] = probe(case, n)
        return seen[n][0]

    def rec(a, b):
        if b - a <= 256:
            return
        m = (a + b) // 512 * 256
        if sig(m) != sig(a):
            rec(a, m)
        if sig(m) != sig(b):
            rec(m, b)
    if sig(lo) != sig(hi):
        rec(lo, hi)
    paths = []
    for n in sorted(seen):
        if not paths or paths[-1][1] != sig(n):
            paths.append((n, sig(n)))
    return paths, {n: o for n, (s, o) in seen.items() if s != "error"}


def show(name, paths):
    print("%s: %s" % (name, "; ".join("from %d bytes: %s" % (n, s if s == "error" else "%d words" % s) for n, s in paths)))


def same_bits(case, outs_by_size):
    """integer operands: every size gives the same bits"""
    sizes = sorted(outs_by_size)
    for n in sizes[1:]:
        for a, b in zip(outs_by_size[sizes[0]], outs_by_size[n]):
            assert torch.equal(a, b), "%s: ws_bytes = %d and %d give different bits" % (case.name, sizes[0], n)


SCALES = np.array([0.5, 1.0, 2.0], np.float32)


def affine(rng, C):
    """per-channel scale in {1/2, 1, 2} and shift in multiples of 1/4"""
    return SCALES[rng.integers(0, 3, C)], (np.float32(0.25) * rng.integers(-8, 9, C)).astype(np.float32)


# ============================================================================================================================================
# operand builders (integer operands: every partial sum exact in fp32; cribbed from test_gpu_ops / test_gpu_exact_sums)
# ============================================================================================================================================
@functools.lru_cache(maxsize=None)
def conv3_case(kind, N, H, W, Cin, Cout):
    """myolo_conv3x3_fwd ("bias" / "plain") / _affine_act_fwd ("affine") / _bwd_data / _bwd_weight on x, dy in -4..4, w in -2..2, bias in -8..8"""
    rng = np.random.default_rng(201)
    x, w, b = ints(rng, (N, H, W, Cin), -4, 4), ints(rng, (3, 3, Cin, Cout), -2, 2), ints(rng, (Cout,), -8, 8)
    dy = ints(rng, (N, H, W, Cout), -4, 4)
    xt, wt, bt, dyt = dev(x), dev(w), dev(b), dev(dy)
    pads = (1, 1, 1, 1)
    guard = 2 * X.workspace_bytes(N * H * W, Cin, Cout) + 80 * N * H * W * max(Cin, Cout) * 4
    if kind in ("bias", "plain"):
        ref = O.conv2d(x, w, pads=pads, bias=b if kind == "bias" else None, acc=np.float64)
        return Case("conv3x3_fwd(%s)" % kind, lambda: [nan(N, H, W, Cout)],
                    lambda p, n, o: X.call("myolo_conv3x3_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt) if kind == "bias" else None, X.ptr(o[0]), N, H, W, Cin, Cout, p, n, X.stream()),
                    lambda o: exact(o[0], ref, 9 * Cin * 8 + 8, 1.0, "conv3x3_fwd y"), guard)
    if kind == "affine":
        sc, sh = affine(rng, Cout)
        sct, sht = dev(sc), dev(sh)
        ref = np.maximum(O.conv2d(x, w, pads=pads, bias=b, acc=np.float64).astype(np.float64) * sc + sh, 0)
        return Case("conv3x3_affine_act_fwd(relu)", lambda: [nan(N, H, W, Cout)],
                    lambda p, n, o: X.call("myolo_conv3x3_affine_act_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), X.ptr(sct), X.ptr(sht), X.ptr(o[0]), N, H, W, Cin, Cout, 1, p, n, X.stream()),
                    lambda o: exact(o[0], ref, (9 * Cin * 8 + 8) * 2 + 2, 0.25, "conv3x3_affine_act_fwd y"), guard)
    rdx, rdw, _ = O.conv2d_bwd(x, w, dy, pads=pads, acc=np.float64)
    if kind == "bwd_data":
        return Case("conv3x3_bwd_data", lambda: [nan(N, H, W, Cin)],
                    lambda p, n, o: X.call("myolo_conv3x3_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(o[0]), N, H, W, Cin, Cout, p, n, X.stream()),
                    lambda o: exact(o[0], rdx, 9 * Cout * 8, 1.0, "conv3x3_bwd_data dx"), guard)
    assert kind == "bwd_weight"
    return Case("conv3x3_bwd_weight", lambda: [nan(3, 3, Cin, Cout)],
                lambda p, n, o: X.call("myolo_conv3x3_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(o[0]), N, H, W, Cin, Cout, p, n, X.stream()),
                lambda o: exact(o[0], rdw, N * H * W * 16, 1.0, "conv3x3_bwd_weight dw"), guard)


@functools.lru_cache(maxsize=None)
def pw_case(kind, M, Cin, Cout, options=()):
    """myolo_pwconv1x1_fwd ("bias" / "plain") / _affine_act_fwd ("affine") / _bwd_data / _bwd_weight / _bwd_weight_affine_in"""
    rng = np.random.default_rng(202)
    lim = 2 if M > 8192 else 4
    x, w, b, dy = ints(rng, (M, Cin), -lim, lim), ints(rng, (Cin, Cout), -2, 2), ints(rng, (Cout,), -8, 8), ints(rng, (M, Cout), -lim, lim)
    xt, wt, bt, dyt = dev(x), dev(w), dev(b), dev(dy)
    guard = 2 * X.workspace_bytes(M, Cin, Cout) + (80 * M * max(Cin, Cout) * 4 if M <= 1024 else 0)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    if kind in ("bias", "plain"):
        ref = x64 @ w64 + (b if kind == "bias" else 0)
        return Case("pwconv1x1_fwd(%s)" % kind, lambda: [nan(M, Cout)],
                    lambda p, n, o: X.call("myolo_pwconv1x1_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt) if kind == "bias" else None, X.ptr(o[0]), M, Cin, Cout, p, n, X.stream()),
                    lambda o: exact(o[0], ref, Cin * 8 + 8, 1.0, "pwconv1x1_fwd y"), guard, dict(options))
    if kind == "affine":
        sc, sh = affine(rng, Cout)
        sct, sht = dev(sc), dev(sh)
        ref = np.maximum((x64 @ w64) * sc + sh, 0)
        return Case("pwconv1x1_affine_act_fwd(relu)", lambda: [nan(M, Cout)],
                    lambda p, n, o: X.call("myolo_pwconv1x1_affine_act_fwd", X.ptr(xt), X.ptr(wt), X.ptr(sct), X.ptr(sht), 1, X.ptr(o[0]), M, Cin, Cout, p, n, X.stream()),
                    lambda o: exact(o[0], ref, Cin * 8 * 2 + 2, 0.25, "pwconv1x1_affine_act_fwd y"), guard, dict(options))
    if kind == "bwd_data":
        return Case("pwconv1x1_bwd_data", lambda: [nan(M, Cin)],
                    lambda p, n, o: X.call("myolo_pwconv1x1_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(o[0]), M, Cin, Cout, p, n, X.stream()),
                    lambda o: exact(o[0], dy64 @ w64.T, Cout * 8, 1.0, "pwconv1x1_bwd_data dx"), guard, dict(options))
    if kind == "bwd_weight":
        return Case("pwconv1x1_bwd_weight", lambda: [nan(Cin, Cout)],
                    lambda p, n, o: X.call("myolo_pwconv1x1_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(o[0]), M, Cin, Cout, p, n, X.stream()),
                    lambda o: exact(o[0], x64.T @ dy64, M * lim * lim, 1.0, "pwconv1x1_bwd_weight dw"), guard, dict(options))
    assert kind == "bwd_weight_affine_in"
    xp, isc, ish, _, a = pre_activation_operands(rng, (M, Cin), 2)
    xpt, isct, isht = dev(xp), dev(isc), dev(ish)
    return Case("pwconv1x1_bwd_weight_affine_in", lambda: [nan(Cin, Cout)],
                lambda p, n, o: X.call("myolo_pwconv1x1_bwd_weight_affine_in", X.ptr(xpt), X.ptr(isct), X.ptr(isht), 2, X.ptr(dyt), X.ptr(o[0]), M, Cin, Cout, p, n, X.stream()),
                lambda o: exact(o[0], a.astype(np.float64).T @ dy64, M * 6 * lim, 0.25, "pwconv1x1_bwd_weight_affine_in dw"), guard, dict(options))


@functools.lru_cache(maxsize=None)
def deconv_case(kind, N, H, W, Cin, Cout, options=()):
    """myolo_deconv2x2s2_fwd (ReLU) / _bwd_data / _bwd_weight on x, dy in -2..2, w in -2..2, bias in -8..8"""
    rng = np.random.default_rng(203)
    x, w, b = ints(rng, (N, H, W, Cin), -2, 2), ints(rng, (2, 2, Cout, Cin), -2, 2), ints(rng, (Cout,), -8, 8)
    dy = ints(rng, (N, 2 * H, 2 * W, Cout), -2, 2)
    xt, wt, bt, dyt = dev(x), dev(w), dev(b), dev(dy)
    M = N * H * W
    guard = 2 * X.workspace_bytes(M, Cin, Cout) + 4 * Cin * Cout * 8 + (80 * M * Cin * 4 if M <= 1024 else 0)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    if kind == "fwd":
        ref = np.maximum(O.deconv2x2s2(x64, w64, b.astype(np.float64)).astype(np.float64), 0)
        return Case("deconv2x2s2_fwd", lambda: [nan(N, 2 * H, 2 * W, Cout)],
                    lambda p, n, o: X.call("myolo_deconv2x2s2_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), X.ptr(o[0]), N, H, W, Cin, Cout, 1, p, n, X.stream()),
                    lambda o: exact(o[0], ref, Cin * 4 + 8, 1.0, "deconv2x2s2_fwd y"), guard, dict(options))
    rdx, rdw, _ = O.deconv2x2s2_bwd(x64, w64, dy64)
    if kind == "bwd_data":
        return Case("deconv2x2s2_bwd_data", lambda: [nan(N, H, W, Cin)],
                    lambda p, n, o: X.call("myolo_deconv2x2s2_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(o[0]), N, H, W, Cin, Cout, p, n, X.stream()),
                    lambda o: exact(o[0], rdx, 4 * Cout * 4, 1.0, "deconv2x2s2_bwd_data dx"), guard, dict(options))
    assert kind == "bwd_weight"
    return Case("deconv2x2s2_bwd_weight", lambda: [nan(2, 2, Cout, Cin)],
                lambda p, n, o: X.call("myolo_deconv2x2s2_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(o[0]), N, H, W, Cin, Cout, p, n, X.stream()),
                lambda o: exact(o[0], rdw, M * 4, 1.0, "deconv2x2s2_bwd_weight dw"), guard, dict(options))


@functools.lru_cache(maxsize=None)
def dw_wgrad_case(kind, N, H, W, C, S):
    """myolo_dwconv3x3_bwd_weight ("plain") / _bwd_weight_affine_in ("affine_in": ReLU6 of x * scale + shift formed on load)"""
    rng = np.random.default_rng(204)
    Ho, Wo = H // S, W // S
    dy = ints(rng, (N, Ho, Wo, C), -3, 3)
    dyt = dev(dy)
    wdummy = np.zeros((3, 3, C), np.float32)
    guard = X.dw_bwd_weight_ws_bytes(N, H, W, C, S)
    if kind == "plain":
        x = ints(rng, (N, H, W, C), -3, 3)
        xt = dev(x)
        _, ref = O.dwconv3x3_bwd(x, wdummy, dy, S)
        return Case("dwconv3x3_bwd_weight", lambda: [nan(3, 3, C)],
                    lambda p, n, o: X.call("myolo_dwconv3x3_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(o[0]), N, H, W, C, S, p, n, X.stream()),
                    lambda o: exact(o[0], ref, N * Ho * Wo * 9, 1.0, "dwconv3x3_bwd_weight dw"), guard)
    x, isc, ish, _, a = pre_activation_operands(rng, (N, H, W, C), 2)
    xt, isct, isht = dev(x), dev(isc), dev(ish)
    _, ref = O.dwconv3x3_bwd(a, wdummy, dy, S)
    return Case("dwconv3x3_bwd_weight_affine_in", lambda: [nan(3, 3, C)],
                lambda p, n, o: X.call("myolo_dwconv3x3_bwd_weight_affine_in", X.ptr(xt), X.ptr(isct), X.ptr(isht), 2, X.ptr(dyt), X.ptr(o[0]), N, H, W, C, S, p, n, X.stream()),
                lambda o: exact(o[0], ref, N * Ho * Wo * 18, 0.25, "dwconv3x3_bwd_weight_affine_in dw"), guard)


def bn_params(rng, C):
    gamma = (SCALES[rng.integers(0, 3, C)] * np.where(rng.random(C) < 0.2, -1, 1)).astype(np.float32)
    beta = (np.float32(0.25) * rng.integers(-8, 9, C)).astype(np.float32)
    return gamma, beta


def stats_outs(shape, C):
    """y, mean, var, scale, shift (NaN) and the moving averages (in / out: 0 and 1)"""
    return [nan(*shape)] + [nan(C) for _ in range(4)] + [torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]


def moving_averages(y2d, g, b, o):
    """the whole statistics set of stats_outs, moving_mean / moving_var included, through test_gpu_ops._check_bn_outputs (oracle.bn_train + bn_moving_update)"""
    C = y2d.shape[1]
    _check_bn_outputs(np.asarray(y2d, np.float32), g, b, np.zeros(C, np.float32), np.ones(C, np.float32), *o[1:7])


@functools.lru_cache(maxsize=None)
def dw_bnstats_case(N, H, W, C, S):
    rng = np.random.default_rng(205)
    x, isc, ish, _, a = pre_activation_operands(rng, (N, H, W, C), 2)
    w = two_tap_filters(rng, C)
    g, b = bn_params(rng, C)
    yref = O.dwconv3x3(a, w, S)
    t = [dev(v) for v in (x, isc, ish, w, g, b)]
    Ho, Wo = H // S, W // S

    def call(p, n, o):
        X.call("myolo_dwconv3x3_bnstats_fwd", X.ptr(t[0]), X.ptr(t[1]), X.ptr(t[2]), 2, X.ptr(t[3]), X.ptr(o[0]), X.ptr(t[4]), X.ptr(t[5]),
               X.ptr(o[1]), X.ptr(o[2]), X.ptr(o[3]), X.ptr(o[4]), X.ptr(o[5]), X.ptr(o[6]), N, H, W, C, S, 3, p, n, X.stream())

    def verify(o):
        exact(o[0], yref, 12, 0.25, "dw bnstats y")
        check_stats("dw bnstats", yref.reshape(-1, C), g, b, *o[1:5])
        moving_averages(yref.reshape(-1, C), g, b, o)
    return Case("dwconv3x3_bnstats_fwd", lambda: stats_outs((N, Ho, Wo, C), C), call, verify,
                X.dw_bnstats_ws_bytes(N, H, W, C, S))


@functools.lru_cache(maxsize=None)
def conv1_bnstats_case(N, H, W, Co):
    rng = np.random.default_rng(206)
    x, w = ints(rng, (N, H, W, 3), 0, 3), ints(rng, (3, 3, 3, Co), -2, 2)
    g, b = bn_params(rng, Co)
    yref = O.conv2d(x, w, stride=2, pads=O.conv1_pads(), acc=np.float64)
    t = [dev(v) for v in (x, w, g, b)]

    def call(p, n, o):
        X.call("myolo_conv3x3s2_c3_bnstats_fwd", X.ptr(t[0]), X.ptr(t[1]), X.ptr(o[0]), X.ptr(t[2]), X.ptr(t[3]), X.ptr(o[1]), X.ptr(o[2]), X.ptr(o[3]), X.ptr(o[4]),
               X.ptr(o[5]), X.ptr(o[6]), N, H, W, Co, 3, p, n, X.stream())

    def verify(o):
        exact(o[0], yref, 27 * 6, 1.0, "conv1 bnstats y")
        check_stats("conv1 bnstats", yref.reshape(-1, Co), g, b, *o[1:5])
        moving_averages(yref.reshape(-1, Co), g, b, o)
    return Case("conv3x3s2_c3_bnstats_fwd", lambda: stats_outs((N, H // 2, W // 2, Co), Co), call, verify, X.conv1_bnstats_ws_bytes(N, H, W, Co))


@functools.lru_cache(maxsize=None)
def pw_bnstats_case(M, Cin, Cout):
    """y = relu6(x * in_scale + in_shift) @ w with two +-1 entries per column of w (|y| <= 12: the sum of y^2 stays exact), and y's statistics"""
    rng = np.random.default_rng(207)
    x, isc, ish, _, a = pre_activation_operands(rng, (M, Cin), 2)
    w = np.zeros((Cin, Cout), np.float32)
    for _ in range(2):
        w[rng.integers(0, Cin, Cout), np.arange(Cout)] = rng.choice(np.array([-1, 1], np.float32), Cout)
    g, b = bn_params(rng, Cout)
    yref = a.astype(np.float64) @ w
    t = [dev(v) for v in (x, isc, ish, w, g, b)]

    def call(p, n, o):
        X.call("myolo_pwconv1x1_bnstats_fwd", X.ptr(t[0]), X.ptr(t[1]), X.ptr(t[2]), 2, X.ptr(t[3]), X.ptr(o[0]), X.ptr(t[4]), X.ptr(t[5]),
               X.ptr(o[1]), X.ptr(o[2]), X.ptr(o[3]), X.ptr(o[4]), X.ptr(o[5]), X.ptr(o[6]), M, Cin, Cout, 3, p, n, X.stream())

    def verify(o):
        exact(o[0], yref, 12, 0.25, "pw bnstats y")
        check_stats("pw bnstats", yref, g, b, *o[1:5])
        moving_averages(yref, g, b, o)
    return Case("pwconv1x1_bnstats_fwd", lambda: stats_outs((M, Cout), Cout), call, verify, X.pw_bnstats_ws_bytes(M, Cin, Cout))


@functools.lru_cache(maxsize=None)
def matmul_case(products, M, K, N, b_is_nk):
    rng = np.random.default_rng(208)
    A, B = ints(rng, (M, K), -8, 8), ints(rng, (N, K) if b_is_nk else (K, N), -8, 8)
    At, Bt = dev(A), dev(B)
    ref = A.astype(np.float64) @ (B.T if b_is_nk else B).astype(np.float64)
    return Case("matmul_f32(products=%d)" % products, lambda: [nan(M, N)],
                lambda p, n, o: X.call("myolo_matmul_f32", X.ptr(At), X.ptr(Bt), X.ptr(o[0]), M, K, N, b_is_nk, products, p, n, X.stream()),
                lambda o: exact(o[0], ref, K * 64, 1.0, "matmul_f32 C"), X.matmul_ws_bytes(K, N, b_is_nk, products))


@functools.lru_cache(maxsize=None)
def mask_sel_case(C, ids):
    """myolo_mask_head_out_bwd_sel (test_gpu_exact_sums.test_mask_head_out_bwd_sel_exact's operands)"""
    rng = np.random.default_rng(209)
    hw, Cin = 784, 256
    ids = np.array(ids, np.int32)
    NR = len(ids)
    M = NR * hw
    x = np.maximum(ints(rng, (M, Cin), -3, 3), 0)
    w = ints(rng, (Cin, C), -2, 2)
    dzs = ints(rng, (M,), -2, 2) * np.repeat(ids > 0, hw)
    dz = np.zeros((M, C), np.float64)
    dz[np.arange(M), np.repeat(ids, hw)] = dzs
    dz[:, 0] = 0
    t = [dev(x), dev(w), dev(dzs.astype(np.float32)), dev(ids)]
    x64, w64 = x.astype(np.float64), w.astype(np.float64)

    def verify(o):
        exact(o[0], (dz @ w64.T) * (x > 0), 8, 1.0, "mask sel dx")
        exact(o[1], x64.T @ dz, M * 6, 1.0, "mask sel dw")
        exact(o[2], dz.sum(0), M * 2, 1.0, "mask sel db")
    return Case("mask_head_out_bwd_sel", lambda: [nan(M, Cin), nan(Cin, C), nan(C)],
                lambda p, n, o: X.call("myolo_mask_head_out_bwd_sel", X.ptr(t[0]), X.ptr(t[1]), X.ptr(t[2]), X.ptr(t[3]), X.ptr(o[0]), X.ptr(o[1]), X.ptr(o[2]),
                                       M, Cin, C, hw, p, n, X.stream()),
                verify, X.mask_bwd_sel_ws_bytes(NR, Cin))


@functools.lru_cache(maxsize=None)
def conv7_case(kind, N, H, W, Co):
    """myolo_conv7x7s2_c3_fwd / _bnstats_fwd / _affine_act_fwd / _bwd_weight (ZeroPadding2D(3) + 7x7 stride 2) on x in 0..3, w, dy in -2..2, bias in -8..8"""
    rng = np.random.default_rng(210)
    x, w, b = ints(rng, (N, H, W, 3), 0, 3), ints(rng, (7, 7, 3, Co), -2, 2), ints(rng, (Co,), -8, 8)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = ints(rng, (N, Ho, Wo, Co), -2, 2)
    xt, wt, bt, dyt = dev(x), dev(w), dev(b), dev(dy)
    pads = (3, 3, 3, 3)
    guard = X.conv7x7s2_ws_bytes(N, H, W, Co)
    if kind == "bnstats":
        # the training stem: two +-1 taps per output channel on x in 0..1, bias in -1..1, so that the sum of y^2 stays exact (check_stats' precondition)
        x1 = ints(rng, (N, H, W, 3), 0, 1)
        w2 = np.zeros((147, Co), np.float32)
        for _ in range(2):
            w2[rng.integers(0, 147, Co), np.arange(Co)] = rng.choice(np.array([-1, 1], np.float32), Co)
        w2 = w2.reshape(7, 7, 3, Co)
        b1 = ints(rng, (Co,), -1, 1)
        g, be = bn_params(rng, Co)
        yref = O.conv2d(x1, w2, stride=2, pads=pads, bias=b1, acc=np.float64)
        t = [dev(v) for v in (x1, w2, b1, g, be)]

        def verify(o):
            exact(o[0], yref, 3, 1.0, "conv7x7 bnstats y")
            check_stats("conv7x7 bnstats", yref.reshape(-1, Co), g, be, *o[1:5])
            moving_averages(yref.reshape(-1, Co), g, be, o)
        return Case("conv7x7s2_c3_bnstats_fwd", lambda: stats_outs((N, Ho, Wo, Co), Co),
                    lambda p, n, o: X.call("myolo_conv7x7s2_c3_bnstats_fwd", X.ptr(t[0]), X.ptr(t[1]), X.ptr(t[2]), X.ptr(o[0]), X.ptr(t[3]), X.ptr(t[4]),
                                           *[X.ptr(v) for v in o[1:7]], N, H, W, Co, p, n, X.stream()),
                    verify, guard)
    if kind == "affine":
        sc, sh = affine(rng, Co)
        sct, sht = dev(sc), dev(sh)
        ref = np.maximum(O.conv2d(x, w, stride=2, pads=pads, bias=b, acc=np.float64).astype(np.float64) * sc + sh, 0)
        return Case("conv7x7s2_c3_affine_act_fwd(relu)", lambda: [nan(N, Ho, Wo, Co)],
                    lambda p, n, o: X.call("myolo_conv7x7s2_c3_affine_act_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), X.ptr(sct), X.ptr(sht), 1, X.ptr(o[0]),
                                           N, H, W, Co, p, n, X.stream()),
                    lambda o: exact(o[0], ref, (147 * 6 + 8) * 2 + 2, 0.25, "conv7x7 affine_act y"), guard)
    if kind == "fwd":
        ref = O.conv2d(x, w, stride=2, pads=pads, bias=b, acc=np.float64)
        assert ref.shape == (N, Ho, Wo, Co)
        return Case("conv7x7s2_c3_fwd", lambda: [nan(N, Ho, Wo, Co)],
                    lambda p, n, o: X.call("myolo_conv7x7s2_c3_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), X.ptr(o[0]), N, H, W, Co, p, n, X.stream()),
                    lambda o: exact(o[0], ref, 147 * 6 + 8, 1.0, "conv7x7 y"), guard)
    _, rdw, rdb = O.conv2d_bwd(x, w, dy, stride=2, pads=pads, acc=np.float64, need_dx=False)

    def verify(o):
        exact(o[0], rdw, N * Ho * Wo * 6, 1.0, "conv7x7 dw")
        exact(o[1], rdb, N * Ho * Wo * 2, 1.0, "conv7x7 db")
    return Case("conv7x7s2_c3_bwd_weight", lambda: [nan(7, 7, 3, Co), nan(Co)],
                lambda p, n, o: X.call("myolo_conv7x7s2_c3_bwd_weight", X.ptr(xt), X.ptr(dyt), X.ptr(o[0]), X.ptr(o[1]), N, H, W, Co, p, n, X.stream()),
                verify, guard)


@functools.lru_cache(maxsize=None)
def deconv_mask_case(N, H, W, Cin, Cout, C):
    """myolo_deconv2x2s2_mask_fwd (test_gpu_ops.test_deconv_mask_fused's operands): sigmoid outputs, held to test_gpu_ops.check at TOL"""
    rng = np.random.default_rng(4)
    rnd = lambda *s, scale=1.0: (rng.standard_normal(s) * scale).astype(np.float32)      # noqa: E731
    x, w, b = rnd(N, H, W, Cin), rnd(2, 2, Cout, Cin, scale=0.05), rnd(Cout)
    w2, b2 = rnd(Cout, C, scale=0.1), rnd(C)
    t = [dev(v) for v in (x, w, b, w2, b2)]
    d = O.relu(O.deconv2x2s2(x, w, b)).astype(np.float64)
    ref = 1 / (1 + np.exp(-(d.reshape(-1, Cout) @ w2 + b2))).reshape(N, 2 * H, 2 * W, C)
    return Case("deconv2x2s2_mask_fwd", lambda: [nan(N, 2 * H, 2 * W, C)],
                lambda p, n, o: X.call("myolo_deconv2x2s2_mask_fwd", X.ptr(t[0]), X.ptr(t[1]), X.ptr(t[2]), X.ptr(t[3]), X.ptr(t[4]), X.ptr(o[0]), N, H, W, Cin, Cout, C, p, n, X.stream()),
                lambda o: check(o[0], ref, TOL, "fused deconv+mask"), X.deconv_mask_ws_bytes(N, H, W, Cin, Cout, C))


def _rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wino_operands(N, H, W, Cin, Cout):
    """test_gpu_ops.test_conv3x3_winograd's operands and float64 references, computed once"""
    rng = np.random.default_rng(2)
    x, w, b = _rnd(rng, N, H, W, Cin), _rnd(rng, 3, 3, Cin, Cout, scale=0.05), _rnd(rng, Cout)
    dy = _rnd(rng, N, H, W, Cout)
    ref = O.conv2d(x, w, pads=(1, 1, 1, 1), bias=b, acc=np.float64)
    rdx, rdw, _ = O.conv2d_bwd(x, w, dy, pads=(1, 1, 1, 1), acc=np.float64)
    return dict(t=[dev(v) for v in (x, w, b, dy)], y=ref, dx=rdx, dw=rdw)


def wino_case(which, N, H, W, Cin, Cout, options=()):
    """myolo_conv3x3_wino_{fwd, bwd_data, bwd_weight (from x)} against the float64 oracle through test_gpu_ops.check (TOL)"""
    k = wino_operands(N, H, W, Cin, Cout)
    xt, wt, bt, dyt = k["t"]
    guard = max(X.wino_ws_bytes(N, H, W, Cin, Cout, j) for j in (0, 1, 2))
    with X.option("wino_x6", dict(options).get("wino_x6", 0)):
        guard = max([guard] + [X.wino_ws_bytes(N, H, W, Cin, Cout, j) for j in (0, 1, 2)])
    if which == 0:
        return Case("conv3x3_wino_fwd", lambda: [nan(N, H, W, Cout)],
                    lambda p, n, o: X.call("myolo_conv3x3_wino_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), None, None, X.ptr(o[0]), N, H, W, Cin, Cout, 0, None, p, n, X.stream()),
                    lambda o: check(o[0], k["y"], what="wino fwd"), guard, dict(options))
    if which == 1:
        return Case("conv3x3_wino_bwd_data", lambda: [nan(N, H, W, Cin)],
                    lambda p, n, o: X.call("myolo_conv3x3_wino_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(o[0]), N, H, W, Cin, Cout, p, n, X.stream()),
                    lambda o: check(o[0], k["dx"], what="wino dx"), guard, dict(options))
    return Case("conv3x3_wino_bwd_weight", lambda: [nan(3, 3, Cin, Cout)],
                lambda p, n, o: X.call("myolo_conv3x3_wino_bwd_weight", X.ptr(xt), None, X.ptr(dyt), X.ptr(o[0]), N, H, W, Cin, Cout, p, n, X.stream()),
                lambda o: check(o[0], k["dw"], what="wino dw (from x)"), guard, dict(options))


def wino63_case(which, N, Cin, Cout):
    """myolo_conv3x3_wino63_{fwd, bwd_data, bwd_weight (from x)} (test_gpu_ops.test_winograd_f63_conv_operators) through test_gpu_ops.check (TOL)"""
    k = wino_operands(N, 14, 14, Cin, Cout)
    xt, wt, bt, dyt = k["t"]
    guard = max(X.wino63_ws_bytes(N, Cin, Cout, j) for j in (0, 1, 2))
    if which == 0:
        return Case("conv3x3_wino63_fwd", lambda: [nan(N, 14, 14, Cout)],
                    lambda p, n, o: X.call("myolo_conv3x3_wino63_fwd", X.ptr(xt), X.ptr(wt), X.ptr(bt), None, None, X.ptr(o[0]), N, Cin, Cout, 0, None, p, n, X.stream()),
                    lambda o: check(o[0], k["y"], what="wino63 fwd"), guard)
    if which == 1:
        assert X.wino63_ok(14, 14, Cout, Cin)
        return Case("conv3x3_wino63_bwd_data", lambda: [nan(N, 14, 14, Cin)],
                    lambda p, n, o: X.call("myolo_conv3x3_wino63_bwd_data", X.ptr(dyt), X.ptr(wt), X.ptr(o[0]), N, Cin, Cout, p, n, X.stream()),
                    lambda o: check(o[0], k["dx"], what="wino63 dx"), guard)
    return Case("conv3x3_wino63_bwd_weight", lambda: [nan(3, 3, Cin, Cout)],
                lambda p, n, o: X.call("myolo_conv3x3_wino63_bwd_weight", X.ptr(xt), None, X.ptr(dyt), X.ptr(o[0]), N, Cin, Cout, p, n, X.stream()),
                lambda o: check(o[0], k["dw"], what="wino63 dw (from x)"), guard)


@functools.lru_cache(maxsize=None)
def conv1_pieces():
    """The mask head's conv1 on the F(6,3) tiling, as test_gpu_ops.test_winograd_f63_conv1_pieces builds it: M planes of a conv, the lazily formed output
    gradient, its V / Q transforms -- and, as references, every scratch-taking piece run once on ample zeroed scratch (the runs that op test holds to
    the F(4,3) kernels) plus the F(4,3) results themselves."""
    rng = np.random.default_rng(12)
    B, FH, FW, C, nb, Co = 2, 28, 28, 256, 9, 256
    st = X.stream()
    img = _rnd(rng, B, FH, FW, C)
    y1 = rng.random((nb, 1)).astype(np.float32) * 0.5
    boxes = np.concatenate([y1, y1 * 0.7, y1 + 0.4, y1 * 0.7 + 0.45], 1).astype(np.float32)
    bind = rng.integers(0, B, nb).astype(np.int32)
    a = [dev(img), dev(boxes), dev(bind)]
    ap = tuple(X.ptr(t) for t in a)
    V2 = nan(X.wino63_plane_elems(nb, C))
    X.call("myolo_wino63_input_transform_roialign", *ap, X.ptr(V2), B, FH, FW, C, nb, st)
    w_t, b_t = dev(_rnd(rng, 3, 3, C, Co, scale=0.05)), dev(_rnd(rng, Co))
    U, M = torch.empty(X.wino63_u_elems(C, Co), device=DEV), torch.empty(X.wino63_plane_elems(nb, Co), device=DEV)
    X.call("myolo_wino63_weight_transform", X.ptr(w_t), X.ptr(U), C, Co, st)
    X.call("myolo_wino63_multiply", X.ptr(V2), X.ptr(U), X.ptr(M), nb, C, Co, st)
    gamma, beta = dev(1 + 0.1 * _rnd(rng, Co)), dev(_rnd(rng, Co, scale=0.1))
    y_pre = nan(nb, 14, 14, Co)
    X.call("myolo_wino63_boundary", X.ptr(M), X.ptr(b_t), None, None, 0, X.ptr(y_pre), None, 0, None, 0, None, nb, Co, st)
    big = torch.zeros(256 << 20, dtype=torch.uint8, device=DEV)
    wsa = (big.data_ptr(), big.numel())
    stats = [nan(Co) for _ in range(4)] + [torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)]
    X.call("myolo_bn_stats", X.ptr(y_pre), X.ptr(gamma), X.ptr(beta), *[X.ptr(t) for t in stats], nb * 196, Co, *wsa, st)
    sc, sh = stats[2], stats[3]
    npos = 4
    inv = np.full(nb, -1, np.int32)
    inv[[1, 4, 7, 8]] = np.arange(npos)
    inv_t, dyc = dev(inv), dev(_rnd(rng, npos, 196, Co))
    ka, kb = dev(_rnd(rng, Co, scale=0.01)), dev(_rnd(rng, Co, scale=0.01))
    lazy = (X.ptr(y_pre), X.ptr(dyc), X.ptr(inv_t), X.ptr(sc), X.ptr(sh), X.ptr(ka), X.ptr(kb), 1)
    V43 = nan(36, nb * 16, C)
    X.call("myolo_wino_input_transform_roialign", *ap, X.ptr(V43), B, FH, FW, C, nb, 14, 14, st)
    dw43, dx43, dw63, dx63 = nan(3, 3, C, Co), nan(nb, 14, 14, C), nan(3, 3, C, Co), nan(nb, 14, 14, C)
    X.call("myolo_conv3x3_wino_bwd_weight_lazybn", X.ptr(V43), *lazy, X.ptr(dw43), nb, 14, 14, C, Co, *wsa, st)
    X.call("myolo_conv3x3_wino_bwd_data_lazybn", *lazy, X.ptr(w_t), X.ptr(dx43), nb, 14, 14, C, Co, *wsa, st)
    X.call("myolo_wino63_bwd_weight_lazybn", X.ptr(V2), *lazy, X.ptr(dw63), nb, C, Co, *wsa, st)
    X.call("myolo_wino63_bwd_data_lazybn", *lazy, X.ptr(w_t), X.ptr(dx63), nb, C, Co, *wsa, st)
    pe = X.wino63_plane_elems(nb, Co)
    Vd, Qd = nan(pe), nan(pe)
    X.call("myolo_wino63_lazybn_transforms", *lazy, X.ptr(Vd), X.ptr(Qd), nb, Co, st)
    torch.cuda.synchronize()
    del big
    return dict(nb=nb, C=C, Co=Co, V2=V2, M=M, b=b_t, gamma=gamma, beta=beta, y_pre=y_pre, stats=stats, lazy=lazy, w=w_t, Vd=Vd, Qd=Qd,
                dw43=dw43, dx43=dx43, dw63=dw63, dx63=dx63, keep=(a, U, inv_t, dyc, ka, kb, sc, sh, V43))


def _bits_and_check(got, same, near, what):
    """a conv1 piece: the bits of the same entry on ample scratch, and the F(4,3) kernel's result on the same operands within the op test's bound
    (test_gpu_ops.check_f63_equals_f43, as test_winograd_f63_conv1_pieces asserts it)"""
    assert bool(torch.isfinite(got).all()), what
    assert torch.equal(got, same), "%s: bits differ from the run on ample scratch" % what
    check_f63_equals_f43(got, near, what)


def wino63_piece_case(kind):
    k = conv1_pieces()
    nb, C, Co, st = k["nb"], k["C"], k["Co"], X.stream
    if kind == "bwd_weight":
        return Case("wino63_bwd_weight_lazybn", lambda: [nan(3, 3, C, Co)],
                    lambda p, n, o: X.call("myolo_wino63_bwd_weight_lazybn", X.ptr(k["V2"]), *k["lazy"], X.ptr(o[0]), nb, C, Co, p, n, st()),
                    lambda o: _bits_and_check(o[0], k["dw63"], k["dw43"], "wino63 lazybn dw"), X.wino63_bwd_weight_ws_bytes(nb, C, Co))
    if kind == "bwd_data":
        return Case("wino63_bwd_data_lazybn", lambda: [nan(nb, 14, 14, C)],
                    lambda p, n, o: X.call("myolo_wino63_bwd_data_lazybn", *k["lazy"], X.ptr(k["w"]), X.ptr(o[0]), nb, C, Co, p, n, st()),
                    lambda o: _bits_and_check(o[0], k["dx63"], k["dx43"], "wino63 lazybn dx"), X.wino63_bwd_data_ws_bytes(nb, C, Co))
    if kind == "from_v":
        return Case("wino63_bwd_data_from_v", lambda: [nan(nb, 14, 14, C)],
                    lambda p, n, o: X.call("myolo_wino63_bwd_data_from_v", X.ptr(k["Vd"]), X.ptr(k["w"]), X.ptr(o[0]), nb, C, Co, p, n, st()),
                    lambda o: _bits_and_check(o[0], k["dx63"], k["dx43"], "wino63 dx from V"), X.wino63_bwd_data_from_v_ws_bytes(nb, C, Co))
    if kind == "from_q":
        return Case("wino63_bwd_weight_from_q", lambda: [nan(3, 3, C, Co)],
                    lambda p, n, o: X.call("myolo_wino63_bwd_weight_from_q", X.ptr(k["V2"]), X.ptr(k["Qd"]), X.ptr(o[0]), nb, C, Co, p, n, st()),
                    lambda o: _bits_and_check(o[0], k["dw63"], k["dw43"], "wino63 dw from Q"), X.wino63_bwd_weight_from_q_ws_bytes(nb, C, Co))
    assert kind == "out_bn"

    def verify(o):
        assert torch.equal(o[0], k["y_pre"]), "wino63 output transform + statistics: y differs from the plain boundary's"
        check_stats_agree(o[1:7], k["stats"], "wino63 out_bn")                      # the six statistics against myolo_bn_stats of the same y
        check_mean_var_float64(o[1], o[2], k["y_pre"].view(-1, Co), "wino63 out_bn")
    return Case("wino63_output_transform_bn_stats", lambda: stats_outs((nb, 14, 14, Co), Co),
                lambda p, n, o: X.call("myolo_wino63_output_transform_bn_stats", X.ptr(k["M"]), X.ptr(k["b"]), X.ptr(o[0]), nb, Co, X.ptr(k["gamma"]), X.ptr(k["beta"]),
                                       X.ptr(o[1]), X.ptr(o[2]), X.ptr(o[3]), X.ptr(o[4]), X.ptr(o[5]), X.ptr(o[6]), p, n, st()),
                verify, X.wino63_out_bn_ws_bytes(nb, Co))


@functools.lru_cache(maxsize=None)
def wino_out_bn_case(N, H, W, C):
    """myolo_wino_output_transform_bn_stats (test_gpu_ops.test_winograd_transforms_with_folded_batchnorm): y = the plain output transform's bits, the six
    statistics = myolo_bn_stats of it (check_stats_agree), mean / var = the float64 statistics of y (check_mean_var_float64)"""
    rng = np.random.default_rng(11)
    T = N * ((H + 3) // 4) * ((W + 3) // 4)
    t = [dev(v) for v in (_rnd(rng, 36, T, C), _rnd(rng, C), 1 + 0.1 * _rnd(rng, C), _rnd(rng, C, scale=0.1))]
    y_ref = nan(N * H * W, C)
    st = X.stream()
    X.call("myolo_wino_output_transform", X.ptr(t[0]), X.ptr(t[1]), None, None, X.ptr(y_ref), N, H, W, C, 0, st)
    big = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    stats = [nan(C) for _ in range(4)] + [torch.zeros(C, device=DEV), torch.ones(C, device=DEV)]
    X.call("myolo_bn_stats", X.ptr(y_ref), X.ptr(t[2]), X.ptr(t[3]), *[X.ptr(s) for s in stats], N * H * W, C, big.data_ptr(), big.numel(), st)
    torch.cuda.synchronize()

    def verify(o):
        assert torch.equal(o[0], y_ref)
        check_stats_agree(o[1:7], stats, "wino out_bn")                              # the six statistics against myolo_bn_stats of the same y
        check_mean_var_float64(o[1], o[2], y_ref, "wino out_bn")
    return Case("wino_output_transform_bn_stats", lambda: stats_outs((N * H * W, C), C),
                lambda p, n, o: X.call("myolo_wino_output_transform_bn_stats", X.ptr(t[0]), X.ptr(t[1]), X.ptr(o[0]), N, H, W, C, X.ptr(t[2]), X.ptr(t[3]),
                                       X.ptr(o[1]), X.ptr(o[2]), X.ptr(o[3]), X.ptr(o[4]), X.ptr(o[5]), X.ptr(o[6]), p, n, X.stream()),
                verify, X.wino_out_bn_ws_bytes(C))


@functools.lru_cache(maxsize=None)
def augment_case(H, W, T):
    """myolo_augment_batch on test_gpu_augment.test_c_abi_ragged_tail_and_other_slot_count's operands, against the numpy restatement of its arithmetic
    contract (tests/augment_ref.py) bit for bit"""
    import augment_ref as R
    rs = np.random.RandomState(5)
    B, G, A, C = 3, 2, 2, 2
    images = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    masks = np.zeros((B, H, W, T), np.uint8)
    masks[0, 5:20, 8:30, 0] = 1
    masks[0, 25:40, 0:12, 2] = 1
    masks[1, 0:40, 0:40, 1] = 1
    masks[1, 10:12, 10:12, 2] = 1
    masks[2, 30:36, 30:40, 0] = 1
    masks[2, 2:9, 3:7, 1] = 1
    masks[2, 18:22, 18:22, 2] = 1
    ids = np.zeros((B, T), np.int32)
    ids[:, :3] = [[1, 0, 1], [0, 1, 0], [1, 1, 1]]
    th = np.radians(20.)
    rows = np.array([[1, 0, 0, 0, 1, 0, 1, 0],
                     [np.cos(th) / .8, np.sin(th) / .8, 3.25, -np.sin(th) / .8, np.cos(th) / .8, -6.5, 1.1, -9.],
                     [-1.2, 0, 44.5, 0, 1.2, -4.75, .9, 12.]], np.float64)
    anchors = np.array([0.6, 0.7, 1.4, 1.2], np.float64)
    cval = 37.0
    want = R.augment_batch(images, masks, ids, rows, cval, H, W, T, G, A, C, anchors)
    src = [dev(a) for a in (images, masks, ids, rows, anchors)]
    keys = ("images", "gt_masks", "gt_boxes", "gt_ids", "y_true", "true_boxes")

    def outs():
        return [torch.full((B, H, W, 3), float("nan"), device=DEV), torch.full((B, H, W, T), 9, dtype=torch.uint8, device=DEV),
                torch.full((B, T, 4), -1, dtype=torch.int32, device=DEV), torch.full((B, T), -1, dtype=torch.int32, device=DEV),
                torch.full((B, G, G, A, 5 + C), float("nan"), device=DEV), torch.full((B, T, 4), float("nan"), device=DEV)]

    def verify(o):
        for k, t in zip(keys, o):
            got = t.cpu().numpy()
            assert got.dtype == want[k].dtype and got.shape == want[k].shape, k
            assert got.tobytes() == want[k].tobytes(), (k, int((got != want[k]).sum()))
    return Case("augment_batch", outs,
                lambda p, n, o: X.call("myolo_augment_batch", X.ptr(src[0]), X.ptr(src[1]), X.ptr(src[2]), X.ptr(src[3]), cval, X.ptr(src[4]),
                                       *[X.ptr(t) for t in o], B, H, W, T, G, A, C, p, n, X.stream()),
                verify, X.augment_ws_bytes(B, T))


# ============================================================================================================================================
# Part 1: the planner contract
# ============================================================================================================================================
# planner -> (builder of the entry's Case, planner figure, the entry refuses anything below the planner figure (MYOLO_NEED_WS of that figure))
WINO = (2, 14, 14, 64, 256)
W63 = (3, 256, 256)
PLANNERS = {
    "workspace_bytes/conv3x3_bwd_weight": (lambda: conv3_case("bwd_weight", 2, 14, 14, 32, 64), lambda: X.workspace_bytes(2 * 196, 32, 64), False),
    "workspace_bytes/conv3x3_bwd_data": (lambda: conv3_case("bwd_data", 2, 14, 14, 32, 64), lambda: X.workspace_bytes(2 * 196, 32, 64), False),
    "workspace_bytes/pwconv1x1_bwd_weight": (lambda: pw_case("bwd_weight", 1568, 64, 128), lambda: X.workspace_bytes(1568, 64, 128), False),
    "workspace_bytes/deconv2x2s2_bwd_weight": (lambda: deconv_case("bwd_weight", 2, 14, 14, 64, 64), lambda: X.workspace_bytes(2 * 196, 64, 64), False),
    "wino_ws_bytes(0)": (lambda: wino_case(0, *WINO), lambda: X.wino_ws_bytes(*WINO, 0), True),
    "wino_ws_bytes(1)": (lambda: wino_case(1, *WINO), lambda: X.wino_ws_bytes(*WINO, 1), True),
    "wino_ws_bytes(2)": (lambda: wino_case(2, *WINO), lambda: X.wino_ws_bytes(*WINO, 2), True),
    "wino63_ws_bytes(0)": (lambda: wino63_case(0, *W63), lambda: X.wino63_ws_bytes(*W63, 0), True),
    "wino63_ws_bytes(1)": (lambda: wino63_case(1, *W63), lambda: X.wino63_ws_bytes(*W63, 1), True),
    "wino63_ws_bytes(2)": (lambda: wino63_case(2, *W63), lambda: X.wino63_ws_bytes(*W63, 2), True),
    "wino63_bwd_weight_ws_bytes": (lambda: wino63_piece_case("bwd_weight"), None, True),
    "wino63_bwd_data_ws_bytes": (lambda: wino63_piece_case("bwd_data"), None, True),
    "wino63_bwd_data_from_v_ws_bytes": (lambda: wino63_piece_case("from_v"), None, True),
    "wino63_bwd_weight_from_q_ws_bytes": (lambda: wino63_piece_case("from_q"), None, True),
    "wino63_out_bn_ws_bytes": (lambda: wino63_piece_case("out_bn"), None, True),
    "wino_out_bn_ws_bytes": (lambda: wino_out_bn_case(3, 9, 6, 64), None, True),
    "matmul_ws_bytes(native)": (lambda: matmul_case(X.PRODUCTS_NATIVE, 300, 256, 256, 1), None, False),
    "matmul_ws_bytes(bf16x6)": (lambda: matmul_case(X.PRODUCTS_BF16X6, 300, 256, 256, 1), None, True),
    "matmul_ws_bytes(bf16x6,kn)": (lambda: matmul_case(X.PRODUCTS_BF16X6, 300, 256, 256, 0), None, True),
    "conv1_bnstats_ws_bytes": (lambda: conv1_bnstats_case(2, 32, 32, 16), None, True),
    "dw_bnstats_ws_bytes": (lambda: dw_bnstats_case(2, 16, 16, 32, 1), None, True),
    "dw_bnstats_ws_bytes(generic)": (lambda: dw_bnstats_case(2, 9, 13, 16, 1), None, True),
    "dw_bwd_weight_ws_bytes": (lambda: dw_wgrad_case("plain", 2, 16, 16, 32, 1), None, False),
    "dw_bwd_weight_ws_bytes(affine_in)": (lambda: dw_wgrad_case("affine_in", 2, 16, 16, 32, 2), None, False),
    "pw_bnstats_ws_bytes": (lambda: pw_bnstats_case(300, 64, 64), None, True),
    "pw_bnstats_ws_bytes(split-K)": (lambda: pw_bnstats_case(300, 512, 128), None, True),
    "deconv_mask_ws_bytes": (lambda: deconv_mask_case(2, 5, 7, 32, 128, 1), None, True),
    "mask_bwd_sel_ws_bytes": (lambda: mask_sel_case(8, (2, 0, 7, 2, 5, 0)), None, True),
    "augment_ws_bytes": (lambda: augment_case(40, 40, 3), None, True),
    "conv7x7s2_ws_bytes/bnstats_fwd": (lambda: conv7_case("bnstats", 2, 32, 32, 64), None, False),          # (its minimum: test_conv7x7_stem_minimum)
    "conv7x7s2_ws_bytes/affine_act_fwd": (lambda: conv7_case("affine", 2, 32, 32, 64), None, False),
    "conv7x7s2_ws_bytes/fwd": (lambda: conv7_case("fwd", 2, 32, 32, 64), None, False),
    "conv7x7s2_ws_bytes/bwd_weight": (lambda: conv7_case("bwd_weight", 2, 32, 32, 64), None, False),
}


@pytest.mark.parametrize("planner", list(PLANNERS))
def test_entry_at_its_planner_bytes(planner):
    """the entry at exactly the planner's bytes: succeeds, guard intact, 0xFF scratch gives the bits of 0x00 scratch, result correct; where the figure is a
    hard minimum, 256 bytes less raises the workspace error with every output untouched"""
    build, figure, hard = PLANNERS[planner]
    case = build()
    need = figure() if figure else case.guard          # (a Case's guard is its planner figure unless the table gives the figure)
    assert case.guard >= need
    _, words = both_fills(case, need)
    print("%s: %s at %d bytes overwrote %d scratch words" % (planner, case.name, need, words))
    assert words * 4 <= need
    if hard and need > 0:
        expect_ws_error(case, max(need - 256, 0))


# ============================================================================================================================================
# Part 2: the size sweep
# ============================================================================================================================================
def nn_sweep(case, MN, base):
    """ws_bytes = base + j M N 4 for j = 0 .. max_splits + 1 (max_splits: what an unclipped run used).  The split count of each call is read off the poisoned
    scratch: words overwritten, less the weight region, over M N.  Every size exact (both_fills).  -> {j: splits}"""
    per = MN * 4

    def splits_of(words):
        w = words - base // 4
        assert w >= 0 and w % MN == 0, "%s: %d words beyond the weight region are no whole number of [M][N] partials" % (case.name, w)
        return max(w // MN, 1)
    assert case.guard >= base + 64 * per
    _, words = run_at(case, base + 64 * per, 0xFF)
    top = splits_of(words)
    seen = {}
    for j in range(top + 2):
        _, words = both_fills(case, base + j * per)
        seen[j] = splits_of(words)
        assert seen[j] <= max(j, 1), "%s: %d splits on scratch for %d" % (case.name, seen[j], j)
    print("%s: unclipped %d splits; partial slabs offered -> splits used: %s" % (case.name, top, ", ".join("%d->%d" % kv for kv in sorted(seen.items()))))
    return seen


# The two predicates below and the "empty last split" expression in the pointwise sweep restate one line of gemm_nn_fast -- split i of s owns the k tiles
# [i ceil(nk / s), (i + 1) ceil(nk / s)), k tiles of 16, CONV3 groups of 18 -- because the cases this file must show it reached (a ragged last split, an
# empty one, a mid-group start) are defined by it.  They only classify split counts that were OBSERVED; no size or split count is derived from them.
def ragged(nk, s):
    """the last of s splits of ceil(nk / s) k tiles owns fewer than the others (but some)"""
    per = -(-nk // s)
    return s > 1 and 0 < nk - (s - 1) * per < per


def mid_group(nk, s, group=18):
    """some split starts inside a group of `group` k tiles"""
    per = -(-nk // s)
    return any((i * per) % group for i in range(1, s) if i * per < nk)


CONV3_SWEEP = [("bias", 128, 48), ("plain", 128, 48), ("affine", 128, 48), ("bwd_data", 48, 128)]


@pytest.mark.parametrize("kind,Cin,Cout", CONV3_SWEEP, ids=[c[0] for c in CONV3_SWEEP])
def test_conv3x3_split_count_sweep(kind, Cin, Cout):
    """the 3x3 entries that reach launch_nn, one row tile (N = 1, H = 6, W = 10), 128 contraction channels (nk = 72 k tiles of 16, grouped CONV3 order):
    clipped split counts, a ragged last split, a split that starts mid-group"""
    N, H, W = 1, 6, 10
    case = conv3_case(kind, N, H, W, Cin, Cout)
    Cc, Nout = (Cout, Cin) if kind == "bwd_data" else (Cin, Cout)           # contraction channels, output columns
    nk = 9 * Cc // 16
    base = 9 * Cin * Cout * 4 if kind == "bwd_data" else 0                    # the transposed weights in front of the partials (a multiple of 256 here)
    assert base % 256 == 0 and Cc % 32 == 0
    seen = nn_sweep(case, N * H * W * Nout, base)
    counts = set(seen.values())
    assert len(counts) >= 3, "only the split counts %s were reached" % sorted(counts)
    assert any(ragged(nk, s) for s in counts), "no split count with a ragged last split among %s" % sorted(counts)
    assert any(mid_group(nk, s) for s in counts), "no split that starts mid-group among %s" % sorted(counts)
    if kind == "bwd_data":
        expect_ws_error(case, base - 256)


@pytest.mark.parametrize("kind", ["bias", "affine", "plain", "bwd_data"])
def test_pointwise_split_count_sweep_with_an_empty_last_split(kind):
    """PLAIN form, K = 1424 (nk = 89), two output tiles: eleven splits of nine k tiles leave the eleventh with none.  The three epilogues splitk_epilogue
    reproduces: bias, affine + ReLU, neither; and the data gradient (K = Cout), whose partials lie behind the transposed weights."""
    M, Cin, Cout = (200, 48, 1424) if kind == "bwd_data" else (200, 1424, 48)
    case = pw_case(kind, M, Cin, Cout, (("pw_no_smallm", 1),))
    nk = max(Cin, Cout) // 16
    base = Cin * Cout * 4 if kind == "bwd_data" else 0
    assert base % 256 == 0
    seen = nn_sweep(case, M * min(Cin, Cout), base)
    counts = set(seen.values())
    assert len(counts) >= 3, "only the split counts %s were reached" % sorted(counts)
    assert any(ragged(nk, s) for s in counts)
    empty = [s for s in counts if s > 1 and (s - 1) * -(-nk // s) >= nk]
    assert empty, "no split count whose last split owns no k tile among %s" % sorted(counts)
    print("split counts with an empty last split: %s" % empty)
    if base:
        expect_ws_error(case, base - 256)


def test_deconv_bwd_data_split_count_sweep():
    """myolo_deconv2x2s2_bwd_data's fp32 form (AM_DECONV, K = 4 Cout = 512: nk = 32), one row tile"""
    N, H, W, Cin, Cout = 1, 6, 10, 48, 128
    case = deconv_case("bwd_data", N, H, W, Cin, Cout)
    seen = nn_sweep(case, N * H * W * Cin, 0)
    counts = set(seen.values())
    assert len(counts) >= 3, "only the split counts %s were reached" % sorted(counts)
    assert any(ragged(4 * Cout // 16, s) for s in counts)


def fallbacks(case, lo, hi, want_paths, lowest_is_error=True):
    """find_paths over [lo, hi]; at least `want_paths` distinct successful paths; same bits at every size (integer operands)"""
    paths, outs = find_paths(case, lo, hi)
    show(case.name, paths)
    ok = [s for _, s in paths if s != "error"]
    assert len(set(ok)) >= want_paths, "%s: %d path(s) reached, %d expected: %s" % (case.name, len(set(ok)), want_paths, paths)
    if lowest_is_error:
        assert paths[0][1] == "error" and all(s != "error" for _, s in paths[1:]), paths
    same_bits(case, outs)
    return paths, outs


X6 = (("wino_x6", 1), ("pw_x6_min_rows", 128), ("pw_no_smallm", 1))


def test_pwconv1x1_bwd_data_fits_or_falls_back():
    """256 channels under FP32_MATMUL = "bf16x6": the NT kernel where its piece planes fit, the transposed-weights path (gemm_nn_fast, one split: the piece
    planes fit before a second slab of partials would) below, the workspace error below the weights"""
    M, Cin, Cout = 512, 256, 256
    case = pw_case("bwd_data", M, Cin, Cout, X6)
    fallbacks(case, 0, case.guard, 2)


@pytest.mark.parametrize("kind", ["bwd_weight", "bwd_weight_affine_in"])
def test_pwconv1x1_bwd_weight_fits_or_falls_back(kind):
    """the thin kernel (32 -> 64 channels from 16 384 rows) where its partials fit, launch_tn below, its error below that; and at 256 channels under "bf16x6"
    wino_tn_x6_kernel where the planner's figure fits, launch_tn below.  choose_splits does not look at the size: every size from the need up gives the bits
    of the exact-need run (same_bits), one step below the need gives the error."""
    M, Cin, Cout = 16384, 32, 64
    case = pw_case(kind, M, Cin, Cout)
    fallbacks(case, 0, case.guard, 2)
    M, Cin, Cout = 128 * 300, 256, 256          # (up to 256 slabs of 128 rows the two kernels ask for the same bytes: the fp32 kernel is reached only beyond)
    case = pw_case(kind, M, Cin, Cout, (("wino_x6", 1),))
    fallbacks(case, 0, case.guard, 2)


@pytest.mark.parametrize("kind,HW,Cin,Cout", [("fwd", (64, 64), 16, 256), ("bwd_data", (64, 64), 256, 16), ("bwd_weight", (150, 256), 256, 64)], ids=["fwd", "bwd_data", "bwd_weight"])
def test_deconv2x2s2_fits_or_falls_back(kind, HW, Cin, Cout):
    """the narrowest eligible channels under "bf16x6": the bf16x6 kernels where their pieces / partials fit, the fp32 kernels below; forward and weight
    gradient refuse what is below their need.  Forward and data gradient at 4096 input pixels, the hard-coded row floor of the bf16x6 forms.  The weight
    gradient at 38 400: up to 256 slabs of 128 pixels wino_tn_x6_kernel and launch_tn ask for the same bytes (seen at 4096 pixels: one threshold, 8 MiB,
    below it the error), so the fp32 kernel is reached "because the x6 partials do not fit" only beyond."""
    N, (H, W) = 1, HW
    case = deconv_case(kind, N, H, W, Cin, Cout, (("wino_x6", 1),))
    fallbacks(case, 0, case.guard, 2, lowest_is_error=kind != "bwd_data")


DW3 = [("plain", (1000, 2, 2, 512, 1)), ("affine_in", (1000, 2, 2, 512, 1)), ("plain", (1000, 4, 4, 512, 2))]


@pytest.mark.parametrize("kind,shape", DW3, ids=["plain-s1", "affine_in-s1", "plain-s2"])
def test_dwconv3x3_bwd_weight_reaches_its_three_kernels(kind, shape):
    """One shape that dw_rows_ok accepts and whose channel quads divide 256 -- a thousand images of 2 x 2 output pixels, 512 channels: a row of partials per
    image for dw_rows_wgrad_kernel, the tiled dw_wgrad_kernel's cap on its workgroups below that, run_colreduce's slabs of 32 pixels below that again, so
    each kernel is taken exactly where the one before it no longer fits (three different amounts of scratch written).  (Where a later kernel asks for more
    than an earlier one -- most shapes of the net -- it cannot be reached through the size at all.)  256 bytes below the lowest threshold: the error."""
    case = dw_wgrad_case(kind, *shape)
    paths, _ = fallbacks(case, 0, case.guard, 3)
    expect_ws_error(case, paths[1][0] - 256)


@pytest.mark.parametrize("kind", ["bnstats", "fwd", "affine", "bwd_weight"])
def test_conv7x7_stem_minimum(kind):
    """myolo_conv7x7s2_c3_*: the planner's figure is an upper bound (the larger of two users of the scratch behind the im2col matrix and the padded
    weights), so the minimum each entry enforces is found by bisection below it: the workspace error under it (one call 256 bytes below, outputs
    untouched, guard intact), the exact result and the same bits from it up.  _bnstats_fwd, the training stem, is the entry that needs scratch behind the
    two matrices."""
    case = conv7_case(kind, 2, 32, 32, 64)
    paths, _ = fallbacks(case, 0, case.guard, 1)
    expect_ws_error(case, paths[1][0] - 256)


def test_conv3x3_bwd_weight_needs_its_partials():
    """launch_tn (AM_CONV3): every size from the need up gives the bits of the exact-need run, one step below it the error"""
    case = conv3_case("bwd_weight", 2, 14, 14, 32, 64)
    paths, _ = fallbacks(case, 0, case.guard, 1)
    assert len(paths) == 2, paths


def test_winograd_f43_weight_gradient_under_bf16x6():
    """wino_tn_all under "bf16x6", 256 -> 256 channels.  The entry asks for its whole planner figure up front (the larger of the x6 partials and the batched
    fp32 TN partials) and hands wino_tn_all exactly that, so through myolo_conv3x3_wino_bwd_weight the "x6 partials do not fit" branch of wino_tn_all cannot
    be taken: one threshold, below it the workspace error, from it up one x6 launch over all planes and the same bits at every size.  The per-run fp32 TN
    GEMMs are reached at the same sizes through the ablation switch tn_no_x6 (less scratch written).  Not exact (the transform constants are not dyadic):
    every call is held to test_gpu_ops.check at TOL."""
    shape = (2, 14, 14, 256, 256)
    case = wino_case(2, *shape, options=(("wino_x6", 1),))
    paths, outs = find_paths(case, 0, 2 * case.guard)
    show(case.name + " (wino_tn_x6_kernel)", paths)
    assert [s == "error" for _, s in paths] == [True, False], paths
    same_bits(case, outs)
    fp32 = wino_case(2, *shape, options=(("wino_x6", 1), ("tn_no_x6", 1)))
    _, words = both_fills(fp32, paths[1][0])
    print("%s (tn_no_x6: batched gemm_tn_fast per run of planes): %d words at %d bytes" % (case.name, words, paths[1][0]))
    assert words < paths[1][1]


# ============================================================================================================================================
# Part 3: the engine on dirty scratch
# ============================================================================================================================================
# Baseline (two runs on zero-filled buffers, this commit's parent): which tensors repeat bit for bit.  Those must repeat bit for bit under poison; the
# others are named here with the reason and held to compare_step's oracle bounds on both runs instead.
STEP_NOT_BITWISE = {}        # {tensor name: reason}; empty: every output and gradient of the step repeated bit for bit in the baseline
STEP_TENSORS = ("yolo_output", "yolo_proposals", "output_rois", "feature_map", "myolo_mask", "target_class_ids", "target_mask", "n_pos")
STEP_SCALARS = ("loss", "yolo_sum_loss", "mask_loss", "loss_xy", "loss_wh", "loss_conf", "loss_class", "recall")


def fill_engine_scratch(net, fill, training):
    """Every scratch buffer the net owns, filled: the compute stream's, the two side streams', every lane workspace that exists, and the prepared-weights
    arena of the run to come -- the step's (Net._wprep) or the inference path's (Net._iprep).  The engine creates its arena inside the first step /
    forward, so it is created here the way the engine does (same class, same capacity): nothing in it is valid yet, and the run must not care what it
    holds.  These are private fields of the engine: the test is about exactly these buffers.  -> [(name, buffer, data_ptr)] for still_in_use."""
    bufs = [("ws_main", net._ws_main), ("yolo_side.ws", net._yolo_side.ws), ("wgrad_side.ws", net._wgrad_side.ws)]
    bufs += [("lane %s ws" % k, st["ws"]) for k, st in net._lanes.items() if "ws" in st]
    if training and net.weight_prep and net._wprep is None:
        net._wprep_cap = net._wprep_arena_bytes()
        net._wprep = X.WeightPrep(net.dev, arena_bytes=net._wprep_cap)
    if not training and net.infer_weight_cache and net._iprep is None:
        net._iprep = X.WeightPrep(net.dev, arena_bytes=min(net._wprep_arena_bytes(), 256 << 20))
    out = [(name, w, w.buf.data_ptr()) for name, w in bufs]
    for name, prep in (("wprep arena", net._wprep), ("iprep arena", net._iprep)):
        if prep is not None:
            out.append((name, prep, prep.arena.data_ptr()))
    for name, owner, _ in out:
        (owner.arena if hasattr(owner, "arena") else owner.buf).fill_(fill)
    torch.cuda.synchronize()
    return out


def still_in_use(net, filled):
    """the buffers that were filled are the ones the run used: none was replaced (Workspace.ensure allocates a new one when it grows, which would drop the
    fill), and the arenas are still the net's"""
    for name, owner, ptr in filled:
        now = (owner.arena if hasattr(owner, "arena") else owner.buf).data_ptr()
        assert now == ptr, "%s was reallocated during the run: the fill was not what the kernels saw" % name
    arenas = [o for _, o, _ in filled if hasattr(o, "arena")]
    assert all(o is net._wprep or o is net._iprep for o in arenas)


def train_step_on(fill, fp32_matmul):
    """test_gpu_step.compare_step, unchanged, on a model whose scratch is filled after the parameters are loaded -> (oracle rows, outputs, gradients)"""
    import test_gpu_step as S
    from myolo.config import ShapesConfig
    cfg, P, batch, ref = S.make_case(ShapesConfig, 128, 0.5, 4)
    got = {}

    class Filled(S.MaskYOLO):
        def load_state_dict(self, sd, strict=True):
            r = super().load_state_dict(sd, strict)
            got["buffers"] = fill_engine_scratch(self.net, fill, True)
            return r

        def train_on_batch(self, b, learning_rate=None):
            out = super().train_on_batch(b, learning_rate=learning_rate)
            got["out"] = {k: np.array(out[k]) for k in STEP_TENSORS + STEP_SCALARS}
            got["model"] = self
            return out
    orig = S.MaskYOLO
    S.MaskYOLO = Filled
    try:
        rows = S.compare_step(cfg, P, batch, ref, fp32_matmul=fp32_matmul)
    finally:
        S.MaskYOLO = orig
    grads = got["model"].net.grads_dict()
    assert len(got["buffers"]) >= 4 and any(name == "wprep arena" for name, _, _ in got["buffers"])
    still_in_use(got["model"].net, got["buffers"])
    return rows, got["out"], grads


def differing(a, b):
    return sorted(k for k in a if not np.array_equal(a[k], b[k], equal_nan=False))


@pytest.mark.parametrize("fp32_matmul", ["bf16x6", "native"])
def test_train_step_on_poisoned_scratch(fp32_matmul):
    """one train_on_batch(learning_rate=0) of the Shapes 128 x 128 / batch 4 case on 0xFF-filled scratch against the same step on zero-filled scratch: every
    output, loss term and gradient bit for bit (all of them repeat bit for bit between two zero-filled runs), and compare_step's oracle bounds on both"""
    rows0, out0, g0 = train_step_on(0x00, fp32_matmul)
    rows1, out1, g1 = train_step_on(0xFF, fp32_matmul)
    assert set(out0) == set(out1) and set(g0) == set(g1)
    diff = differing(out0, out1) + ["grad " + k for k in differing(g0, g1)]
    print("train step (%s): %d outputs and %d gradients compared; not bit-identical under 0xFF scratch: %s" % (fp32_matmul, len(out0), len(g0), diff or "none"))
    unexpected = [k for k in diff if k not in STEP_NOT_BITWISE]
    assert not unexpected, "tensors that repeat bit for bit on zeroed scratch differ on 0xFF scratch: %s" % unexpected
    for rows in (rows0, rows1):
        bad = [r for r in rows if not r[1] <= STEP_TOL]          # compare_step's oracle bounds, as test_gpu_step asserts them
        assert not bad, bad


def predict_on(fill, dtype):
    import test_gpu_step as S
    from myolo.config import ShapesConfig, make_config
    from myolo.model import MaskYOLO
    cfg, P, batch, _ = S.make_case(ShapesConfig, 128, 0.5, 4)
    cfg = make_config(type(cfg), INFERENCE_DTYPE=dtype)
    model = MaskYOLO(mode="inference", config=cfg)
    model.load_state_dict(P)
    filled = fill_engine_scratch(model.net, fill, False)
    assert len(filled) >= 4 and any(name == "iprep arena" for name, _, _ in filled)
    outs = model.keras_model.predict([batch[0]])
    torch.cuda.synchronize()
    still_in_use(model.net, filled)
    return [np.array(o) for o in outs]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_predict_on_poisoned_scratch(dtype):
    """one inference forward of the same case, fp32 and bf16 mask head: the three outputs finite and bit-identical between 0xFF and zero-filled scratch"""
    a, b = predict_on(0x00, dtype), predict_on(0xFF, dtype)
    assert len(a) == len(b) == 3
    for name, u, v in zip(("yolo_output", "detections", "myolo_mask"), a, b):
        assert np.isfinite(u).all() and np.isfinite(v).all(), name
        assert np.array_equal(u, v), "%s (%s inference) differs between zeroed and 0xFF scratch" % (name, dtype)

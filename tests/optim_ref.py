"""The optimiser pass of the training recipe restated in numpy (contract: include/myolo_hip_internal.h), for
tests/test_optim_host.py and tests/test_gpu_optim.py.  The update is float32 operation for float32 operation in the written order; the exact
squared norm is math.fsum over float64 squares (a float32 squared is exact in float64)."""
import math
import struct

import numpy as np

F32 = np.float32
STATS_BYTES = 24


def unpack_stats(raw):
    """24 bytes -> dict(sumsq, norm, scale, skipped, steps)"""
    sumsq, norm, scale, skipped, steps = struct.unpack("<dffii", bytes(raw))
    return dict(sumsq=sumsq, norm=norm, scale=scale, skipped=skipped, steps=steps)


def trainable_elements(flags, n):
    return np.repeat((np.asarray(flags, np.uint8) & 1).astype(bool), 4)[:n]


def decayed_elements(flags, n):
    return np.repeat((np.asarray(flags, np.uint8) & 2).astype(bool), 4)[:n]


def sumsq_exact(g, flags, gs):
    """the correctly rounded sum of (double)x * (double)x over the trainable groups, x = g * gs in float32"""
    with np.errstate(all="ignore"):
        x = (np.asarray(g, F32) * F32(gs))[trainable_elements(flags, len(g))].astype(np.float64)
        sq = x * x
    if not np.isfinite(sq).all():
        return float(sq.sum())                        # NaN or inf: fsum refuses mixed infinities; only finiteness matters then
    return math.fsum(sq.tolist())


def finish(sumsq, clip):
    """-> (norm float32, scale float32, skipped bool) from a float64 sumsq, as the record's rules state"""
    sumsq, clip = float(sumsq), float(F32(clip))
    norm = F32(math.sqrt(sumsq)) if sumsq >= 0 else F32(np.nan)
    if not math.isfinite(sumsq):
        return norm, F32(0.0), True
    if clip == 0.0 or sumsq <= clip * clip:
        return norm, F32(1.0), False
    return norm, F32(clip / math.sqrt(sumsq)), False


def step(p, g, m, v, ema, flags, scale, skipped, lr_t, b1, b2, eps, gs, lr_wd, ema_d, ema_omd):
    """-> (p, m, v, ema) after myolo_adamw_ema_step; ema may be None.  Inputs are not modified."""
    p, g, m, v = (np.array(a, F32) for a in (p, g, m, v))
    ema = None if ema is None else np.array(ema, F32)
    if skipped:
        return p, m, v, ema
    lr_t, b1, b2, eps, gs, lr_wd, ema_d, ema_omd, scale = (F32(x) for x in (lr_t, b1, b2, eps, gs, lr_wd, ema_d, ema_omd, scale))
    n = len(p)
    tr, dec = trainable_elements(flags, n), decayed_elements(flags, n)
    with np.errstate(all="ignore"):
        gi = (g * gs) * scale
        mi = b1 * m + (F32(1.0) - b1) * gi
        vi = b2 * v + ((F32(1.0) - b2) * gi) * gi
        pn = p - (lr_t * mi) / (np.sqrt(vi) + eps)
        pn = np.where(dec, pn - lr_wd * p, pn)
        for a in (gi, mi, vi, pn):
            assert a.dtype == F32
        if ema is not None:
            en = ema_d * ema + ema_omd * pn
            assert en.dtype == F32
            ema = np.where(tr, en, ema)
    return np.where(tr, pn, p), np.where(tr, mi, m), np.where(tr, vi, v), ema


def lr_t_of(lr, t, b1=0.9, b2=0.999):
    """the host scalar of Net.adam_step / Net.recipe_step"""
    return float(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def ema_coefficients(decay, t):
    d = min(float(decay), (1.0 + t) / (10.0 + t))
    return float(F32(d)), float(F32(1.0 - d))

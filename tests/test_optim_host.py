"""Host side of the training recipe (myolo/optim.py), no GPU: the Schedule by hand values, the Recipe's range checks, the
flags byte on a walk of the flat layout for the Shapes and the ResNet-50 configurations, the numpy restatement's own rules, and the refusals of
the three entry points through the C-ABI (argument checks come before any launch)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from myolo.config import make_config, ShapesConfig
from myolo.optim import Recipe, Schedule, check_recipe, group_flags, FLAG_TRAINABLE, FLAG_DECAYED
import optim_ref as R

BASE = 1e-3


# ---------------------------------------------------------------- Schedule
def test_constant_is_base_everywhere():
    s = Schedule()
    assert all(s.lr_at(k, 100, BASE) == BASE for k in (0, 1, 50, 99, 100, 1000))


def test_warmup_endpoints_and_middle():
    s = Schedule("constant", warmup_steps=10, warmup_from=0.1)
    assert s.lr_at(0, 100, BASE) == BASE * 0.1
    assert s.lr_at(10, 100, BASE) == BASE                      # base at the end of the warm-up
    assert s.lr_at(5, 100, BASE) == BASE * (0.1 + 0.9 * 0.5)
    assert s.lr_at(9, 100, BASE) < BASE and s.lr_at(11, 100, BASE) == BASE
    lrs = [s.lr_at(k, 100, BASE) for k in range(11)]
    assert lrs == sorted(lrs)


def test_cosine_endpoints_and_halfway():
    s = Schedule("cosine", final=0.01)
    assert s.lr_at(0, 100, BASE) == BASE
    assert math.isclose(s.lr_at(100, 100, BASE), 0.01 * BASE, rel_tol=1e-12)
    assert math.isclose(s.lr_at(50, 100, BASE), BASE * (0.01 + 0.99 * 0.5), rel_tol=1e-12)
    assert math.isclose(s.lr_at(500, 100, BASE), 0.01 * BASE, rel_tol=1e-12)         # past the end: stays at the floor
    w = Schedule("cosine", warmup_steps=20, warmup_from=0.0, final=0.1)
    assert w.lr_at(0, 120, BASE) == 0.0 and w.lr_at(20, 120, BASE) == BASE
    assert math.isclose(w.lr_at(70, 120, BASE), BASE * (0.1 + 0.9 * 0.5), rel_tol=1e-12)   # halfway between the warm-up's end and total_steps
    assert math.isclose(w.lr_at(120, 120, BASE), 0.1 * BASE, rel_tol=1e-12)


def test_step_at_and_around_milestones():
    s = Schedule("step", milestones=(0.5, 0.7), gamma=0.1)
    assert s.lr_at(49, 100, BASE) == BASE
    assert s.lr_at(50, 100, BASE) == BASE * 0.1
    assert s.lr_at(51, 100, BASE) == BASE * 0.1
    assert s.lr_at(69, 100, BASE) == BASE * 0.1
    assert s.lr_at(70, 100, BASE) == BASE * 0.1 ** 2
    assert s.lr_at(6, 10, BASE) == BASE * 0.1 and s.lr_at(7, 10, BASE) == BASE * 0.1 ** 2     # 0.7 * 10 is not 7.0 in binary64: rounded


def test_schedule_is_pure_and_float64():
    s = Schedule("cosine", warmup_steps=3)
    a = [s.lr_at(k, 37, 0.01) for k in range(40)]
    assert a == [Schedule("cosine", warmup_steps=3).lr_at(k, 37, 0.01) for k in range(40)]
    assert all(type(x) is float for x in a)


@pytest.mark.parametrize("kw", [dict(kind="linear"), dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(warmup_from=1.5), dict(final=-0.1),
                                dict(milestones=(0.7, 0.5)), dict(milestones=(0.0,)), dict(milestones=(1.0,)), dict(gamma=0.0), dict(gamma=2.0)])
def test_schedule_range_checks(kw):
    with pytest.raises(ValueError):
        Schedule(**kw)


# ---------------------------------------------------------------- Recipe
@pytest.mark.parametrize("kw", [dict(clip_norm=0.0), dict(clip_norm=-1.0), dict(clip_norm=float("inf")), dict(clip_norm=float("nan")),
                                dict(weight_decay=-1e-4), dict(weight_decay=float("nan")), dict(ema=0.0), dict(ema=1.0), dict(ema=1.5)])
def test_recipe_range_checks(kw):
    with pytest.raises(ValueError):
        Recipe(**kw)


def test_recipe_type_errors_and_repr():
    with pytest.raises(TypeError):
        Recipe(schedule="cosine")
    for bad in ("adamw", dict(clip_norm=5.0), 5.0, Schedule()):
        with pytest.raises(TypeError):
            check_recipe(bad)
    r = Recipe(clip_norm=5, weight_decay=1e-4, ema=0.999, schedule=Schedule("cosine", warmup_steps=7))
    assert check_recipe(r) is r
    assert repr(r) == ("Recipe(clip_norm=5.0, weight_decay=0.0001, ema=0.999, schedule=Schedule(kind='cosine', warmup_steps=7, warmup_from=0.1, "
                       "final=0.01, milestones=(), gamma=0.1))")
    assert repr(Recipe()) == "Recipe(clip_norm=None, weight_decay=0.0, ema=None, schedule=None)"
    assert Recipe().lr_at(3, 10, 0.5) == 0.5 and r.lr_at(0, 100, 1.0) == 0.1


def test_from_config_takes_the_reference_figures():
    cfg = make_config(ShapesConfig)
    r = Recipe.from_config(cfg)
    assert r.clip_norm == 5.0 == cfg.GRADIENT_CLIP_NORM and r.weight_decay == 0.0001 == cfg.WEIGHT_DECAY and r.ema is None and r.schedule is None
    s = Schedule("step", milestones=(0.5,))
    r = Recipe.from_config(make_config(ShapesConfig, GRADIENT_CLIP_NORM=1.5, WEIGHT_DECAY=0.0), ema=0.99, schedule=s)
    assert (r.clip_norm, r.weight_decay, r.ema, r.schedule) == (1.5, 0.0, 0.99, s)


def test_ema_coefficients_warm_up_then_hold():
    r = Recipe(ema=0.999)
    d1, o1 = r.ema_coefficients(1)
    assert d1 == float(np.float32(2.0 / 11.0)) and o1 == float(np.float32(1.0 - 2.0 / 11.0))
    d, o = r.ema_coefficients(10 ** 6)
    assert d == float(np.float32(0.999)) and o == float(np.float32(1.0 - 0.999))
    assert (d1, o1) == R.ema_coefficients(0.999, 1) and (d, o) == R.ema_coefficients(0.999, 10 ** 6)


# ---------------------------------------------------------------- the flags byte
@pytest.mark.parametrize("kw", [dict(), dict(BACKBONE="resnet50", IMAGE_SHAPE=[128, 128, 3])], ids=["shapes", "resnet50"])
def test_flags_byte_on_a_walk_of_the_layout(kw):
    from myolo.engine import layer_table, param_layout
    cfg = make_config(ShapesConfig, **kw)
    pslots, _, buckets, nparam, _ = param_layout(layer_table(cfg))
    assert nparam % 4 == 0 and buckets[0][0] == 0 and buckets[-1][1] == nparam
    regex = r"(myolo_mask.*)"
    flags = group_flags(pslots, nparam, lambda layer: bool(re.fullmatch(regex, layer)))
    assert flags.dtype == np.uint8 and flags.shape == (nparam // 4,)
    seen = np.zeros(nparam // 4, bool)
    slots = set()
    n_frozen = n_trainable = 0
    for k, (off, shp) in pslots.items():
        layer, slot = k.split("/")
        slots.add(slot)
        assert off % 4 == 0                                     # a group of four never straddles two tensors
        lo, hi = off // 4, off // 4 + (int(np.prod(shp)) + 3) // 4
        assert not seen[lo:hi].any()
        seen[lo:hi] = True
        f = flags[lo:hi]
        if slot in ("gamma", "beta", "bias"):
            assert not (f & FLAG_DECAYED).any(), k
        else:
            assert slot in ("kernel", "depthwise_kernel") and (f & FLAG_DECAYED).all(), k
        if layer.startswith("myolo_mask"):
            assert (f & FLAG_TRAINABLE).all(), k
            n_trainable += 1
        else:
            assert not (f & FLAG_TRAINABLE).any(), k            # frozen layers lack bit 0
            n_frozen += 1
    assert seen.all() and n_frozen > 10 and n_trainable > 5
    assert {"kernel", "gamma", "beta", "bias"} <= slots
    everything = group_flags(pslots, nparam)
    assert (everything & FLAG_TRAINABLE).all() and np.array_equal(everything & FLAG_DECAYED, flags & FLAG_DECAYED)
    with pytest.raises(ValueError):
        group_flags(pslots, nparam + 1)


# ---------------------------------------------------------------- the restatement's own rules
def test_reference_finish_rules():
    assert R.finish(25.0, 5.0) == (np.float32(5.0), np.float32(1.0), False)           # norm == clip: exactly 1
    assert R.finish(1e30, 0.0)[1:] == (np.float32(1.0), False)                        # clip off
    n, s, sk = R.finish(100.0, 5.0)
    assert (n, s, sk) == (np.float32(10.0), np.float32(0.5), False)
    assert R.finish(0.0, 1.0) == (np.float32(0.0), np.float32(1.0), False)
    for bad in (float("inf"), float("nan")):
        n, s, sk = R.finish(bad, 5.0)
        assert s == 0.0 and sk
    g = np.array([3, 4, 0, 0, np.nan, 1, 1, 1], np.float32)
    assert R.sumsq_exact(g, [1, 0], 1.0) == 25.0 and R.sumsq_exact(g, [1, 0], 0.5) == 6.25 and math.isnan(R.sumsq_exact(g, [1, 1], 1.0))


def test_reference_step_by_hand():
    one = np.ones(4, np.float32)
    p, m, v, e = R.step(one, 2 * one, 0 * one, 0 * one, one, [3], 0.5, False, 0.1, 0.9, 0.999, 1e-8, 1.0, 0.01, 0.5, 0.5)
    f = np.float32
    gi = f(1.0)
    mi = (f(1) - f(0.9)) * gi
    vi = ((f(1) - f(0.999)) * gi) * gi
    pn = f(1) - (f(0.1) * mi) / (np.sqrt(vi) + f(1e-8))
    pn = pn - f(0.01) * f(1)
    assert p[0] == pn and m[0] == mi and v[0] == vi and e[0] == f(0.5) * f(1) + f(0.5) * pn
    frozen = R.step(one, 2 * one, 0 * one, 0 * one, one, [2], 0.5, False, 0.1, 0.9, 0.999, 1e-8, 1.0, 0.01, 0.5, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(frozen, (one, 0 * one, 0 * one, one)))
    skipped = R.step(one, 2 * one, 0 * one, 0 * one, None, [3], 0.0, True, 0.1, 0.9, 0.999, 1e-8, 1.0, 0.01, 0.5, 0.5)
    assert np.array_equal(skipped[0], one) and skipped[3] is None


# ---------------------------------------------------------------- refusals through the C-ABI (nothing is launched)
def _lib():
    from myolo import _ext as X
    if not os.path.exists(X.LIB_PATH):
        pytest.skip("library not built")
    return X.load()


def test_entry_points_refuse_bad_arguments_without_gpu():
    lib = _lib()
    F = ctypes.c_float
    A = 0x10000                                                   # an aligned address that is never dereferenced on the host

    def sumsq(g=A, flags=A, n=8, gs=1.0, clip=0.0, stats=A, partials=A):
        return lib.myolo_grad_sumsq(g, flags, n, F(gs), F(clip), stats, partials, None)

    def step(p=A, g=A, m=A, v=A, ema=None, flags=A, n=8, stats=A):
        return lib.myolo_adamw_ema_step(p, g, m, v, ema, flags, n, stats, F(1e-3), F(0.9), F(0.999), F(1e-8), F(1.0), F(0.0), F(0.0), F(0.0), None)

    for bad in (dict(g=None), dict(flags=None), dict(stats=None), dict(partials=None), dict(n=0), dict(n=-4), dict(n=6), dict(n=1021),
                dict(clip=-1.0), dict(clip=float("inf")), dict(clip=float("nan"))):
        assert sumsq(**bad) == -1 and b"grad_sumsq" in lib.myolo_last_error_string(), bad
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(flags=None), dict(stats=None), dict(n=0), dict(n=7), dict(n=1022)):
        assert step(**bad) == -1 and b"adamw_ema_step" in lib.myolo_last_error_string(), bad
    for a, b, n in ((None, A, 8), (A, None, 8), (A, A, 0), (A, A, 5), (A, A, 1023)):
        assert lib.myolo_swap_f32(a, b, n, None) == -1 and b"swap_f32" in lib.myolo_last_error_string(), (a, b, n)

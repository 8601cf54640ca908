"""The training recipe on the device (csrc/optim_kernels.hip, Net.recipe_step, MaskYOLO.train(recipe=...)).

Through ctypes: myolo_grad_sumsq within the bound of any-order double summation of the exact sum and bit-repeatable; given the device's own sumsq
bits, scale / norm / p / m / v / ema equal the numpy restatement (tests/optim_ref.py) bit for bit over three steps, at sizes that are one group,
two groups, either side of a workgroup and one grid sweep of the update plus a group; the edges of the contract; myolo_swap_f32.  Every buffer
the entries write lies between guard words that must keep their bits.
Through the engine and the model (the data-parallel test's small case): a clipped step, frozen layers, ema_weights(), checkpoints, train() with a
Schedule, and two gloo ranks on one GPU."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import np_ops as O                                        # noqa: E402
from myolo import _ext as X                                            # noqa: E402
from myolo import optim as MO                                          # noqa: E402
from myolo.optim import Recipe, Schedule                               # noqa: E402
import optim_ref as R                                                  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
GUARD = 4                                                              # floats in front of and behind every written buffer (16 bytes: alignment kept)
SENTINEL = 0x7FC0DEAD                                                  # a quiet NaN no arithmetic produces
# one full sweep of the update's largest grid, plus one group: the grid-stride loop takes a second turn and the last workgroup is partial; the
# reduction's grid (half as many workgroups) then takes a third
N_SWEEP = MO.UPDATE_BLOCKS * MO.THREADS * 4 + 4
SIZES = [4, 8, 1020, 1024, 1028, N_SWEEP]
B1, B2, EPS = 0.9, 0.999, 1e-8


class Guarded(object):
    """a float32 device buffer of n elements between guard words"""

    def __init__(self, a):
        a = np.ascontiguousarray(a, F32)
        self.n = len(a)
        full = np.full(self.n + 2 * GUARD, 0, np.uint32)
        full[:] = SENTINEL
        full[GUARD:GUARD + self.n] = a.view(np.uint32)
        self.t = torch.from_numpy(full.view(np.int32)).to(DEV)
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def bits(self):
        return self.t.cpu().numpy().view(np.uint32)[GUARD:GUARD + self.n]

    def host(self):
        return self.bits().view(F32)

    def guards_intact(self):
        w = self.t.cpu().numpy().view(np.uint32)
        return bool((w[:GUARD] == SENTINEL).all() and (w[GUARD + self.n:] == SENTINEL).all())


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _assert_bits(got, want, what):
    got, want = _bits(got), _bits(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d words differ, first at %d (%r against %r)" % (
        what, bad.size, got.size, bad[0], got.view(F32)[bad[0]], want.view(F32)[bad[0]])


class Device(object):
    """the optimiser's buffers on the device and the numpy restatement's beside them"""

    def __init__(self, n, flags, rng, ema=True, zero_moments=False):
        self.n, self.flags_h = n, np.asarray(flags, np.uint8)
        assert self.flags_h.shape == (n // 4,)
        self.ref = dict(p=rng.standard_normal(n).astype(F32),
                        m=np.zeros(n, F32) if zero_moments else (0.1 * rng.standard_normal(n)).astype(F32),
                        v=np.zeros(n, F32) if zero_moments else (0.01 * rng.random(n)).astype(F32),
                        ema=rng.standard_normal(n).astype(F32) if ema else None)
        self.dev = {k: (None if a is None else Guarded(a)) for k, a in self.ref.items()}
        self.flags = torch.from_numpy(self.flags_h).to(DEV)
        self.stats = torch.zeros(R.STATS_BYTES, dtype=torch.uint8, device=DEV)
        self.partials = torch.full((MO.SUMSQ_BLOCKS,), float("nan"), dtype=torch.float64, device=DEV)
        self.t = 0

    def read_stats(self):
        return R.unpack_stats(self.stats.cpu().numpy().tobytes())

    def sumsq(self, g, gs=1.0, clip=0.0):
        self.g = Guarded(g)
        X.call("myolo_grad_sumsq", self.g.ptr, X.ptr(self.flags), self.n, gs, clip, X.ptr(self.stats), X.ptr(self.partials), X.stream())
        return self.read_stats()

    def step(self, g, lr=1e-3, gs=1.0, clip=0.0, wd=0.0, ema_decay=0.99):
        """one recipe step on the device and in numpy from the device's own sumsq bits -> the device's stats"""
        self.t += 1
        st = self.sumsq(g, gs, clip)
        lr_t = R.lr_t_of(lr, self.t, B1, B2)
        lr_wd = float(F32(lr * wd))
        ema_d, ema_omd = R.ema_coefficients(ema_decay, self.t)
        d = self.dev
        X.call("myolo_adamw_ema_step", d["p"].ptr, self.g.ptr, d["m"].ptr, d["v"].ptr, None if d["ema"] is None else d["ema"].ptr,
               X.ptr(self.flags), self.n, X.ptr(self.stats), lr_t, B1, B2, EPS, gs, lr_wd, ema_d, ema_omd, X.stream())
        norm, scale, skipped = R.finish(st["sumsq"], clip)
        _assert_bits([st["scale"]], [scale], "scale")
        if not (np.isnan(norm) and np.isnan(st["norm"])):                  # (a NaN's sign and payload are not part of the contract)
            _assert_bits([st["norm"]], [norm], "norm")
        r = self.ref
        r["p"], r["m"], r["v"], r["ema"] = R.step(r["p"], g, r["m"], r["v"], r["ema"], self.flags_h, scale, skipped, lr_t, B1, B2, EPS, gs,
                                                  lr_wd, ema_d, ema_omd)
        self.check("step %d" % self.t)
        _assert_bits(self.g.host(), g, "g is read only")
        assert np.array_equal(self.flags.cpu().numpy(), self.flags_h)
        after = self.read_stats()
        assert after == st or (np.isnan(st["sumsq"]) and after["steps"] == st["steps"]), "the update wrote the record"
        return st

    def check(self, what):
        for k, buf in self.dev.items():
            if buf is not None:
                _assert_bits(buf.host(), self.ref[k], "%s: %s" % (what, k))
                assert buf.guards_intact(), "%s: %s written outside [0, n)" % (what, k)
        assert self.g.guards_intact()


def _mixed_flags(n):
    """all four combinations, adjacent, starting with trainable + decayed"""
    return np.resize(np.array([3, 1, 2, 0], np.uint8), n // 4)


# ---------------------------------------------------------------- entries through ctypes
@pytest.mark.parametrize("n", SIZES)
def test_sumsq_within_the_double_summation_bound_and_repeatable(n):
    rng = np.random.default_rng(n)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 2, n))).astype(F32)
    flags = (rng.random(n // 4) < 0.7).astype(np.uint8) | 2
    flags[0] |= 1
    d = Device(n, flags, rng)
    a = d.sumsq(g, 1.0, 1.0)
    raw_a = d.stats.cpu().numpy().tobytes()[:8]
    exact = R.sumsq_exact(g, flags, 1.0)
    # any-order summation of n non-negative doubles: relative error <= (n - 1) u + O(u^2), u = 2^-53 (the squares themselves are exact)
    assert abs(a["sumsq"] - exact) <= n * 2.0 ** -53 * exact, (a["sumsq"], exact)
    d.partials.fill_(float("nan"))
    b = d.sumsq(g, 1.0, 1.0)
    assert d.stats.cpu().numpy().tobytes()[:8] == raw_a                    # the same 8 bytes
    assert (a["steps"], b["steps"], b["skipped"]) == (1, 2, 0)
    assert d.g.guards_intact()
    _assert_bits([a["norm"]], [F32(np.sqrt(a["sumsq"]))], "norm")


@pytest.mark.parametrize("n", SIZES)
def test_three_steps_equal_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    d = Device(n, _mixed_flags(n), rng)
    frozen = ~R.trainable_elements(d.flags_h, n)
    before = {k: v.copy() for k, v in d.ref.items()}
    for _ in range(3):
        g = rng.standard_normal(n).astype(F32)
        clip = 0.5 * float(np.sqrt(R.sumsq_exact(g, d.flags_h, 1.0)))      # clipping is active
        st = d.step(g, clip=clip, wd=0.05, ema_decay=0.9)
        assert 0.0 < st["scale"] < 1.0 and st["skipped"] == 0
    for k in before:                                                       # the sentinel side of the mixed flags: frozen groups keep their bits
        _assert_bits(d.dev[k].host()[frozen], before[k][frozen], "frozen " + k)
        assert n < 16 or frozen.any()
        assert not np.array_equal(_bits(d.dev[k].host()[~frozen]), _bits(before[k][~frozen]))
    assert d.read_stats()["steps"] == 3


N_EDGE = 1028


def test_clip_off_and_norm_at_and_just_above_the_clip():
    rng = np.random.default_rng(1)
    flags = np.full(N_EDGE // 4, 3, np.uint8)
    g = np.zeros(N_EDGE, F32)
    g[5], g[1027] = 3.0, 4.0                                               # sumsq = 25 exactly, in any order
    d = Device(N_EDGE, flags, rng)
    st = d.step(1e4 * g, clip=0.0)                                         # clip off: scale exactly 1 whatever the norm
    assert st["sumsq"] == 25e8 and st["scale"] == 1.0 and st["norm"] == 5e4
    st = d.step(g, clip=5.0)                                               # norm == clip: exactly 1
    assert st["sumsq"] == 25.0 and st["scale"] == 1.0 and st["norm"] == 5.0
    below = float(np.nextafter(F32(5.0), F32(0.0)))
    st = d.step(g, clip=below)                                             # norm just above the clip
    assert st["scale"] == float(F32(below / 5.0)) < 1.0 and st["skipped"] == 0


def test_all_zero_gradient():
    rng = np.random.default_rng(2)
    d = Device(N_EDGE, _mixed_flags(N_EDGE), rng, zero_moments=True)
    st = d.step(np.zeros(N_EDGE, F32), clip=1.0, wd=0.1)
    assert st["sumsq"] == 0.0 and st["norm"] == 0.0 and st["scale"] == 1.0 and st["skipped"] == 0
    for k, buf in d.dev.items():
        assert np.isfinite(buf.host()).all(), k                            # 0 / (sqrt(0) + eps): no NaN anywhere


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_gradient_skips_the_step_and_the_next_proceeds(bad):
    rng = np.random.default_rng(3)
    d = Device(N_EDGE, _mixed_flags(N_EDGE), rng)
    before = {k: v.copy() for k, v in d.ref.items()}
    g = rng.standard_normal(N_EDGE).astype(F32)
    g[16] = bad                                                            # group 4: trainable + decayed
    st = d.step(g, clip=1.0, wd=0.1)
    assert st["scale"] == 0.0 and st["skipped"] == 1 and st["steps"] == 1 and not np.isfinite(st["sumsq"])
    for k in before:
        _assert_bits(d.dev[k].host(), before[k], "skipped step: " + k)     # nothing but stats changed
    st = d.step(rng.standard_normal(N_EDGE).astype(F32), clip=1.0, wd=0.1)
    assert 0.0 < st["scale"] < 1.0 and st["skipped"] == 1 and st["steps"] == 2
    assert not np.array_equal(_bits(d.dev["p"].host()), _bits(before["p"]))


def test_non_finite_value_in_a_frozen_group_does_not_skip():
    rng = np.random.default_rng(4)
    flags = _mixed_flags(N_EDGE)
    d = Device(N_EDGE, flags, rng)
    g = rng.standard_normal(N_EDGE).astype(F32)
    assert flags[2] == 2 and flags[3] == 0
    g[8], g[9], g[13] = np.nan, np.inf, -np.inf                            # groups 2 and 3: frozen
    st = d.step(g, clip=1.0, wd=0.1)
    assert np.isfinite(st["sumsq"]) and st["skipped"] == 0 and 0.0 < st["scale"] < 1.0
    assert all(np.isfinite(buf.host()).all() for buf in d.dev.values())


def test_without_ema_and_with_a_gradient_scale():
    rng = np.random.default_rng(5)
    d = Device(N_EDGE, _mixed_flags(N_EDGE), rng, ema=False)
    for _ in range(2):
        g = rng.standard_normal(N_EDGE).astype(F32)
        st = d.step(g, gs=0.5, clip=3.0, wd=0.01)
        exact = R.sumsq_exact(g, d.flags_h, 0.5)
        assert abs(st["sumsq"] - exact) <= N_EDGE * 2.0 ** -53 * exact and 0.0 < st["scale"] < 1.0
    d2 = Device(N_EDGE, _mixed_flags(N_EDGE), rng, ema=True)
    d2.step(rng.standard_normal(N_EDGE).astype(F32), gs=0.5, clip=3.0, wd=0.01)


def test_everything_off_agrees_with_the_adam_oracle():
    """no clip, decay 0, no EMA, every group trainable: the plain Adam step, held to what test_gpu_ops.py::test_adam_three_steps holds
    myolo_adam_step to"""
    rng = np.random.default_rng(12)
    n = 10008
    d = Device(n, np.full(n // 4, 1, np.uint8), rng, ema=False, zero_moments=True)
    rp, rm, rv = d.ref["p"].copy(), np.zeros(n, F32), np.zeros(n, F32)
    for t in range(1, 4):
        g = rng.standard_normal(n).astype(F32)
        d.step(g, clip=0.0, wd=0.0)
        rp, rm, rv = O.adam_step(rp, g, rm, rv, t)
    got = d.dev["p"].host().astype(np.float64)
    assert np.isfinite(got).all()
    assert np.abs(got - rp).max() / max(1.0, np.abs(rp).max()) <= 1e-6


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bits(n):
    rng = np.random.default_rng(200 + n)
    a, b = rng.integers(0, 2 ** 32, n, dtype=np.uint32), rng.integers(0, 2 ** 32, n, dtype=np.uint32)      # any bit pattern, NaNs included
    A, B = Guarded(a.view(F32)), Guarded(b.view(F32))
    X.call("myolo_swap_f32", A.ptr, B.ptr, n, X.stream())
    assert np.array_equal(A.bits(), b) and np.array_equal(B.bits(), a) and A.guards_intact() and B.guards_intact()
    X.call("myolo_swap_f32", A.ptr, B.ptr, n, X.stream())
    assert np.array_equal(A.bits(), a) and np.array_equal(B.bits(), b)


def test_refusals_on_the_device():
    t = torch.zeros(64, device=DEV)
    for n in (0, 6, 1021):
        with pytest.raises(RuntimeError, match="n % 4"):
            X.call("myolo_swap_f32", X.ptr(t), X.ptr(t), n, X.stream())
    with pytest.raises(RuntimeError, match="clip"):
        X.call("myolo_grad_sumsq", X.ptr(t), X.ptr(t), 8, 1.0, -1.0, X.ptr(t), X.ptr(t), X.stream())
    with pytest.raises(RuntimeError, match="null"):
        X.call("myolo_adamw_ema_step", X.ptr(t), None, X.ptr(t), X.ptr(t), None, X.ptr(t), 8, X.ptr(t), 1e-3, B1, B2, EPS, 1.0, 0.0, 0.0, 0.0,
               X.stream())
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0


# ---------------------------------------------------------------- engine and model
def _case():
    from myolo.config import make_config, ShapesConfig
    from myolo.shapes import make_shapes_samples
    from myolo.myolo_utils import BatchGenerator
    from myolo.engine import init_state_dict
    cfg = make_config(ShapesConfig, IMAGE_SHAPE=[128, 128, 3], ALPHA=0.5, BATCH_SIZE=4)
    P = init_state_dict(cfg, seed=5)
    batches, images = [], []
    for r in range(2):
        samples = make_shapes_samples(4, cfg, start_index=40 + 4 * r)
        images += [s[0] for s in samples]
        batches.append(BatchGenerator(samples, cfg, 'training', shuffle=False, norm=True)[0][0])
    return cfg, P, batches, images


@pytest.fixture(scope="module")
def case():
    return _case()


def _model(case, mode="training"):
    from myolo.model import MaskYOLO
    cfg, P, _, _ = case
    model = MaskYOLO(mode=mode, config=cfg, device=DEV)
    model.load_state_dict(P)
    model.set_trainable(".*")
    model.compile(1e-3, 0.9)
    return model


def test_clipped_step_moves_the_weights_no_further_than_the_clip_allows(case):
    """Adam's first step from zero moments is lr * sqrt(1-b2) * g / (sqrt(1-b2) |g| + eps) per element, so |dp| <= lr * sqrt(1-b2) * |g| / eps and
    ||dp||_2 <= lr * sqrt(1-b2) / eps * ||g||_2 <= lr * sqrt(1-b2) / eps * clip once the gradient is clipped; 1e-4 relative covers the float32
    roundings of the update, 2^-23 ||p|| the rounding of p - x to float32.  The unclipped step is about lr in every element."""
    model = _model(case)
    lr, clip = 1e-3, 1e-7
    with pytest.raises(TypeError, match="myolo.optim.Recipe"):
        model.train_on_batch(case[2][0], recipe=dict(clip_norm=clip))
    before = model.net.flat_p.double().clone()
    out = model.train_on_batch(case[2][0], lr, recipe=Recipe(clip_norm=clip))
    assert np.isfinite(out["loss"])
    st = model.optimizer_stats()
    assert st["steps"] == 1 and st["skipped"] == 0 and 0.0 < st["scale"] < 1.0 and st["norm"] > clip
    assert abs(st["scale"] - clip / np.sqrt(st["sumsq"])) <= 1e-6 * st["scale"]
    moved = float((model.net.flat_p.double() - before).norm())
    bound = lr * np.sqrt(1.0 - B2) / EPS * clip * (1.0 + 1e-4) + 2.0 ** -23 * float(before.norm())
    free = _model(case)
    free_before = free.net.flat_p.double().clone()
    free.train_on_batch(case[2][0], lr, recipe=Recipe())
    free_moved = float((free.net.flat_p.double() - free_before).norm())
    print("clipped step ||dp|| = %.4e (bound %.4e), unclipped %.4e, norm %.4e scale %.4e" % (moved, bound, free_moved, st["norm"], st["scale"]))
    assert 0.0 < moved <= bound
    assert free.optimizer_stats()["scale"] == 1.0 and free_moved > 10.0 * bound


def test_frozen_layers_and_their_average_keep_their_bits(case):
    model = _model(case)
    net = model.net
    model.set_trainable(r"myolo_mask.*")
    recipe = Recipe(clip_norm=5.0, weight_decay=1e-2, ema=0.9)
    p0 = net.flat_p.clone()
    model.train_on_batch(case[2][0], 1e-3, recipe=recipe)
    torch.cuda.synchronize()
    fz = torch.from_numpy(np.repeat((model._recipe_flags().cpu().numpy() & 1) == 0, 4)).to(DEV)
    kernels = torch.from_numpy(np.repeat((model._recipe_flags().cpu().numpy() & 3) == 3, 4)).to(DEV)
    assert bool(fz.any()) and bool(kernels.any())
    assert torch.equal(net.flat_p[fz].view(torch.int32), p0[fz].view(torch.int32))
    assert torch.equal(net.flat_ema[fz].view(torch.int32), p0[fz].view(torch.int32))
    assert float(net.flat_m[fz].abs().max()) == 0.0 and float(net.flat_v[fz].abs().max()) == 0.0
    assert bool((net.flat_p[kernels] != p0[kernels]).any())                # the decay alone moves the trainable kernels
    # the step does not touch flat_g: the frozen layers' gradients are still there (the plain path zeroes them), and a second step leaves every bit
    assert float(net.flat_g[fz].abs().max()) > 0.0
    g = net.flat_g.clone()
    net.recipe_step(1e-3, recipe, model._recipe_flags())
    torch.cuda.synchronize()
    assert torch.equal(net.flat_g.view(torch.int32), g.view(torch.int32))
    assert torch.equal(net.flat_p[fz].view(torch.int32), p0[fz].view(torch.int32))


def test_ema_weights_context(case):
    model = _model(case, mode="inference")
    net = model.net
    images = case[3][:4]

    def scores():
        return np.concatenate([r["confidence_scores"] for r in model.detect_many(images, cs_threshold=0.0)])

    live0 = scores()
    with model.ema_weights():                                              # before any step the average is a copy of the weights
        assert np.array_equal(scores(), live0)
    assert len(live0) > 0
    recipe = Recipe(clip_norm=5.0, weight_decay=1e-4, ema=0.9)
    for k in range(3):
        model.train_on_batch(case[2][k % 2], 1e-2, recipe=recipe)
    torch.cuda.synchronize()
    live, shadow = net.flat_p.clone(), net.flat_ema.clone()
    assert not torch.equal(live, shadow)
    first = next(iter(net.p))
    ptrs = (net.flat_p.data_ptr(), net.flat_ema.data_ptr(), net.p[first].data_ptr())
    outside = scores()
    with model.ema_weights():
        sd = model.state_dict()
        for k, (off, shp) in net.pslots.items():
            assert np.array_equal(sd[k].view(np.uint32).ravel(), shadow[off:off + int(np.prod(shp))].cpu().numpy().view(np.uint32)), k
        assert torch.equal(net.flat_ema.view(torch.int32), live.view(torch.int32))
        inside = scores()
    assert torch.equal(net.flat_p.view(torch.int32), live.view(torch.int32)) and torch.equal(net.flat_ema.view(torch.int32), shadow.view(torch.int32))
    assert ptrs == (net.flat_p.data_ptr(), net.flat_ema.data_ptr(), net.p[first].data_ptr())                  # nothing was rebound
    assert inside.shape != outside.shape or not np.array_equal(inside, outside)
    assert np.array_equal(scores(), outside)


def _injected_steps(model, recipe, first, last, total):
    """optimiser steps first .. last-1 of a run of `total` on seeded gradients written into flat_g"""
    net = model.net
    real = np.zeros(net.nparam, bool)                  # the words between tensors (16-byte padding) belong to no tensor: their gradient is always 0
    for off, shp in net.pslots.values():
        real[off:off + int(np.prod(shp))] = True
    for k in range(first, last):
        g = torch.from_numpy(np.where(real, np.random.default_rng(1000 + k).standard_normal(net.nparam), 0.0).astype(F32))
        net.flat_g.copy_(g)
        net.recipe_step(recipe.lr_at(k, total, 1e-3), recipe, model._recipe_flags())
        model.global_step = k + 1


def test_checkpoint_resumes_the_optimiser_bit_for_bit(case, tmp_path):
    from myolo.model import MaskYOLO
    recipe = Recipe(clip_norm=5.0, weight_decay=1e-2, ema=0.95, schedule=Schedule("cosine", warmup_steps=2))
    K = 6
    whole = _model(case)
    _injected_steps(whole, recipe, 0, K, K)
    first = _model(case)
    _injected_steps(first, recipe, 0, K // 2, K)
    first.epoch = 1
    path = str(tmp_path / "run.npz")
    first.save_checkpoint(path)
    second = MaskYOLO(mode="training", config=case[0], device=DEV, seed=9)          # a fresh model with other weights
    with pytest.raises(ValueError, match="load_checkpoint"):
        second.train(None, None, 1e-3, 2, "all", recipe=recipe, initial_epoch=1)
    second.load_checkpoint(path)
    assert (second.net.adam_t, second.global_step, second.epoch) == (K // 2, K // 2, 1)
    _injected_steps(second, recipe, K // 2, K, K)
    torch.cuda.synchronize()
    for name in ("flat_p", "flat_m", "flat_v", "flat_ema", "flat_s"):
        a, b = getattr(whole.net, name), getattr(second.net, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert whole.net.adam_t == second.net.adam_t == K
    assert whole.optimizer_stats()["skipped"] == 0 and whole.optimizer_stats()["scale"] < 1.0


def test_train_with_a_schedule_and_without_a_recipe(case):
    from myolo.model import MaskYOLO
    from myolo.shapes import ShapesDataset
    cfg = case[0]
    ds = ShapesDataset(1234)
    ds.load_shapes(8, 128, 128)
    ds.prepare()

    def run(**kw):
        model = MaskYOLO(mode="training", config=cfg, seed=3)
        lrs, step = [], model.train_on_batch

        def spy(db, *a, **k):
            lrs.append(a[0] if a else None)
            return step(db, *a, **k)
        model.train_on_batch = spy
        logs = []
        hist = model.train(ds, None, learning_rate=1e-3, epochs=2, layers="all", max_samples=8, verbose=0,
                           custom_callbacks=[lambda ep, lg: logs.append(lg)], **kw)
        return model, hist, lrs, logs

    plain = [run(), run()]                                                 # the untouched path: the same call twice within this run
    for model, hist, lrs, logs in plain:
        assert sorted(model.history) == ["loss", "val_loss"] and lrs == [None] * 4 and all(sorted(lg) == ["loss"] for lg in logs)
        assert model.net.flat_ema is None and model.optimizer_stats()["steps"] == 0
    assert plain[0][1] == plain[1][1] and plain[0][0].history["loss"] == plain[1][0].history["loss"]
    assert np.array_equal(plain[0][0].history["val_loss"], plain[1][0].history["val_loss"], equal_nan=True)

    sched = Schedule("cosine", warmup_steps=2, warmup_from=0.1, final=0.01)
    recipe = Recipe(clip_norm=5.0, weight_decay=1e-4, ema=0.9, schedule=sched)
    model, hist, lrs, logs = run(recipe=recipe)
    assert lrs == [sched.lr_at(k, 4, 1e-3) for k in range(4)]
    assert [lg["lr"] for lg in logs] == [sched.lr_at(1, 4, 1e-3), sched.lr_at(3, 4, 1e-3)] == model.history["lr"]
    assert sorted(model.history) == ["grad_norm", "loss", "lr", "skipped_steps", "val_loss"]
    assert all(np.isfinite(lg["grad_norm"]) and lg["grad_norm"] > 0 and lg["skipped_steps"] == 0 for lg in logs)
    st = model.optimizer_stats()
    assert st["steps"] == 4 and model.global_step == 4 and model.net.adam_t == 4 and logs[-1]["grad_norm"] == st["norm"]
    assert len(hist) == 2 and np.all(np.isfinite(hist)) and model.net.flat_ema is not None
    with pytest.raises(TypeError, match="myolo.optim.Recipe"):
        model.train(ds, None, learning_rate=1e-3, epochs=1, layers="all", recipe="adamw", verbose=0)
    with pytest.raises(ValueError, match="load_checkpoint"):
        model.train(ds, None, learning_rate=1e-3, epochs=2, layers="all", recipe=recipe, initial_epoch=1, verbose=0)


# ---------------------------------------------------------------- two ranks
def _rank(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from myolo.model import MaskYOLO
        from myolo.dist import GradReducer
        cfg, P, batches, _ = _case()
        model = MaskYOLO(mode="training", config=cfg, device=DEV)
        model.load_state_dict(P)
        model._reducer = GradReducer(model.net.flat_g, model.net.bucket_ranges).attach(model.net)
        model.set_trainable(".*")
        model.compile(1e-3, 0.9)
        recipe = Recipe(clip_norm=0.5, weight_decay=1e-4, ema=0.9)
        sumsq, scales = [], []
        for k in range(2):
            model.train_on_batch(batches[(rank + k) % 2], 1e-3, recipe=recipe)
            st = model.optimizer_stats()
            sumsq.append(np.float64(st["sumsq"]).tobytes().hex())
            scales.append(st["scale"])
        torch.cuda.synchronize()
        same = {}
        for name in ("flat_p", "flat_ema"):
            mine = getattr(model.net, name).cpu()
            gathered = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(gathered, mine)
            same[name] = all(torch.equal(gathered[0].view(torch.int32), t.view(torch.int32)) for t in gathered)
        q.put((rank, sumsq, scales, same, float(model.net.grad_scale), bool(torch.equal(model.net.flat_p, model.net.flat_ema))))
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_identical_weights_average_and_norm():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (r0, sumsq0, scales0, same0, gs0, eq0), (r1, sumsq1, scales1, same1, gs1, eq1) = res
    assert (r0, r1) == (0, 1) and gs0 == gs1 == 0.5
    assert sumsq0 == sumsq1 and len(sumsq0) == 2                          # the same 8 bytes on both ranks, step after step
    assert scales0 == scales1 and all(0.0 < s < 1.0 for s in scales0)       # clipping was active
    assert same0 == same1 == {"flat_p": True, "flat_ema": True}
    assert not eq0 and not eq1                                              # the average is not the weights

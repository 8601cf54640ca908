"""The training recipe: what MaskYOLO.train(recipe=...) and train_on_batch(recipe=...) take.

Recipe     global-norm gradient clipping, decoupled (AdamW) weight decay on the convolution kernels, an exponential moving average of the
           weights, a learning-rate Schedule.  The arithmetic runs on the device in one optimiser pass (Net.recipe_step: myolo_grad_sumsq +
           myolo_adamw_ema_step, csrc/optim_kernels.hip); this module holds the host side only -- ranges, the schedule, the per-step scalars
           and the flags byte -- and needs no GPU.
Schedule   the learning rate as a pure float64 function of (step, total_steps, base_lr): the same on every rank."""
import math

import numpy as np

FLAG_TRAINABLE, FLAG_DECAYED = 1, 2
DECAYED_SLOTS = ("kernel", "depthwise_kernel")      # never gamma, beta or bias
# launch shapes of csrc/optim_kernels.hip (the tests size their largest case by them): threads per workgroup, the update's and the
# reduction's largest grids
THREADS, UPDATE_BLOCKS, SUMSQ_BLOCKS = 256, 2048, 1024


class Schedule(object):
    """Learning rate per optimiser step.

    kind          "constant", "cosine" (base -> final*base at total_steps, half a cosine) or "step" (times gamma at every milestone)
    warmup_steps  the first steps rise linearly from warmup_from*base (step 0) to base (step warmup_steps)
    warmup_from   fraction of base the warm-up starts at, in [0, 1]
    final         cosine: fraction of base reached at total_steps, in [0, 1]
    milestones    step: fractions of total_steps in (0, 1), ascending; milestone m takes effect at step round(m*total_steps)
    gamma         step: factor per milestone, in (0, 1]"""

    KINDS = ("constant", "cosine", "step")

    def __init__(self, kind="constant", warmup_steps=0, warmup_from=0.1, final=0.01, milestones=(), gamma=0.1):
        if kind not in self.KINDS:
            raise ValueError("kind must be one of %r, got %r" % (self.KINDS, kind))
        self.kind = kind
        if isinstance(warmup_steps, bool) or int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError("warmup_steps is a step count >= 0, got %r" % (warmup_steps,))
        self.warmup_steps = int(warmup_steps)
        self.warmup_from = _fraction("warmup_from", warmup_from)
        self.final = _fraction("final", final)
        ms = tuple(float(m) for m in milestones)
        if any(not 0.0 < m < 1.0 for m in ms) or list(ms) != sorted(set(ms)):
            raise ValueError("milestones are ascending fractions of total_steps in (0, 1), got %r" % (milestones,))
        self.milestones = ms
        gamma = float(gamma)
        if not 0.0 < gamma <= 1.0:
            raise ValueError("gamma is a factor in (0, 1], got %r" % (gamma,))
        self.gamma = gamma

    def lr_at(self, step, total_steps, base_lr):
        """float64 learning rate of optimiser step `step` (0-based) of a run of total_steps"""
        step, total, base = int(step), int(total_steps), float(base_lr)
        if step < 0 or total < 1:
            raise ValueError("need step >= 0 and total_steps >= 1, got %r, %r" % (step, total_steps))
        if step < self.warmup_steps:
            return base * (self.warmup_from + (1.0 - self.warmup_from) * (step / float(self.warmup_steps)))
        if self.kind == "cosine":
            span = max(total - self.warmup_steps, 1)
            x = min(max((step - self.warmup_steps) / float(span), 0.0), 1.0)
            return base * (self.final + (1.0 - self.final) * (0.5 * (1.0 + math.cos(math.pi * x))))
        if self.kind == "step":
            passed = sum(1 for m in self.milestones if step >= int(round(m * total)))
            return base * self.gamma ** passed
        return base

    def __repr__(self):
        return ("Schedule(kind=%r, warmup_steps=%r, warmup_from=%r, final=%r, milestones=%r, gamma=%r)" %
                (self.kind, self.warmup_steps, self.warmup_from, self.final, self.milestones, self.gamma))


def _fraction(name, x):
    x = float(x)
    if not 0.0 <= x <= 1.0:
        raise ValueError("%s is a fraction in [0, 1], got %r" % (name, x))
    return x


class Recipe(object):
    """What MaskYOLO.train(recipe=...) and train_on_batch(recipe=...) take.

    clip_norm     the gradient of all trainable weights together is scaled down to this Euclidean norm when it is longer (> 0); None = off.
                  A step whose norm is NaN or infinite is skipped on the device (weights, moments and the average keep their bits)
    weight_decay  decoupled decay (AdamW): p -= lr * weight_decay * p beside the Adam update, on convolution kernels only (>= 0)
    ema           decay in (0, 1) of the averaged copy of the weights (MaskYOLO.ema_weights()); None = none is kept.  The decay of step t is
                  min(ema, (1 + t) / (10 + t)), t the optimiser's step count: the average follows quickly at first
    schedule      a Schedule; None = the constant learning rate train() was given"""

    def __init__(self, clip_norm=None, weight_decay=0.0, ema=None, schedule=None):
        if clip_norm is not None:
            clip_norm = float(clip_norm)
            if not (clip_norm > 0.0 and math.isfinite(clip_norm)):
                raise ValueError("clip_norm is a finite norm > 0 (or None), got %r" % (clip_norm,))
        self.clip_norm = clip_norm
        weight_decay = float(weight_decay)
        if not (weight_decay >= 0.0 and math.isfinite(weight_decay)):
            raise ValueError("weight_decay is finite and >= 0, got %r" % (weight_decay,))
        self.weight_decay = weight_decay
        if ema is not None:
            ema = float(ema)
            if not 0.0 < ema < 1.0:
                raise ValueError("ema is a decay in (0, 1) (or None), got %r" % (ema,))
        self.ema = ema
        if schedule is not None and not isinstance(schedule, Schedule):
            raise TypeError("schedule must be a myolo.optim.Schedule, got %r" % type(schedule).__name__)
        self.schedule = schedule

    @classmethod
    def from_config(cls, cfg, ema=None, schedule=None):
        """the reference's own figures: GRADIENT_CLIP_NORM and WEIGHT_DECAY of the config (its compile() leaves both unused)"""
        return cls(clip_norm=cfg.GRADIENT_CLIP_NORM, weight_decay=cfg.WEIGHT_DECAY, ema=ema, schedule=schedule)

    def lr_at(self, step, total_steps, base_lr):
        return float(base_lr) if self.schedule is None else self.schedule.lr_at(step, total_steps, base_lr)

    def ema_coefficients(self, t):
        """-> (ema_d, ema_omd) of optimiser step t (1-based, Net.adam_t after its increment), each rounded once to float32 from float64"""
        d = min(self.ema, (1.0 + t) / (10.0 + t))
        return float(np.float32(d)), float(np.float32(1.0 - d))

    def __repr__(self):
        return "Recipe(clip_norm=%r, weight_decay=%r, ema=%r, schedule=%r)" % (self.clip_norm, self.weight_decay, self.ema, self.schedule)


def check_recipe(recipe):
    if not isinstance(recipe, Recipe):
        raise TypeError("recipe must be a myolo.optim.Recipe, got %r" % type(recipe).__name__)
    return recipe


def group_flags(pslots, nparam, is_trainable=None):
    """-> uint8 [nparam/4]: one byte per group of four consecutive parameters of the flat buffer (every tensor is padded to 16 bytes, so a group
    never straddles two tensors): bit 0 = trainable (is_trainable(layer name); None = all), bit 1 = decayed (kernel and depthwise_kernel slots)."""
    if nparam % 4:
        raise ValueError("nparam must be a multiple of 4")
    flags = np.zeros(nparam // 4, np.uint8)
    for k, (off, shp) in pslots.items():
        layer, slot = k.split("/")
        n = (int(np.prod(shp)) + 3) // 4
        f = FLAG_TRAINABLE if (is_trainable is None or is_trainable(layer)) else 0
        if slot in DECAYED_SLOTS:
            f |= FLAG_DECAYED
        flags[off // 4:off // 4 + n] = f
    return flags

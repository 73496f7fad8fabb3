"""The update step's policy, host only: the names sqdet_optimizer_options_t takes by index, the learning-rate
schedules and the record a checkpoint keeps of both.  No torch, no device: ops.py, drivers.py and the trainers import it.

    lr_at(step, policy, mc)     the learning rate of the update that follows `step` applied updates (trainer.global_step)
    optim_policy(a, mc)         (the policy of a command line, the policy of one without any of the flags)
    trainer_options(policy)     what ops.Optimizer takes
"""
import math

RULES = ("momentum", "nesterov", "adamw")                 # sqdet_optimizer_options_t.rule by index
CLIP_MODES = ("per_variable", "global")                   # sqdet_optimizer_options_t.clip by index
SCHEDULES = ("staircase", "constant", "cosine", "linear")
# ops.Optimizer's defaults: the reference's rule (TF's MomentumOptimizer with tf.clip_by_norm per variable), Adam's usual constants
OPTIONS = dict(rule="momentum", clip="per_variable", momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.0, ema_warmup=False)
WARMUP_FACTOR = 0.001


def lr_at(step, policy, mc):
    """base = policy lr or mc.LEARNING_RATE; min_lr = base * min_lr_ratio; progress = clip((step - W) / max(1, T - W), 0, 1).
    staircase: base * LR_DECAY_FACTOR ** (step // DECAY_STEPS) (the reference's, train.py:97-102); constant: base;
    cosine: min_lr + 0.5 * (base - min_lr) * (1 + cos(pi * progress)); linear: base + (min_lr - base) * progress.
    For step < W every schedule is multiplied by f + (1 - f) * step / W.  A Python float (float64)."""
    step = int(step)
    base = policy.get("lr") or mc.LEARNING_RATE
    sched, W = policy["lr_schedule"], int(policy["warmup_steps"])
    if sched == "staircase":
        lr = base * mc.LR_DECAY_FACTOR ** (step // mc.DECAY_STEPS)
    elif sched == "constant":
        lr = base
    else:
        T = int(policy["lr_total_steps"])
        min_lr = base * float(policy["min_lr_ratio"])
        progress = min(max((step - W) / max(1, T - W), 0.0), 1.0)
        if sched == "cosine":
            lr = min_lr + 0.5 * (base - min_lr) * (1.0 + math.cos(math.pi * progress))
        elif sched == "linear":
            lr = base + (min_lr - base) * progress
        else:
            raise ValueError("lr_schedule %r is not one of %s" % (sched, ", ".join(SCHEDULES)))
    if step < W:
        f = float(policy["warmup_factor"])
        lr = lr * (f + (1.0 - f) * step / W)
    return lr


def optim_policy(a, mc):
    """(the policy of --optimizer ... --ema_warmup as a checkpoint records it, the policy of a run without any of the flags -- what a
    checkpoint without the record was trained with); sets mc.WEIGHT_DECAY.  lr is None where the config's LEARNING_RATE holds;
    lr_total_steps is recorded only under the schedules that read it (cosine, linear), so a staircase run may be resumed
    with a larger --max_steps, as ever."""
    off = dict(optimizer="momentum", momentum=float(mc.MOMENTUM), adam_beta1=OPTIONS["beta1"], adam_beta2=OPTIONS["beta2"],
               adam_eps=OPTIONS["eps"], weight_decay=float(mc.WEIGHT_DECAY), clip_norm="per_variable", lr=None, lr_schedule="staircase",
               warmup_steps=0, warmup_factor=WARMUP_FACTOR, min_lr_ratio=0.0, lr_total_steps=None, ema_decay=0.0, ema_warmup=False)
    get = lambda key: getattr(a, key, off[key])
    policy = dict(off, optimizer=str(get("optimizer")), adam_beta1=float(get("adam_beta1")), adam_beta2=float(get("adam_beta2")),
                  adam_eps=float(get("adam_eps")), weight_decay=float(get("weight_decay")), clip_norm=str(get("clip_norm")),
                  lr=None if get("lr") is None else float(get("lr")), lr_schedule=str(get("lr_schedule")),
                  warmup_steps=int(get("warmup_steps")), warmup_factor=float(get("warmup_factor")),
                  min_lr_ratio=float(get("min_lr_ratio")), ema_decay=float(get("ema_decay")), ema_warmup=bool(get("ema_warmup")))
    if policy["lr_schedule"] in ("cosine", "linear"):
        total = getattr(a, "lr_total_steps", getattr(a, "max_steps", None))
        if total is None:
            raise ValueError("lr_schedule %s needs lr_total_steps (or max_steps)" % policy["lr_schedule"])
        policy["lr_total_steps"] = int(total)
    mc.WEIGHT_DECAY = policy["weight_decay"]
    return policy, off


def trainer_options(policy):
    """ops.Optimizer's options of a policy record."""
    return dict(rule=policy["optimizer"], clip=policy["clip_norm"], momentum=policy["momentum"], beta1=policy["adam_beta1"],
                beta2=policy["adam_beta2"], eps=policy["adam_eps"], ema_decay=policy["ema_decay"], ema_warmup=policy["ema_warmup"])

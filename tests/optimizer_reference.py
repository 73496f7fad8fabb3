"""NumPy restatement of sqdet_optimizer_step_opt (include/sqdet.h), operation for operation.

Element-wise arithmetic is float32 with one rounding per operator (NumPy float32 arrays and float32 scalars), the norms are
float64 sums in the kernel's own partition and order -- thread t of block b of a variable with nb blocks adds the squares of
elements b*256 + t, + nb*256, ... in turn, the 256 threads fold by the tree 128, 64, .. 1, the blocks are added in order -- and
the state (t, beta1^t, beta2^t) is float64 running products.  `mutate` switches ONE deliberate mistake on: the host tests show
that a named case tells each of them from the definition.

lr_reference restates squeezedet_amd.optim.lr_at the same way.
"""
import math

import numpy as np

RULES = ("momentum", "nesterov", "adamw")
CLIP_MODES = ("per_variable", "global")
MUTATIONS = ("no_bias_correction", "coupled_adamw", "no_lookahead", "per_variable_under_global", "ema_old_w", "ema_on_skip",
             "t_on_skip")
LR_MUTATIONS = ("warmup_after_W",)
DEFAULTS = dict(rule="momentum", clip="per_variable", momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-8, ema_decay=0.0, ema_warmup=False)
F32 = np.float32


def new_state():
    return np.array([0.0, 1.0, 1.0, 0.0], np.float64)


def nblocks(count):
    """sqdet_optimizer_create: one block per 2048 elements, at least 1, at most 64."""
    return min(64, max(1, -(-int(count) // 2048)))


def block_partials(g):
    """The float64 partial sums of squares opt_sumsq_kernel leaves for one variable (g: its float32 gradient), one per block."""
    c, nb = g.size, nblocks(g.size)
    stride = nb * 256
    laps = -(-c // stride)
    sq = np.zeros(laps * stride, np.float64)
    g64 = g.astype(np.float64)
    sq[:c] = g64 * g64                              # (double)gi * (double)gi: exact
    sq = sq.reshape(laps, nb, 256)
    acc = np.zeros((nb, 256), np.float64)
    for lap in range(laps):                         # each thread's own elements, in turn (a padding 0.0 adds nothing)
        acc = acc + sq[lap]
    off = 128
    while off > 0:                                  # red[t] += red[t + off] for t < off
        acc[:, :off] = acc[:, :off] + acc[:, off:2 * off]
        off >>= 1
    return acc[:, 0].copy()


def variable_sum(g):
    s = 0.0
    for p in block_partials(g):
        s = s + float(p)
    return s


def step(P, G, A, A2, E, state, offs, cnts, decs, lr, max_norm, grad_scale, options=None, mutate=None):
    """One call of sqdet_optimizer_step_opt on float32 arrays P, G, A (and A2 under adamw, E with ema_decay > 0; else None) and the
    float64 [4] state, all updated IN PLACE.  Returns (found_inf, the float32 clip factors)."""
    assert mutate in (None,) + MUTATIONS
    o = dict(DEFAULTS, **(options or {}))
    rule, glob = o["rule"], o["clip"] == "global"
    assert rule in RULES and o["clip"] in CLIP_MODES
    adamw, use_ema = rule == "adamw", o["ema_decay"] > 0.0
    assert (A2 is not None) or not adamw
    assert (E is not None) or not use_ema
    lr, max_norm, gs = F32(lr), F32(max_norm), F32(grad_scale)
    mom, b1, b2, eps = F32(o["momentum"]), F32(o["beta1"]), F32(o["beta2"]), F32(o["eps"])
    omb1, omb2 = F32(1.0 - float(b1)), F32(1.0 - float(b2))          # formed in float64 from the float32 betas, rounded once
    couple = not adamw or mutate == "coupled_adamw"
    with np.errstate(all="ignore"):
        # pass 1
        sums, bad = [], False
        for off, c, d in zip(offs, cnts, decs):
            s = slice(off, off + c)
            g = G[s] * gs
            if couple and F32(d) != 0:
                g = g + F32(d) * P[s]
            G[s] = g
            sums.append(variable_sum(G[s]))
        # pass 2
        norms = [F32(math.sqrt(s)) if s >= 0 else F32(np.nan) for s in sums]       # (a NaN sum: NaN norm)
        bad = any(not (n <= F32(3.0e38)) for n in norms)
        factors = [max_norm / np.fmax(n, max_norm) for n in norms]
        if glob:
            S = 0.0
            for s in sums:
                S = S + s
            N = F32(math.sqrt(S)) if S >= 0 else F32(np.nan)
            bad = bad or not (N <= F32(3.0e38))
            if mutate != "per_variable_under_global":
                factors = [max_norm / np.fmax(N, max_norm)] * len(sums)
        factors = np.array(factors, np.float32)
        if not bad or mutate == "t_on_skip":
            t, p1, p2 = state[0] + 1.0, state[1] * float(b1), state[2] * float(b2)
            state[0], state[1], state[2] = t, p1, p2
        t, p1, p2 = float(state[0]), float(state[1]), float(state[2])
        c1 = F32(1.0 / (1.0 - p1)) if p1 != 1.0 else F32(np.inf)
        c2 = F32(1.0 / (1.0 - p2)) if p2 != 1.0 else F32(np.inf)
        if mutate == "no_bias_correction":
            c1 = c2 = F32(1.0)
        d = float(o["ema_decay"])
        if o["ema_warmup"]:
            d = min(d, (1.0 + t) / (10.0 + t))
        om = F32(1.0 - d)
        # pass 3
        if bad and not (mutate == "ema_on_skip" and use_ema):
            return 1, factors
        for v, (off, c, dec) in enumerate(zip(offs, cnts, decs)):
            s = slice(off, off + c)
            if bad:                                                    # (mutation ema_on_skip only: the average moves regardless)
                E[s] = E[s] + om * (P[s] - E[s])
                continue
            w_old = P[s].copy()
            gc = G[s] * factors[v]
            if adamw:
                m = b1 * A[s] + omb1 * gc
                v2 = b2 * A2[s] + omb2 * (gc * gc)
                u = (m * c1) / (np.sqrt(v2 * c2) + eps)
                if F32(dec) != 0 and mutate != "coupled_adamw":
                    u = u + F32(dec) * P[s]
                A[s], A2[s] = m, v2
                P[s] = P[s] - lr * u
            else:
                a = mom * A[s] + gc
                A[s] = a
                if rule == "nesterov" and mutate != "no_lookahead":
                    P[s] = P[s] - lr * (gc + mom * a)
                else:
                    P[s] = P[s] - lr * a
            if use_ema:
                w = w_old if mutate == "ema_old_w" else P[s]
                E[s] = E[s] + om * (w - E[s])
    return int(bad), factors


def lr_reference(step, base, schedule="staircase", warmup_steps=0, warmup_factor=0.001, min_lr_ratio=0.0, total_steps=None,
                 decay_factor=0.5, decay_steps=10000, mutate=None):
    """squeezedet_amd.optim.lr_at, restated on plain numbers."""
    assert mutate in (None,) + LR_MUTATIONS
    W = warmup_steps
    if schedule == "staircase":
        lr = base * decay_factor ** (step // decay_steps)
    elif schedule == "constant":
        lr = base
    else:
        min_lr = base * min_lr_ratio
        progress = min(max((step - W) / max(1, total_steps - W), 0.0), 1.0)
        lr = (min_lr + 0.5 * (base - min_lr) * (1.0 + math.cos(math.pi * progress)) if schedule == "cosine"
              else base + (min_lr - base) * progress)
    if W > 0 and (step < W or mutate == "warmup_after_W"):
        lr = lr * (warmup_factor + (1.0 - warmup_factor) * step / W)
    return lr

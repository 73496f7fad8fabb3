"""The update step with options without a GPU: the NumPy restatement of sqdet_optimizer_step_opt
(tests/optimizer_reference.py) against numbers worked separately in float64, the schedules of squeezedet_amd.optim.lr_at against
hand-worked values, mutation checks (each deliberate mistake is told from the definition by a named case), and the flag /
policy / checkpoint plumbing of train.py, eval.py and tools/bench_train.py."""
import argparse
import importlib.util
import json
import math
import os

import numpy as np
import pytest

from squeezedet_amd import optim
from tests import optimizer_cases as OC, optimizer_reference as OR

U32 = 2.0 ** -24
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(name):
    """A driver script of the repository root as a module (eval.py shares its name with a builtin)."""
    spec = importlib.util.spec_from_file_location("_script_" + name, os.path.join(ROOT, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _arrays(*rows):
    return [None if r is None else np.array(r, np.float32) for r in rows]


# ---------------------------------------------------------------- the restatement against hand-worked numbers
def _hand64(rule, w, g, a, a2, e, decay, lr, max_norm, gs, mom=0.9, b1=0.9, b2=0.999, eps=1e-8, d=0.0, t=1, glob_norm=None):
    """One update of ONE variable in float64, written from the issue's definition with pow for the bias correction (the kernel
    keeps running products: the two differ by a few 2^-53).  Returns (w, g, a, a2, e)."""
    w, g, a, a2, e = [None if x is None else np.array(x, np.float64) for x in (w, g, a, a2, e)]
    g = g * gs
    if rule != "adamw" and decay:
        g = g + decay * w
    n = math.sqrt(float((g * g).sum())) if glob_norm is None else glob_norm
    gc = g * (max_norm / max(n, max_norm))
    if rule == "adamw":
        a = b1 * a + (1 - b1) * gc
        a2 = b2 * a2 + (1 - b2) * gc * gc
        u = (a / (1 - b1 ** t)) / (np.sqrt(a2 / (1 - b2 ** t)) + eps)
        if decay:
            u = u + decay * w
        w = w - lr * u
    else:
        a = mom * a + gc
        w = w - lr * ((gc + mom * a) if rule == "nesterov" else a)
    if e is not None:
        e = e + (1 - d) * (w - e)
    return w, g, a, a2, e


HAND_CASES = [  # (w, g, accum, accum2, ema, decay, max_norm): one element below the clip; two elements of norm 5 clipped to 1, decayed
    ([1.0], [0.5], [0.2], [0.04], [0.9], 0.0, 1.0),
    ([1.0, -2.0], [3.0, 4.0], [0.2, -0.1], [0.04, 0.09], [0.9, -1.9], 0.25, 1.0),
]


@pytest.mark.parametrize("rule", OR.RULES)
@pytest.mark.parametrize("case", range(len(HAND_CASES)))
def test_one_update_against_hand_worked_float64(rule, case):
    """Every output is at most ten float32 operations on values of magnitude <= 5, each rounding within 2^-24 relative of its
    result: |restatement - float64| <= 16 * 2^-24 * 5 element-wise.  The numbers of the first case, momentum: accum = 0.9 * 0.2 +
    0.5 = 0.68, w = 1 - 0.1 * 0.68 = 0.932, ema = 0.9 + 0.5 * (0.932 - 0.9) = 0.916; nesterov: w = 1 - 0.1 * (0.5 + 0.9 * 0.68) =
    0.8888."""
    w, g, a, a2, e, decay, max_norm = HAND_CASES[case]
    lr, gs, d = 0.1, 0.5 if case else 1.0, 0.5
    P, G, A, A2, E = _arrays(w, g, a, a2, e)
    state = OR.new_state()
    bad, factors = OR.step(P, G, A, A2 if rule == "adamw" else None, E, state, [0], [len(w)], [decay], lr, max_norm, gs,
                           dict(rule=rule, ema_decay=d))
    rw, rg, ra, ra2, re = _hand64(rule, w, g, a, a2, e, decay, lr, max_norm, gs, d=d)
    tol = 16 * U32 * 5
    assert bad == 0 and list(state[:3]) == [1.0, float(F32(0.9)), float(F32(0.999))]
    for what, got, ref in (("params", P, rw), ("grads", G, rg), ("accum", A, ra), ("ema", E, re)) + ((("accum2", A2, ra2),) if rule == "adamw" else ()):
        assert np.abs(got.astype(np.float64) - ref).max() <= tol, (what, got, ref)
    if case == 0 and rule != "adamw":
        want = {"momentum": (0.932, 0.68, 0.916), "nesterov": (0.8888, 0.68, 0.8944)}[rule]
        assert np.allclose([P[0], A[0], E[0]], want, rtol=0, atol=tol)
    if case == 1:
        assert factors[0] < 1.0                      # clipped


def test_three_adam_steps_with_bias_correction_and_ema_warmup():
    """Three AdamW updates of two variables under the global clip, decay on the second, EMA with warm-up: c1 = 1 / (1 - 0.9^t), c2 =
    1 / (1 - 0.999^t) and d = min(0.999, (1 + t) / (10 + t)) = 2/11, 3/12, 4/13 all change per step.  u is a quotient of products
    (eps only damps it), so its relative error is the sum of its ~10 roundings' and of m's and v's own relative errors, |u| <= ~3;
    w and the average carry earlier errors with factors <= 1.  Values <= 2: |restatement - float64| <= 3 * 64 * 2^-24."""
    offs, cnts, decs = [0, 2], [2, 1], [0.0, 0.1]
    P, A, A2, E = _arrays([1.0, -2.0, 0.5], [0.0] * 3, [0.0] * 3, [1.0, -2.0, 0.5])
    ref = [P.astype(np.float64), A.astype(np.float64), A2.astype(np.float64), E.astype(np.float64)]
    grads = [[0.3, -0.4, 1.2], [0.1, 0.2, -0.3], [-3.0, 0.5, 2.0]]
    state, opts = OR.new_state(), dict(rule="adamw", clip="global", ema_decay=0.999, ema_warmup=True)
    for t, g in enumerate(grads, 1):
        G = np.array(g, np.float32)
        assert OR.step(P, G, A, A2, E, state, offs, cnts, decs, 0.05, 1.0, 1.0, opts)[0] == 0
        n = math.sqrt(sum(x * x for x in g))
        d = min(0.999, (1 + t) / (10 + t))
        assert d == [2 / 11, 3 / 12, 4 / 13][t - 1]
        for o, c, dec in zip(offs, cnts, decs):
            s = slice(o, o + c)
            ref[0][s], _, ref[1][s], ref[2][s], ref[3][s] = _hand64("adamw", ref[0][s], np.array(g)[s], ref[1][s], ref[2][s], ref[3][s], dec,
                                                                    0.05, 1.0, 1.0, d=d, t=t, glob_norm=n)
    assert state[0] == 3.0 and abs(state[1] - 0.9 ** 3) < 1e-7 and abs(state[2] - 0.999 ** 3) < 1e-7
    assert state[1] == float(F32(0.9)) ** 2 * float(F32(0.9)) and state[2] == float(F32(0.999)) ** 2 * float(F32(0.999))    # running products
    for what, got, want in zip(("params", "accum", "accum2", "ema"), (P, A, A2, E), ref):
        assert np.abs(got.astype(np.float64) - want).max() <= 3 * 64 * U32, what
    assert np.abs(P.astype(np.float64) - np.array([1.0, -2.0, 0.5])).max() > 0.05       # the updates are of the order of lr each


def test_default_options_restate_the_reference_rule():
    """Defaults = Momentum + per-variable clip, the rule of opt_reference64 (tests/test_gpu_train_kernels.py), within its bound."""
    from tests import test_gpu_train_kernels as TK
    offs, cnts, decs, total = OC.layout()
    P, G, A, _, _ = OC.buffers(offs, cnts, total, seed=1)
    Pr, Gr, Ar, fr, (tolP, tolG, tolA) = TK.opt_reference64(P, G, A, offs, cnts, decs, 0.01, 0.9, 1.0, 0.5)
    inside = OC.inside_mask(offs, cnts, total)
    P0, G0, A0 = P.copy(), G.copy(), A.copy()
    bad, factors = OR.step(P, G, A, None, None, OR.new_state(), offs, cnts, decs, 0.01, 1.0, 0.5)
    assert bad == 0 and (np.abs(factors - fr) <= 2.0 ** -22 * fr).all() and 2 <= int((fr < 1).sum()) <= 7
    for got, ref, tol, before in ((P, Pr, tolP, P0), (G, Gr, tolG, G0), (A, Ar, tolA, A0)):
        assert (np.abs(got[inside].astype(np.float64) - ref[inside]) <= 8 * U32 * tol[inside]).all()
        assert np.array_equal(OC.bits(got)[~inside], OC.bits(before)[~inside])


def test_block_partials_follow_the_kernels_partition():
    """nblocks and the per-thread order, on a variable past the 64-block cap: thread t of block b owns b*256 + t + k * nb*256."""
    assert [OR.nblocks(c) for c in (1, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 10 ** 6)] == [1, 1, 2, 64, 64, 64]
    c = 64 * 2048 + 1
    g = np.zeros(c, np.float32)
    g[0], g[64 * 256], g[5 * 256 + 7] = 2.0, 3.0, 5.0       # element 16384 = block 0, thread 0, second lap
    p = OR.block_partials(g)
    assert p.shape == (64,) and p[0] == 13.0 and p[5] == 25.0 and p.sum() == 38.0
    rs = np.random.RandomState(0)
    g = rs.randn(5000).astype(np.float32)
    assert abs(OR.variable_sum(g) - float((g.astype(np.float64) ** 2).sum())) <= 1e-12 * 5000


@pytest.mark.parametrize("rule", OR.RULES)
def test_each_rule_decreases_a_quadratic(rule):
    """0.5 * ||w - c||^2 with g = w - c, 50 updates, no clip in effect: each rule ends below a tenth of where it began (AdamW's
    steps are of size lr whatever the gradient: it ends within ~lr of c per element, the other two far closer)."""
    rs = np.random.RandomState(3)
    offs, cnts, decs = [0, 70], [65, 3], [0.0, 0.0]
    c = rs.randn(73).astype(np.float32)
    P, A, A2 = np.zeros(73, np.float32), np.zeros(73, np.float32), np.zeros(73, np.float32)
    state = OR.new_state()
    f = lambda: 0.5 * float(((P.astype(np.float64) - c)[np.r_[0:65, 70:73]] ** 2).sum())
    f0 = f()
    for _ in range(50):
        G = (P - c).astype(np.float32)
        OR.step(P, G, A, A2 if rule == "adamw" else None, None, state, offs, cnts, decs, 0.1, 1e6, 1.0, dict(rule=rule, momentum=0.5))
    assert f() < 0.1 * f0 and state[0] == 50.0


# ---------------------------------------------------------------- mutation checks
def _run(options, mutate=None, steps=2, inf_at_step=None, seed=11):
    offs, cnts, decs, total = OC.layout()
    offs, cnts, decs = offs[:7], cnts[:7], decs[:7]          # (the small variables: the host cases need no 131 073-element one)
    P, _, A, A2, E = OC.buffers(offs, cnts, total, seed)
    state = OR.new_state()
    o = dict(OR.DEFAULTS, **options)
    for k in range(steps):
        G = OC.gradients(offs, cnts, total, seed + 1 + k)
        if inf_at_step == k:
            G[offs[-1] + cnts[-1] - 1] = np.inf
        OR.step(P, G, A, A2 if o["rule"] == "adamw" else None, E if o["ema_decay"] > 0 else None, state, offs, cnts, decs, 0.01, 1.0, 0.5,
                options, mutate=mutate)
    return dict(P=P, A=A, A2=A2, E=E, state=state)


def _differs(a, b, keys):
    return [k for k in keys if not np.array_equal(OC.bits(a[k]), OC.bits(b[k]))]


MUTATION_CASES = dict(
    no_bias_correction=(dict(rule="adamw"), {}, ["P"]),
    coupled_adamw=(dict(rule="adamw"), {}, ["P", "A"]),
    no_lookahead=(dict(rule="nesterov"), {}, ["P"]),
    per_variable_under_global=(dict(clip="global"), {}, ["P", "A"]),
    ema_old_w=(dict(ema_decay=0.9), {}, ["E"]),
    ema_on_skip=(dict(ema_decay=0.9), dict(steps=1, inf_at_step=0), ["E"]),
    t_on_skip=(dict(rule="adamw"), dict(steps=2, inf_at_step=0), ["state", "P"]),
)
assert set(MUTATION_CASES) == set(OR.MUTATIONS)


@pytest.mark.parametrize("mutation", OR.MUTATIONS)
def test_each_mutation_is_caught_by_its_case(mutation):
    """Bias correction dropped, decay coupled under adamw, the look-ahead missing, a per-variable factor under the global clip, EMA
    fed the old w, EMA / t advanced on a skipped step: the named case gives other bits in the named outputs."""
    options, kw, outputs = MUTATION_CASES[mutation]
    good, bad = _run(options, **kw), _run(options, mutate=mutation, **kw)
    assert set(outputs) <= set(_differs(good, bad, ["P", "A", "A2", "E", "state"])), mutation
    if mutation == "ema_old_w":
        assert not _differs(good, bad, ["P", "A"])           # only the average tells
    if mutation in ("ema_on_skip", "t_on_skip"):
        skipped = _run(options, steps=1, inf_at_step=0)
        start = _run(options, steps=0)
        assert not _differs(skipped, start, ["P", "A", "A2", "E", "state"])        # the definition: a skipped step touches nothing


# ---------------------------------------------------------------- schedules
def _mc():
    from squeezedet_amd import config
    return config.kitti_squeezeDet_config()


def _policy(argv=(), mc=None, max_steps=None):
    T = _script("train")
    a = T.parse_args(list(argv) + ([] if max_steps is None else ["--max_steps", str(max_steps)]))
    return optim.optim_policy(a, mc or _mc())


def test_default_schedule_is_todays_expression_as_the_same_float():
    mc = _mc()
    policy, off = _policy(mc=mc)
    assert policy == off
    D = int(mc.DECAY_STEPS)
    for step in [0, 1, D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1, 5 * D + 3]:
        today = mc.LEARNING_RATE * mc.LR_DECAY_FACTOR ** (step // mc.DECAY_STEPS)
        assert optim.lr_at(step, policy, mc) == today and isinstance(optim.lr_at(step, policy, mc), float)
        assert OR.lr_reference(step, mc.LEARNING_RATE, decay_factor=mc.LR_DECAY_FACTOR, decay_steps=mc.DECAY_STEPS) == today
    # the trainer's own method, on an object that has none of the new attributes
    from squeezedet_amd.train import _TrainerBase
    tr = _TrainerBase.__new__(_TrainerBase)
    tr.mc, tr.global_step = mc, D + 1
    assert tr.learning_rate() == mc.LEARNING_RATE * mc.LR_DECAY_FACTOR
    tr.optim = dict(policy, lr_schedule="constant", lr=0.5)
    assert tr.learning_rate() == 0.5


def test_cosine_and_linear_hand_worked():
    """base 0.1, W = 10, f = 0.01, T = 110, min_lr_ratio 0.1 (min_lr 0.01).  Warm-up: step 0 -> f, step 5 -> 0.01 + 0.99 / 2 = 0.505
    times the schedule (whose progress is 0 before W: the base rate).  Mid-point, step 60, progress 0.5: cosine 0.01 + 0.045 * (1 + cos(pi/2))
    = 0.055, linear 0.1 - 0.09 / 2 = 0.055.  End, step 110 and past it: min_lr."""
    mc = _mc()
    for sched in ("cosine", "linear"):
        p, _ = _policy(["--lr", "0.1", "--lr_schedule", sched, "--warmup_steps", "10", "--warmup_factor", "0.01", "--min_lr_ratio", "0.1",
                        "--lr_total_steps", "110"], mc)
        lr = lambda s: optim.lr_at(s, p, mc)
        assert lr(0) == pytest.approx(0.1 * 0.01, rel=1e-15) and lr(5) == pytest.approx(0.1 * 0.505, rel=1e-15)
        assert lr(10) == pytest.approx(0.1, rel=1e-15)                       # the multiplier ends AT W
        assert lr(60) == pytest.approx(0.055, rel=1e-12)
        assert lr(110) == pytest.approx(0.01, rel=1e-12) and lr(111) == lr(110) == lr(10 ** 6)
        quarter = 0.01 + 0.045 * (1 + math.cos(math.pi / 4)) if sched == "cosine" else 0.1 - 0.09 / 4
        assert lr(35) == pytest.approx(quarter, rel=1e-12)
        for s in (0, 5, 9, 10, 11, 60, 110, 200):
            assert lr(s) == OR.lr_reference(s, 0.1, sched, 10, 0.01, 0.1, 110)
        assert OR.lr_reference(60, 0.1, sched, 10, 0.01, 0.1, 110, mutate="warmup_after_W") != lr(60)       # the mutation: caught at 60
        assert OR.lr_reference(5, 0.1, sched, 10, 0.01, 0.1, 110, mutate="warmup_after_W") == lr(5)


def test_schedule_edges_no_warmup_total_equal_to_warmup_and_past_total():
    mc = _mc()
    p, _ = _policy(["--lr_schedule", "cosine", "--lr_total_steps", "100"], mc)                  # W = 0: no division by W, step 0 at the base rate
    assert p["warmup_steps"] == 0 and optim.lr_at(0, p, mc) == mc.LEARNING_RATE
    assert optim.lr_at(100, p, mc) == pytest.approx(0.0, abs=1e-18) and optim.lr_at(150, p, mc) == optim.lr_at(100, p, mc)
    p, _ = _policy(["--lr_schedule", "linear", "--lr_total_steps", "4", "--warmup_steps", "4", "--lr", "1.0"], mc)    # T = W: max(1, 0)
    assert optim.lr_at(3, p, mc) == pytest.approx(0.001 + 0.999 * 0.75) and optim.lr_at(4, p, mc) == 1.0 and optim.lr_at(5, p, mc) == 0.0
    p, _ = _policy(["--lr_schedule", "constant", "--warmup_steps", "2", "--lr", "0.25"], mc)
    assert [optim.lr_at(s, p, mc) for s in (0, 1, 2, 99)] == pytest.approx([0.25 * 0.001, 0.25 * (0.001 + 0.999 * 0.5), 0.25, 0.25], rel=1e-15)
    assert optim.lr_at(2, p, mc) == 0.25
    p, _ = _policy(["--warmup_steps", "2"], mc)                                                 # staircase with a warm-up
    assert optim.lr_at(1, p, mc) == pytest.approx(mc.LEARNING_RATE * (0.001 + 0.999 * 0.5), rel=1e-15) and optim.lr_at(2, p, mc) == mc.LEARNING_RATE
    p, _ = _policy(["--lr_schedule", "cosine"], mc, max_steps=40)                               # T defaults to --max_steps
    assert p["lr_total_steps"] == 40


# ---------------------------------------------------------------- flags, policy, checkpoint record
BAD_FLAGS = [
    ["--adam_beta1", "0.8"], ["--adam_beta2", "0.99", "--optimizer", "nesterov"], ["--adam_eps", "1e-6"],           # --adam_* without adamw
    ["--min_lr_ratio", "0.1"], ["--min_lr_ratio", "0.1", "--lr_schedule", "constant"], ["--lr_total_steps", "10"],  # ... without cosine / linear
    ["--ema_warmup"], ["--ema_warmup", "--ema_decay", "0"],
    ["--optimizer", "adam"], ["--clip_norm", "none"], ["--lr_schedule", "step"],
    ["--optimizer", "adamw", "--adam_beta1", "1"], ["--optimizer", "adamw", "--adam_beta1", "-0.1"], ["--optimizer", "adamw", "--adam_beta2", "nan"],
    ["--optimizer", "adamw", "--adam_eps", "0"], ["--optimizer", "adamw", "--adam_eps", "inf"],
    ["--weight_decay", "-1"], ["--weight_decay", "nan"], ["--lr", "0"], ["--lr", "inf"], ["--warmup_steps", "-1"],
    ["--warmup_factor", "1.5"], ["--warmup_factor", "nan"], ["--lr_schedule", "cosine", "--min_lr_ratio", "2"],
    ["--lr_schedule", "cosine", "--min_lr_ratio", "nan"], ["--lr_schedule", "linear", "--lr_total_steps", "0"],
    ["--ema_decay", "1"], ["--ema_decay", "-0.5"], ["--ema_decay", "nan"],
]


@pytest.mark.parametrize("argv", BAD_FLAGS, ids=lambda a: " ".join(a))
def test_flag_errors(argv, capsys):
    from tools import bench_train as BT
    for parse in (_script("train").parse_args, BT.parse_args):
        with pytest.raises(SystemExit):
            parse(list(argv))
    assert "error" in capsys.readouterr().err            # raised through ap.error


def test_policy_defaults_and_flags():
    T = _script("train")
    a = T.parse_args([])
    for key in ("optimizer", "adam_beta1", "adam_beta2", "adam_eps", "weight_decay", "clip_norm", "lr", "lr_schedule", "warmup_steps",
                "warmup_factor", "min_lr_ratio", "lr_total_steps", "ema_decay", "ema_warmup"):
        assert not hasattr(a, key), key                  # a flag that is not given leaves no attribute behind
    mc = _mc()
    wd = mc.WEIGHT_DECAY
    policy, off = optim.optim_policy(a, mc)
    assert policy == off == dict(optimizer="momentum", momentum=mc.MOMENTUM, adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, weight_decay=wd,
                                 clip_norm="per_variable", lr=None, lr_schedule="staircase", warmup_steps=0, warmup_factor=0.001,
                                 min_lr_ratio=0.0, lr_total_steps=None, ema_decay=0.0, ema_warmup=False)
    assert mc.WEIGHT_DECAY == wd and json.loads(json.dumps(policy)) == policy
    a = T.parse_args(["--optimizer", "adamw", "--adam_beta1", "0.8", "--adam_beta2", "0.99", "--adam_eps", "1e-6", "--weight_decay", "0.05",
                      "--clip_norm", "global", "--lr", "0.001", "--lr_schedule", "cosine", "--warmup_steps", "3", "--warmup_factor", "0.1",
                      "--min_lr_ratio", "0.05", "--ema_decay", "0.999", "--ema_warmup", "--max_steps", "77"])
    policy, off2 = optim.optim_policy(a, mc)
    assert off2 == off and mc.WEIGHT_DECAY == 0.05
    assert policy == dict(off, optimizer="adamw", adam_beta1=0.8, adam_beta2=0.99, adam_eps=1e-6, weight_decay=0.05, clip_norm="global",
                          lr=0.001, lr_schedule="cosine", warmup_steps=3, warmup_factor=0.1, min_lr_ratio=0.05, lr_total_steps=77,
                          ema_decay=0.999, ema_warmup=True)
    assert json.loads(json.dumps(policy)) == policy
    assert optim.trainer_options(policy) == dict(rule="adamw", clip="global", momentum=mc.MOMENTUM, beta1=0.8, beta2=0.99, eps=1e-6,
                                                 ema_decay=0.999, ema_warmup=True)
    assert set(optim.trainer_options(off)) == set(optim.OPTIONS) == set(OR.DEFAULTS) and optim.OPTIONS == OR.DEFAULTS
    assert (optim.RULES, optim.CLIP_MODES) == (OR.RULES, OR.CLIP_MODES)
    assert T.parse_args(["--lr_schedule", "cosine", "--lr_total_steps", "5"]).lr_total_steps == 5


def test_bench_train_takes_the_flags():
    from tools import bench_train as BT
    a = BT.parse_args([])
    mc, _ = BT.make_config(a)
    assert BT.make_optim(a, mc) is None                  # no flag: the trainer's own update
    a = BT.parse_args(["--optimizer", "adamw", "--ema_decay", "0.999", "--lr_schedule", "cosine", "--steps", "7", "--warmup", "2"])
    mc, _ = BT.make_config(a)
    p = BT.make_optim(a, mc)
    assert (p["optimizer"], p["ema_decay"], p["lr_schedule"], p["lr_total_steps"]) == ("adamw", 0.999, "cosine", 9)


def test_resume_under_another_optimizer_policy_is_refused():
    T = _script("train")
    mc = _mc()
    loss_off = dict(bbox_loss="delta_l2", focal_gamma=0.0, bbox_loss_coef=5.0)
    adamw, off = optim.optim_policy(argparse.Namespace(optimizer="adamw", lr_schedule="cosine", max_steps=100), mc)
    base = dict(net="squeezeDet", dtype="fp32", augment=T.AUGMENT_OFF, mosaic=0.0, loss=loss_off)
    saved = lambda **kw: json.loads(json.dumps(dict(base, **kw)))          # (a record comes back from the state file as JSON)
    T.check_resume_record(saved(), dict(base), loss_off, off)                                    # absent in both: a run without the flags
    T.check_resume_record(saved(optim=off), dict(base), loss_off, off)
    T.check_resume_record(saved(optim=adamw), dict(base, optim=adamw), loss_off, off)            # recorded and matching
    with pytest.raises(SystemExit, match="--resume: the checkpoint was trained with optim .*momentum.*this run asks for .*adamw"):
        T.check_resume_record(saved(), dict(base, optim=adamw), loss_off, off)                   # absent key: trained with `off`
    with pytest.raises(SystemExit, match="trained with optim .*adamw.*asks for .*momentum"):
        T.check_resume_record(saved(optim=adamw), dict(base), loss_off, off)                     # ... and the reverse
    with pytest.raises(SystemExit, match="optim"):
        T.check_resume_record(saved(optim=adamw), dict(base, optim=dict(adamw, lr_total_steps=200)), loss_off, off)
    with pytest.raises(SystemExit, match="optim"):
        T.check_resume_record(saved(optim=adamw), dict(base, optim=dict(adamw, ema_decay=0.9)), loss_off, off)
    with pytest.raises(SystemExit, match="mosaic"):                                              # the earlier keys still hold
        T.check_resume_record(saved(mosaic=0.5), dict(base), loss_off, off)
    T.check_resume_record(saved(), dict(base), loss_off)                                         # the three-argument form, as before


def test_ema_file_path_rule_and_eval_never_globs_it(tmp_path):
    from squeezedet_amd import checkpoint
    ev = _script("eval")
    d = str(tmp_path)
    assert checkpoint.ema_path(d, 5) == os.path.join(d, "ema", "model.ckpt-5.npz")
    assert checkpoint.ema_of(os.path.join(d, "model.ckpt-5.npz")) == checkpoint.ema_path(d, 5)
    os.makedirs(os.path.join(d, "ema"))
    os.makedirs(os.path.join(d, "state"))
    touch = lambda p: np.savez(p, x=np.zeros(1))
    touch(checkpoint.ema_path(d, 9)); touch(os.path.join(d, "ema", ".tmp-1.npz"))
    assert ev.latest_checkpoint(d) is None and checkpoint.latest(d) is None          # an EMA file alone is no checkpoint
    touch(os.path.join(d, "model.ckpt-5.npz")); touch(os.path.join(d, "state", "step-5.npz")); touch(checkpoint.ema_path(d, 5))
    assert ev.latest_checkpoint(d) == os.path.join(d, "model.ckpt-5.npz") and checkpoint.steps(d) == [5]
    # eval.py --ema: a directory polls <dir>/ema, a file resolves to <dirname>/ema/<basename> and must exist
    assert ev.ema_checkpoint_path(d, run_once=False) == os.path.join(d, "ema")
    assert ev.latest_checkpoint(ev.ema_checkpoint_path(d, run_once=False)) == checkpoint.ema_path(d, 9)
    assert ev.ema_checkpoint_path(os.path.join(d, "model.ckpt-5.npz"), run_once=True) == checkpoint.ema_path(d, 5)
    with pytest.raises(SystemExit, match="--ema: .*ema.model.ckpt-7.npz does not exist"):
        ev.ema_checkpoint_path(os.path.join(d, "model.ckpt-7.npz"), run_once=True)
    a = ev.parse_args([])
    assert a.ema is False and "ema" not in vars(a) and ev.parse_args(["--ema"]).ema is True

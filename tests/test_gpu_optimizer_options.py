"""sqdet_optimizer_step_opt and the trainers behind it on the GPU.

The kernels against tests/optimizer_reference.py BIT FOR BIT -- every buffer, the float64 state and every gap between segments
-- on the layout of tests/optimizer_cases.py (odd and aligned offsets, tails, a variable past the 64-block cap) and on the
300-variable layout of tests/test_gpu_train_kernels.py; the default options against sqdet_optimizer_step itself; the skipped step;
the argument checks.  Then train.py's Run at the trainers' small shape (2 x 128 x 256) with --optimizer adamw --lr_schedule cosine
--warmup_steps 2 --ema_decay 0.9 --ema_warmup: resumed == straight, graphed == eager, the recorded learning rates, the EMA file
and its way into a model through eval.py's loader; and a run without any flag, which keeps the state keys and files it had."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import optimizer_cases as OC, optimizer_reference as OR
from tests.test_gpu_train_kernels import opt_buffers, opt_layout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from squeezedet_amd import ops
    return ops


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dev(a, shift=0):
    """The array on the device; shift: its base pointer moved `shift` floats off the allocation's (so off 16-byte alignment)."""
    if not shift:
        return torch.from_numpy(a).to(DEV)
    t = torch.zeros(a.size + shift, dtype=torch.float32, device=DEV)
    t[shift:].copy_(torch.from_numpy(a))
    return t[shift:]


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.flatnonzero(OC.bits(got) != OC.bits(want))
    assert bad.size == 0, "%s: %d elements differ, first at %d: %r != %r" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


# ---------------------------------------------------------------- the kernels
@pytest.mark.parametrize("which", ["cases", "300"])
def test_default_options_are_the_bits_of_sqdet_optimizer_step(which):
    """rule 0 / clip 0 / no EMA against sqdet_optimizer_step: params, the written-back grads, accum and found_inf, two steps."""
    ops = _ops()
    offs, cnts, decs, total = OC.layout() if which == "cases" else opt_layout()
    P, _, M, inside = opt_buffers(offs, cnts, total, seed=1)
    old, new = ops.MomentumOptimizer(offs, cnts, decs, DEV), ops.Optimizer(offs, cnts, decs, DEV)
    Po, Mo, Pn, Mn = _dev(P), _dev(M), _dev(P), _dev(M)
    fo, fn = [torch.full((1,), 7, dtype=torch.int32, device=DEV) for _ in range(2)]
    for step in range(2):
        G = opt_buffers(offs, cnts, total, seed=2 + step)[1]
        Go, Gn = _dev(G), _dev(G)
        old.step(Po, Go, Mo, 0.01, 0.9, 1.0, 0.5, found_inf=fo)
        new.step(Pn, Gn, Mn, 0.01, 1.0, 0.5, found_inf=fn)
        torch.cuda.synchronize()
        assert int(fo.item()) == int(fn.item()) == 0
        for what, a, b in (("params", Pn, Po), ("grads", Gn, Go), ("accum", Mn, Mo)):
            _same(a, b.cpu().numpy(), "step %d %s" % (step, what))
    assert new.state.cpu().tolist()[0] == 2.0 and not np.array_equal(OC.bits(Pn.cpu().numpy())[inside], OC.bits(P)[inside])


def _against_restatement(offs, cnts, decs, total, options, steps, max_norms, shift=0, seed=20):
    ops = _ops()
    o = dict(OR.DEFAULTS, **options)
    adamw, ema = o["rule"] == "adamw", o["ema_decay"] > 0.0
    ref = OC.buffers(offs, cnts, total, seed)
    start = [b.copy() for b in ref]
    gaps = ~OC.inside_mask(offs, cnts, total)
    dev = [_dev(b, shift) for b in ref]
    state = OR.new_state()
    opt = ops.Optimizer(offs, cnts, decs, DEV, options)
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    for k in range(steps):
        G = OC.gradients(offs, cnts, total, seed + 1 + k)
        ref[1], dev[1] = G.copy(), _dev(G, shift)
        g_in = G.copy()
        opt.step(dev[0], dev[1], dev[2], 0.01, max_norms[k % len(max_norms)], 0.5, accum2=dev[3] if adamw else None,
                 ema=dev[4] if ema else None, found_inf=flag)
        bad, factors = OR.step(ref[0], ref[1], ref[2], ref[3] if adamw else None, ref[4] if ema else None, state, offs, cnts, decs, 0.01,
                               max_norms[k % len(max_norms)], 0.5, options)
        torch.cuda.synchronize()
        assert int(flag.item()) == bad == 0, "a non-finite value in a GAP tripped found_inf"
        for what, d, r, before in zip(("params", "grads", "accum", "accum2", "ema"), dev, ref, start[:1] + [g_in] + start[2:]):
            got = d.cpu().numpy()
            _same(got, r, "step %d %s" % (k, what))
            assert np.array_equal(OC.bits(got)[gaps], OC.bits(before)[gaps]), "step %d: a gap of %s changed" % (k, what)
        _same(opt.state, state, "step %d state" % k)
    used = [0, 2] + ([3] if adamw else []) + ([4] if ema else [])
    for i in (0, 2, 3, 4):                   # the buffers of the rule moved; the others were not touched at all
        moved = not np.array_equal(OC.bits(ref[i]), OC.bits(start[i]))
        assert moved == (i in used), i
    return factors


@pytest.mark.parametrize("ema", OC.EMAS, ids=["noema", "ema", "emawarm"])
@pytest.mark.parametrize("clip", OC.CLIPS)
@pytest.mark.parametrize("rule", OC.RULES)
def test_every_rule_clip_and_ema_against_the_restatement(rule, clip, ema):
    """Three steps; max_norm 1, 50, 1: the per-variable norms (~3 and ~0.3, halved by grad_scale) lie on both sides of 1, the global
    norm above 1 and below 50.  All five buffers, the state and every gap, bit for bit."""
    offs, cnts, decs, total = OC.layout()
    f = _against_restatement(offs, cnts, decs, total, dict(rule=rule, clip=clip, ema_decay=ema[0], ema_warmup=ema[1]), 3, [1.0, 50.0])
    assert (f < 1.0).any() and ((f == 1.0).any() or clip == "global")         # (the last step ran at max_norm 1)


@pytest.mark.parametrize("rule", OC.RULES)
def test_unaligned_base_pointers_take_the_scalar_path_to_the_same_bits(rule):
    """Every base pointer one float off 16-byte alignment: no vector access is possible, the restatement's bits all the same."""
    offs, cnts, decs, total = OC.layout()
    _against_restatement(offs, cnts, decs, total, dict(rule=rule, ema_decay=0.99), 2, [1.0], shift=1)


def test_300_variables_under_the_global_clip():
    """More variables than opt_norm_kernel has threads: its laps of 256 add the per-variable sums in variable-index order."""
    offs, cnts, decs, total = opt_layout()
    ops = _ops()
    P, G, M, inside = opt_buffers(offs, cnts, total, seed=1)
    E = P.copy()
    state = OR.new_state()
    options = dict(rule="nesterov", clip="global", ema_decay=0.9)
    opt = ops.Optimizer(offs, cnts, decs, DEV, options)
    Pd, Gd, Md, Ed = [_dev(a) for a in (P, G, M, E)]
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    opt.step(Pd, Gd, Md, 0.01, 1.0, 0.5, ema=Ed, found_inf=flag)
    bad, factors = OR.step(P, G, M, None, E, state, offs, cnts, decs, 0.01, 1.0, 0.5, options)
    torch.cuda.synchronize()
    assert int(flag.item()) == bad == 0 and len(set(factors.tolist())) == 1 and factors[0] < 0.1
    for what, d, r in (("params", Pd, P), ("grads", Gd, G), ("accum", Md, M), ("ema", Ed, E)):
        _same(d, r, what)
    _same(opt.state, state, "state")


def test_overflow_in_the_last_element_skips_every_buffer_and_the_state():
    """An inf in the last element of the last variable: found_inf = 1; params, accum, accum2, ema and the state keep their bits.  The
    following finite step applies, as update t = 1."""
    ops = _ops()
    offs, cnts, decs, total = OC.layout()
    options = dict(rule="adamw", clip="global", ema_decay=0.99, ema_warmup=True)
    bufs = OC.buffers(offs, cnts, total, seed=5)
    bufs[1][offs[-1] + cnts[-1] - 1] = np.inf
    dev = [_dev(b) for b in bufs]
    opt = ops.Optimizer(offs, cnts, decs, DEV, options)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    opt.step(dev[0], dev[1], dev[2], 0.01, 1.0, 0.5, accum2=dev[3], ema=dev[4], found_inf=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1
    for i, what in ((0, "params"), (2, "accum"), (3, "accum2"), (4, "ema")):
        _same(dev[i], bufs[i], what)
    _same(opt.state, OR.new_state(), "state")
    state = OR.new_state()
    G = OC.gradients(offs, cnts, total, seed=6)
    dev[1] = _dev(G)
    opt.step(dev[0], dev[1], dev[2], 0.01, 1.0, 0.5, accum2=dev[3], ema=dev[4], found_inf=flag)
    assert OR.step(bufs[0], G, bufs[2], bufs[3], bufs[4], state, offs, cnts, decs, 0.01, 1.0, 0.5, options)[0] == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and opt.state.cpu().tolist()[0] == 1.0
    for i, what in ((0, "params"), (2, "accum"), (3, "accum2"), (4, "ema")):
        _same(dev[i], bufs[i], "the finite step's " + what)
    _same(opt.state, state, "state")


def test_bad_arguments_are_refused_before_anything_is_launched():
    ops = _ops()
    from squeezedet_amd._lib import SqdetError
    offs, cnts, decs, total = [0, 8], [5, 3], [0.0, 0.1], 12
    rs = np.random.RandomState(0)
    host = [rs.randn(total).astype(np.float32) for _ in range(5)]
    host[3] = np.abs(host[3])

    def refused(options, accum2=True, ema=True, decays=decs, match="optimizer_step_opt"):
        dev = [_dev(b) for b in host]
        opt = ops.Optimizer(offs, cnts, decays, DEV, options)
        flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
        with pytest.raises(SqdetError, match=match):
            opt.step(dev[0], dev[1], dev[2], 0.01, 1.0, 1.0, accum2=dev[3] if accum2 else None, ema=dev[4] if ema else None, found_inf=flag)
        torch.cuda.synchronize()
        for d, h in zip(dev, host):
            _same(d, h, "a buffer of a refused call")
        assert int(flag.item()) == 7 and opt.state.cpu().tolist() == [0.0, 1.0, 1.0, 0.0]

    refused(dict(rule="adamw"), accum2=False, match="accum2")
    refused(dict(ema_decay=0.9), ema=False, match="ema")
    for key in ("momentum", "beta1", "beta2"):
        for v in (1.0, -0.1, float("nan"), float("inf")):
            refused({key: v}, match="momentum|beta")
    for v in (0.0, -1e-8, float("nan"), float("inf")):
        refused(dict(eps=v), match="eps")
    for v in (1.0, -0.5, float("nan")):
        refused(dict(ema_decay=v), match="ema_decay")
    for v in (-1e-4, float("nan"), float("inf")):
        refused({}, decays=[0.0, v], match="decay")
    with pytest.raises(SqdetError):
        ops.Optimizer(offs, cnts, decs, DEV, dict(rule="adam"))
    with pytest.raises(SqdetError):
        ops.Optimizer(offs, cnts, decs, DEV, dict(beta3=0.5))


# ---------------------------------------------------------------- the trainers, through train.py's Run
FLAGS = ["--optimizer", "adamw", "--lr_schedule", "cosine", "--warmup_steps", "2", "--ema_decay", "0.9", "--ema_warmup"]
STATE_KEYS = ("flat_params", "flat_accum", "flat_accum2", "flat_ema")
_STRAIGHT = {}


def _train():
    if "T" not in _STRAIGHT:
        _STRAIGHT["T"] = _load("train")
    return _STRAIGHT["T"]


def _args(train_dir, dtype, *more):
    os.makedirs(str(train_dir), exist_ok=True)          # (the summaries are written from the first step on)
    return _train().parse_args(["--synthetic", "4", "--seed", "3", "--train_dir", str(train_dir), "--summary_step", "2", "--max_steps", "6",
                                "--image_size", "128", "256", "--batch_size", "2", "--dtype", dtype] + list(more))


def _state(run):
    run.tr.flush()
    torch.cuda.synchronize()
    tr = run.tr
    d = {k: getattr(tr, k).clone().view(torch.int32) for k in STATE_KEYS}
    d["optim_state"] = tr.opt.state.clone().view(torch.int64)
    d["global_step"] = tr.global_step
    return d


def _assert_same_state(a, b):
    assert a["global_step"] == b["global_step"]
    for k in STATE_KEYS + ("optim_state",):
        assert torch.equal(a[k], b[k]), k + " differs"


def _straight(dtype, tmp_path_factory):
    """Six graphed steps (summary steps 0, 2, 4 eager) and the checkpoint of step 5, once per dtype: (state, learning rates asked
    for, the EMA values, the train_dir)."""
    if dtype not in _STRAIGHT:
        from squeezedet_amd.optim import lr_at
        args = _args(tmp_path_factory.mktemp("straight_" + dtype), dtype, *FLAGS)
        run = _train().Run(args)
        assert run.stepper is not None and run.tr.flat_accum2 is not None and run.tr.flat_ema is not None
        start = run.tr.flat_params.clone()
        assert torch.equal(run.tr.flat_ema, start)                       # the average starts as a copy of the variables
        want_lr = {}
        for s in range(6):
            want_lr[s] = lr_at(run.tr.global_step, run.tr.optim, run.mc)
            run.step(s)
        st = _state(run)
        run.save(5)
        ema = {n: v.clone() for n, v in run.tr.ema_params().items()}
        frozen = {n: v.clone() for n, v in run.model.params.items() if not run.model.trainable[n]}
        names, shapes = list(run.tr.names), {n: tuple(run.tr.view[n].shape) for n in run.tr.names}
        run.close()
        _STRAIGHT[dtype] = dict(state=st, lr=want_lr, ema=ema, frozen=frozen, dir=args.train_dir, start=start, names=names, shapes=shapes,
                                skipped=run.tr.skipped_steps, policy=dict(run.tr.optim), base_lr=run.mc.LEARNING_RATE)
    return _STRAIGHT[dtype]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_resumed_run_is_bitwise_the_straight_one(dtype, tmp_path, tmp_path_factory):
    """Six steps straight against three steps, a save, --resume and three more: the variables, both moments, the average, the device
    state and global_step.  And the same checkpoint refuses --resume under another --optimizer, naming `optim`."""
    want = _straight(dtype, tmp_path_factory)
    T = _train()
    args = _args(tmp_path / "resumed", dtype, *FLAGS)
    b = T.Run(args)
    for s in range(3):
        b.step(s)
    b.save(2)
    b.close()
    del b
    from squeezedet_amd import checkpoint
    assert checkpoint.read_extra(args.train_dir, 2)["optim"]["optimizer"] == "adamw"
    with np.load(checkpoint.paths(args.train_dir, 2)[1]) as z:
        assert {"trainer/flat_accum2", "trainer/flat_ema", "trainer/optim_state"} <= set(z.files)
        assert z["trainer/optim_state"].dtype == np.float64 and z["trainer/optim_state"].shape == (4,)
    c = T.Run(args, resume_step=2)
    assert c.first == 3
    for s in range(3, 6):
        c.step(s)
    got = _state(c)
    c.close()
    del c
    _assert_same_state(want["state"], got)
    assert want["state"]["global_step"] + want["skipped"] == 6 and want["state"]["global_step"] >= 3
    assert not torch.equal(want["state"]["flat_ema"], want["start"].view(torch.int32))
    if dtype == "fp32":
        with pytest.raises(SystemExit, match="--resume: the checkpoint was trained with optim .*adamw.*asks for .*nesterov"):
            T.Run(_args(tmp_path / "resumed", dtype, *(FLAGS[2:] + ["--optimizer", "nesterov"])), resume_step=2)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_graph_replay_is_bitwise_the_eager_run(dtype, tmp_path, tmp_path_factory):
    want = _straight(dtype, tmp_path_factory)
    b = _train().Run(_args(tmp_path / "eager", dtype, "--no_graph", *FLAGS))
    assert b.stepper is None
    for s in range(6):
        b.step(s)
    got = _state(b)
    b.close()
    _assert_same_state(want["state"], got)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_recorded_learning_rates_and_the_ema_file(dtype, tmp_path_factory):
    """summaries.jsonl's learning_rate of steps 0, 2, 4 is lr_at of the updates applied by then (W = 2, T = 6: warm-up, then the
    cosine); ema/model.ckpt-5.npz holds ema_params() for the trainable variables and the model's values for the frozen ones; and
    eval.py's --ema path rule and loader put exactly those values into a model."""
    from squeezedet_amd import checkpoint, weights
    want = _straight(dtype, tmp_path_factory)
    lines = [json.loads(l) for l in open(os.path.join(want["dir"], "summaries.jsonl"))]
    assert [l["step"] for l in lines] == [0, 2, 4]
    for l in lines:
        assert l["learning_rate"] == want["lr"][l["step"]], l["step"]
    if dtype == "fp32":                  # no skipped step: the hand values.  step 0: f * base; step 2: progress 0; step 4: progress 1/2
        base = want["base_lr"]
        assert want["skipped"] == 0 and want["policy"]["lr_total_steps"] == 6
        assert [l["learning_rate"] for l in lines] == pytest.approx([0.001 * base, base, 0.5 * base], rel=1e-12)
    path = checkpoint.ema_path(want["dir"], 5)
    assert os.path.isfile(path) and os.path.isfile(checkpoint.paths(want["dir"], 5)[0])
    assert sorted(os.listdir(os.path.join(want["dir"], "ema"))) == ["model.ckpt-5.npz"]
    saved = weights.load_params(path)
    assert set(saved) == set(want["ema"]) | set(want["frozen"]) and want["frozen"]
    for n, v in list(want["ema"].items()) + list(want["frozen"].items()):
        _same(v.float().cpu().numpy().ravel(), saved[n].ravel(), n)
    raw = weights.load_params(checkpoint.paths(want["dir"], 5)[0])
    assert any(not np.array_equal(raw[n], saved[n]) for n in want["ema"])          # the average is not the raw weights
    if dtype == "fp32":
        E = _load("eval")
        a = E.parse_args(["--ema", "--run_once", "--checkpoint_path", checkpoint.paths(want["dir"], 5)[0], "--batch_size", "1"])
        ckpt = E.ema_checkpoint_path(a.checkpoint_path, a.run_once)
        assert ckpt == path
        mc, model = E.make_model(a.net, a.gpu, a.dtype, a.batch_size)
        assert E.load_weights(a, model, ckpt) == "5"
        torch.cuda.synchronize()
        for n, v in list(want["ema"].items()) + list(want["frozen"].items()):
            _same(model.params[n].float().cpu().numpy().ravel(), v.float().cpu().numpy().ravel(), "eval's " + n)
        with pytest.raises(SystemExit, match="--ema: .* does not exist"):
            E.ema_checkpoint_path(os.path.join(want["dir"], "model.ckpt-4.npz"), True)


def test_a_run_without_the_flags_keeps_its_state_keys_and_files(tmp_path):
    """No new flag: state_dict() has the twelve keys it had, the state file no new array and no `optim` record, no ema/ directory
    appears; and a state with the new arrays does not load into it (nor one without them into a trainer that has them)."""
    from squeezedet_amd import checkpoint, ops
    from squeezedet_amd._lib import SqdetError
    T = _train()
    args = T.parse_args(["--synthetic", "4", "--seed", "3", "--train_dir", str(tmp_path / "plain"), "--summary_step", "0", "--max_steps", "2",
                         "--image_size", "128", "256", "--batch_size", "2"])
    os.makedirs(args.train_dir)
    run = T.Run(args)
    assert run.tr.optim is None and type(run.tr.opt) is ops.MomentumOptimizer and run.tr.flat_accum2 is None and run.tr.flat_ema is None
    for s in range(2):
        run.step(s)
    run.save(1)
    d = run.tr.state_dict()
    assert set(d) == {"names", "shapes", "flat_params", "flat_accum", "global_step", "loss_scale", "clean_steps", "skipped_steps", "seed",
                      "rank", "mask_calls", "half"}
    with np.load(checkpoint.paths(args.train_dir, 1)[1]) as z:
        assert {k for k in z.files if k.startswith("trainer/")} == {"trainer/" + k for k in (set(d) - {"names", "shapes"}) | {"names_json", "shapes_json"}}
    assert "optim" not in checkpoint.read_extra(args.train_dir, 1)
    assert {"model.ckpt-1.npz", "state"} <= set(os.listdir(args.train_dir)) and "ema" not in os.listdir(args.train_dir)
    with pytest.raises(SqdetError, match="ema_params|no EMA"):
        run.tr.ema_params()
    for key in ("flat_accum2", "flat_ema", "optim_state"):
        with pytest.raises(SqdetError, match=key):
            run.tr.load_state_dict(dict(d, **{key: d["flat_params"]}))
    run.close()
    del run
    other = T.Run(T.parse_args(["--synthetic", "4", "--seed", "3", "--train_dir", str(tmp_path / "ema"), "--summary_step", "0", "--max_steps", "2",
                                "--image_size", "128", "256", "--batch_size", "2", "--no_graph", "--ema_decay", "0.9"]))
    assert other.tr.flat_ema is not None and other.tr.flat_accum2 is None
    with pytest.raises(SqdetError, match="flat_ema"):
        other.tr.load_state_dict(d)
    full = other.tr.state_dict()
    assert set(full) == set(d) | {"flat_ema", "optim_state"}
    other.tr.load_state_dict(full)
    other.close()

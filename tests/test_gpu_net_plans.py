"""The plan executor's own logic (squeezedet_amd/csrc/net.cpp, sqdet_net_*) on the GPU: every plan structure the planner emits
over the golden matrix -- one small case each, tests/net_plan_cases.CASES; tests/test_net_plan_cases_host.py proves the list
complete -- runs on GUARDED buffers: workspace and preds sit inside allocations of the test's own, between a 64 KiB guard and one at
least as large as the buffer, everything filled with 0xFF bytes (a NaN in both dtypes) before each forward.  A buffer undersized
after absorb_pool's role swap or in a chained run's BUF_S / BUF_T alternation shows as a changed guard byte, a read of something no
launch of this forward wrote as a NaN in preds.  Per case: guards intact, preds finite, input unchanged; preds against the CPU
oracle (float32 plans: the oracle in float64); the batch rolled by one image gives the rolled preds bitwise (batch slots are
independent); a second forward on a re-poisoned workspace gives the same bits; and, for the options test_gpu_model.py states it for,
the plan against the op-by-op graph.

Then the entry points no test called: a weight reload into a live plan (sqdet_net_set_param's second copy of a kernel into a chain
stream, the lazy BN refold, sqdet_net_set_bn_epsilon), sqdet_net_forward_timed, the probe, the signal event, and the post job's
one-shot contract across sqdet_net_forward_timed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import resnet_oracle as R
from oracle import sqdet_oracle as O
from tests import net_plan_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEAD = 64 << 10
TORCH_DTYPE = {"f16": torch.float16, "f32": torch.float32}
ORACLE_ARCH = {"squeezedet": "squeezeDet", "squeezedet_plus": "squeezeDet+"}
OBSERVED = {}      # (arch, dtype) -> largest observed max-error / bound against the oracle (printed by test_zz_report)


# ------------------------------------------------------------------ models and references
def _vgg():
    from tests import test_gpu_vgg16 as V      # the VGG16 oracle is assembled there from the oracle's layer functions
    return V


@functools.lru_cache(maxsize=None)
def _params(arch, dtype, seed):
    """The arch's synthetic parameters as its own model test draws them (kernels rounded to the storage type)."""
    storage = "fp16" if dtype == "f16" else "fp32"
    if arch in ORACLE_ARCH:
        return O.init_params(ORACLE_ARCH[arch], seed=seed, storage=storage)
    if arch == "resnet50":
        return R.init_params(seed=seed)
    return _vgg().vgg16_params(seed, storage)


def _config(arch, size):
    import squeezedet_amd as S
    from squeezedet_amd import config as cfg
    if arch == "squeezedet":
        return S.kitti_squeezeDet_config_for_input(*size)
    if arch == "resnet50":
        return S.kitti_res50_config_for_input(*size)
    if arch == "vgg16":
        return S.kitti_vgg16_config_for_input(*size)
    mc = S.kitti_squeezeDetPlus_config()         # SqueezeDet+ on another input: the grid its VALID 7x7/s2 stem and 3x3/s2 pools give
    mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH = int(size[0]), int(size[1])
    g = []
    for n in size:
        n = (n - 7) // 2 + 1                     # conv1, VALID
        for _ in range(3):
            n = (n - 3) // 2 + 1                 # pool1, pool4, pool8, VALID
        g.append(n)
    mc.ANCHOR_BOX = cfg.set_anchors(mc, g[0], g[1], cfg.SQUEEZEDET_ANCHOR_SHAPES)
    mc.ANCHORS = len(mc.ANCHOR_BOX)
    return mc


def _model(arch, dtype, batch, size, seed=0, bn_eps=None):
    from squeezedet_amd import nets
    mc = _config(arch, size)
    mc.LOAD_PRETRAINED_MODEL = False
    mc.BATCH_SIZE = batch
    if bn_eps is not None:
        mc.BATCH_NORM_EPSILON = bn_eps
    cls = {"squeezedet": nets.SqueezeDet, "squeezedet_plus": nets.SqueezeDetPlus, "resnet50": nets.ResNet50ConvDet,
           "vgg16": nets.VGG16ConvDet}[arch]
    m = cls(mc, gpu_id="0", dtype=TORCH_DTYPE[dtype])
    m.load_params(_params(arch, dtype, seed))
    return m, mc


def _images(dtype, batch, size):
    return O.synthetic_images(batch, size[0], size[1], seed=batch + 7 * size[0] + size[1], storage="fp16" if dtype == "f16" else "fp32")


def _compared(batch):
    """Images are independent: all of a small batch, the first and the last of a large one."""
    return list(range(batch)) if batch <= 3 else [0, batch - 1]


@functools.lru_cache(maxsize=None)
def _reference(arch, dtype, batch, size):
    """The oracle's preds of the compared images (no option reaches the oracle: one reference per shape).  float16 plans: the
    oracle's float16-storage mode; float32 plans: the same functions in float64."""
    x = _images(dtype, batch, size)[_compared(batch)]
    p = _params(arch, dtype, 0)
    if dtype == "f16":
        if arch in ORACLE_ARCH:
            ref = O.forward(ORACLE_ARCH[arch], p, x, "fp16")
        elif arch == "resnet50":
            ref = R.forward(p, x, "fp16")
        else:
            ref = _vgg().vgg16_oracle(p, x, "fp16")
    else:
        p64, x64 = {k: v.double() for k, v in p.items()}, x.double()
        if arch in ORACLE_ARCH:
            ref = O.forward(ORACLE_ARCH[arch], p64, x64, "fp32")
        elif arch == "resnet50":
            ref = R.forward_float64(p, x)
        else:
            ref = _vgg().vgg16_oracle(p64, x64, "fp32")
        assert ref.dtype == torch.float64
    return ref.double().numpy()


def _check_oracle(got, ref, arch, dtype, what, capsys):
    got = got.double().cpu().numpy()
    assert got.shape == ref.shape, what
    scale, err = np.abs(ref).max(), np.abs(got - ref).max()
    # float32: 1e-3 relative (north star).  float16: tests/test_gpu_model.py::_check_layers' bound -- both sides round every activation
    # to float16 and one-ulp flips propagate; documented there as twice the largest observed
    bound = 1e-3 * scale + 1e-5 if dtype == "f32" else 5e-3 * scale + 1e-3
    OBSERVED[(arch, dtype)] = max(OBSERVED.get((arch, dtype), 0.0), float(err / bound))
    with capsys.disabled():
        print("\n  [%s] max err %.3e of scale %.3e = %.3e; err / bound %.3f" % (what, err, scale, err / max(scale, 1e-30), err / bound))
    assert err <= bound, "%s: max err %g vs scale %g" % (what, err, scale)


# ------------------------------------------------------------------ guarded buffers
class Guarded:
    """[64 KiB guard | body of nbytes, 256-byte aligned | guard of max(nbytes, 1 MiB)] in one uint8 tensor of the test's own:
    an overrun of the body is observed in the guards, not faulted on."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.raw = torch.empty(HEAD + self.nbytes + max(self.nbytes, 1 << 20) + 256, dtype=torch.uint8, device=DEV)
        self.off = HEAD + (-(self.raw.data_ptr() + HEAD)) % 256
        self.body = self.raw[self.off:self.off + self.nbytes]
        assert self.body.data_ptr() % 256 == 0

    def poison(self):
        self.raw.fill_(0xFF)

    def guards_intact(self):
        head, tail = self.raw[:self.off], self.raw[self.off + self.nbytes:]
        assert head.numel() >= HEAD and tail.numel() >= max(self.nbytes, 1 << 20)
        return bool((head == 0xFF).all()) and bool((tail == 0xFF).all())


class GuardedPlan:
    """A NetPlan re-bound (sqdet_net_bind, same param_mem) to a guarded workspace, writing guarded preds."""

    def __init__(self, plan):
        from squeezedet_amd import _lib
        self.plan = plan
        self.ws = Guarded(plan.workspace.numel())
        _lib.check(_lib.lib().sqdet_net_bind(plan._h, C.c_void_p(plan.param_mem.data_ptr()), C.c_void_p(self.ws.body.data_ptr())),
                   "sqdet_net_bind")
        plan.workspace = self.ws.body
        shape = (plan.batch, plan.gh, plan.gw, plan.out_ch)
        self.out = Guarded(int(np.prod(shape)) * torch.empty((), dtype=plan.dtype).element_size())
        self.preds = self.out.body.view(plan.dtype).view(shape)

    def forward(self, x, what):
        """One forward on freshly poisoned buffers; returns a copy of preds."""
        keep = x.clone()
        self.ws.poison()
        self.out.poison()
        got = self.plan.forward(x, preds=self.preds)
        torch.cuda.synchronize()
        assert got.data_ptr() == self.preds.data_ptr()
        assert self.ws.guards_intact(), "%s: a launch wrote outside the %d-byte workspace" % (what, self.ws.nbytes)
        assert self.out.guards_intact(), "%s: a launch wrote outside preds" % what
        assert bool(torch.isfinite(self.preds).all()), "%s: preds hold values no launch of this forward computed" % what
        assert torch.equal(x, keep), "%s: the input tensor was modified" % what
        return self.preds.clone()


class _Option:
    """ops.set_option for the time of a case: set before the plan is created, kept through the forwards (some launchers re-check
    their eligibility at launch), restored on the way out."""

    def __init__(self, option):
        self.option = option

    def __enter__(self):
        from squeezedet_amd import ops
        if self.option is not None:
            ops.set_option(self.option[0], self.option[1])

    def __exit__(self, *exc):
        from squeezedet_amd import ops
        if self.option is not None:
            ops.set_option(self.option[0], self.option[2])


# ------------------------------------------------------------------ every plan structure
@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_id)
def test_plan_structure_on_guarded_buffers(case, capsys):
    arch, dtype, batch, size, option = case
    what = NC.case_id(case)
    m, mc = _model(arch, dtype, batch, size)
    x = _images(dtype, batch, size).to(DEV, TORCH_DTYPE[dtype])
    from squeezedet_amd import _lib
    want = NC.structure(_lib.lib(), *case)                           # (sets and restores the option itself: ahead of _Option)
    with _Option(option):
        plan = m._native_plan(batch)
        assert tuple(r[0] for r in plan.layer_table()) == want, what  # the plan that runs is the plan the host test counted
        g = GuardedPlan(plan)
        p1 = g.forward(x, what)
        p2 = g.forward(x, what + " (second forward)")
        assert torch.equal(p2, p1), "%s: a second forward of the same input on a re-poisoned workspace differs" % what
        # batch slots are independent: no kernel of the forward states a slot-dependent summation order, so this is bitwise
        p3 = g.forward(torch.roll(x, 1, 0), what + " (batch rolled by one)")
        assert torch.equal(p3, torch.roll(p1, 1, 0)), "%s: an image's preds depend on its slot in the batch" % what
        graph = None
        if option is None or option[:2] == ("stem_algo", 2):         # what test_gpu_model.py claims of plan vs op-by-op graph
            graph = m.run([m.preds], {m.image_input: x}, use_plan=False)[0]
            torch.cuda.synchronize()
    idx = _compared(batch)
    _check_oracle(p1[idx], _reference(arch, dtype, batch, size), arch, dtype, what, capsys)
    if graph is not None:
        if dtype == "f32":
            assert torch.equal(p1, graph), "%s: native plan and op-by-op graph must run the same kernels" % what
        elif option is not None:
            assert torch.equal(p1, graph), "%s: native plan (strip stem) and op-by-op graph must run the same kernels" % what
        else:
            d = (p1.float() - graph.float()).abs().max().item()
            scale = graph.float().abs().max().item()
            assert d <= 4e-3 * scale + 1e-4, "%s: plan vs graph: %g of %g" % (what, d, scale)


def test_zz_report(capsys):
    """Prints the largest observed error / bound against the oracle per (arch, dtype) of the cases above (runs behind them)."""
    with capsys.disabled():
        print("\nlargest observed max-error / bound vs the oracle:")
        for k in sorted(OBSERVED):
            print("  %-16s %-4s %.3f" % (k[0], k[1], OBSERVED[k]))


# ------------------------------------------------------------------ parameter reload into a live plan
RELOAD_SIZE = {"squeezedet": (130, 236), "squeezedet_plus": (97, 131), "resnet50": (97, 131), "vgg16": (97, 131)}


@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("arch", ["squeezedet", "squeezedet_plus", "resnet50", "vgg16"])
def test_param_reload_into_a_live_plan(arch, dtype):
    """Parameters A, a forward, parameters B (another seed), a forward: bitwise what a fresh plan that only ever saw B computes --
    every copy of every kernel followed (the packed kernel, its second copy in a chain launch's stream, the lazily re-folded BN).  An
    unknown name raises and changes nothing.  ResNet50: sqdet_net_set_bn_epsilon on the live plan = a plan created with that epsilon."""
    from squeezedet_amd import _lib
    size, batch = RELOAD_SIZE[arch], 2
    x = _images(dtype, batch, size).to(DEV, TORCH_DTYPE[dtype])
    m, mc = _model(arch, dtype, batch, size, seed=0)
    plan = m._native_plan(batch)
    if (arch, dtype) == ("squeezedet", "f16"):          # both launches whose kernels travel outside their own parameter slot
        names = [r[0] for r in plan.layer_table()]
        assert names[0] == "conv1+pool1+fire2/squeeze1x1", names
        assert plan.overlap_layer() >= 0 and "/expand" in names[plan.overlap_layer()], names
    pa = plan.forward(x).clone()
    m.load_params(_params(arch, dtype, 1))
    assert m._native_plan(batch) is plan                # the live plan takes the new values (sqdet_net_set_param)
    pb = plan.forward(x).clone()
    fresh, _ = _model(arch, dtype, batch, size, seed=1)
    pf = fresh._native_plan(batch).forward(x).clone()
    torch.cuda.synchronize()
    assert not torch.equal(pa, pb)
    assert torch.equal(pb, pf), "a reloaded plan differs from a fresh plan with the same parameters"
    with pytest.raises(_lib.SqdetError):
        plan.set_param("fire99/squeeze1x1/kernels", torch.zeros(16, device=DEV))
    pc = plan.forward(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(pc, pb), "a refused set_param changed the plan"
    if arch == "resnet50":
        plan.set_bn_epsilon(1e-2)
        pe = plan.forward(x).clone()
        other, _ = _model(arch, dtype, batch, size, seed=1, bn_eps=1e-2)
        po = other._native_plan(batch).forward(x).clone()
        torch.cuda.synchronize()
        assert not torch.equal(pe, pb)
        assert torch.equal(pe, po), "set_bn_epsilon on a live plan differs from a plan created with that epsilon"


# ------------------------------------------------------------------ measuring and signalling entry points
SMALL = ("squeezedet", "f16", 2, (130, 236))


@pytest.fixture()
def small():
    m, mc = _model(*SMALL)
    x = _images(*SMALL[1:]).to(DEV, torch.float16)
    plan = m._native_plan(SMALL[2])
    p0 = plan.forward(x).clone()
    torch.cuda.synchronize()
    return m, mc, plan, x, p0


def test_forward_timed_equals_forward(small):
    m, mc, plan, x, p0 = small
    preds, ms = plan.forward_timed(x)
    torch.cuda.synchronize()
    assert torch.equal(preds, p0)
    assert len(ms) == len(plan.layer_table()) and all(np.isfinite(v) and v >= 0.0 for v in ms), ms


def test_probe_records_what_the_latest_set_probe_allows(small):
    """sqdet_net_set_probe(layer, max_records): the next forwards time that layer's launch, max_records times at the most, until
    sqdet_net_read_probe takes the records; a later, smaller max_records holds (the events of the earlier, larger one stay allocated)."""
    from squeezedet_amd import _lib
    m, mc, plan, x, p0 = small
    nl = len(plan.layer_table())
    layer = plan.overlap_layer()

    def forwards(k):
        for _ in range(k):
            plan.forward(x)
        torch.cuda.synchronize()

    plan.set_probe(layer, 3)
    forwards(5)
    got = plan.read_probe(8)
    assert len(got) == 3 and all(np.isfinite(v) and v >= 0.0 for v in got), got
    assert plan.read_probe(8) == []                      # taken: nothing is left without further forwards
    plan.set_probe(layer, 1)
    forwards(5)
    got = plan.read_probe(8)
    assert len(got) == 1 and np.isfinite(got[0]) and got[0] >= 0.0, "set_probe(%d, 1) after set_probe(%d, 3): %d records" % (layer, layer, len(got))
    plan.set_probe(-1, 0)
    forwards(2)
    assert plan.read_probe(8) == []
    for bad in (nl, -2):
        with pytest.raises(_lib.SqdetError):
            plan.set_probe(bad, 1)
    with pytest.raises(_lib.SqdetError):
        plan.set_probe(0, -1)
    assert torch.equal(plan.forward(x), p0)


def test_signal_event_is_recorded_by_the_forward(small):
    from squeezedet_amd import _lib
    m, mc, plan, x, p0 = small
    nl = len(plan.layer_table())
    ev, before = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev.record()                                          # recorded once: its handle exists
    torch.cuda.current_stream().synchronize()
    before.record()
    plan.set_signal(plan.overlap_layer(), ev)
    p1 = plan.forward(x).clone()
    torch.cuda.current_stream().synchronize()
    assert ev.query(), "the signal event has not completed behind a synchronised forward"
    assert before.elapsed_time(ev) > 0.0, "the forward did not record the signal event again (it still holds its first record)"
    assert torch.equal(p1, p0)
    for bad in (nl, -1):
        with pytest.raises(_lib.SqdetError):
            plan.set_signal(bad, ev)
    plan.set_signal(-1, None)                            # cleared
    p2 = plan.forward(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(p2, p0)


def test_post_job_is_one_shot_across_forward_timed(small):
    """sqdet_net_set_post_job is consumed by ONE forward, whichever entry point launches it: a timed forward carries the riders
    (outputs = sqdet_detect_filter's, as test_gpu_model.py::test_post_job_riders_equal_the_filter_launch states it), and the next
    forward carries none."""
    from squeezedet_amd import ops
    m, mc, plan, x, p0 = small
    batch = SMALL[2]
    assert plan.rider_capacity() >= batch and plan.scores_supported()
    scores = torch.empty((batch, mc.ANCHORS), dtype=torch.float32, device=DEV)
    preds = plan.forward(x, scores=scores).clone()
    want = ops.detect_filter(preds, m.anchors_f32(), mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH,
                             mc.TOP_N_DETECTION, mc.NMS_THRESH, scratch=scores, scores_ready=True)
    out = [torch.full_like(t, -7) for t in want]
    plan.set_post_job(preds, scores, m.anchors_f32(), out, mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT,
                      mc.EXP_THRESH, mc.TOP_N_DETECTION, mc.NMS_THRESH)
    p1, _ = plan.forward_timed(x)                        # carries the riders
    torch.cuda.synchronize()
    assert torch.equal(p1, preds) and torch.equal(preds, p0)
    for g_, w_ in zip(out, want):
        assert torch.equal(g_, w_)
    for t in out:
        t.fill_(-7)
    plan.forward(x)                                      # one-shot: no riders this time
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out), "the post job rode again in the forward behind forward_timed"

"""GPU tests of sqdet_build_labels_opt (squeezedet_amd/csrc/assign.hip): the kernel against the sequential
NumPy restatement (tests/assign_reference.py) on every case of tests/assign_cases.py under both modes; tests/test_assign_host.py
shows without a GPU that every case reaches the branch it is named after and that every tie rule decides at least one case.

Every case x mode: input_mask, box_input, labels, anchor_index, assigned_box and positives equal the restatement exactly;
box_delta_input[..., 0:2] has the bits of the float64 quotient rounded once; [..., 2:4] is within rtol 1e-6 / atol 1e-7 of the
float64 log rounded once, with identical infinities and no NaN (the comparison tests/test_gpu_input_path.py applies to `log`).
The outputs and the workspace live inside larger poisoned tensors whose guard cells must stay untouched, and are dirty on entry.
Then: the default route against sqdet_build_labels bit for bit, the refusals, GraphedStep under atss against the eager step, and
train.py --assign atss with its checkpoint record."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import assign_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                 # poisoned cells in front of and behind every output view
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the cases' arrays are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _options(case, mode):
    from squeezedet_amd import assign
    return assign.assign_options(mode, case.iou_thresh, case.max_per_box, case.topk)


class Guarded:
    """A view of `shape` inside a larger tensor filled with `fill`: GUARD cells before and behind it."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.before = self.whole.clone()
        self.view = self.whole[GUARD:GUARD + n].view(shape)
        self.n = n

    def guards_untouched(self):
        w, b = _bits(self.whole.cpu().numpy()), _bits(self.before.cpu().numpy())
        return np.array_equal(w[:GUARD], b[:GUARD]) and np.array_equal(w[GUARD + self.n:], b[GUARD + self.n:])


def _guarded_outputs(B, A, M, C, ws_bytes):
    f = lambda *s: Guarded(s, torch.float32, float("nan"))
    i = lambda *s: Guarded(s, torch.int32, -7)
    return [f(B, A), f(B, A, 4), f(B, A, 4), f(B, A, C), i(B, M), i(B, A), i(B, M), Guarded((max(8, ws_bytes),), torch.uint8, 0xA5)]


def _abi(case, mode, outs, dims=None, apg=None, opt=None):
    """The C entry on outputs the caller allocated."""
    import ctypes
    from squeezedet_amd import _lib, assign, ops
    c = case.label
    (B, M), A = c.cls.shape, len(c.anchors)
    o = _options(case, mode) if opt is None else opt
    rec = ops._AssignOptions(assign.ASSIGN_MODES.index(o.mode), o.iou_thresh, o.max_per_box, o.topk)
    ins = [_t(c.anchors), _t(c.gt), _t(c.cls), _t(c.cnt)]
    p = [ctypes.c_void_p(t.data_ptr()) for t in ins + outs]
    rc = _lib.lib().sqdet_build_labels_opt(*p, *(dims or (B, A, M, c.C)), case.apg if apg is None else apg,
                                           ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _workspace_bytes(case, mode):
    import ctypes
    from squeezedet_amd import _lib, assign, ops
    o = _options(case, mode)
    rec = ops._AssignOptions(assign.ASSIGN_MODES.index(o.mode), o.iou_thresh, o.max_per_box, o.topk)
    (B, M), A = case.label.cls.shape, len(case.label.anchors)
    return int(_lib.lib().sqdet_build_labels_opt_workspace_bytes(B, A, M, case.apg, ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p)))


def _check(name, mode, outs):
    ref = AC.reference(name, mode)
    mask, delta, box, lab, aidx, abox, pos = [t.cpu().numpy() for t in outs[:7]]
    what = "%s / %s: " % (name, mode)
    assert aidx.dtype == abox.dtype == pos.dtype == np.int32 and mask.dtype == delta.dtype == box.dtype == lab.dtype == np.float32
    assert np.array_equal(aidx, ref.aidx), what + "anchor_index"
    assert np.array_equal(abox, ref.assigned_box), what + "assigned_box differs at %s" % np.argwhere(abox != ref.assigned_box)[:8].tolist()
    assert np.array_equal(pos, ref.positives), what + "positives"
    assert np.array_equal(mask, ref.mask), what + "input_mask"
    assert np.array_equal(lab, ref.labels), what + "labels"
    assert np.array_equal(box, ref.box), what + "box_input"
    with np.errstate(over="ignore"):
        want = ref.delta64.astype(np.float32)                   # rounded once
    assert np.array_equal(_bits(delta[..., 0:2]), _bits(want[..., 0:2])), what + "box_delta_input[..., 0:2] bits"
    np.testing.assert_allclose(delta[..., 2:4], want[..., 2:4], rtol=1e-6, atol=1e-7, err_msg=what + "box_delta_input[..., 2:4]")
    assert np.array_equal(np.isinf(delta), np.isinf(want)) and not np.isnan(delta).any()


@pytest.mark.parametrize("mode", AC.MODES)
@pytest.mark.parametrize("name", AC.ASSIGN_CASES)
def test_kernel_equals_the_restatement_on_guarded_dirty_buffers(name, mode):
    """The entry on poisoned outputs inside poisoned buffers, twice (the second call meets the first call's results in the outputs
    and the workspace): both equal the restatement, the guard cells keep their bits."""
    case = AC.assign_case(name)
    c = case.label
    (B, M), A = c.cls.shape, len(c.anchors)
    ws_bytes = _workspace_bytes(case, mode)
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    g = _guarded_outputs(B, A, M, c.C, ws_bytes)
    for _ in range(2):
        assert _abi(case, mode, [x.view for x in g]) == 0
        _check(name, mode, [x.view for x in g])
        assert all(x.guards_untouched() for x in g), "%s / %s: a guard cell was written" % (name, mode)


@pytest.mark.parametrize("name", ["identical", "counts", "kitti"])
def test_ops_route_and_default_route(name):
    """ops.build_labels under both modes returns seven tensors equal to the restatement; assign=None and mode `reference` return
    sqdet_build_labels' five, bit for bit what the entry without the keyword returns."""
    from squeezedet_amd import assign, ops
    case = AC.assign_case(name)
    c = case.label
    ins = lambda: (_t(c.anchors), _t(c.gt), _t(c.cls), _t(c.cnt))
    for mode in AC.MODES:
        outs = ops.build_labels(*ins(), c.C, assign=_options(case, mode), anchors_per_grid=case.apg)
        torch.cuda.synchronize()
        assert len(outs) == 7
        _check(name, mode, outs)
    plain = ops.build_labels(*ins(), c.C)
    for opt in (None, assign.assign_options(), assign.assign_options("reference", 0.1, 3, 2)):
        got = ops.build_labels(*ins(), c.C, assign=opt, anchors_per_grid=case.apg)
        torch.cuda.synchronize()
        assert len(got) == len(plain) == 5
        for a, b in zip(got, plain):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    ref = AC.reference(name, "reference")
    assert np.array_equal(plain[0].cpu().numpy(), ref.mask) and np.array_equal(plain[4].cpu().numpy(), ref.aidx)


@pytest.mark.parametrize("bad", ["A%apg", "max_per_box=65", "topk=33", "mode=0", "opt=NULL", "thresh<0", "topk=0", "candidates>1024"])
def test_refusals_leave_the_outputs_untouched(bad):
    import ctypes
    from squeezedet_amd import _lib, assign
    case = AC.assign_case("classes1")
    c = case.label
    (B, M), A = c.cls.shape, len(c.anchors)
    g = _guarded_outputs(B, A, M, c.C, 1 << 16)
    outs = [x.view for x in g]
    O = assign.AssignOptions
    mode, apg, opt, code = "iou", None, None, _lib.SQDET_EUNSUPPORTED
    if bad == "A%apg":
        apg, code = 4, -1
    elif bad == "max_per_box=65":
        opt = O("iou", 0.5, 65, 9)
    elif bad == "topk=33":
        opt = O("atss", 0.5, 16, 33)
    elif bad == "mode=0":
        opt, code = O("reference", 0.5, 16, 9), -1
    elif bad == "thresh<0":
        opt, code = O("iou", -0.5, 16, 9), -1
    elif bad == "topk=0":
        opt, code = O("atss", 0.5, 16, 0), -1
    if bad == "opt=NULL":
        p = [ctypes.c_void_p(t.data_ptr()) for t in [_t(c.anchors), _t(c.gt), _t(c.cls), _t(c.cnt)] + outs]
        rc = _lib.lib().sqdet_build_labels_opt(*p, B, A, M, c.C, case.apg, None, _lib.stream_ptr())
        code = -1
    elif bad == "candidates>1024":
        big = AC.AssignCase("big", AC.IC.label_case("cap"), 40, 0.5, 16, 32)       # 1080 anchors: 40 shapes x min(32, 27) = 1080 > 1024
        cb = big.label
        (B, M), A = cb.cls.shape, len(cb.anchors)
        g = _guarded_outputs(B, A, M, cb.C, 1 << 16)
        outs = [x.view for x in g]
        rc = _abi(big, "atss", outs)
    else:
        rc = _abi(case, mode, outs, apg=apg, opt=opt)
    assert rc == code, "%s: code %d" % (bad, rc)
    assert _lib.lib().sqdet_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs[:4]) and all(bool((t == -7).all()) for t in outs[4:7]) and bool((outs[7] == 0xA5).all())


def _trainer(assign_opt, seed=9):
    import squeezedet_amd as S
    from oracle import sqdet_oracle as O
    from squeezedet_amd import nets
    from squeezedet_amd.train import SqueezeDetTrainer
    mc = S.kitti_squeezeDet_config_for_input(128, 256)
    mc.LOAD_PRETRAINED_MODEL = False
    mc.IS_TRAINING = True
    mc.BATCH_SIZE = 2
    m = nets.SqueezeDet(mc, gpu_id="0", dtype=torch.float32)
    m.load_params(O.init_params("squeezeDet", seed=seed))
    return SqueezeDetTrainer(m, assign=assign_opt), mc


def test_graphed_step_under_atss_equals_the_eager_step():
    """GraphedStep with the atss label build captured on the side stream against trainer.step on ops.build_labels' tensors, at
    2 x 128 x 256: one step leaves bit-identical variables, momentum and losses; three more replays with fresh boxes keep
    following the eager steps (the captured build reads its static inputs, not the boxes of the capture)."""
    from oracle import sqdet_oracle as O
    from squeezedet_amd import assign, ops
    from squeezedet_amd.train import GraphedStep
    opt = assign.assign_options("atss", topk=9)
    omc = O.squeezeDet_config_for_input(128, 256)
    rs = np.random.RandomState(77)
    B, M = 2, 5

    def boxes():
        gt = np.stack([rs.uniform(0, 256, (B, M)), rs.uniform(0, 128, (B, M)), rs.uniform(20, 120, (B, M)), rs.uniform(20, 90, (B, M))], 2)
        return _t(gt), _t(rs.randint(0, 3, (B, M)).astype(np.int32)), _t(np.array([5, rs.randint(1, 5)], np.int32))
    batches = [(O.synthetic_images(B, 128, 256, seed=80 + i).to(DEV), boxes()) for i in range(4)]
    res = []
    for graphed in (False, True):
        tr, mc = _trainer(opt)
        tr.seed = 4321
        anchors = torch.from_numpy(omc.ANCHOR_BOX).to(DEV)
        gs = GraphedStep(tr, anchors, 3) if graphed else None
        assert gs is None or gs.assign == opt
        trace = []
        for x, (gt, cls, cnt) in batches:
            if graphed:
                out = gs.step(x, gt, cls, cnt)
            else:
                lab = ops.build_labels(anchors, gt, cls, cnt, 3, assign=opt, anchors_per_grid=int(mc.ANCHOR_PER_GRID))
                out = tr.step(x, *lab[:4])
            torch.cuda.synchronize()
            trace.append(([float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss")], float(out["num_objects"]),
                          tr.flat_params.clone(), tr.flat_accum.clone()))
        res.append(trace)
    for step, (e, g) in enumerate(zip(*res)):
        assert e[0] == g[0] and e[1] == g[1], "step %d: losses / num_objects %s vs %s" % (step, e[:2], g[:2])
        assert torch.equal(e[2], g[2]) and torch.equal(e[3], g[3]), "step %d: variables or momentum differ" % step
    assert len({e[1] for e in res[0]}) > 1 and all(e[1] > 5 for e in res[0])      # more positives than objects, changing with the boxes


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_driver_records_the_policy_and_refuses_another_on_resume(tmp_path, capsys):
    """train.py --synthetic 8 --max_steps 4 --assign atss: runs, every checkpoint carries the `assign` record, the summaries line
    reports more than one positive per object; --resume --assign iou on that directory is refused."""
    import re
    from squeezedet_amd import checkpoint
    T = _load("train")
    d = str(tmp_path / "run")
    common = ["--synthetic", "8", "--seed", "3", "--train_dir", d, "--image_size", "128", "256", "--batch_size", "2", "--summary_step", "2",
              "--checkpoint_step", "2"]
    T.main(common + ["--max_steps", "4", "--assign", "atss"])
    out = capsys.readouterr().out
    notes = [float(v) for v in re.findall(r"positives per object: ([0-9.]+)", out)]
    assert len(notes) == 2 and all(v > 1.0 for v in notes), out
    for step in (0, 2, 3):
        assert checkpoint.read_extra(d, step)["assign"] == dict(mode="atss", topk=9)
    with pytest.raises(SystemExit) as e:
        T.main(common + ["--max_steps", "6", "--resume", "--assign", "iou"])
    assert "assign" in str(e.value)

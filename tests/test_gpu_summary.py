"""sqdet_tensor_stats_many (csrc/summary.hip) through squeezedet_amd.summary.tensor_stats against NumPy on the same float32
values.  Every integer field and min / max: exact.  sum / sumsq: against float64 (math.fsum for the small cases) within the
bound of a float64 recursive sum in ANY order, |err| <= n * 2^-53 * sum(|x|) (resp. sum(x^2): a float32 square is exact in
float64) -- computed per case, not tuned."""
import math

import numpy as np
import pytest
import torch

from squeezedet_amd import summary

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53


def ref_record(x, edges):
    """NumPy reference of one record on float32 values x."""
    x = np.asarray(x, np.float32)
    fin = np.isfinite(x)
    xf = x[fin]
    idx = np.searchsorted(edges, xf, side="right")
    cnt = np.bincount(idx, minlength=len(edges) + 1)
    xd = xf.astype(np.float64)
    if len(xf) <= 5000:
        s, ss, sa = math.fsum(xd), math.fsum(xd * xd), math.fsum(np.abs(xd))
    else:
        s, ss, sa = float(xd.sum()), float((xd * xd).sum()), float(np.abs(xd).sum())
    return dict(count=len(x), nonfinite=int((~fin).sum()), zeros=int((xf == 0).sum()),
                min=float(xf.min()) if len(xf) else float("inf"), max=float(xf.max()) if len(xf) else float("-inf"),
                sum=s, sumsq=ss, sumabs=sa, under=int(cnt[0]), hist=cnt[1:-1], over=int(cnt[-1]))


def check(rec, ref, what):
    n = max(int(ref["count"]) - int(ref["nonfinite"]), 1)
    line = "%s: count %d sum err %.3e (bound %.3e) sumsq err %.3e (bound %.3e)" % (
        what, ref["count"], abs(float(rec["sum"]) - ref["sum"]), n * U * ref["sumabs"], abs(float(rec["sumsq"]) - ref["sumsq"]),
        n * U * ref["sumsq"])
    print(line)
    for k in ("count", "nonfinite", "zeros", "under", "over"):
        assert int(rec[k]) == ref[k], (what, k, int(rec[k]), ref[k])
    assert np.array_equal(np.asarray(rec["hist"]), ref["hist"]), (what, "hist")
    assert float(rec["min"]) == ref["min"] and float(rec["max"]) == ref["max"], (what, float(rec["min"]), ref["min"], float(rec["max"]), ref["max"])
    assert int(rec["under"]) + int(np.asarray(rec["hist"]).sum()) + int(rec["over"]) == ref["count"] - ref["nonfinite"]
    assert abs(float(rec["sum"]) - ref["sum"]) <= n * U * ref["sumabs"], line
    assert abs(float(rec["sumsq"]) - ref["sumsq"]) <= n * U * ref["sumsq"], line


def values(n, seed, edges, f16=False):
    """n float32 values over many magnitudes with the special ones planted (as far as n allows): NaN, +-inf, +-0, denormals,
    and elements exactly equal to edges -- the first and the last included -- and their float32 neighbours."""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal(n) * 10.0 ** rs.uniform(-9, 3, n)).astype(np.float32)
    x[rs.uniform(size=n) < 0.3] = 0.0
    e = np.asarray(edges, np.float32)
    pick = e[[0, -1, len(e) // 2, 1, len(e) // 3, -2]] if len(e) >= 6 else e
    special = np.concatenate([np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-42, 1.4e-45], np.float32), pick,
                              np.nextafter(pick, np.float32(np.inf)), np.nextafter(pick, np.float32(-np.inf))]).astype(np.float32)
    if n >= 4:
        pos = rs.permutation(n)[:min(len(special), n // 2)]
        x[pos] = special[:len(pos)]
    if f16:
        with np.errstate(over="ignore"):
            x = x.astype(np.float16).astype(np.float32)       # (values beyond 65504 become inf: counted as non-finite)
    return x


SMALL = [0, 1, 63, 64, 65, 4097]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("bins", ["default", "one"])
def test_segments_of_any_length_and_alignment(dtype, bins):
    """Counts 0, 1, 63, 64, 65, 4097 as segments of one buffer in one call, each at starts that are not 16-byte aligned
    (element offsets 1, 2, 3 past a 64-element boundary, and 0); the gaps between the segments hold NaN, so a read outside
    a segment shows as a non-finite count."""
    f16 = dtype == torch.float16
    edges = summary.default_edges() if bins == "default" else np.array([-0.5, 0.25], np.float32)
    offs, cnts, o = [], [], 0
    for shift in (1, 0, 2, 3):
        for c in SMALL:
            o = (o + 63) // 64 * 64 + shift
            offs.append(o)
            cnts.append(c)
            o += c
    total = o + 64
    host = np.full(total, np.nan, np.float32)
    want = []
    for k, (off, c) in enumerate(zip(offs, cnts)):
        host[off:off + c] = values(c, 100 + k, edges, f16)
        want.append(ref_record(host[off:off + c], edges))
    flat = torch.from_numpy(host).to(DEV, dtype)
    rec = summary.decode(summary.tensor_stats(flat, offs, cnts, edges=edges).cpu(), len(edges) - 1)
    for k, w in enumerate(want):
        check(rec[k], w, "segment %d (offset %d, count %d)" % (k, offs[k], cnts[k]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_large_segment_beside_small_ones_and_repeatability(dtype):
    """2^25 + 5 elements from a 4-byte (2-byte) aligned start, a 16-element and a 1-element segment in the same call; the same
    call twice gives bitwise the same records."""
    f16 = dtype == torch.float16
    edges = summary.default_edges()
    n = 2 ** 25 + 5
    offs, cnts = [3, n + 64, n + 64 + 16 + 1], [n, 16, 1]
    host = np.full(n + 200, np.nan, np.float32)
    for k, (off, c) in enumerate(zip(offs, cnts)):
        host[off:off + c] = values(c, 7 + k, edges, f16)
    flat = torch.from_numpy(host).to(DEV, dtype)
    r1 = summary.tensor_stats(flat, offs, cnts).cpu()
    r2 = summary.tensor_stats(flat, offs, cnts).cpu()
    assert torch.equal(r1, r2), "two calls on the same data differ"
    rec = summary.decode(r1, len(edges) - 1)
    for k, (off, c) in enumerate(zip(offs, cnts)):
        check(rec[k], ref_record(host[off:off + c], edges), "segment %d (count %d)" % (k, c))


def test_trainer_layout_padding_is_not_counted():
    """A flat buffer laid out as the trainers lay theirs out (every variable padded to a multiple of 64 elements, starts
    256-byte aligned), the padding filled with NaN."""
    edges = summary.default_edges()
    shapes = [(16,), (3, 3, 16, 64), (64,), (1, 1, 64, 100), (100,), (4097,), (1,)]
    offs, cnts, o = [], [], 0
    for s in shapes:
        c = int(np.prod(s))
        offs.append(o)
        cnts.append(c)
        o += (c + 63) // 64 * 64
    host = np.full(o, np.nan, np.float32)
    rs = np.random.RandomState(3)
    for off, c in zip(offs, cnts):
        host[off:off + c] = (rs.standard_normal(c) * 0.05).astype(np.float32)
    flat = torch.from_numpy(host).to(DEV)
    rec = summary.decode(summary.tensor_stats(flat, offs, cnts).cpu(), len(edges) - 1)
    views = [flat[off:off + c].view(s) for off, c, s in zip(offs, cnts, shapes)]
    rec2 = summary.decode(summary.tensor_stats(views).cpu(), len(edges) - 1)              # the list form: one launch, same records
    for k, (off, c) in enumerate(zip(offs, cnts)):
        assert int(rec[k]["nonfinite"]) == 0
        check(rec[k], ref_record(host[off:off + c], edges), "variable %d" % k)
        assert rec[k].tobytes() == rec2[k].tobytes()


def test_list_of_tensors_from_several_buffers_and_rejected_calls():
    from squeezedet_amd._lib import SqdetError
    edges = summary.default_edges()
    rs = np.random.RandomState(9)
    a = torch.from_numpy(rs.standard_normal(1000).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rs.standard_normal((7, 33)).astype(np.float32)).to(DEV).half()
    c = a[100:357]
    rec = summary.decode(summary.tensor_stats([a, b, c]).cpu(), len(edges) - 1)
    for k, t in enumerate((a, b, c)):
        check(rec[k], ref_record(t.float().cpu().numpy().reshape(-1), edges), "tensor %d" % k)
    with pytest.raises(SqdetError):
        summary.tensor_stats(a, [990], [11])                          # leaves the buffer
    with pytest.raises(SqdetError):
        summary.tensor_stats(a, [0], [10], edges=np.array([1.0, 1.0], np.float32))
    with pytest.raises(SqdetError):
        summary.tensor_stats([a.cpu()])


def test_gradient_records_of_a_real_trainer():
    """One training step at the small shape of the training tests (2 x 128 x 256): the per-variable records of flat_grads equal
    NumPy on trainer.gview[n], and sqrt(sumsq) agrees with gview[n].double().norm().  Tolerance of the norm: sumsq carries
    at most n * 2^-53 * sumsq (the bound above), so sqrt(sumsq) carries at most half of n * 2^-53 * norm; torch's own float64
    reduction carries as much again; plus the two final roundings."""
    import squeezedet_amd as S
    from squeezedet_amd import nets, ops, synthetic
    from squeezedet_amd.train import SqueezeDetTrainer
    mc = S.kitti_squeezeDet_config_for_input(128, 256)
    mc.LOAD_PRETRAINED_MODEL, mc.IS_TRAINING, mc.BATCH_SIZE = False, True, 2
    m = nets.SqueezeDet(mc, gpu_id="0", dtype=torch.float32)
    m.load_params(synthetic.synthetic_params(m, seed=0))
    tr = SqueezeDetTrainer(m, seed=1)
    rs = np.random.RandomState(3)
    gt = np.stack([rs.uniform(0, 256, (2, 4)), rs.uniform(0, 128, (2, 4)), rs.uniform(20, 120, (2, 4)), rs.uniform(20, 90, (2, 4))], 2)
    cls, cnt = rs.randint(0, 3, (2, 4)).astype(np.int32), np.array([4, 2], np.int32)
    x = synthetic.synthetic_images(2, 128, 256, seed=9)
    out = tr.step(x, *ops.build_labels(mc.ANCHOR_BOX, gt, cls, cnt, 3, device=DEV)[:4], keep_activations=True)
    tr.flush()
    edges = summary.default_edges()
    ts = summary.TrainSummary(tr, "", write=False)
    ts.record(0, out, tr.learning_rate())
    ts.close()
    line = ts.last
    rec = summary.decode(summary.tensor_stats([tr.gview[n] for n in tr.names]).cpu(), len(edges) - 1)
    assert len(rec) == len(tr.names) > 40
    for k, n in enumerate(tr.names):
        g = tr.gview[n]
        w = ref_record(g.cpu().numpy().reshape(-1), edges)
        check(rec[k], w, n + "/gradients")
        norm = float(g.double().norm())
        tol = w["count"] * U * norm + 4 * np.spacing(norm)
        assert abs(math.sqrt(float(rec[k]["sumsq"])) - norm) <= tol, (n, math.sqrt(float(rec[k]["sumsq"])), norm, tol)
        # the summary line carries the same record, by the reference's names
        e = line["variables"][n + "/gradients"]
        assert e["count"] == g.numel() and e["sumsq"] == float(rec[k]["sumsq"]) and e["grad_norm"] == math.sqrt(e["sumsq"])
        assert e["clip_scale"] == mc.MAX_GRAD_NORM / max(e["grad_norm"], mc.MAX_GRAD_NORM)
        assert line["variables"][n]["count"] == tr.view[n].numel()
    for name, t in out["activations"].items():
        e = line["activations"]["activation_summary/" + name]
        a = t.float().cpu().numpy().reshape(-1)
        assert e["count"] == a.size and e["zeros"] == int((a == 0).sum()) and e["sparsity"] == e["zeros"] / e["count"]
        assert e["max"] == float(a.max()) and e["min"] == float(a.min())

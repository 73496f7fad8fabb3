"""The distillation terms (include/sqdet.h "distillation") restated in NumPy float64, one plain step after
the other, with the hand-derived gradient -- the reference of tests/test_distill_host.py and tests/test_gpu_distill.py -- and the
same forward in torch (any dtype) for float64 autograd and for the float32 evaluation whose own error sets the GPU tests' bound.

Channels of a cell's K*(C+5) values, as loss_kernel's: class logits at k*C + c, the confidence logit at K*C + k, the four deltas at
K*(C+1) + 4k + d.  Options: (temperature T, class_coef, conf_coef, bbox_coef, conf_floor).

`mutate` builds a deliberately WRONG variant, for the tests that show each mistake is caught by a named case:
  drop_T2          the class term without its T^2 (gradient c T w (p - q) / Bg -> c w (p - q) / (T Bg))
  student_weight   w from the student's confidence instead of the teacher's
  conf_no_A        the confidence term divided by Bg only, not Bg * A
  kl_reversed      KL(p || q) instead of KL(q || p)
  exclusive_floor  w = ct only where ct > conf_floor
"""
import numpy as np

MUTATIONS = ("drop_T2", "student_weight", "conf_no_A", "kl_reversed", "exclusive_floor")


def split(x, K, C):
    """preds [B,gh,gw,K*(C+5)] -> (class logits [B,A,C], confidence logits [B,A], deltas [B,A,4]) views' copies, A = gh*gw*K."""
    B = x.shape[0]
    v = x.reshape(B, -1, K * (C + 5))
    cells = v.shape[1]
    return (v[..., :K * C].reshape(B, cells * K, C), v[..., K * C:K * (C + 1)].reshape(B, cells * K),
            v[..., K * (C + 1):].reshape(B, cells * K, 4))


def join(gz, gu, gd, shape, K, C):
    """The inverse of split for gradients: [B,A,C], [B,A], [B,A,4] -> `shape`."""
    B = shape[0]
    cells = gz.shape[1] // K
    out = np.concatenate([gz.reshape(B, cells, K * C), gu.reshape(B, cells, K), gd.reshape(B, cells, K * 4)], axis=-1)
    return out.reshape(shape)


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return (z - m) - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def distill_reference64(student, teacher, K, C, opt, global_batch=0, mutate=None):
    """(terms [3] = class, conf, box; gradient w.r.t. the student's preds, the student's shape), float64.  student / teacher: arrays
    of any float dtype, evaluated on their stored values."""
    assert mutate is None or mutate in MUTATIONS
    T, c_cls, c_conf, c_box, floor = [float(v) for v in opt]
    s, t = np.asarray(student, np.float64), np.asarray(teacher, np.float64)
    zs, us, ds = split(s, K, C)
    zt, ut, dt = split(t, K, C)
    B, A = us.shape
    Bg = float(global_batch if global_batch > 0 else B)
    with np.errstate(over="ignore"):
        ct, cs = 1.0 / (1.0 + np.exp(-ut)), 1.0 / (1.0 + np.exp(-us))
    src = cs if mutate == "student_weight" else ct
    keep = src > floor if mutate == "exclusive_floor" else src >= floor
    w = np.where(keep, src, 0.0)
    # class term
    lq, lp = log_softmax(zt / T), log_softmax(zs / T)
    q, p = np.exp(lq), np.exp(lp)
    if mutate == "kl_reversed":
        kl = (p * (lp - lq)).sum(axis=-1)
        core = p * ((lp - lq) - kl[..., None])          # T * d KL(p || q) / d zs
    else:
        kl = (q * (lq - lp)).sum(axis=-1)
        core = p - q
    t2, t1 = (1.0, 1.0 / T) if mutate == "drop_T2" else (T * T, T)
    l_cls = c_cls * t2 * (w * kl).sum() / Bg
    gz = c_cls * t1 * w[..., None] * core / Bg
    # confidence term
    na = Bg if mutate == "conf_no_A" else Bg * A
    l_conf = c_conf * (ct * (ut - us) + softplus(us) - softplus(ut)).sum() / na
    gu = c_conf * (cs - ct) / na
    # box term
    diff = ds - dt
    l_box = c_box * (w * (diff * diff).sum(axis=-1)).sum() / Bg
    gd = 2.0 * c_box * w[..., None] * diff / Bg
    return np.array([l_cls, l_conf, l_box]), join(gz, gu, gd, s.shape, K, C)


def distill_forward_torch(student, teacher, K, C, opt, global_batch=0):
    """The three terms as torch scalars of student's dtype, differentiable in `student` (the weight and everything of the teacher are
    constants: the teacher tensor carries no gradient)."""
    import torch
    import torch.nn.functional as F
    T, c_cls, c_conf, c_box, floor = [float(v) for v in opt]
    B = student.shape[0]

    def parts(x):
        v = x.reshape(B, -1, K * (C + 5))
        cells = v.shape[1]
        return (v[..., :K * C].reshape(B, cells * K, C), v[..., K * C:K * (C + 1)].reshape(B, cells * K),
                v[..., K * (C + 1):].reshape(B, cells * K, 4))
    zs, us, ds = parts(student)
    zt, ut, dt = parts(teacher)
    A = us.shape[1]
    Bg = float(global_batch if global_batch > 0 else B)
    ct = torch.sigmoid(ut)
    w = torch.where(ct >= floor, ct, torch.zeros_like(ct)).detach()
    lq, lp = F.log_softmax(zt / T, dim=-1), F.log_softmax(zs / T, dim=-1)
    l_cls = c_cls * T * T * (w * (lq.exp() * (lq - lp)).sum(-1)).sum() / Bg
    l_conf = c_conf * (ct * (ut - us) + F.softplus(us) - F.softplus(ut)).sum() / (Bg * A)
    l_box = c_box * (w * ((ds - dt) ** 2).sum(-1)).sum() / Bg
    return l_cls, l_conf, l_box


def distill_autograd64(student, teacher, K, C, opt, global_batch=0):
    """(terms [3], gradient) by float64 autograd of distill_forward_torch."""
    import torch
    s = torch.tensor(np.asarray(student, np.float64), requires_grad=True)
    t = torch.tensor(np.asarray(teacher, np.float64))
    terms = distill_forward_torch(s, t, K, C, opt, global_batch)
    (terms[0] + terms[1] + terms[2]).backward()
    return np.array([float(v.detach()) for v in terms]), s.grad.numpy()


def distill_torch32(student, teacher, K, C, opt, global_batch=0):
    """(terms [3], gradient) of the float32 torch-CPU evaluation (forward and autograd in float32) on the stored values of student /
    teacher: the evaluation whose error against float64 is the GPU tests' e_ref."""
    import torch
    s = torch.tensor(np.asarray(student, np.float32), requires_grad=True)
    t = torch.tensor(np.asarray(teacher, np.float32))
    terms = distill_forward_torch(s, t, K, C, opt, global_batch)
    (terms[0] + terms[1] + terms[2]).backward()
    return np.array([float(v.detach()) for v in terms], np.float64), s.grad.numpy().astype(np.float64)

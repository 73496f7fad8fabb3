"""The loss with options (sqdet_loss_fwd_bwd_opt) restated on the CPU -- from the formulas of that
section and from the reference's lines (nn_skeleton.py:142-327), as loss_reference64 of tests/test_gpu_train_kernels.py is,
not from the kernel.  Nothing here touches the GPU or the library.

  loss_options_reference64   NumPy float64: losses [3], ious [B,A], dpreds.  The gradient is HAND-DERIVED (no autograd).
  loss_options_torch         the same forward in torch-CPU (float64 or float32), gradient by autograd.  In float64 it checks
                             the hand derivation; in float32 it plays the part the float32 oracle plays in the existing loss test:
                             its error against float64 is the yardstick e_ref of the kernel's.

TIE RULE (the kernel's, one rule for every min, max and clip): a coordinate of the prediction receives gradient through a min /
max / clip only where it is STRICTLY the selected argument; at equality the other argument -- the ground truth's coordinate,
the 0 of the intersection's max(0, .), the image border -- takes it.  An edge exactly on the border counts as clipped.
(`mutate="tie_swapped"` gives the prediction the gradient at equality instead: a mutation for the tests, as are the other
`mutate` values.)  torch's own choice at ties differs, which is why the compared cases stay 1e-3 px away from every tie.
"""
import numpy as np
import torch

BOX_LOSSES = ("delta_l2", "iou", "giou", "diou", "ciou")
MUTATIONS = ("no_clip_mask", "no_slope", "alpha_grad", "tie_swapped")
K4 = 4.0 / np.pi ** 2


def _unpack(mc, preds, mask, delta_in, box_in, labels, xp_from):
    p = xp_from(preds)
    B = p.shape[0]
    K, C, A = int(mc.ANCHOR_PER_GRID), int(mc.CLASSES), int(mc.ANCHORS)
    p = p.reshape(B, A // K, K * (C + 5))
    return (p, B, K, C, A, xp_from(mask).reshape(B, A), xp_from(delta_in).reshape(B, A, 4), xp_from(box_in).reshape(B, A, 4),
            xp_from(labels).reshape(B, A, C), xp_from(np.asarray(mc.ANCHOR_BOX).astype(np.float32)))


def decode64(mc, dl, anc):
    """float64 decode of deltas [..,4] on anchors: raw edges (before the clip) and the clipped '+1' corner form the IoU is formed on."""
    thr = float(np.float32(mc.EXP_THRESH))
    slope = float(np.exp(thr))
    sexp = lambda w: np.where(w > thr, slope * (w - thr + 1.0), np.exp(np.minimum(w, thr)))
    cx, cy = anc[:, 0] + dl[..., 0] * anc[:, 2], anc[:, 1] + dl[..., 1] * anc[:, 3]
    bw, bh = anc[:, 2] * sexp(dl[..., 2]), anc[:, 3] * sexp(dl[..., 3])
    w1, h1 = float(mc.IMAGE_WIDTH) - 1.0, float(mc.IMAGE_HEIGHT) - 1.0
    raw = [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]
    xmin, ymin, xmax, ymax = np.clip(raw[0], 0, w1), np.clip(raw[1], 0, h1), np.clip(raw[2], 0, w1), np.clip(raw[3], 0, h1)
    w2, h2 = xmax - xmin + 1.0, ymax - ymin + 1.0
    dcx, dcy = xmin + 0.5 * w2, ymin + 0.5 * h2
    return raw, [dcx - w2 / 2, dcy - h2 / 2, dcx + w2 / 2, dcy + h2 / 2]


def loss_options_reference64(mc, preds, mask, delta_in, box_in, labels, box_loss="delta_l2", gamma=0.0, global_batch=0, mutate=None):
    """losses [3] (class, conf, bbox), ious [B,A], dpreds (preds' shape): float64, gradient by hand."""
    assert box_loss in BOX_LOSSES and gamma >= 0 and mutate in (None,) + MUTATIONS
    f = lambda a: np.asarray(a, np.float64)
    p, B, K, C, A, m, dl_in, bx, lab, anc = _unpack(mc, preds, mask, delta_in, box_in, labels, f)
    eps = float(np.float32(mc.EPSILON))
    nobj = m.sum()
    Bmean = global_batch if global_batch > 0 else B
    dp = np.zeros_like(p)
    # ---- class term: softmax, focal factor, gradient through the softmax
    lg = p[..., :K * C].reshape(B, A, C)
    e = np.exp(lg - lg.max(axis=2, keepdims=True))
    pc = e / e.sum(axis=2, keepdims=True)
    lp, lq = -np.log(pc + eps), -np.log(1 - pc + eps)
    if gamma == 0:
        fc = lab * lp + (1 - lab) * lq
        dfc = -lab / (pc + eps) + (1 - lab) / (1 - pc + eps)
    else:
        q = 1 - pc
        with np.errstate(divide="ignore", invalid="ignore"):
            dqg = np.where(q > 0, gamma * q ** gamma / q, 0.0)          # d(b^g)/db, 0 at b == 0
            dpg = np.where(pc > 0, gamma * pc ** gamma / pc, 0.0)
        fc = lab * q ** gamma * lp + (1 - lab) * pc ** gamma * lq
        dfc = lab * (-dqg * lp - q ** gamma / (pc + eps)) + (1 - lab) * (dpg * lq + pc ** gamma / (1 - pc + eps))
    m3 = m[..., None]
    class_loss = (fc * m3 * mc.LOSS_COEF_CLASS).sum() / nobj
    gc = m3 * mc.LOSS_COEF_CLASS / nobj * dfc
    dp[..., :K * C] = (pc * (gc - (gc * pc).sum(axis=2, keepdims=True))).reshape(B, A // K, K * C)
    # ---- decode, IoU target, confidence term (the reference's)
    zc = p[..., K * C:K * C + K].reshape(B, A)
    conf = 1 / (1 + np.exp(-zc))
    dl = p[..., K * C + K:].reshape(B, A, 4)
    raw, a = decode64(mc, dl, anc)
    b = [bx[..., 0] - bx[..., 2] / 2, bx[..., 1] - bx[..., 3] / 2, bx[..., 0] + bx[..., 2] / 2, bx[..., 1] + bx[..., 3] / 2]
    iwr, ihr = np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]), np.minimum(a[3], b[3]) - np.maximum(a[1], b[1])
    iw, ih = np.maximum(iwr, 0), np.maximum(ihr, 0)
    inter = iw * ih
    pw, ph, gw, gh = a[2] - a[0], a[3] - a[1], b[2] - b[0], b[3] - b[1]
    uni = pw * ph + gw * gh - inter
    iou1 = inter / (uni + eps)
    ious = iou1 * m
    wgt = m * mc.LOSS_COEF_CONF_POS / nobj + (1 - m) * mc.LOSS_COEF_CONF_NEG / (A - nobj)
    conf_loss = (((ious - conf) ** 2) * wgt).sum() / Bmean
    dp[..., K * C:K * C + K] = (2 * (conf - ious) * wgt / Bmean * conf * (1 - conf)).reshape(B, A // K, K)
    # ---- box term
    coef = float(mc.LOSS_COEF_BBOX)
    if box_loss == "delta_l2":
        df = m3 * (dl - dl_in)
        bbox_loss = (coef * df ** 2).sum() / nobj
        ddl = 2 * coef * m3 * df / nobj
    else:
        pos = m != 0
        swapped = mutate == "tie_swapped"
        gt_, lt_ = (np.greater_equal, np.less_equal) if swapped else (np.greater, np.less)       # "is the selected argument"
        fx, fy = gt_(iwr, 0) * 1.0, gt_(ihr, 0) * 1.0
        # corner order x0, y0, x1, y1
        di = [-(gt_(a[0], b[0]) * fx) * ih, -(gt_(a[1], b[1]) * fy) * iw, (lt_(a[2], b[2]) * fx) * ih, (lt_(a[3], b[3]) * fy) * iw]
        da = [-ph, -pw, ph, pw]
        ue = uni + eps
        du = [da[j] - di[j] for j in range(4)]
        X = iou1.copy()
        dX = [(di[j] - iou1 * du[j]) / ue for j in range(4)]
        if box_loss != "iou":
            Cw, Ch = np.maximum(a[2], b[2]) - np.minimum(a[0], b[0]), np.maximum(a[3], b[3]) - np.minimum(a[1], b[1])
            s = [-1.0 * lt_(a[0], b[0]), -1.0 * lt_(a[1], b[1]), 1.0 * gt_(a[2], b[2]), 1.0 * gt_(a[3], b[3])]
            if box_loss == "giou":
                Ca = Cw * Ch
                T = (Ca - uni) / (Ca + eps)
                dC = [s[0] * Ch, s[1] * Cw, s[2] * Ch, s[3] * Cw]
                X = X - T
                dX = [dX[j] - ((dC[j] - du[j]) - T * dC[j]) / (Ca + eps) for j in range(4)]
            else:
                c2e = Cw ** 2 + Ch ** 2 + eps
                ex, ey = (a[0] + a[2]) / 2 - (b[0] + b[2]) / 2, (a[1] + a[3]) / 2 - (b[1] + b[3]) / 2
                D = (ex ** 2 + ey ** 2) / c2e
                dr = [ex, ey, ex, ey]
                dc2 = [2 * Cw * s[0], 2 * Ch * s[1], 2 * Cw * s[2], 2 * Ch * s[3]]
                X = X - D
                dX = [dX[j] - (dr[j] - D * dc2[j]) / c2e for j in range(4)]
                if box_loss == "ciou":
                    with np.errstate(divide="ignore", invalid="ignore"):
                        dat = np.where(pos, np.arctan(gw / np.where(pos, gh, 1.0)) - np.arctan(pw / ph), 0.0)
                    v = K4 * dat ** 2
                    den = 1 - iou1 + v + eps
                    alpha = v / den
                    s2 = pw ** 2 + ph ** 2
                    vw, vh = -2 * K4 * dat * ph / s2, 2 * K4 * dat * pw / s2
                    dv = [-vw, -vh, vw, vh]
                    X = X - alpha * v
                    dX = [dX[j] - alpha * dv[j] for j in range(4)]
                    if mutate == "alpha_grad":            # d(alpha * v) with alpha = v / (1 - IoU + v + eps) differentiated too
                        diou = [(di[j] - iou1 * du[j]) / ue for j in range(4)]
                        dX = [dX[j] - v * (dv[j] * den - v * (dv[j] - diou[j])) / den ** 2 for j in range(4)]
        sc = np.where(pos, coef * m / nobj, 0.0)
        bbox_loss = (sc * np.where(pos, 1 - X, 0.0)).sum()
        w1, h1 = float(mc.IMAGE_WIDTH) - 1.0, float(mc.IMAGE_HEIGHT) - 1.0
        hi = [w1, h1, w1, h1]
        g = []
        for j in range(4):
            inside = np.ones_like(m) if mutate == "no_clip_mask" else (gt_(raw[j], 0) & lt_(raw[j], hi[j])) * 1.0
            g.append(np.where(pos, -sc * dX[j] * inside, 0.0))
        thr = float(np.float32(mc.EXP_THRESH))
        slope = float(np.exp(thr))
        dexp = lambda w: np.exp(w) if mutate == "no_slope" else np.where(w > thr, slope, np.exp(np.minimum(w, thr)))
        ddl = np.stack([anc[:, 2] * (g[0] + g[2]), anc[:, 3] * (g[1] + g[3]),
                        0.5 * anc[:, 2] * dexp(dl[..., 2]) * (g[2] - g[0]), 0.5 * anc[:, 3] * dexp(dl[..., 3]) * (g[3] - g[1])], axis=-1)
    dp[..., K * C + K:] = ddl.reshape(B, A // K, 4 * K)
    return np.array([class_loss, conf_loss, bbox_loss]), ious, dp.reshape(np.asarray(preds).shape)


def box_measures64(a, b, eps=1e-16):
    """(iou, giou, diou, ciou) of corner boxes a, b (lists of four arrays), float64: the X of each kind, for the ordering test."""
    iw = np.maximum(np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]), 0)
    ih = np.maximum(np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]), 0)
    inter = iw * ih
    pw, ph, gw, gh = a[2] - a[0], a[3] - a[1], b[2] - b[0], b[3] - b[1]
    uni = pw * ph + gw * gh - inter
    iou = inter / (uni + eps)
    Cw, Ch = np.maximum(a[2], b[2]) - np.minimum(a[0], b[0]), np.maximum(a[3], b[3]) - np.minimum(a[1], b[1])
    giou = iou - (Cw * Ch - uni) / (Cw * Ch + eps)
    rho2 = ((a[0] + a[2]) / 2 - (b[0] + b[2]) / 2) ** 2 + ((a[1] + a[3]) / 2 - (b[1] + b[3]) / 2) ** 2
    diou = iou - rho2 / (Cw ** 2 + Ch ** 2 + eps)
    v = K4 * (np.arctan(gw / gh) - np.arctan(pw / ph)) ** 2
    return iou, giou, diou, diou - v / (1 - iou + v + eps) * v


def loss_options_torch(mc, preds, mask, delta_in, box_in, labels, box_loss="delta_l2", gamma=0.0, global_batch=0, dtype=torch.float64):
    """The same forward in torch-CPU `dtype`; dpreds by autograd (alpha detached, ious without gradient).  Returns float64 arrays."""
    assert box_loss in BOX_LOSSES
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype)
    p0 = t(preds).requires_grad_(True)
    p, B, K, C, A, m, dl_in, bx, lab, anc = _unpack(mc, p0, mask, delta_in, box_in, labels, lambda a: a if isinstance(a, torch.Tensor) else t(a))
    eps = float(np.float32(mc.EPSILON))
    nobj = m.sum()
    Bmean = global_batch if global_batch > 0 else B
    pc = torch.softmax(p[..., :K * C].reshape(B, A, C), dim=2)
    conf = torch.sigmoid(p[..., K * C:K * C + K].reshape(B, A))
    dl = p[..., K * C + K:].reshape(B, A, 4)
    thr = float(np.float32(mc.EXP_THRESH))
    slope = float(np.exp(thr))
    sexp = lambda w: torch.where(w > thr, slope * (w - thr + 1.0), torch.exp(torch.clamp(w, max=thr)))
    cx, cy = anc[:, 0] + dl[..., 0] * anc[:, 2], anc[:, 1] + dl[..., 1] * anc[:, 3]
    bw, bh = anc[:, 2] * sexp(dl[..., 2]), anc[:, 3] * sexp(dl[..., 3])
    w1, h1 = float(mc.IMAGE_WIDTH) - 1.0, float(mc.IMAGE_HEIGHT) - 1.0
    xmin, ymin = torch.clamp(cx - bw / 2, 0.0, w1), torch.clamp(cy - bh / 2, 0.0, h1)
    xmax, ymax = torch.clamp(cx + bw / 2, 0.0, w1), torch.clamp(cy + bh / 2, 0.0, h1)
    w2, h2 = xmax - xmin + 1.0, ymax - ymin + 1.0
    dcx, dcy = xmin + 0.5 * w2, ymin + 0.5 * h2
    a = [dcx - w2 / 2, dcy - h2 / 2, dcx + w2 / 2, dcy + h2 / 2]
    b = [bx[..., 0] - bx[..., 2] / 2, bx[..., 1] - bx[..., 3] / 2, bx[..., 0] + bx[..., 2] / 2, bx[..., 1] + bx[..., 3] / 2]
    iw = torch.clamp(torch.minimum(a[2], b[2]) - torch.maximum(a[0], b[0]), min=0.0)
    ih = torch.clamp(torch.minimum(a[3], b[3]) - torch.maximum(a[1], b[1]), min=0.0)
    inter = iw * ih
    pw, ph, gw, gh = a[2] - a[0], a[3] - a[1], b[2] - b[0], b[3] - b[1]
    uni = pw * ph + gw * gh - inter
    iou1 = inter / (uni + eps)
    ious = (iou1 * m).detach()
    m3 = m.reshape(B, A, 1)
    lp, lq = -torch.log(pc + eps), -torch.log(1 - pc + eps)
    if gamma == 0:
        fc = lab * lp + (1 - lab) * lq
    else:
        # b^g with the derivative g * b^g / b, and 0 at b == 0 (autograd's own 0^(g-1) * 0 there is NaN for g < 1)
        one, zero = torch.ones_like(pc), torch.zeros_like(pc)
        powg = lambda b: torch.where(b > 0, torch.where(b > 0, b, one) ** gamma, zero)
        fc = lab * powg(1 - pc) * lp + (1 - lab) * powg(pc) * lq
    class_loss = (fc * m3 * mc.LOSS_COEF_CLASS).sum() / nobj
    conf_loss = (((ious - conf) ** 2) * (m * mc.LOSS_COEF_CONF_POS / nobj + (1 - m) * mc.LOSS_COEF_CONF_NEG / (A - nobj))).sum() / Bmean
    if box_loss == "delta_l2":
        bbox_loss = (mc.LOSS_COEF_BBOX * (m3 * (dl - dl_in)) ** 2).sum() / nobj
    else:
        X = iou1
        if box_loss != "iou":
            Cw, Ch = torch.maximum(a[2], b[2]) - torch.minimum(a[0], b[0]), torch.maximum(a[3], b[3]) - torch.minimum(a[1], b[1])
            if box_loss == "giou":
                X = X - (Cw * Ch - uni) / (Cw * Ch + eps)
            else:
                ex, ey = (a[0] + a[2]) / 2 - (b[0] + b[2]) / 2, (a[1] + a[3]) / 2 - (b[1] + b[3]) / 2
                X = X - (ex ** 2 + ey ** 2) / (Cw ** 2 + Ch ** 2 + eps)
                if box_loss == "ciou":
                    pos = m != 0
                    one = torch.ones_like(gh)
                    v = K4 * (torch.atan(torch.where(pos, gw, one) / torch.where(pos, gh, one)) - torch.atan(pw / ph)) ** 2
                    alpha = (v / (1 - iou1 + v + eps)).detach()
                    X = X - alpha * v
        pos = m != 0
        bbox_loss = (torch.where(pos, mc.LOSS_COEF_BBOX * m * (1 - X), torch.zeros_like(X))).sum() / nobj
    (dp,) = torch.autograd.grad(class_loss + conf_loss + bbox_loss, p0)
    return (np.array([class_loss.item(), conf_loss.item(), bbox_loss.item()], np.float64), ious.numpy().astype(np.float64),
            dp.numpy().astype(np.float64))

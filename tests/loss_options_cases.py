"""Seeded inputs of the loss-with-options tests (tests/test_loss_options_host.py, tests/test_gpu_loss_options.py).

Small cases: grids of 2 x 3 and 3 x 5 cells on a 320 x 160 input, K = 1 and 9 anchors per cell, C = 1, 3 and 20 classes, B = 1
and 3, each with A > num_objects >= 1; one case at the full KITTI grid (24 x 78 x 9 anchors) with B = 8, where the kernel's
grid-stride loop and several laps of loss_finish_kernel run.  The positive anchors of EVERY case include five planted ones
that between them are every situation the box losses' gradient distinguishes:

  P1  clipped at the LEFT and the TOP border, CONTAINS its ground truth, width delta above EXP_THRESH (safe_exp's linear branch)
  P2  clipped at the RIGHT and the BOTTOM border, CONTAINED in its ground truth, height delta above EXP_THRESH
  P3  DISJOINT from its ground truth (IoU 0: only the GIoU / DIoU / CIoU penalties carry gradient)
  P4  partly OVERLAPPING its ground truth
  P5  EQUAL to its ground truth to within a pixel (offsets of 0.2 .. 0.4 px per edge)

(five anchors, because the smallest case has A = 6), plus -- where there is room -- random positives.  Every compared pair of
coordinates of a positive anchor (corner against corner, intersection side against 0, raw edge against either border, width /
height delta against EXP_THRESH) is at least MIN_SEPARATION = 1e-3 apart, by rejection in the generator; `min_separation`
measures it and the host test asserts it for every case, so no compared gradient sits on a kink and no anchor is excluded.

`tie_case()` is the one case ON ties, built of small integers so that the ties are exact in float32 and float64 alike.
"""
import numpy as np

from squeezedet_amd import config as CFG

from tests.loss_options_reference import decode64

MIN_SEPARATION = 1e-3
SMALL_IMAGE = (160, 320)         # H, W

# name: (grid h, grid w, K, C, B, number of random positives beside the five planted)
CASES = {
    "g2x3_k1_c3_b1": (2, 3, 1, 3, 1, 0),            # A = 6, five positives
    "g2x3_k9_c1_b3": (2, 3, 9, 1, 3, 6),
    "g3x5_k1_c20_b3": (3, 5, 1, 20, 3, 4),          # A = 15, nine positives
    "g3x5_k9_c3_b1": (3, 5, 9, 3, 1, 7),
    "g3x5_k9_c20_b3": (3, 5, 9, 20, 3, 9),
    "kitti_b8": (24, 78, 9, 3, 8, 40),
}
SMALL_CASES = [n for n in CASES if n != "kitti_b8"]


def case_config(gh, gw, K, C, full=False):
    mc = CFG.kitti_squeezeDet_config()
    if not full:
        mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH = SMALL_IMAGE
        shapes = CFG.SQUEEZEDET_ANCHOR_SHAPES * 0.2 if K == 9 else np.array([[60.0, 40.0]])
        mc.ANCHOR_BOX = CFG.set_anchors(mc, gh, gw, shapes)
        mc.ANCHORS = len(mc.ANCHOR_BOX)
        mc.ANCHOR_PER_GRID = K
    mc.CLASSES = C
    assert mc.ANCHORS == gh * gw * K and mc.ANCHOR_PER_GRID == K
    return mc


def _deltas_for(mc, anc, raw):
    """The float32 deltas whose decode on anchor `anc` has the raw (unclipped) edges `raw` = (x0, y0, x1, y1)."""
    thr = float(np.float32(mc.EXP_THRESH))
    inv = lambda r: np.log(r) if r <= np.exp(thr) else r / np.exp(thr) - 1.0 + thr         # safe_exp's inverse
    bw, bh = raw[2] - raw[0], raw[3] - raw[1]
    return np.array([((raw[0] + raw[2]) / 2 - anc[0]) / anc[2], ((raw[1] + raw[3]) / 2 - anc[1]) / anc[3], inv(bw / anc[2]), inv(bh / anc[3])],
                    np.float32)


def _cxcywh(c):
    return np.array([(c[0] + c[2]) / 2, (c[1] + c[3]) / 2, c[2] - c[0], c[3] - c[1]], np.float32)


def _corners_of(mc, anc, d):
    raw, a = decode64(mc, np.asarray(d, np.float64)[None], np.asarray(anc, np.float64)[None])
    return [float(v[0]) for v in raw], [float(v[0]) for v in a]


def _planted(kind, mc, anc, rs):
    """(float32 deltas, float32 ground-truth box (cx, cy, w, h)) of planted positive `kind` on anchor `anc`."""
    w1, h1 = mc.IMAGE_WIDTH - 1.0, mc.IMAGE_HEIGHT - 1.0
    aw, ah = anc[2], anc[3]
    u = lambda lo, hi: float(rs.uniform(lo, hi))
    if kind == "P1":
        bw, bh = aw * u(3.0, 3.4), ah * u(1.2, 1.6)
        x0, y0 = -u(.1, .3) * bw, -u(.1, .3) * bh
        d = _deltas_for(mc, anc, (x0, y0, x0 + bw, y0 + bh))
    elif kind == "P2":
        bw, bh = aw * u(0.7, 0.9), ah * u(3.0, 3.3)
        x1, y1 = w1 + u(.2, .4) * bw, h1 + u(.2, .4) * bh
        d = _deltas_for(mc, anc, (x1 - bw, y1 - bh, x1, y1))
    else:
        d = np.array([u(-.2, .2), u(-.2, .2), u(-.3, .3), u(-.3, .3)], np.float32)
    _, a = _corners_of(mc, anc, d)
    pw, ph = a[2] - a[0], a[3] - a[1]
    if kind == "P1":
        g = (a[0] + u(.3, .45) * pw, a[1] + u(.15, .25) * ph, a[0] + u(.55, .7) * pw, a[1] + u(.75, .85) * ph)      # (another aspect ratio: CIoU's v)
    elif kind == "P2":
        g = (a[0] - u(4, 9), a[1] - u(4, 9), a[2] + u(4, 9), a[3] + u(4, 9))
    elif kind == "P3":
        g = (a[2] + u(5, 15), a[3] + u(4, 12), a[2] + u(5, 15) + pw * u(.8, 1.2) + 15, a[3] + u(4, 12) + ph * u(.8, 1.2) + 12)
    elif kind == "P4":
        sx, sy = u(.25, .4) * pw, -u(.2, .35) * ph
        g = (a[0] + sx, a[1] + sy, a[2] + sx + u(2, 6), a[1] + sy + ph * u(1.4, 1.7))
    else:                                          # P5
        g = (a[0] + u(.2, .4), a[1] - u(.2, .4), a[2] - u(.2, .4), a[3] + u(.2, .4))
    return d, _cxcywh(g)


def _random_positive(mc, anc, rs):
    d = (rs.randn(4) * 0.4).astype(np.float32)
    box = anc * np.array([1, 1, 0, 0]) + anc[[2, 3, 2, 3]] * np.array([rs.uniform(-.3, .3), rs.uniform(-.3, .3), rs.uniform(.6, 1.5), rs.uniform(.6, 1.5)])
    return d, box.astype(np.float32)


def pair_separation(mc, anc, d, box):
    """The smallest distance of any compared pair of one positive anchor: float32 inputs, float64 arithmetic."""
    raw, a = _corners_of(mc, np.asarray(anc, np.float32), d)
    bx = np.asarray(box, np.float64)
    b = [bx[0] - bx[2] / 2, bx[1] - bx[3] / 2, bx[0] + bx[2] / 2, bx[1] + bx[3] / 2]
    w1, h1 = mc.IMAGE_WIDTH - 1.0, mc.IMAGE_HEIGHT - 1.0
    thr = float(np.float32(mc.EXP_THRESH))
    gaps = [abs(a[j] - b[j]) for j in range(4)]
    gaps += [abs(min(a[2], b[2]) - max(a[0], b[0])), abs(min(a[3], b[3]) - max(a[1], b[1]))]
    gaps += [abs(raw[0]), abs(raw[0] - w1), abs(raw[2]), abs(raw[2] - w1), abs(raw[1]), abs(raw[1] - h1), abs(raw[3]), abs(raw[3] - h1)]
    gaps += [abs(float(d[2]) - thr), abs(float(d[3]) - thr)]
    return min(gaps)


def loss_case(name):
    """(mc, preds [B,gh,gw,K*(C+5)] float32, mask [B,A,1], delta [B,A,4], box [B,A,4], labels [B,A,C], planted {kind: (b, a)})."""
    gh, gw, K, C, B, extra = CASES[name]
    mc = case_config(gh, gw, K, C, full=(name == "kitti_b8"))
    A = mc.ANCHORS
    rs = np.random.RandomState(sum(map(ord, name)) + 7)
    preds = (rs.randn(B, gh, gw, K * (C + 5)) * 1.2).astype(np.float32)
    anchors = np.asarray(mc.ANCHOR_BOX).astype(np.float32)
    mask, delta = np.zeros((B, A, 1), np.float32), np.zeros((B, A, 4), np.float32)
    box, labels = np.zeros((B, A, 4), np.float32), np.zeros((B, A, C), np.float32)
    pv = preds.reshape(B, A // K, K * (C + 5))
    kinds = ["P1", "P2", "P3", "P4", "P5"] + ["R"] * extra
    assert len(kinds) < A
    # (P1 / P2 need an anchor whose box, 3.4 times as wide / 3.3 times as high, still has its far edge inside the image)
    fits = {"P1": lambda an: an[2] * 3.4 < mc.IMAGE_WIDTH - 1.0 and an[3] * 1.6 < mc.IMAGE_HEIGHT - 1.0,
            "P2": lambda an: an[3] * 3.3 * 0.8 < mc.IMAGE_HEIGHT - 1.0}
    used = set()
    planted = {}
    for kind in kinds:
        while True:
            s = int(rs.randint(B * A))
            if s not in used and fits.get(kind, lambda an: True)(anchors[s % A]):
                break
        used.add(s)
        b, a = int(s // A), int(s % A)
        for _ in range(1000):
            d, g = _planted(kind, mc, anchors[a], rs) if kind != "R" else _random_positive(mc, anchors[a], rs)
            if pair_separation(mc, anchors[a], d, g) >= 2 * MIN_SEPARATION:
                break
        else:
            raise AssertionError("%s: no separated draw for %s" % (name, kind))
        mask[b, a, 0] = 1.0
        pv[b, a // K, K * (C + 1) + 4 * (a % K):K * (C + 1) + 4 * (a % K) + 4] = d
        box[b, a] = g
        delta[b, a] = rs.randn(4) * 0.4
        labels[b, a, rs.randint(C)] = 1.0
        if kind != "R":
            planted[kind] = (b, a)
    return mc, preds, mask, delta, box, labels, planted


def positives(mc, preds, mask, box):
    """[(b, a, anchor, float32 deltas, float32 box)] of the positive anchors."""
    B = preds.shape[0]
    K, C, A = mc.ANCHOR_PER_GRID, mc.CLASSES, mc.ANCHORS
    pv = preds.reshape(B, A // K, K * (C + 5))
    anchors = np.asarray(mc.ANCHOR_BOX).astype(np.float32)
    return [(b, a, anchors[a], pv[b, a // K, K * (C + 1) + 4 * (a % K):K * (C + 1) + 4 * (a % K) + 4], box[b, a])
            for b, a in np.argwhere(mask[..., 0] > 0)]


def min_separation(mc, preds, mask, box):
    return min(pair_separation(mc, anc, d, g) for _, _, anc, d, g in positives(mc, preds, mask, box))


# ---------------------------------------------------------------- the case on ties
TIE_ANCHORS = np.array([[64, 32, 40, 20],       # T1: the prediction IS its ground truth (all four corners tie)
                        [20, 64, 40, 20],       # T2: raw left edge exactly 0
                        [235, 10, 40, 20],      # T3: raw right edge exactly w1 = 255 and raw top edge exactly 0
                        [128, 117, 40, 20],     # T4: raw bottom edge exactly h1 = 127
                        [128, 64, 40, 20],      # T5: width delta exactly EXP_THRESH (the exp branch: `>` selects the line)
                        [200, 64, 40, 20]], np.float64)   # (unlabelled)


def tie_case():
    """(mc, preds, mask, delta, box, labels): 256 x 128 input, 2 x 3 cells, K = 1, C = 3, B = 1, all deltas 0 but T5's."""
    mc = CFG.kitti_squeezeDet_config()
    mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH = 128, 256
    mc.ANCHOR_BOX, mc.ANCHORS, mc.ANCHOR_PER_GRID, mc.CLASSES = TIE_ANCHORS.copy(), 6, 1, 3
    rs = np.random.RandomState(5)
    preds = (rs.randn(1, 2, 3, 8) * 1.2).astype(np.float32)
    preds[..., 4:] = 0.0
    preds.reshape(6, 8)[4, 6] = np.float32(mc.EXP_THRESH)
    mask, delta = np.zeros((1, 6, 1), np.float32), (rs.randn(1, 6, 4) * 0.4).astype(np.float32)
    box, labels = np.zeros((1, 6, 4), np.float32), np.zeros((1, 6, 3), np.float32)
    mask[0, :5, 0] = 1.0
    labels[0, np.arange(5), rs.randint(3, size=5)] = 1.0
    box[0, 0] = [64.5, 32.5, 41, 21]                 # corners (44, 22, 85, 43): the decoded box of T1
    for a in range(1, 5):                            # an overlapping ground truth off every tie
        box[0, a] = TIE_ANCHORS[a] + np.array([3.25, -2.75, 5.5, 3.5])
    delta[0, 5] = 0.0
    return mc, preds, mask, delta, box, labels

"""Seeded inputs of the distillation tests (tests/test_distill_host.py, tests/test_gpu_distill.py).

The grid sizes are those of tests/loss_options_cases.py: 2 x 3 and 3 x 5 cells, K = 1 and 9 anchors per cell, C = 1, 3 and 20
classes, B = 1 and 3; one case at the full KITTI grid (24 x 78 x 9 anchors, C = 3) with B = 2, where the kernel's grid-stride loop
(132 workgroups of 256 anchors) and three laps of loss_finish_kernel run.  Student and teacher preds are float32 draws of std 1.2
(the teacher's partly correlated with the student's, as a trained pair's would be) whose values are exactly representable in float16, so
that every dtype pair of the GPU tests evaluates the same numbers.  Between them the cases' options cover T in {0.5, 1, 2, 4},
floors 0, 0.3, 0.5 and 0.6, and a zero coefficient in each position.

Every anchor's teacher confidence is at least MIN_SEPARATION = 1e-3 away from its case's floor, by rejection in the generator;
`floor_separation` measures it and the host test asserts it, so no compared value sits on the floor's step.  `tie_case()` is the
one case ON the floor: confidence logits of exactly 0 under a floor of 0.5.
"""
import numpy as np

MIN_SEPARATION = 1e-3

# name: (grid h, grid w, K, C, B, (T, class_coef, conf_coef, bbox_coef, conf_floor))
CASES = {
    "g2x3_k1_c3_b1": (2, 3, 1, 3, 1, (1.0, 1.0, 1.0, 1.0, 0.0)),            # the defaults
    "g2x3_k9_c1_b3": (2, 3, 9, 1, 3, (2.0, 1.0, 0.5, 2.0, 0.3)),            # C = 1: no class term
    "g3x5_k1_c20_b3": (3, 5, 1, 20, 3, (4.0, 0.7, 0.0, 1.5, 0.5)),          # no confidence term
    "g3x5_k9_c3_b1": (3, 5, 9, 3, 1, (0.5, 2.0, 1.0, 0.0, 0.6)),            # no box term
    "g3x5_k9_c20_b3": (3, 5, 9, 20, 3, (2.0, 0.0, 3.0, 1.0, 0.3)),          # no class term by its coefficient
    "kitti_b2": (24, 78, 9, 3, 2, (4.0, 1.0, 1.0, 1.0, 0.5)),
}
SMALL_CASES = [n for n in CASES if n != "kitti_b2"]


def _f16_exact(a):
    return a.astype(np.float16).astype(np.float32)


def sigmoid64(u):
    return 1.0 / (1.0 + np.exp(-np.asarray(u, np.float64)))


def conf_logits(x, K, C):
    """The confidence logits [B, cells, K] of preds x (a view)."""
    return x.reshape(x.shape[0], -1, K * (C + 5))[..., K * C:K * (C + 1)]


def floor_separation(teacher, K, C, floor):
    """The smallest distance of any anchor's teacher confidence from the floor (float64 on the stored values)."""
    return float(np.abs(sigmoid64(conf_logits(teacher, K, C)) - floor).min())


def distill_case(name):
    """(K, C, student preds, teacher preds [B,gh,gw,K*(C+5)] float32, options)."""
    gh, gw, K, C, B, opt = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 20)
    shape = (B, gh, gw, K * (C + 5))
    student = _f16_exact((rs.randn(*shape) * 1.2).astype(np.float32))
    teacher = _f16_exact((0.6 * student + rs.randn(*shape) * 1.0).astype(np.float32))
    ut = conf_logits(teacher, K, C)
    for _ in range(100):                       # redraw the confidence logits that sit near the floor's step
        near = np.abs(sigmoid64(ut) - opt[4]) < 4 * MIN_SEPARATION
        if not near.any():
            break
        ut[near] = _f16_exact((rs.randn(int(near.sum())) * 1.2).astype(np.float32))
    else:
        raise AssertionError("%s: no separated draw" % name)
    return K, C, student, teacher, opt


def tie_case():
    """(K, C, student, teacher, options): 2 x 3 cells, K = 1, C = 3, B = 1, conf_floor 0.5.  Anchors 0 and 1 have a teacher confidence
    logit of exactly 0 -- sigmoid(0) = 0.5 in every precision: ON the floor, kept (inclusive) with weight 0.5; anchor 2 lies below the
    floor (logit -1), the others above it."""
    K, C = 1, 3
    rs = np.random.RandomState(11)
    student = _f16_exact((rs.randn(1, 2, 3, 8) * 1.2).astype(np.float32))
    teacher = _f16_exact((rs.randn(1, 2, 3, 8) * 1.2).astype(np.float32))
    conf_logits(teacher, K, C)[0, :, 0] = [0.0, 0.0, -1.0, 0.5, 1.0, 2.0]
    return K, C, student, teacher, (1.0, 1.0, 1.0, 1.0, 0.5)


def extreme_case():
    """(K, C, student, teacher, options): class logits of +-60000 at T = 0.5 (finite in float16: the largest is 65504), confidence
    logits of +-30 and +-60000, on 2 x 3 cells, K = 1, C = 3."""
    K, C = 1, 3
    student, teacher = np.zeros((1, 2, 3, 8), np.float32), np.zeros((1, 2, 3, 8), np.float32)
    s, t = student.reshape(6, 8), teacher.reshape(6, 8)
    s[:, :3] = [[60000, -60000, 0], [-60000, 60000, 0], [60000, 60000, -60000], [0, 0, 0], [-60000, 0, 60000], [1, 2, 3]]
    t[:, :3] = [[-60000, 60000, 0], [-60000, 60000, 0], [0, 0, 0], [60000, -60000, 60000], [60000, 0, -60000], [3, 2, 1]]
    s[:, 3] = [30, -30, 60000, -60000, 0, 1]
    t[:, 3] = [-30, 30, 60000, 60000, -60000, 2]
    s[:, 4:] = np.arange(24).reshape(6, 4) * 0.25
    t[:, 4:] = 1.0
    return K, C, student, teacher, (0.5, 1.0, 1.0, 1.0, 0.0)

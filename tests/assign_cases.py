"""Small inputs of sqdet_build_labels_opt (squeezedet_amd/csrc/assign.hip), each named after the branch it reaches (test
infrastructure, no GPU).  Shared by tests/test_assign_host.py, which shows on the NumPy restatement alone that every case reaches
its branch and that every tie rule decides at least one case, and by tests/test_gpu_assign.py (the kernel against the restatement
on all of them, under both modes).

The tables are the dyadic ones of tests/input_path_cases.py: on them IoUs and squared distances are exact in float64, so ties
really occur; on S2 (S twice) every value ties between anchor a and a + 273.  `kitti` is the real table (16 848 anchors, 9 per
cell) with two images of about 20 boxes, the density of a mosaic."""
import collections
import functools

import numpy as np

from tests import assign_reference as R
from tests import input_path_cases as IC

AssignCase = collections.namedtuple("AssignCase", "name label apg iou_thresh max_per_box topk")
MODES = ("iou", "atss")
ASSIGN_CASES = ["identical", "boundary", "cap_tie", "k1", "all_candidates", "far", "zero_width", "edge", "variance", "empty", "counts",
                "classes1", "classes20", "apg1", "three", "one", "kitti", "over_cap"]
STAGE_CAP = 4096                 # assign.hip ASSIGN_STAGE_CAP: what assign_describe_kernel stages in LDS per box


def _lattice(rs, n):
    """Boxes with centres and sizes on multiples of 16 inside S's 448 x 256 extent."""
    return np.stack([16.0 * rs.randint(2, 27, n), 16.0 * rs.randint(2, 15, n), 16.0 * rs.randint(1, 8, n), 16.0 * rs.randint(1, 8, n)], 1)


@functools.lru_cache(maxsize=None)
def kitti_table():
    from squeezedet_amd.config import kitti_squeezeDet_config
    mc = kitti_squeezeDet_config()
    t = np.ascontiguousarray(np.asarray(mc.ANCHOR_BOX, np.float64))
    assert t.shape == (16848, 4) and int(mc.ANCHOR_PER_GRID) == 9
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def assign_case(name):
    rs = np.random.RandomState(ASSIGN_CASES.index(name) + 301)
    S, S2 = IC.table("S"), IC.table("S2")
    case = lambda label, apg=3, iou_thresh=0.5, max_per_box=16, topk=9: AssignCase(name, label, apg, iou_thresh, max_per_box, topk)
    if name == "identical":          # two identical boxes: every anchor eligible for one is eligible for the other at the same IoU
        twin = [208.0, 128.0, 96.0, 80.0]
        g = np.concatenate([[twin], IC._random_boxes(rs, 3, 448, 256), [twin], IC._random_boxes(rs, 2, 448, 256)])
        return case(IC._pack(S, [g], [7], rs.randint(0, 3, (1, 7)), 3, name), iou_thresh=0.25, max_per_box=8)
    if name == "boundary":           # half an anchor, a quarter of one: IoU exactly 0.5 and 0.25 with the twin the claim left free
        g = np.array([[64.0, 64.0, 24.0, 32.0], [256.0, 128.0, 48.0, 16.0], [352.0, 192.0, 96.0, 32.0], [160.0, 96.0, 16.0, 96.0]])
        return case(IC._pack(S2, [g], [4], [[0, 1, 2, 0]], 3, name), iou_thresh=0.5, max_per_box=4)
    if name == "cap_tie":            # S2 and an odd K: the K-th and (K+1)-th anchors are a and a + 273, equal in IoU
        return case(IC._pack(S2, [_lattice(rs, 6)], [6], rs.randint(0, 3, (1, 6)), 3, name), iou_thresh=0.0, max_per_box=3, topk=3)
    if name == "k1":                 # K = 1 and topk = 1 on S2: the one place goes to the higher / the lower of a tied pair
        return case(IC._pack(S2, [_lattice(rs, 5), IC._random_boxes(rs, 4, 448, 256)], [5, 4], rs.randint(0, 3, (2, 5)), 3, name),
                    iou_thresh=0.0, max_per_box=1, topk=1)
    if name == "all_candidates":     # topk above the number of cells: every anchor is a candidate; K = 64, the largest
        t = IC.grid(3, 2)
        return case(IC._pack(t, [IC._random_boxes(rs, 3, 128, 96), _lattice(rs, 2) / 4.0], [3, 2], rs.randint(0, 3, (2, 3)), 3, name),
                    iou_thresh=0.1, max_per_box=64, topk=8)
    if name == "far":                # no anchor overlaps: the claimed anchor (distance sweep) is the only positive
        g = IC._random_boxes(rs, 6, 448, 256)
        g[:, 0] -= 5000.0
        return case(IC._pack(S2, [g], [6], rs.randint(0, 3, (1, 6)), 3, name), iou_thresh=0.0)
    if name == "zero_width":
        return case(IC.label_case("degenerate"), iou_thresh=0.0, max_per_box=4)
    if name == "edge":               # gl = 64 and gr = 96 are anchor columns, no column lies between: centres ON the edge only
        g = np.array([[80.0, 64.0, 32.0, 64.0], [300.0, 150.0, 70.0, 50.0]])
        return case(IC._pack(S, [g], [2], [[1, 2]], 3, name), iou_thresh=0.3, max_per_box=6, topk=4)
    if name == "variance":           # three candidates (topk 1): e * e lies between the population and the sample variance
        g = np.array(VARIANCE_BOXES)
        return case(IC._pack(S, [g], [len(g)], [[k % 3 for k in range(len(g))]], 3, name), iou_thresh=0.4, max_per_box=2, topk=1)
    if name == "empty":              # an image without boxes beside one with boxes
        return case(IC._pack(S, [np.zeros((0, 4)), IC._random_boxes(rs, 5, 448, 256)], [0, 5], rs.randint(0, 3, (2, 5)), 3, name), iou_thresh=0.3)
    if name == "counts":             # counts above M and below 0, as the reader never writes them
        g = [IC._random_boxes(rs, 6, 448, 256) for _ in range(3)]
        return case(IC._pack(S, g, [12, -3, 2], rs.randint(0, 3, (3, 6)), 3, name), iou_thresh=0.3, max_per_box=5, topk=5)
    if name in ("classes1", "classes20"):
        return case(IC.label_case(name), iou_thresh=0.3, max_per_box=6, topk=5)
    if name == "apg1":               # one shape: the candidates of the only shape are the topk nearest cells
        t = IC.grid(6, 5, IC.SHAPES3[:1])
        return case(IC._pack(t, [IC._random_boxes(rs, 4, 224, 192), _lattice(rs, 3) / 2.0], [4, 3], rs.randint(0, 2, (2, 4)), 2, name), apg=1,
                    iou_thresh=0.2, max_per_box=5, topk=6)
    if name == "three":
        return case(IC.label_case("three"), iou_thresh=0.0, max_per_box=2, topk=1)
    if name == "one":
        return case(IC.label_case("one"), apg=1, iou_thresh=0.0, max_per_box=1, topk=1)
    if name == "kitti":              # the real table at mosaic-like density
        def boxes(n):
            return np.stack([rs.uniform(0, 1248, n), rs.uniform(0, 384, n), rs.uniform(20, 300, n), rs.uniform(20, 200, n)], 1)
        g = [boxes(21), boxes(18)]
        return case(IC._pack(kitti_table(), g, [21, 18], rs.randint(0, 3, (2, 21)), 3, name), apg=9, iou_thresh=0.5, max_per_box=16, topk=9)
    if name == "over_cap":           # 4200 cells of one shape and a box that overlaps all of them: neither fits the LDS stage
        t = IC.grid(70, 60, IC.SHAPES3[:1])
        g = np.concatenate([[[1136.0, 976.0, 2400.0, 2000.0]], IC._random_boxes(rs, 2, 2240, 1920)])
        return case(IC._pack(t, [g], [3], [[0, 1, 0]], 2, name), apg=1, iou_thresh=0.0, max_per_box=16, topk=9)
    raise KeyError(name)


# (found by a seeded search over S's lattice, checked by tests/test_assign_host.py: under topk = 1 each has a candidate that the
# population variance admits and the sample variance does not)
VARIANCE_BOXES = [[80.0, 128.0, 112.0, 16.0], [176.0, 160.0, 80.0, 112.0], [288.0, 32.0, 80.0, 32.0]]


def mode_kwargs(case, mode):
    return dict(iou_thresh=case.iou_thresh, max_per_box=case.max_per_box) if mode == "iou" else dict(topk=case.topk)


@functools.lru_cache(maxsize=None)
def reference(name, mode, **switches):
    """tests/assign_reference.assign_reference of the case under `mode` (computed once, read-only), with the given mutation switches."""
    c = assign_case(name)
    ref = R.assign_reference(c.label, mode, c.apg, **mode_kwargs(c, mode), **switches)
    for t in ref[:7]:
        t.setflags(write=False)
    return ref

"""The shared cases of the optimizer-with-options tests (tests/test_optimizer_host.py, tests/test_gpu_optimizer_options.py).

The layout: variables of 1, 2, 63, 64, 65, 2047, 2048, 2049 and 64 * 2048 + 1 elements -- around the 64-element padding of the
trainers, around the 2048 elements of a block, and one past the 64-block cap, whose blocks take a second lap of the stride loop.
Offsets alternate between multiples of four (the 16-byte path, with 0 .. 3 tail elements) and odd ones (the scalar path); every
second variable has a decay; gaps of 1 .. 4 elements hold a sentinel, every third gap element NaN and every fifth inf -- in all
five buffers.  Gradient norms are about 3 for every other pair of variables and about 0.3 for the rest: both sides of a clip at 1.
"""
import numpy as np

COUNTS = [1, 2, 63, 64, 65, 2047, 2048, 2049, 64 * 2048 + 1]
SENTINEL = -123.456
DECAY = 1e-2


def layout():
    """(offsets, counts, decays, total)."""
    offs, o = [], 3
    for v, c in enumerate(COUNTS):
        o += 1                                       # a gap of at least one element
        if v % 2 == 0:
            o = (o + 3) // 4 * 4                     # a multiple of four
        elif o % 2 == 0:
            o += 1                                   # odd
        offs.append(o)
        o += c
    decs = [DECAY if v % 2 == 1 else 0.0 for v in range(len(COUNTS))]
    return offs, list(COUNTS), decs, o + 5


def inside_mask(offs, cnts, total):
    m = np.zeros(total, bool)
    for o, c in zip(offs, cnts):
        m[o:o + c] = True
    return m


def buffers(offs, cnts, total, seed):
    """[P, G, A, A2, E] float32: values inside the segments, the sentinel / NaN / inf pattern in the gaps."""
    rs = np.random.RandomState(seed)
    bufs = [np.full(total, SENTINEL, np.float32) for _ in range(5)]
    gaps = np.flatnonzero(~inside_mask(offs, cnts, total))
    for b in bufs:
        b[gaps[::3]] = np.nan
        b[gaps[::5]] = np.inf
    P, G, A, A2, E = bufs
    for v, (o, c) in enumerate(zip(offs, cnts)):
        n = 3.0 if (v // 2) % 2 == 0 else 0.3
        P[o:o + c] = rs.randn(c) * 0.1
        G[o:o + c] = rs.randn(c) * (n / np.sqrt(c)) if c > 1 else n
        A[o:o + c] = rs.randn(c) * 0.01
        A2[o:o + c] = np.abs(rs.randn(c)) * 1e-4
        E[o:o + c] = P[o:o + c] + rs.randn(c).astype(np.float32) * 0.01
    return bufs


def gradients(offs, cnts, total, seed):
    return buffers(offs, cnts, total, seed)[1]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# every rule x clip mode x EMA off / on / warm-up
RULES = ("momentum", "nesterov", "adamw")
CLIPS = ("per_variable", "global")
EMAS = ((0.0, False), (0.99, False), (0.99, True))

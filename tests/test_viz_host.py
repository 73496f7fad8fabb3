"""CPU-side checks of the drawing entry points (include/sqdet.h "drawing", squeezedet_amd/viz.py): exports, argument validation
without a device, the font table, the NumPy restatement (tests/draw_reference.py) against hand-written 12 x 12 pictures, the
drivers' new flags and the pixel restore rule."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from squeezedet_amd import _lib, viz
from squeezedet_amd import build as sqbuild
from tests import draw_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGR_MEANS = (103.939, 116.779, 123.68)


@pytest.fixture(scope="module")
def lib():
    sqbuild.build(verbose=False)
    return _lib.lib()


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_the_drawing_symbols(lib):
    for n in ("sqdet_draw_items", "sqdet_draw_build_items", "sqdet_draw_font5x7"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES


def test_bad_arguments_return_codes_without_a_device(lib):
    fake = lambda k=1: C.c_void_p(0x10000 * k)            # 16-byte aligned, never dereferenced on the host
    means = (C.c_float * 3)(*BGR_MEANS)
    tabs, cnts = (C.c_void_p * 4)(*[0x10000 * k for k in range(1, 5)]), (C.c_void_p * 4)(*[0x20000 * k for k in range(1, 5)])
    caps = lambda *v: (C.c_int * 4)(*(list(v) + [1] * (4 - len(v))))
    draw = lib.sqdet_draw_items
    assert draw(None, fake(), 0, 1, 8, 8, means, 1, tabs, cnts, caps(4), 1, None) == -1 and b"null" in lib.sqdet_last_error()
    assert draw(fake(), None, 0, 1, 8, 8, means, 1, tabs, cnts, caps(4), 1, None) == -1
    assert draw(fake(), fake(2), 0, 1, 8, 8, None, 1, tabs, cnts, caps(4), 1, None) == -1          # float input without means
    assert draw(fake(), fake(2), 0, 0, 8, 8, means, 1, tabs, cnts, caps(4), 1, None) == -1         # B <= 0
    assert draw(fake(), fake(2), 0, -3, 8, 8, means, 1, tabs, cnts, caps(4), 1, None) == -1
    assert draw(fake(), fake(2), 0, 1, 0, 8, means, 1, tabs, cnts, caps(4), 1, None) == -1
    assert draw(fake(), fake(2), 7, 1, 8, 8, means, 1, tabs, cnts, caps(4), 1, None) == -1         # bad in_type
    assert draw(fake(), fake(2), 0, 1, 8, 8, means, 1, tabs, cnts, caps(4), 5, None) == -1         # too many tables
    assert draw(fake(), fake(2), 0, 1, 8, 8, means, 1, None, cnts, caps(4), 1, None) == -1
    assert draw(fake(), fake(2), 0, 1, 8, 8, means, 1, tabs, cnts, caps(257), 1, None) == _lib.SQDET_EUNSUPPORTED
    assert b"257" in lib.sqdet_last_error()
    assert draw(fake(), fake(2), 0, 1, 8, 8, means, 1, tabs, cnts, caps(200, 57), 2, None) == _lib.SQDET_EUNSUPPORTED
    assert draw(fake(), fake(2), 2, 4, 40000, 40000, None, 1, tabs, cnts, caps(4), 1, None) == _lib.SQDET_EUNSUPPORTED   # >= 2^31 pixels
    build = lib.sqdet_draw_build_items
    ok = [fake(1), 0, fake(2), fake(3), fake(4), 2, 64, 0, 0.4, fake(5), 3, None, 0, 255, 0, 1, 0, fake(6), fake(7), 64, None]

    def with_(**kw):
        names = ["boxes", "f64", "probs", "cls", "counts", "n", "rows", "diagonal", "thresh", "names", "classes", "class_bgr", "b", "g", "r",
                 "fmt", "anchor", "items", "item_counts", "cap", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return build(*a)
    for k in ("boxes", "cls", "counts", "names", "items", "item_counts"):
        assert with_(**{k: None}) == -1, k
    assert with_(probs=None) == -1                          # "name: (p)" without probabilities
    assert with_(n=0) == -1 and with_(rows=0) == -1 and with_(classes=0) == -1
    assert with_(fmt=3) == -1 and with_(anchor=2) == -1 and with_(g=256) == -1
    assert with_(rows=257, cap=257) == _lib.SQDET_EUNSUPPORTED
    assert with_(rows=64, cap=32) == _lib.SQDET_EUNSUPPORTED
    assert lib.sqdet_draw_font5x7(None, 665) == -1
    buf = (C.c_ubyte * 665)()
    assert lib.sqdet_draw_font5x7(buf, 664) == -1 and lib.sqdet_draw_font5x7(buf, 665) == 0


def _glyph(*rows):
    return [int(r.replace(".", "0").replace("#", "1"), 2) for r in rows]


def test_font_table(lib):
    f = viz.font()
    assert f.shape == (95, 7) and f.dtype == np.uint8 and int(f.max()) < 32
    assert not f[0].any(), "space is empty"
    assert all(f[i].any() for i in range(1, 95)), "every other glyph has ink"
    assert len(set(bytes(g) for g in f)) == 95, "glyphs are pairwise distinct"
    pinned = {"0": _glyph(".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
              "1": _glyph("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
              ":": _glyph(".....", ".##..", ".##..", ".....", ".##..", ".##..", ".....")}
    for ch, rows in pinned.items():
        assert f[ord(ch) - 32].tolist() == rows, ch


def _art(rows, colours):
    """12 text rows -> uint8 [12, 12, 3]: '.' is the background 7, another character its colour."""
    assert len(rows) == 12 and all(len(r) == 12 for r in rows)
    out = np.full((12, 12, 3), 7, np.uint8)
    for y, r in enumerate(rows):
        for x, ch in enumerate(r):
            if ch != ".":
                out[y, x] = colours[ch]
    return out


BLANK = "............"
A, B_ = (10, 20, 30), (200, 100, 50)
HAND = {
    "inside": ([(2, 3, 8, 9, A, b"", "bottom_left")],
               [BLANK] * 3 + ["..#######..."] + ["..#.....#..."] * 5 + ["..#######..."] + [BLANK] * 2),
    "crosses left": ([(-3, 2, 4, 6, A, b"", "bottom_left")],
                     [BLANK] * 2 + ["#####......."] + ["....#......."] * 3 + ["#####......."] + [BLANK] * 5),
    "crosses right": ([(7, 2, 15, 6, A, b"", "bottom_left")],
                      [BLANK] * 2 + [".......#####"] + [".......#...."] * 3 + [".......#####"] + [BLANK] * 5),
    "crosses top": ([(3, -4, 9, 2, A, b"", "bottom_left")],
                    ["...#.....#.."] * 2 + ["...#######.."] + [BLANK] * 9),
    "crosses bottom": ([(3, 9, 9, 20, A, b"", "bottom_left")],
                       [BLANK] * 9 + ["...#######.."] + ["...#.....#.."] * 2),
    "swapped corners": ([(8, 9, 2, 3, A, b"", "bottom_left")],
                        [BLANK] * 3 + ["..#######..."] + ["..#.....#..."] * 5 + ["..#######..."] + [BLANK] * 2),
    "one pixel": ([(5, 5, 5, 5, A, b"", "bottom_left")], [BLANK] * 5 + [".....#......"] + [BLANK] * 6),
    "wholly outside": ([(20, 20, 30, 30, A, b"11", "bottom_left"), (-9, -9, -2, -2, A, b"11", "top_left")], [BLANK] * 12),
    "label bottom left": ([(2, 1, 9, 10, A, b"1", "bottom_left")],
                          [BLANK, "..########..", "..#......#..", "..#..#...#..", "..#.##...#.."] + ["..#..#...#.."] * 4 +
                          ["..#.###..#..", "..########..", BLANK]),
    "label top left": ([(2, 1, 9, 10, A, b"1", "top_left")],
                       [BLANK, "..########..", "..#.##...#.."] + ["..#..#...#.."] * 4 + ["..#.###..#.."] + ["..#......#.."] * 2 +
                       ["..########..", BLANK]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_against_hand_pictures(lib, name):
    items, rows = HAND[name]
    img = np.full((1, 12, 12, 3), 7, np.uint8)
    got = R.draw(img, [[items]], viz.font(), order="bgr")[0]
    assert np.array_equal(got, _art(rows, {"#": A})), name
    rgb = R.draw(img, [[items]], viz.font(), order="rgb")[0]
    assert np.array_equal(rgb, got[..., ::-1])


def test_restatement_later_item_wins(lib):
    a, b = (1, 1, 6, 6, A, b"", "bottom_left"), (4, 4, 9, 9, B_, b"", "bottom_left")
    img = np.full((1, 12, 12, 3), 7, np.uint8)
    ab = [BLANK, ".aaaaaa.....", ".a....a.....", ".a....a.....", ".a..bbbbbb..", ".a..b.a..b..", ".aaabaa..b..", "....b....b..",
          "....b....b..", "....bbbbbb..", BLANK, BLANK]
    ba = list(ab)
    ba[4], ba[6] = ".a..bbabbb..", ".aaaaaa..b.."
    cols = {"a": A, "b": B_}
    assert np.array_equal(R.draw(img, [[[a, b]]], viz.font(), "bgr")[0], _art(ab, cols))
    assert np.array_equal(R.draw(img, [[[b, a]]], viz.font(), "bgr")[0], _art(ba, cols))
    # two tables are drawn one after the other: the same picture as one table holding both
    assert np.array_equal(R.draw(img, [[[a]], [[b]]], viz.font(), "bgr")[0], _art(ab, cols))


def test_driver_flags_parse():
    t, e, d = _load("train"), _load("eval"), _load("demo")
    assert t.parse_args([]).image_summary == 0 and t.parse_args(["--image_summary", "4"]).image_summary == 4
    a = e.parse_args([])
    assert (a.visualize, a.seed) == (0, 0)
    a = e.parse_args(["--visualize", "10", "--seed", "7"])
    assert (a.visualize, a.seed) == (10, 7)
    a = d.parse_args([])
    assert (a.mode, a.draw, a.crop, a.batch) == ("image", "pil", [500, 205, 239, 439], 1)
    a = d.parse_args(["--mode", "video", "--draw", "gpu", "--crop", "1", "2", "3", "4", "--batch", "8", "--demo_net", "squeezeDet+"])
    assert (a.mode, a.draw, a.crop, a.batch) == ("video", "gpu", [1, 2, 3, 4], 8)
    with pytest.raises(AssertionError):
        d.parse_args(["--mode", "video", "--demo_net", "resnet50"])


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_restore_rule_round_trips_every_byte(dtype):
    """rint(float32(storage(v - mean)) + mean) == v for every uint8 v and each mean: below |x| < 256 a float16 is at most 0.0625
    from the value it stores, so the rounding lands on v again."""
    v = np.arange(256, dtype=np.float32).reshape(256, 1)
    m = np.asarray(BGR_MEANS, np.float32).reshape(1, 3)
    x = (v - m).astype(dtype)
    assert float(np.abs(x.astype(np.float32) - (v - m)).max()) <= 0.0625
    assert np.array_equal(R.restore(x, BGR_MEANS), np.broadcast_to(v, (256, 3)).astype(np.uint8))
    # and the clamp / half-to-even edges of the rule itself
    e = np.asarray([[-200.0, 0.5 - 103.939, 1.5 - 103.939], [400.0, 254.5 - 116.779, 255.6 - 123.68]], np.float32)
    got = R.restore(e, BGR_MEANS)
    want = np.clip(np.rint(e + m), 0, 255).astype(np.uint8)
    assert np.array_equal(got, want) and got[0, 0] == 0 and got[1, 0] == 255

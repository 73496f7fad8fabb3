"""tests/net_plan_cases.CASES -- the plans tests/test_gpu_net_plans.py executes -- against the golden matrix of
make_net_plans_golden.py, on the host (plan creation needs no device).  A condition, not a measurement: per (arch, dtype), EVERY
layer-name sequence that occurs among the matrix's 1920 plans is planned by at least one case, so deleting the only case of a
structure fails here.  Also: the pixel cap, every option on every arch whose plans it changes, and a default float16 SqueezeDet case
that holds ring-chain launches with room for riders.

Layer names cannot tell a streaming expand + squeeze launch from a ring-chain launch -- both are "<fire>/expand+<next>/squeeze1x1";
sqdet_net_overlap_layer (the first chain launch) is what shows a chain, and the last test reads it."""
import collections

import pytest

from tests import net_plan_cases as NC
from tests.golden import make_net_plans_golden as G


@pytest.fixture(scope="module")
def lib():
    return G.load_lib()


@pytest.fixture(scope="module")
def case_texts(lib):
    return [NC.case_text(lib, c) for c in NC.CASES]


@pytest.fixture(scope="module")
def matrix_texts(lib):
    return [(row, G.plan_text(lib, *row[1:])) for row in G.matrix()]


def _field(text, name):
    (line,) = [ln for ln in text.split("\n") if ln.startswith(name + " ")]
    return int(line.split(" ")[1])


def test_cases_are_well_formed():
    assert len(NC.CASES) == len(set(NC.case_id(c) for c in NC.CASES)), "a case is listed twice"
    assert 40 <= len(NC.CASES) <= 60
    for arch, dtype, batch, size, option in NC.CASES:
        assert arch in NC.ARCH_ID and dtype in NC.DTYPE_ID and batch >= 1 and min(size) >= 64
        assert option is None or option in G.OPTIONS


def test_every_matrix_structure_is_planned_by_a_case(lib, case_texts, matrix_texts):
    ids = {name: i for name, i in G.ARCHS}
    dts = {name: i for name, i in G.DTYPES}
    have = collections.defaultdict(set)
    for case, text in zip(NC.CASES, case_texts):
        have[(ids[case[0]], dts[case[1]])].add(NC.names_of(text))
    want = collections.defaultdict(dict)
    for (key, arch, dtype, batch, size, opt), text in matrix_texts:
        want[(arch, dtype)].setdefault(NC.names_of(text), key)
    assert sum(len(v) for v in want.values()) == 37, {k: len(v) for k, v in want.items()}     # 11 + 5 + 11 + 2 + 4 x 2
    missing = [key for ad, sts in want.items() for st, key in sts.items() if st not in have[ad]]
    assert not missing, "no case plans the structure of: %s (make_net_plans_golden.py --show KEY prints it)" % missing
    # structure() is the same reading of the same plan
    c = NC.CASES[0]
    assert NC.structure(lib, *c) == NC.names_of(case_texts[0]) == NC.structure(lib, ids[c[0]], dts[c[1]], *c[2:])


def test_pixel_cap():
    over = []
    for case in NC.CASES:
        px = case[2] * case[3][0] * case[3][1]
        if px > NC.PIXEL_CAP:
            over.append(case)
            assert px <= NC.OVER_CAP_LIMIT, NC.case_id(case)
    # the two structures that keep fire4 / fire5 out of the pixel rule's reach need 100000 map pixels at 1/64 of the input's
    # (net_plan_cases's docstring): exactly those two cases, nothing else, may pass the cap
    assert over == NC.OVER_CAP and sorted((c[0], c[1], c[4][:2]) for c in over) == [("squeezedet", "f16", ("fire_fuse", 6)),
                                                                                    ("squeezedet", "f32", ("fire_fuse", 10))]
    for c in over:       # ... and they are as small as the rule allows: one image fewer plans another structure
        assert (c[2] - 1) * 81 <= 100000 < c[2] * 81 and c[3] == (65, 65)


def test_every_option_is_run_on_every_arch_whose_plans_it_changes(lib, case_texts, matrix_texts):
    default = {row[1:5]: text for row, text in matrix_texts if row[5] is None}
    changed = set()
    for (key, arch, dtype, batch, size, opt), text in matrix_texts:
        if opt is not None and text != default[(arch, dtype, batch, size)]:
            changed.add((arch, opt))
    names = {i: name for name, i in G.ARCHS}
    run = set()
    for case, text in zip(NC.CASES, case_texts):       # a case counts where its option changes the plan at the case's own shape
        if case[4] is not None and text != NC.case_text(lib, case[:4] + (None,)):
            run.add((case[0], case[4]))
    missing = sorted((names[a], o[:2]) for a, o in changed if (names[a], o) not in run)
    assert not missing, missing
    # and every entry of OPTIONS runs somewhere ("stem_algo" 3 changes no plan text, only the stem kernel under the launch)
    assert set(G.OPTIONS) == set(c[4] for c in NC.CASES)


def test_default_squeezedet_f16_case_has_chain_launches_with_riders(case_texts):
    found = 0
    for case, text in zip(NC.CASES, case_texts):
        if case[:2] == ("squeezedet", "f16") and case[4] is None:
            names = NC.names_of(text)
            ov = _field(text, "overlap_layer")
            assert ov >= 0 and "/expand+" in names[ov] and _field(text, "rider_capacity") >= case[2] > 0, NC.case_id(case)
            found += "conv1+pool1+fire2/squeeze1x1" in names
    assert found >= 1, "no default float16 SqueezeDet case with the stem + squeeze launch"

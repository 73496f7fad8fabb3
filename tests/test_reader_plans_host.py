"""BatchReader.next_plan against tests/golden/reader_plans.json: under every augmentation policy the plans and the generator's
state are, bit for bit, those of the commit the fixture was written from (tests/golden/make_reader_plans.py).  No GPU."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_reader_plans", os.path.join(HERE, "golden", "make_reader_plans.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


G = _generator()
with open(G.OUT) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_the_case_matrix():
    assert (GOLDEN["seed"], GOLDEN["plans"]) == (G.SEED, G.PLANS)
    assert sorted(GOLDEN["cases"]) == sorted(G.cases()) and len(GOLDEN["cases"]) == 49


@pytest.mark.parametrize("name", list(G.cases()))
def test_plans_are_the_fixtures(name):
    sha, trail, labels = G.run_case(*G.cases()[name])
    want = GOLDEN["cases"][name]
    if sha != want["sha256"]:
        got, old = [[t[i:i + 4] for i in range(0, len(t), 4)] for t in (trail, want["trail"])]
        first = next((i for i, (a, b) in enumerate(zip(got, old)) if a != b), min(len(got), len(old)))
        where = labels[first] if first < len(labels) else "the number of fields (%d, the fixture has %d)" % (len(got), len(old))
        pytest.fail("case %r: the first difference from the fixture is at %s" % (name, where))
    assert trail == want["trail"]

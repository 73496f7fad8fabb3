"""The planner (squeezedet_amd/csrc/net.cpp) against tests/golden/net_plans.json: every plan of make_net_plans_golden.py's
matrix -- 4 archs x 2 dtypes x 4 batches x 4 image sizes x 15 option settings -- is rebuilt on the host (plan creation needs
no device) and must equal, exactly, what the commit that wrote the fixture planned: layer names, flops, bytes, the parameter
table, param / workspace bytes, output dims, rider capacity, overlap layer, score support."""
import json

import pytest

from tests.golden import make_net_plans_golden as G


@pytest.fixture(scope="module")
def lib():
    return G.load_lib()


@pytest.fixture(scope="module")
def golden():
    with open(G.PATH) as f:
        return json.load(f)


def test_fixture_covers_the_matrix(golden):
    keys = [r[0] for r in G.matrix()]
    assert len(keys) == len(set(keys)) == 4 * 2 * 4 * 4 * 15
    assert sorted(golden["digests"]) == sorted(keys)
    full = [G.key_of(an, dn, b, s, None) for an, _ in G.ARCHS for dn, _ in G.DTYPES for b, s in G.FULL]
    assert sorted(golden["tables"]) == sorted(full)


def test_every_plan_matches_the_fixture(lib, golden):
    rows = G.matrix()
    bad = []
    for key, arch, dtype, batch, size, opt in rows:
        text = G.plan_text(lib, arch, dtype, batch, size, opt)
        if key in golden["tables"]:
            assert text.split("\n") == golden["tables"][key], key      # (a readable diff for the plans stored whole)
        if G.digest(text) != golden["digests"][key]:
            bad.append(key)
    assert not bad, "%d of %d plans differ (make_net_plans_golden.py --show KEY prints one), first: %s" % (len(bad), len(rows), bad[:8])

"""Every output bit of the twelve latent-prep / LCM-step entries (csrc/lcm.hip) against tests/golden/lcm_family_digests.json: SHA-256 digests
that tools/lcm_family_ab.py wrote on the library of the commit before the family was folded into one kernel body per op.  "Masked with an
all-ones mask == the plain step" holds by construction since then (one function computes both), so it no longer ties the plain kernel's bits
to anything; this does.  The case list is the tool's (cases(): sizes 1, 257 and 2048 * 256 + 3, nb, row strides, both step kinds, the optional
outputs, the three scalar sets, mask kinds, level thresholds, content modes, both storage types).  A digest that moves means the arithmetic of
that instantiation changed: find the operation in the device code; the fixture is never rewritten from the code under test."""
import json
import os

import pytest

from tools import lcm_family_ab as ab

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lcm_family_digests.json")
CASES = ab.cases()
GROUPS = sorted({c[:3] for c in CASES}, key=str)                   # (op, storage type, flavour): 32 tests over all the cases


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_is_the_case_list(golden):
    assert set(golden) == {str(c) for c in CASES}


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "-".join(str(v) for v in (g[0], g[1]) + g[2]))
def test_digests(fie, golden, group):
    mine = [c for c in CASES if c[:3] == group]
    got = {str(c): ab.run_case(c) for c in mine}
    bad = ab.differing(got, {k: golden[k] for k in got})
    assert not bad, f"{len(bad)} of {len(mine)} cases moved: {bad[:8]}"

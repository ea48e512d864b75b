"""Every covered entry point stays inside its outputs and its workspace (docs/memory_contract.md).

Each case of tests/_entry_cases.py runs with every array it sees -- inputs, outputs, in/out arrays, the workspace at exactly the
queried size -- carved from one arena with 1 MiB guards around each (tests/_guarded.py), under {aligned, least} placement x
{guards 0x00 / workspace and outputs 0xFF, guards 0xFF / workspace and outputs 0x00}, through _lib.lib() on raw pointers.  Asserted
per case, family and shape:

  1. rc        the return code is 0
  2. guards    every guard byte is intact (the message names the array and the offset)
  3. inputs    every const input is bitwise unchanged
  4. fill      over the documented extent the outputs of the two fills are bitwise equal (the case's bar where the header
               promises no repeatable result): no dependence on what the workspace or the outputs held, no over-read that
               reaches the result
  5. placement the same between aligned and least placement
  6. extent    no element inside the documented extent still holds its fill
  7. short     one byte less than the query is MGP_ERR_WORKSPACE and touches nothing

tests/test_guarded_cpu.py shows on planted defects that each of these fails when it should.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _guarded as G                      # noqa: E402
import _entry_cases as E                  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the memory contract is checked on the MI355X only")
    return torch.device("cuda:0")


@pytest.mark.parametrize("name,family,shape_id", E.params(), ids=["%s-%s-%s" % p for p in E.params()])
def test_entry_point_keeps_the_memory_contract(dev, name, family, shape_id):
    case = E.CASES[name]
    with case.families[family]():
        found = G.run_contract(case.fn, case.shapes_of(family)[shape_id], dev, sync=torch.cuda.synchronize)
    print("%s %s %s: %s" % (name, family, shape_id, {c: len(found[c]) for c in G.CHECKS}))
    for check in G.CHECKS:
        assert not found[check], "%s [%s, %s] breaks check `%s`:\n%s" % (name, family, shape_id, check, G.report(found))

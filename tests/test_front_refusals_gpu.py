"""Every refusal of the four front-end objects and the chain, status and sdr_last_error() text, against
tests/golden/front_refusals.json - recorded once with the library as it stood before the objects shared a host core
(tests/front_refusals.py holds the table and record()).  A call that is wrong in two ways fails as it failed then, which pins
the order of the checks; a good call behind every refusal and the object's sample count show that the refusal moved nothing."""
import json

import pytest

import front_refusals as FR
from parity_tools import capi  # noqa: F401

pytestmark = pytest.mark.gpu


def test_every_refusal_keeps_its_status_and_text(capi):
    with open(FR.GOLDEN) as f:
        want = json.load(f)
    got = {}
    ids = FR.run(capi, lambda name, status, text: got.__setitem__(name, [status, text]))
    assert sorted(want) == sorted(ids) == sorted(got), "the table and the golden file list the same cases"
    wrong = {name: (got[name], want[name]) for name in ids if got[name] != want[name]}
    assert not wrong, wrong
    # the table does what it says: every status a refusal can have, and two-way cases on every object
    assert {s for s, _ in want.values()} == {capi.ERR_BAD_ARG, capi.ERR_BAD_SIZE, capi.ERR_STATE}
    for obj in ("ddc", "chan", "fine", "nb", "chain"):
        assert sum(name.startswith(obj + ".") and "+" in name for name in ids) >= 4, obj

"""GPU: every refusal of tests/abi_refusal_cases.py answers what tests/golden/abi_refusals.json recorded: the same return code and the
same message, byte for byte.  The pairs of the table carry two bad arguments at once, so the message also pins which of two refusals
an entry point makes first.  The file was recorded (tools/record_abi_refusals.py) from the library before its host side was folded
into shared helpers; it is not regenerated.  A refused call launches nothing: every output buffer still holds its sentinel and the
four env states are what they were before the first call."""
import json
import os

import pytest

import abi_refusal_cases as A

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_refusals.json")


@pytest.fixture(scope="module")
def run():
    return A.run_cases()


def test_table_and_recording_hold_the_same_cases():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(name for name, _, _ in A.CASES)
    assert all(rc < 0 and msg for rc, msg in golden.values())
    assert {entry for _, entry, _ in A.CASES} == set(A.ORDER)


def test_every_refusal_is_the_recorded_one(run):
    with open(GOLDEN) as f:
        golden = json.load(f)
    results, _ = run
    wrong = {name: (got, golden.get(name)) for name, got in results.items() if golden.get(name) != got}
    for name, (got, want) in wrong.items():
        print(name, "\n   now      ", got, "\n   recorded ", want)
    assert not wrong, "%d of %d refusals differ from the recording" % (len(wrong), len(results))
    assert len(results) == len(golden)


def test_refusals_touch_no_buffer_and_no_state(run):
    assert run[1] == []

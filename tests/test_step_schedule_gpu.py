"""GPU: the host-side schedule of whole train steps, entry by entry (tests/schedule_trace.py), against the traces stored in
tests/step_schedule.json.  Results alone do not show a dropped event wait; the order of launches, records and waits does.
A pull request that changes the schedule on purpose regenerates the file (tools/step_schedule.py --write) and shows the
change as its diff."""
import json
import os

import pytest

from tests.schedule_trace import SCHEDULE_CASES, first_difference, trace_case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_schedule.json")) as fh:
    STORED = json.load(fh)


@pytest.mark.parametrize("name", list(SCHEDULE_CASES))
def test_schedule_is_the_stored_one(name, monkeypatch):
    got = trace_case(name, monkeypatch.setenv)
    want = STORED["traces"][STORED["cases"][name]]
    diff = first_difference(want, got)
    if diff:
        print(diff)
    assert diff is None, f"{name}: {diff.splitlines()[0]}"

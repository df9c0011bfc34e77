"""CPU: the stored schedule file names every case of tests/schedule_trace.py, and a difference between two traces is found
and printed with its context."""
import json
import os

from tests.schedule_trace import SCHEDULE_CASES, first_difference


def test_every_case_is_stored():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_schedule.json")) as fh:
        stored = json.load(fh)
    assert sorted(stored["cases"]) == sorted(SCHEDULE_CASES)
    assert sorted(set(stored["cases"].values())) == sorted(stored["traces"])
    traces = list(stored["traces"].values())
    assert all(len(t) > 50 for t in traces) and all(a != b for i, a in enumerate(traces) for b in traces[i + 1:])


def test_first_difference_names_the_entry_and_its_context():
    want = [f"bd_k{i} on bh" for i in range(20)]
    assert first_difference(want, list(want)) is None
    dropped_wait = want[:12] + want[13:]
    text = first_difference(want, dropped_wait)
    assert text.splitlines()[0] == "first difference at entry 12 (stored 20 entries, this run 19)"
    assert len(text.splitlines()) == 1 + 11 and ">>    12  stored: bd_k12 on bh" in text and "this run: bd_k13 on bh" in text
    assert "bd_k7 on bh" in text and "bd_k6 on bh" not in text
    longer = first_difference(want, want + ["record e0 on bh"])
    assert "entry 20" in longer and "<end>" in longer

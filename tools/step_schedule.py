#!/usr/bin/env python3
"""The schedule of the train step per configuration (tests/schedule_trace.py) against tests/step_schedule.json.

    python tools/step_schedule.py            compare, print the first difference of every case that differs
    python tools/step_schedule.py --write    regenerate the file (each distinct trace once, each case -> its trace)
    python tools/step_schedule.py --show small-pipelined
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STORE = os.path.join(ROOT, "tests", "step_schedule.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--show", metavar="CASE")
    ap.add_argument("--out", default=STORE, help="the file --write fills")
    args = ap.parse_args()
    from tests.schedule_trace import SCHEDULE_CASES, first_difference, trace_case

    def run(name):
        before = dict(os.environ)
        try:
            return trace_case(name, os.environ.__setitem__)
        finally:
            os.environ.clear()
            os.environ.update(before)

    if args.show:
        print("\n".join(run(args.show)))
        return 0
    got = {name: run(name) for name in SCHEDULE_CASES}
    if args.write:
        traces, cases = {}, {}
        for name, entries in got.items():
            key = next((k for k, v in traces.items() if v == entries), None)
            if key is None:
                key = f"t{len(traces)}"
                traces[key] = entries
            cases[name] = key
        with open(args.out, "w") as fh:
            json.dump({"cases": cases, "traces": traces}, fh, indent=0)
            fh.write("\n")
        print(f"{len(cases)} cases, {len(traces)} distinct traces, {sum(map(len, traces.values()))} entries -> {args.out}")
        return 0
    with open(STORE) as fh:
        stored = json.load(fh)
    bad = 0
    for name, entries in got.items():
        diff = first_difference(stored["traces"][stored["cases"][name]], entries) if name in stored["cases"] else "not stored"
        print(f"{name}: {'same' if diff is None else diff}")
        bad += diff is not None
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

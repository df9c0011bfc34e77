"""The launch schedule of whole train steps as a list of strings: every bd_* call with the role of the stream it was
queued on, every event record and stream wait with the roles involved.  No pointers, so traces compare across processes;
tests/test_step_schedule_gpu.py holds them against tests/step_schedule.json, tools/step_schedule.py --write regenerates it."""
import dataclasses

import torch

from big_dreamer_amd import _cabi as cabi
from big_dreamer_amd import synth
from tests.helpers import CASES as GAUSS, CAT_CASES

PATCHED_MODULES = ("big_dreamer_amd.engine", "big_dreamer_amd.conv", "big_dreamer_amd.conv_stack", "big_dreamer_amd.replica",
                   "big_dreamer_amd.diagnostics_device")
ROLES = (("wm", "_s_wm"), ("bh", "_s_bh"), ("side", "_side"), ("early", "_s_early"))
# fields of the argument block that select a kernel form or an accumulation
BLOCK_SCALARS = {
    "bd_mlp_backward": lambda a: f"M={a.M} accumulate={a.accumulate}",
}


def _null(p):
    return "NULL" if not p else "set"


class _Library:
    """Stands in for the modules' `lib`: logs every bd_* call, then makes it."""

    def __init__(self, trace):
        self._trace = trace

    def __getattr__(self, key):
        real = getattr(cabi.lib, key)
        if not key.startswith("bd_"):
            return real
        trace = self._trace

        def call(*args):
            entry = f"{key} on {trace.role()}"
            if key == "bd_lambda_return_backward":
                entry += " " + " ".join(_null(v) if t is cabi.P else f"{v:.9g}" if t is cabi.F32 else str(v)
                                        for v, t in zip(args[:-1], real.argtypes))
            elif key in BLOCK_SCALARS:
                entry += " " + BLOCK_SCALARS[key](args[0]._obj)
            trace.entries.append(entry)
            return real(*args)
        return call


class ScheduleTrace:
    """Context manager: while active, `entries` collects the schedule `eng` queues."""

    def __init__(self, eng):
        self.eng, self.entries = eng, []
        self._events, self._keep = {}, []

    # ---- naming -------------------------------------------------------------------------------------------------------
    def role(self, stream=None):
        stream = torch.cuda.current_stream() if stream is None else stream
        for name, attr in ROLES:
            if stream == getattr(self.eng, attr):
                return name
        return "caller"

    def event(self, ev):
        if id(ev) not in self._events:
            self._events[id(ev)] = f"e{len(self._events)}"
            self._keep.append(ev)           # an id is unique only while its object lives
        return self._events[id(ev)]

    # ---- events and stream waits --------------------------------------------------------------------------------------
    def __enter__(self):
        import importlib
        trace = self
        self._saved = []
        for m in map(importlib.import_module, PATCHED_MODULES):
            self._saved.append((m, "lib", m.lib))
            m.lib = _Library(self)
        record, wait_event, wait_stream = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

        def traced_record(ev, stream=None):
            trace.entries.append(f"record {trace.event(ev)} on {trace.role(stream)}")
            return record(ev) if stream is None else record(ev, stream)

        def traced_wait_event(stream, ev):
            trace.entries.append(f"{trace.role(stream)} waits {trace.event(ev)}")
            return wait_event(stream, ev)

        def traced_wait_stream(stream, other):
            trace.entries.append(f"{trace.role(stream)} waits stream {trace.role(other)}")
            return wait_stream(stream, other)

        for obj, k, new in ((torch.cuda.Event, "record", traced_record), (torch.cuda.Stream, "wait_event", traced_wait_event),
                            (torch.cuda.Stream, "wait_stream", traced_wait_stream)):
            self._saved.append((obj, k, getattr(obj, k)))
            setattr(obj, k, new)
        return self

    def __exit__(self, *exc):
        for obj, k, old in reversed(self._saved):
            setattr(obj, k, old)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _small(attrs=None, hp=None, env=None):
    return dict(dims="small", attrs=attrs or {}, hp=hp or {}, env=env or {})


DISCRETE_TINY = (dataclasses.replace(synth.TINY, A=6, discrete_actions=True), 0, {}, True)    # tests/test_discrete_actions_gpu.py
SHAPES = {**GAUSS, **CAT_CASES, "discrete_tiny": DISCRETE_TINY}

# name -> dims (a key of SHAPES), engine attributes set after construction, hyper-parameters, environment, the step
SCHEDULE_CASES = {
    "small-pipelined": _small(),
    "small-serial": _small(dict(pipeline=False)),
    "small-one-chunk": _small(dict(bh_chunks=1)),
    "small-chunks-221": _small(dict(bh_chunks=(2, 2, 1))),
    "small-mix-0.5": _small(hp=dict(gradient_mixing=0.5)),
    "small-mix-0.0": _small(hp=dict(gradient_mixing=0.0)),
    "small-heads-unfused": _small(dict(heads_fused=False)),
    "small-actor-in-scan": _small(env=dict(BD_ACTOR_BWD_CHAIN="0")),
    "small-defer-opt": _small(dict(defer_opt=True)),
    "cat_tiny": dict(dims="cat_tiny", hp=dict(gradient_mixing=-1)),
    "cat_tiny-mix-0.0": dict(dims="cat_tiny", hp=dict(gradient_mixing=0.0)),
    "tiny_discount": dict(dims="tiny_discount", hp=dict(gradient_mixing=-1)),
    "tiny_discount-mix-0.5": dict(dims="tiny_discount", hp=dict(gradient_mixing=0.5)),
    "tiny_pixel": dict(dims="tiny_pixel"),
    "discrete_tiny": dict(dims="discrete_tiny"),
    "tiny-world-model-step": dict(dims="tiny", step="world_model_step"),
}


def trace_case(name, setenv):
    """Three un-synchronised steps of case `name` in a fresh engine, then join() -> the list of trace entries.  (Three:
    the waits indexed by step parity first fire in the third.)  setenv(key, value) sets an environment variable for the
    caller's scope: monkeypatch.setenv in a test."""
    from big_dreamer_amd.engine import DreamerEngine
    case = SCHEDULE_CASES[name]
    d, seed, hp, _ = SHAPES[case["dims"]]
    for k, v in case.get("env", {}).items():
        setenv(k, v)
    torch.manual_seed(1234)
    eng = DreamerEngine(d, dict(hp, **case.get("hp", {})), "cuda", params=synth.make_params(d, seed))
    for k, v in case.get("attrs", {}).items():
        setattr(eng, k, v)
    batches = [{k: torch.as_tensor(v).cuda().contiguous() for k, v in synth.make_batch(d, seed + i).items()} for i in range(3)]
    torch.cuda.synchronize()
    with ScheduleTrace(eng) as trace:
        for batch in batches:
            getattr(eng, case.get("step", "train_step"))(batch, sync_logs=False)
        eng.join()
    torch.cuda.synchronize()
    return trace.entries


def first_difference(want, got, context=5):
    """None when equal, else a printable account of the first differing entry with `context` entries before and after."""
    if want == got:
        return None
    i = next((k for k, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
    lo, hi = max(0, i - context), i + context + 1
    lines = [f"first difference at entry {i} (stored {len(want)} entries, this run {len(got)})"]
    for k in range(lo, min(hi, max(len(want), len(got)))):
        a, b = (want[k] if k < len(want) else "<end>"), (got[k] if k < len(got) else "<end>")
        lines.append(f"{'>>' if a != b else '  '} {k:5d}  stored: {a:<70}  this run: {b}")
    return "\n".join(lines)

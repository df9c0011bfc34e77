"""Diagnostic: which chain binds the pipelined step.  Runs the default workload with the span events on every step and
prints the gaps between span events of the dynamics and the behaviour chain across consecutive steps (a chain that
restarts right after its own previous end, while the other waits for it, is the one that binds).  Run from the root of
the tree to be measured: `python tools/step_chains.py`."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from big_dreamer_amd import synth
from big_dreamer_amd.engine import DreamerEngine
from big_dreamer_amd.memory import ExperienceReplay
d, dev = synth.CONFIG2, torch.device("cuda", 0)
eng = DreamerEngine(d, None, dev, params=synth.make_params(d, 0))
rep = synth.make_replay(d, rows=5000, seed=0)
buf = ExperienceReplay(5000, d.A, 5, False, d.O, dev)
for k, v in rep.items():
    getattr(buf, k)[:] = v
buf.idx, buf.full = 0, True
buf.sync_device()
def steps(n):
    for _ in range(n):
        o, a, r, nt = buf.sample(d.B, d.L)
        eng.train_step({"observations": o, "actions": a, "rewards": r, "nonterminals": nt}, None, sync_logs=False)
steps(40)
eng.flush_optimizers(); eng.join(); torch.cuda.synchronize()
eng.enable_timers(True, 1)
N = 30
steps(N)
eng.flush_optimizers(); eng.join(); torch.cuda.synchronize()
ev = eng._timer_events
print({k: len(v) for k, v in ev.items()})
def gap(a, ia, b, ib, off):      # time from event a[k + off] to event b[k]
    out = []
    for k in range(max(0, -off) + 3, N - max(0, off) - 1):
        out.append(ev[a][k + off][ia].elapsed_time(ev[b][k][ib]))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))
per = [ev["encoder_fwd"][k][0].elapsed_time(ev["encoder_fwd"][k + 1][0]) for k in range(3, N - 1)]
print("dynamics period  median %.4f" % np.median(per))
per = [ev["imagine_fwd"][k][0].elapsed_time(ev["imagine_fwd"][k + 1][0]) for k in range(3, N - 1)]
print("behaviour period median %.4f" % np.median(per))
print("opt_model end k   -> imagine_fwd start k   : median %.4f (%.4f .. %.4f)" % gap("opt_model", 1, "imagine_fwd", 0, 0))
print("opt_actor end k-1 -> imagine_fwd start k   : median %.4f (%.4f .. %.4f)" % gap("opt_actor", 1, "imagine_fwd", 0, -1))
print("opt_model end k-1 -> encoder_fwd start k   : median %.4f (%.4f .. %.4f)" % gap("opt_model", 1, "encoder_fwd", 0, -1))
print("encoder_fwd start k -> opt_model end k (dynamics chain length): median %.4f (%.4f .. %.4f)" % gap("encoder_fwd", 0, "opt_model", 1, 0))
print("imagine_fwd start k -> opt_actor end k (behaviour chain length): median %.4f (%.4f .. %.4f)" % gap("imagine_fwd", 0, "opt_actor", 1, 0))
print({k: round(v[0], 4) for k, v in eng.timer_summary().items()})

"""Per-chunk timeline of the behaviour chain from a kernel trace ("Chunked behaviour chain").

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 20 --warmup 10 --no-secondary --no-cpu-baseline
    python3 tools/chunk_timeline.py DIR [steps-from-the-end, default 2]

For the last steps of the run: every launch of the two imagination scans, the fused heads and the tall dense backward
chains (actor hidden chain, critic) with its hardware queue, start and end (us from the step's first scan launch), and how
much of each heads / chain launch ran while a scan launch was running.  A heads chunk that starts only after the scan's last
chunk has ended shares a hardware queue with the scan (or the overlap stream is busy): the plan then buys nothing.

The grouped weight-gradient launches and their reduces are listed too, named by the hardware queue they run on: `actor` on
the queue of the backward scan (the behaviour stream), `critic` on the queue of the critic's backward chain, `model` on any
other; the summary gives their mean durations and where the actor's launch starts and ends relative to the critic's."""
import csv
import glob
import os
import sys

src = sys.argv[1]
last = int(sys.argv[2]) if len(sys.argv) > 2 else 2
path = src if src.endswith(".csv") else glob.glob(os.path.join(src, "**", "*_kernel_trace.csv"), recursive=True)[0]
KINDS = (("imagine_fwd_kernel", "scan_fwd"), ("imagine_bwd_kernel", "scan_bwd"), ("img_heads_kernel", "heads"),
         ("mlp_bwd_tall_kernel", "chain_bwd"), ("wgrad_wide_kernel", "wgrad"), ("wgrad_wide_reduce_kernel", "wgrad_red"),
         ("wgrad_grouped_reduce_kernel", "wgrad_red"))
WG = ("wgrad", "wgrad_red")
rows = []
for r in csv.DictReader(open(path)):
    kind = next((k for pat, k in KINDS if pat in r["Kernel_Name"]), None)
    if kind:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, r.get("Queue_Id", "?")))
rows.sort()
# a step starts at a forward-scan launch that follows a launch of another kind
def prev_kind(i):
    return next((rows[j][2] for j in range(i - 1, -1, -1) if rows[j][2] not in WG), None)


starts = [i for i, r in enumerate(rows) if r[2] == "scan_fwd" and prev_kind(i) not in ("scan_fwd", "heads")]
wg_dur, rel = {}, []
total = {"heads": [0.0, 0.0], "chain_bwd": [0.0, 0.0]}
for s, e in list(zip(starts, starts[1:] + [len(rows)]))[-last - 1:-1]:
    step = rows[s:e]
    t0 = step[0][0]
    print(f"step at {t0} ns: {len(step)} launches")
    bh = next((q for _, _, k, q in step if k == "scan_bwd"), None)
    side = next((q for _, _, k, q in step if k == "chain_bwd" and q != bh), None)
    who = lambda q: "actor" if q == bh else ("critic" if q == side else "model")
    span = {}
    for a, b, kind, q in step:
        if kind in WG:
            wg_dur.setdefault((kind, who(q)), []).append((b - a) / 1e3)
            if kind == "wgrad":
                span[who(q)] = (a, b)
            kind = f"{kind}[{who(q)}]"
        over = ""
        if kind in total:
            scan = "scan_fwd" if kind == "heads" else "scan_bwd"
            ov = sum(max(0, min(b, b2) - max(a, a2)) for a2, b2, k2, _ in step if k2 == scan)
            total[kind][0] += ov / 1e3
            total[kind][1] += (b - a) / 1e3
            over = f"   {ov / 1e3:7.1f} us under {scan}"
        print(f"  {kind:17s} queue {q:>3s}  {(a - t0) / 1e3:8.1f} .. {(b - t0) / 1e3:8.1f} us  ({(b - a) / 1e3:6.1f}){over}")
    if "actor" in span and "critic" in span:
        rel.append(((span["actor"][0] - span["critic"][0]) / 1e3, (span["actor"][1] - span["critic"][1]) / 1e3))
for (kind, w), v in sorted(wg_dur.items()):
    print(f"{kind}[{w}]: mean {sum(v) / len(v):.1f} us, min {min(v):.1f}, max {max(v):.1f} over {len(v)} launches")
if rel:
    print("actor's wgrad against the critic's: starts " + ", ".join(f"{x:+.1f}" for x, _ in rel) + " us after its start, ends "
          + ", ".join(f"{y:+.1f}" for _, y in rel) + " us after its end")
for kind, (ov, dur) in total.items():
    if dur:
        print(f"{kind}: {ov:.1f} of {dur:.1f} us ({100 * ov / dur:.0f} %) ran under a scan launch (chain_bwd includes the critic's chains)")

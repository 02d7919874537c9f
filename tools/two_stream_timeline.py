#!/usr/bin/env python3
"""The window between the projection and the compositing of the bench step, on both streams, from a
`rocprofv3 --kernel-trace --output-format csv` directory: when the SH forward and each list kernel start and end
relative to the end of `project_fwd_kernel`, on which queue, and what of the two chains overlaps.
    python tools/two_stream_timeline.py <dir> [label]   -> medians over the timed steps, and the median step's timeline"""
import csv
import glob
import statistics as st
import sys

d = sys.argv[1]
label = sys.argv[2] if len(sys.argv) > 2 else d
K = []
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    K += list(csv.DictReader(open(f)))
for r in K:
    r["a"], r["b"], r["q"], r["n"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), r["Kernel_Name"]
K.sort(key=lambda r: r["a"])
proj = [i for i, r in enumerate(K) if "project_fwd" in r["n"]]
is_list = lambda r: "gsr_bsort::" in r["n"] or "gsr_p2::" in r["n"] or "tile_jobs" in r["n"]  # noqa: E731
is_sh = lambda r: "sh16_fwd" in r["n"] or "sh_fwd_kernel" in r["n"]  # noqa: E731
steps = []
for n in range(len(proj) // 4, len(proj) - 1):  # (the warm-up steps come first)
    it = K[proj[n]:proj[n + 1]]
    pe = it[0]["b"]
    comp = [r for r in it if "raster_fwd" in r["n"]]
    sh = [r for r in it if is_sh(r)]
    lists = [r for r in it if is_list(r)]
    if not comp or not sh or not lists:
        continue
    window = [r for r in it[1:] if r["a"] < comp[0]["a"]]
    l0, l1 = min(r["a"] for r in lists), max(r["b"] for r in lists)
    both = sum(max(0, min(r["b"], s["b"]) - max(r["a"], s["a"])) for r in lists for s in window if not is_list(s))
    steps.append({
        "step": (K[proj[n + 1]]["a"] - it[0]["a"]) / 1e3,
        "window": (comp[0]["a"] - pe) / 1e3,
        "sh_dur": (sh[0]["b"] - sh[0]["a"]) / 1e3,
        "sh_start": (sh[0]["a"] - pe) / 1e3,
        "lists_busy": sum(r["b"] - r["a"] for r in lists) / 1e3,
        "lists_start": (l0 - pe) / 1e3,
        "lists_span": (l1 - l0) / 1e3,
        "colour_busy": sum(r["b"] - r["a"] for r in window if not is_list(r)) / 1e3,
        "overlap": both / 1e3,
        "queues": len({r["q"] for r in window}),
        "rows": [(r["q"], (r["a"] - pe) / 1e3, (r["b"] - r["a"]) / 1e3, r["n"][:60]) for r in window + comp[:1]],
    })
if not steps:
    sys.exit(f"{label}: no complete step found")
keys = ("step", "window", "sh_dur", "sh_start", "lists_busy", "lists_start", "lists_span", "colour_busy", "overlap", "queues")
print(f"{label}: {len(steps)} steps; medians, us: " + "  ".join(f"{k}={st.median(s[k] for s in steps):.1f}" for k in keys))
mid = sorted(steps, key=lambda s: s["window"])[len(steps) // 2]
print(f"  the step with the median window ({mid['window']:.1f} us); times from the end of project_fwd_kernel")
print("  queue  start_us   dur_us  kernel")
for q, a, dur, name in mid["rows"]:
    print(f"  {q:>5} {a:9.1f} {dur:8.1f}  {name}")

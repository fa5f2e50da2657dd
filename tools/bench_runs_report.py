"""Labelled bench.py result lines (a label line, then the JSON line of that run, ...) ->
median and spread (max - min) of us per step per label: python tools/bench_runs_report.py FILE"""
import json
import statistics
import sys

runs, lab = {}, None
for line in open(sys.argv[1]):
    line = line.strip()
    if line.startswith("{"):
        runs.setdefault(lab, []).append(json.loads(line))
    elif line:
        lab = line
for lab, rs in runs.items():
    us = [r["ms_per_step"] * 1e3 for r in rs]
    print(f"{lab:28s} n={len(us)}  median {statistics.median(us):.3f} us  spread (max-min) {max(us) - min(us):.3f}"
          f"  runs {' '.join(f'{u:.3f}' for u in us)}")
    for r in rs:
        if "roofline" in r:
            o = r.get("overlapped_launches", {}).get("ms_per_step")
            print(f"{'':28s} --full: roofline.kernel_us_avg {r['roofline']['kernel_us_avg']:.3f}"
                  f"  overlapped_launches {o * 1e3 if o else float('nan'):.3f} us  headline {r['ms_per_step'] * 1e3:.3f} us")

"""Steady-state extract of a rocprofv3 kernel trace of bench.py:
python tools/launch_chain_trace.py <kernel_trace.csv> <us per step of that run>"""
import csv
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1])) if "quad_rollout_rows_kernel" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
k = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), r.get("Stream_Id", "?")) for r in rows]
# the last 1000 launches: the timed graph replay
k = k[-1000:]
dur = [e - s for s, e, _, _ in k]
step = (k[-1][0] - k[0][0]) / (len(k) - 1)
over = sum(1 for a, b in zip(k, k[1:]) if b[0] < a[1])
print(f"quad_rollout_rows_kernel launches in the trace: {len(rows)}; the last {len(k)} (one graph replay):")
print(f"  average kernel duration      {sum(dur) / len(dur) / 1e3:.3f} us (min {min(dur) / 1e3:.3f}, max {max(dur) / 1e3:.3f})")
print(f"  average start-to-start       {step / 1e3:.3f} us")
print(f"  kernel i+1 starts before kernel i ends: {over} of {len(k) - 1} pairs")
print(f"  hardware queues seen: {sorted(set(q for _, _, q, _ in k))}")
if len(sys.argv) > 2:
    print(f"  bench.py of the same (profiled) run: {sys.argv[2]} us per step")
t0 = k[500][0]
print("  twelve consecutive launches (us from the first start; queue):")
for s, e, q, st in k[500:512]:
    print(f"    start {(s - t0) / 1e3:8.3f}  end {(e - t0) / 1e3:8.3f}  dur {(e - s) / 1e3:6.3f}  queue {q}")

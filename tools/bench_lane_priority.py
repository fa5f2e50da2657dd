"""bench.py with the lane-priority measurement hook set first, optionally in a
process that has already used CROWD other streams:
CROWD=8 python tools/bench_lane_priority.py MODE <bench.py arguments>"""
import os
import runpy
import sys

sys.path.insert(0, os.getcwd())
mode = int(sys.argv[1])
sys.argv = ["bench.py"] + sys.argv[2:]
from apg_trajectory_tracking_amd import _capi  # noqa: E402
assert _capi.lib().apg_launch_chain_set_lane_priority(mode) == 0
crowd = int(os.environ.get("CROWD", "0"))
if crowd:
    import torch
    keep = []
    for _ in range(crowd):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            keep.append(torch.ones(1024, device="cuda") * 2)
    torch.cuda.synchronize()
runpy.run_path("bench.py", run_name="__main__")

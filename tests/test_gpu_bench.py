"""bench.py's plain run on the GPU: exactly --steps timed steps, a lean line,
and --dump-outputs writing what the timed launches computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu


def _bench(*argv):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *argv],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_times_its_steps_and_dumps_the_last_step(tmp_path):
    """1 200 steps = a graph of 1 000 replayed once and one of 200; the last
    timed step ran buffer set 199 % 20 = 19.  Two runs with the same arguments
    dump the same arrays, and those are what one eager launch on set 19 returns."""
    from apg_trajectory_tracking_amd import functional as F, synthetic
    from apg_trajectory_tracking_amd.dynamics.quad_dynamics_flightmare import (
        FlightmareDynamics)
    runs = [_bench("--gpus", "1", "--steps", "1200", "--warmup", "5",
                   "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    d = runs[0]
    assert d["steps"] == 1200 and d["config"]["timed_steps"] == 1200
    assert d["config"]["replays"] == 2
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 65536 * 10 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for key in ("roofline", "cpu_baseline", "train_step", "secondary", "steps_summary"):
        assert key not in d, key                      # measured with --full only
    a, b = ({n: np.load(tmp_path / r / f"{n}.npy") for n in ("loss", "grad_actions")}
            for r in ("a", "b"))
    assert sorted(os.listdir(tmp_path / "a")) == ["grad_actions.npy", "loss.npy"]
    for n in a:
        assert a[n].dtype == np.float32 and np.array_equal(a[n], b[n]), n

    dev = torch.device("cuda:0")
    s = synthetic.quad_polynomial_batch(65536, 10, 0.1, seed=1000 * 19)
    ref6 = torch.cat((s["ref"][:, :, :3], s["ref"][:, :, 6:9]), 2)
    res = F.quad_rollout_fwd_bwd(
        synthetic.to_packed_state(s["state0"]).to(dev),
        synthetic.to_packed_seq(s["actions"]).to(dev),
        synthetic.to_packed_seq(ref6).to(dev), 0.1, FlightmareDynamics().params,
        layout="packed", want_grad_state0=False)
    assert np.array_equal(a["grad_actions"], res["grad_actions"].cpu().numpy())
    assert abs(a["loss"][0] - res["loss"].item()) <= 1e-6 * abs(res["loss"].item())

"""GPU-box validation of schema admission on the benchmark's wire path.

Like the other test_gpu_host files this validates the host, not a kernel:
the bench spawns the standalone apiserver, which validates HealthChecks by
default, so a short bench run with validation on and one with it off must
both complete and must leave the same persisted status counters. Nothing
here touches the device beyond what bench.py itself does.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _bench(dump_dir, validation):
    env = {k: v for k, v in os.environ.items() if k != "AM_SCHEMA_VALIDATION"}
    if not validation:
        env["AM_SCHEMA_VALIDATION"] = "0"
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--crs", "50", "--steps", "2", "--warmup", "1",
         "--dump-outputs", str(dump_dir)],
        capture_output=True, text=True, timeout=300, cwd=REPO, env=env,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    data = json.loads(out.stdout.strip().splitlines()[-1])
    assert data["metric"] == "sustained_healthcheck_cycles_per_sec"
    assert data["value"] > 0
    return np.load(os.path.join(dump_dir, "healthcheck_status.npy"))


def test_validation_changes_no_persisted_counter_on_the_wire_path(tmp_path):
    validated = _bench(tmp_path / "on", validation=True)
    stored_as_given = _bench(tmp_path / "off", validation=False)
    assert validated.shape == stored_as_given.shape == (50, 8)
    assert validated[:, 5].min() >= 4  # settle + warmup + two timed waves
    assert np.array_equal(validated, stored_as_given)

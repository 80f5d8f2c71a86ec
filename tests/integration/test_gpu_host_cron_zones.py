"""GPU-box validation of cron time zones.

Like the other test_gpu_host files this validates the host, not a kernel:
named zones only work where a zone database is found (the system's or the
``tzdata`` package), so the benchmark host must load the zones the suite
uses and give the pinned instants; and a short bench run, whose fleet is 30%
cron CRs, must complete with the zone-aware parser in the cron branch.
Nothing here touches the device beyond what bench.py itself does.
"""
import json
import os
import subprocess
import sys
from datetime import timezone
from zoneinfo import ZoneInfo

import numpy as np
import pytest

from active_monitor_amd.engine.cronx import parse_standard
from tests.cron_zone_cases import PINNED, ZONES, instant

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize("name", ZONES)
def test_host_zone_database_has_the_zone(name):
    """A failure here is a finding about the host's zone database."""
    assert ZoneInfo(name).key == name
    assert parse_standard(f"CRON_TZ={name} @daily").zone == ZoneInfo(name)


def test_pinned_instants_hold_on_gpu_host():
    for spec, after, expected in PINNED:
        got = parse_standard(spec).next(instant(after))
        assert got == instant(expected), (spec, after, got.astimezone(timezone.utc).isoformat())


def test_short_bench_runs_every_cr_with_the_new_cron_branch(tmp_path):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--crs", "50", "--steps", "2", "--warmup", "1",
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    data = json.loads(out.stdout.strip().splitlines()[-1])
    assert data["metric"] == "sustained_healthcheck_cycles_per_sec"
    status = np.load(os.path.join(tmp_path, "healthcheck_status.npy"))
    assert status.shape == (50, 8)
    assert status[:, 5].min() >= 4  # totalHealthCheckRuns, cron CRs included

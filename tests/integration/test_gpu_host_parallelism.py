"""GPU-box validation of bounded execution.

Like the other test_gpu_host files this validates the host, not a kernel:
how many processes a fleet of checks has alive at once, and whether two
checks that share a mutex ever overlap, depends on the host's fork, pipes
and scheduler, so it is measured there: six checks, ``max_processes=4``,
two of them exclusive of each other.
"""
import asyncio

import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.workflow import LocalWorkflowEngine

from .test_bounded_fleet import peak_check

pytestmark = pytest.mark.gpu


def test_fleet_of_six_under_max_processes_with_two_exclusive_checks(run, tmp_path):
    async def go():
        client = MemoryClient(MemoryApiServer())
        engine = LocalWorkflowEngine(client, ttl_seconds=None, max_processes=4)
        manager = Manager(client, max_workers=4)
        await engine.start()
        await manager.start()
        try:
            for i in range(6):
                await client.create(peak_check(i, tmp_path, mutex="device" if i < 2 else None))
            for _ in range(3000):
                checks = await client.list(API_VERSION, "HealthCheck", "health")
                if [(c.get("status") or {}).get("successCount", 0) for c in checks] == [1] * 6:
                    return engine.stats()
                await asyncio.sleep(0.01)
            raise AssertionError([c.get("status") for c in checks])
        finally:
            await manager.stop()
            await engine.stop()

    stats = run(go(), timeout=45)
    seen = [int(n) for n in (tmp_path / "peak").read_text().split()]
    assert len(seen) == 6
    assert max(seen) == 4
    assert stats["postponed_total"] == 1  # the second holder of the mutex
    assert (stats["running"], stats["queued"], stats["processes"]) == (0, 0, 0)
    # what the two exclusive checks wrote, in order: one span, then the other
    spans = [line.split() for line in (tmp_path / "spans").read_text().splitlines()]
    exclusive = [(what, i) for what, i in spans if i in ("0", "1")]
    assert [what for what, _ in exclusive] == ["start", "end", "start", "end"]
    assert exclusive[0][1] == exclusive[1][1] != exclusive[2][1] == exclusive[3][1]

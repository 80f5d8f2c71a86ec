"""GPU-box validation of HTTP probes.

Like the other test_gpu_host files this validates the host, not a kernel:
eight HealthChecks probe one server on the box's loopback through the full
controller loop, and what is host-dependent is the loopback itself and the
scheduler that carries eight sockets on one event loop. One round, under a
time limit of its own; nothing here touches the device.
"""
import asyncio

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.workflow import LocalWorkflowEngine
from tests.probeserver import ProbeServer, Route

from .conftest import make_hc

pytestmark = pytest.mark.gpu

WF = ("argoproj.io/v1alpha1", "Workflow")


def test_eight_checks_probe_one_server_on_gpu_host(run):
    async def go():
        routes = {"/healthz": Route(body=b'{"status":"ok"}', delay=0.05),
                  "/broken": Route(500, "Internal Server Error", body=b"boom", delay=0.05)}
        async with ProbeServer(routes) as srv:
            client = MemoryClient(MemoryApiServer())
            engine = LocalWorkflowEngine(client, ttl_seconds=None, max_processes=1)
            manager = Manager(client, max_workers=4)
            await engine.start()
            await manager.start()
            try:
                for i in range(8):
                    path = "/broken" if i in (2, 5) else "/healthz"
                    await client.create(make_hc(
                        name=f"probe-{i}", repeat=3600, timeout=20,
                        inline=yaml.safe_dump({
                            "apiVersion": WF[0], "kind": WF[1],
                            "spec": {"entrypoint": "probe", "templates": [
                                {"name": "probe", "http": {
                                    "url": f"{srv.url}{path}?check={i}",
                                    "timeoutSeconds": 10}}]}})))
                statuses = {}
                for _ in range(2000):
                    for obj in await client.list(API_VERSION, "HealthCheck", "health"):
                        st = obj.get("status") or {}
                        if st.get("successCount", 0) + st.get("failedCount", 0) >= 1:
                            statuses[obj["metadata"]["name"]] = st
                    if len(statuses) == 8:
                        break
                    await asyncio.sleep(0.01)
                settled = await srv.settled()
                for _ in range(500):
                    if not engine.stats()["running"]:
                        break
                    await asyncio.sleep(0.01)
                wfs = await client.list(*WF, "health")
                return statuses, srv, settled, engine.stats(), wfs
            finally:
                await manager.stop()
                await engine.stop()

    statuses, srv, settled, stats, wfs = run(go(), timeout=45)
    assert sorted(statuses) == [f"probe-{i}" for i in range(8)]
    passed = sorted(n for n, st in statuses.items() if st.get("successCount", 0) == 1)
    failed = sorted(n for n, st in statuses.items() if st.get("failedCount", 0) == 1)
    assert passed == [f"probe-{i}" for i in (0, 1, 3, 4, 6, 7)]
    assert failed == ["probe-2", "probe-5"]
    assert all(st.get("successCount", 0) + st.get("failedCount", 0) == 1
               for st in statuses.values())
    # one round: one request each, over a connection of its own, all closed
    assert sorted(srv.paths()) == sorted(
        f"{'/broken' if i in (2, 5) else '/healthz'}?check={i}" for i in range(8))
    assert srv.connections == 8 and settled and srv.open == 0
    assert srv.closed_early == []
    assert stats["running"] == 0 and stats["queued"] == 0 and stats["processes"] == 0
    assert len(wfs) == 8
    for wf in wfs:
        (node,) = wf["status"]["nodes"].values()
        assert node["type"] == "HTTP"
    messages = sorted(wf["status"].get("message", "") for wf in wfs)
    assert messages == [""] * 6 + ["received non-2xx response code: 500"] * 2

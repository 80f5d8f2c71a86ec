"""GPU-box validation of workflow logs.

Like test_gpu_host_workflows.py this validates the host, not a kernel: the
DAG example runs through the full controller loop with a log store and every
step's output is served over the wire, and a leaf whose shell left a child
holding its pipes still ends with its output kept when the deadline kills the
group — pipes and process groups being the host-dependent part. One run each,
under a time limit of its own; nothing here touches the device.
"""
import asyncio
import os
import pathlib
import time

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import LocalWorkflowEngine
from active_monitor_amd.workflow.logs import LogStore

pytestmark = pytest.mark.gpu

EXAMPLES = pathlib.Path(__file__).parents[2] / "examples"
WF = ("argoproj.io/v1alpha1", "Workflow")


def test_dag_example_logs_over_the_wire_on_gpu_host(run):
    doc = yaml.safe_load((EXAMPLES / "inline-dag.yaml").read_text())
    meta = doc["metadata"]

    async def go():
        server = MemoryApiServer()
        client = MemoryClient(server)
        logs = LogStore()
        engine = LocalWorkflowEngine(client, ttl_seconds=None, logs=logs)
        frontend = ApiServerFrontend(server, logs=logs)
        manager = Manager(client, max_workers=2)
        await frontend.start()
        await engine.start()
        await manager.start()
        http = HttpClient(frontend.url, qps=0)
        await http.start()
        try:
            await client.create(doc)
            status = {}
            for _ in range(1000):
                obj = await client.get(API_VERSION, "HealthCheck",
                                       meta["namespace"], meta["name"])
                status = obj.get("status") or {}
                if status.get("successCount", 0) >= 1 or status.get("failedCount", 0) >= 1:
                    break
                await asyncio.sleep(0.02)
            assert status.get("successCount", 0) >= 1, status
            (wf,) = await client.list(*WF, meta["namespace"])
            pods = [n for n in wf["status"]["nodes"].values() if n["type"] == "Pod"]
            assert sorted(n["displayName"] for n in pods) == ["high", "low", "report", "sample"]
            served = {}
            for n in pods:
                served[n["displayName"]] = b"".join([
                    c async for c in http.logs(meta["namespace"], wf["metadata"]["name"],
                                               node=n["id"])])
            return served
        finally:
            await http.close()
            await manager.stop()
            await engine.stop()
            await frontend.stop()
            logs.close()

    served = run(go(), timeout=30)
    assert all(served.values()), served  # every Pod node said something
    assert served["sample"] == b"17\n"
    assert served["low"] == b"17 -ge 0: holds\n"
    assert served["high"] == b"17 -lt 500: holds\n"
    assert served["report"] == b"queue depth 17 is within bounds\n"


def _surviving(pid):
    """False once the process is dead — reaped, or a zombie that the init
    process has yet to reap (it runs nothing and holds no pipe)."""
    try:
        with open(f"/proc/{pid}/stat") as f:
            # pid (comm) state ...; comm may hold spaces and parentheses
            return f.read().rpartition(")")[2].split()[0] != "Z"
    except (OSError, IndexError):
        return False


def test_orphaning_shell_deadline_keeps_the_log_on_gpu_host(run, tmp_path):
    """The shell exits at once; only its background child, which still holds
    the leaf's pipes, keeps the leaf running until the deadline."""
    pidfile = tmp_path / "pids"

    async def go():
        client = MemoryClient(MemoryApiServer())
        logs = LogStore()
        engine = LocalWorkflowEngine(client, logs=logs)
        await engine.start()
        try:
            await client.create({
                "apiVersion": WF[0], "kind": WF[1],
                "metadata": {"name": "doomed", "namespace": "health"},
                "spec": {
                    "entrypoint": "main",
                    "activeDeadlineSeconds": 1,
                    "templates": [{"name": "main", "container": {"command": [
                        "sh", "-c", f"sleep 30 & echo $$ $! > {pidfile}; echo started"]}}],
                },
            })
            status = {}
            for _ in range(500):
                wf = await client.get(*WF, "health", "doomed")
                status = wf.get("status") or {}
                if status.get("phase") in ("Succeeded", "Failed"):
                    break
                await asyncio.sleep(0.02)
            log = b"".join([c async for c in logs.read("health", "doomed", follow=True)])
            return status, log
        finally:
            await engine.stop()
            logs.close()

    status, log = run(go(), timeout=15)
    assert status["phase"] == "Failed" and status["message"] == "deadline exceeded"
    assert log == b"started\n"
    pids = [int(p) for p in pidfile.read_text().split()]
    assert len(pids) == 2
    deadline = time.monotonic() + 2.0
    alive = list(pids)
    while alive and time.monotonic() < deadline:
        alive = [pid for pid in alive if _surviving(pid)]
        if alive:
            time.sleep(0.02)
    assert not alive, f"still running two seconds after the Failed phase: {alive}"

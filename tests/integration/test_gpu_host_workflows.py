"""GPU-box validation of the local executor's Argo surface.

Like test_gpu_host.py this validates the host, not a kernel: the DAG and
loops examples complete through the full controller loop there, and
cancelling a workflow kills its whole process group — process-group handling
being the host-dependent part. One run each; nothing here touches the device.
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
from active_monitor_amd.workflow import LocalWorkflowEngine

pytestmark = pytest.mark.gpu

EXAMPLES = pathlib.Path(__file__).parents[2] / "examples"
WF = ("argoproj.io/v1alpha1", "Workflow")


async def full_loop(relpath, timeout=30.0):
    doc = yaml.safe_load((EXAMPLES / relpath).read_text())
    meta = doc["metadata"]
    client = MemoryClient(MemoryApiServer())
    engine = LocalWorkflowEngine(client, ttl_seconds=None)
    await engine.start()
    manager = Manager(client, max_workers=2)
    await manager.start()
    try:
        await client.create(doc)
        deadline = time.monotonic() + timeout
        status = {}
        while time.monotonic() < deadline:
            obj = await client.get(API_VERSION, "HealthCheck", meta["namespace"], meta["name"])
            status = obj.get("status") or {}
            if status.get("successCount", 0) >= 1 or status.get("failedCount", 0) >= 1:
                break
            await asyncio.sleep(0.02)
        workflows = await client.list(*WF, meta["namespace"])
        return status, workflows
    finally:
        await manager.stop()
        await engine.stop()


def pods(workflows):
    assert len(workflows) == 1
    return sorted(n["displayName"] for n in workflows[0]["status"]["nodes"].values()
                  if n["type"] == "Pod" and n["phase"] == "Succeeded")


def test_dag_example_completes_on_gpu_host(run):
    status, workflows = run(full_loop("inline-dag.yaml"))
    assert status.get("successCount", 0) >= 1, status
    assert pods(workflows) == ["high", "low", "report", "sample"]


def test_loops_example_completes_on_gpu_host(run):
    status, workflows = run(full_loop("inline-loops.yaml"))
    assert status.get("successCount", 0) >= 1, status
    assert pods(workflows) == [
        "directory(0:/)", "directory(1:/tmp)", "directory(2:/etc)",
        "threshold(0)", "threshold(1)",
    ]


@pytest.mark.parametrize("tail", ["; wait", ""], ids=["waiting", "orphaning"])
def test_deadline_kills_process_group_on_gpu_host(run, tmp_path, tail):
    """``waiting``: the shell waits for its background child. ``orphaning``:
    the shell exits at once and only the child, which still holds the leaf's
    stdout, keeps the leaf running."""
    pidfile = tmp_path / "pids"

    async def go():
        client = MemoryClient(MemoryApiServer())
        engine = LocalWorkflowEngine(client)
        await engine.start()
        await client.create({
            "apiVersion": WF[0], "kind": WF[1],
            "metadata": {"name": "doomed", "namespace": "health"},
            "spec": {
                "entrypoint": "main",
                "activeDeadlineSeconds": 1,
                "templates": [{"name": "main", "container": {"command": [
                    "sh", "-c", f"sleep 30 & echo $$ $! > {pidfile}{tail}"]}}],
            },
        })
        deadline = time.monotonic() + 15
        status = {}
        while time.monotonic() < deadline:
            wf = await client.get(*WF, "health", "doomed")
            status = wf.get("status") or {}
            if status.get("phase") in ("Succeeded", "Failed"):
                break
            await asyncio.sleep(0.02)
        await engine.stop()
        return status

    status = run(go())
    assert status["phase"] == "Failed" and "deadline" in status["message"]
    pids = [int(p) for p in pidfile.read_text().split()]
    assert len(pids) == 2
    deadline = time.monotonic() + 2.0
    alive = list(pids)
    while alive and time.monotonic() < deadline:
        for pid in list(alive):
            try:
                os.kill(pid, 0)
            except ProcessLookupError:
                alive.remove(pid)
        if alive:
            time.sleep(0.02)
    assert not alive, f"still running two seconds after the Failed phase: {alive}"

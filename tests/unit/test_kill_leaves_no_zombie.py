"""A workflow that is reported Failed after its deadline has left nothing in
the process table: the kill path waits for the killed group to be empty,
also where a member of it had lost its parent and is reaped by init."""
import asyncio
import os
import time

import pytest

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine


@pytest.mark.parametrize("tail", ["; wait", ""], ids=["waiting", "orphaning"])
def test_group_is_empty_when_the_deadline_failure_is_reported(run, tmp_path, tail):
    pidfile = tmp_path / "pids"

    async def go():
        client = MemoryClient(MemoryApiServer())
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        await engine.start()
        try:
            await client.create({
                "apiVersion": WF_API_VERSION, "kind": WF_KIND,
                "metadata": {"name": "doomed", "namespace": "health"},
                "spec": {"entrypoint": "main", "activeDeadlineSeconds": 1, "templates": [
                    {"name": "main", "container": {"command": [
                        "sh", "-c", f"sleep 30 & echo $$ $! > {pidfile}{tail}"]}}]},
            })
            give_up = time.monotonic() + 15
            while time.monotonic() < give_up:
                wf = await client.get(WF_API_VERSION, WF_KIND, "health", "doomed")
                status = wf.get("status") or {}
                if status.get("phase") == "Failed":
                    # looked at in the same step of the loop that saw Failed
                    shell, child = [int(p) for p in pidfile.read_text().split()]
                    return status, [pid for pid in (shell, child) if _exists(pid)]
                await asyncio.sleep(0.02)
            raise AssertionError("the workflow did not fail")
        finally:
            await engine.stop()

    status, left = run(go(), timeout=30)
    assert status["message"] == "deadline exceeded"
    assert left == []


def _exists(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    return True

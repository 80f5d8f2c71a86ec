"""GPU-box validation of step deadlines.

Like the other test_gpu_host files this validates the host, not a kernel:
four HealthChecks run one round through the full controller loop, and what
is host-dependent is the kill of a leaf's process group and its reaping
under the box's real scheduler and init. One round, under a time limit of
its own; nothing here touches the device.
"""
import asyncio
import os

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.workflow import LocalWorkflowEngine

from .conftest import make_hc

pytestmark = pytest.mark.gpu

WF = ("argoproj.io/v1alpha1", "Workflow")


def inline(spec):
    return yaml.safe_dump({"apiVersion": WF[0], "kind": WF[1], "spec": spec})


def checks(pids):
    """The four checks by name; the two that hang record the pid of their
    leaf, the leader of its group, under ``pids``."""
    say = {"name": "say", "inputs": {"parameters": [{"name": "what"}]},
           "container": {"command": ["echo", "{{inputs.parameters.what}}"]}}
    return {
        # the first attempt hangs and is cut, the second answers
        "hang-then-retry": {"entrypoint": "flaky", "templates": [{
            "name": "flaky", "activeDeadlineSeconds": 1, "retryStrategy": {"limit": 1},
            "script": {"command": ["sh"], "source": (
                f'if [ "{{{{retries}}}}" = 0 ]; then echo $$ > {pids}/retry; sleep 30 & '
                'sleep 30; fi\necho ok\n')}}]},
        "step-timeout": {"entrypoint": "hang", "templates": [{
            "name": "hang", "timeout": "1s",
            "script": {"command": ["sh"], "source":
                       f"echo $$ > {pids}/timeout\nsleep 30 &\nsleep 30\n"}}]},
        "continue-on": {"entrypoint": "main", "templates": [
            {"name": "main", "steps": [
                [{"name": "probe", "template": "bad", "continueOn": {"failed": True}}],
                [{"name": "diagnose", "template": "say",
                  "when": "{{steps.probe.status}} == Failed",
                  "arguments": {"parameters": [{"name": "what", "value": "diagnostics"}]}}]]},
            {"name": "bad", "container": {"command": ["sh", "-c", "exit 3"]}}, say]},
        "sequence": {"entrypoint": "main", "templates": [
            {"name": "main", "steps": [[
                {"name": "probe", "template": "say", "withSequence": {"count": 3},
                 "arguments": {"parameters": [{"name": "what", "value": "{{item}}"}]}}]]},
            say]},
    }


def group_is_gone(pgid):
    try:
        os.killpg(pgid, 0)
    except ProcessLookupError:
        return True
    return False


def test_four_checks_contain_their_steps_on_gpu_host(run, tmp_path):
    specs = checks(tmp_path)

    async def go():
        client = MemoryClient(MemoryApiServer())
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        manager = Manager(client, max_workers=4)
        await engine.start()
        await manager.start()
        try:
            for name, spec in specs.items():
                await client.create(make_hc(name=name, repeat=3600, timeout=20,
                                            inline=inline(spec)))
            statuses = {}
            for _ in range(2000):
                for obj in await client.list(API_VERSION, "HealthCheck", "health"):
                    st = obj.get("status") or {}
                    if st.get("successCount", 0) + st.get("failedCount", 0) >= 1:
                        statuses[obj["metadata"]["name"]] = st
                if len(statuses) == len(specs):
                    break
                await asyncio.sleep(0.01)
            # each sleep had more than 20 s left when its check was counted
            gone = {f: group_is_gone(int((tmp_path / f).read_text()))
                    for f in ("retry", "timeout")}
            for _ in range(500):
                if not engine.stats()["running"]:
                    break
                await asyncio.sleep(0.01)
            return statuses, gone, engine.stats(), await client.list(*WF, "health")
        finally:
            await manager.stop()
            await engine.stop()

    statuses, gone, stats, wfs = run(go(), timeout=45)
    assert sorted(statuses) == sorted(specs)
    counts = {name: (st.get("successCount", 0), st.get("failedCount", 0))
              for name, st in statuses.items()}
    assert counts == {"hang-then-retry": (1, 0), "step-timeout": (0, 1),
                      "continue-on": (1, 0), "sequence": (1, 0)}
    assert gone == {"retry": True, "timeout": True}
    assert stats["running"] == 0 and stats["queued"] == 0 and stats["processes"] == 0

    by_check = {wf["metadata"]["generateName"]: wf["status"] for wf in wfs}
    assert len(wfs) == 4
    assert by_check["step-timeout-wf-"]["phase"] == "Failed"
    assert by_check["step-timeout-wf-"]["message"] == "Step exceeded its deadline"
    retried = {n["displayName"]: n for n in by_check["hang-then-retry-wf-"]["nodes"].values()}
    assert [(n["phase"], n["message"]) for name, n in sorted(retried.items())
            if name.endswith(")")] == [
        ("Failed", "Pod was active on the node longer than the specified deadline"),
        ("Succeeded", "")]
    continued = {n["displayName"]: n["phase"]
                 for n in by_check["continue-on-wf-"]["nodes"].values()}
    assert continued["probe"] == "Failed" and continued["diagnose"] == "Succeeded"
    looped = sorted(n["displayName"] for n in by_check["sequence-wf-"]["nodes"].values()
                    if n["type"] == "Pod")
    assert looped == ["probe(0:0)", "probe(1:1)", "probe(2:2)"]

"""GPU-box validation of shared templates.

Like the other test_gpu_host files this validates the host, not a kernel:
four checks share one WorkflowTemplate, each leaf is a forked shell that
appends to one file, and a second round is triggered by run requests after
the template was edited. Whether every leaf of a round saw that round's text,
and whether the engine ends with nothing alive, depends on the host's fork,
pipes and scheduler, so it is checked there.
"""
import asyncio

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.api.runrequest import RUN_REQUESTED_ANNOTATION, new_run_token
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.workflow import LocalWorkflowEngine

pytestmark = pytest.mark.gpu

ARGO = "argoproj.io/v1alpha1"
WHO = ["alpha", "beta", "gamma", "delta"]


def shared(text, path):
    return {"entrypoint": "main",
            "arguments": {"parameters": [{"name": "who"}]},
            "templates": [{"name": "main", "container": {"command": [
                "sh", "-c", f'echo "{text} $0" >> {path}', "{{workflow.parameters.who}}"]}}]}


def check(who):
    return {
        "apiVersion": API_VERSION, "kind": "HealthCheck",
        "metadata": {"name": who, "namespace": "health"},
        "spec": {"repeatAfterSec": 600, "level": "cluster", "workflow": {
            "generateName": f"{who}-wf-", "workflowtimeout": 30,
            "resource": {"namespace": "health", "serviceAccount": "fleet-sa",
                         "source": {"inline": yaml.safe_dump({
                             "apiVersion": ARGO, "kind": "Workflow",
                             "spec": {"workflowTemplateRef": {"name": "shared"},
                                      "arguments": {"parameters": [
                                          {"name": "who", "value": who}]}}})}}}},
    }


def test_four_checks_share_a_template_across_an_edit_on_gpu_host(run, tmp_path):
    written = tmp_path / "written"

    async def all_succeeded(client, times):
        for _ in range(3000):
            checks = await client.list(API_VERSION, "HealthCheck", "health")
            if [(c.get("status") or {}).get("successCount", 0) for c in checks] == [times] * 4:
                return
            await asyncio.sleep(0.01)
        raise AssertionError([c.get("status") for c in checks])

    async def go():
        client = MemoryClient(MemoryApiServer())
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        manager = Manager(client, max_workers=4)
        await engine.start()
        await manager.start()
        try:
            await client.create({"apiVersion": ARGO, "kind": "WorkflowTemplate",
                                 "metadata": {"name": "shared", "namespace": "health"},
                                 "spec": shared("old", written)})
            for who in WHO:
                await client.create(check(who))
            await all_succeeded(client, 1)

            template = await client.get(ARGO, "WorkflowTemplate", "health", "shared")
            template["spec"] = shared("new", written)
            edited = await client.update(template)
            for _ in range(1000):  # until the engine's watch has delivered the edit
                cached = engine.cached_template("shared", "health")
                if cached["metadata"]["resourceVersion"] == \
                        edited["metadata"]["resourceVersion"]:
                    break
                await asyncio.sleep(0.01)
            for who in WHO:
                await client.patch(
                    API_VERSION, "HealthCheck", "health", who,
                    {"metadata": {"annotations": {RUN_REQUESTED_ANNOTATION: new_run_token()}}})
            await all_succeeded(client, 2)
            return engine.stats()
        finally:
            await manager.stop()
            await engine.stop()

    stats = run(go(), timeout=60)
    lines = written.read_text().splitlines()
    assert sorted(lines[:4]) == sorted(f"old {who}" for who in WHO)
    assert sorted(lines[4:]) == sorted(f"new {who}" for who in WHO)
    assert (stats["running"], stats["queued"], stats["processes"]) == (0, 0, 0)

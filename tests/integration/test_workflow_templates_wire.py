"""Shared templates over the wire: the standalone apiserver serves both
kinds, ``HttpClient`` reaches them, ``amctl`` shows them, and the sample's
two HealthChecks run through the whole controller loop with an engine and a
manager that are HTTP clients themselves."""
import asyncio
import pathlib

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.cmd.ctl import build_parser
from active_monitor_amd.cmd.ctl import run as ctl_run
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube.errors import NotFoundError
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.memory import MemoryApiServer
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import LocalWorkflowEngine

REPO = pathlib.Path(__file__).parents[2]
SAMPLE = REPO / "config" / "samples" / "activemonitor_v1alpha1_healthcheck_workflowtemplate.yaml"
ARGO = "argoproj.io/v1alpha1"


def template(kind, name, namespace=None, labels=None):
    meta = {"name": name}
    if namespace:
        meta["namespace"] = namespace
    if labels:
        meta["labels"] = labels
    return {"apiVersion": ARGO, "kind": kind, "metadata": meta, "spec": {"templates": [
        {"name": "ok", "container": {"command": ["true"]}}]}}


class Stack:
    async def __aenter__(self):
        self.server = MemoryApiServer()
        self.frontend = ApiServerFrontend(self.server)
        await self.frontend.start()
        self.client = HttpClient(self.frontend.url, qps=0)
        await self.client.start()
        return self

    async def __aexit__(self, *exc):
        await self.client.close()
        await self.frontend.stop()

    async def ctl(self, *argv):
        args = build_parser().parse_args(["--server", self.frontend.url, *argv])
        return await asyncio.wait_for(ctl_run(args), 30)


def test_both_rest_paths_serve_every_verb(run):
    async def go():
        async with Stack() as s:
            c = s.client
            base = f"/apis/{ARGO}"
            assert c._object_path(ARGO, "WorkflowTemplate", "health", "t") == \
                f"{base}/namespaces/health/workflowtemplates/t"
            # a cluster-scoped template has no namespace in its path
            assert c._object_path(ARGO, "ClusterWorkflowTemplate", "health", "t") == \
                f"{base}/clusterworkflowtemplates/t"

            for kind, ns in (("WorkflowTemplate", "health"), ("ClusterWorkflowTemplate", "")):
                sub = c.watch(ARGO, kind, ns or None)
                events = []

                async def read():
                    async for ev in sub:
                        events.append((ev["type"], ev["object"]["metadata"]["name"]))

                reader = asyncio.ensure_future(read())
                # a namespace in a cluster-scoped object is ignored
                await c.create(template(kind, "t", "health", {"team": "net"}))
                await c.create(template(kind, "u", ns or None))
                assert [o["metadata"]["name"] for o in await c.list(ARGO, kind, ns or None)] \
                    == ["t", "u"]
                assert [o["metadata"]["name"] for o in await c.list(
                    ARGO, kind, ns or None, label_selector="team=net")] == ["t"]
                got = await c.get(ARGO, kind, ns, "t")
                got["spec"]["templates"].append(
                    {"name": "more", "container": {"command": ["true"]}})
                await c.update(got)
                await c.patch(ARGO, kind, ns, "t", {"metadata": {"labels": {"team": "gpu"}}})
                got = await c.get(ARGO, kind, "anything" if not ns else ns, "t")
                assert len(got["spec"]["templates"]) == 2
                assert got["metadata"]["labels"] == {"team": "gpu"}
                assert "status" not in got
                await c.delete(ARGO, kind, ns, "t")
                with pytest.raises(NotFoundError) as err:
                    await c.get(ARGO, kind, ns, "t")
                assert f'{kind.lower()}s.argoproj.io "t" not found' in str(err.value)
                for _ in range(500):
                    if ("DELETED", "t") in events:
                        break
                    await asyncio.sleep(0.01)
                sub.close()
                reader.cancel()
                assert events == [("ADDED", "t"), ("ADDED", "u"), ("MODIFIED", "t"),
                                  ("MODIFIED", "t"), ("DELETED", "t")]

    run(go())


def test_sample_applies_shows_and_runs_through_the_controller_loop(run, capsys):
    async def go():
        async with Stack() as s:
            engine = LocalWorkflowEngine(s.client, ttl_seconds=None)
            manager = Manager(s.client, max_workers=2)
            await engine.start()
            await manager.start()
            try:
                assert await s.ctl("apply", "-f", str(SAMPLE)) == 0
                applied = capsys.readouterr().out.splitlines()
                for _ in range(2000):
                    checks = await s.client.list(API_VERSION, "HealthCheck", "health")
                    if [(c.get("status") or {}).get("successCount") for c in checks] == [1, 1]:
                        break
                    await asyncio.sleep(0.01)
                else:
                    raise AssertionError([c.get("status") for c in checks])
                workflows = await s.client.list(ARGO, "Workflow", "health")

                await s.client.create(template("ClusterWorkflowTemplate", "tools"))
                shown = {}
                for argv in (("get", "wftmpl"), ("get", "workflowtemplates", "-n", "health"),
                             ("get", "wftmpl", "-n", "elsewhere"),
                             ("get", "cwft"), ("get", "cwftmpl", "-n", "elsewhere"),
                             ("get", "clusterworkflowtemplate", "tools", "-o", "yaml"),
                             ("describe", "wftmpl", "net-checks"),
                             ("describe", "cwft", "tools"),
                             ("delete", "workflowtemplate", "net-checks"),
                             ("delete", "clusterworkflowtemplates", "tools", "-n", "x"),
                             ("get", "wftmpl", "net-checks")):
                    rc = await s.ctl(*argv)
                    shown[argv] = (rc, capsys.readouterr().out)
                return applied, workflows, shown, engine.stats()
            finally:
                await manager.stop()
                await engine.stop()

    applied, workflows, shown, stats = run(go(), timeout=60)
    assert applied == ["workflowtemplate/net-checks created",
                       "healthcheck/net-probe-gateway created",
                       "healthcheck/net-probe-pair created"]
    assert (stats["running"], stats["queued"], stats["processes"]) == (0, 0, 0)
    by_check = {wf["metadata"]["name"].rsplit("-", 1)[0]: wf["status"] for wf in workflows}
    assert set(by_check) == {"net-probe-gateway", "net-probe-pair"}
    gateway, pair = by_check["net-probe-gateway"], by_check["net-probe-pair"]
    assert gateway["phase"] == pair["phase"] == "Succeeded"
    assert gateway["storedWorkflowTemplateSpec"]["entrypoint"] == "main"
    assert sorted(pair["storedTemplates"]) == ["namespaced/net-checks/probe",
                                               "namespaced/net-checks/report"]
    (summary,) = [n for n in pair["nodes"].values() if n["displayName"] == "summary"]
    assert summary["outputs"]["result"] == "probed a.internal, probed b.internal"
    assert summary["templateRef"] == {"name": "net-checks", "template": "report"}

    rc, out = shown[("get", "wftmpl")]
    rows = [line.split() for line in out.splitlines()]
    assert rc == 0 and rows[0] == ["NAME", "TEMPLATES", "AGE"]
    assert rows[1][:2] == ["net-checks", "3"] and len(rows) == 2
    assert shown[("get", "workflowtemplates", "-n", "health")] == (rc, out)
    assert len(shown[("get", "wftmpl", "-n", "elsewhere")][1].splitlines()) == 1
    for argv in (("get", "cwft"), ("get", "cwftmpl", "-n", "elsewhere")):  # -n is ignored
        rc, out = shown[argv]
        assert rc == 0 and [line.split()[:2] for line in out.splitlines()] == [
            ["NAME", "TEMPLATES"], ["tools", "1"]]
    rc, out = shown[("get", "clusterworkflowtemplate", "tools", "-o", "yaml")]
    assert rc == 0 and yaml.safe_load(out)["kind"] == "ClusterWorkflowTemplate"
    rc, out = shown[("describe", "wftmpl", "net-checks")]
    assert rc == 0 and yaml.safe_load(out)["spec"]["entrypoint"] == "main"
    rc, out = shown[("describe", "cwft", "tools")]
    assert rc == 0 and yaml.safe_load(out)["metadata"]["name"] == "tools"
    assert shown[("delete", "workflowtemplate", "net-checks")] == (
        0, "workflowtemplate/net-checks deleted\n")
    assert shown[("delete", "clusterworkflowtemplates", "tools", "-n", "x")][0] == 0
    assert shown[("get", "wftmpl", "net-checks")][0] == 1  # it is gone


def test_logs_and_run_do_not_take_the_new_aliases():
    for command in ("logs", "run"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["--server", "http://x", command, "wftmpl", "name"])

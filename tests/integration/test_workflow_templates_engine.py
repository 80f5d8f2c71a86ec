"""Shared templates under ``LocalWorkflowEngine`` over the memory store: the
watch-fed cache, the snapshot a run keeps, admission from the effective spec,
the namespace filter and a durable store."""
import asyncio
import time

import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine

WF = (WF_API_VERSION, WF_KIND)
WFT = (WF_API_VERSION, "WorkflowTemplate")
TEMPLATE_KINDS = ("WorkflowTemplate", "ClusterWorkflowTemplate")


def sh(name, script):
    return {"name": name, "container": {"command": ["sh", "-c", script]}}


def wft(name, spec, namespace="health", cluster=False):
    meta = {"name": name}
    if not cluster:
        meta["namespace"] = namespace
    return {"apiVersion": WF_API_VERSION,
            "kind": "ClusterWorkflowTemplate" if cluster else "WorkflowTemplate",
            "metadata": meta, "spec": spec}


def workflow(name, spec, namespace="health"):
    return {"apiVersion": WF_API_VERSION, "kind": WF_KIND,
            "metadata": {"name": name, "namespace": namespace}, "spec": spec}


def health_check(name, spec):
    return {
        "apiVersion": API_VERSION, "kind": "HealthCheck",
        "metadata": {"name": name, "namespace": "health"},
        "spec": {"repeatAfterSec": 600, "level": "cluster", "workflow": {
            "generateName": f"{name}-wf-", "workflowtimeout": 30,
            "resource": {"namespace": "health", "serviceAccount": "sa",
                         "source": {"inline": yaml.safe_dump({
                             "apiVersion": WF_API_VERSION, "kind": WF_KIND,
                             "spec": spec})}}}},
    }


async def status_when(client, name, phases=("Succeeded", "Failed"), namespace="health",
                      timeout=15.0):
    deadline = time.monotonic() + timeout
    while time.monotonic() < deadline:
        status = (await client.get(*WF, namespace, name)).get("status") or {}
        if status.get("phase") in phases:
            return status
        await asyncio.sleep(0.01)
    raise AssertionError(f"{name} did not reach {phases}: {status}")


def pod_outputs(status):
    return [n["outputs"]["result"] for n in status["nodes"].values() if n["type"] == "Pod"]


def test_a_run_keeps_the_template_text_it_started_with(run):
    async def go():
        client = MemoryClient(MemoryApiServer())
        await client.create(wft("lib", {"entrypoint": "say", "templates": [
            sh("say", "sleep 0.3; echo old")]}))
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        await engine.start()
        try:
            await client.create(workflow("one", {"workflowTemplateRef": {"name": "lib"}}))
            running = await status_when(client, "one", ("Running",))
            assert running["storedWorkflowTemplateSpec"]["templates"][0]["name"] == "say"
            lib = await client.get(*WFT, "health", "lib")
            lib["spec"]["templates"] = [sh("say", "echo new")]
            await client.update(lib)
            first = await status_when(client, "one")
            await client.create(workflow("two", {"workflowTemplateRef": {"name": "lib"}}))
            second = await status_when(client, "two")
            await client.delete(*WFT, "health", "lib")
            await asyncio.sleep(0.05)
            await client.create(workflow("three", {"workflowTemplateRef": {"name": "lib"}}))
            return first, second, await status_when(client, "three")
        finally:
            await engine.stop()

    first, second, third = run(go())
    assert (first["phase"], pod_outputs(first)) == ("Succeeded", ["old"])
    assert (second["phase"], pod_outputs(second)) == ("Succeeded", ["new"])
    command = ["sh", "-c", "sleep 0.3; echo old"]
    assert first["storedWorkflowTemplateSpec"]["templates"][0]["container"]["command"] == command
    assert third["message"] == 'workflowtemplates.argoproj.io "lib" not found'


class DeafToTemplates(MemoryClient):
    """A client whose template watches never deliver anything: what the
    engine's cache looks like in the instant before an event arrives."""

    def watch(self, api_version, kind, namespace=None):
        if kind in TEMPLATE_KINDS:
            return MemoryClient(MemoryApiServer()).watch(api_version, kind, namespace)
        return super().watch(api_version, kind, namespace)


def test_template_and_workflow_created_in_the_same_instant(run):
    async def go(client):
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        await engine.start()
        try:
            # back to back, nothing awaited in between that yields
            await client.create(wft("lib", {"templates": [sh("say", "echo hello")]}))
            await client.create(workflow("wf", {"entrypoint": "main", "templates": [
                {"name": "main", "steps": [[
                    {"name": "s", "templateRef": {"name": "lib", "template": "say"}}]]}]}))
            status = await status_when(client, "wf")
            await client.create(workflow("gone", {"workflowTemplateRef": {"name": "nope"}}))
            return status, await status_when(client, "gone"), engine.template_reads
        finally:
            await engine.stop()

    status, _, _ = run(go(MemoryClient(MemoryApiServer())))
    assert (status["phase"], pod_outputs(status)) == ("Succeeded", ["hello"])
    # the cache never hears of it: one direct read finds it, and one
    # confirms that the other name is not there
    status, gone, reads = run(go(DeafToTemplates(MemoryApiServer())))
    assert (status["phase"], pod_outputs(status)) == ("Succeeded", ["hello"])
    assert gone["message"] == 'workflowtemplates.argoproj.io "nope" not found'
    assert reads == 2


class CountingClient(MemoryClient):
    def __init__(self, server):
        super().__init__(server)
        self.template_requests = 0

    async def get(self, api_version, kind, *args, **kwargs):
        self.template_requests += kind in TEMPLATE_KINDS
        return await super().get(api_version, kind, *args, **kwargs)

    async def list(self, api_version, kind, *args, **kwargs):
        self.template_requests += kind in TEMPLATE_KINDS
        return await super().list(api_version, kind, *args, **kwargs)


def test_resolving_a_run_asks_the_apiserver_nothing(run):
    async def go():
        client = CountingClient(MemoryApiServer())
        await client.create(wft("lib", {"entrypoint": "main", "templates": [
            {"name": "main", "steps": [[
                {"name": "s", "templateRef": {"name": "tools", "template": "ok",
                                              "clusterScope": True}}]]}]}))
        await client.create(wft("tools", {"templates": [sh("ok", "true")]}, cluster=True))
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        await engine.start()
        primed = client.template_requests
        try:
            for i in range(20):
                await client.create(workflow(f"wf{i}", {"workflowTemplateRef": {"name": "lib"}}))
            phases = [(await status_when(client, f"wf{i}"))["phase"] for i in range(20)]
            return primed, client.template_requests, phases, engine.template_reads
        finally:
            await engine.stop()

    primed, after, phases, reads = run(go(), timeout=60)
    assert phases == ["Succeeded"] * 20
    assert primed == 2  # one list per kind, at start
    assert after - primed == 0
    assert reads == 0


def test_a_mutex_named_only_in_the_template_excludes(run, tmp_path):
    spans = tmp_path / "spans"

    async def go():
        client = MemoryClient(MemoryApiServer())
        await client.create(wft("exclusive", {
            "entrypoint": "main", "synchronization": {"mutex": {"name": "device"}},
            "arguments": {"parameters": [{"name": "who", "value": "?"}]},
            "templates": [sh("main", f"echo start {{{{workflow.parameters.who}}}} >> {spans}; "
                                     f"sleep 0.3; echo end {{{{workflow.parameters.who}}}} "
                                     f">> {spans}")]}))
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        await engine.start()
        try:
            for who in ("a", "b"):
                await client.create(workflow(who, {
                    "workflowTemplateRef": {"name": "exclusive"},
                    "arguments": {"parameters": [{"name": "who", "value": who}]}}))
            waiting = await status_when(client, "b", ("Pending",))
            done = [await status_when(client, who) for who in ("a", "b")]
            return waiting, done, engine.stats()
        finally:
            await engine.stop()

    waiting, done, stats = run(go())
    assert waiting["message"] == "Waiting for health/Mutex/device lock"
    assert [st["phase"] for st in done] == ["Succeeded", "Succeeded"]
    assert spans.read_text().split() == ["start", "a", "end", "a", "start", "b", "end", "b"]
    assert (stats["running"], stats["queued"], stats["postponed_total"]) == (0, 0, 1)


def test_a_priority_set_only_in_the_template_orders_the_queue(run, tmp_path):
    order = tmp_path / "order"

    async def go():
        client = MemoryClient(MemoryApiServer())
        for name, extra in (("plain", {}), ("urgent", {"priority": 10})):
            await client.create(wft(name, {
                "entrypoint": "main", **extra,
                "templates": [sh("main", f"echo {name} >> {order}")]}))
        engine = LocalWorkflowEngine(client, ttl_seconds=None, parallelism=1)
        await engine.start()
        try:
            await client.create(workflow("blocker", {"entrypoint": "main", "templates": [
                sh("main", f"sleep 0.3; echo blocker >> {order}")]}))
            await status_when(client, "blocker", ("Running",))
            for name in ("plain", "urgent"):
                await client.create(workflow(name, {"workflowTemplateRef": {"name": name}}))
            return [(await status_when(client, n))["phase"]
                    for n in ("blocker", "plain", "urgent")]
        finally:
            await engine.stop()

    assert run(go()) == ["Succeeded"] * 3
    assert order.read_text().split() == ["blocker", "urgent", "plain"]


def test_a_workflow_found_pending_after_a_restart_is_resolved_anew(run):
    async def go():
        client = MemoryClient(MemoryApiServer())
        await client.create(wft("lib", {"entrypoint": "say", "templates": [sh("say", "echo old")]}))
        first = LocalWorkflowEngine(client, ttl_seconds=None, parallelism=1)
        await first.start()
        try:
            await client.create(workflow("blocker", {"entrypoint": "main", "templates": [
                sh("main", "sleep 5")]}))
            await status_when(client, "blocker", ("Running",))
            await client.create(workflow("queued", {"workflowTemplateRef": {"name": "lib"}}))
            await status_when(client, "queued", ("Pending",))
        finally:
            await first.stop()
        lib = await client.get(*WFT, "health", "lib")
        lib["spec"]["templates"] = [sh("say", "echo new")]
        await client.update(lib)
        second = LocalWorkflowEngine(client, ttl_seconds=None, parallelism=1, recover=True)
        await second.start()
        try:
            return await status_when(client, "blocker"), await status_when(client, "queued")
        finally:
            await second.stop()

    blocker, queued = run(go())
    assert blocker["message"] == LocalWorkflowEngine.INTERRUPTED_MESSAGE
    assert (queued["phase"], pod_outputs(queued)) == ("Succeeded", ["new"])


def test_an_engine_of_one_namespace_sees_its_templates_and_the_cluster_ones(run):
    async def go():
        client = MemoryClient(MemoryApiServer())
        await client.create(wft("mine", {"templates": [sh("say", "echo mine")]}))
        await client.create(wft("theirs", {"templates": [sh("say", "echo theirs")]},
                                namespace="other"))
        await client.create(wft("everyones", {"templates": [sh("say", "echo everyones")]},
                                cluster=True))
        engine = LocalWorkflowEngine(client, namespace="health", ttl_seconds=None)
        await engine.start()
        try:
            def calling(name, **ref):
                return workflow(f"calls-{name}", {"entrypoint": "main", "templates": [
                    {"name": "main", "steps": [[{"name": "s", "templateRef": {
                        "name": name, "template": "say", **ref}}]]}]})

            await client.create(calling("mine"))
            await client.create(calling("theirs"))
            await client.create(calling("everyones", clusterScope=True))
            # a template that arrives later, in each namespace
            await client.create(wft("late", {"templates": [sh("say", "echo late")]}))
            await client.create(wft("late-theirs", {"templates": [sh("say", "true")]},
                                    namespace="other"))
            await asyncio.sleep(0.05)
            await client.create(calling("late"))
            cached = engine.cached_templates()
            return [await status_when(client, f"calls-{n}")
                    for n in ("mine", "theirs", "everyones", "late")], cached
        finally:
            await engine.stop()

    (mine, theirs, everyones, late), cached = run(go())
    assert pod_outputs(mine) == ["mine"]
    assert pod_outputs(everyones) == ["everyones"]
    assert pod_outputs(late) == ["late"]
    assert theirs["phase"] == "Failed"
    assert theirs["message"] == 'workflowtemplates.argoproj.io "theirs" not found'
    assert cached == ["cluster/everyones", "namespaced/health/late", "namespaced/health/mine"]


def test_a_template_survives_a_restart_of_a_durable_store(run, tmp_path):
    data_dir = str(tmp_path / "store")

    async def first_life():
        server = MemoryApiServer.open(data_dir)
        try:
            await MemoryClient(server).create(wft("lib", {
                "entrypoint": "main",
                "arguments": {"parameters": [{"name": "text", "value": "unset"}]},
                "templates": [sh("main", "echo {{workflow.parameters.text}}")]}))
        finally:
            server.close()

    async def second_life():
        server = MemoryApiServer.open(data_dir)
        client = MemoryClient(server)
        engine = LocalWorkflowEngine(client, ttl_seconds=None, recover=True)
        manager = Manager(client, max_workers=2)
        await engine.start()
        await manager.start()
        try:
            kept = await client.get(*WFT, "health", "lib")
            await client.create(health_check("uses-lib", {
                "workflowTemplateRef": {"name": "lib"},
                "arguments": {"parameters": [{"name": "text", "value": "after restart"}]}}))
            for _ in range(1500):
                hc = await client.get(API_VERSION, "HealthCheck", "health", "uses-lib")
                if (hc.get("status") or {}).get("successCount") == 1:
                    (wf,) = await client.list(*WF, "health")
                    return kept, wf["status"]
                await asyncio.sleep(0.01)
            raise AssertionError(hc.get("status"))
        finally:
            await manager.stop()
            await engine.stop()
            server.close()

    run(first_life())
    kept, status = run(second_life())
    assert kept["spec"]["entrypoint"] == "main"
    assert pod_outputs(status) == ["after restart"]
    stored = status["storedWorkflowTemplateSpec"]
    # what the controller injects wins over the template, as on a cluster
    assert stored["activeDeadlineSeconds"] == 30
    assert stored["serviceAccountName"] == "sa"
    assert "workflowTemplateRef" not in stored


MALFORMED = [
    {"entrypoint": "m", "templates": [{"name": "m", "dag": [{"name": "x"}]}]},
    {"entrypoint": "m", "templates": 5},
    {"entrypoint": "m", "templates": [{"name": "m", "steps": 7}]},
    {"entrypoint": "m", "templates": [{"name": ["m"], "container": {"command": ["true"]}}]},
    {"workflowTemplateRef": {"name": "lib"}, "templates": 5},
    {"workflowTemplateRef": {"name": "lib"}, "arguments": {"parameters": 5}},
    {"workflowTemplateRef": {"name": "lib"}, "templates": [{"name": {"a": 1}}]},
    {"entrypoint": "m", "templates": [{"name": "m", "steps": [[
        {"name": "s", "template": ["x"], "templateRef": 3}]]}]},
]


def test_a_malformed_workflow_does_not_stop_the_ones_after_it(run):
    async def go():
        client = MemoryClient(MemoryApiServer())
        await client.create(wft("lib", {"entrypoint": "say", "templates": [sh("say", "echo ok")]}))
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        await engine.start()
        try:
            for i, spec in enumerate(MALFORMED):
                await client.create(workflow(f"bad{i}", spec))
                await client.create(workflow(f"good{i}", {"workflowTemplateRef": {"name": "lib"}}))
            good = [await status_when(client, f"good{i}") for i in range(len(MALFORMED))]
            # the two shapes that used to end the watch loop are told what is wrong
            bad = [await status_when(client, f"bad{i}") for i in (0, 1)]
            return good, bad, engine._task.done()
        finally:
            await engine.stop()

    good, bad, loop_ended = run(go())
    assert [st["phase"] for st in good] == ["Succeeded"] * len(MALFORMED)
    assert not loop_ended
    assert [st["phase"] for st in bad] == ["Failed", "Failed"]
    assert bad[1]["message"] == "spec.templates is not a list"


class SlowTemplateReads(MemoryClient):
    """Template watches deliver nothing and a direct read of a template
    waits until ``release`` is set."""

    def __init__(self, server):
        super().__init__(server)
        self.reading = asyncio.Event()
        self.release = asyncio.Event()

    def watch(self, api_version, kind, namespace=None):
        if kind in TEMPLATE_KINDS:
            return MemoryClient(MemoryApiServer()).watch(api_version, kind, namespace)
        return super().watch(api_version, kind, namespace)

    async def get(self, api_version, kind, *args, **kwargs):
        if kind in TEMPLATE_KINDS:
            self.reading.set()
            await self.release.wait()
        return await super().get(api_version, kind, *args, **kwargs)


def test_a_workflow_deleted_while_its_template_is_read_never_runs(run, tmp_path):
    ran = tmp_path / "ran"

    async def go():
        client = SlowTemplateReads(MemoryApiServer())
        engine = LocalWorkflowEngine(client, ttl_seconds=None, parallelism=1)
        await engine.start()
        try:
            await client.create(wft("lib", {"entrypoint": "say", "templates": [
                sh("say", f"echo $0 >> {ran}")]}))
            await client.create(workflow("doomed", {"workflowTemplateRef": {"name": "lib"}}))
            await asyncio.wait_for(client.reading.wait(), 5)
            await client.delete(*WF, "health", "doomed")
            for _ in range(500):  # until the engine has seen the deletion
                if not any(rec.confirming for rec in engine._records.values()):
                    break
                await asyncio.sleep(0.01)
            client.release.set()
            await client.create(workflow("next", {"workflowTemplateRef": {"name": "lib"}}))
            status = await status_when(client, "next")
            return status, engine.completed, engine.stats()
        finally:
            await engine.stop()

    status, completed, stats = run(go())
    assert status["phase"] == "Succeeded"
    assert completed == 1  # "next" alone
    assert ran.read_text().splitlines() == ["sh"]
    assert (stats["running"], stats["queued"], stats["processes"]) == (0, 0, 0)

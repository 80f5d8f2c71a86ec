"""Restarting over a durable store (MemoryApiServer.open): a hard kill loses
nothing acknowledged, a fleet carries on where it stopped without being
re-applied, and the workflow engines recover what the old process left."""
import asyncio
import os
import signal
import subprocess
import sys
import time

from active_monitor_amd import API_VERSION
from active_monitor_amd.api.types import format_k8s_time
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient, NotFoundError
from active_monitor_amd.workflow import (
    LocalWorkflowEngine,
    ScriptedWorkflowEngine,
    always_succeed,
)

from .conftest import WF, make_hc

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
INTERRUPTED = "workflow interrupted: engine restarted"

_WRITER = """
import sys
from active_monitor_amd.kube import MemoryApiServer
server = MemoryApiServer.open(sys.argv[1], compact_threshold=16)
i = 0
while True:
    made = server.create({"apiVersion": "v1", "kind": "ConfigMap",
                          "metadata": {"generateName": "cm-", "namespace": "health"},
                          "data": {"i": str(i)}})
    if i % 3 == 0:  # keep the journal ahead of the object count: compactions
        server.patch("v1", "ConfigMap", "health", made["metadata"]["name"],
                     {"data": {"again": "1"}})
    print(made["metadata"]["name"], flush=True)
    i += 1
"""


def test_hard_kill_loses_nothing_acknowledged(tmp_path):
    d = str(tmp_path / "store")
    child = subprocess.Popen([sys.executable, "-c", _WRITER, d], cwd=REPO,
                             stdout=subprocess.PIPE, text=True)
    try:
        acked = [child.stdout.readline().strip() for _ in range(40)]
    finally:
        child.send_signal(signal.SIGKILL)
        child.wait(timeout=10)
        child.stdout.close()
    assert all(acked), acked

    server = MemoryApiServer.open(d)  # the kill released the lock
    try:
        found = {o["metadata"]["name"]: o for o in server.list("v1", "ConfigMap", "health")}
        assert set(acked) <= set(found)
        top = int(server.resource_version())
        assert top >= len(acked)
        for name in acked:
            assert 1 <= int(found[name]["metadata"]["resourceVersion"]) <= top
    finally:
        server.close()


def fail_sick_pass_rest(wf):
    name = wf["metadata"]["name"]
    if name.startswith("sick-wf-"):
        return ("Failed", "check failed")
    return ("Succeeded", "")


class DurableEnv:
    """conftest.Env's shape over a store kept in a directory."""

    def __init__(self, data_dir, policy=always_succeed):
        self.server = MemoryApiServer.open(data_dir)
        self.client = MemoryClient(self.server)
        self.manager = Manager(self.client, max_workers=4)
        self.engine = ScriptedWorkflowEngine(self.client, policy=policy, recover=True)

    async def __aenter__(self):
        await self.engine.start()
        await self.manager.start()
        return self

    async def __aexit__(self, *exc):
        await self.manager.stop()
        await self.engine.stop()
        self.server.close()

    async def statuses(self, names):
        out = {}
        for name in names:
            hc = await self.client.get(API_VERSION, "HealthCheck", "health", name)
            out[name] = hc.get("status") or {}
        return out


def runs(status):
    return status.get("successCount", 0) + status.get("failedCount", 0)


async def wait_for(pred, timeout, msg):
    deadline = time.monotonic() + timeout
    while time.monotonic() < deadline:
        v = await pred()
        if v:
            return v
        await asyncio.sleep(0.05)
    raise AssertionError(f"timed out waiting for {msg}")


def test_fleet_carries_on_after_a_restart(tmp_path, run):
    d = str(tmp_path / "store")
    names = ["ok-a", "ok-b", "sick"]

    async def first_life():
        async with DurableEnv(d, fail_sick_pass_rest) as env:
            for name in ("ok-a", "ok-b"):
                await env.client.create(make_hc(name=name, repeat=1))
            sick = make_hc(name="sick", repeat=1, remedy=True)
            sick["spec"]["remedyRunsLimit"] = 1000
            sick["spec"]["remedyResetInterval"] = 3600
            await env.client.create(sick)

            async def everyone_ran_twice():
                st = await env.statuses(names)
                return all(runs(s) >= 2 for s in st.values()) and st

            await wait_for(everyone_ran_twice, 30, "two runs of every check")

    async def second_life(at_shutdown):
        async with DurableEnv(d, fail_sick_pass_rest) as env:
            # nothing is re-applied: the objects are simply there
            st = await env.statuses(names)
            for name in names:
                assert runs(st[name]) >= runs(at_shutdown[name]), name
            assert st["sick"].get("remedyTotalRuns", 0) >= at_shutdown["sick"]["remedyTotalRuns"]

            async def everyone_ran_again():
                now = await env.statuses(names)
                return all(runs(now[n]) > runs(at_shutdown[n]) for n in names) and now

            now = await wait_for(everyone_ran_again, 10, "runs after the restart")
            assert now["sick"]["failedCount"] > at_shutdown["sick"]["failedCount"]
            assert now["sick"]["remedyTotalRuns"] >= at_shutdown["sick"]["remedyTotalRuns"]

    run(first_life(), timeout=45)
    # read what was left behind only after everything has stopped
    between = MemoryApiServer.open(d)
    uids = {}
    at_shutdown = {}
    for name in names:
        hc = between.get(API_VERSION, "HealthCheck", "health", name)
        uids[name] = hc["metadata"]["uid"]
        at_shutdown[name] = hc["status"]
    between.close()
    assert all(runs(s) >= 2 for s in at_shutdown.values())
    assert at_shutdown["sick"]["remedyTotalRuns"] >= 1

    run(second_life(at_shutdown), timeout=30)
    after = MemoryApiServer.open(d)
    try:
        for name in names:
            hc = after.get(API_VERSION, "HealthCheck", "health", name)
            assert hc["metadata"]["uid"] == uids[name]
    finally:
        after.close()


def _wf(name, status=None, spec=None):
    obj = {"apiVersion": WF[0], "kind": WF[1],
           "metadata": {"name": name, "namespace": "health"},
           "spec": spec or {"entrypoint": "main",
                            "templates": [{"name": "main",
                                           "container": {"command": ["true"]}}]}}
    if status is not None:
        obj["status"] = status
    return obj


def _seed_three(data_dir):
    """What a stopped process can leave: one workflow never picked up, one
    cut off mid-run, one finished ten seconds ago."""
    server = MemoryApiServer.open(data_dir)
    server.create(_wf("pending"))
    server.create(_wf("running", {"phase": "Running",
                                  "startedAt": format_k8s_time(_ago(30))}))
    server.create(_wf("done", {"phase": "Succeeded",
                               "finishedAt": format_k8s_time(_ago(10))}))
    server.close()


def _ago(seconds):
    from datetime import datetime, timedelta, timezone

    return datetime.now(timezone.utc) - timedelta(seconds=seconds)


def test_engine_recovers_each_workflow_by_its_state(tmp_path, run):
    d = str(tmp_path / "store")
    _seed_three(d)
    asked = []

    def policy(wf):
        asked.append(wf["metadata"]["name"])
        return ("Succeeded", "")

    async def go():
        server = MemoryApiServer.open(d)
        client = MemoryClient(server)
        engine = ScriptedWorkflowEngine(client, policy=policy, ttl_seconds=11,
                                        recover=True)
        try:
            present_at_start = await client.get(*WF, "health", "done")
            assert present_at_start["status"]["phase"] == "Succeeded"
            started = time.monotonic()
            await engine.start()

            async def phase_of(name):
                wf = await client.get(*WF, "health", name)
                return (wf.get("status") or {}).get("phase")

            async def both_settled():
                return (await phase_of("pending") == "Succeeded"
                        and await phase_of("running") == "Failed")

            await wait_for(both_settled, 5, "pending run and running failed")
            failed = await client.get(*WF, "health", "running")
            assert failed["status"]["message"] == INTERRUPTED
            assert failed["status"]["finishedAt"]
            assert asked == ["pending"]  # the interrupted one was never re-run

            async def done_collected():
                try:
                    await client.get(*WF, "health", "done")
                except NotFoundError:
                    return True
                return False

            # ttl 11 s, finished 10 s ago: about one second left, not eleven
            await wait_for(done_collected, 5, "TTL of the finished workflow")
            assert time.monotonic() - started < 5
            # the two that finished just now keep their full TTL
            assert await phase_of("pending") and await phase_of("running")
        finally:
            await engine.stop()
            server.close()

    run(go(), timeout=30)


def test_recovery_is_off_by_default(tmp_path, run):
    d = str(tmp_path / "store")
    _seed_three(d)
    asked = []

    def policy(wf):
        asked.append(wf["metadata"]["name"])
        return ("Succeeded", "")

    async def go():
        server = MemoryApiServer.open(d)
        client = MemoryClient(server)
        before = await client.list(*WF, "health")
        engine = ScriptedWorkflowEngine(client, policy=policy, ttl_seconds=0.2)
        try:
            await engine.start()
            # the engine is alive — a new workflow runs — and by the time it
            # has, anything start() had taken from the store would show
            await client.create(_wf("fresh"))

            async def fresh_done():
                wf = await client.get(*WF, "health", "fresh")
                return (wf.get("status") or {}).get("phase") == "Succeeded"

            await wait_for(fresh_done, 5, "a workflow added after start")
            assert asked == ["fresh"]
            now = await client.list(*WF, "health")
            assert [w for w in now if w["metadata"]["name"] != "fresh"] == before
        finally:
            await engine.stop()
            server.close()

    run(go(), timeout=30)


def test_local_engine_never_reruns_an_interrupted_workflow(tmp_path, run):
    d = str(tmp_path / "store")
    marker = tmp_path / "ran"
    spec = {"entrypoint": "main",
            "templates": [{"name": "main",
                           "container": {"command": ["touch", str(marker)]}}]}
    server = MemoryApiServer.open(d)
    server.create(_wf("remedy", {"phase": "Running",
                                 "startedAt": format_k8s_time(_ago(5))}, spec=spec))
    server.close()

    async def go():
        server = MemoryApiServer.open(d)
        client = MemoryClient(server)
        engine = LocalWorkflowEngine(client, ttl_seconds=None, recover=True)
        try:
            await engine.start()

            async def failed():
                wf = await client.get(*WF, "health", "remedy")
                return wf["status"]["phase"] == "Failed" and wf

            wf = await wait_for(failed, 5, "the interrupted workflow to fail")
            assert wf["status"]["message"] == INTERRUPTED
            # prove the engine does run things: a sibling touches its file
            other = tmp_path / "other-ran"
            await client.create(_wf("sibling", spec={
                "entrypoint": "main",
                "templates": [{"name": "main",
                               "container": {"command": ["touch", str(other)]}}]}))

            async def sibling_done():
                wf = await client.get(*WF, "health", "sibling")
                return (wf.get("status") or {}).get("phase") == "Succeeded"

            await wait_for(sibling_done, 10, "the sibling workflow")
            assert other.exists()
        finally:
            await engine.stop()
            server.close()

    run(go(), timeout=30)
    assert not marker.exists()


def test_listed_and_watched_workflow_runs_once(tmp_path, run):
    d = str(tmp_path / "store")
    calls = []

    def policy(wf):
        calls.append(wf["metadata"]["name"])
        return ("Succeeded", "")

    class SlowListClient(MemoryClient):
        """Creates a workflow after the engine's watch opened and before its
        list returns — the one the engine meets through both."""

        raced = False

        async def list(self, *a, **kw):
            if not self.raced:
                self.raced = True
                await self.create(_wf("racer"))
            return await super().list(*a, **kw)

    async def go():
        server = MemoryApiServer.open(d)
        server.create(_wf("pending"))
        client = SlowListClient(server)
        engine = ScriptedWorkflowEngine(client, policy=policy, ttl_seconds=None,
                                        recover=True)
        try:
            await engine.start()

            async def settled():
                wfs = await MemoryClient(server).list(*WF, "health")
                return all((w.get("status") or {}).get("phase") == "Succeeded"
                           for w in wfs)

            await wait_for(settled, 5, "both workflows")
            # events are handled in order: once a later workflow has run, a
            # duplicate of the racer's ADDED would have run as well
            await client.create(_wf("sentinel"))

            async def sentinel_ran():
                return "sentinel" in calls

            await wait_for(sentinel_ran, 5, "the sentinel workflow")
            assert sorted(calls) == ["pending", "racer", "sentinel"]
        finally:
            await engine.stop()
            server.close()

    run(go(), timeout=30)


def test_recovery_bookkeeping_does_not_outlive_the_overlap(tmp_path, run):
    """The uids taken from the start-up list are dropped at the first event
    newer than that list, and the re-armed TTL timers are queued shortest
    first (the engine prunes spent timers from the front)."""
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    server.create(_wf("running", {"phase": "Running"}))
    for name, age in (("long", 1), ("short", 50), ("mid", 20)):
        server.create(_wf(name, {"phase": "Succeeded",
                                 "finishedAt": format_k8s_time(_ago(age))}))
    server.close()

    async def go():
        server = MemoryApiServer.open(d)
        client = MemoryClient(server)
        engine = ScriptedWorkflowEngine(client, ttl_seconds=60, recover=True)
        try:
            await engine.start()
            whens = [h.when() for h in engine._ttl_handles]
            assert len(whens) == 3 and whens == sorted(whens)
            assert len(engine._recovered) == 1  # the interrupted one
            await client.create(_wf("fresh"))

            async def fresh_done():
                wf = await client.get(*WF, "health", "fresh")
                return (wf.get("status") or {}).get("phase") == "Succeeded"

            await wait_for(fresh_done, 5, "a workflow added after start")
            assert engine._recovered == set()
            whens = [h.when() for h in engine._ttl_handles]
            assert whens == sorted(whens)
        finally:
            await engine.stop()
            server.close()

    run(go(), timeout=30)

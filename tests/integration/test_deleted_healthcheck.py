"""What the controller still holds once a HealthCheck is gone: nothing.

A Manager runs over the wire (HttpClient -> ApiServerFrontend ->
MemoryApiServer) with a scripted workflow engine on the store, and with the
informer resync switched off, so that only the watch's Replace after a
re-list can tell it about a deletion it missed. The deletions are missed
deterministically: the listener is stopped, the store is changed directly
with its event history compacted, a new listener starts on the same port.
"""
import asyncio
import json
import urllib.request

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.metrics import MonitorSuccess, exposition
from active_monitor_amd.workflow import ScriptedWorkflowEngine, always_succeed

from .conftest import make_hc

KIND = "HealthCheck"
WF = ("argoproj.io/v1alpha1", "Workflow")


class WireEnv:
    def __init__(self, policy=always_succeed, engine_delay=0.0, **manager_kw):
        self.policy = policy
        self.engine_delay = engine_delay
        self.manager_kw = manager_kw

    async def __aenter__(self):
        self.store = MemoryApiServer()
        self.frontend = ApiServerFrontend(self.store)
        await self.frontend.start()
        self.port = self.frontend.port
        # the engine plays the in-cluster Argo controller: direct store access
        self.engine = ScriptedWorkflowEngine(
            MemoryClient(self.store), policy=self.policy, delay=self.engine_delay)
        await self.engine.start()
        self.client = HttpClient(self.frontend.url, qps=0)
        await self.client.start()
        # resync off: nothing but the watch can heal a missed deletion
        self.manager = Manager(self.client, max_workers=4, resync_period=0,
                               **self.manager_kw)
        await self.manager.start()
        self.rec = self.manager.reconciler
        return self

    async def __aexit__(self, *exc):
        await self.manager.stop()
        await self.engine.stop()
        await self.client.close()
        await self.frontend.stop()

    async def until(self, pred, what, timeout=15.0):
        deadline = asyncio.get_running_loop().time() + timeout
        while not pred():
            assert asyncio.get_running_loop().time() < deadline, f"timed out: {what}"
            await asyncio.sleep(0.01)

    async def outage(self, change):
        """A forced 410 window: see the module docstring."""
        subs = [self.manager._sub, self.manager.wf_hub._sub]
        # both watches stream: neither is between two connects, where it
        # would miss the stop and keep its connection to the store
        await self.until(lambda: len(self.frontend._live_subs) == len(subs),
                         "watches streaming")
        before = [sub.relists for sub in subs]
        await self.frontend.stop()
        self.store.history_window = 0
        change()
        self.store.history_window = 4096
        self.frontend = ApiServerFrontend(self.store, port=self.port)
        await self.frontend.start()
        await self.until(
            lambda: all(s.relists > b for s, b in zip(subs, before)),
            "re-list after the outage")

    def status(self, name, ns="health"):
        return self.store.get(API_VERSION, KIND, ns, name).get("status") or {}

    def owned_workflows(self, uid, ns="health"):
        return [
            wf["metadata"]["name"] for wf in self.store.list(*WF, ns)
            if any(ref.get("uid") == uid
                   for ref in wf["metadata"].get("ownerReferences") or [])
        ]


def _fetch_json(url):
    with urllib.request.urlopen(url, timeout=5) as resp:
        return json.loads(resp.read())


def test_missed_deletion_does_not_resurrect(run):
    async def go():
        async with WireEnv(health_addr=("127.0.0.1", 0)) as env:
            created = await env.client.create(make_hc(name="ghost", repeat=1))
            uid = created["metadata"]["uid"]
            await env.until(lambda: env.rec.completed_runs >= 1, "the first run")
            assert ("health", "ghost") in env.manager.hc_cache

            await env.outage(
                lambda: env.store.delete(API_VERSION, KIND, "health", "ghost"))

            await env.until(lambda: ("health", "ghost") not in env.manager.hc_cache,
                            "the cache entry to go", timeout=5.0)
            await env.until(
                lambda: env.rec.get_timer_by_name("ghost", "health") is None,
                "the repeat timer to go", timeout=5.0)
            assert env.rec.active_watches() == 0
            # the repeat interval is 1 s: a check still driven submits again
            # (a workflow submitted for an owner that is gone is not
            # garbage-collected with it, so it would stay to be counted)
            first = len(env.owned_workflows(uid))
            reconciles = env.rec.reconcile_count
            await asyncio.sleep(2.5)
            assert len(env.owned_workflows(uid)) == first
            assert env.rec.reconcile_count == reconciles
            assert env.rec.get_timer_by_name("ghost", "health") is None

            assert env.manager._sub.relists >= 1
            assert env.manager._sub.synthetic_deletes == 1
            port = env.manager._servers[0].sockets[0].getsockname()[1]
            stats = await asyncio.get_running_loop().run_in_executor(
                None, _fetch_json, f"http://127.0.0.1:{port}/statusz")
            assert stats["watch_relists"] == env.manager._sub.relists
            assert stats["watch_synthetic_deletes"] == 1

    run(go(), timeout=60)


def test_statusz_counters_are_zero_without_them(run):
    """The in-process backend's watch cannot expire and has no counters."""

    async def go():
        manager = Manager(MemoryClient(MemoryApiServer()), max_workers=1,
                          health_addr=("127.0.0.1", 0))
        await manager.start()
        try:
            port = manager._servers[0].sockets[0].getsockname()[1]
            stats = await asyncio.get_running_loop().run_in_executor(
                None, _fetch_json, f"http://127.0.0.1:{port}/statusz")
            assert stats["watch_relists"] == 0
            assert stats["watch_synthetic_deletes"] == 0
        finally:
            await manager.stop()

    run(go(), timeout=30)


def test_recreated_inside_the_window_starts_from_zero(run):
    """Deleted and re-created while its second run is in flight: the run of
    the old object is dropped, and neither its result nor, two seconds later,
    its time-out is written into the new object's status."""

    async def go():
        async with WireEnv(engine_delay=0.6) as env:
            old = await env.client.create(make_hc(name="phoenix", repeat=1, timeout=2))
            old_uid = old["metadata"]["uid"]
            await env.until(lambda: env.rec.completed_runs >= 1, "the first run")
            assert env.status("phoenix")["successCount"] == 1
            await env.until(
                lambda: env.rec.completed_runs == 1 and env.rec.active_watches() == 1
                and len(env.owned_workflows(old_uid)) == 2,
                "the second run in flight")
            old_names = set(env.owned_workflows(old_uid))
            new = {}

            def change():
                env.store.delete(API_VERSION, KIND, "health", "phoenix")
                new["obj"] = env.store.create(make_hc(name="phoenix", repeat=1, timeout=2))

            await env.outage(change)
            new_uid = new["obj"]["metadata"]["uid"]
            assert new_uid != old_uid
            assert env.status("phoenix") == {}

            # every status the new object ever shows, until well past the
            # old run's 2 s time-out, counts the new object's runs alone
            loop = asyncio.get_running_loop()
            deadline = loop.time() + 3.0
            seen = []
            while loop.time() < deadline:
                st = env.status("phoenix")
                if st and (not seen or st != seen[-1]):
                    seen.append(st)
                    assert st.get("failedCount", 0) == 0, st
                    assert st.get("lastFailedWorkflow", "") == "", st
                    assert st["lastSuccessfulWorkflow"] not in old_names, st
                    assert st["lastSuccessfulWorkflow"] in env.owned_workflows(new_uid)
                    assert st["successCount"] == len(seen), seen
                    assert st["totalHealthCheckRuns"] == len(seen), seen
                await asyncio.sleep(0.01)
            assert seen, "the new object never ran"
            assert seen[0]["successCount"] == 1
            assert env.manager._sub.synthetic_deletes == 1

    run(go(), timeout=60)


def _metric_policy(help_text):
    def policy(wf):
        value = json.dumps({"metrics": [
            {"name": "latency", "value": 7, "metrictype": "gauge", "help": help_text},
        ]})
        return ("Succeeded", "", {"parameters": [{"name": "m", "value": value}]})

    return policy


def _samples(name=None):
    """Sample lines of the exposition, or those of one HealthCheck."""
    lines = [ln for ln in exposition().decode().splitlines()
             if ln and not ln.startswith("#")]
    if name is None:
        return lines
    return [ln for ln in lines if f'healthcheck_name="{name}"' in ln]


_STATIC = ("healthcheck_success_count", "healthcheck_runtime_seconds",
           "healthcheck_starttime", "healthcheck_finishedtime")


def test_deleted_check_drops_its_series_and_can_register_again(run):
    async def go():
        help_text = {"now": "first help"}
        async with WireEnv(policy=lambda wf: _metric_policy(help_text["now"])(wf)) as env:
            await env.client.create(make_hc(name="mlc-check", repeat=1))
            await env.until(lambda: env.rec.completed_runs >= 1, "a run")
            got = _samples("mlc-check")
            for series in _STATIC:
                assert any(ln.startswith(series + "{") for ln in got), (series, got)
            assert any(ln.startswith("mlc_check_latency{") for ln in got), got
            assert "# HELP mlc_check_latency first help" in exposition().decode()

            await env.client.delete(API_VERSION, KIND, "health", "mlc-check")
            await env.until(lambda: not _samples("mlc-check"), "its series to go",
                            timeout=5.0)
            assert "mlc_check_latency" not in exposition().decode()
            assert env.rec.get_timer_by_name("mlc-check", "health") is None

            # the gauge's name is free again, help text included
            help_text["now"] = "second help"
            runs = env.rec.completed_runs
            await env.client.create(make_hc(name="mlc-check", repeat=1))
            await env.until(lambda: env.rec.completed_runs > runs, "a run of the new one")
            text = exposition().decode()
            assert "# HELP mlc_check_latency second help" in text
            assert 'mlc_check_latency{healthcheck_name="mlc-check"} 7.0' in text
            assert MonitorSuccess.value("mlc-check", "healthCheck") == 1.0
            await env.client.delete(API_VERSION, KIND, "health", "mlc-check")
            await env.until(lambda: not _samples("mlc-check"), "its series to go",
                            timeout=5.0)

    run(go(), timeout=60)


def test_same_name_in_two_namespaces_shares_the_series(run):
    async def go():
        async with WireEnv(policy=_metric_policy("twin help")) as env:
            await env.client.create(make_hc(name="mlc-twin", ns="health", repeat=1))
            await env.client.create(make_hc(name="mlc-twin", ns="other", repeat=1))
            await env.until(
                lambda: MonitorSuccess.value("mlc-twin", "healthCheck") >= 2
                and env.rec.get_timer_by_name("mlc-twin", "health") is not None
                and env.rec.get_timer_by_name("mlc-twin", "other") is not None,
                "a run of each")

            await env.client.delete(API_VERSION, KIND, "health", "mlc-twin")
            # the timer goes in the same step that decides about the series
            await env.until(
                lambda: env.rec.get_timer_by_name("mlc-twin", "health") is None,
                "the first deletion to be reconciled", timeout=5.0)
            assert MonitorSuccess.value("mlc-twin", "healthCheck") >= 2
            got = _samples("mlc-twin")
            for series in _STATIC + ("mlc_twin_latency",):
                assert any(ln.startswith(series + "{") for ln in got), (series, got)

            await env.client.delete(API_VERSION, KIND, "other", "mlc-twin")
            await env.until(lambda: not _samples("mlc-twin"), "the series to go",
                            timeout=5.0)
            assert "mlc_twin_latency" not in exposition().decode()

    run(go(), timeout=60)


def test_churn_leaves_the_exposition_as_it_was(run):
    async def go():
        async with WireEnv(policy=_metric_policy("churn help")) as env:
            before = len(_samples())
            peak = before
            for i in range(30):
                name = f"mlc-churn-{i}"
                runs = env.rec.completed_runs
                await env.client.create(make_hc(name=name, repeat=1))
                await env.until(lambda: env.rec.completed_runs > runs, f"a run of {name}")
                peak = max(peak, len(_samples()))
                await env.client.delete(API_VERSION, KIND, "health", name)
                await env.until(lambda: not _samples(name), f"the series of {name} to go",
                                timeout=5.0)
            assert peak > before  # the rounds did emit series
            assert len(_samples()) == before
            assert not env.rec._metric_namespaces
            assert not env.rec._driven_uid

    run(go(), timeout=90)

"""Running a HealthCheck on demand: the run-requested annotation through the
reconciler's scheduler branches, the repeat timer, the in-flight guard and
the acknowledgement write.

Every check here that could otherwise run by its schedule has
``repeat=3600``, so a second Workflow can only come from the request."""
import asyncio
import logging
import time

from active_monitor_amd import API_VERSION
from active_monitor_amd.api import (
    RUN_HANDLED_ANNOTATION,
    RUN_REQUEST_ANNOTATION,
    RUN_REQUESTED_ANNOTATION,
    RUN_WORKFLOW_ANNOTATION,
)
from active_monitor_amd.engine import Manager
from active_monitor_amd.engine.shards import shard_of
from active_monitor_amd.kube.errors import ApiError

from .conftest import Env, make_hc

TERMINAL = ("Succeeded", "Failed")
STOPPED_MESSAGE = (
    "workflow execution is stopped; either spec.RepeatAfterSec or "
    "spec.Schedule must be provided. spec.RepeatAfterSec set to 0. "
    "spec.Schedule set to {Cron:}"
)


async def annotate(client, name, token, ns="health"):
    return await client.patch(
        API_VERSION, "HealthCheck", ns, name,
        {"metadata": {"annotations": {RUN_REQUESTED_ANNOTATION: token}}})


async def annotations(env, name, ns="health"):
    obj = await env.client.get(API_VERSION, "HealthCheck", ns, name)
    return obj["metadata"].get("annotations") or {}


def check_wfs(wfs, name):
    """The check Workflows of ``name`` (not its remedies), oldest first."""
    own = [w for w in wfs if w["metadata"]["name"].startswith(f"{name}-wf-")]
    return sorted(own, key=lambda w: int(w["metadata"]["resourceVersion"]))


def in_flight(wfs):
    return [w for w in wfs if (w.get("status") or {}).get("phase") not in TERMINAL]


def total_runs(env, name, n):
    async def pred():
        hc = await env.get_hc(name)
        return hc.status.total_healthcheck_runs >= n and hc
    return pred


def handled(env, name, token):
    async def pred():
        ann = await annotations(env, name)
        return ann.get(RUN_HANDLED_ANNOTATION) == token and ann
    return pred


class PatchHook:
    """A client whose HealthCheck patches pass through ``hook`` first."""

    def __init__(self, inner, hook):
        self._inner = inner
        self._hook = hook
        self.hc_patches = 0

    def __getattr__(self, name):
        return getattr(self._inner, name)

    async def patch(self, api_version, kind, namespace, name, patch, **kw):
        if kind == "HealthCheck":
            self.hc_patches += 1
            await self._hook(self.hc_patches)
        return await self._inner.patch(api_version, kind, namespace, name, patch, **kw)


def test_a_request_runs_the_check_now(run):
    async def go():
        async with Env() as env:
            rec = env.manager.reconciler
            await env.create_hc(make_hc(name="now", repeat=3600))
            await env.wait_for(total_runs(env, "now", 1), msg="the first run")
            (first,) = check_wfs(await env.workflows(), "now")
            assert "annotations" not in first["metadata"]  # a scheduled run
            assert rec.on_demand_runs == 0

            await annotate(env.client, "now", "t1")
            hc = await env.wait_for(total_runs(env, "now", 2), msg="the run on demand")
            assert hc.status.total_healthcheck_runs == 2
            wfs = check_wfs(await env.workflows(), "now")
            assert len(wfs) == 2 and wfs[0]["metadata"]["name"] == first["metadata"]["name"]
            second = wfs[1]
            ann = await annotations(env, "now")
            assert ann[RUN_HANDLED_ANNOTATION] == "t1"
            assert ann[RUN_WORKFLOW_ANNOTATION] == second["metadata"]["name"]
            assert second["metadata"]["annotations"] == {RUN_REQUEST_ANNOTATION: "t1"}
            assert hc.status.last_successful_workflow == second["metadata"]["name"]
            assert rec.on_demand_runs == 1

            await env.manager.recorder.flush()
            events = await env.client.list("v1", "Event", "health")
            assert [e for e in events
                    if e["message"] == "Workflow run requested on demand"
                    and e["type"] == "Normal"
                    and e["involvedObject"]["name"] == "now"]

            # the schedule goes on from this run's completion
            timer = rec.get_timer_by_name("now", "health")
            assert timer is not None and not timer.fired
            assert not rec._run_acks and not rec._rerun_after_watch

    run(go(), timeout=45)


def test_the_same_token_or_none_asks_for_nothing(run):
    async def go():
        async with Env() as env:
            await env.create_hc(make_hc(name="once", repeat=3600))
            await env.wait_for(total_runs(env, "once", 1), msg="the first run")
            await annotate(env.client, "once", "t1")
            await env.wait_for(total_runs(env, "once", 2), msg="the run on demand")

            await annotate(env.client, "once", "t1")  # the same token again
            # any other write to the object: the request stays served
            await env.client.patch(API_VERSION, "HealthCheck", "health", "once",
                                   {"metadata": {"labels": {"touched": "yes"}}})
            await annotate(env.client, "once", None)  # the annotation removed
            await asyncio.sleep(1.0)
            assert len(check_wfs(await env.workflows(), "once")) == 2
            assert (await env.get_hc("once")).status.total_healthcheck_runs == 2
            assert env.manager.reconciler.on_demand_runs == 1
            ann = await annotations(env, "once")
            assert RUN_REQUESTED_ANNOTATION not in ann
            assert ann[RUN_HANDLED_ANNOTATION] == "t1"

    run(go(), timeout=45)


def _deferred(run, tokens):
    async def go():
        async with Env(engine_delay=0.5) as env:
            await env.create_hc(make_hc(name="busy", repeat=3600))

            async def first_started():
                wfs = check_wfs(await env.workflows(), "busy")
                return wfs and (wfs[0].get("status") or {}).get("phase") == "Running"

            await env.wait_for(first_started, msg="the first run to be in flight")
            for token in tokens:
                await annotate(env.client, "busy", token)
                await asyncio.sleep(0.05)
            # the run in flight started before the request: no ack for it
            assert RUN_HANDLED_ANNOTATION not in await annotations(env, "busy")

            seen_two = False
            deadline = time.monotonic() + 20.0
            while time.monotonic() < deadline:
                wfs = check_wfs(await env.workflows(), "busy")
                assert len(in_flight(wfs)) <= 1, "two check Workflows at once"
                if len(wfs) >= 2:
                    # the second was created after the first had finished
                    assert (wfs[0].get("status") or {}).get("phase") in TERMINAL
                    seen_two = True
                hc = await env.get_hc("busy")
                if hc.status.total_healthcheck_runs >= 2:
                    break
                await asyncio.sleep(0.01)
            assert seen_two and hc.status.total_healthcheck_runs == 2

            wfs = check_wfs(await env.workflows(), "busy")
            ann = await env.wait_for(handled(env, "busy", tokens[-1]), msg="the ack")
            assert ann[RUN_WORKFLOW_ANNOTATION] == wfs[1]["metadata"]["name"]
            assert wfs[1]["metadata"]["annotations"] == {RUN_REQUEST_ANNOTATION: tokens[-1]}
            assert "annotations" not in wfs[0]["metadata"]

            # served once: a third run would have started (and, at 0.5 s a
            # run, finished) by now
            await asyncio.sleep(1.0)
            assert len(check_wfs(await env.workflows(), "busy")) == 2
            assert env.manager.reconciler.on_demand_runs == 1
            assert not env.manager.reconciler._rerun_after_watch

    run(go(), timeout=60)


def test_a_request_during_a_run_is_deferred_not_dropped(run):
    _deferred(run, ["t1"])


def test_two_requests_during_a_run_collapse_into_one(run):
    _deferred(run, ["t1", "t2"])


def test_a_request_just_before_the_tick_never_doubles_the_run(run):
    async def go():
        async with Env(engine_delay=0.3) as env:
            await env.create_hc(make_hc(name="tick", repeat=2))
            await env.wait_for(total_runs(env, "tick", 1), msg="the first run")
            await asyncio.sleep(1.6)  # the tick is due 2 s after completion
            await annotate(env.client, "tick", "t1")
            most = 0
            end = time.monotonic() + 5.0
            while time.monotonic() < end:
                flying = in_flight(check_wfs(await env.workflows(), "tick"))
                most = max(most, len(flying))
                assert most <= 1, "two check Workflows overlap"
                await asyncio.sleep(0.01)
            assert most == 1
            ann = await annotations(env, "tick")
            assert ann[RUN_HANDLED_ANNOTATION] == "t1"
            # the schedule went on: the request's run, then at least one tick
            hc = await env.get_hc("tick")
            assert hc.status.total_healthcheck_runs >= 3
            assert env.manager.reconciler.on_demand_runs == 1
            before = hc.status.total_healthcheck_runs
            await env.wait_for(total_runs(env, "tick", before + 1), msg="runs keep coming")

    run(go(), timeout=60)


def test_a_run_on_demand_that_vanishes_leaves_the_check_scheduled(run):
    """The request's run takes the pending tick's place; if its Workflow is
    gone before a result could be read, the timer is armed all the same."""

    def policy(wf):
        # the first run passes; the run on demand never ends by itself
        if (wf["metadata"].get("annotations") or {}).get(RUN_REQUEST_ANNOTATION):
            return None
        return ("Succeeded", "")

    async def go():
        async with Env(policy=policy) as env:
            rec = env.manager.reconciler
            await env.create_hc(make_hc(name="lost", repeat=3600, timeout=30))
            await env.wait_for(total_runs(env, "lost", 1), msg="the first run")
            first_timer = rec.get_timer_by_name("lost", "health")
            assert first_timer is not None
            await annotate(env.client, "lost", "t1")
            ann = await env.wait_for(handled(env, "lost", "t1"), msg="the ack")
            # submitted: the pending tick is gone, the run stands for it
            assert rec.get_timer_by_name("lost", "health") is None
            assert rec.active_watches() == 1
            await env.client.delete("argoproj.io/v1alpha1", "Workflow", "health",
                                    ann[RUN_WORKFLOW_ANNOTATION])

            async def rearmed():
                timer = rec.get_timer_by_name("lost", "health")
                return rec.active_watches() == 0 and timer

            timer = await env.wait_for(rearmed, msg="the timer to be armed again")
            assert timer is not first_timer and not timer.fired
            assert (await env.get_hc("lost")).status.total_healthcheck_runs == 1

    run(go(), timeout=45)


def test_a_paused_check_is_a_manual_only_check(run):
    async def go():
        async with Env() as env:
            rec = env.manager.reconciler
            await env.create_hc(make_hc(name="manual", repeat=0))

            async def stopped():
                hc = await env.get_hc("manual")
                return hc.status.status == "Stopped" and hc

            await env.wait_for(stopped, msg="Stopped status")
            assert await env.workflows() == []

            await annotate(env.client, "manual", "t1")
            await env.wait_for(total_runs(env, "manual", 1), msg="the manual run")

            async def stopped_after(n):
                hc = await env.get_hc("manual")
                return (hc.status.status == "Stopped"
                        and hc.status.total_healthcheck_runs == n and hc)

            hc = await env.wait_for(lambda: stopped_after(1), msg="Stopped again")
            assert hc.status.error_message == STOPPED_MESSAGE
            assert hc.status.success_count == 1 and hc.status.failed_count == 0
            ann = await annotations(env, "manual")
            assert ann[RUN_HANDLED_ANNOTATION] == "t1"
            assert hc.status.last_successful_workflow == ann[RUN_WORKFLOW_ANNOTATION]
            (wf,) = check_wfs(await env.workflows(), "manual")
            assert wf["metadata"]["name"] == ann[RUN_WORKFLOW_ANNOTATION]
            assert rec.get_timer_by_name("manual", "health") is None

            await asyncio.sleep(2.0)
            assert len(check_wfs(await env.workflows(), "manual")) == 1
            assert rec.get_timer_by_name("manual", "health") is None
            assert not rec._manual_runs and not rec._rerun_after_watch

            await annotate(env.client, "manual", "t2")
            hc = await env.wait_for(lambda: stopped_after(2), msg="the second manual run")
            assert hc.status.success_count == 2
            assert len(check_wfs(await env.workflows(), "manual")) == 2
            assert (await annotations(env, "manual"))[RUN_HANDLED_ANNOTATION] == "t2"
            assert rec.get_timer_by_name("manual", "health") is None
            assert rec.on_demand_runs == 2

    run(go(), timeout=60)


def test_a_failing_run_on_demand_triggers_the_remedy_within_its_limit(run):
    def policy(wf):
        if "-remedy-wf-" in wf["metadata"]["name"]:
            return ("Succeeded", "")
        return ("Failed", "probe failed")

    async def go():
        async with Env(policy=policy) as env:
            await env.create_hc(make_hc(
                name="sick", repeat=3600, remedy=True,
                extra_spec={"remedyRunsLimit": 2, "remedyResetInterval": 3600}))
            hc = await env.wait_for(total_runs(env, "sick", 1), msg="the first run")
            assert hc.status.failed_count == 1 and hc.status.remedy_total_runs == 1

            await annotate(env.client, "sick", "t1")
            hc = await env.wait_for(total_runs(env, "sick", 2), msg="the run on demand")
            assert hc.status.failed_count == 2 and hc.status.status == "Failed"
            assert hc.status.remedy_total_runs == 2  # the remedy ran for it

            await annotate(env.client, "sick", "t2")
            hc = await env.wait_for(total_runs(env, "sick", 3), msg="the second run on demand")
            assert hc.status.failed_count == 3
            assert hc.status.remedy_total_runs == 2  # remedyRunsLimit holds
            wfs = await env.workflows()
            assert len(check_wfs(wfs, "sick")) == 3
            assert len([w for w in wfs if "-remedy-wf-" in w["metadata"]["name"]]) == 2
            ann = await annotations(env, "sick")
            assert ann[RUN_HANDLED_ANNOTATION] == "t2"
            assert hc.status.last_failed_workflow == ann[RUN_WORKFLOW_ANNOTATION]

    run(go(), timeout=60)


def test_a_failed_ack_is_retried_without_another_run(run):
    async def go():
        async def fail_first(n):
            if n == 1:
                raise ApiError("the apiserver is having a moment")

        env = Env()
        flaky = PatchHook(env.client, fail_first)
        env.manager = Manager(flaky, max_workers=4)
        async with env:
            rec = env.manager.reconciler
            await env.create_hc(make_hc(name="flaky", repeat=3600))
            await env.wait_for(total_runs(env, "flaky", 1), msg="the first run")
            await annotate(env.client, "flaky", "t1")  # not through the hook
            ann = await env.wait_for(handled(env, "flaky", "t1"), msg="the ack, on the retry")
            assert flaky.hc_patches == 2
            await env.wait_for(total_runs(env, "flaky", 2), msg="the run on demand")
            await asyncio.sleep(1.0)
            wfs = check_wfs(await env.workflows(), "flaky")
            assert len(wfs) == 2  # the first run and exactly one on demand
            assert ann[RUN_WORKFLOW_ANNOTATION] == wfs[1]["metadata"]["name"]
            assert rec.on_demand_runs == 1
            assert not rec._run_acks

    run(go(), timeout=45)


def test_a_request_made_with_no_controller_is_served_once_at_start(run):
    async def go():
        env = Env()
        await env.create_hc(make_hc(name="waiting", repeat=3600))
        await annotate(env.client, "waiting", "t1")
        async with env:
            ann = await env.wait_for(handled(env, "waiting", "t1"), msg="the ack")
            await env.wait_for(total_runs(env, "waiting", 1), msg="the run")
            await asyncio.sleep(1.0)
            (wf,) = check_wfs(await env.workflows(), "waiting")
            assert ann[RUN_WORKFLOW_ANNOTATION] == wf["metadata"]["name"]
            assert wf["metadata"]["annotations"] == {RUN_REQUEST_ANNOTATION: "t1"}
            assert (await env.get_hc("waiting")).status.total_healthcheck_runs == 1
            assert env.manager.reconciler.on_demand_runs == 1

    run(go(), timeout=45)


def test_delete_during_the_run_leaves_no_ack_and_no_state(run, caplog):
    async def go():
        env = Env(engine_delay=0.5)

        async def delete_first(n):
            # the Workflow is submitted and watched, the ack not yet written
            if n == 1:
                assert env.manager.reconciler.active_watches() == 1
                await env.client.delete(API_VERSION, "HealthCheck", "health", "gone")

        hooked = PatchHook(env.client, delete_first)
        env.manager = Manager(hooked, max_workers=4)
        async with env:
            rec = env.manager.reconciler
            await env.create_hc(make_hc(name="gone", repeat=3600))
            await env.wait_for(total_runs(env, "gone", 1), msg="the first run")
            await annotate(env.client, "gone", "t1")

            async def forgotten():
                return hooked.hc_patches >= 1 and rec.active_watches() == 0

            await env.wait_for(forgotten, msg="the run to be dropped")
            await asyncio.sleep(0.7)  # past the moment the run would have ended
            key = ("health", "gone")
            assert hooked.hc_patches == 1  # no second try at the ack
            assert key not in rec._run_acks
            assert key not in rec._rerun_after_watch
            assert key not in rec._manual_runs
            assert key not in rec._driven_uid
            assert key not in rec._watch_tasks
            assert key not in rec.repeat_timers_by_name
            assert rec.completed_runs == 1
            assert await env.client.list(API_VERSION, "HealthCheck", "health") == []

    with caplog.at_level(logging.WARNING, logger="active_monitor_amd"):
        run(go(), timeout=45)
    assert [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING] == []


def test_only_the_owning_shard_serves_a_request(run):
    names = {}
    i = 0
    while len(names) < 2:
        names.setdefault(shard_of(f"sh-{i}", 2), f"sh-{i}")
        i += 1

    async def go():
        env = Env()
        env.manager = Manager(env.client, max_workers=2, shard_index=0, shard_count=2)
        other = Manager(env.client, max_workers=2, shard_index=1, shard_count=2)
        async with env:
            await other.start()
            try:
                for name in names.values():
                    await env.create_hc(make_hc(name=name, repeat=3600))
                for name in names.values():
                    await env.wait_for(total_runs(env, name, 1), msg=f"first run of {name}")
                await annotate(env.client, names[1], "t1")
                await env.wait_for(total_runs(env, names[1], 2), msg="the run on demand")
                await env.wait_for(handled(env, names[1], "t1"), msg="the ack")
                await asyncio.sleep(1.0)
                wfs = await env.workflows()
                assert len(check_wfs(wfs, names[1])) == 2  # served once
                assert len(check_wfs(wfs, names[0])) == 1
                assert other.reconciler.on_demand_runs == 1
                assert env.manager.reconciler.on_demand_runs == 0
                assert other.reconciler.completed_runs == 2
                assert env.manager.reconciler.completed_runs == 1
            finally:
                await other.stop()

    run(go(), timeout=45)

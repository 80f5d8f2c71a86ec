"""Admission in the workflow engine: ``parallelism``, ``namespace_parallelism``,
``spec.priority``, mutexes, deletion and expiry in the queue, recovery of
``Pending`` workflows and ``stop()`` with a queue.

Every leaf appends its workflow's name to ``started`` and then waits for the
test to create ``release.NAME``, so what runs at a given moment is counted,
not guessed from timing.
"""
import asyncio
import time

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine, engines

WF = (WF_API_VERSION, WF_KIND)


def spec_for(tmp, name, **extra):
    script = (f"echo {name} >> {tmp}/started; "
              f"while [ ! -e {tmp}/release.{name} ]; do sleep 0.02; done")
    return {"entrypoint": "main",
            "templates": [{"name": "main", "container": {"command": ["sh", "-c", script]}}],
            **extra}


def workflow(tmp, name, ns="a", status=None, created=None, **extra):
    obj = {"apiVersion": WF_API_VERSION, "kind": WF_KIND,
           "metadata": {"name": name, "namespace": ns},
           "spec": spec_for(tmp, name, **extra)}
    if created:
        obj["metadata"]["creationTimestamp"] = created
    if status:
        obj["status"] = status
    return obj


def started(tmp):
    path = tmp / "started"
    return path.read_text().split() if path.exists() else []


def release(tmp, *names):
    for name in names:
        (tmp / f"release.{name}").touch()


async def until(pred, what, timeout=10.0):
    deadline = time.monotonic() + timeout
    while time.monotonic() < deadline:
        value = pred()
        if asyncio.iscoroutine(value):
            value = await value
        if value:
            return value
        await asyncio.sleep(0.01)
    raise AssertionError(f"timed out waiting for {what}")


class Stack:
    def __init__(self, tmp, server=None, **engine_options):
        self.tmp = tmp
        self.server = server or MemoryApiServer()
        self.client = MemoryClient(self.server)
        self.engine = LocalWorkflowEngine(self.client, ttl_seconds=None, **engine_options)

    async def __aenter__(self):
        await self.engine.start()
        return self

    async def __aexit__(self, *exc):
        await self.engine.stop()

    async def create(self, name, ns="a", **extra):
        await self.client.create(workflow(self.tmp, name, ns, **extra))

    async def status(self, name, ns="a"):
        return (await self.client.get(*WF, ns, name)).get("status") or {}

    async def phase(self, name, ns="a"):
        return (await self.status(name, ns)).get("phase")

    async def pending(self, *names, ns="a"):
        for name in names:
            if await self.phase(name, ns) != "Pending":
                return False
        return True

    async def all_in(self, phase, *names, ns="a"):
        for name in names:
            if await self.phase(name, ns) != phase:
                return False
        return True


def test_parallelism_queues_what_does_not_fit_and_admits_the_oldest_first(run, tmp_path):
    names = [f"w{i}" for i in range(5)]

    async def go():
        async with Stack(tmp_path, parallelism=2) as s:
            for name in names:
                await s.create(name)
            await until(lambda: len(started(tmp_path)) >= 2, "two leaves")
            await until(lambda: s.pending("w2", "w3", "w4"), "three Pending")
            assert sorted(started(tmp_path)) == ["w0", "w1"]
            for name in ("w2", "w3", "w4"):
                st = await s.status(name)
                assert st == {"phase": "Pending", "message": engines.POSTPONED_MESSAGE}
            assert s.engine.stats()["running"] == 2
            assert s.engine.stats()["queued"] == 3

            release(tmp_path, "w0")
            await until(lambda: len(started(tmp_path)) >= 3, "a third leaf")
            await until(lambda: s.all_in("Succeeded", "w0"), "w0 to finish")
            assert started(tmp_path)[2] == "w2"
            stats = s.engine.stats()
            assert (stats["running"], stats["queued"]) == (2, 2)
            assert len(started(tmp_path)) == 3

            release(tmp_path, *names)
            await until(lambda: s.all_in("Succeeded", *names), "all to succeed")
            stats = s.engine.stats()
            assert stats["postponed_total"] == 3
            assert (stats["running"], stats["queued"]) == (0, 0)
            assert stats["limits"] == {"parallelism": 2, "namespace_parallelism": None,
                                       "max_processes": None}
            assert started(tmp_path)[3:] == ["w3", "w4"]

    run(go(), timeout=30)


def test_higher_priority_leaves_the_queue_first(run, tmp_path):
    async def go():
        async with Stack(tmp_path, parallelism=1) as s:
            await s.create("blocker")
            await until(lambda: started(tmp_path) == ["blocker"], "the blocker")
            await s.create("p0", priority=0)
            await s.create("p5", priority=5)
            await s.create("p1", priority=1)
            await until(lambda: s.pending("p0", "p5", "p1"), "three Pending")
            release(tmp_path, "blocker", "p0", "p5", "p1")
            await until(lambda: s.all_in("Succeeded", "p0", "p5", "p1"), "all to succeed")
            assert started(tmp_path) == ["blocker", "p5", "p1", "p0"]

    run(go(), timeout=30)


def test_namespace_parallelism_holds_back_only_its_namespace(run, tmp_path):
    async def go():
        async with Stack(tmp_path, namespace_parallelism=1) as s:
            await s.create("a1", ns="a")
            await s.create("a2", ns="a")
            await s.create("b1", ns="b")
            await until(lambda: sorted(started(tmp_path)) == ["a1", "b1"], "a1 and b1")
            await until(lambda: s.pending("a2"), "a2 Pending")
            assert (await s.status("a2"))["message"] == engines.POSTPONED_MESSAGE
            assert await s.phase("b1", "b") == "Running"
            release(tmp_path, "a1")
            await until(lambda: "a2" in started(tmp_path), "a2 to start")
            release(tmp_path, "a2", "b1")
            await until(lambda: s.all_in("Succeeded", "a1", "a2"), "a to succeed")
            await until(lambda: s.all_in("Succeeded", "b1", ns="b"), "b to succeed")

    run(go(), timeout=30)


def test_deleted_while_queued_never_runs_and_passes_the_slot_on(run, tmp_path):
    async def go():
        async with Stack(tmp_path, parallelism=1) as s:
            await s.create("first")
            await until(lambda: started(tmp_path) == ["first"], "the first")
            await s.create("doomed")
            await s.create("next")
            await until(lambda: s.pending("doomed", "next"), "two Pending")
            await s.client.delete(*WF, "a", "doomed")
            await until(lambda: s.engine.stats()["queued"] == 1, "the queue to shrink")
            release(tmp_path, "first", "doomed", "next")
            await until(lambda: s.all_in("Succeeded", "first", "next"), "both to succeed")
            assert started(tmp_path) == ["first", "next"]
            await until(lambda: s.engine.stats()["running"] == 0, "nothing running")
            assert s.engine.stats()["queued"] == 0

    run(go(), timeout=30)


def test_deadline_runs_out_in_the_queue(run, tmp_path):
    async def go():
        async with Stack(tmp_path, parallelism=1) as s:
            await s.create("blocker")
            await until(lambda: started(tmp_path) == ["blocker"], "the blocker")
            await s.create("late", activeDeadlineSeconds=1)
            await until(lambda: s.all_in("Failed", "late"), "late to expire", timeout=5)
            st = await s.status("late")
            assert st["message"] == engines.QUEUE_EXPIRED_MESSAGE
            assert st["finishedAt"]
            assert "nodes" not in st and "outputs" not in st and "startedAt" not in st
            assert started(tmp_path) == ["blocker"]
            assert await s.phase("blocker") == "Running"
            stats = s.engine.stats()
            assert stats["expired_in_queue"] == 1
            assert (stats["running"], stats["queued"]) == (1, 0)
            release(tmp_path, "blocker")
            await until(lambda: s.all_in("Succeeded", "blocker"), "the blocker to succeed")
            assert started(tmp_path) == ["blocker"]

    run(go(), timeout=30)


def test_mutex_excludes_within_a_namespace_without_any_limit(run, tmp_path):
    gpu0 = {"mutex": {"name": "gpu0"}}

    async def go():
        async with Stack(tmp_path) as s:
            await s.create("one", synchronization=gpu0)
            await s.create("two", synchronization={"mutexes": [{"name": "gpu0"}]})
            await s.create("other", synchronization={"mutex": {"name": "gpu1"}})
            await s.create("elsewhere", ns="b", synchronization=gpu0)
            await until(lambda: len(started(tmp_path)) >= 3, "three leaves")
            await until(lambda: s.pending("two"), "two Pending")
            assert sorted(started(tmp_path)) == ["elsewhere", "one", "other"]
            assert await s.status("two") == {
                "phase": "Pending", "message": "Waiting for a/Mutex/gpu0 lock"}

            # wants a free mutex and a held one: takes neither
            await s.create("both", synchronization={
                "mutexes": [{"name": "gpu2"}, {"name": "gpu0"}]})
            await until(lambda: s.pending("both"), "both Pending")
            assert (await s.status("both"))["message"] == "Waiting for a/Mutex/gpu0 lock"
            await s.create("free", synchronization={"mutex": {"name": "gpu2"}})
            await until(lambda: "free" in started(tmp_path), "gpu2 to be free")
            assert "two" not in started(tmp_path)

            release(tmp_path, "one")
            await until(lambda: "two" in started(tmp_path), "two to start")
            assert await s.phase("one") == "Succeeded"
            assert "both" not in started(tmp_path)
            release(tmp_path, "two", "other", "elsewhere", "free", "both")
            await until(lambda: s.all_in("Succeeded", "two", "other", "free", "both"),
                        "a to succeed")
            await until(lambda: s.all_in("Succeeded", "elsewhere", ns="b"), "b to succeed")
            assert s.engine.stats()["postponed_total"] == 2

    run(go(), timeout=30)


def test_without_limits_or_mutexes_a_workflow_is_written_twice_and_never_pending(
        run, tmp_path):
    class Counting(MemoryClient):
        def __init__(self, server):
            super().__init__(server)
            self.phases = []

        async def update(self, obj):
            if obj.get("kind") == WF_KIND:
                self.phases.append((obj["metadata"]["name"],
                                    (obj.get("status") or {}).get("phase")))
            return await super().update(obj)

    async def go():
        client = Counting(MemoryApiServer())
        engine = LocalWorkflowEngine(client, ttl_seconds=None)
        await engine.start()
        try:
            names = [f"w{i}" for i in range(4)]
            release(tmp_path, *names)
            for name in names:
                await client.create(workflow(tmp_path, name))

            async def done():
                objs = await client.list(*WF, "a")
                return all((o.get("status") or {}).get("phase") == "Succeeded" for o in objs)

            await until(done, "all to succeed")
            for name in names:
                assert [p for n, p in client.phases if n == name] == ["Running", "Succeeded"]
        finally:
            await engine.stop()

    run(go(), timeout=30)


def test_semaphores_and_template_synchronization_are_ignored_with_one_warning(
        run, tmp_path, caplog):
    async def go():
        async with Stack(tmp_path) as s:
            release(tmp_path, "sem")
            spec = spec_for(tmp_path, "sem", synchronization={
                "semaphore": {"configMapKeyRef": {"name": "limits", "key": "gpu"}}})
            spec["templates"][0]["synchronization"] = {"mutex": {"name": "inner"}}
            await s.client.create({"apiVersion": WF_API_VERSION, "kind": WF_KIND,
                                   "metadata": {"name": "sem", "namespace": "a"}, "spec": spec})
            await until(lambda: s.all_in("Succeeded", "sem"), "sem to succeed")
            assert s.engine.stats()["postponed_total"] == 0

    with caplog.at_level("WARNING", logger="active_monitor_amd.workflow"):
        run(go(), timeout=30)
    warnings = [r.getMessage() for r in caplog.records if r.levelname == "WARNING"]
    assert len(warnings) == 1
    assert "semaphores" in warnings[0] and "template-level synchronization (main)" in warnings[0]


def test_a_pending_workflow_is_recovered_and_runs(run, tmp_path):
    async def go():
        server = MemoryApiServer()
        release(tmp_path, "left")
        server.create(workflow(tmp_path, "left", status={
            "phase": "Pending", "message": engines.POSTPONED_MESSAGE}))
        async with Stack(tmp_path, server=server, recover=True) as s:
            await until(lambda: s.all_in("Succeeded", "left"), "left to succeed")
            assert started(tmp_path) == ["left"]

    run(go(), timeout=30)


def test_recovered_pending_workflows_run_one_by_one_in_creation_order(run, tmp_path):
    async def go():
        server = MemoryApiServer()
        pending = {"phase": "Pending", "message": engines.POSTPONED_MESSAGE}
        # stored newest first: the order has to come from creationTimestamp
        server.create(workflow(tmp_path, "newer", status=dict(pending),
                               created="2024-05-01T10:00:07Z"))
        server.create(workflow(tmp_path, "older", status=dict(pending),
                               created="2024-05-01T10:00:03Z"))
        async with Stack(tmp_path, server=server, recover=True, parallelism=1) as s:
            await until(lambda: started(tmp_path) == ["older"], "the older one")
            assert await s.phase("newer") == "Pending"
            assert s.engine.stats()["queued"] == 1
            release(tmp_path, "older")
            await until(lambda: started(tmp_path) == ["older", "newer"], "the newer one")
            assert await s.phase("older") == "Succeeded"
            release(tmp_path, "newer")
            await until(lambda: s.all_in("Succeeded", "newer"), "newer to succeed")

    run(go(), timeout=30)


def test_stop_leaves_the_queue_pending_and_kills_what_runs(run, tmp_path):
    async def go():
        s = Stack(tmp_path, parallelism=1)
        await s.engine.start()
        try:
            await s.create("running")
            await until(lambda: started(tmp_path) == ["running"], "the running one")
            await s.create("q1")
            await s.create("q2")
            await until(lambda: s.pending("q1", "q2"), "two Pending")
        finally:
            await s.engine.stop()
        # the leaf is gone: releasing it now starts nothing, here or in the queue
        release(tmp_path, "running", "q1", "q2")
        assert await s.pending("q1", "q2")
        assert "startedAt" not in await s.status("q1")
        assert await s.phase("running") == "Running"  # as today: killed, not finished
        assert s.engine.stats()["queued"] == 2
        assert not s.engine._tasks
        assert started(tmp_path) == ["running"]

    run(go(), timeout=30)


def test_stop_kills_the_run_of_a_workflow_whose_name_was_created_again(run, tmp_path):
    finished = tmp_path / "finished"
    script = (f"echo x >> {tmp_path}/started; "
              f"while [ ! -e {tmp_path}/release.x ]; do sleep 0.02; done; "
              f"echo x >> {finished}")
    wf = workflow(tmp_path, "x")
    wf["spec"]["templates"][0]["container"]["command"] = ["sh", "-c", script]

    async def go():
        s = Stack(tmp_path)
        await s.engine.start()
        try:
            await s.client.create(wf)
            await until(lambda: started(tmp_path) == ["x"], "the first run")
            await s.client.delete(*WF, "a", "x")
            await s.client.create(wf)
            await until(lambda: started(tmp_path) == ["x", "x"], "the second run")
            # both runs are in flight, the first one's Workflow is gone
            assert s.engine.stats()["running"] == 2
        finally:
            await s.engine.stop()
        assert not s.engine._tasks
        release(tmp_path, "x")
        await asyncio.sleep(0.5)
        assert not finished.exists()

    run(go(), timeout=30)

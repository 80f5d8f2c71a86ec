"""The workflow log store on its own, and the executor's drain loop over it."""
import asyncio
import os
import time

import pytest

from active_monitor_amd.kube.errors import NotFoundError
from active_monitor_amd.workflow.executor import RESULT_MAX_BYTES, WorkflowRun
from active_monitor_amd.workflow.logs import LogStore

KIB = 1024


async def collect(stream):
    return b"".join([chunk async for chunk in stream])


def files_under(path):
    return sorted(
        os.path.join(root, f) for root, _, names in os.walk(path) for f in names
    )


def bytes_under(path):
    return sum(os.path.getsize(f) for f in files_under(path))


# -- reading ----------------------------------------------------------------


def test_nodes_in_start_order_and_followed_lines_in_arrival_order(run, tmp_path):
    async def go():
        store = LogStore(str(tmp_path / "logs"))
        store.start_run("ns", "wf")
        followed = store.read("ns", "wf", follow=True, prefix=True)
        task = asyncio.ensure_future(collect(followed))
        await asyncio.sleep(0)  # the follower stands before the first write
        a = store.writer("ns", "wf", "wf.a", "a")
        b = store.writer("ns", "wf", "wf.b", "b")
        a.write(b"a1\n")
        b.write(b"b1\n")
        a.write(b"a2\na")
        b.write(b"b2\n")
        a.write(b"3\n")  # completes the partial line "a3"
        a.close()
        b.close()
        await asyncio.sleep(0.05)
        assert not task.done()  # only finish_run ends a followed read
        store.finish_run("ns", "wf")
        assert await asyncio.wait_for(task, 5) == (
            b"a: a1\nb: b1\na: a2\nb: b2\na: a3\n")

        assert await collect(store.read("ns", "wf")) == b"a1\na2\na3\nb1\nb2\n"
        assert await collect(store.read("ns", "wf", prefix=True)) == (
            b"a: a1\na: a2\na: a3\nb: b1\nb: b2\n")
        # tail_lines applies to each node
        assert await collect(store.read("ns", "wf", tail_lines=1)) == b"a3\nb2\n"
        assert await collect(store.read("ns", "wf", tail_lines=0)) == b""
        assert await collect(store.read("ns", "wf", limit_bytes=4)) == b"a1\na"
        # by id, else by display name
        assert await collect(store.read("ns", "wf", node="wf.b")) == b"b1\nb2\n"
        assert await collect(store.read("ns", "wf", node="a")) == b"a1\na2\na3\n"
        # following a finished run serves it and ends
        assert await asyncio.wait_for(
            collect(store.read("ns", "wf", follow=True)), 5) == b"a1\na2\na3\nb1\nb2\n"
        store.close()

    run(go())


def test_follow_started_midway_serves_each_line_once(run, tmp_path):
    async def go():
        store = LogStore(str(tmp_path / "logs"))
        w = store.writer("ns", "wf", "n", "n")
        w.write(b"one\n")
        stream = store.read("ns", "wf", follow=True)
        w.write(b"two\n")  # after read(), before the first __anext__
        task = asyncio.ensure_future(collect(stream))
        await asyncio.sleep(0)
        w.write(b"three\n")
        late = store.writer("ns", "wf", "m", "m")  # a node that starts later
        late.write(b"four\n")
        store.finish_run("ns", "wf")
        assert await asyncio.wait_for(task, 5) == b"one\ntwo\nthree\nfour\n"
        store.close()

    run(go())


def test_unknown_run_or_node_is_not_found(run, tmp_path):
    async def go():
        store = LogStore(str(tmp_path / "logs"))
        with pytest.raises(NotFoundError):
            store.read("ns", "nothing")
        store.writer("ns", "wf", "n", "n").close()
        with pytest.raises(NotFoundError):
            store.read("ns", "wf", node="other")
        store.finish_run("ns", "wf")
        with pytest.raises(NotFoundError):
            store.read("ns", "wf", node="other", follow=True)
        store.discard("ns", "wf")
        with pytest.raises(NotFoundError):
            store.read("ns", "wf")
        store.close()

    run(go())


# -- caps -------------------------------------------------------------------


@pytest.mark.parametrize("newlines", [True, False], ids=["short-lines", "no-newline"])
def test_per_node_cap(run, tmp_path, newlines):
    cap = 64 * KIB
    total = 8 * cap

    async def go():
        store = LogStore(str(tmp_path / "logs"), max_node_bytes=cap)
        w = store.writer("ns", "wf", "n", "n")
        if newlines:
            line = b"%07d\n"  # 8 bytes a line
            written = b"".join(line % i for i in range(total // 8))
        else:
            written = bytes(i % 251 for i in range(total))
        assert len(written) == total
        node_files = lambda: [f for f in files_under(tmp_path / "logs")  # noqa: E731
                              if os.path.basename(f) != "index"]
        step = 5000  # no multiple of the line length or of the segment size
        for at in range(0, total, step):
            w.write(written[at:at + step])
            assert sum(os.path.getsize(f) for f in node_files()) <= cap
        w.close()
        store.finish_run("ns", "wf")
        assert bytes_under(tmp_path / "logs") <= cap + 256  # the index line
        served = await collect(store.read("ns", "wf"))
        head, _, payload = served.partition(b"\n")
        assert head.startswith(b"[log truncated: ") and head.endswith(b" bytes dropped]")
        dropped = int(head.split()[2])
        assert dropped + len(payload) == total
        assert len(payload) >= cap // 2
        assert payload == written[dropped:]  # the newest bytes, none missing
        if newlines:
            assert payload[:8] == b"%07d\n" % (dropped // 8)  # cut at a line start
        store.close()

    run(go())


def test_total_cap_drops_oldest_finished_runs_first(run, tmp_path):
    async def go():
        store = LogStore(str(tmp_path / "logs"), max_node_bytes=256 * KIB,
                         max_total_bytes=100 * KIB)
        line = b"x" * 1023 + b"\n"
        open_writer = store.writer("ns", "open", "n", "n")
        open_writer.write(line * 10)
        for name in ("first", "second", "third"):
            w = store.writer("ns", name, "n", "n")
            w.write(line * 40)
            w.close()
            store.finish_run("ns", name)
        open_writer.write(line * 10)
        # 140 KiB were written: the two oldest finished runs had to go
        assert store.runs() == [("ns", "open"), ("ns", "third")]
        assert sorted(os.listdir(tmp_path / "logs" / "ns")) == ["open", "third"]
        assert store.total_bytes <= 100 * KIB
        assert bytes_under(tmp_path / "logs") <= 100 * KIB
        open_writer.close()
        assert await collect(store.read("ns", "open")) == line * 20
        assert await collect(store.read("ns", "third")) == line * 40
        # an open run is never dropped, however far over the cap it goes
        big = store.writer("ns", "big", "n", "n")
        big.write(line * 120)
        assert store.runs() == [("ns", "open"), ("ns", "big")]
        assert await collect(store.read("ns", "big")) == line * 120
        store.close()

    run(go())


# -- paths ------------------------------------------------------------------


def test_no_file_outside_the_store_directory(run, tmp_path):
    root = tmp_path / "data" / "logs"

    async def go():
        store = LogStore(str(root))
        for i, item in enumerate(["/", "../x"]):
            w = store.writer("ns", "wf", f"wf.dir({i}:{item})", f"dir({i}:{item})")
            w.write(b"listing of %s\n" % item.encode())
            w.close()
        assert await collect(store.read("ns", "wf", node="wf.dir(1:../x)")) == (
            b"listing of ../x\n")
        assert await collect(store.read("ns", "wf", node="dir(0:/)")) == b"listing of /\n"
        for namespace, name in [("../ns", "wf"), ("ns", "../wf"), ("a/b", "wf"),
                                ("ns", "a/b"), ("..", "wf"), ("ns", ".."),
                                ("ns", "/abs"), ("ns", "")]:
            with pytest.raises(ValueError):
                store.start_run(namespace, name)
            with pytest.raises(ValueError):
                store.writer(namespace, name, "n", "n")
            with pytest.raises(NotFoundError):
                store.read(namespace, name)
            store.discard(namespace, name)
        store.close()

    run(go())
    inside = str(root) + os.sep
    for path in files_under(tmp_path):
        assert path.startswith(inside), path
    # and the only names below it are the generated ones
    assert sorted(os.listdir(root / "ns" / "wf")) == ["0.0", "1.0", "index"]


# -- restart ----------------------------------------------------------------


def test_reopening_a_directory(run, tmp_path):
    d = str(tmp_path / "logs")

    async def go():
        first = LogStore(d, max_node_bytes=4 * KIB)
        for name in ("kept", "gone"):
            w = first.writer("ns", name, f"{name}.main", "main")
            w.write(b"hello from %s\n" % name.encode())
            w.close()
            first.finish_run("ns", name)
        w = first.writer("ns", "killed", "killed.main", "main")
        w.write(b"partial\n" * 1024)  # twice the cap: a segment was dropped
        w.write(b"no newline yet")
        # the process is killed here: no close(), no finish_run()
        del first, w

        store = LogStore.open(d, live=[("ns", "kept"), ("ns", "killed"),
                                       ("ns", "never-ran")],
                              max_node_bytes=4 * KIB)
        assert sorted(store.runs()) == [("ns", "kept"), ("ns", "killed")]
        assert sorted(os.listdir(tmp_path / "logs" / "ns")) == ["kept", "killed"]
        assert await collect(store.read("ns", "kept", node="main")) == b"hello from kept\n"
        with pytest.raises(NotFoundError):
            store.read("ns", "gone")
        # the unclosed node is served as it stands on disk, and a follow ends
        served = await asyncio.wait_for(
            collect(store.read("ns", "killed", follow=True)), 5)
        head, _, payload = served.partition(b"\n")
        dropped = int(head.split()[2])
        assert dropped % 8 == 0 and dropped + len(payload) == 8 * 1024
        assert payload == b"partial\n" * (len(payload) // 8)
        assert store.total_bytes == bytes_under(tmp_path / "logs")
        # a second run of the same name starts over, it does not append
        w = store.writer("ns", "killed", "killed.main", "main")
        w.write(b"again\n")
        w.close()
        assert await collect(store.read("ns", "killed")) == b"again\n"
        store.close()
        assert os.path.isdir(d)  # a directory that was given is kept

        # without a live set nothing is removed
        again = LogStore.open(d)
        assert sorted(again.runs()) == [("ns", "kept"), ("ns", "killed")]
        again.close()

    run(go())


def test_a_store_without_a_directory_cleans_up(run):
    async def go():
        store = LogStore()
        w = store.writer("ns", "wf", "n", "n")
        w.write(b"x\n")
        assert os.path.basename(store.directory).startswith("am-logs-")
        assert os.path.isdir(store.directory)
        store.close()
        assert not os.path.exists(store.directory)

    run(go())


# -- the executor -----------------------------------------------------------


def leaf_spec(script, **extra):
    return {"entrypoint": "main", "templates": [
        {"name": "main", "container": {"command": ["sh", "-c", script]}}], **extra}


def without_times(nodes):
    return {k: {f: v for f, v in n.items() if f not in ("startedAt", "finishedAt")}
            for k, n in nodes.items()}


def test_failing_leaf_keeps_both_streams_and_its_message(run):
    async def go():
        store = LogStore()
        wf = WorkflowRun(leaf_spec("echo out; echo err >&2; exit 3"), "wf", "ns", logs=store)
        assert await wf.run_entrypoint() == ("Failed", "exit code 3: err\n")
        assert wf.nodes["wf"]["message"] == "exit code 3: err\n"
        log = await collect(store.read("ns", "wf"))
        assert sorted(log.splitlines()) == [b"err", b"out"]
        store.close()

    run(go())


def test_succeeding_leaf_is_the_same_with_and_without_a_store(run):
    spec = {"entrypoint": "main", "templates": [
        {"name": "main", "steps": [[{"name": "a", "template": "say"}],
                                   [{"name": "b", "template": "fail"}]]},
        {"name": "say", "script": {"command": ["sh"],
                                   "source": "echo result; echo noise >&2\n"}},
        {"name": "fail", "container": {"command": ["sh", "-c", "echo only-out; exit 2"]}},
    ]}

    async def go():
        store = LogStore()
        with_store = WorkflowRun(spec, "wf", "ns", logs=store)
        without = WorkflowRun(spec, "wf", "ns", logs=None)
        assert await with_store.run_entrypoint() == await without.run_entrypoint()
        assert with_store.nodes["wf[0].a"]["outputs"] == {"result": "result"}
        # stderr is empty: the message falls back to stdout, as before
        assert with_store.nodes["wf[1].b"]["message"] == "exit code 2: only-out\n"
        assert without_times(with_store.nodes) == without_times(without.nodes)
        assert await collect(store.read("ns", "wf", node="a")) in (
            b"result\nnoise\n", b"noise\nresult\n")
        store.close()

    run(go())


def test_long_failure_message_is_the_last_500_characters(run):
    # multi-byte characters, and a length that is no multiple of any chunk
    script = "i=0; while [ $i -lt 700 ]; do printf 'é%d-' $i >&2; i=$((i+1)); done; exit 1"

    async def go():
        wf = WorkflowRun(leaf_spec(script), "wf", "ns")
        phase, message = await wf.run_entrypoint()
        whole = "".join(f"é{i}-" for i in range(700))
        assert (phase, message) == ("Failed", "exit code 1: " + whole[-500:])

    run(go())


@pytest.mark.parametrize("with_store", [False, True], ids=["logs-none", "64KiB-cap"])
def test_chatty_leaf_finishes_and_keeps_the_first_64k(run, with_store):
    script = "head -c 4194304 /dev/zero | tr '\\0' q"

    async def go():
        store = LogStore(max_node_bytes=64 * KIB) if with_store else None
        wf = WorkflowRun(leaf_spec(script), "wf", "ns", logs=store)
        assert await wf.run_entrypoint() == ("Succeeded", "")
        assert RESULT_MAX_BYTES == 64 * KIB
        assert wf.nodes["wf"]["outputs"]["result"] == "q" * RESULT_MAX_BYTES
        if store is not None:
            assert bytes_under(store.directory) <= 64 * KIB + 256
            served = await collect(store.read("ns", "wf"))
            head, _, payload = served.partition(b"\n")
            assert int(head.split()[2]) + len(payload) == 4 * KIB * KIB
            store.close()

    run(go())


def test_deadline_keeps_what_was_printed_before_the_kill(run):
    from active_monitor_amd.kube import MemoryApiServer, MemoryClient
    from active_monitor_amd.workflow import LocalWorkflowEngine

    async def go():
        store = LogStore()
        client = MemoryClient(MemoryApiServer())
        engine = LocalWorkflowEngine(client, ttl_seconds=None, logs=store)
        sub = client.watch("argoproj.io/v1alpha1", "Workflow", "ns")
        await engine.start()
        try:
            await client.create({
                "apiVersion": "argoproj.io/v1alpha1", "kind": "Workflow",
                "metadata": {"name": "hung", "namespace": "ns"},
                "spec": leaf_spec("echo before; sleep 30", activeDeadlineSeconds=1),
            })
            async for ev in sub:
                status = ev["object"].get("status") or {}
                if status.get("phase") in ("Succeeded", "Failed"):
                    break
        finally:
            sub.close()
            await engine.stop()
        assert status["phase"] == "Failed" and status["message"] == "deadline exceeded"
        # finished: a follow ends by itself
        log = await asyncio.wait_for(collect(store.read("ns", "hung", follow=True)), 2)
        assert log == b"before\n"
        store.close()

    started = time.monotonic()
    run(go())
    assert time.monotonic() - started < 5

"""The Workflows' ``log`` subresource over loopback: apiserver frontend,
HttpClient and the local engine around one log store."""
import asyncio
import os
import time

import aiohttp
import pytest

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.errors import BadRequestError, NotFoundError
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import LocalWorkflowEngine, ScriptedWorkflowEngine
from active_monitor_amd.workflow.logs import LogStore

WF = ("argoproj.io/v1alpha1", "Workflow")
BASE = "/apis/argoproj.io/v1alpha1/namespaces/health/workflows"


def workflow(name, spec):
    return {"apiVersion": WF[0], "kind": WF[1],
            "metadata": {"name": name, "namespace": "health"}, "spec": spec}


def sh(script, **extra):
    return {"entrypoint": "main", "templates": [
        {"name": "main", "container": {"command": ["sh", "-c", script]}}], **extra}


TWO_STEPS = {"entrypoint": "main", "templates": [
    {"name": "main", "steps": [[{"name": "first", "template": "say",
                                 "arguments": {"parameters": [{"name": "t", "value": "one"}]}}],
                               [{"name": "second", "template": "say",
                                 "arguments": {"parameters": [{"name": "t", "value": "two"}]}}]]},
    {"name": "say", "inputs": {"parameters": [{"name": "t"}]},
     "container": {"command": ["echo", "{{inputs.parameters.t}}"]}},
]}


class Env:
    """Store, log store, local engine, frontend and a client, on loopback."""

    def __init__(self, server=None, logs=None, ttl=None, tokens=None, recover=False,
                 engine=LocalWorkflowEngine):
        self.server = server or MemoryApiServer()
        self.logs = logs
        self.memory = MemoryClient(self.server)
        options = {"logs": logs} if engine is LocalWorkflowEngine else {}
        self.engine = engine(self.memory, ttl_seconds=ttl, recover=recover, **options)
        self.frontend = ApiServerFrontend(self.server, accepted_tokens=tokens, logs=logs)
        self.token = next(iter(tokens)) if tokens else None

    async def __aenter__(self):
        await self.frontend.start()
        await self.engine.start()
        self.client = HttpClient(self.frontend.url, token=self.token, qps=0)
        await self.client.start()
        self.http = aiohttp.ClientSession()
        return self

    async def __aexit__(self, *exc):
        await self.http.close()
        await self.client.close()
        await self.engine.stop()
        await self.frontend.stop()

    async def finished(self, name, timeout=10.0):
        return await self.phase_in(name, ("Succeeded", "Failed"), timeout)

    async def phase_in(self, name, phases, timeout=10.0):
        deadline = time.monotonic() + timeout
        while time.monotonic() < deadline:
            wf = await self.memory.get(*WF, "health", name)
            if (wf.get("status") or {}).get("phase") in phases:
                return wf
            await asyncio.sleep(0.01)
        raise AssertionError(f"{name} did not reach {phases}")

    async def get(self, path, method="GET", **kwargs):
        async with self.http.request(method, self.frontend.url + path, **kwargs) as resp:
            return resp.status, resp.headers, await resp.read()

    async def text(self, name, **kwargs):
        return b"".join([c async for c in self.client.logs("health", name, **kwargs)])


def test_get_of_a_finished_workflow(run):
    async def go():
        logs = LogStore()
        async with Env(logs=logs) as env:
            await env.memory.create(workflow("two", TWO_STEPS))
            await env.finished("two")
            status, headers, body = await env.get(f"{BASE}/two/log")
            assert status == 200 and body == b"one\ntwo\n"
            assert headers["Content-Type"] == "text/plain"
            assert headers["Content-Length"] == "8"
            assert "Transfer-Encoding" not in headers
            assert await env.text("two") == b"one\ntwo\n"
            assert await env.text("two", node="two[1].second") == b"two\n"  # by id
            assert await env.text("two", node="first") == b"one\n"  # by display name
            assert await env.text("two", prefix=True) == b"first: one\nsecond: two\n"
            assert await env.text("two", limit_bytes=5) == b"one\nt"
            assert await env.text("two", tail_lines=0) == b""
            # the connection is kept alive after a log
            status, _, _ = await env.get(f"{BASE}/two")
            assert status == 200
        logs.close()

    run(go())


def test_follow_streams_while_running_and_ends_with_the_run(run):
    async def go():
        logs = LogStore()
        async with Env(logs=logs) as env:
            await env.memory.create(workflow("slow", sh("echo one; sleep 0.5; echo two")))
            await env.phase_in("slow", ("Running",))
            stream = env.client.logs("health", "slow", follow=True)
            first = await asyncio.wait_for(stream.__anext__(), 5)
            assert first == b"one\n"
            wf = await env.memory.get(*WF, "health", "slow")
            assert wf["status"]["phase"] == "Running"
            # the server ends the stream: the client never closes it
            rest = await asyncio.wait_for(_drain(stream), 5)
            assert rest == b"two\n"
            assert (await env.finished("slow"))["status"]["phase"] == "Succeeded"
            assert env.frontend._live_subs == []

            # the raw response is chunked and closes the connection
            async with env.http.get(env.frontend.url + f"{BASE}/slow/log?follow=true") as resp:
                assert resp.status == 200
                assert resp.headers["Transfer-Encoding"] == "chunked"
                assert resp.headers["Content-Type"] == "text/plain"
                assert await resp.read() == b"one\ntwo\n"
        logs.close()

    run(go())


async def _drain(stream):
    return b"".join([c async for c in stream])


def test_kick_watches_ends_a_followed_log(run):
    async def go():
        logs = LogStore()
        async with Env(logs=logs) as env:
            await env.memory.create(workflow("long", sh("echo up; sleep 30")))
            await env.phase_in("long", ("Running",))
            stream = env.client.logs("health", "long", follow=True)
            assert await asyncio.wait_for(stream.__anext__(), 5) == b"up\n"
            env.frontend.kick_watches()
            assert await asyncio.wait_for(_drain(stream), 5) == b""
        logs.close()

    run(go())


def test_404_400_405(run):
    async def go():
        logs = LogStore()
        async with Env(logs=logs) as env:
            await env.memory.create(workflow("ran", sh("echo hi")))
            await env.finished("ran")

            status, _, body = await env.get(f"{BASE}/missing/log")
            assert status == 404 and b'"kind":"Status"' in body.replace(b" ", b"")
            with pytest.raises(NotFoundError, match="missing"):
                await env.text("missing")

            with pytest.raises(NotFoundError, match="has no node 'nope'"):
                await env.text("ran", node="nope")

            with pytest.raises(BadRequestError, match="tailLines"):
                await env.text("ran", tail_lines="x")
            status, _, _ = await env.get(f"{BASE}/ran/log?limitBytes=1.5")
            assert status == 400

            status, _, body = await env.get(f"{BASE}/ran/log", method="POST", data=b"{}")
            assert status == 405 and b"Status" in body
            status, _, _ = await env.get(f"{BASE}/ran/log", method="DELETE")
            assert status == 405
            assert (await env.memory.get(*WF, "health", "ran"))["metadata"]["name"] == "ran"

            status, _, body = await env.get("/apis/argoproj.io/v1alpha1")
            import json
            by_name = {r["name"]: r for r in json.loads(body)["resources"]}
            assert by_name["workflows/log"]["verbs"] == ["get"]
            assert by_name["workflows/log"]["namespaced"] is True
        logs.close()

        # a workflow the scripted engine wrote has no logs, and says so
        logs = LogStore()
        async with Env(logs=logs, engine=ScriptedWorkflowEngine) as env:
            await env.memory.create(workflow("scripted", sh("echo never-runs")))
            await env.finished("scripted")
            with pytest.raises(NotFoundError, match="not run by the local executor"):
                await env.text("scripted")
        logs.close()

        # and so does a frontend built without a store
        async with Env(logs=None) as env:
            await env.memory.create(workflow("nolog", sh("echo hi")))
            await env.finished("nolog")
            with pytest.raises(NotFoundError, match="keeps no workflow logs"):
                await env.text("nolog")

    run(go())


def test_log_needs_a_token_when_tokens_are_set(run):
    async def go():
        logs = LogStore()
        async with Env(logs=logs, tokens={"s3cret"}) as env:
            await env.memory.create(workflow("ran", sh("echo hi")))
            await env.finished("ran")
            status, headers, _ = await env.get(f"{BASE}/ran/log")
            assert status == 401 and headers["WWW-Authenticate"] == "Bearer"
            status, _, _ = await env.get(f"{BASE}/ran/log?follow=true")
            assert status == 401
            status, _, body = await env.get(
                f"{BASE}/ran/log", headers={"Authorization": "Bearer s3cret"})
            assert status == 200 and body == b"hi\n"
            assert await env.text("ran") == b"hi\n"
        logs.close()

    run(go())


def test_deleting_the_workflow_removes_its_logs(run, tmp_path):
    async def go():
        logs = LogStore(str(tmp_path / "logs"))
        run_dir = tmp_path / "logs" / "health" / "doomed"
        async with Env(logs=logs) as env:
            await env.memory.create(workflow("doomed", sh("echo hi")))
            await env.finished("doomed")
            assert run_dir.is_dir()
            await env.client.delete(*WF, "health", "doomed")
            await _until(lambda: not run_dir.exists())
            with pytest.raises(NotFoundError):
                await env.text("doomed")
            # deleted while it runs: what it prints afterwards is not kept either
            await env.memory.create(workflow("doomed", sh("echo a; sleep 0.3; echo b")))
            await env.phase_in("doomed", ("Running",))
            await _until(lambda: run_dir.is_dir())
            await env.client.delete(*WF, "health", "doomed")
            await _until(lambda: env.engine.completed == 2)
            assert not run_dir.exists()
        assert os.listdir(tmp_path / "logs") == []

        async with Env(logs=logs, ttl=0.2) as env:  # the engine's own TTL
            await env.memory.create(workflow("doomed", sh("echo hi")))
            await env.finished("doomed")
            assert run_dir.is_dir()
            await _until(lambda: not run_dir.exists())
            with pytest.raises(NotFoundError):
                await env.memory.get(*WF, "health", "doomed")
        assert os.listdir(tmp_path / "logs") == []
        logs.close()

    run(go())


async def _until(cond, timeout=5.0):
    deadline = time.monotonic() + timeout
    while not cond():
        assert time.monotonic() < deadline, "condition not reached"
        await asyncio.sleep(0.01)


def test_logs_survive_a_restart_over_a_data_directory(run, tmp_path):
    data, log_dir = str(tmp_path), str(tmp_path / "logs")

    def live(server):
        return [(w["metadata"]["namespace"], w["metadata"]["name"])
                for w in server.list(*WF)]

    async def go():
        server = MemoryApiServer.open(data)
        logs = LogStore.open(log_dir, live=live(server))
        async with Env(server=server, logs=logs, recover=True) as env:
            await env.memory.create(workflow("done", TWO_STEPS))
            await env.finished("done")
            await env.memory.create(workflow("cut", sh("echo partial; sleep 30")))
            await env.phase_in("cut", ("Running",))
            stream = env.client.logs("health", "cut", follow=True)
            assert await asyncio.wait_for(stream.__anext__(), 5) == b"partial\n"
            await env.memory.create(workflow("removed", sh("echo bye")))
            await env.finished("removed")
        logs.close()
        server.close()

        # a Workflow deleted while no engine was there to see it go
        server = MemoryApiServer.open(data)
        server.delete(*WF, "health", "removed")
        server.close()

        server = MemoryApiServer.open(data)
        logs = LogStore.open(log_dir, live=live(server))
        assert sorted(os.listdir(tmp_path / "logs" / "health")) == ["cut", "done"]
        async with Env(server=server, logs=logs, recover=True) as env:
            assert await env.text("done") == b"one\ntwo\n"
            cut = await env.finished("cut")
            assert cut["status"]["phase"] == "Failed"
            assert cut["status"]["message"] == "workflow interrupted: engine restarted"
            assert await env.text("cut", follow=True) == b"partial\n"
            with pytest.raises(NotFoundError):
                await env.text("removed")
        logs.close()
        server.close()

    run(go())

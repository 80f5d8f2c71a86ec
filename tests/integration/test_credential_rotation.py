"""Credential rotation over an authenticated wire: ApiServerFrontend with
bearer authn, a client built from a kubeconfig whose user is a (fake) exec
credential plugin, and the server's accepted token changing underneath it."""
import asyncio
import json

import aiohttp
import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.auth import CredentialError
from active_monitor_amd.kube.config import get_config, load_kubeconfig
from active_monitor_amd.kube.errors import ApiError, UnauthorizedError
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import ScriptedWorkflowEngine, always_succeed
from tests.credplugin import exec_stanza, runs, write_kubeconfig, write_plugin

from .conftest import make_hc

HC = (API_VERSION, "HealthCheck")


def configmap(name):
    return {"apiVersion": "v1", "kind": "ConfigMap",
            "metadata": {"name": name, "namespace": "health"}, "data": {"k": "v"}}


class AuthedWire:
    """MemoryApiServer behind a frontend that accepts ``tok-1``, and an
    HttpClient that gets its credentials from the fake plugin."""

    def __init__(self, tmp_path, plugin_env=None):
        self.store = MemoryApiServer()
        self.tokens = {"tok-1"}
        self.frontend = ApiServerFrontend(self.store, accepted_tokens=self.tokens)
        self.counter = tmp_path / "counter"
        self.tmp_path = tmp_path
        self.plugin_env = plugin_env
        self.client = None

    def rotate(self, token):
        self.tokens.clear()
        self.tokens.add(token)

    async def __aenter__(self):
        await self.frontend.start()
        plugin = write_plugin(self.tmp_path)
        cfg = load_kubeconfig(write_kubeconfig(
            self.tmp_path,
            {"exec": exec_stanza(plugin, self.counter, env=self.plugin_env)},
            server=self.frontend.url,
        ))
        self.client = cfg.make_client()
        self.client._limiter.qps = 0
        await self.client.start()
        return self

    async def __aexit__(self, *exc):
        await self.client.close()
        await self.frontend.stop()


def test_requests_without_a_valid_token_get_401(run, tmp_path):
    async def go():
        async with AuthedWire(tmp_path) as w:
            url = w.frontend.url
            async with aiohttp.ClientSession() as s:
                for headers in ({}, {"Authorization": "Bearer nope"},
                                {"Authorization": "Basic tok-1"},
                                {"Authorization": "Bearer tok-1x"}):
                    for target in ("/api/v1/namespaces/health/configmaps",
                                   "/api/v1/namespaces/health/configmaps?watch=true",
                                   "/apis"):
                        async with s.get(url + target, headers=headers) as r:
                            assert r.status == 401, (headers, target)
                            body = json.loads(await r.text())
                            assert body["kind"] == "Status"
                            assert body["reason"] == "Unauthorized"
                            assert body["code"] == 401
                assert w.frontend.unauthorized_count == 12
                # health probes and /version stay open, as on a real apiserver
                for target in ("/healthz", "/livez", "/readyz", "/version"):
                    async with s.get(url + target) as r:
                        assert r.status == 200, target
                async with s.get(url + "/api/v1/namespaces/health/configmaps",
                                 headers={"Authorization": "Bearer tok-1"}) as r:
                    assert r.status == 200
                assert w.frontend.unauthorized_count == 12

            # the client without credentials, and with a fixed wrong token
            for token in (None, "wrong"):
                anon = HttpClient(url, token=token, qps=0)
                await anon.start()
                try:
                    await anon.ping()  # /version
                    with pytest.raises(UnauthorizedError) as exc:
                        await anon.list("v1", "ConfigMap", "health")
                    assert exc.value.code == 401 and isinstance(exc.value, ApiError)
                finally:
                    await anon.close()
            # a fixed token is not retried: one 401 each
            assert w.frontend.unauthorized_count == 14
            assert runs(w.counter) == 0

    run(go())


def test_frontend_without_accepted_tokens_stays_open(run):
    async def go():
        fe = ApiServerFrontend(MemoryApiServer())
        await fe.start()
        client = HttpClient(fe.url, qps=0)
        await client.start()
        try:
            assert await client.list("v1", "ConfigMap", "health") == []
            assert fe.unauthorized_count == 0
        finally:
            await client.close()
            await fe.stop()

    run(go())


@pytest.mark.parametrize("path", ["pool", "aiohttp"])
def test_create_survives_a_rotated_token(run, tmp_path, path):
    async def go():
        async with AuthedWire(tmp_path) as w:
            if path == "aiohttp":
                w.client._pool = None  # the unary path https targets take
            assert await w.client.list("v1", "ConfigMap", "health") == []
            assert runs(w.counter) == 1
            assert w.frontend.unauthorized_count == 0

            w.rotate("tok-2")
            made = await w.client.create(configmap("after-rotation"))
            assert made["metadata"]["name"] == "after-rotation"
            assert runs(w.counter) == 2
            assert w.frontend.unauthorized_count == 1
            assert len(w.store.list("v1", "ConfigMap", "health")) == 1

            # the refreshed credential is reused: no further 401, no further run
            await w.client.get("v1", "ConfigMap", "health", "after-rotation")
            assert runs(w.counter) == 2 and w.frontend.unauthorized_count == 1

    run(go())


def test_eight_concurrent_requests_share_one_refresh(run, tmp_path):
    async def go():
        async with AuthedWire(tmp_path) as w:
            await w.client.create(configmap("shared"))
            w.rotate("tok-2")
            await w.client.get("v1", "ConfigMap", "health", "shared")
            assert runs(w.counter) == 2

            w.rotate("tok-3")
            got = await asyncio.gather(*(
                w.client.get("v1", "ConfigMap", "health", "shared") for _ in range(8)
            ))
            assert [g["metadata"]["name"] for g in got] == ["shared"] * 8
            assert runs(w.counter) == 3

    run(go())


def test_patch_survives_a_rotated_token(run, tmp_path):
    async def go():
        async with AuthedWire(tmp_path) as w:
            await w.client.create(configmap("patched"))
            w.rotate("tok-2")
            out = await w.client.patch("v1", "ConfigMap", "health", "patched",
                                       {"data": {"k": "v2"}})
            assert out["data"]["k"] == "v2"
            assert runs(w.counter) == 2 and w.frontend.unauthorized_count == 1

    run(go())


def test_open_watch_survives_rotation_and_kick(run, tmp_path, caplog):
    async def go():
        async with AuthedWire(tmp_path) as w:
            sub = w.client.watch("v1", "ConfigMap", "health")
            try:
                await w.client.create(configmap("before"))
                ev = await asyncio.wait_for(sub.__anext__(), 5)
                assert ev["object"]["metadata"]["name"] == "before"
                assert runs(w.counter) == 1

                w.rotate("tok-2")
                w.frontend.kick_watches()
                w.store.create(configmap("after"))
                ev = await asyncio.wait_for(sub.__anext__(), 5)
                assert (ev["type"], ev["object"]["metadata"]["name"]) == ("ADDED", "after")
                assert runs(w.counter) == 2
                assert w.frontend.unauthorized_count == 1
            finally:
                sub.close()

    with caplog.at_level("INFO", logger="active_monitor_amd.kube.http"):
        run(go())
    # reconnected at once with a fresh credential, not through the
    # warn-and-sleep reconnect loop
    assert not [r for r in caplog.records
                if r.name == "active_monitor_amd.kube.http" and r.levelname == "WARNING"]


def test_always_rejected_token_raises_after_exactly_two_401s(run, tmp_path):
    async def go():
        async with AuthedWire(tmp_path, plugin_env={"FAKE_TOKEN": "revoked"}) as w:
            with pytest.raises(UnauthorizedError):
                await w.client.create(configmap("never"))
            assert w.frontend.unauthorized_count == 2
            assert runs(w.counter) == 2
            assert w.store.list("v1", "ConfigMap", "health") == []

    run(go())


def test_credential_error_reaches_the_caller(run, tmp_path):
    async def go():
        env = {"FAKE_FAIL": "1", "FAKE_STDERR": "sso session expired"}
        async with AuthedWire(tmp_path, plugin_env=env) as w:
            with pytest.raises(CredentialError, match="sso session expired"):
                await w.client.list("v1", "ConfigMap", "health")
            assert w.frontend.unauthorized_count == 0

    run(go())


def test_token_file_client_survives_rotation(run, tmp_path):
    async def go():
        token_file = tmp_path / "sa-token"
        token_file.write_text("tok-1\n")
        tokens = {"tok-1"}
        store = MemoryApiServer()
        fe = ApiServerFrontend(store, accepted_tokens=tokens)
        await fe.start()
        client = get_config(server=fe.url, token_file=str(token_file)).make_client()
        client._limiter.qps = 0
        await client.start()
        try:
            await client.create(configmap("first"))
            assert fe.unauthorized_count == 0

            token_file.write_text("tok-2\n")  # the kubelet rewrites the projection
            tokens.clear()
            tokens.add("tok-2")
            await client.create(configmap("second"))
            assert fe.unauthorized_count == 1
            assert len(store.list("v1", "ConfigMap", "health")) == 2
        finally:
            await client.close()
            await fe.stop()

    run(go())


def test_standalone_token_file_flag(tmp_path):
    from active_monitor_amd.kube import standalone

    assert standalone.parse_args([]).token_file is None  # open unless asked
    tokens = tmp_path / "tokens"
    tokens.write_text("alpha\n\n  beta  \n")
    args = standalone.parse_args(["--token-file", str(tokens)])
    assert standalone.read_accepted_tokens(args.token_file) == {"alpha", "beta"}
    tokens.write_text("\n")
    with pytest.raises(SystemExit):
        standalone.read_accepted_tokens(str(tokens))


def test_manager_full_loop_over_rotating_credentials(run, tmp_path):
    async def go():
        async with AuthedWire(tmp_path) as w:
            # the engine plays the in-cluster Argo controller, server side
            engine = ScriptedWorkflowEngine(MemoryClient(w.store), policy=always_succeed)
            await engine.start()
            manager = Manager(w.client, max_workers=2)
            await manager.start()
            rec = manager.reconciler
            try:
                async def runs_reach(n):
                    deadline = asyncio.get_running_loop().time() + 20
                    while rec.completed_runs < n:
                        assert asyncio.get_running_loop().time() < deadline, (
                            f"stuck at {rec.completed_runs} runs (wanted {n})")
                        await asyncio.sleep(0.02)

                await w.client.create(make_hc(name="authed", repeat=3600, timeout=5))
                await runs_reach(1)
                assert runs(w.counter) == 1 and w.frontend.unauthorized_count == 0

                w.rotate("tok-2")
                w.frontend.kick_watches()  # watches re-authenticate as well
                manager.queue.add_nowait(("health", "authed"), {"timer"})
                await runs_reach(2)

                assert runs(w.counter) == 2
                assert w.frontend.unauthorized_count >= 1
                hc = w.store.get(*HC, "health", "authed")
                assert hc["status"]["successCount"] == 2
                assert not manager.fatal.is_set()
            finally:
                await manager.stop()
                await engine.stop()

    run(go())

"""kubeconfig ``exec`` credential plugins (client-go ExecCredential contract)
against a fake plugin: caching, expiry, single-flight refresh, the request
document, command resolution, and every failure mode."""
import asyncio
import json
import os
import time

import pytest

from active_monitor_amd.kube.auth import (
    Credential,
    CredentialError,
    ExecPluginSource,
    parse_rfc3339,
)
from active_monitor_amd.kube.config import ConfigError, load_kubeconfig
from tests.credplugin import Clock, exec_stanza, runs, write_kubeconfig, write_plugin

V1 = "client.authentication.k8s.io/v1"
V1BETA1 = "client.authentication.k8s.io/v1beta1"
CLUSTER = {"server": "https://api.example:6443",
           "certificate-authority-data": "Q0EgUEVN"}


@pytest.fixture
def plugin(tmp_path):
    return write_plugin(tmp_path)


@pytest.fixture
def counter(tmp_path):
    return tmp_path / "counter"


def make_source(plugin, counter, tmp_path, now=time.time, timeout=10.0,
                cluster=CLUSTER, **stanza):
    return ExecPluginSource(exec_stanza(plugin, counter, **stanza), cluster=cluster,
                            kubeconfig_dir=str(tmp_path), timeout=timeout, now=now)


def test_kubeconfig_exec_user_yields_exec_source(run, tmp_path, plugin, counter):
    cfg = load_kubeconfig(write_kubeconfig(tmp_path, {"exec": exec_stanza(plugin, counter)}))
    assert isinstance(cfg.credential_source, ExecPluginSource)
    assert cfg.token is None
    assert runs(counter) == 0, "the plugin must not run at load time"
    client = cfg.make_client()
    assert client._credentials is cfg.credential_source
    assert run(cfg.credential_source.get()).token == "tok-1"


def test_first_get_runs_plugin_second_is_cached(run, tmp_path, plugin, counter):
    src = make_source(plugin, counter, tmp_path)

    async def go():
        return await src.get(), await src.get()

    first, second = run(go())
    assert first == Credential("tok-1", None)
    assert second is first
    assert runs(counter) == 1


@pytest.mark.parametrize("stamp,epoch", [
    ("2023-11-14T22:13:20Z", 1_700_000_000.0),
    ("2023-11-14T22:13:20+00:00", 1_700_000_000.0),
    ("2023-11-14T23:13:20.5+01:00", 1_700_000_000.5),
])
def test_expiration_timestamp_forms(run, tmp_path, plugin, counter, stamp, epoch):
    assert parse_rfc3339(stamp) == epoch
    src = make_source(plugin, counter, tmp_path, now=Clock(epoch - 100),
                      env={"FAKE_EXPIRY": stamp})
    assert run(src.get()).expiry == epoch


def test_expiry_on_injected_clock(run, tmp_path, plugin, counter):
    clock = Clock(1_700_000_000.0 - 600)
    src = make_source(plugin, counter, tmp_path, now=clock,
                      env={"FAKE_EXPIRY": "2023-11-14T22:13:20Z"})

    async def go():
        a = await src.get()
        clock.advance(599)  # one second short of the expiry
        b = await src.get()
        assert b is a and runs(counter) == 1
        clock.advance(1)  # now == expiry: client-go's rule is now >= expiry
        c = await src.get()
        assert runs(counter) == 2
        return a, c

    a, c = run(go())
    assert (a.token, c.token) == ("tok-1", "tok-2")


def test_sixteen_concurrent_gets_run_the_plugin_once(run, tmp_path, plugin, counter):
    src = make_source(plugin, counter, tmp_path, env={"FAKE_SLEEP": "0.05"})

    async def go():
        return await asyncio.gather(*(src.get() for _ in range(16)))

    creds = run(go())
    assert runs(counter) == 1
    assert all(c is creds[0] for c in creds)


def test_invalidate_with_stale_credential_is_a_no_op(run, tmp_path, plugin, counter):
    src = make_source(plugin, counter, tmp_path)

    async def go():
        old = await src.get()
        src.invalidate(old)
        new = await src.get()
        assert (old.token, new.token) == ("tok-1", "tok-2")
        # a second caller that was refused with the *old* credential arrives late
        src.invalidate(old)
        again = await src.get()
        assert again is new
        # equal by value but not the cached object: still not the one in use
        src.invalidate(Credential("tok-2", None))
        assert await src.get() is new

    run(go())
    assert runs(counter) == 2


def test_args_env_and_exec_info_arrive(run, tmp_path, plugin, counter, monkeypatch):
    dump = tmp_path / "dump.json"
    monkeypatch.setenv("FROM_PROCESS_ENV", "inherited")
    monkeypatch.setenv("OVERRIDDEN", "process")
    src = make_source(plugin, counter, tmp_path, api_version=V1BETA1,
                      interactive_mode=None,
                      args=["get-token", "--cluster", "c1"],
                      env={"FAKE_DUMP": dump, "OVERRIDDEN": "stanza"})
    run(src.get())
    seen = json.loads(dump.read_text())
    assert seen["argv"] == ["get-token", "--cluster", "c1"]
    assert seen["env"]["FROM_PROCESS_ENV"] == "inherited"
    assert seen["env"]["OVERRIDDEN"] == "stanza"
    assert seen["stdin"] == "", "stdin must be /dev/null"
    info = seen["exec_info"]
    assert info["apiVersion"] == V1BETA1
    assert info["kind"] == "ExecCredential"
    assert info["spec"]["interactive"] is False
    assert "cluster" not in info["spec"]


def test_provide_cluster_info(run, tmp_path, plugin, counter):
    dump = tmp_path / "dump.json"
    cluster = dict(CLUSTER)
    cluster.update({
        "insecure-skip-tls-verify": True,
        "tls-server-name": "api.internal",
        "extensions": [
            {"name": "something-else", "extension": {"x": 1}},
            {"name": "client.authentication.k8s.io/exec",
             "extension": {"audience": "sts", "region": "eu-1"}},
        ],
    })
    src = make_source(plugin, counter, tmp_path, cluster=cluster,
                      env={"FAKE_DUMP": dump}, provideClusterInfo=True)
    run(src.get())
    spec = json.loads(dump.read_text())["exec_info"]["spec"]
    assert spec["interactive"] is False
    assert spec["cluster"] == {
        "server": "https://api.example:6443",
        "certificate-authority-data": "Q0EgUEVN",
        "insecure-skip-tls-verify": True,
        "tls-server-name": "api.internal",
        "config": {"audience": "sts", "region": "eu-1"},
    }


def test_relative_command_resolves_against_kubeconfig_dir(run, tmp_path, counter,
                                                          monkeypatch):
    cfg_dir = tmp_path / "kube"
    write_plugin(cfg_dir, "bin/fake-plugin")
    elsewhere = tmp_path / "elsewhere"
    elsewhere.mkdir()
    monkeypatch.chdir(elsewhere)
    cfg = load_kubeconfig(write_kubeconfig(
        cfg_dir, {"exec": exec_stanza("./bin/fake-plugin", counter)}))
    assert run(cfg.credential_source.get()).token == "tok-1"


def test_bare_command_is_looked_up_on_path(run, tmp_path, counter, monkeypatch):
    bindir = tmp_path / "pathdir"
    write_plugin(bindir, "fake-plugin-on-path")
    monkeypatch.setenv("PATH", f"{bindir}{os.pathsep}{os.environ.get('PATH', '')}")
    src = make_source("fake-plugin-on-path", counter, tmp_path)
    assert run(src.get()).token == "tok-1"


# -- failures ---------------------------------------------------------------


def failing(run, src):
    with pytest.raises(CredentialError) as exc:
        run(src.get())
    assert isinstance(exc.value, ConfigError)
    return str(exc.value)


def test_nonzero_exit_carries_stderr(run, tmp_path, plugin, counter):
    src = make_source(plugin, counter, tmp_path,
                      env={"FAKE_FAIL": "3", "FAKE_STDERR": "token endpoint said no"})
    msg = failing(run, src)
    assert plugin in msg and "status 3" in msg and "token endpoint said no" in msg


def test_command_not_found_carries_install_hint(run, tmp_path, counter):
    hint = "install it with: brew install no-such-credential-helper"
    src = make_source("no-such-credential-helper", counter, tmp_path, installHint=hint)
    msg = failing(run, src)
    assert "no-such-credential-helper" in msg and "not found" in msg and hint in msg
    src = make_source("./missing/helper", counter, tmp_path, installHint=hint)
    msg = failing(run, src)
    assert "./missing/helper" in msg and "not found" in msg and hint in msg


@pytest.mark.parametrize("mode,expect", [
    ("notjson", "not JSON"),
    ("wrongkind", "TokenReview"),
    ("wrongversion", "v1alpha1"),
    ("empty", "neither a token nor certificate data"),
    ("certonly", "certificate-issuing exec plugins are not supported"),
])
def test_bad_plugin_output(run, tmp_path, plugin, counter, mode, expect):
    src = make_source(plugin, counter, tmp_path, env={"FAKE_OUTPUT": mode})
    msg = failing(run, src)
    assert plugin in msg and expect in msg
    assert runs(counter) == 1


def test_failure_is_not_cached(run, tmp_path, plugin, counter):
    src = make_source(plugin, counter, tmp_path, env={"FAKE_OUTPUT": "empty"})
    failing(run, src)
    failing(run, src)
    assert runs(counter) == 2


def test_timeout_kills_and_reaps_the_child(run, tmp_path, plugin, counter):
    pidfile = tmp_path / "pid"
    src = make_source(plugin, counter, tmp_path, timeout=0.5,
                      env={"FAKE_SLEEP": "30", "FAKE_PIDFILE": pidfile})
    t0 = time.monotonic()
    msg = failing(run, src)
    took = time.monotonic() - t0
    assert plugin in msg and "timed out" in msg
    assert took < 5.0, f"timeout took {took:.1f}s"
    pid = int(pidfile.read_text())
    # killed *and* reaped: signalling a zombie would still succeed
    with pytest.raises(ProcessLookupError):
        os.kill(pid, 0)


def test_default_timeout_is_the_projects_external_wait_bound(tmp_path, plugin, counter):
    from active_monitor_amd.engine.parse import ARTIFACT_READ_TIMEOUT

    src = ExecPluginSource(exec_stanza(plugin, counter), cluster=CLUSTER,
                           kubeconfig_dir=str(tmp_path))
    assert src.timeout == ARTIFACT_READ_TIMEOUT


# -- load-time validation ---------------------------------------------------


@pytest.mark.parametrize("stanza_kwargs,expect", [
    ({"api_version": V1, "interactive_mode": None}, "interactiveMode must be set"),
    ({"api_version": V1, "interactive_mode": "Always"}, "Always"),
    ({"api_version": V1BETA1, "interactive_mode": "Always"}, "Always"),
    ({"api_version": "client.authentication.k8s.io/v1alpha1"}, "v1alpha1"),
])
def test_rejected_at_load_time(tmp_path, plugin, counter, stanza_kwargs, expect):
    path = write_kubeconfig(tmp_path, {"exec": exec_stanza(plugin, counter, **stanza_kwargs)})
    with pytest.raises(ConfigError, match=expect):
        load_kubeconfig(path)
    assert runs(counter) == 0


@pytest.mark.parametrize("api_version,mode", [
    (V1, "Never"), (V1, "IfAvailable"), (V1BETA1, None), (V1BETA1, "IfAvailable"),
])
def test_accepted_at_load_time(tmp_path, plugin, counter, api_version, mode):
    path = write_kubeconfig(tmp_path, {"exec": exec_stanza(
        plugin, counter, api_version=api_version, interactive_mode=mode)})
    assert isinstance(load_kubeconfig(path).credential_source, ExecPluginSource)


def test_literal_token_wins_over_exec(tmp_path, plugin, counter):
    cfg = load_kubeconfig(write_kubeconfig(
        tmp_path, {"token": "literal", "exec": exec_stanza(plugin, counter)}))
    assert cfg.token == "literal" and cfg.credential_source is None


def test_auth_provider_warns_and_names_the_user(tmp_path, caplog):
    path = write_kubeconfig(tmp_path, {"auth-provider": {"name": "gcp", "config": {}}})
    with caplog.at_level("WARNING", logger="active_monitor_amd.kube.config"):
        cfg = load_kubeconfig(path)
    assert cfg.token is None and cfg.credential_source is None
    text = caplog.text
    assert "'u1'" in text and "auth-provider" in text and "exec" in text

"""Rotating token files: the projected service-account token in-cluster and
kubeconfig ``tokenFile`` / ``--token-file``."""
import asyncio
import os

import pytest

from active_monitor_amd.kube import config as config_mod
from active_monitor_amd.kube.auth import (
    TOKEN_FILE_PERIOD,
    CredentialError,
    StaticToken,
    TokenFileSource,
)
from active_monitor_amd.kube.config import get_config, in_cluster_config, load_kubeconfig
from tests.credplugin import Clock, write_kubeconfig


def test_reread_after_the_period_and_not_before(run, tmp_path):
    path = tmp_path / "token"
    path.write_text("one\n")
    clock = Clock()
    src = TokenFileSource(str(path), now=clock)
    assert src.period == TOKEN_FILE_PERIOD == 60.0

    async def go():
        first = await src.get()
        assert first.token == "one"
        path.write_text("two\n")
        clock.advance(59.9)
        assert await src.get() is first  # not yet a minute old
        clock.advance(0.1)
        second = await src.get()
        assert second.token == "two"
        clock.advance(59.9)
        assert await src.get() is second

    run(go())


def test_period_is_a_constructor_argument(run, tmp_path):
    path = tmp_path / "token"
    path.write_text("one")
    clock = Clock()
    src = TokenFileSource(str(path), period=5.0, now=clock)

    async def go():
        assert (await src.get()).token == "one"
        path.write_text("two")
        clock.advance(4.0)
        assert (await src.get()).token == "one"
        clock.advance(1.0)
        assert (await src.get()).token == "two"

    run(go())


def test_initial_value_is_used_until_a_read_is_due(run, tmp_path):
    path = tmp_path / "token"
    path.write_text("from-file")
    clock = Clock()
    src = TokenFileSource(str(path), initial="seed", now=clock)

    async def go():
        assert (await src.get()).token == "seed"
        clock.advance(60)
        assert (await src.get()).token == "from-file"

    run(go())


def test_unchanged_file_keeps_the_same_credential_object(run, tmp_path):
    path = tmp_path / "token"
    path.write_text("same")
    clock = Clock()
    src = TokenFileSource(str(path), now=clock)

    async def go():
        first = await src.get()
        clock.advance(60)
        assert await src.get() is first

    run(go())


def test_unreadable_or_empty_file_keeps_the_old_token(run, tmp_path, caplog):
    path = tmp_path / "token"
    path.write_text("good")
    clock = Clock()
    src = TokenFileSource(str(path), now=clock)

    async def go():
        assert (await src.get()).token == "good"
        path.write_text("  \n")  # mid-rewrite: empty
        clock.advance(60)
        assert (await src.get()).token == "good"
        os.unlink(path)  # gone altogether
        clock.advance(60)
        assert (await src.get()).token == "good"
        path.write_text("better")
        clock.advance(60)
        assert (await src.get()).token == "better"

    with caplog.at_level("WARNING", logger="active_monitor_amd.kube.auth"):
        run(go())
    warnings = [r for r in caplog.records if "keeping the previous token" in r.getMessage()]
    assert len(warnings) == 2
    assert str(path) in warnings[0].getMessage()


def test_raises_only_when_there_has_never_been_a_token(run, tmp_path):
    path = tmp_path / "absent"
    src = TokenFileSource(str(path))
    with pytest.raises(CredentialError, match="absent"):
        run(src.get())
    path.write_text("")
    with pytest.raises(CredentialError, match="empty"):
        run(src.get())
    path.write_text("late")
    assert run(src.get()).token == "late"


def test_invalidate_forces_the_reread_whatever_the_age(run, tmp_path):
    path = tmp_path / "token"
    path.write_text("one")
    clock = Clock()
    src = TokenFileSource(str(path), now=clock)

    async def go():
        first = await src.get()
        path.write_text("two")
        assert await src.get() is first  # clock has not moved
        src.invalidate(first)
        second = await src.get()
        assert second.token == "two"
        # a late invalidate() from a request that used the old token
        path.write_text("three")
        src.invalidate(first)
        assert await src.get() is second

    run(go())


def test_concurrent_gets_share_one_read(run, tmp_path, monkeypatch):
    path = tmp_path / "token"
    path.write_text("one")
    src = TokenFileSource(str(path))
    reads = []
    real = TokenFileSource._refresh

    async def counting(self):
        reads.append(1)
        await asyncio.sleep(0.01)
        return await real(self)

    monkeypatch.setattr(TokenFileSource, "_refresh", counting)

    async def go():
        return await asyncio.gather(*(src.get() for _ in range(16)))

    creds = run(go())
    assert len(reads) == 1 and all(c is creds[0] for c in creds)


def test_static_token(run):
    src = StaticToken("fixed")

    async def go():
        cred = await src.get()
        assert cred.token == "fixed" and cred.expiry is None
        src.invalidate(cred)
        assert (await src.get()).token == "fixed"

    run(go())


def test_in_cluster_config_wires_the_file_source(run, tmp_path, monkeypatch):
    (tmp_path / "token").write_text("sa-token-1\n")
    (tmp_path / "ca.crt").write_text("CA")
    monkeypatch.setattr(config_mod, "SA_DIR", tmp_path)
    monkeypatch.setenv("KUBERNETES_SERVICE_HOST", "10.0.0.1")
    monkeypatch.setenv("KUBERNETES_SERVICE_PORT", "6443")

    cfg = in_cluster_config()
    assert cfg.server == "https://10.0.0.1:6443"
    assert cfg.token == "sa-token-1"  # as before
    assert cfg.token_file == str(tmp_path / "token")
    src = cfg.credential_source
    assert isinstance(src, TokenFileSource) and src.path == cfg.token_file
    assert get_config().credential_source.path == cfg.token_file
    assert cfg.make_client()._credentials is src

    async def go():
        first = await src.get()
        assert first.token == "sa-token-1"
        (tmp_path / "token").write_text("sa-token-2\n")  # the kubelet rotates it
        src.invalidate(first)
        assert (await src.get()).token == "sa-token-2"

    run(go())


def test_kubeconfig_token_file_takes_precedence(run, tmp_path, monkeypatch):
    (tmp_path / "tok").write_text("from-file\n")
    # relative tokenFile resolves against the kubeconfig's directory; a
    # literal token and an exec stanza next to it both lose
    path = write_kubeconfig(tmp_path, {
        "tokenFile": "tok",
        "token": "literal",
        "exec": {"apiVersion": "client.authentication.k8s.io/v1beta1",
                 "command": "never-run"},
    })
    cfg = load_kubeconfig(path)
    assert isinstance(cfg.credential_source, TokenFileSource)
    assert cfg.token_file == str(tmp_path / "tok")
    assert run(cfg.credential_source.get()).token == "from-file"


def test_kubeconfig_literal_token_bridges_an_unreadable_token_file(run, tmp_path):
    path = write_kubeconfig(tmp_path, {"tokenFile": str(tmp_path / "later"),
                                       "token": "literal"})
    src = load_kubeconfig(path).credential_source

    async def go():
        first = await src.get()
        assert first.token == "literal"
        (tmp_path / "later").write_text("from-file")
        src.invalidate(first)
        assert (await src.get()).token == "from-file"

    run(go())


def test_get_config_token_file(run, tmp_path, monkeypatch):
    monkeypatch.delenv("KUBERNETES_SERVICE_HOST", raising=False)
    (tmp_path / "tok").write_text("flag-token")
    cfg = get_config(server="http://127.0.0.1:8001", token_file=str(tmp_path / "tok"))
    assert cfg.token_file == str(tmp_path / "tok")
    assert run(cfg.credential_source.get()).token == "flag-token"
    # a plain token stays the plain, source-less config it always was
    plain = get_config(server="http://127.0.0.1:8001", token="t")
    assert plain.credential_source is None and plain.token_file is None
    assert plain.make_client()._credentials is None


def test_token_file_flags():
    from active_monitor_amd.cmd.ctl import build_parser as ctl_parser
    from active_monitor_amd.cmd.main import build_parser as main_parser

    args = main_parser().parse_args(["--backend", "http", "--server", "http://x",
                                     "--token-file", "/run/tok"])
    assert args.token_file == "/run/tok"
    assert main_parser().parse_args([]).token_file is None
    args = ctl_parser().parse_args(["--server", "http://x", "--token-file", "/run/tok",
                                    "get", "hc"])
    assert args.token_file == "/run/tok"

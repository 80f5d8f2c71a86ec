"""Schema validation on the command lines: the standalone apiserver validates
by default and can be told not to, ``amctl apply`` reports what the server
refused, and the offline linter applies the same schema."""
import asyncio
import contextlib
import json
import os
import subprocess
import sys

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.cmd.ctl import build_parser
from active_monitor_amd.cmd.ctl import run as ctl_run
from active_monitor_amd.kube import InvalidError, MemoryApiServer
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.memory import healthcheck_schemas
from active_monitor_amd.kube.server import ApiServerFrontend

from .conftest import make_hc

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STANDALONE = [sys.executable, "-m", "active_monitor_amd.kube.standalone"]
LINT = [sys.executable, "-m", "active_monitor_amd.workflow", "lint"]
HC = (API_VERSION, "HealthCheck")


def invalid_hc(name="bad"):
    hc = make_hc(name=name)
    hc["spec"]["repeatAfterSec"] = "sixty"
    return hc


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k != "AM_SCHEMA_VALIDATION"}
    env.update(extra)
    return env


async def post_invalid_to_standalone(argv, env):
    """Start the standalone apiserver, POST one invalid HealthCheck, stop it.
    Returns (the error or None, what the server logged)."""
    proc = await asyncio.create_subprocess_exec(
        *STANDALONE, "--engine", "none", *argv,
        stdout=asyncio.subprocess.PIPE, stderr=asyncio.subprocess.PIPE,
        cwd=REPO, env=env,
    )
    try:
        line = await asyncio.wait_for(proc.stdout.readline(), 60)
        assert line.startswith(b"READY "), (line, await proc.stderr.read())
        client = HttpClient(json.loads(line[len(b"READY "):])["url"], qps=0)
        await client.start()
        error = None
        try:
            await asyncio.wait_for(client.create(invalid_hc()), 10)
        except InvalidError as e:
            error = e
        finally:
            await client.close()
    finally:
        proc.terminate()
        _, err = await asyncio.wait_for(proc.communicate(), 20)
    assert proc.returncode == 0, err
    return error, err.decode()


def test_standalone_validates_by_default(run):
    error, log = run(post_invalid_to_standalone([], _env()), timeout=120)
    assert error is not None and "spec.repeatAfterSec" in error.message
    assert error.causes[0]["reason"] == "FieldValueTypeInvalid"
    assert ("schema validation: HealthCheck "
            "(activemonitor.keikoproj.io/v1alpha1)") in log


@pytest.mark.parametrize("argv,extra", [
    (["--no-schema-validation"], {}),
    ([], {"AM_SCHEMA_VALIDATION": "0"}),
], ids=["flag", "environment"])
def test_standalone_validation_can_be_turned_off(run, argv, extra):
    error, log = run(post_invalid_to_standalone(argv, _env(**extra)), timeout=120)
    assert error is None
    assert "schema validation: off" in log


def test_controller_rejects_no_schema_validation_with_http_backend():
    out = subprocess.run(
        [sys.executable, "-m", "active_monitor_amd.cmd.main", "--backend", "http",
         "--server", "http://127.0.0.1:1", "--no-schema-validation"],
        capture_output=True, text=True, timeout=60, cwd=REPO, env=_env(),
    )
    assert out.returncode == 2, out.stderr  # argparse's argument-error status
    assert "--no-schema-validation" in out.stderr and "usage:" in out.stderr


def test_controller_memory_backend_validates_unless_told_not_to(run, monkeypatch):
    """``--backend memory`` installs the schema, with or without --serve-api."""
    from active_monitor_amd.cmd import main as cmd_main
    from active_monitor_amd.kube import MemoryApiServer as Store

    monkeypatch.delenv("AM_SCHEMA_VALIDATION", raising=False)
    made = []

    class Recording(Store):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr("active_monitor_amd.kube.MemoryApiServer", Recording)

    async def start_and_stop(*argv):
        args = cmd_main.build_parser().parse_args([
            "--metrics-bind-address", "0", "--health-probe-bind-address", "0",
            "--workflow-engine", "none", "--gc-threshold", "0", *argv])
        stop = asyncio.Event()
        stop.set()
        assert await cmd_main.run(args, stop) == 0
        return made.pop()

    store = run(start_and_stop())
    with pytest.raises(InvalidError):
        store.create(invalid_hc())
    store = run(start_and_stop("--no-schema-validation"))
    store.create(invalid_hc())
    monkeypatch.setenv("AM_SCHEMA_VALIDATION", "0")
    store = run(start_and_stop())
    store.create(invalid_hc())


@contextlib.asynccontextmanager
async def validating_frontend():
    server = MemoryApiServer(schemas=healthcheck_schemas())
    frontend = ApiServerFrontend(server)
    await frontend.start()
    try:
        yield server, frontend.url
    finally:
        await frontend.stop()


def test_amctl_apply_reports_the_refused_document_and_goes_on(run, capsys, tmp_path):
    f = tmp_path / "two.yaml"
    f.write_text(yaml.safe_dump_all([invalid_hc("first"), make_hc(name="second")]))

    async def go():
        async with validating_frontend() as (server, url):
            rc = await ctl_run(build_parser().parse_args(
                ["--server", url, "apply", "-f", str(f)]))
            captured = capsys.readouterr()
            assert rc == 1
            assert captured.err.startswith(
                'error: HealthCheck.activemonitor.keikoproj.io "first" is invalid: '
                "spec.repeatAfterSec: Invalid value")
            assert "Traceback" not in captured.err
            assert captured.out == "healthcheck/second created\n"
            assert [o["metadata"]["name"] for o in server.list(*HC)] == ["second"]

    run(go())


def test_amctl_apply_validate_modes(run, capsys, tmp_path):
    doc = make_hc(name="typo", repeat=0)
    doc["spec"]["repeatAfterSecs"] = 60
    f = tmp_path / "typo.yaml"
    f.write_text(yaml.safe_dump(doc))

    async def go():
        async with validating_frontend() as (server, url):
            async def apply(*argv):
                rc = await ctl_run(build_parser().parse_args(
                    ["--server", url, "apply", "-f", str(f), *argv]))
                return rc, capsys.readouterr()

            # strict is the default, as it is kubectl's
            rc, said = await apply()
            assert rc == 1 and said.out == ""
            assert said.err == (
                'error: HealthCheck in version "v1alpha1" cannot be handled as a '
                'HealthCheck: strict decoding error: unknown field '
                '"spec.repeatAfterSecs"\n')
            assert server.list(*HC) == []

            rc, said = await apply("--validate", "warn")
            assert rc == 0 and said.out == "healthcheck/typo created\n"
            assert said.err == 'Warning: unknown field "spec.repeatAfterSecs"\n'
            assert "repeatAfterSecs" not in server.get(*HC, "health", "typo")["spec"]

            server.delete(*HC, "health", "typo")
            rc, said = await apply("--validate", "ignore")
            assert rc == 0 and said.out == "healthcheck/typo created\n"
            assert said.err == ""

    run(go())


def test_lint_applies_the_schema_before_anything_else(tmp_path):
    bad = invalid_hc()
    bad["spec"]["repeatAfterSecs"] = 60  # reported only once the errors are gone
    f = tmp_path / "bad.yaml"
    f.write_text(yaml.safe_dump(bad))
    out = subprocess.run(LINT + [str(f)], capture_output=True, text=True,
                         timeout=60, cwd=REPO)
    assert out.returncode == 1, out.stderr
    assert out.stdout == (
        f'{f}: invalid HealthCheck: spec.repeatAfterSec: Invalid value: "string": '
        'spec.repeatAfterSec in body must be of type integer: "string"\n')

    del bad["spec"]["repeatAfterSec"]
    f.write_text(yaml.safe_dump(bad))
    out = subprocess.run(LINT + [str(f)], capture_output=True, text=True,
                         timeout=60, cwd=REPO)
    assert out.returncode == 1, out.stderr
    assert out.stdout == (
        f'{f}: invalid HealthCheck: unknown field "spec.repeatAfterSecs"\n')


def test_lint_output_for_a_valid_example_is_unchanged():
    out = subprocess.run(LINT + ["examples/inline-hello.yaml"], capture_output=True,
                         text=True, timeout=60, cwd=REPO)
    assert out.returncode == 0, out.stderr
    assert out.stdout == "ok\n"

"""An ``http`` check through the whole controller loop (Manager + local
engine + log store + wire), and through the offline ``lint`` / ``run``
commands with the shipped example."""
import asyncio
import os
import pathlib
import sys

import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.api import RUN_REQUESTED_ANNOTATION, HealthCheck
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import LocalWorkflowEngine
from active_monitor_amd.workflow.logs import LogStore
from tests.probeserver import ProbeServer, Route

from .conftest import make_hc

REPO = pathlib.Path(__file__).parents[2]
WF = ("argoproj.io/v1alpha1", "Workflow")
SECRET = "Bearer s3cret-token"


def workflow_yaml(templates, entrypoint):
    return yaml.safe_dump({"apiVersion": WF[0], "kind": WF[1],
                           "spec": {"entrypoint": entrypoint, "templates": templates}})


def test_an_http_check_counts_fails_and_is_remedied(run, tmp_path):
    marker = tmp_path / "remedied"

    async def go():
        routes = {"/healthz": [Route(body=b'{"status":"ok"}'),
                               Route(503, "Service Unavailable", body=b"draining\n")]}
        async with ProbeServer(routes) as srv:
            server = MemoryApiServer()
            client = MemoryClient(server)
            logs = LogStore()
            engine = LocalWorkflowEngine(client, ttl_seconds=None, logs=logs)
            frontend = ApiServerFrontend(server, logs=logs)
            manager = Manager(client, max_workers=2)
            await frontend.start()
            await engine.start()
            await manager.start()
            http = HttpClient(frontend.url, qps=0)
            await http.start()

            async def status_when(pred):
                for _ in range(1000):
                    obj = await client.get(API_VERSION, "HealthCheck", "health", "web")
                    hc = HealthCheck.from_dict(obj)
                    if pred(hc.status):
                        return hc.status
                    await asyncio.sleep(0.01)
                raise AssertionError(f"never reached: {obj.get('status')}")

            try:
                await client.create(make_hc(
                    name="web", repeat=3600, timeout=10, remedy=True,
                    inline=workflow_yaml([{"name": "probe", "http": {
                        "url": srv.url + "/healthz",
                        "headers": [{"name": "Authorization", "value": SECRET}],
                        "successCondition":
                            'response.statusCode == 200 && '
                            'jsonpath(response.body, "$.status") == "ok"',
                    }}], "probe"),
                    remedy_inline=workflow_yaml([{"name": "fix", "container": {
                        "command": ["sh", "-c", f"echo fixed > {marker}"]}}], "fix")))
                first = await status_when(lambda s: s.total_healthcheck_runs >= 1)
                assert first.success_count == 1 and first.failed_count == 0
                assert not marker.exists()

                await client.patch(API_VERSION, "HealthCheck", "health", "web", {
                    "metadata": {"annotations": {RUN_REQUESTED_ANNOTATION: "again"}}})
                second = await status_when(
                    lambda s: s.total_healthcheck_runs >= 2 and s.remedy_total_runs >= 1
                    and s.remedy_success_count + s.remedy_failed_count >= 1)
                failed = await client.get(*WF, "health", second.last_failed_workflow)
                text = b"".join([c async for c in http.logs(
                    "health", second.last_failed_workflow)]).decode()
                return first, second, failed, text, srv.requests, await srv.settled()
            finally:
                await http.close()
                await manager.stop()
                await engine.stop()
                await frontend.stop()
                logs.close()

    first, second, failed, text, requests, settled = run(go(), timeout=45)
    assert second.success_count == 1 and second.failed_count == 1
    assert second.status == "Failed" and second.remedy_success_count == 1
    assert marker.read_text() == "fixed\n"
    assert failed["status"]["phase"] == "Failed"
    assert "evaluated false (status 503)" in failed["status"]["message"]
    (node,) = failed["status"]["nodes"].values()
    assert node["type"] == "HTTP"
    # both requests carried the header; the log shows neither value
    assert [r.headers["authorization"] for r in requests] == [SECRET, SECRET]
    lines = text.splitlines()
    assert lines[0].startswith("> GET http://127.0.0.1:") and lines[0].endswith("/healthz")
    assert lines[1].startswith("< 503 Service Unavailable (9 bytes, ")
    assert lines[2] == "draining"
    assert "s3cret" not in text and "Authorization" not in text
    assert settled


def cli_env():
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    return env


def test_cli_lints_and_runs_the_shipped_example(run):
    async def cli(*args):
        proc = await asyncio.create_subprocess_exec(
            sys.executable, "-m", "active_monitor_amd.workflow", *args, cwd=str(REPO),
            env=cli_env(), stdout=asyncio.subprocess.PIPE, stderr=asyncio.subprocess.STDOUT)
        out, _ = await asyncio.wait_for(proc.communicate(), 60)
        return proc.returncode, out.decode()

    async def go():
        routes = {"/healthz": Route(body=b'{"status":"ok","since":"boot"}')}
        async with ProbeServer(routes) as srv:
            linted = await cli("lint", "examples/inline-http.yaml")
            ran = await cli("run", "examples/inline-http.yaml", "-p",
                            f"url={srv.url}/healthz", "--logs")
            return linted, ran, srv.paths()

    linted, (rc, out), paths = run(go(), timeout=90)
    assert linted == (0, "ok\n")
    assert rc == 0, out
    assert paths == ["/healthz"]
    assert "phase: Succeeded" in out and "output status: ok" in out
    rows = [line.split() for line in out.splitlines()]
    assert ["run", "Retry", "Succeeded"] in rows
    assert ["run(0)", "HTTP", "Succeeded"] in rows  # the first attempt passed
    at = out.splitlines().index("--- run(0) ---")
    log = out.splitlines()[at + 1:]
    assert log[0].endswith("/healthz") and log[0].startswith("> GET http://127.0.0.1:")
    assert log[1].startswith("< 200 OK (30 bytes, ")
    assert log[2] == '{"status":"ok","since":"boot"}'

"""The engine's limits from the command line down: a fleet of checks under
``--workflow-parallelism``, the limits on ``/statusz``, and the flags of both
entry points."""
import asyncio
import json
import urllib.request

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.cmd.main import build_parser, main
from active_monitor_amd.cmd.main import run as cli_run
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube import standalone
from active_monitor_amd.kube.http import HttpClient

API_PORT, METRICS_PORT = 18391, 18392


def peak_check(i, tmp, timeout=30, mutex=None):
    """A HealthCheck that runs once; its leaf records how many leaves of the
    fleet are alive with it, and when it started and ended."""
    script = (f"cd {tmp} && mkdir alive.$$; ls -d alive.* | wc -l >> peak; "
              f"echo start {i} >> spans; sleep 0.3; echo end {i} >> spans; rmdir alive.$$")
    spec = {"entrypoint": "main", "templates": [
        {"name": "main", "container": {"command": ["sh", "-c", script]}}]}
    if mutex:
        spec["synchronization"] = {"mutex": {"name": mutex}}
    return {
        "apiVersion": API_VERSION, "kind": "HealthCheck",
        "metadata": {"name": f"fleet-{i}", "namespace": "health"},
        "spec": {"repeatAfterSec": 600, "level": "cluster", "workflow": {
            "generateName": f"fleet-{i}-wf-", "workflowtimeout": timeout,
            "resource": {"namespace": "health", "serviceAccount": "fleet-sa",
                         "source": {"inline": yaml.safe_dump({
                             "apiVersion": "argoproj.io/v1alpha1", "kind": "Workflow",
                             "spec": spec})}}}},
    }


def _fetch_json(url):
    with urllib.request.urlopen(url, timeout=5) as r:
        return json.loads(r.read())


def test_six_checks_under_workflow_parallelism_two(run, tmp_path):
    async def go():
        args = build_parser().parse_args([
            "--backend", "memory", "--workflow-parallelism", "2",
            "--serve-api", f"127.0.0.1:{API_PORT}",
            "--metrics-bind-address", f"127.0.0.1:{METRICS_PORT}", "--no-metrics-secure",
            "--health-probe-bind-address", "0",
        ])
        stop = asyncio.Event()
        task = asyncio.ensure_future(cli_run(args, stop))
        client = HttpClient(f"http://127.0.0.1:{API_PORT}")
        await client.start()
        loop = asyncio.get_running_loop()
        try:
            deadline = loop.time() + 15
            while True:
                try:
                    await client.ping()
                    break
                except Exception:
                    assert loop.time() < deadline and not task.done()
                    await asyncio.sleep(0.05)
            for i in range(6):
                await client.create(peak_check(i, tmp_path))
            deadline = loop.time() + 30
            while True:
                checks = await client.list(API_VERSION, "HealthCheck", "health")
                counts = [(c.get("status") or {}).get("successCount", 0) for c in checks]
                if counts == [1] * 6:
                    break
                assert loop.time() < deadline, [c.get("status") for c in checks]
                await asyncio.sleep(0.05)
            statusz = await loop.run_in_executor(
                None, _fetch_json, f"http://127.0.0.1:{METRICS_PORT}/statusz")
            return checks, statusz
        finally:
            await client.close()
            stop.set()
            assert await asyncio.wait_for(task, 15) == 0

    checks, statusz = run(go(), timeout=70)
    assert all((c["status"].get("failedCount") or 0) == 0 for c in checks)
    seen = [int(n) for n in (tmp_path / "peak").read_text().split()]
    assert len(seen) == 6
    assert max(seen) == 2
    engine = statusz["workflow_engine"]
    assert engine["limits"] == {"parallelism": 2, "namespace_parallelism": None,
                                "max_processes": None}
    assert engine["postponed_total"] == 4
    assert (engine["running"], engine["queued"], engine["processes"]) == (0, 0, 0)
    assert statusz["ready"] is True  # the keys that were there stay


@pytest.mark.parametrize("flag", ["--workflow-parallelism", "--workflow-namespace-parallelism",
                                  "--workflow-max-processes"])
def test_limit_flags_are_for_the_memory_backend_and_positive(flag, capsys):
    with pytest.raises(SystemExit) as exc:
        main(["--backend", "http", "--server", "http://127.0.0.1:1", flag, "2"])
    assert exc.value.code == 2
    assert f"{flag} applies to --backend memory only" in capsys.readouterr().err
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit) as exc:
            main([flag, bad])
        assert exc.value.code == 2
        assert f"{flag} must be a positive integer" in capsys.readouterr().err


def test_standalone_flags_reach_the_engine(capsys):
    args = standalone.parse_args([
        "--engine", "local", "--engine-parallelism", "3",
        "--engine-namespace-parallelism", "2", "--engine-max-processes", "5"])
    options = standalone.limit_options(args, "engine")
    for kind in ("local", "scripted-bench"):
        engine = standalone.build_engine(kind, MemoryClient(MemoryApiServer()), None, **options)
        assert engine.stats()["limits"] == {
            "parallelism": 3, "namespace_parallelism": 2, "max_processes": 5}
    assert standalone.limit_options(standalone.parse_args([]), "engine") == {}
    with pytest.raises(SystemExit):
        standalone.parse_args(["--engine-max-processes", "0"])
    assert "--engine-max-processes must be a positive integer" in capsys.readouterr().err

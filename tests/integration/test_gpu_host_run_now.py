"""GPU-box validation of running a check on demand.

Like the other test_gpu_host files this validates the host, not a kernel:
the manual-only example is applied to a standalone stack and run with
``amctl run --wait --logs`` over the wire, whose subprocess leaf, log pipe
and HTTP follow stream are the host-dependent part; and a short bench run
must complete with the scheduler branches the feature touches carrying the
benchmark fleet. Nothing here touches the device beyond what bench.py does.
"""
import asyncio
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.api import RUN_HANDLED_ANNOTATION, RUN_WORKFLOW_ANNOTATION
from active_monitor_amd.cmd.ctl import build_parser
from active_monitor_amd.cmd.ctl import run as ctl_run
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import LocalWorkflowEngine
from active_monitor_amd.workflow.logs import LogStore

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).parents[2]
WF = ("argoproj.io/v1alpha1", "Workflow")


def test_amctl_runs_the_manual_only_example_over_the_wire_on_gpu_host(run, capsys):
    example = REPO / "examples" / "manual-only.yaml"
    meta = yaml.safe_load(example.read_text())["metadata"]
    name, ns = meta["name"], meta["namespace"]

    async def go():
        server = MemoryApiServer()
        client = MemoryClient(server)
        logs = LogStore()
        engine = LocalWorkflowEngine(client, ttl_seconds=None, logs=logs)
        frontend = ApiServerFrontend(server, logs=logs)
        manager = Manager(client, max_workers=2)
        await frontend.start()
        await engine.start()
        await manager.start()

        async def ctl(*argv):
            args = build_parser().parse_args(["--server", frontend.url, *argv])
            return await asyncio.wait_for(ctl_run(args), 30)

        try:
            assert await ctl("apply", "-f", str(example)) == 0
            for _ in range(1000):
                hc = await client.get(API_VERSION, "HealthCheck", ns, name)
                if (hc.get("status") or {}).get("status") == "Stopped":
                    break
                await asyncio.sleep(0.01)
            assert await client.list(*WF, ns) == []  # it never runs by itself
            capsys.readouterr()
            rc = await ctl("run", "hc", name, "-n", ns, "--wait", "--logs",
                           "--timeout", "25")
            out = capsys.readouterr().out
            hc = await client.get(API_VERSION, "HealthCheck", ns, name)
            return rc, out, hc, await client.list(*WF, ns)
        finally:
            await manager.stop()
            await engine.stop()
            await frontend.stop()
            logs.close()

    rc, out, hc, wfs = run(go(), timeout=40)
    assert rc == 0, out
    (wf,) = wfs
    wf_name = wf["metadata"]["name"]
    assert wf["status"]["phase"] == "Succeeded"
    annotations = hc["metadata"]["annotations"]
    assert annotations[RUN_WORKFLOW_ANNOTATION] == wf_name
    assert annotations[RUN_HANDLED_ANNOTATION] in out.splitlines()[0]
    lines = out.splitlines()
    assert f"{wf_name}: checked on demand" in lines  # the step's output
    assert lines[-1] == f"healthcheck/{name} Succeeded (workflow {wf_name})"


def test_short_bench_runs_every_cr_with_the_changed_scheduler_branches(tmp_path):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--crs", "50", "--steps", "2", "--warmup", "1",
         "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    data = json.loads(out.stdout.strip().splitlines()[-1])
    assert data["metric"] == "sustained_healthcheck_cycles_per_sec"
    status = np.load(os.path.join(tmp_path, "healthcheck_status.npy"))
    assert status.shape == (50, 8)
    assert status[:, 5].min() >= 4  # totalHealthCheckRuns of every CR

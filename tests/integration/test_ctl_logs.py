"""``amctl logs`` against the HTTP frontend, ``workflow run --logs`` and the
log flags of the controller's command line."""
import asyncio
import os
import subprocess
import sys

from active_monitor_amd import API_VERSION
from active_monitor_amd.cmd.ctl import build_parser
from active_monitor_amd.cmd.ctl import run as ctl_run
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import LocalWorkflowEngine
from active_monitor_amd.workflow.logs import LogStore

from .conftest import make_hc

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WF = ("argoproj.io/v1alpha1", "Workflow")

FAILING_WF = """\
apiVersion: argoproj.io/v1alpha1
kind: Workflow
spec:
  entrypoint: probe
  templates:
    - name: probe
      container:
        command: [sh, -c, "echo probing resolver; echo resolver down >&2; exit 1"]
"""


def sh(script):
    return {"entrypoint": "main", "templates": [
        {"name": "main", "container": {"command": ["sh", "-c", script]}}]}


class Cluster:
    """A standalone process's parts: store, log store, engine, controller
    and REST frontend."""

    def __init__(self, ttl=None, controller=True):
        self.server = MemoryApiServer()
        self.client = MemoryClient(self.server)
        self.logs = LogStore()
        self.engine = LocalWorkflowEngine(self.client, ttl_seconds=ttl, logs=self.logs)
        self.manager = Manager(self.client, max_workers=2) if controller else None
        self.frontend = ApiServerFrontend(self.server, logs=self.logs)

    async def __aenter__(self):
        await self.frontend.start()
        await self.engine.start()
        if self.manager is not None:
            await self.manager.start()
        return self

    async def __aexit__(self, *exc):
        if self.manager is not None:
            await self.manager.stop()
        await self.engine.stop()
        await self.frontend.stop()
        self.logs.close()

    async def hc_status(self, name, until):
        for _ in range(1000):
            hc = await self.client.get(API_VERSION, "HealthCheck", "health", name)
            status = hc.get("status") or {}
            if until(status):
                return status
            await asyncio.sleep(0.01)
        raise AssertionError(f"healthcheck {name} never got there: {status}")


def make_ctl(cluster, capsys):
    async def ctl(*argv):
        args = build_parser().parse_args(["--server", cluster.frontend.url, *argv])
        rc = await asyncio.wait_for(ctl_run(args), 10)
        captured = capsys.readouterr()
        return rc, captured.out, captured.err

    return ctl


def test_logs_of_a_workflow(run, capsys):
    async def go():
        async with Cluster() as c:
            ctl = make_ctl(c, capsys)
            await c.client.create({
                "apiVersion": WF[0], "kind": WF[1],
                "metadata": {"name": "w1", "namespace": "health"},
                "spec": sh("echo one; sleep 0.3; echo two"),
            })
            # -f returns by itself, once the workflow has finished
            rc, out, err = await ctl("logs", "wf", "w1", "-f")
            assert rc == 0 and out == "w1: one\nw1: two\n"
            assert err.startswith("==> workflow w1 (") and err.endswith(") <==\n")
            wf = await c.client.get(*WF, "health", "w1")
            assert wf["status"]["phase"] == "Succeeded"

            rc, out, err = await ctl("logs", "wf", "w1", "-n", "health")
            assert rc == 0 and out == "w1: one\nw1: two\n"
            assert err == "==> workflow w1 (Succeeded) <==\n"
            rc, out, _ = await ctl("logs", "workflow", "w1", "--no-prefix", "--tail", "1")
            assert rc == 0 and out == "two\n"
            rc, out, _ = await ctl("logs", "wf", "w1", "--node", "w1")
            assert rc == 0 and out == "one\ntwo\n"

            rc, out, err = await ctl("logs", "wf", "nothing")
            assert rc == 1 and out == "" and err.startswith("Error: ") and "nothing" in err

            # the workflow outlives its logs only when they are dropped
            c.logs.discard("health", "w1")
            rc, out, err = await ctl("logs", "wf", "w1")
            assert rc == 1 and out == ""
            assert err.splitlines()[-1].startswith("Error: ")
            assert "w1" in err and "engine TTL" in err

    run(go())


def test_logs_of_a_healthcheck(run, capsys):
    async def go():
        async with Cluster() as c:
            ctl = make_ctl(c, capsys)
            await c.client.create(make_hc(name="dns", repeat=3600, inline=FAILING_WF))
            status = await c.hc_status("dns", lambda st: st.get("failedCount", 0) >= 1)
            assert status["status"] == "Failed"
            wf_name = status["lastFailedWorkflow"]

            rc, out, err = await ctl("logs", "hc", "dns", "-n", "health")
            assert rc == 0, err
            # the entrypoint is a leaf: its node carries the workflow's name
            assert sorted(out.splitlines()) == [
                f"{wf_name}: probing resolver", f"{wf_name}: resolver down"]
            assert err == f"==> workflow {wf_name} (Failed) <==\n"

            rc, out, _ = await ctl("logs", "hc", "dns", "--failed", "--no-prefix")
            assert rc == 0 and sorted(out.splitlines()) == ["probing resolver", "resolver down"]

            rc, out, err = await ctl("logs", "hc", "dns", "--succeeded")
            assert rc == 1 and out == ""
            assert err == "Error: healthcheck dns has no successful workflow yet\n"

            # the workflow is gone (TTL, or a delete): worded, with its name
            await c.client.delete(*WF, "health", wf_name)
            rc, out, err = await ctl("logs", "hc", "dns")
            assert rc == 1 and out == ""
            assert err.startswith("Error: ") and wf_name in err and "engine TTL" in err

            rc, _, err = await ctl("logs", "hc", "absent")
            assert rc == 1 and err.startswith("Error: ")

        # a HealthCheck no controller has run yet
        async with Cluster(controller=False) as c:
            ctl = make_ctl(c, capsys)
            await c.client.create(make_hc(name="idle", repeat=3600))
            rc, out, err = await ctl("logs", "hc", "idle")
            assert (rc, out, err) == (1, "", "Error: healthcheck idle has not run yet\n")

    run(go())


def test_workflow_run_prints_a_block_per_pod_node():
    out = subprocess.run(
        [sys.executable, "-m", "active_monitor_amd.workflow", "run",
         "examples/inline-dag.yaml", "--logs"],
        capture_output=True, text=True, timeout=60, cwd=REPO,
    )
    assert out.returncode == 0, out.stdout + out.stderr
    table, _, blocks = out.stdout.partition("--- ")
    assert "phase: Succeeded" in table and "report" in table
    blocks = ("--- " + blocks).splitlines()
    heads = [line for line in blocks if line.startswith("--- ")]
    assert heads == ["--- sample ---", "--- low ---", "--- high ---", "--- report ---"]
    assert blocks[blocks.index("--- sample ---") + 1] == "17"
    assert blocks[-1] == "queue depth 17 is within bounds"
    # without the flag the output ends with the node table, as before
    plain = subprocess.run(
        [sys.executable, "-m", "active_monitor_amd.workflow", "run",
         "examples/inline-dag.yaml"],
        capture_output=True, text=True, timeout=60, cwd=REPO,
    )
    assert plain.returncode == 0 and "--- " not in plain.stdout
    assert plain.stdout == table


def test_controller_rejects_log_flags_with_http_backend():
    for flags in (["--log-max-bytes", "1"], ["--log-max-total-bytes", "4096"],
                  ["--no-workflow-logs"]):
        out = subprocess.run(
            [sys.executable, "-m", "active_monitor_amd.cmd.main", "--backend", "http",
             "--server", "http://127.0.0.1:1", *flags],
            capture_output=True, text=True, timeout=60, cwd=REPO,
        )
        assert out.returncode == 2, out.stderr  # argparse's argument-error status
        assert f"{flags[0]} applies to --backend memory only" in out.stderr
        assert "usage:" in out.stderr

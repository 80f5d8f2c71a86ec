"""``amctl run`` against the HTTP frontend: the request, ``--wait`` and its
exit statuses, ``--all`` and ``--logs``."""
import asyncio
import time

from active_monitor_amd import API_VERSION
from active_monitor_amd.api import (
    RUN_HANDLED_ANNOTATION,
    RUN_REQUEST_ANNOTATION,
    RUN_REQUESTED_ANNOTATION,
    RUN_WORKFLOW_ANNOTATION,
)
from active_monitor_amd.cmd.ctl import _run_verdict, build_parser
from active_monitor_amd.cmd.ctl import run as ctl_run
from active_monitor_amd.kube.http import HttpClient

from .conftest import make_hc
from .test_ctl_logs import FAILING_WF, WF, Cluster

PASSING_WF = """\
apiVersion: argoproj.io/v1alpha1
kind: Workflow
spec:
  entrypoint: probe
  templates:
    - name: probe
      container:
        command: [sh, -c, "echo resolver answers"]
"""


def make_ctl(cluster, capsys):
    async def ctl(*argv):
        args = build_parser().parse_args(["--server", cluster.frontend.url, *argv])
        rc = await asyncio.wait_for(ctl_run(args), 30)
        captured = capsys.readouterr()
        return rc, captured.out, captured.err

    return ctl


async def annotations(cluster, name):
    hc = await cluster.client.get(API_VERSION, "HealthCheck", "health", name)
    return hc["metadata"].get("annotations") or {}


def token_of(line, name):
    head = f"healthcheck/{name} run requested ("
    assert line.startswith(head) and line.endswith(")"), line
    return line[len(head):-1]


def test_run_sets_the_annotation_and_prints_the_token(run, capsys):
    async def go():
        async with Cluster(controller=False) as c:
            ctl = make_ctl(c, capsys)
            await c.client.create(make_hc(name="dns", repeat=3600))
            rc, out, err = await ctl("run", "hc", "dns", "-n", "health")
            assert rc == 0 and err == ""
            (line,) = out.splitlines()
            token = token_of(line, "dns")
            # by convention an RFC 3339 UTC time to the microsecond
            assert len(token) == len("2026-01-02T03:04:05.000006Z") and token.endswith("Z")
            assert await annotations(c, "dns") == {RUN_REQUESTED_ANNOTATION: token}

            # a new value each time: a new request
            rc, out, _ = await ctl("run", "hc", "dns")
            again = token_of(out.strip(), "dns")
            assert rc == 0 and again != token
            assert (await annotations(c, "dns"))[RUN_REQUESTED_ANNOTATION] == again

            rc, out, err = await ctl("run", "hc", "absent")
            assert rc == 1 and out == "" and err.startswith("Error: ") and "absent" in err

            # usage errors
            rc, out, err = await ctl("run", "hc", "dns", "--all")
            assert rc == 2 and out == "" and "--all" in err
            rc, out, err = await ctl("run", "hc")
            assert rc == 2 and out == "" and err.startswith("error: ")
            rc, out, err = await ctl("run", "hc", "dns", "other", "--logs")
            assert rc == 2 and out == "" and "--logs" in err
            assert (await annotations(c, "dns"))[RUN_REQUESTED_ANNOTATION] == again

    run(go())


def test_wait_returns_0_for_a_passing_check(run, capsys):
    async def go():
        async with Cluster() as c:
            ctl = make_ctl(c, capsys)
            await c.client.create(make_hc(name="ok", repeat=3600, inline=PASSING_WF))
            await c.hc_status("ok", lambda st: st.get("successCount", 0) >= 1)
            rc, out, err = await ctl("run", "hc", "ok", "--wait")
            assert rc == 0, err
            requested, running, verdict = out.splitlines()
            token = token_of(requested, "ok")
            ann = await annotations(c, "ok")
            assert ann[RUN_HANDLED_ANNOTATION] == token
            wf_name = ann[RUN_WORKFLOW_ANNOTATION]
            assert running == f"healthcheck/ok running as workflow {wf_name}"
            assert verdict == f"healthcheck/ok Succeeded (workflow {wf_name})"
            wf = await c.client.get(*WF, "health", wf_name)
            assert wf["status"]["phase"] == "Succeeded"
            assert wf["metadata"]["annotations"][RUN_REQUEST_ANNOTATION] == token
            status = await c.hc_status("ok", lambda st: st.get("successCount", 0) >= 2)
            assert status["lastSuccessfulWorkflow"] == wf_name

            # a workflow that is gone already (TTL) has left its verdict in
            # the status
            await c.client.delete(*WF, "health", wf_name)
            http = HttpClient(c.frontend.url, qps=0)
            await http.start()
            try:
                assert await _run_verdict(http, "health", "ok", "health", wf_name,
                                          time.monotonic() + 5.0) == "Succeeded"
            finally:
                await http.close()

    run(go())


def test_wait_returns_1_for_a_failing_check(run, capsys):
    async def go():
        async with Cluster() as c:
            ctl = make_ctl(c, capsys)
            await c.client.create(make_hc(name="dns", repeat=3600, inline=FAILING_WF))
            await c.hc_status("dns", lambda st: st.get("failedCount", 0) >= 1)
            rc, out, err = await ctl("run", "hc", "dns", "--wait", "--timeout", "20")
            assert rc == 1, err
            wf_name = (await annotations(c, "dns"))[RUN_WORKFLOW_ANNOTATION]
            assert out.splitlines()[-1] == f"healthcheck/dns Failed (workflow {wf_name})"

    run(go())


def test_wait_returns_2_when_no_controller_runs(run, capsys):
    async def go():
        async with Cluster(controller=False) as c:
            ctl = make_ctl(c, capsys)
            await c.client.create(make_hc(name="idle", repeat=3600))
            rc, out, err = await ctl("run", "hc", "idle", "--wait", "--timeout", "1")
            assert rc == 2
            token = token_of(out.strip(), "idle")
            assert err == ("error: healthcheck/idle: no controller handled the request: "
                           "is one running, and does it own this check?\n")
            # the request stands: a controller that starts later serves it
            assert await annotations(c, "idle") == {RUN_REQUESTED_ANNOTATION: token}

    run(go())


def test_all_covers_every_check_of_the_namespace(run, capsys):
    async def go():
        async with Cluster() as c:
            ctl = make_ctl(c, capsys)
            await c.client.create(make_hc(name="one", repeat=3600, inline=PASSING_WF))
            await c.client.create(make_hc(name="two", repeat=3600, inline=FAILING_WF))
            await c.hc_status("one", lambda st: st.get("successCount", 0) >= 1)
            await c.hc_status("two", lambda st: st.get("failedCount", 0) >= 1)
            rc, out, err = await ctl("run", "hc", "--all", "--wait", "-n", "health")
            assert rc == 1, err  # one of the two fails
            lines = out.splitlines()
            tokens = {name: token_of(line, name)
                      for name, line in zip(("one", "two"), sorted(lines[:2]))}
            for name, phase in (("one", "Succeeded"), ("two", "Failed")):
                ann = await annotations(c, name)
                assert ann[RUN_HANDLED_ANNOTATION] == tokens[name]
                wf_name = ann[RUN_WORKFLOW_ANNOTATION]
                assert f"healthcheck/{name} running as workflow {wf_name}" in lines
                assert f"healthcheck/{name} {phase} (workflow {wf_name})" in lines
            assert len(await c.client.list(*WF, "health")) == 4

    run(go())


def test_logs_prints_what_the_leaf_printed(run, capsys):
    async def go():
        async with Cluster() as c:
            ctl = make_ctl(c, capsys)
            # a manual-only check: nothing has run before the request
            await c.client.create(make_hc(name="manual", repeat=0, inline=PASSING_WF))
            await c.hc_status("manual", lambda st: st.get("status") == "Stopped")
            rc, out, err = await ctl("run", "hc", "manual", "--logs", "--timeout", "20")
            assert rc == 0, err
            wf_name = (await annotations(c, "manual"))[RUN_WORKFLOW_ANNOTATION]
            lines = out.splitlines()
            assert lines[1] == f"healthcheck/manual running as workflow {wf_name}"
            # the entrypoint is a leaf: its node carries the workflow's name
            assert f"{wf_name}: resolver answers" in lines
            assert lines[-1] == f"healthcheck/manual Succeeded (workflow {wf_name})"
            assert len(await c.client.list(*WF, "health")) == 1

    run(go())

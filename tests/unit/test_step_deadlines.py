"""Per-step deadlines of the local executor: a template's ``timeout`` bounds
the node as a whole, its ``activeDeadlineSeconds`` one attempt. The proof of
a kill is state: the node's message, which attempt nodes exist, and that the
leaf's process group is empty while its ``sleep 30`` had most of its time
left. Every deadline is 1 s against 30 s or against an instant leaf, so the
only time asserted is "sooner than the sleep"."""
import asyncio
import os
import time

import pytest

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine
from active_monitor_amd.workflow.executor import (
    POD_DEADLINE_MESSAGE,
    STEP_DEADLINE_MESSAGE,
    Bound,
    WorkflowRun,
)
from active_monitor_amd.workflow.logs import LogStore
from active_monitor_amd.workflow.validate import validate_workflow_spec
from tests.probeserver import ProbeServer, Route

WF = (WF_API_VERSION, WF_KIND)
#: what the bounded ``sleep`` would have taken
SLEEP = 30


def test_the_messages_are_the_documented_ones():
    assert STEP_DEADLINE_MESSAGE == "Step exceeded its deadline"
    assert POD_DEADLINE_MESSAGE == (
        "Pod was active on the node longer than the specified deadline")


async def run_workflow(spec, shared=(), logs=None, timeout=20.0):
    """Run ``spec`` to its end under a LocalWorkflowEngine and return the
    status as seen in the step of the loop that first saw it terminal."""
    client = MemoryClient(MemoryApiServer())
    for obj in shared:
        await client.create(obj)
    engine = LocalWorkflowEngine(client, ttl_seconds=None, logs=logs)
    await engine.start()
    try:
        await client.create({"apiVersion": WF[0], "kind": WF[1],
                             "metadata": {"name": "wf", "namespace": "health"}, "spec": spec})
        give_up = time.monotonic() + timeout
        while time.monotonic() < give_up:
            status = (await client.get(*WF, "health", "wf")).get("status") or {}
            if status.get("phase") in ("Succeeded", "Failed"):
                return status
            await asyncio.sleep(0.01)
        raise AssertionError(f"the workflow did not end: {status}")
    finally:
        await engine.stop()


def by_name(status):
    return {n["displayName"]: n for n in status["nodes"].values()}


def group_is_gone(pgid):
    try:
        os.killpg(pgid, 0)
    except ProcessLookupError:
        return True
    return False


#: prints, records its pid (the leader of its group), leaves a child in the
#: background and sleeps
HANG = ("echo before the cut\necho $$ > {{inputs.parameters.pidfile}}\n"
        f"sleep {SLEEP} &\nsleep {SLEEP}\n")


def hanging(pidfile, **fields):
    return {"name": "hang", "inputs": {"parameters": [{"name": "pidfile", "value": str(pidfile)}]},
            "script": {"command": ["sh"], "source": HANG}, **fields}


def test_timeout_kills_the_group_and_keeps_the_log(run, tmp_path):
    pidfile = tmp_path / "pid"
    seen = {}

    async def go():
        store = LogStore(str(tmp_path / "logs"))
        try:
            began = time.monotonic()
            status = await run_workflow(
                {"entrypoint": "hang", "templates": [hanging(pidfile, timeout="1s")]}, logs=store)
            # looked at as soon as Failed is seen: nothing may be left by then
            seen["gone"] = group_is_gone(int(pidfile.read_text()))
            seen["took"] = time.monotonic() - began
            chunks = [c async for c in store.read("health", "wf")]
            return status, b"".join(chunks)
        finally:
            store.close()

    status, logged = run(go(), timeout=40)
    assert status["phase"] == "Failed"
    (node,) = status["nodes"].values()
    assert node["phase"] == "Failed" and node["type"] == "Pod"
    assert node["message"] == "Step exceeded its deadline"
    assert status["message"] == "Step exceeded its deadline"
    assert "outputs" not in node and "outputs" not in status
    assert seen["gone"], "the leaf's process group still has a member"
    assert seen["took"] < SLEEP
    assert logged == b"before the cut\n"


def test_active_deadline_is_one_attempt_that_a_retry_follows(run):
    spec = {"entrypoint": "flaky", "templates": [{
        "name": "flaky", "activeDeadlineSeconds": 1, "retryStrategy": {"limit": 1},
        "script": {"command": ["sh"], "source":
                   f'if [ "{{{{retries}}}}" = 0 ]; then sleep {SLEEP}; fi\necho ok\n'}}]}
    began = time.monotonic()
    status = run(run_workflow(spec), timeout=40)
    assert time.monotonic() - began < SLEEP
    assert status["phase"] == "Succeeded", status
    nodes = by_name(status)
    assert sorted(nodes) == ["wf", "wf(0)", "wf(1)"]
    assert nodes["wf(0)"]["phase"] == "Failed"
    assert nodes["wf(0)"]["message"] == POD_DEADLINE_MESSAGE
    assert "outputs" not in nodes["wf(0)"]
    assert nodes["wf(1)"]["phase"] == "Succeeded"
    assert nodes["wf(1)"]["outputs"]["result"] == "ok"
    assert nodes["wf"]["type"] == "Retry" and nodes["wf"]["phase"] == "Succeeded"
    assert nodes["wf"]["outputs"]["result"] == "ok"


def test_timeout_spans_the_retries_and_abandons_the_backoff(run):
    spec = {"entrypoint": "bad", "templates": [{
        "name": "bad", "timeout": "1s",
        "retryStrategy": {"limit": 5, "backoff": {"duration": "10s"}},
        "container": {"command": ["sh", "-c", "exit 1"]}}]}
    began = time.monotonic()
    status = run(run_workflow(spec), timeout=40)
    assert time.monotonic() - began < 10  # the first backoff wait alone is 10 s
    assert status["phase"] == "Failed"
    assert status["message"] == STEP_DEADLINE_MESSAGE
    nodes = by_name(status)
    assert sorted(nodes) == ["wf", "wf(0)"]  # no second attempt
    assert nodes["wf"]["type"] == "Retry"
    assert nodes["wf"]["message"] == STEP_DEADLINE_MESSAGE
    assert nodes["wf(0)"]["message"].startswith("exit code 1")  # it ended by itself


def test_timeout_cuts_the_attempt_that_runs_under_a_retry(run, tmp_path):
    pidfile = tmp_path / "pid"
    spec = {"entrypoint": "hang", "templates": [
        hanging(pidfile, timeout="1s", retryStrategy={"limit": 3})]}
    status = run(run_workflow(spec), timeout=40)
    assert group_is_gone(int(pidfile.read_text()))
    nodes = by_name(status)
    assert sorted(nodes) == ["wf", "wf(0)"]
    assert {n["message"] for n in nodes.values()} == {STEP_DEADLINE_MESSAGE}
    assert {n["phase"] for n in nodes.values()} == {"Failed"}


@pytest.mark.parametrize("field, value, phase, message", [
    ("timeout", "500ms", "Failed", STEP_DEADLINE_MESSAGE),
    ("activeDeadlineSeconds", 1, "Succeeded", ""),
])
def test_the_two_clocks_differ_while_a_leaf_waits_for_a_slot(run, tmp_path, field, value,
                                                             phase, message):
    """The only process slot is held for 1.5 s. ``timeout`` counts the wait,
    so 500 ms run out in it and no process ever starts; the clock of
    ``activeDeadlineSeconds`` starts with the process, which takes no time."""
    marker = tmp_path / "started"
    spec = {"entrypoint": "quick", "templates": [{
        "name": "quick", field: value,
        "container": {"command": ["sh", "-c", f"touch {marker}"]}}]}

    async def go():
        slots = Bound(1)
        await slots.acquire()
        wf_run = WorkflowRun(spec, "wf", "health", process_slots=slots)
        task = asyncio.ensure_future(wf_run.run_entrypoint())
        await asyncio.sleep(1.5)
        started_while_held = marker.exists()
        slots.release()
        result = await task
        return result, wf_run.nodes, started_while_held, slots.held

    result, nodes, started_while_held, held = run(go(), timeout=30)
    assert result == (phase, message)
    assert not started_while_held
    assert marker.exists() == (phase == "Succeeded")
    assert held == 0
    (node,) = nodes.values()
    assert node["phase"] == phase and node["message"] == message


def referring(pidfile, limit=None, d=None):
    """``timeout`` from an input parameter or ``activeDeadlineSeconds`` from
    a workflow parameter."""
    tmpl = hanging(pidfile)
    params = []
    if limit is not None:
        tmpl["inputs"]["parameters"].append({"name": "limit", "value": limit})
        tmpl["timeout"] = "{{inputs.parameters.limit}}"
    if d is not None:
        params.append({"name": "d", "value": d})
        tmpl["activeDeadlineSeconds"] = "{{workflow.parameters.d}}"
    return {"entrypoint": "hang", "arguments": {"parameters": params}, "templates": [tmpl]}


@pytest.mark.parametrize("given, message", [
    ({"limit": "1s"}, STEP_DEADLINE_MESSAGE),
    ({"d": "1"}, POD_DEADLINE_MESSAGE),
])
def test_references_are_honoured(run, tmp_path, given, message):
    pidfile = tmp_path / "pid"
    spec = referring(pidfile, **given)
    assert validate_workflow_spec(spec) == []
    began = time.monotonic()
    status = run(run_workflow(spec), timeout=40)
    assert time.monotonic() - began < SLEEP
    assert group_is_gone(int(pidfile.read_text()))
    assert status["phase"] == "Failed" and status["message"] == message


@pytest.mark.parametrize("given, prefix", [
    ({"limit": "soon"}, "invalid timeout:"),
    ({"limit": "0"}, "invalid timeout:"),
    ({"d": "soon"}, "invalid activeDeadlineSeconds:"),
    ({"d": "0"}, "invalid activeDeadlineSeconds:"),
])
def test_a_reference_that_resolves_to_nothing_valid_fails_the_node_unstarted(
        run, tmp_path, given, prefix):
    pidfile = tmp_path / "pid"
    status = run(run_workflow(referring(pidfile, **given)), timeout=40)
    assert status["phase"] == "Failed"
    assert status["message"].startswith(prefix), status["message"]
    (node,) = status["nodes"].values()
    assert node["phase"] == "Failed" and node["message"] == status["message"]
    assert not pidfile.exists()  # the script never ran


def test_timeout_on_an_http_template_closes_the_socket(run):
    async def go():
        async with ProbeServer({"/slow": Route(delay=SLEEP, body=b"late")}) as srv:
            began = time.monotonic()
            status = await run_workflow({"entrypoint": "probe", "templates": [
                {"name": "probe", "timeout": "1s",
                 "http": {"url": srv.url + "/slow", "timeoutSeconds": 20}}]})
            took = time.monotonic() - began
            return status, took, await srv.settled(), len(srv.requests)

    status, took, settled, requests = run(go(), timeout=40)
    assert took < 20  # the probe's own timeout, and the answer after it, never came
    assert status["phase"] == "Failed" and status["message"] == STEP_DEADLINE_MESSAGE
    (node,) = status["nodes"].values()
    assert node["type"] == "HTTP" and node["message"] == STEP_DEADLINE_MESSAGE
    assert requests == 1
    assert settled, "the probe's connection is still open"


def test_timeout_on_a_suspend_template(run):
    status = run(run_workflow({"entrypoint": "pause", "templates": [
        {"name": "pause", "timeout": "1s", "suspend": {"duration": f"{SLEEP}s"}}]}), timeout=40)
    assert status["phase"] == "Failed" and status["message"] == STEP_DEADLINE_MESSAGE


def test_a_leaf_reached_from_on_exit_is_bounded(run, tmp_path):
    pidfile = tmp_path / "pid"
    spec = {"entrypoint": "fine", "onExit": "hang", "templates": [
        {"name": "fine", "container": {"command": ["true"]}},
        hanging(pidfile, activeDeadlineSeconds=1)]}
    began = time.monotonic()
    status = run(run_workflow(spec), timeout=40)
    assert time.monotonic() - began < SLEEP
    assert group_is_gone(int(pidfile.read_text()))
    assert status["phase"] == "Failed" and status["message"] == POD_DEADLINE_MESSAGE
    assert by_name(status)["wf.onExit"]["message"] == POD_DEADLINE_MESSAGE
    assert by_name(status)["wf"]["phase"] == "Succeeded"


def test_a_leaf_reached_through_template_ref_is_bounded(run, tmp_path):
    pidfile = tmp_path / "pid"
    lib = {"apiVersion": WF[0], "kind": "WorkflowTemplate",
           "metadata": {"name": "lib", "namespace": "health"},
           "spec": {"templates": [hanging(pidfile, timeout="1s")]}}
    spec = {"entrypoint": "main", "templates": [{"name": "main", "steps": [[
        {"name": "call", "templateRef": {"name": "lib", "template": "hang"}}]]}]}
    began = time.monotonic()
    status = run(run_workflow(spec, shared=[lib]), timeout=40)
    assert time.monotonic() - began < SLEEP
    assert group_is_gone(int(pidfile.read_text()))
    assert status["phase"] == "Failed" and status["message"] == STEP_DEADLINE_MESSAGE
    call = by_name(status)["call"]
    assert call["templateRef"] == {"name": "lib", "template": "hang"}
    assert call["message"] == STEP_DEADLINE_MESSAGE


def test_the_workflow_deadline_still_wins(run, tmp_path):
    """Control: this passes without the feature too."""
    pidfile = tmp_path / "pid"
    out = hanging(pidfile, timeout="20s")
    out["outputs"] = {"parameters": [{"name": "late", "value": "x", "globalName": "late"}]}
    spec = {"entrypoint": "hang", "activeDeadlineSeconds": 1, "templates": [out]}
    status = run(run_workflow(spec), timeout=40)
    assert group_is_gone(int(pidfile.read_text()))
    assert status["phase"] == "Failed" and status["message"] == "deadline exceeded"
    (node,) = status["nodes"].values()
    assert node["message"] == "deadline exceeded"
    assert "outputs" not in status  # timed_out: nothing is published


def leaf(**fields):
    return {"entrypoint": "main", "arguments": {"parameters": [{"name": "d", "value": "5"}]},
            "templates": [{"name": "main", "container": {"command": ["true"]}, **fields}]}


@pytest.mark.parametrize("spec, problem", [
    ({"entrypoint": "main", "templates": [
        {"name": "main", "timeout": "30s", "steps": [[{"name": "a", "template": "ok"}]]},
        {"name": "ok", "container": {"command": ["true"]}}]},
     "template 'main': timeout is not supported on steps and dag templates"),
    ({"entrypoint": "main", "templates": [
        {"name": "main", "timeout": "30s", "dag": {"tasks": [{"name": "a", "template": "ok"}]}},
        {"name": "ok", "container": {"command": ["true"]}}]},
     "template 'main': timeout is not supported on steps and dag templates"),
    (leaf(timeout="soon"), "template 'main': invalid timeout: invalid duration 'soon'"),
    (leaf(activeDeadlineSeconds=0),
     "template 'main': invalid activeDeadlineSeconds: 0 is not a positive integer"),
    (leaf(activeDeadlineSeconds=-1),
     "template 'main': invalid activeDeadlineSeconds: -1 is not a positive integer"),
    (leaf(activeDeadlineSeconds=1.5),
     "template 'main': invalid activeDeadlineSeconds: 1.5 is not a positive integer"),
    (leaf(activeDeadlineSeconds=True),
     "template 'main': invalid activeDeadlineSeconds: True is not a positive integer"),
])
def test_lint_names_a_bad_deadline(spec, problem):
    assert validate_workflow_spec(spec) == [problem]


@pytest.mark.parametrize("spec", [
    leaf(timeout="{{workflow.parameters.d}}"),
    leaf(activeDeadlineSeconds="{{workflow.parameters.d}}"),
    leaf(timeout="30s"),
    leaf(timeout="1m30s"),
    leaf(timeout="45"),
    leaf(timeout=0),
    leaf(timeout=""),
    leaf(activeDeadlineSeconds=30),
    leaf(activeDeadlineSeconds="45"),
    {"entrypoint": "main", "templates": [
        {"name": "main", "activeDeadlineSeconds": 5, "http": {"url": "http://127.0.0.1:1/"}}]},
    {"entrypoint": "main", "templates": [
        {"name": "main", "activeDeadlineSeconds": 5,
         "steps": [[{"name": "a", "template": "ok"}]]},
        {"name": "ok", "container": {"command": ["true"]}}]},
])
def test_lint_accepts(spec):
    assert validate_workflow_spec(spec) == []

"""``http`` templates through LocalWorkflowEngine: node type and outputs, the
non-2xx rule, ``successCondition``, output parameters, retries, DAG data
flow, the deadline, and that a probe never takes a process slot."""
import asyncio
import json
import time

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine
from active_monitor_amd.workflow.executor import HTTP_MAX_IN_FLIGHT
from tests.probeserver import ProbeServer, Route


async def run_workflow(make_spec, routes, timeout=20.0, watch=None, **engine_kw):
    """Start a server with ``routes``, run ``make_spec(server)`` to its end
    and return ``(status, server, engine)``; ``watch(engine)`` is called on
    every poll while the workflow runs."""
    async with ProbeServer(routes) as srv:
        client = MemoryClient(MemoryApiServer())
        engine = LocalWorkflowEngine(client, **engine_kw)
        await engine.start()
        try:
            await client.create({
                "apiVersion": WF_API_VERSION, "kind": WF_KIND,
                "metadata": {"name": "wf", "namespace": "health"},
                "spec": make_spec(srv),
            })
            deadline = time.monotonic() + timeout
            status = {}
            while time.monotonic() < deadline:
                wf = await client.get(WF_API_VERSION, WF_KIND, "health", "wf")
                status = wf.get("status") or {}
                if watch is not None:
                    watch(engine)
                if status.get("phase") in ("Succeeded", "Failed"):
                    break
                await asyncio.sleep(0.005)
            assert await srv.settled()
            while engine.stats()["running"] and time.monotonic() < deadline:
                await asyncio.sleep(0.005)  # the run's task ends after its last write
            stats = engine.stats()
        finally:
            await engine.stop()
        return status, srv, stats


def one(path, **http):
    def make(srv):
        return {"entrypoint": "probe", "templates": [
            {"name": "probe", "http": {"url": srv.url + path, **http}}]}
    return make


def test_a_200_succeeds_with_an_http_node_and_the_body_as_result(run):
    st, srv, stats = run(run_workflow(one("/ok"), {"/ok": Route(body=b'{"status":"ok"}\n')}))
    assert st["phase"] == "Succeeded", st
    (node,) = st["nodes"].values()
    assert node["type"] == "HTTP" and node["phase"] == "Succeeded"
    assert node["templateName"] == "probe"
    assert node["outputs"] == {"result": '{"status":"ok"}\n'}
    assert [(r.method, r.target) for r in srv.requests] == [("GET", "/ok")]
    assert stats["processes"] == 0 and stats["running"] == 0


def test_a_503_without_a_condition_fails_with_argos_message(run):
    st, _, _ = run(run_workflow(one("/down"), {"/down": Route(503, "Unavailable", body=b"no")}))
    assert st["phase"] == "Failed"
    assert st["message"] == "received non-2xx response code: 503"
    (node,) = st["nodes"].values()
    assert node["type"] == "HTTP" and node["phase"] == "Failed" and "outputs" not in node


def test_the_condition_alone_decides(run):
    routes = {"/gone": Route(404, "Not Found", body=b"nothing here"),
              "/ok": Route(body=b'{"status":"degraded"}')}
    st, _, _ = run(run_workflow(
        one("/gone", successCondition="response.statusCode == 404"), routes))
    assert st["phase"] == "Succeeded", st
    (node,) = st["nodes"].values()
    assert node["outputs"]["result"] == "nothing here"

    cond = 'response.statusCode == 200 && jsonpath(response.body, "$.status") == "ok"'
    st, _, _ = run(run_workflow(one("/ok", successCondition=cond), routes))
    assert st["phase"] == "Failed"
    assert st["message"] == f"successCondition {cond!r} evaluated false (status 200)"

    st, _, _ = run(run_workflow(one("/ok", successCondition="response.statusCode"), routes))
    assert st["phase"] == "Failed"
    assert st["message"].startswith("invalid successCondition: ") and "int" in st["message"]

    st, _, _ = run(run_workflow(
        one("/gone", successCondition='jsonpath(response.body, "$.status") == "ok"'), routes))
    assert st["phase"] == "Failed"
    assert st["message"].startswith("invalid successCondition: jsonpath()")


def test_request_fields_are_substituted_and_expression_outputs_surface(run):
    metrics = {"metrics": [{"name": "depth", "value": 17, "metrictype": "gauge"}]}

    def make(srv):
        return {
            "entrypoint": "probe",
            "arguments": {"parameters": [{"name": "base", "value": srv.url},
                                         {"name": "want", "value": "201"}]},
            "templates": [{
                "name": "probe",
                "inputs": {"parameters": [{"name": "who", "value": "ops"}]},
                "http": {
                    "url": "{{workflow.parameters.base}}/submit",
                    "method": "POST",
                    "headers": [{"name": "X-Who", "value": "{{inputs.parameters.who}}"}],
                    "body": "from {{workflow.name}}",
                    "successCondition": "response.statusCode == {{workflow.parameters.want}}",
                },
                "outputs": {"parameters": [
                    {"name": "depth", "valueFrom": {
                        "expression": 'jsonpath(response.body, "$.metrics[0].value")'}},
                    {"name": "all", "globalName": "custom-metrics", "valueFrom": {
                        "expression": 'jsonpath(response.body, "$.metrics")'}},
                    {"name": "kind", "valueFrom": {
                        "expression": 'response.headers["content-type"][0]'}},
                    {"name": "missing", "valueFrom": {
                        "expression": 'jsonpath(response.body, "$.nope")', "default": "none"}},
                    {"name": "fixed", "value": "{{inputs.parameters.who}}"},
                ]},
            }],
        }

    st, srv, _ = run(run_workflow(make, {"/submit": Route(
        201, "Created", headers=[("Content-Type", "application/json")],
        body=json.dumps(metrics))}))
    assert st["phase"] == "Succeeded", st
    (seen,) = srv.requests
    assert (seen.method, seen.target, seen.body) == ("POST", "/submit", b"from wf")
    assert seen.headers["x-who"] == "ops"
    (node,) = st["nodes"].values()
    assert {p["name"]: p["value"] for p in node["outputs"]["parameters"]} == {
        "depth": "17", "all": json.dumps(metrics["metrics"]), "kind": "application/json",
        "missing": "none", "fixed": "ops"}
    # a leaf's parameters surface under globalName or their own name
    assert {p["name"]: p["value"] for p in st["outputs"]["parameters"]} == {
        "depth": "17", "custom-metrics": json.dumps(metrics["metrics"]),
        "kind": "application/json", "missing": "none", "fixed": "ops"}


def test_an_expression_output_without_a_value_or_default_fails_the_node(run):
    def make(srv):
        return {"entrypoint": "probe", "templates": [{
            "name": "probe", "http": {"url": srv.url + "/ok"},
            "outputs": {"parameters": [{"name": "depth", "valueFrom": {
                "expression": 'jsonpath(response.body, "$.depth")'}}]}}]}

    st, _, _ = run(run_workflow(make, {"/ok": Route(body=b"{}")}))
    assert st["phase"] == "Failed"
    assert st["message"].startswith("output parameter 'depth': jsonpath()")


def test_retry_strategy_retries_the_probe(run):
    def make(srv):
        return {"entrypoint": "probe", "templates": [{
            "name": "probe", "retryStrategy": {"limit": 2},
            "http": {"url": srv.url + "/flaky?try={{retries}}"}}]}

    st, srv, _ = run(run_workflow(make, {"/flaky": [
        Route(503, "Unavailable"), Route(503, "Unavailable"), Route(body=b"up")]}))
    assert st["phase"] == "Succeeded", st
    assert srv.paths() == ["/flaky?try=0", "/flaky?try=1", "/flaky?try=2"]
    attempts = sorted((n for n in st["nodes"].values() if n["type"] == "HTTP"),
                      key=lambda n: n["displayName"])
    assert [(n["displayName"], n["phase"]) for n in attempts] == [
        ("wf(0)", "Failed"), ("wf(1)", "Failed"), ("wf(2)", "Succeeded")]
    assert attempts[0]["message"] == "received non-2xx response code: 503"
    (retry,) = [n for n in st["nodes"].values() if n["type"] == "Retry"]
    assert retry["phase"] == "Succeeded" and retry["outputs"] == {"result": "up"}


def test_a_dag_task_consumes_the_probes_result(run, tmp_path):
    out = tmp_path / "seen"

    def make(srv):
        return {"entrypoint": "main", "templates": [
            {"name": "main", "dag": {"tasks": [
                {"name": "probe", "template": "get"},
                {"name": "skipped", "template": "get", "when": "1 == 2"},
                {"name": "use", "template": "write", "dependencies": ["probe"],
                 "arguments": {"parameters": [
                     {"name": "text", "value": "{{tasks.probe.outputs.result}}"},
                     {"name": "code", "value": "{{tasks.probe.outputs.parameters.code}}"}]}},
            ]}},
            {"name": "get", "http": {"url": srv.url + "/version"},
             "outputs": {"parameters": [
                 {"name": "code", "valueFrom": {"expression": "response.statusCode"}}]}},
            {"name": "write", "inputs": {"parameters": [{"name": "text"}, {"name": "code"}]},
             "container": {"command": ["sh", "-c", f'printf "%s %s" "$0" "$1" > {out}',
                                       "{{inputs.parameters.text}}",
                                       "{{inputs.parameters.code}}"]}},
        ]}

    st, srv, _ = run(run_workflow(make, {"/version": Route(body=b"v1.2.3")}))
    assert st["phase"] == "Succeeded", st
    assert out.read_text() == "v1.2.3 200"
    types = {n["displayName"]: (n["type"], n["phase"]) for n in st["nodes"].values()}
    assert types["probe"] == ("HTTP", "Succeeded") and types["use"] == ("Pod", "Succeeded")
    assert types["skipped"] == ("Skipped", "Skipped")
    assert len(srv.requests) == 1


def test_the_deadline_closes_the_socket_and_holds_no_process(run):
    def make(srv):
        return {"entrypoint": "probe", "activeDeadlineSeconds": 1, "templates": [
            {"name": "probe", "http": {"url": srv.url + "/slow", "timeoutSeconds": 60}}]}

    began = time.monotonic()
    st, srv, stats = run(run_workflow(make, {"/slow": Route(delay=30, body=b"late")}))
    # the server would have answered after 30 s; the bound follows from that gap
    assert time.monotonic() - began < 10
    assert st["phase"] == "Failed" and st["message"] == "deadline exceeded"
    (node,) = st["nodes"].values()
    assert node["type"] == "HTTP" and node["phase"] == "Failed"
    assert node["message"] == "deadline exceeded"
    assert srv.closed_early == ["/slow"] and srv.open == 0
    assert stats["processes"] == 0 and stats["running"] == 0


def test_the_probes_own_timeout_fails_the_node(run):
    st, srv, _ = run(run_workflow(
        one("/slow", timeoutSeconds=1), {"/slow": Route(delay=30)}))
    assert st["phase"] == "Failed"
    assert st["message"] == "http request failed: timed out after 1s"
    assert srv.closed_early == ["/slow"]


def test_a_hundred_probes_take_no_process_slot_and_at_most_64_run_at_once(run):
    held = []

    def make(srv):
        return {"entrypoint": "main", "templates": [
            {"name": "main", "steps": [[
                {"name": "fan", "template": "get", "withItems": list(range(100)),
                 "arguments": {"parameters": [{"name": "i", "value": "{{item}}"}]}}]]},
            {"name": "get", "inputs": {"parameters": [{"name": "i"}]},
             "http": {"url": srv.url + "/p?i={{inputs.parameters.i}}"}},
        ]}

    st, srv, stats = run(run_workflow(
        make, {"/p": Route(delay=0.1, body=b"ok")}, max_processes=1,
        watch=lambda engine: held.append((engine.process_slots.held, engine.http_slots.held))))
    assert st["phase"] == "Succeeded", st.get("message")
    probes = [n for n in st["nodes"].values() if n["type"] == "HTTP"]
    assert len(probes) == 100 and all(n["phase"] == "Succeeded" for n in probes)
    assert sorted(srv.paths()) == sorted(f"/p?i={i}" for i in range(100))
    assert HTTP_MAX_IN_FLIGHT == 64
    # more than one process' worth ran side by side, and never more than the bound
    assert 1 < srv.peak <= 64, srv.peak
    assert max(h for _, h in held) <= 64
    assert {p for p, _ in held} == {0}  # the one process slot was never taken
    assert stats["processes"] == 0

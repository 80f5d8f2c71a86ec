"""Static checks of ``http`` templates: a clean one has no problems, each
mistake is exactly one problem that names it."""
import pytest

from active_monitor_amd.workflow.validate import (
    BODY_TYPES,
    UNSUPPORTED_BODY_TYPES,
    validate_workflow_spec,
)

CLEAN = {
    "url": "http://{{workflow.parameters.host}}/healthz",
    "method": "POST",
    "headers": [{"name": "Authorization", "value": "Bearer {{inputs.parameters.token}}"},
                {"name": "Content-Type", "value": "application/json"}],
    "body": '{"deep": true}',
    "timeoutSeconds": 2,
    "insecureSkipVerify": False,
    "successCondition":
        'response.statusCode in 200..299 && jsonpath(response.body, "$.status") == "ok" '
        '&& response.headers["content-type"][0] startsWith "application/json"',
}


def spec(http=None, outputs=None, **extra):
    tmpl = {"name": "probe", "inputs": {"parameters": [{"name": "token", "value": "t"}]},
            "http": dict(CLEAN) if http is None else http, **extra}
    if outputs is not None:
        tmpl["outputs"] = {"parameters": outputs}
    return {"entrypoint": "probe",
            "arguments": {"parameters": [{"name": "host", "value": "127.0.0.1:1"}]},
            "templates": [tmpl]}


def changed(**kv):
    http = dict(CLEAN)
    for k, v in kv.items():
        if v is None:
            http.pop(k, None)
        else:
            http[k] = v
    return spec(http)


def test_http_is_a_body_the_executor_runs():
    assert "http" in BODY_TYPES and "http" not in UNSUPPORTED_BODY_TYPES


def test_a_clean_template_has_no_problems():
    assert validate_workflow_spec(spec()) == []
    assert validate_workflow_spec(spec({"url": "https://example.test/"})) == []
    assert validate_workflow_spec(spec(outputs=[
        {"name": "depth", "valueFrom": {"expression": 'jsonpath(response.body, "$.depth")',
                                        "default": "0"}},
        {"name": "code", "valueFrom": {"expression": "string(response.statusCode)"}},
        {"name": "fixed", "value": "v"},
    ])) == []
    # an expression that is put together at run time is judged then
    assert validate_workflow_spec(changed(
        successCondition="response.statusCode == {{inputs.parameters.token}}")) == []


@pytest.mark.parametrize("bad,needles", [
    (changed(url=None), ["http.url", "non-empty string"]),
    (changed(url=""), ["http.url", "non-empty string"]),
    (changed(url=8080), ["http.url", "non-empty string"]),
    (changed(method="FETCH"), ["http.method", "'FETCH'", "GET, HEAD, POST"]),
    (changed(method="get"), ["http.method", "'get'"]),
    (changed(headers=[{"name": "Authorization",
                       "valueFrom": {"secretKeyRef": {"name": "s", "key": "k"}}}]),
     ["'Authorization'", "valueFrom", "secret references have no local equivalent"]),
    (changed(headers={"Accept": "text/plain"}), ["http.headers", "not a list"]),
    (changed(headers=[{"name": "Accept"}]), ["http.headers", "{name, value}"]),
    (changed(headers=[{"name": "Accept", "value": 1}]), ["http.headers", "{name, value}"]),
    (changed(bodyFrom={"bytes": "aGk="}), ["http.bodyFrom", "not supported"]),
    (changed(body={"k": 1}), ["http.body", "string"]),
    (changed(timeoutSeconds=0), ["http.timeoutSeconds", "positive integer"]),
    (changed(timeoutSeconds="2"), ["http.timeoutSeconds", "positive integer"]),
    (changed(timeoutSeconds=True), ["http.timeoutSeconds", "positive integer"]),
    (changed(insecureSkipVerify="yes"), ["http.insecureSkipVerify"]),
    (changed(successCondition="response.statusCode == "),
     ["invalid successCondition", "offset 23"]),
    (changed(successCondition="response.statusCode = 200"),
     ["invalid successCondition", "offset 20"]),
    (changed(successCondition=""), ["successCondition", "non-empty string"]),
    (changed(successCondition="sha256(response.body) == 'x'"),
     ["successCondition", "unknown function 'sha256'"]),
    (changed(successCondition="__import__('os') == nil"),
     ["successCondition", "unknown function '__import__'"]),
    (changed(successCondition="response.status == 200"),
     ["successCondition", "unknown name 'response.status'"]),
    (changed(successCondition="response.duration < 2"),
     ["successCondition", "unknown name 'response.duration'"]),
    (changed(successCondition="status == 200"), ["successCondition", "unknown name 'status'"]),
    (changed(successCondition="response.statusCode == {{inputs.parameters.nope}}"),
     ["{{inputs.parameters.nope}}", "undeclared input parameter"]),
    (changed(url="http://{{workflow.parameters.nope}}/"),
     ["{{workflow.parameters.nope}}", "undeclared workflow parameter"]),
    (spec(outputs=[{"name": "d", "valueFrom": {"expression": "jsonpath(response.body"}}]),
     ["outputs.parameters.d", "invalid", "offset"]),
    (spec(outputs=[{"name": "d", "valueFrom": {"expression": "first(response.body)"}}]),
     ["outputs.parameters.d", "unknown function 'first'"]),
    (spec("http://127.0.0.1/"), ["http is not a map"]),
    (spec(container={"command": ["true"]}), ["several bodies", "container, http"]),
])
def test_each_mistake_is_one_problem(bad, needles):
    problems = validate_workflow_spec(bad)
    assert len(problems) == 1, problems
    assert problems[0].startswith("template 'probe': ")
    for needle in needles:
        assert needle in problems[0], problems[0]


def test_resource_templates_stay_unsupported():
    problems = validate_workflow_spec({"entrypoint": "k8s", "templates": [
        {"name": "k8s", "resource": {"action": "create", "manifest": "kind: ConfigMap"}}]})
    assert problems == ["template 'k8s': resource templates are not supported"]

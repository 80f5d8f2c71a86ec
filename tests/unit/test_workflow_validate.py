"""validate_workflow_spec: static problems are found before any process
starts, and every shipped example is clean."""
import pathlib

import pytest
import yaml

from active_monitor_amd.api import HealthCheck
from active_monitor_amd.engine.parse import (
    parse_remedy_workflow_from_healthcheck,
    parse_workflow_from_healthcheck,
)
from active_monitor_amd.workflow import validate_workflow_spec

OK = {"name": "ok", "container": {"command": ["true"]}}


def dag(tasks, **extra):
    return {
        "entrypoint": "main",
        "templates": [{"name": "main", "dag": {"tasks": tasks, **extra}}, OK],
    }


def test_clean_spec_has_no_problems():
    spec = {
        "entrypoint": "main",
        "onExit": "bye",
        "arguments": {"parameters": [{"name": "site", "value": "x"}]},
        "templates": [
            {"name": "main", "dag": {"tasks": [
                {"name": "a", "template": "echo",
                 "arguments": {"parameters": [{"name": "m", "value": "{{workflow.parameters.site}}"}]}},
                {"name": "b", "template": "echo", "dependencies": ["a"],
                 "arguments": {"parameters": [{"name": "m", "value": "{{tasks.a.outputs.result}}"}]}},
                {"name": "c", "template": "echo", "depends": "a && b", "withItems": [1, 2],
                 "arguments": {"parameters": [{"name": "m", "value": "{{ item }}"}]}},
            ]}},
            {"name": "echo", "inputs": {"parameters": [{"name": "m"}]},
             "retryStrategy": {"limit": 1},
             "container": {"command": ["echo", "{{inputs.parameters.m}}", "{{retries}}"]}},
            {"name": "bye", "steps": [[
                {"name": "s", "template": "echo", "when": "{{workflow.status}} == Failed",
                 "arguments": {"parameters": [{"name": "m", "value": "{{workflow.name}}"}]}},
            ]]},
        ],
    }
    assert validate_workflow_spec(spec) == []


def test_cycle_names_a_task():
    problems = validate_workflow_spec(dag([
        {"name": "first", "template": "ok"},
        {"name": "ping", "template": "ok", "dependencies": ["first", "pong"]},
        {"name": "pong", "template": "ok", "dependencies": ["ping"]},
    ]))
    assert len(problems) == 1
    assert "cycle" in problems[0]
    assert "'ping'" in problems[0] or "'pong'" in problems[0]


def test_self_dependency_is_a_cycle():
    problems = validate_workflow_spec(dag([
        {"name": "loop", "template": "ok", "dependencies": ["loop"]},
    ]))
    assert any("cycle" in p and "'loop'" in p for p in problems)


def test_unknown_dependency_names_task_and_dependency():
    problems = validate_workflow_spec(dag([
        {"name": "a", "template": "ok", "dependencies": ["ghost"]},
    ]))
    assert len(problems) == 1
    assert "'a'" in problems[0] and "'ghost'" in problems[0]


def test_duplicate_task():
    problems = validate_workflow_spec(dag([
        {"name": "twin", "template": "ok"},
        {"name": "twin", "template": "ok"},
    ]))
    assert any("'twin'" in p and "more than once" in p for p in problems)


def test_unknown_template_in_task_and_step():
    problems = validate_workflow_spec(dag([{"name": "a", "template": "nowhere"}]))
    assert any("'a'" in p and "'nowhere'" in p for p in problems)
    problems = validate_workflow_spec({
        "entrypoint": "main",
        "templates": [{"name": "main", "steps": [[{"name": "s", "template": "nowhere"}]]}],
    })
    assert any("'s'" in p and "'nowhere'" in p for p in problems)


def test_missing_entrypoint_and_on_exit():
    assert validate_workflow_spec({"entrypoint": "nope", "templates": []}) == [
        "entrypoint 'nope' not found"
    ]
    problems = validate_workflow_spec({"entrypoint": "ok", "onExit": "gone", "templates": [OK]})
    assert problems == ["onExit template 'gone' not found"]


def test_undeclared_input_and_workflow_parameters():
    problems = validate_workflow_spec({
        "entrypoint": "main",
        "templates": [{
            "name": "main",
            "inputs": {"parameters": [{"name": "declared", "default": "d"}]},
            "container": {"command": [
                "echo", "{{inputs.parameters.declared}}", "{{inputs.parameters.typo}}",
                "{{workflow.parameters.unset}}",
            ]},
        }],
    })
    assert len(problems) == 2
    assert "{{inputs.parameters.typo}}" in problems[0] and "undeclared" in problems[0]
    assert "{{workflow.parameters.unset}}" in problems[1] and "undeclared" in problems[1]


@pytest.mark.parametrize("expr", ["a.Failed", "a || b", "!a", "(a && b)", "a.Succeeded && b"])
def test_unsupported_depends(expr):
    problems = validate_workflow_spec(dag([
        {"name": "a", "template": "ok"},
        {"name": "b", "template": "ok"},
        {"name": "c", "template": "ok", "depends": expr},
    ]))
    assert len(problems) == 1
    assert "'c'" in problems[0] and "depends" in problems[0]


def test_template_bodies():
    problems = validate_workflow_spec({
        "entrypoint": "none",
        "templates": [
            {"name": "none"},
            {"name": "both", "container": {"command": ["true"]}, "script": {"source": ""}},
            {"name": "k8s", "resource": {"action": "create"}},
        ],
    })
    assert any("'none'" in p and "no body" in p for p in problems)
    assert any("'both'" in p and "several" in p for p in problems)
    assert any("'k8s'" in p and "not supported" in p for p in problems)


def test_unknown_namespace_and_expression_tags():
    problems = validate_workflow_spec({
        "entrypoint": "main",
        "templates": [{"name": "main", "container": {
            "command": ["echo", "{{pod.name}}", "{{=1+1}}", "{{.GoTemplate}}"],
        }}],
    })
    assert any("{{pod.name}}" in p and "namespace" in p for p in problems)
    assert any("{{=" in p for p in problems)
    assert len(problems) == 2


def test_item_only_inside_a_looping_step_or_task():
    def spec(step, leaf_arg="{{inputs.parameters.m}}"):
        return {
            "entrypoint": "main",
            "templates": [
                {"name": "main", "steps": [[{"name": "s", "template": "echo", **step}]]},
                {"name": "echo", "inputs": {"parameters": [{"name": "m", "default": "d"}]},
                 "container": {"command": ["echo", leaf_arg]}},
            ],
        }

    use_item = {"arguments": {"parameters": [{"name": "m", "value": "{{item.host}}"}]}}
    assert validate_workflow_spec(spec({**use_item, "withItems": [{"host": "a"}]})) == []
    assert validate_workflow_spec(spec({**use_item, "withParam": '[{"host": "a"}]'})) == []
    problems = validate_workflow_spec(spec(use_item))
    assert len(problems) == 1
    assert "'s'" in problems[0] and "{{item.host}}" in problems[0] and "withItems" in problems[0]
    # inside the called template's body no loop reaches {{item}}
    problems = validate_workflow_spec(spec({"withItems": [1]}, leaf_arg="{{item}}"))
    assert len(problems) == 1
    assert "'echo'" in problems[0] and "{{item}}" in problems[0]


def _example_specs():
    root = pathlib.Path(__file__).parents[2] / "examples"
    for path in sorted(root.rglob("*.yaml")):
        hc = HealthCheck.from_dict(yaml.safe_load(path.read_text()))
        rel = str(path.relative_to(root))
        wf = hc.spec.workflow
        if wf.resource is not None and wf.resource.source.inline is not None:
            yield pytest.param(parse_workflow_from_healthcheck(hc)[0], id=rel)
        remedy = hc.spec.remedy_workflow
        if (not remedy.is_empty() and remedy.resource is not None
                and remedy.resource.source.inline is not None):
            yield pytest.param(parse_remedy_workflow_from_healthcheck(hc)[0], id=rel + ":remedy")


@pytest.mark.parametrize("spec", list(_example_specs()))
def test_every_inline_example_validates_clean(spec):
    assert validate_workflow_spec(spec) == []


def test_new_examples_are_among_those_checked():
    ids = {p.id for p in _example_specs()}
    assert {"inline-loops.yaml", "inline-dag.yaml", "remedy/exit-handler.yaml:remedy"} <= ids

"""``withSequence``: the pure expansion, the loop it makes in the executor,
what lint says of it, and the example that uses it."""
import os
import pathlib
import subprocess
import sys

import pytest
import yaml

from active_monitor_amd.workflow.executor import WorkflowRun
from active_monitor_amd.workflow.template import (
    SEQUENCE_MAX_ITEMS,
    TemplateError,
    expand_sequence,
)
from active_monitor_amd.workflow.validate import validate_workflow_spec

REPO = pathlib.Path(__file__).parents[2]
EXAMPLE = REPO / "examples" / "inline-step-deadline.yaml"


@pytest.mark.parametrize("seq, items", [
    ({"count": 3}, "0 1 2"),
    ({"count": 3, "start": 5}, "5 6 7"),
    ({"start": 1, "end": 3}, "1 2 3"),
    ({"start": 3, "end": 1}, "3 2 1"),
    ({"end": 2}, "0 1 2"),
    ({"end": -2}, "0 -1 -2"),
    ({"start": 4, "end": 4}, "4"),
    ({"count": 0}, ""),
    ({"count": "2"}, "0 1"),
    ({"count": "2", "start": "-1"}, "-1 0"),
    ({"count": 2, "format": "%02d"}, "00 01"),
    ({"count": 2, "format": "probe-%d"}, "probe-0 probe-1"),
    ({"start": 10, "count": 2, "format": "%X"}, "A B"),
    ({"start": 10, "count": 2, "format": "%x"}, "a b"),
    ({"start": 255, "count": 1, "format": "0x%04X;"}, "0x00FF;"),
    ({"start": 8, "count": 2, "format": "%o"}, "10 11"),
    ({"count": SEQUENCE_MAX_ITEMS, "format": "%05d"},
     " ".join(f"{i:05d}" for i in range(SEQUENCE_MAX_ITEMS))),
])
def test_expansion(seq, items):
    assert expand_sequence(seq) == items.split()


def test_references_are_resolved_in_the_scope():
    scope = {"workflow.parameters.n": "2", "inputs.parameters.fmt": "%02d"}
    assert expand_sequence({"count": "{{workflow.parameters.n}}",
                            "format": "{{inputs.parameters.fmt}}"}, scope) == ["00", "01"]
    with pytest.raises(TemplateError, match="failed to resolve"):
        expand_sequence({"count": "{{workflow.parameters.n}}"})


@pytest.mark.parametrize("seq, message", [
    ({"count": 1, "end": 2}, "count or end, not both"),
    ({}, "needs count or end"),
    ({"start": 2}, "needs count or end"),
    ({"count": -1}, "negative"),
    ({"count": "x"}, "withSequence.count 'x' is not an integer"),
    ({"count": 1.5}, "not an integer"),
    ({"count": True}, "not an integer"),
    ({"count": 1, "start": "1e3"}, "withSequence.start '1e3' is not an integer"),
    ({"count": 1, "format": "%s"}, "withSequence.format '%s'"),
    ({"count": 1, "format": "%d-%d"}, "withSequence.format"),
    ({"count": 1, "format": "%(x)d"}, "withSequence.format"),
    ({"count": 1, "format": "%*d"}, "withSequence.format"),
    ({"count": 1, "format": "plain"}, "withSequence.format"),
    ({"count": 1, "format": 7}, "withSequence.format"),
    ({"count": 1, "step": 2}, "withSequence.step is not supported"),
    (3, "withSequence is not a map"),
    ({"count": SEQUENCE_MAX_ITEMS + 1},
     "withSequence expands to 10001 items, more than the cap of 10000"),
    ({"start": 1, "end": -SEQUENCE_MAX_ITEMS}, "more than the cap of 10000"),
    ({"count": 10 ** 30}, "more than the cap of 10000"),
])
def test_expansion_errors(seq, message):
    with pytest.raises(TemplateError) as e:
        expand_sequence(seq)
    assert message in str(e.value)


def looping(seq, n="3"):
    return {"entrypoint": "main",
            "arguments": {"parameters": [{"name": "n", "value": n}]},
            "templates": [
                {"name": "main", "steps": [
                    [{"name": "probe", "template": "say", "withSequence": seq,
                      "arguments": {"parameters": [{"name": "i", "value": "{{item}}"}]}}],
                    [{"name": "after", "template": "say",
                      "arguments": {"parameters": [
                          {"name": "i", "value": "{{steps.probe.status}}"}]}}]]},
                {"name": "say", "inputs": {"parameters": [{"name": "i"}]},
                 "container": {"command": ["echo", "item {{inputs.parameters.i}}"]}}]}


def run_spec(run, spec):
    assert validate_workflow_spec(spec) == []
    wf_run = WorkflowRun(spec, "wf", "health")
    phase, message = run(wf_run.run_entrypoint(), timeout=30)
    return phase, message, wf_run.nodes


def test_the_engine_runs_one_node_per_item(run):
    phase, _, nodes = run_spec(run, looping({"count": "{{workflow.parameters.n}}"}))
    assert phase == "Succeeded"
    pods = {n["displayName"]: n["outputs"]["result"] for n in nodes.values()
            if n["type"] == "Pod"}
    assert pods == {"probe(0:0)": "item 0", "probe(1:1)": "item 1", "probe(2:2)": "item 2",
                    "after": "item Succeeded"}
    assert "wf[0].probe(1:1)" in nodes


def test_formatted_items_name_their_nodes(run):
    phase, _, nodes = run_spec(run, looping({"start": 9, "end": 10, "format": "n-%02d"}))
    assert phase == "Succeeded"
    assert nodes["wf[0].probe(0:n-09)"]["outputs"]["result"] == "item n-09"
    assert nodes["wf[0].probe(1:n-10)"]["outputs"]["result"] == "item n-10"


def test_an_empty_sequence_succeeds(run):
    phase, _, nodes = run_spec(run, looping({"count": "{{workflow.parameters.n}}"}, n="0"))
    assert phase == "Succeeded"
    assert [n["displayName"] for n in nodes.values() if n["type"] == "Pod"] == ["after"]


def test_a_bad_sequence_fails_the_call(run):
    phase, message, nodes = run_spec(run, looping({"count": "{{workflow.parameters.n}}"}, n="many"))
    assert phase == "Failed"
    assert message == "withSequence.count 'many' is not an integer"
    assert nodes["wf[0].probe"]["phase"] == "Failed"

    phase, message, _ = run_spec(run, looping({"count": "{{workflow.parameters.n}}"}, n="10001"))
    assert phase == "Failed" and f"cap of {SEQUENCE_MAX_ITEMS}" in message


def test_lint():
    assert validate_workflow_spec(looping({"count": 3})) == []  # {{item}} is allowed there
    where = "template 'main': step 'probe': "

    both = looping({"count": 3})
    both["templates"][0]["steps"][0][0]["withItems"] = [1, 2]
    assert validate_workflow_spec(both) == [
        where + "withItems and withSequence are mutually exclusive"]
    assert validate_workflow_spec(looping(3)) == [where + "withSequence is not a map"]
    assert validate_workflow_spec(looping({"count": 1, "end": 2})) == [
        where + "withSequence takes count or end, not both"]
    assert validate_workflow_spec(looping({"count": "{{workflow.parameters.n}}", "end": 2})) == [
        where + "withSequence takes count or end, not both"]
    assert validate_workflow_spec(looping({"count": 2, "format": "%s"}))[0].startswith(
        where + "withSequence.format '%s'")
    assert validate_workflow_spec(looping({"count": "{{workflow.parameters.missing}}"})) == [
        where + "{{workflow.parameters.missing}} refers to an undeclared workflow parameter"]

    outside = looping({"count": 3})
    del outside["templates"][0]["steps"][0][0]["withSequence"]
    (problem,) = validate_workflow_spec(outside)
    assert problem == (where + "{{item}} is only available in a step or task "
                       "with withItems or withParam")  # the text other tests pin


def test_the_example_validates():
    doc = yaml.safe_load(EXAMPLE.read_text())
    inline = yaml.safe_load(doc["spec"]["workflow"]["resource"]["source"]["inline"])
    assert validate_workflow_spec(inline["spec"]) == []
    text = yaml.safe_dump(inline)
    for field in ("activeDeadlineSeconds", "retryStrategy", "continueOn", "withSequence"):
        assert field in text


def test_the_example_runs_through_the_command_line():
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-m", "active_monitor_amd.workflow", "run", str(EXAMPLE)],
        capture_output=True, text=True, timeout=60, cwd=str(REPO), env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "phase: Succeeded" in out.stdout
    rows = {line.split()[0]: line for line in out.stdout.splitlines() if line.strip()}
    assert "Pod was active on the node longer than the specified deadline" in rows["probe(0)"]
    assert "Succeeded" in rows["diagnose"]
    assert "Succeeded" in rows["sample(2:2)"]

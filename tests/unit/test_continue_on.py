"""``continueOn: {failed: true}`` on steps and DAG tasks: the failed call
keeps its ``Failed`` nodes and status, publishes nothing, and its caller goes
on as if it had succeeded."""
import pytest

from active_monitor_amd.workflow.executor import WorkflowRun
from active_monitor_amd.workflow.validate import validate_workflow_spec

CONTINUE = {"failed": True}


def sh(name, script, **fields):
    return {"name": name, "container": {"command": ["sh", "-c", script]}, **fields}


def run_spec(run, spec):
    """``(phase, message, nodes by display name)`` of one validated run."""
    assert validate_workflow_spec(spec) == []
    wf_run = WorkflowRun(spec, "wf", "health")
    phase, message = run(wf_run.run_entrypoint(), timeout=30)
    return phase, message, {n["displayName"]: n for n in wf_run.nodes.values()}


def probe_then_report(**probe):
    return {"entrypoint": "main", "templates": [
        {"name": "main", "steps": [
            [{"name": "probe", "template": "bad", **probe}],
            [{"name": "report", "template": "say",
              "when": "{{steps.probe.status}} == Failed"}]]},
        sh("bad", "echo broken >&2; exit 3"),
        sh("say", "echo diagnostics")]}


def test_steps_go_on_past_a_continued_failure(run):
    phase, message, nodes = run_spec(run, probe_then_report(continueOn=CONTINUE))
    assert (phase, message) == ("Succeeded", "")
    assert nodes["probe"]["phase"] == "Failed"
    assert nodes["probe"]["message"].startswith("exit code 3: broken")
    assert "outputs" not in nodes["probe"]
    assert nodes["[0]"]["phase"] == "Succeeded" and nodes["[0]"]["message"] == ""
    assert nodes["report"]["phase"] == "Succeeded"
    assert nodes["report"]["outputs"]["result"] == "diagnostics"
    assert nodes["wf"]["phase"] == "Succeeded"


@pytest.mark.parametrize("probe", [{}, {"continueOn": {"error": True}},
                                   {"continueOn": {"failed": False}}])
def test_without_it_the_failure_fails_the_workflow(run, probe):
    """Control for ``{}``: that case passes without the feature too."""
    phase, message, nodes = run_spec(run, probe_then_report(**probe))
    assert phase == "Failed" and message.startswith("exit code 3")
    assert nodes["[0]"]["phase"] == "Failed"
    assert "report" not in nodes and "[1]" not in nodes


@pytest.mark.parametrize("parallelism", [None, 1])
def test_a_dag_that_fails_fast_goes_on_past_it(run, parallelism):
    """``a`` fails and is continued past: ``b``, which depends on it, starts,
    and ``c``, independent and slower, is neither cancelled nor, under
    ``parallelism: 1``, left ``Omitted`` by the latch of the DAG's bound."""
    main = {"name": "main", "dag": {"tasks": [
        {"name": "a", "template": "bad", "continueOn": CONTINUE},
        {"name": "b", "template": "say", "dependencies": ["a"],
         "arguments": {"parameters": [{"name": "was", "value": "{{tasks.a.status}}"}]}},
        {"name": "c", "template": "slow"}]}}
    if parallelism is not None:
        main["parallelism"] = parallelism
    spec = {"entrypoint": "main", "templates": [
        main, sh("bad", "exit 1"), sh("slow", "sleep 0.3; echo done"),
        sh("say", "echo a was {{inputs.parameters.was}}",
           inputs={"parameters": [{"name": "was"}]})]}
    phase, message, nodes = run_spec(run, spec)
    assert (phase, message) == ("Succeeded", "")
    assert {name: nodes[name]["phase"] for name in "abc"} == {
        "a": "Failed", "b": "Succeeded", "c": "Succeeded"}
    assert nodes["b"]["outputs"]["result"] == "a was Failed"
    assert nodes["c"]["outputs"]["result"] == "done"
    assert not [n for n in nodes.values() if n["phase"] == "Omitted"]


def test_a_dag_failure_that_is_not_continued_still_omits(run):
    """Control: passes without the feature too."""
    spec = {"entrypoint": "main", "templates": [
        {"name": "main", "dag": {"tasks": [
            {"name": "a", "template": "bad"},
            {"name": "b", "template": "bad", "dependencies": ["a"]}]}},
        sh("bad", "exit 1")]}
    phase, _, nodes = run_spec(run, spec)
    assert phase == "Failed"
    assert nodes["b"]["phase"] == "Omitted"


def test_a_loop_is_judged_after_all_of_its_items(run):
    spec = {"entrypoint": "main", "templates": [
        {"name": "main", "parallelism": 1, "steps": [
            [{"name": "each", "template": "judge", "withItems": ["ok", "bad", "ok"],
              "continueOn": CONTINUE,
              "arguments": {"parameters": [{"name": "v", "value": "{{item}}"}]}}],
            [{"name": "after", "template": "say",
              "arguments": {"parameters": [{"name": "v", "value": "{{steps.each.status}}"}]}}]]},
        sh("judge", "test {{inputs.parameters.v}} = ok", inputs={"parameters": [{"name": "v"}]}),
        sh("say", "echo {{inputs.parameters.v}}", inputs={"parameters": [{"name": "v"}]})]}
    phase, _, nodes = run_spec(run, spec)
    assert phase == "Succeeded"
    items = {name: n["phase"] for name, n in nodes.items() if name.startswith("each(")}
    assert items == {"each(0:ok)": "Succeeded", "each(1:bad)": "Failed",
                     "each(2:ok)": "Succeeded"}
    assert nodes["after"]["outputs"]["result"] == "Failed"


def test_retries_come_first(run):
    spec = probe_then_report(continueOn=CONTINUE)
    spec["templates"][1]["retryStrategy"] = {"limit": 1}
    phase, _, nodes = run_spec(run, spec)
    assert phase == "Succeeded"
    assert nodes["probe"]["type"] == "Retry" and nodes["probe"]["phase"] == "Failed"
    assert nodes["probe(0)"]["phase"] == nodes["probe(1)"]["phase"] == "Failed"
    assert "probe(2)" not in nodes
    assert nodes["report"]["phase"] == "Succeeded"


def test_a_continued_failure_publishes_no_outputs(run):
    spec = {"entrypoint": "main", "templates": [
        {"name": "main", "steps": [
            [{"name": "probe", "template": "bad", "continueOn": CONTINUE}],
            [{"name": "read", "template": "say",
              "arguments": {"parameters": [
                  {"name": "v", "value": "{{steps.probe.outputs.result}}"}]}}]]},
        sh("bad", "echo half; exit 1"),
        sh("say", "echo {{inputs.parameters.v}}", inputs={"parameters": [{"name": "v"}]})]}
    phase, message, nodes = run_spec(run, spec)
    assert phase == "Failed"
    assert message == "failed to resolve {{steps.probe.outputs.result}}"
    assert nodes["read"]["phase"] == "Failed" and nodes["read"]["message"] == message


def test_a_continued_step_deadline(run):
    """The two halves together: the hung probe is cut and the check goes on."""
    spec = probe_then_report(continueOn=CONTINUE)
    spec["templates"][1] = sh("bad", "sleep 30", timeout="1s")
    phase, _, nodes = run_spec(run, spec)
    assert phase == "Succeeded"
    assert nodes["probe"]["message"] == "Step exceeded its deadline"
    assert nodes["report"]["phase"] == "Succeeded"


def with_continue_on(value):
    return probe_then_report(continueOn=value)


@pytest.mark.parametrize("value, problem", [
    (True, "continueOn is not a map"),
    ({"failed": "yes"}, "continueOn.failed must be true or false"),
    ({"sometimes": True}, "continueOn.sometimes is not supported (failed, error)"),
])
def test_lint_names_a_bad_continue_on(value, problem):
    assert validate_workflow_spec(with_continue_on(value)) == [
        f"template 'main': step 'probe': {problem}"]


def test_lint_accepts_both_keys():
    assert validate_workflow_spec(with_continue_on({"failed": True, "error": True})) == []

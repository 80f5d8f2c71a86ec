"""``python -m active_monitor_amd.workflow`` with template documents: ``lint``
and ``run`` on the shared-template sample, ``--templates``, and problems that
name the scope they are in."""
import pathlib

import yaml

from active_monitor_amd.workflow.__main__ import main

REPO = pathlib.Path(__file__).parents[2]
SAMPLE = REPO / "config" / "samples" / "activemonitor_v1alpha1_healthcheck_workflowtemplate.yaml"


def split_sample(tmp_path):
    """The sample's HealthChecks in one file, its template in a directory."""
    docs = list(yaml.safe_load_all(SAMPLE.read_text()))
    checks = tmp_path / "checks.yaml"
    checks.write_text(yaml.safe_dump_all([d for d in docs if d["kind"] == "HealthCheck"]))
    library = tmp_path / "library"
    library.mkdir()
    (library / "net-checks.yaml").write_text(
        yaml.safe_dump_all([d for d in docs if d["kind"] == "WorkflowTemplate"]))
    (library / "README.txt").write_text("not YAML: {")
    return checks, library


def test_the_sample_holds_what_it_should():
    docs = list(yaml.safe_load_all(SAMPLE.read_text()))
    assert [d["kind"] for d in docs] == ["WorkflowTemplate", "HealthCheck", "HealthCheck"]
    inline = [yaml.safe_load(d["spec"]["workflow"]["resource"]["source"]["inline"])["spec"]
              for d in docs[1:]]
    assert inline[0]["workflowTemplateRef"] == {"name": "net-checks"}
    assert inline[0]["arguments"]["parameters"]
    tasks = inline[1]["templates"][0]["dag"]["tasks"]
    assert {t["templateRef"]["template"] for t in tasks} == {"probe", "report"}


def test_lint_accepts_the_sample(capsys):
    assert main(["lint", str(SAMPLE)]) == 0
    assert capsys.readouterr().out == "ok\n"


def test_lint_names_a_template_that_is_not_given(tmp_path, capsys):
    checks, library = split_sample(tmp_path)
    assert main(["lint", str(checks)]) == 1
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4  # the workflowTemplateRef, and three tasks
    assert all('workflowtemplates.argoproj.io "net-checks" not found' in line
               for line in lines)
    assert lines[0].startswith(f"{checks}[0] (workflow): spec.workflowTemplateRef: ")

    assert main(["lint", str(checks), "--templates", str(library)]) == 0
    assert capsys.readouterr().out == "ok\n"
    assert main(["lint", str(checks), "--templates",
                 str(library / "net-checks.yaml")]) == 0
    capsys.readouterr()


def test_lint_checks_a_template_document_as_a_library(tmp_path, capsys):
    doc = {"apiVersion": "argoproj.io/v1alpha1", "kind": "ClusterWorkflowTemplate",
           "metadata": {"name": "loops"},
           "spec": {"templates": [  # no entrypoint, no arguments
               {"name": "ring", "dag": {"tasks": [
                   {"name": "a", "template": "leaf", "dependencies": ["b"]},
                   {"name": "b", "template": "leaf", "dependencies": ["a"]}]}},
               {"name": "leaf",
                "container": {"command": ["echo", "{{workflow.parameters.anything}}"]}},
               {"name": "far", "steps": [[
                   {"name": "s", "templateRef": {"name": "nowhere", "template": "t"}}]]},
           ]}}
    path = tmp_path / "loops.yaml"
    path.write_text(yaml.safe_dump(doc))
    assert main(["lint", str(path)]) == 1
    out = capsys.readouterr().out.splitlines()
    assert out == [f"{path}: template 'far' of ClusterWorkflowTemplate 'loops': step 's': "
                   'workflowtemplates.argoproj.io "nowhere" not found']

    del doc["spec"]["templates"][2]
    path.write_text(yaml.safe_dump(doc))
    assert main(["lint", str(path)]) == 1
    out = capsys.readouterr().out.splitlines()
    assert out == [f"{path}: template 'ring' of ClusterWorkflowTemplate 'loops': "
                   "dependency cycle through task 'a'"]


def test_lint_still_refuses_other_kinds(tmp_path, capsys):
    path = tmp_path / "cm.yaml"
    path.write_text("kind: ConfigMap\n")
    assert main(["lint", str(path)]) == 1
    assert "expected kind Workflow, HealthCheck, WorkflowTemplate" in capsys.readouterr().out


def test_run_executes_the_first_check_of_the_sample(capsys):
    assert main(["run", str(SAMPLE)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "phase: Succeeded"
    assert out[1].split() == ["NODE", "TYPE", "PHASE", "MESSAGE"]
    assert [line.split()[:3] for line in out[2:]] == [
        ["run", "Steps", "Succeeded"], ["[0]", "StepGroup", "Succeeded"],
        ["probe", "Pod", "Succeeded"], ["[1]", "StepGroup", "Succeeded"],
        ["report", "Pod", "Succeeded"]]


def test_run_takes_templates_from_elsewhere(tmp_path, capsys):
    checks, library = split_sample(tmp_path)
    assert main(["run", str(checks)]) == 1
    assert 'message: workflowtemplates.argoproj.io "net-checks" not found' in \
        capsys.readouterr().out
    assert main(["run", str(checks), "--templates", str(library), "--logs",
                 "-p", "target=rack-9"]) == 0
    assert "default: probed rack-9" in capsys.readouterr().out.splitlines()

"""The Argo-surface examples through the full controller loop (Manager +
LocalWorkflowEngine over the in-memory apiserver), and the offline
``python -m active_monitor_amd.workflow`` entry point."""
import asyncio
import os
import pathlib
import subprocess
import sys
import time

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.workflow import LocalWorkflowEngine

REPO = pathlib.Path(__file__).parents[2]
EXAMPLES = REPO / "examples"


async def run_example(relpath, done, timeout=30.0):
    """Apply one example unchanged and poll its status until ``done(status)``;
    returns ``(status, workflows)``."""
    doc = yaml.safe_load((EXAMPLES / relpath).read_text())
    client = MemoryClient(MemoryApiServer())
    engine = LocalWorkflowEngine(client, ttl_seconds=None)
    await engine.start()
    manager = Manager(client, max_workers=2)
    await manager.start()
    try:
        await client.create(doc)
        meta = doc["metadata"]
        deadline = time.monotonic() + timeout
        status = {}
        while time.monotonic() < deadline:
            obj = await client.get(API_VERSION, "HealthCheck", meta["namespace"], meta["name"])
            status = obj.get("status") or {}
            if done(status):
                break
            await asyncio.sleep(0.02)
        else:
            raise AssertionError(f"{relpath}: not done within {timeout}s: {status}")
        workflows = await client.list("argoproj.io/v1alpha1", "Workflow", meta["namespace"])
        return status, workflows
    finally:
        await manager.stop()
        await engine.stop()


def node_names(wf, type_=None):
    return sorted(
        n["displayName"] for n in wf["status"]["nodes"].values()
        if type_ is None or n["type"] == type_
    )


def test_loops_example_full_loop(run):
    status, workflows = run(run_example(
        "inline-loops.yaml", lambda st: st.get("successCount", 0) >= 1))
    assert status.get("failedCount", 0) == 0
    assert node_names(workflows[0], "Pod") == [
        "directory(0:/)", "directory(1:/tmp)", "directory(2:/etc)",
        "threshold(0)", "threshold(1)",
    ]


def test_dag_example_full_loop(run):
    status, workflows = run(run_example(
        "inline-dag.yaml", lambda st: st.get("successCount", 0) >= 1))
    assert status.get("failedCount", 0) == 0
    nodes = workflows[0]["status"]["nodes"].values()
    assert node_names(workflows[0], "Pod") == ["high", "low", "report", "sample"]
    assert next(n for n in nodes if n["displayName"] == "sample")["outputs"]["result"] == "17"
    assert next(n for n in nodes if n["displayName"] == "report")["outputs"]["result"] == (
        "queue depth 17 is within bounds"
    )


def test_exit_handler_example_full_loop(run):
    status, workflows = run(run_example(
        "remedy/exit-handler.yaml",
        lambda st: st.get("failedCount", 0) >= 1 and st.get("remedySuccessCount", 0) >= 1,
    ))
    assert status.get("successCount", 0) == 0
    assert status.get("remedyFailedCount", 0) == 0
    remedy = next(w for w in workflows if "onExit" in w["spec"])
    by_name = {n["displayName"]: n for n in remedy["status"]["nodes"].values()}
    assert by_name["record"]["phase"] == "Succeeded"
    assert by_name["escalate"]["phase"] == "Skipped"


# -- command line -------------------------------------------------------------


def cli(*args):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(
        [sys.executable, "-m", "active_monitor_amd.workflow", *args],
        capture_output=True, text=True, timeout=60, cwd=str(REPO), env=env,
    )


def test_cli_lint_clean_example():
    out = cli("lint", "examples/inline-dag.yaml")
    assert out.returncode == 0, out.stdout + out.stderr


def test_cli_lint_cyclic_dag_names_the_task(tmp_path):
    bad = tmp_path / "cyclic.yaml"
    bad.write_text(yaml.safe_dump({
        "apiVersion": "argoproj.io/v1alpha1", "kind": "Workflow",
        "spec": {"entrypoint": "main", "templates": [
            {"name": "main", "dag": {"tasks": [
                {"name": "chicken", "template": "ok", "dependencies": ["egg"]},
                {"name": "egg", "template": "ok", "dependencies": ["chicken"]},
            ]}},
            {"name": "ok", "container": {"command": ["true"]}},
        ]},
    }))
    out = cli("lint", str(bad))
    assert out.returncode == 1, out.stdout + out.stderr
    assert "cycle" in out.stdout
    assert "chicken" in out.stdout or "egg" in out.stdout


def test_cli_run_failing_workflow_prints_the_failing_node(tmp_path):
    wf = tmp_path / "failing.yaml"
    wf.write_text(yaml.safe_dump({
        "apiVersion": "argoproj.io/v1alpha1", "kind": "Workflow",
        "spec": {"entrypoint": "main", "templates": [
            {"name": "main", "dag": {"tasks": [
                {"name": "fine", "template": "ok"},
                {"name": "broken", "template": "bad", "dependencies": ["fine"]},
            ]}},
            {"name": "ok", "container": {"command": ["true"]}},
            {"name": "bad", "container": {"command": ["sh", "-c", "echo {{workflow.parameters.why}} >&2; exit 3"]}},
        ], "arguments": {"parameters": [{"name": "why", "value": "default-reason"}]}},
    }))
    out = cli("run", str(wf), "-p", "why=disk-full")
    assert out.returncode == 1, out.stdout + out.stderr
    assert "phase: Failed" in out.stdout
    row = next(line for line in out.stdout.splitlines() if line.strip().startswith("broken"))
    assert "Failed" in row and "exit code 3" in row and "disk-full" in row
    fine = next(line for line in out.stdout.splitlines() if line.strip().startswith("fine"))
    assert "Succeeded" in fine


def test_cli_in_process_lint_and_run(tmp_path, capsys):
    """The same entry point called as a function: every shipped example
    lints clean; unreadable input and unknown kinds are problems, not
    tracebacks; ``run`` reports a validation failure as a failed workflow."""
    from active_monitor_amd.workflow.__main__ import main

    shipped = [str(p) for p in sorted(EXAMPLES.rglob("*.yaml"))]
    assert main(["lint", *shipped]) == 0
    assert capsys.readouterr().out.strip() == "ok"

    other = tmp_path / "other.yaml"
    other.write_text("kind: ConfigMap\n")
    broken = tmp_path / "broken.yaml"
    broken.write_text("kind: [unclosed\n")
    assert main(["lint", str(other), str(broken), str(tmp_path / "missing.yaml")]) == 1
    out = capsys.readouterr().out
    assert "ConfigMap" in out and "broken.yaml" in out and "missing.yaml" in out

    wf = tmp_path / "wf.yaml"
    wf.write_text(yaml.safe_dump({
        "kind": "Workflow",
        "spec": {"entrypoint": "main", "templates": [
            {"name": "main", "container": {"command": ["echo", "{{workflow.parameters.who}}"]}},
        ]},
    }))
    assert main(["run", str(wf)]) == 1
    out = capsys.readouterr().out
    assert "phase: Failed" in out and "undeclared workflow parameter" in out
    assert main(["run", str(wf), "-p", "who=operator"]) == 0
    out = capsys.readouterr().out
    assert "phase: Succeeded" in out and "Pod" in out
    assert main(["run", "--remedy", str(wf)]) == 1  # a bare Workflow has no remedy


@pytest.mark.parametrize("args", [
    ("examples/inline-loops.yaml",),
    ("examples/inline-dag.yaml",),
    ("--remedy", "examples/remedy/exit-handler.yaml"),
])
def test_cli_run_new_examples_succeed(args):
    out = cli("run", *args)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "phase: Succeeded" in out.stdout
    assert "NODE" in out.stdout and "Pod" in out.stdout

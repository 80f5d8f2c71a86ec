"""Bounds inside one workflow and over the engine's processes:
``spec.parallelism``, template ``parallelism``, ``max_processes``.

The peak of concurrently alive leaves is measured by the leaves themselves:
each makes a directory, counts the directories there are, and removes its
own after 0.3 s. Unbounded, six items show 6.
"""
import asyncio
import glob
import os
import time

import pytest

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine, validate_workflow_spec
from active_monitor_amd.workflow.__main__ import _specs

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WF = (WF_API_VERSION, WF_KIND)


def sh(script):
    return {"container": {"command": ["sh", "-c", script]}}


def peak_leaf(tmp, name="leaf"):
    return {"name": name, **sh(
        f"cd {tmp} && mkdir alive.$$; ls -d alive.* | wc -l >> peak; sleep 0.3; rmdir alive.$$")}


def peak(tmp):
    return max(int(line) for line in (tmp / "peak").read_text().split())


async def run_workflows(specs, timeout=20.0, **engine_options):
    """Run ``specs`` side by side on one engine; their final statuses, and
    the engine's stats once all have ended."""
    client = MemoryClient(MemoryApiServer())
    engine = LocalWorkflowEngine(client, ttl_seconds=None, **engine_options)
    await engine.start()
    try:
        for i, spec in enumerate(specs):
            await client.create({"apiVersion": WF_API_VERSION, "kind": WF_KIND,
                                 "metadata": {"name": f"wf{i}", "namespace": "health"},
                                 "spec": spec})
        deadline = time.monotonic() + timeout
        while time.monotonic() < deadline:
            statuses = [(wf.get("status") or {}) for wf in await client.list(*WF, "health")]
            if all(st.get("phase") in ("Succeeded", "Failed") for st in statuses):
                return statuses, engine.stats()
            await asyncio.sleep(0.02)
        raise AssertionError(f"workflows did not end: {statuses}")
    finally:
        await engine.stop()


def fan_out(tmp, ways, **spec_extra):
    return {"entrypoint": "main", **spec_extra, "templates": [
        {"name": "main", "steps": [[
            {"name": "each", "template": "leaf", "withItems": list(range(ways))}]]},
        peak_leaf(tmp),
    ]}


def test_spec_parallelism_bounds_the_items_of_a_loop(run, tmp_path):
    (st,), _ = run(run_workflows([fan_out(tmp_path, 6, parallelism=2)]))
    assert st["phase"] == "Succeeded", st.get("message")
    assert len((tmp_path / "peak").read_text().split()) == 6
    assert peak(tmp_path) == 2


def test_dag_template_parallelism_bounds_its_tasks(run, tmp_path):
    (st,), _ = run(run_workflows([{"entrypoint": "main", "templates": [
        {"name": "main", "parallelism": 1, "dag": {"tasks": [
            {"name": t, "template": "leaf"} for t in ("a", "b", "c")]}},
        peak_leaf(tmp_path),
    ]}]))
    assert st["phase"] == "Succeeded", st.get("message")
    assert len((tmp_path / "peak").read_text().split()) == 3
    assert peak(tmp_path) == 1


def test_template_parallelism_does_not_reach_into_a_nested_template(run, tmp_path):
    (st,), _ = run(run_workflows([{"entrypoint": "outer", "templates": [
        {"name": "outer", "parallelism": 1, "steps": [[
            {"name": "only", "template": "inner"}]]},
        {"name": "inner", "steps": [[
            {"name": "each", "template": "leaf", "withItems": [1, 2, 3]}]]},
        peak_leaf(tmp_path),
    ]}]))
    assert st["phase"] == "Succeeded", st.get("message")
    assert peak(tmp_path) == 3


def test_spec_parallelism_one_does_not_deadlock_nested_composites(run, tmp_path):
    spec = {"entrypoint": "d", "parallelism": 1, "templates": [
        {"name": "d", "dag": {"tasks": [{"name": "t", "template": "s"},
                                        {"name": "u", "template": "s"}]}},
        {"name": "s", "steps": [[{"name": "x", "template": "leaf"},
                                 {"name": "y", "template": "leaf"}]]},
        {"name": "leaf", **sh("true")},
    ]}

    async def go():
        return await asyncio.wait_for(run_workflows([spec]), 15)

    (st,), stats = run(go())
    assert st["phase"] == "Succeeded", st.get("message")
    assert stats["processes"] == 0


def test_a_task_in_retry_backoff_holds_no_slot(run, tmp_path):
    order = tmp_path / "order"
    (st,), _ = run(run_workflows([{"entrypoint": "main", "parallelism": 1, "templates": [
        {"name": "main", "dag": {"tasks": [{"name": "flaky", "template": "flaky"},
                                           {"name": "sibling", "template": "sibling"}]}},
        {"name": "flaky",
         "retryStrategy": {"limit": 1, "backoff": {"duration": "1s"}},
         **sh(f"echo flaky{{{{retries}}}} >> {order}; test {{{{retries}}}} -gt 0")},
        {"name": "sibling", **sh(f"echo sibling >> {order}")},
    ]}]))
    assert st["phase"] == "Succeeded", st.get("message")
    assert order.read_text().split() == ["flaky0", "sibling", "flaky1"]


def test_max_processes_bounds_the_leaves_of_all_workflows(run, tmp_path):
    statuses, stats = run(run_workflows([fan_out(tmp_path, 2) for _ in range(3)],
                                        max_processes=2))
    assert [st["phase"] for st in statuses] == ["Succeeded"] * 3
    assert len((tmp_path / "peak").read_text().split()) == 6
    assert peak(tmp_path) == 2
    assert stats["processes"] == 0
    assert stats["limits"]["max_processes"] == 2


def test_deadline_while_leaves_wait_for_a_slot_starts_nothing_more(run, tmp_path):
    marks = tmp_path / "started"
    spec = {"entrypoint": "main", "parallelism": 1, "activeDeadlineSeconds": 1, "templates": [
        {"name": "main", "steps": [[
            {"name": "each", "template": "leaf", "withItems": [1, 2, 3]}]]},
        {"name": "leaf", **sh(f"echo x >> {marks}; sleep 30")},
    ]}
    t0 = time.monotonic()
    (st,), stats = run(run_workflows([spec], max_processes=8))
    assert time.monotonic() - t0 < 10
    assert st["phase"] == "Failed"
    assert st["message"] == "deadline exceeded"
    assert stats["processes"] == 0
    assert marks.read_text().split() == ["x"]  # and none after the kill


def test_fail_fast_dag_does_not_start_a_task_that_waited_for_its_slot(run, tmp_path):
    marks = tmp_path / "started"
    (st,), _ = run(run_workflows([{"entrypoint": "main", "templates": [
        {"name": "main", "parallelism": 1, "dag": {"tasks": [
            {"name": "bad", "template": "bad"}, {"name": "late", "template": "late"}]}},
        {"name": "bad", **sh(f"echo bad >> {marks}; exit 1")},
        {"name": "late", **sh(f"echo late >> {marks}")},
    ]}]))
    assert st["phase"] == "Failed"
    assert marks.read_text().split() == ["bad"]
    assert st["nodes"]["wf0.late"]["phase"] == "Omitted"


def leaf_only(**spec_extra):
    return {"entrypoint": "x", **spec_extra,
            "templates": [{"name": "x", "container": {"command": ["true"]}}]}


@pytest.mark.parametrize("value", [0, "x", True, -1, 1.5])
def test_validator_wants_a_positive_integer_parallelism(value):
    assert validate_workflow_spec(leaf_only(parallelism=value)) == [
        "spec.parallelism must be a positive integer"]
    spec = leaf_only()
    spec["templates"][0]["parallelism"] = value
    assert validate_workflow_spec(spec) == [
        "template 'x': parallelism must be a positive integer"]


def test_validator_wants_an_integer_priority():
    assert validate_workflow_spec(leaf_only(priority="high")) == [
        "spec.priority must be an integer"]
    for fine in (0, -3, 7):
        assert validate_workflow_spec(leaf_only(priority=fine, parallelism=1)) == []


def test_the_documented_mutex_example_lints_clean(tmp_path):
    with open(os.path.join(REPO, "docs", "OPERATIONS.md")) as f:
        blocks = f.read().split("```yaml\n")[1:]
    (block,) = [b.split("```")[0] for b in blocks if "mutex: {name: gpu0}" in b]
    path = tmp_path / "exclusive-device.yaml"
    path.write_text(block)
    found = list(_specs(str(path)))
    assert len(found) == 2
    for label, spec, problems in found:
        assert problems == [], label
        assert validate_workflow_spec(spec) == [], label
        assert spec["synchronization"]


def test_every_example_still_validates_clean():
    paths = sorted(glob.glob(os.path.join(REPO, "examples", "**", "*.yaml"), recursive=True))
    assert paths
    for path in paths:
        for label, spec, problems in _specs(path):
            assert problems == [], label
            if spec is not None:
                assert validate_workflow_spec(spec) == [], label

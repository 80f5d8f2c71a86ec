"""LocalWorkflowEngine: parameters, loops, DAGs, ``when``, exit handlers,
retry backoff, node status and process-group cancellation. Every workflow is
a few ``sh`` / ``echo`` / ``true`` processes; files under ``tmp_path`` are the
observable side effects."""
import asyncio
import os
import time

import pytest

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine


async def run_workflow(spec, timeout=15.0, stop_when=None):
    """Same shape as test_local_engine.run_workflow. ``stop_when`` (a
    callable) makes it stop the engine as soon as it returns true instead of
    waiting for a terminal phase."""
    client = MemoryClient(MemoryApiServer())
    engine = LocalWorkflowEngine(client)
    await engine.start()
    await client.create({
        "apiVersion": WF_API_VERSION, "kind": WF_KIND,
        "metadata": {"name": "wf", "namespace": "health"},
        "spec": spec,
    })
    deadline = time.monotonic() + timeout
    wf = None
    while time.monotonic() < deadline:
        wf = await client.get(WF_API_VERSION, WF_KIND, "health", "wf")
        if (wf.get("status") or {}).get("phase") in ("Succeeded", "Failed"):
            break
        if stop_when is not None and stop_when():
            break
        await asyncio.sleep(0.02)
    await engine.stop()
    return wf["status"]


def sh(name, script, **extra):
    return {"name": name, "container": {"command": ["sh", "-c", script]}, **extra}


def param_args(**kv):
    return {"parameters": [{"name": k, "value": v} for k, v in kv.items()]}


def nodes_named(st, display):
    return [n for n in st["nodes"].values() if n["displayName"] == display]


def node(st, display):
    found = nodes_named(st, display)
    assert len(found) == 1, (display, sorted(n["displayName"] for n in st["nodes"].values()))
    return found[0]


def lines(path):
    return path.read_text().splitlines() if path.exists() else []


#: writes every argv element it receives on a line of its own
ARGV_DUMP = 'for a in "$@"; do printf "%s\\n" "$a"; done > "$OUT"'


# -- parameters ---------------------------------------------------------------


def test_argument_stays_one_argv_element(run, tmp_path):
    out = tmp_path / "argv"
    hostile = f"a b; touch {tmp_path}/pwned"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [[
                {"name": "s", "template": "dump", "arguments": param_args(x=hostile)},
            ]]},
            {"name": "dump", "inputs": {"parameters": [{"name": "x"}]},
             "container": {
                 "command": ["sh", "-c", ARGV_DUMP, "sh"],
                 "args": ["{{inputs.parameters.x}}", "second"],
                 "env": [{"name": "OUT", "value": str(out)},
                         {"name": "IGNORED", "valueFrom": {"secretKeyRef": {"name": "s"}}}],
             }},
        ],
    }))
    assert st["phase"] == "Succeeded", st
    assert lines(out) == [hostile, "second"]
    assert not (tmp_path / "pwned").exists()


def test_parameter_sources_and_single_pass(run, tmp_path):
    out = tmp_path / "argv"
    st = run(run_workflow({
        "entrypoint": "main",
        "arguments": param_args(site="rack-7", sneaky="{{workflow.name}}"),
        "templates": [{
            "name": "main",
            "inputs": {"parameters": [
                {"name": "site"},                     # from spec.arguments
                {"name": "level", "default": "info"},  # default
                {"name": "fixed", "value": "v"},       # value
            ]},
            "container": {
                "command": ["sh", "-c", ARGV_DUMP, "sh"],
                "args": ["{{inputs.parameters.site}}", "{{inputs.parameters.level}}",
                         "{{inputs.parameters.fixed}}", "{{workflow.parameters.site}}",
                         "{{ workflow.name }}", "{{workflow.namespace}}",
                         "{{workflow.parameters.sneaky}}"],
                "env": [{"name": "OUT", "value": str(out)}],
            },
        }],
    }))
    assert st["phase"] == "Succeeded", st
    assert lines(out) == ["rack-7", "info", "v", "rack-7", "wf", "health", "{{workflow.name}}"]


def test_script_source_and_env_are_substituted(run, tmp_path):
    out = tmp_path / "out"
    st = run(run_workflow({
        "entrypoint": "main",
        "arguments": param_args(word="tick"),
        "templates": [{"name": "main", "script": {
            "command": ["sh"],
            "source": 'echo "{{workflow.parameters.word}} $EXTRA" > "$OUT"',
            "env": [{"name": "OUT", "value": str(out)},
                    {"name": "EXTRA", "value": "{{workflow.name}}"}],
        }}],
    }))
    assert st["phase"] == "Succeeded", st
    assert lines(out) == ["tick wf"]


# -- loops --------------------------------------------------------------------


def touch_template(tmp_path):
    return {"name": "touch", "inputs": {"parameters": [{"name": "f"}]},
            "container": {"command": ["touch", f"{tmp_path}/{{{{inputs.parameters.f}}}}"]}}


def test_with_items_scalars(run, tmp_path):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [[
                {"name": "mk", "template": "touch", "withItems": ["a", "b", 3],
                 "arguments": param_args(f="f-{{item}}")},
            ]]},
            touch_template(tmp_path),
        ],
    }))
    assert st["phase"] == "Succeeded", st
    assert sorted(p.name for p in tmp_path.iterdir()) == ["f-3", "f-a", "f-b"]
    pods = [n for n in st["nodes"].values() if n["type"] == "Pod"]
    assert sorted(n["displayName"] for n in pods) == ["mk(0:a)", "mk(1:b)", "mk(2:3)"]
    assert all(n["phase"] == "Succeeded" and n["templateName"] == "touch" for n in pods)


def test_with_items_maps(run, tmp_path):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [[
                {"name": "mk", "template": "touch",
                 "withItems": [{"host": "db", "port": 5432}, {"host": "web", "port": 80}],
                 "arguments": param_args(f="{{item.host}}-{{ item.port }}")},
            ]]},
            touch_template(tmp_path),
        ],
    }))
    assert st["phase"] == "Succeeded", st
    assert sorted(p.name for p in tmp_path.iterdir()) == ["db-5432", "web-80"]
    assert node(st, "mk(0)")["type"] == "Pod" and node(st, "mk(1)")["type"] == "Pod"


def test_with_items_empty_list_succeeds(run, tmp_path):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [
                [{"name": "mk", "template": "touch", "withItems": [],
                  "arguments": param_args(f="{{item}}")}],
                [{"name": "after", "template": "touch", "arguments": param_args(f="after")}],
            ]},
            touch_template(tmp_path),
        ],
    }))
    assert st["phase"] == "Succeeded", st
    assert [p.name for p in tmp_path.iterdir()] == ["after"]
    assert [n["displayName"] for n in st["nodes"].values() if n["type"] == "Pod"] == ["after"]


def test_with_param_from_previous_result(run, tmp_path):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [
                [{"name": "gen", "template": "gen"}],
                [{"name": "mk", "template": "touch",
                  "withParam": "{{steps.gen.outputs.result}}",
                  "arguments": param_args(f="p-{{item}}")}],
            ]},
            {"name": "gen", "container": {"command": ["echo", '["x", "y", 7]']}},
            touch_template(tmp_path),
        ],
    }))
    assert st["phase"] == "Succeeded", st
    assert sorted(p.name for p in tmp_path.iterdir()) == ["p-7", "p-x", "p-y"]


def test_with_param_not_a_list_fails(run, tmp_path):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [[
                {"name": "mk", "template": "touch", "withParam": '{"not": "a list"}',
                 "arguments": param_args(f="{{item}}")},
            ]]},
            touch_template(tmp_path),
        ],
    }))
    assert st["phase"] == "Failed"
    assert "not a JSON list" in st["message"]
    assert list(tmp_path.iterdir()) == []


def test_fanned_out_outputs_are_unresolved(run, tmp_path):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [
                [{"name": "many", "template": "say", "withItems": [1, 2],
                  "arguments": param_args(m="{{item}}")}],
                [{"name": "use", "template": "say",
                  "arguments": param_args(m="{{steps.many.outputs.result}}")}],
            ]},
            {"name": "say", "inputs": {"parameters": [{"name": "m"}]},
             "container": {"command": ["echo", "{{inputs.parameters.m}}"]}},
        ],
    }))
    assert st["phase"] == "Failed"
    assert "failed to resolve {{steps.many.outputs.result}}" in st["message"]


# -- outputs ------------------------------------------------------------------


def test_result_and_path_outputs_flow_between_steps(run, tmp_path):
    out = tmp_path / "argv"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [
                [{"name": "produce", "template": "produce"}],
                [{"name": "consume", "template": "consume", "arguments": param_args(
                    r="{{steps.produce.outputs.result}}",
                    p="{{steps.produce.outputs.parameters.lag}}",
                    d="{{steps.produce.outputs.parameters.absent}}",
                    cwd="{{steps.produce.outputs.parameters.cwd}}",
                )}],
            ], "outputs": {"parameters": [
                {"name": "again", "globalName": "lag-global",
                 "valueFrom": {"parameter": "{{steps.produce.outputs.parameters.lag}}"}},
            ]}},
            sh("produce", "echo 42ms > lag.txt; pwd > cwd.txt; echo line1; echo line2",
               outputs={"parameters": [
                   {"name": "lag", "valueFrom": {"path": "lag.txt"}},
                   {"name": "cwd", "valueFrom": {"path": "cwd.txt"}},
                   {"name": "absent", "valueFrom": {"path": "nope.txt", "default": "fallback"}},
               ]}),
            {"name": "consume",
             "inputs": {"parameters": [{"name": n} for n in ("r", "p", "d", "cwd")]},
             "container": {
                 "command": ["sh", "-c", ARGV_DUMP, "sh"],
                 "args": ["{{inputs.parameters.r}}", "{{inputs.parameters.p}}",
                          "{{inputs.parameters.d}}", "{{inputs.parameters.cwd}}"],
                 "env": [{"name": "OUT", "value": str(out)}]}},
        ],
    }))
    assert st["phase"] == "Succeeded", st
    got = lines(out)
    # a multi-line result stays one argument; one trailing newline is dropped
    assert got[:4] == ["line1", "line2", "42ms", "fallback"]
    workdir = got[4]
    assert workdir != os.getcwd() and not os.path.exists(workdir)  # fresh, and removed
    produced = node(st, "produce")["outputs"]
    assert produced["result"] == "line1\nline2"
    assert {"name": "lag", "value": "42ms"} in produced["parameters"]
    assert {"name": "lag-global", "value": "42ms"} in st["outputs"]["parameters"]


def test_absolute_output_path(run, tmp_path):
    target = tmp_path / "abs.txt"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [sh("main", f"echo absolute > {target}", outputs={"parameters": [
            {"name": "v", "globalName": "v", "valueFrom": {"path": str(target)}},
        ]})],
    }))
    assert st["phase"] == "Succeeded", st
    assert st["outputs"]["parameters"] == [{"name": "v", "value": "absolute"}]


def test_missing_output_path_without_default_fails(run):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [sh("main", "true", outputs={"parameters": [
            {"name": "v", "valueFrom": {"path": "never-written.txt"}},
        ]})],
    }))
    assert st["phase"] == "Failed"
    assert "never-written.txt" in st["message"]


def test_leaf_without_path_output_keeps_working_directory(run, tmp_path):
    out = tmp_path / "cwd"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [sh("main", f"pwd > {out}")],
    }))
    assert st["phase"] == "Succeeded", st
    assert lines(out) == [os.getcwd()]


# -- DAG ----------------------------------------------------------------------


def append_template(log):
    return {"name": "append", "inputs": {"parameters": [{"name": "n"}]},
            "container": {"command": ["sh", "-c", f'echo "$0" >> {log}',
                                      "{{inputs.parameters.n}}"]}}


def task(name, template="append", deps=None, **extra):
    t = {"name": name, "template": template, **extra}
    if template == "append":
        t["arguments"] = param_args(n=name)
    if deps:
        t["dependencies"] = deps
    return t


def test_dag_diamond_ordering(run, tmp_path):
    log = tmp_path / "log"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "dag": {"tasks": [
                # listed out of order on purpose: only dependencies decide
                {**task("D"), "depends": "B && C"},
                task("C", deps=["A"]),
                task("B", deps=["A"]),
                task("A"),
            ]}},
            append_template(log),
        ],
    }))
    assert st["phase"] == "Succeeded", st
    got = lines(log)
    assert got[0] == "A" and got[-1] == "D" and sorted(got) == ["A", "B", "C", "D"]
    root = node(st, "wf")
    assert root["type"] == "DAG" and len(root["children"]) == 4


def test_dag_branches_run_concurrently(run, tmp_path):
    """B waits for a file only C creates and C for a file only B creates:
    this can finish only if both are running at the same time."""
    def rendezvous(mine, theirs):
        return sh(f"meet-{mine}", (
            f"touch {tmp_path}/{mine}; i=0; "
            f"while [ ! -e {tmp_path}/{theirs} ]; do "
            "i=$((i+1)); [ $i -gt 400 ] && exit 1; sleep 0.02; done"
        ))

    st = run(run_workflow({
        "entrypoint": "main",
        "activeDeadlineSeconds": 5,
        "templates": [
            {"name": "main", "dag": {"tasks": [
                task("A", "ok"),
                task("B", "meet-b", deps=["A"]),
                task("C", "meet-c", deps=["A"]),
            ]}},
            {"name": "ok", "container": {"command": ["true"]}},
            rendezvous("b", "c"),
            rendezvous("c", "b"),
        ],
    }))
    assert st["phase"] == "Succeeded", st


def failing_dag(log, **dag_extra):
    return {
        "entrypoint": "main",
        "templates": [
            {"name": "main", "dag": {"tasks": [
                task("bad", "boom"),
                task("after-bad", deps=["bad"]),
                task("last", deps=["after-bad"]),
                task("side"),
                task("side-2", deps=["side"]),
            ], **dag_extra}},
            sh("boom", "echo kaboom >&2; exit 7"),
            append_template(log),
        ],
    }


def test_dag_fail_fast_omits_downstream(run, tmp_path):
    log = tmp_path / "log"
    st = run(run_workflow(failing_dag(log)))
    assert st["phase"] == "Failed"
    assert "exit code 7" in st["message"] and "kaboom" in st["message"]
    assert node(st, "bad")["phase"] == "Failed"
    assert node(st, "after-bad")["phase"] == "Omitted"
    assert node(st, "last")["phase"] == "Omitted"
    assert "after-bad" not in lines(log) and "last" not in lines(log)
    # "side" started together with "bad" and was allowed to finish
    assert node(st, "side")["phase"] == "Succeeded"


def test_dag_without_fail_fast_finishes_independent_branch(run, tmp_path):
    log = tmp_path / "log"
    st = run(run_workflow(failing_dag(log, failFast=False)))
    assert st["phase"] == "Failed"
    assert "exit code 7" in st["message"]
    assert sorted(lines(log)) == ["side", "side-2"]
    assert node(st, "side-2")["phase"] == "Succeeded"
    assert node(st, "after-bad")["phase"] == "Omitted"
    assert node(st, "last")["phase"] == "Omitted"


def test_dag_cycle_fails_before_any_process_starts(run, tmp_path):
    log = tmp_path / "log"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "dag": {"tasks": [
                task("free"),
                task("ping", deps=["pong"]),
                task("pong", deps=["ping"]),
            ]}},
            append_template(log),
        ],
    }))
    assert st["phase"] == "Failed"
    assert "cycle" in st["message"] and ("'ping'" in st["message"] or "'pong'" in st["message"])
    assert not log.exists()
    assert "nodes" not in st


# -- when ---------------------------------------------------------------------


def test_when_false_skips_and_its_output_is_unresolved(run, tmp_path):
    log = tmp_path / "log"
    spec = {
        "entrypoint": "main",
        "arguments": param_args(mode="quick"),
        "templates": [
            {"name": "main", "steps": [
                [{"name": "deep", "template": "append", "arguments": param_args(n="deep"),
                  "when": "{{workflow.parameters.mode}} == full"},
                 {"name": "always", "template": "append", "arguments": param_args(n="always"),
                  "when": "{{workflow.parameters.mode}} != full && 2 > 1"}],
            ]},
            append_template(log),
        ],
    }
    st = run(run_workflow(spec))
    assert st["phase"] == "Succeeded", st
    assert lines(log) == ["always"]
    skipped = node(st, "deep")
    assert skipped["type"] == "Skipped" and skipped["phase"] == "Skipped"
    assert node(st, "always")["phase"] == "Succeeded"

    spec["templates"][0]["steps"].append(
        [{"name": "use", "template": "append",
          "arguments": param_args(n="{{steps.deep.outputs.result}}")}]
    )
    st = run(run_workflow(spec))
    assert st["phase"] == "Failed"
    assert "failed to resolve {{steps.deep.outputs.result}}" in st["message"]


def test_malformed_when_fails_the_node(run, tmp_path):
    marker = tmp_path / "executed"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [[
                {"name": "s", "template": "ok",
                 "when": f"__import__('os').system('touch {marker}') == 0"},
            ]]},
            {"name": "ok", "container": {"command": ["true"]}},
        ],
    }))
    assert st["phase"] == "Failed"
    assert "invalid when expression" in st["message"]
    assert not marker.exists()


# -- exit handler ---------------------------------------------------------------


def exit_spec(tmp_path, main_script, handler_script=None, **extra):
    record = f'echo "$0" > {tmp_path}/status'
    return {
        "entrypoint": "main",
        "onExit": "bye",
        "templates": [
            sh("main", main_script),
            {"name": "bye", "container": {
                "command": ["sh", "-c", handler_script or record, "{{workflow.status}}"]}},
        ],
        **extra,
    }


def test_exit_handler_after_success(run, tmp_path):
    st = run(run_workflow(exit_spec(tmp_path, "true")))
    assert st["phase"] == "Succeeded", st
    assert lines(tmp_path / "status") == ["Succeeded"]


def test_exit_handler_after_failure_keeps_main_message(run, tmp_path):
    st = run(run_workflow(exit_spec(tmp_path, "echo main-broke >&2; exit 2")))
    assert st["phase"] == "Failed"
    assert "main-broke" in st["message"]
    assert lines(tmp_path / "status") == ["Failed"]


def test_exit_handler_after_deadline(run, tmp_path):
    st = run(run_workflow(exit_spec(tmp_path, "sleep 30", activeDeadlineSeconds=1)))
    assert st["phase"] == "Failed"
    assert "deadline" in st["message"]
    assert lines(tmp_path / "status") == ["Failed"]


def test_failing_exit_handler_fails_the_workflow(run, tmp_path):
    st = run(run_workflow(exit_spec(tmp_path, "true", "echo handler-broke >&2; exit 4")))
    assert st["phase"] == "Failed"
    assert "handler-broke" in st["message"]
    # ... but when both fail the entrypoint's message is the one reported
    st = run(run_workflow(exit_spec(tmp_path, "echo main-broke >&2; exit 2",
                                    "echo handler-broke >&2; exit 4")))
    assert st["phase"] == "Failed"
    assert "main-broke" in st["message"]


def test_workflow_status_is_unresolved_outside_the_exit_handler(run):
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [{"name": "main", "container": {"command": ["echo", "{{workflow.status}}"]}}],
    }))
    assert st["phase"] == "Failed"
    assert "failed to resolve {{workflow.status}}" in st["message"]


# -- retries ------------------------------------------------------------------


def test_backoff_with_limit(run, tmp_path):
    attempts = tmp_path / "attempts"
    t0 = time.monotonic()
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [{
            "name": "main",
            "retryStrategy": {"limit": "2", "retryPolicy": "Always",
                              "backoff": {"duration": "0.2s", "factor": 2}},
            "script": {"command": ["sh"],
                       "source": f"echo {{{{retries}}}} >> {attempts}; test {{{{retries}}}} -eq 2"},
        }],
    }))
    elapsed = time.monotonic() - t0
    assert st["phase"] == "Succeeded", st
    assert lines(attempts) == ["0", "1", "2"]
    # waits of 0.2 s and 0.4 s; 50 ms allowed for event-loop timer granularity
    assert elapsed >= 0.6 - 0.05
    assert elapsed < 10  # only here to catch a hang
    retry = node(st, "wf")
    assert retry["type"] == "Retry" and len(retry["children"]) == 3
    assert [st["nodes"][c]["phase"] for c in retry["children"]] == [
        "Failed", "Failed", "Succeeded"]


def test_backoff_max_duration_stops_retrying(run, tmp_path):
    attempts = tmp_path / "attempts"
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [
            {"name": "main", "steps": [[{"name": "s", "template": "flaky"}]]},
            {"name": "flaky",
             "retryStrategy": {"limit": 50, "retryPolicy": "OnFailure", "backoff": {
                 "duration": "0.2s", "factor": 1, "maxDuration": "0.7s"}},
             "container": {"command": ["sh", "-c", f"echo x >> {attempts}; false"]}},
        ],
    }))
    assert st["phase"] == "Failed"
    # attempts at about 0, 0.2, 0.4 and 0.6 s; 0.8 s would be past maxDuration
    assert 1 < len(lines(attempts)) <= 5


def test_retries_without_backoff_are_immediate(run, tmp_path):
    attempts = tmp_path / "attempts"
    t0 = time.monotonic()
    st = run(run_workflow({
        "entrypoint": "main",
        "templates": [{"name": "main", "retryStrategy": {"limit": 3},
                       "container": {"command": ["sh", "-c", f"echo x >> {attempts}; false"]}}],
    }))
    assert st["phase"] == "Failed"
    assert len(lines(attempts)) == 4
    assert time.monotonic() - t0 < 5


# -- cancellation -------------------------------------------------------------


#: the shell stays and waits for its background child
WAITING = "sleep 30 & echo $$ $! > {pidfile}; wait"
#: the shell exits at once; only the background child, which still holds the
#: leaf's stdout, keeps the leaf running
ORPHANING = "sleep 30 & echo $$ $! > {pidfile}"


def pids_spec(pidfile, script=WAITING, **extra):
    return {
        "entrypoint": "main",
        "templates": [sh("main", script.format(pidfile=pidfile))],
        **extra,
    }


def assert_gone_within(pids, seconds):
    deadline = time.monotonic() + seconds
    alive = list(pids)
    while alive and time.monotonic() < deadline:
        for pid in list(alive):
            try:
                os.kill(pid, 0)
            except ProcessLookupError:
                alive.remove(pid)
        if alive:
            time.sleep(0.02)
    assert not alive, f"still running after {seconds}s: {alive}"
    for pid in pids:
        with pytest.raises(ProcessLookupError):
            os.kill(pid, 0)


@pytest.mark.parametrize("script", [WAITING, ORPHANING], ids=["waiting", "orphaning"])
def test_deadline_kills_shell_and_grandchild(run, tmp_path, script):
    pidfile = tmp_path / "pids"
    st = run(run_workflow(pids_spec(pidfile, script, activeDeadlineSeconds=1)))
    assert st["phase"] == "Failed"
    assert "deadline" in st["message"]
    pids = [int(p) for p in pidfile.read_text().split()]
    assert len(pids) == 2
    assert_gone_within(pids, 2.0)
    assert node(st, "wf")["phase"] == "Failed"


@pytest.mark.parametrize("script", [WAITING, ORPHANING], ids=["waiting", "orphaning"])
def test_engine_stop_kills_shell_and_grandchild(run, tmp_path, script):
    pidfile = tmp_path / "pids"
    st = run(run_workflow(
        pids_spec(pidfile, script),
        stop_when=lambda: pidfile.exists() and len(pidfile.read_text().split()) == 2,
    ))
    assert st["phase"] == "Running"  # stopped mid-run: no terminal write
    pids = [int(p) for p in pidfile.read_text().split()]
    assert len(pids) == 2
    assert_gone_within(pids, 2.0)


def test_exit_handler_budget_kills_and_publishes_no_outputs(run, tmp_path):
    """The entrypoint succeeds and has an output; the exit handler runs out
    of its budget. Its processes are killed too, and the workflow, having
    timed out, publishes no outputs."""
    pidfile = tmp_path / "pids"
    st = run(run_workflow({
        "entrypoint": "main",
        "onExit": "bye",
        "activeDeadlineSeconds": 1,
        "templates": [
            sh("main", "true", outputs={"parameters": [{"name": "m", "value": "1"}]}),
            sh("bye", ORPHANING.format(pidfile=pidfile)),
        ],
    }))
    assert st["phase"] == "Failed"
    assert st["message"] == "exit handler: deadline exceeded"
    assert "outputs" not in st
    assert node(st, "wf")["phase"] == "Succeeded"
    assert node(st, "wf.onExit")["phase"] == "Failed"
    assert_gone_within([int(p) for p in pidfile.read_text().split()], 2.0)


def test_cancellation_during_spawn_still_kills_the_child(run, monkeypatch):
    """A cancellation that arrives while the process is still being started
    must not lose track of it."""
    from active_monitor_amd.workflow.executor import WorkflowRun

    real_spawn = asyncio.create_subprocess_exec
    started = []

    async def slow_spawn(*args, **kwargs):
        proc = await real_spawn(*args, **kwargs)
        started.append(proc.pid)
        await asyncio.sleep(0.3)  # the caller is cancelled in here
        return proc

    async def go():
        monkeypatch.setattr(asyncio, "create_subprocess_exec", slow_spawn)
        wf_run = WorkflowRun({
            "entrypoint": "main",
            "templates": [{"name": "main", "container": {"command": ["sleep", "30"]}}],
        }, "wf", "health")
        task = asyncio.ensure_future(wf_run.run_entrypoint())
        while not started:
            await asyncio.sleep(0.01)
        task.cancel()
        with pytest.raises(asyncio.CancelledError):
            await task

    run(go(), timeout=10)
    assert len(started) == 1
    assert_gone_within(started, 2.0)


# -- regression guard -----------------------------------------------------------


def test_steps_spec_keeps_its_shape_and_gains_nodes(run):
    st = run(run_workflow({
        "entrypoint": "pipeline",
        "templates": [
            {"name": "pipeline", "steps": [
                [{"name": "a", "template": "ok"}],
                [{"name": "b", "template": "ok"}, {"name": "c", "template": "ok"}],
            ]},
            {"name": "ok", "container": {"command": ["true"]}},
        ],
    }))
    assert st["phase"] == "Succeeded"
    assert set(st) == {"phase", "finishedAt", "nodes"}
    by_type = {}
    for n in st["nodes"].values():
        by_type.setdefault(n["type"], []).append(n["displayName"])
        assert n["phase"] == "Succeeded"
        assert n["id"] in st["nodes"] and n["startedAt"] and n["finishedAt"]
        assert set(n["children"]) <= set(st["nodes"])
    assert by_type == {"Steps": ["wf"], "StepGroup": ["[0]", "[1]"], "Pod": ["a", "b", "c"]}
    assert st["nodes"]["wf"]["children"] == ["wf[0]", "wf[1]"]

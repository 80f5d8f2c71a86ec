"""Shared templates in standalone mode: ``templateRef`` on steps and tasks,
``spec.workflowTemplateRef``, their scoping, merging, recording and
validation. Leaves are ``echo`` / ``sh -c``; every run goes through
``LocalWorkflowEngine`` over the memory store.
"""
import asyncio
import time

import pytest

from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.registry import DEFAULT_REGISTRY, WF_API_VERSION, WF_KIND
from active_monitor_amd.workflow import LocalWorkflowEngine, validate_workflow_spec
from active_monitor_amd.workflow.templates import (
    has_references,
    lookup_in,
    merge_specs,
    resolve,
)
from active_monitor_amd.workflow.validate import ignored_synchronization

WF = (WF_API_VERSION, WF_KIND)


def echo(name, text):
    return {"name": name, "container": {"command": ["echo", text]}}


def wft(name, spec, namespace="health", cluster=False):
    meta = {"name": name}
    if not cluster:
        meta["namespace"] = namespace
    return {"apiVersion": WF_API_VERSION,
            "kind": "ClusterWorkflowTemplate" if cluster else "WorkflowTemplate",
            "metadata": meta, "spec": spec}


def lookup(*objects):
    return lookup_in({(o["kind"] == "ClusterWorkflowTemplate", o["metadata"]["name"]): o
                      for o in objects})


async def run_one(templates, spec, namespace="health", timeout=15.0):
    """Create ``templates``, start an engine, run ``spec``; the final status."""
    client = MemoryClient(MemoryApiServer())
    for obj in templates:
        await client.create(obj)
    engine = LocalWorkflowEngine(client, ttl_seconds=None)
    await engine.start()
    try:
        await client.create({"apiVersion": WF_API_VERSION, "kind": WF_KIND,
                             "metadata": {"name": "wf", "namespace": namespace},
                             "spec": spec})
        deadline = time.monotonic() + timeout
        while time.monotonic() < deadline:
            status = (await client.get(*WF, namespace, "wf")).get("status") or {}
            if status.get("phase") in ("Succeeded", "Failed"):
                assert engine.stats()["processes"] == 0
                return status
            await asyncio.sleep(0.01)
        raise AssertionError(f"workflow did not end: {status}")
    finally:
        await engine.stop()


def pod_outputs(status):
    return [n["outputs"]["result"] for n in status["nodes"].values() if n["type"] == "Pod"]


# -- registry ---------------------------------------------------------------


def test_both_kinds_are_registered_with_their_scope():
    info = DEFAULT_REGISTRY.by_plural(WF_API_VERSION, "workflowtemplates")
    assert (info.kind, info.namespaced) == ("WorkflowTemplate", True)
    info = DEFAULT_REGISTRY.by_plural(WF_API_VERSION, "clusterworkflowtemplates")
    assert (info.kind, info.namespaced) == ("ClusterWorkflowTemplate", False)


# -- 1. the name clash ------------------------------------------------------

LIB = wft("lib", {"templates": [
    {"name": "main", "steps": [[{"name": "call", "template": "leaf"}]]},
    echo("leaf", "lib"),
]})
CLASH = {"entrypoint": "main", "templates": [
    {"name": "main", "steps": [[
        {"name": "shared", "templateRef": {"name": "lib", "template": "main"}}]]},
    echo("leaf", "own"),
]}


def test_template_of_a_shared_template_never_means_the_workflows_own(run):
    status = run(run_one([LIB], CLASH))
    assert status["phase"] == "Succeeded", status.get("message")
    assert pod_outputs(status) == ["lib"]
    assert sorted(status["storedTemplates"]) == ["namespaced/lib/leaf", "namespaced/lib/main"]
    assert status["storedTemplates"]["namespaced/lib/leaf"] == LIB["spec"]["templates"][1]
    assert "storedWorkflowTemplateSpec" not in status

    nodes = status["nodes"]
    own = nodes["wf"]
    assert own["templateName"] == "main"
    assert "templateScope" not in own and "templateRef" not in own
    shared = nodes["wf[0].shared"]
    assert shared["type"] == "Steps"
    assert shared["templateRef"] == {"name": "lib", "template": "main"}
    assert shared["templateScope"] == "namespaced/lib"
    assert "templateName" not in shared
    leaf = nodes["wf[0].shared[0].call"]
    assert leaf["templateName"] == "leaf"
    assert leaf["templateScope"] == "namespaced/lib"
    assert "templateRef" not in leaf


def test_a_workflow_without_references_gains_no_field(run):
    status = run(run_one([LIB], {"entrypoint": "leaf", "templates": [echo("leaf", "own")]}))
    assert status["phase"] == "Succeeded"
    assert set(status) == {"phase", "finishedAt", "nodes"}
    assert set(status["nodes"]["wf"]) == {
        "id", "displayName", "type", "startedAt", "children", "templateName",
        "phase", "message", "finishedAt", "outputs"}


def test_referenced_template_sees_the_running_workflows_variables(run):
    lib = wft("lib", {"templates": [{
        "name": "say", "inputs": {"parameters": [{"name": "what", "default": "dflt"}]},
        "retryStrategy": {"limit": 1},
        "outputs": {"parameters": [{"name": "seen", "globalName": "seen",
                                    "value": "{{inputs.parameters.what}}"}]},
        "container": {"command": [
            "echo", "{{workflow.name}} {{workflow.parameters.site}} {{inputs.parameters.what}}"]},
    }]})
    spec = {"entrypoint": "main", "arguments": {"parameters": [{"name": "site", "value": "r9"}]},
            "templates": [{"name": "main", "dag": {"tasks": [
                {"name": "each", "templateRef": {"name": "lib", "template": "say"},
                 "withItems": ["a", "b"], "when": "{{item}} != b",
                 "arguments": {"parameters": [{"name": "what", "value": "{{item}}"}]}},
                {"name": "plain", "templateRef": {"name": "lib", "template": "say"}},
            ]}}]}
    status = run(run_one([lib], spec))
    assert status["phase"] == "Succeeded", status.get("message")
    assert sorted(pod_outputs(status)) == ["wf r9 a", "wf r9 dflt"]
    nodes = status["nodes"]
    assert nodes["wf.each(0:a)"]["type"] == "Retry"  # retryStrategy of the shared template
    assert nodes["wf.each(0:a)"]["templateRef"] == {"name": "lib", "template": "say"}
    skipped = nodes["wf.each(1:b)"]
    assert skipped["phase"] == "Skipped" and skipped["templateScope"] == "namespaced/lib"
    assert {"name": "seen", "value": "a"} in status["outputs"]["parameters"]


# -- 2. workflowTemplateRef -------------------------------------------------

BASE = wft("base", {
    "entrypoint": "main", "onExit": "bye", "activeDeadlineSeconds": 300,
    "arguments": {"parameters": [{"name": "a", "value": "ta"}, {"name": "b", "value": "tb"}]},
    "templates": [
        {"name": "main", "steps": [[{"name": "say", "template": "say"}]]},
        echo("say", "template says {{workflow.parameters.a}} {{workflow.parameters.b}}"),
        echo("bye", "bye {{workflow.status}}"),
    ],
})


def test_workflow_template_ref_merge(run):
    own_say = echo("say", "workflow says {{workflow.parameters.a}} {{workflow.parameters.b}} "
                          "{{workflow.parameters.c}}")
    spec = {"workflowTemplateRef": {"name": "base"}, "activeDeadlineSeconds": 30,
            "podGC": {"strategy": "OnPodCompletion"},
            "arguments": {"parameters": [{"name": "b", "value": "wb"},
                                         {"name": "c", "value": "wc"}]},
            "templates": [own_say]}
    status = run(run_one([BASE], spec))
    assert status["phase"] == "Succeeded", status.get("message")
    assert pod_outputs(status) == ["workflow says ta wb wc", "bye Succeeded"]
    assert status["storedWorkflowTemplateSpec"] == {
        "entrypoint": "main", "onExit": "bye", "activeDeadlineSeconds": 30,
        "podGC": {"strategy": "OnPodCompletion"},
        "arguments": {"parameters": [{"name": "a", "value": "ta"}, {"name": "b", "value": "wb"},
                                     {"name": "c", "value": "wc"}]},
        "templates": [BASE["spec"]["templates"][0], own_say, BASE["spec"]["templates"][2]],
    }
    assert "storedTemplates" not in status
    # the merged templates are the workflow's own: its nodes are as ever
    assert all("templateScope" not in n and "templateRef" not in n
               for n in status["nodes"].values())


def test_merge_leaves_both_inputs_alone():
    tspec = {"entrypoint": "t", "arguments": {"parameters": [{"name": "a", "value": "1"}]}}
    wspec = {"workflowTemplateRef": {"name": "x"}, "entrypoint": None,
             "arguments": {"parameters": [{"name": "a", "value": "2"}]}}
    merged = merge_specs(tspec, wspec)
    assert merged == {"entrypoint": "t",
                      "arguments": {"parameters": [{"name": "a", "value": "2"}]}}
    assert tspec["arguments"]["parameters"] == [{"name": "a", "value": "1"}]


def test_value_less_parameter_must_be_supplied(run):
    needy = wft("needy", {"entrypoint": "say", "arguments": {"parameters": [{"name": "site"}]},
                          "templates": [echo("say", "{{workflow.parameters.site}}")]})
    status = run(run_one([needy], {"workflowTemplateRef": {"name": "needy"}}))
    assert status["phase"] == "Failed"
    assert "'site'" in status["message"]
    assert "nodes" not in status  # nothing started
    status = run(run_one([needy], {
        "workflowTemplateRef": {"name": "needy"},
        "arguments": {"parameters": [{"name": "site", "value": "r1"}]}}))
    assert status["phase"] == "Succeeded", status.get("message")
    assert pod_outputs(status) == ["r1"]


# -- 3. cluster scope -------------------------------------------------------


def test_cluster_scope_on_both_reference_forms(run):
    cluster = wft("shared", {"entrypoint": "say", "templates": [echo("say", "cluster")]},
                  cluster=True)
    elsewhere = wft("shared", {"entrypoint": "say", "templates": [echo("say", "elsewhere")]},
                    namespace="other")
    by_step = {"entrypoint": "main", "templates": [{"name": "main", "steps": [[
        {"name": "c", "templateRef": {"name": "shared", "template": "say",
                                      "clusterScope": True}}]]}]}
    status = run(run_one([cluster, elsewhere], by_step))
    assert status["phase"] == "Succeeded", status.get("message")
    assert pod_outputs(status) == ["cluster"]
    assert list(status["storedTemplates"]) == ["cluster/shared/say"]
    node = status["nodes"]["wf[0].c"]
    assert node["templateRef"] == {"name": "shared", "template": "say", "clusterScope": True}
    assert node["templateScope"] == "cluster/shared"

    status = run(run_one([cluster, elsewhere],
                         {"workflowTemplateRef": {"name": "shared", "clusterScope": True}}))
    assert status["phase"] == "Succeeded", status.get("message")
    assert pod_outputs(status) == ["cluster"]

    # without clusterScope the name is looked up in the Workflow's namespace,
    # where there is none: the one in "other" is not found
    status = run(run_one([cluster, elsewhere], {"workflowTemplateRef": {"name": "shared"}}))
    assert status["phase"] == "Failed"
    assert status["message"] == 'workflowtemplates.argoproj.io "shared" not found'
    by_step["templates"][0]["steps"][0][0]["templateRef"].pop("clusterScope")
    status = run(run_one([cluster, elsewhere], by_step))
    assert status["message"] == 'workflowtemplates.argoproj.io "shared" not found'


# -- 4. reference loops -----------------------------------------------------


def test_a_chain_a_b_a_terminates_and_runs(run):
    def hop(name, other):
        return wft(name, {"templates": [
            {"name": "go", "inputs": {"parameters": [{"name": "n"}]}, "steps": [
                [{"name": "say", "template": "say"}],
                [{"name": "next", "templateRef": {"name": other, "template": "go"},
                  "when": "{{inputs.parameters.n}} < 2",
                  "arguments": {"parameters": [{"name": "n", "value": "2"}]}}]]},
            echo("say", name),
        ]})

    spec = {"entrypoint": "main", "templates": [{"name": "main", "steps": [[
        {"name": "start", "templateRef": {"name": "a", "template": "go"},
         "arguments": {"parameters": [{"name": "n", "value": "1"}]}}]]}]}
    found = resolve(spec, lookup(hop("a", "b"), hop("b", "a")))
    assert sorted(found.stored) == ["namespaced/a/go", "namespaced/a/say",
                                    "namespaced/b/go", "namespaced/b/say"]
    status = run(run_one([hop("a", "b"), hop("b", "a")], spec))
    assert status["phase"] == "Succeeded", status.get("message")
    assert pod_outputs(status) == ["a", "b"]


# -- 5. failures and validation ---------------------------------------------


def ref_spec(ref, **call):
    return {"entrypoint": "main", "templates": [
        {"name": "main", "steps": [[{"name": "s", "templateRef": ref, **call}]]},
        echo("leaf", "own")]}


@pytest.mark.parametrize("spec, message", [
    (ref_spec({"name": "gone", "template": "x"}),
     'workflowtemplates.argoproj.io "gone" not found'),
    ({"workflowTemplateRef": {"name": "gone"}},
     'workflowtemplates.argoproj.io "gone" not found'),
    (ref_spec({"name": "gone", "template": "x", "clusterScope": True}),
     'clusterworkflowtemplates.argoproj.io "gone" not found'),
    ({"workflowTemplateRef": {"name": "gone", "clusterScope": True}},
     'clusterworkflowtemplates.argoproj.io "gone" not found'),
    (ref_spec({"name": "lib", "template": "nope"}),
     "template reference lib.nope not found"),
], ids=["step", "spec", "cluster-step", "cluster-spec", "template"])
def test_unresolved_references_fail_the_workflow_before_any_process(run, spec, message):
    status = run(run_one([LIB], spec))
    assert status["phase"] == "Failed"
    assert status["message"] == message
    assert "nodes" not in status and "storedTemplates" not in status
    problems = validate_workflow_spec(spec, lookup(LIB))
    assert len(problems) == 1 and problems[0].endswith(message)


def test_malformed_references_are_one_problem_each():
    both = ref_spec({"name": "lib", "template": "leaf"}, template="leaf")
    (problem,) = validate_workflow_spec(both, lookup(LIB))
    assert problem == ("template 'main': step 's': template and templateRef "
                       "are mutually exclusive")
    (problem,) = validate_workflow_spec(both)
    assert "mutually exclusive" in problem

    body = {"entrypoint": "main", "templates": [
        {"name": "main", "templateRef": {"name": "lib", "template": "leaf"}}]}
    assert validate_workflow_spec(body, lookup(LIB)) == [
        "template 'main': templateRef is not supported"]
    assert validate_workflow_spec(body) == ["template 'main': templateRef is not supported"]


def test_one_argument_validation_says_it_cannot_resolve():
    (problem,) = validate_workflow_spec(ref_spec({"name": "lib", "template": "leaf"}))
    assert problem.startswith("template 'main': step 's': templateRef cannot be resolved here")
    (problem,) = validate_workflow_spec({"workflowTemplateRef": {"name": "base"}})
    assert problem.startswith("spec.workflowTemplateRef cannot be resolved here")
    assert "entrypoint" not in problem


def test_reachable_shared_templates_are_validated_in_their_scope():
    checks = wft("net-checks", {"templates": [
        {"name": "probe", "dag": {"tasks": [
            {"name": "x", "template": "leaf", "dependencies": ["y"]},
            {"name": "y", "template": "leaf", "dependencies": ["x"]}]}},
        echo("leaf", "{{workflow.parameters.undeclared}} {{item}}"),
        {"name": "unreached", "steps": [[{"name": "s", "template": "missing"}]]},
    ]})
    spec = {"entrypoint": "main", "templates": [{"name": "main", "steps": [[
        {"name": "s", "templateRef": {"name": "net-checks", "template": "probe"}}]]}]}
    problems = validate_workflow_spec(spec, lookup(checks))
    assert ("template 'probe' of WorkflowTemplate 'net-checks': "
            "dependency cycle through task 'x'") in problems
    leaf = "template 'leaf' of WorkflowTemplate 'net-checks': "
    assert leaf + ("{{workflow.parameters.undeclared}} refers to an undeclared "
                   "workflow parameter") in problems
    assert any(p.startswith(leaf + "{{item}} is only available") for p in problems)
    assert len(problems) == 3  # nothing about the template that is never reached

    spec["arguments"] = {"parameters": [{"name": "undeclared", "value": "now it is"}]}
    assert len(validate_workflow_spec(spec, lookup(checks))) == 2
    # a resolved bundle serves as well as a lookup
    assert validate_workflow_spec(spec, resolve(spec, lookup(checks))) == \
        validate_workflow_spec(spec, lookup(checks))


def test_in_scope_template_that_is_missing_is_reported_in_scope():
    lib = wft("lib", {"templates": [
        {"name": "main", "steps": [[{"name": "call", "template": "leaf"}]]}]})
    problems = validate_workflow_spec(CLASH, lookup(lib))  # CLASH has a leaf of its own
    assert problems == [
        "template 'main' of WorkflowTemplate 'lib': step 'call': template 'leaf' not found"]


def test_ignored_synchronization_looks_at_reached_shared_templates():
    lib = wft("lib", {"templates": [
        {**echo("leaf", "x"), "synchronization": {"mutex": {"name": "m"}}}]})
    spec = ref_spec({"name": "lib", "template": "leaf"})
    assert ignored_synchronization(spec) == []
    (found,) = ignored_synchronization(spec, resolve(spec, lookup(lib)))
    assert "namespaced/lib/leaf" in found


def test_a_merged_parameter_without_value_runs_with_its_default(run):
    lib = wft("lib", {"entrypoint": "say",
                      "arguments": {"parameters": [{"name": "site", "default": "d1"},
                                                   {"name": "from-file",
                                                    "valueFrom": {"path": "/x"}}]},
                      "templates": [echo("say", "{{workflow.parameters.site}}")]})
    found = resolve({"workflowTemplateRef": {"name": "lib"}}, lookup(lib))
    assert found.spec["arguments"]["parameters"][0] == {
        "name": "site", "default": "d1", "value": "d1"}
    assert "value" not in lib["spec"]["arguments"]["parameters"][0]  # the template is left alone
    ((_, message),) = found.errors  # valueFrom has no local source
    assert "'from-file'" in message
    del lib["spec"]["arguments"]["parameters"][1]
    status = run(run_one([lib], {"workflowTemplateRef": {"name": "lib"}}))
    assert (status["phase"], pod_outputs(status)) == ("Succeeded", ["d1"])


@pytest.mark.parametrize("spec", [
    {"templates": 5},
    {"templates": [5, None, {"name": ["unhashable"]}, {"name": "m", "dag": [{"name": "x"}]}]},
    {"templates": [{"name": "m", "dag": {"tasks": 5}}, {"name": "n", "steps": 7},
                   {"name": "o", "steps": [5, [None, {"name": "s", "templateRef": 3}]]}]},
    {"templates": [{"name": "m", "steps": [[
        {"name": "s", "templateRef": {"name": ["x"], "template": {"y": 1}}},
        {"name": "t", "template": ["x"]},
        {"name": "u", "templateRef": {"name": "bad", "template": "m"}}]]}]},
    {"workflowTemplateRef": 5},
    {"workflowTemplateRef": {"name": "bad"}, "templates": 5, "arguments": 5},
    {"workflowTemplateRef": {"name": "bad"}, "templates": [{"name": {"a": 1}}, 7],
     "arguments": {"parameters": [5, {"name": ["p"]}, {"name": "q"}]}},
    {"workflowTemplateRef": {"name": "bad"}, "arguments": {"parameters": 5}},
], ids=lambda spec: str(sorted(spec))[:30])
def test_resolution_raises_for_nothing_a_stored_spec_may_hold(spec):
    bad = wft("bad", {"templates": [5, {"name": "m", "dag": [1]},
                                    {"name": "n", "steps": [[{"name": "s", "template": ["x"]}]]}],
                      "arguments": {"parameters": 7}})
    has_references(spec)
    for known in (lookup(), lookup(bad), lookup(wft("bad", 5)),
                  lookup(wft("bad", {"templates": 5}))):
        found = resolve(spec, known)
        assert isinstance(found.problems(), list)

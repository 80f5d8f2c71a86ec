"""Run transcripts: the exact observable trace of one reconcile cycle.

The rest of the suite pins outcomes (counters, status strings, RBAC objects
present or absent). These tests pin what a merge of the health-check and
remedy code paths could change without touching any outcome: the ordered
event stream, the objects created and deleted (in order), the apiserver
operation counts, every write to the five ``Monitor*`` series for both
``workflow`` label values, and whether a repeat timer is left armed.

``HealthCheckReconciler`` is driven directly against the in-memory apiserver
with a ``FakeRecorder`` and no watch hub, Manager or workflow engine. The
client stamps a scripted terminal ``status`` into each Workflow as it is
created, so the watch's first poll already sees the terminal phase and
nothing sleeps (the one timeout scenario excepted, ~1 s).

The expected values are what the code does, quirks included (see the notes
on the scenarios); they are not a statement of what it should do.
"""
import copy

import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.api import HealthCheck
from active_monitor_amd.api.types import k8s_now, parse_k8s_time
from active_monitor_amd.engine.reconciler import HealthCheckReconciler
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.client import FakeRecorder
from active_monitor_amd.metrics import (
    MonitorError,
    MonitorFinishedTime,
    MonitorRuntime,
    MonitorStartedTime,
    MonitorSuccess,
)

NS = "health"
WF_API = "argoproj.io/v1alpha1"
TIME_FIELDS = ("startedAt", "finishedAt", "lastFailedAt", "remedyTriggeredAt",
               "remedyFinishedAt", "remedyLastFailedAt")
WF_NAME_FIELDS = ("lastFailedWorkflow", "lastSuccessfulWorkflow")
NO_OPS = {"get": 0, "list": 0, "create": 0, "update": 0, "update_status": 0, "delete": 0}

INLINE_WF = """\
apiVersion: argoproj.io/v1alpha1
kind: Workflow
spec:
  entrypoint: start
  templates:
    - name: start
      container:
        image: busybox
"""

SUCCEEDED = {"phase": "Succeeded"}
FAILED = {"phase": "Failed", "message": "check failed"}
FAILED_NON_STRING = {"phase": "Failed", "message": {"code": 7}}

NOT_FOUND_EVENT = (
    "Warning Warning Error attempting to find workflow for healthcheck. This may "
    "indicate that either the healthcheck was removed or the Workflow was GC'd "
    "before active-monitor could obtain the status"
)


class ScriptedClient(MemoryClient):
    """MemoryClient that plays the workflow engine: a Workflow is created
    already carrying the status scripted for its ``generateName`` (None: no
    status, i.e. it never starts). Creates and deletes are logged in order."""

    def __init__(self, server, script):
        super().__init__(server)
        self.script = script
        self.log = []

    async def create(self, obj, transfer=False):
        meta = obj["metadata"]
        if obj.get("kind") == "Workflow":
            status = self.script[meta["generateName"]]
            if status is not None:
                obj["status"] = copy.deepcopy(status)
            self.log.append(("create", "Workflow", meta["generateName"] + "*"))
        else:
            self.log.append(("create", obj["kind"], meta["name"]))
        return await super().create(obj, transfer)

    async def delete(self, api_version, kind, namespace, name):
        self.log.append(("delete", kind, name))
        await super().delete(api_version, kind, namespace, name)


def make_hc(name, *, level="cluster", sa="check-sa", remedy_sa=None, timeout=30,
            repeat=60, extra_spec=None, status=None):
    spec = {
        "repeatAfterSec": repeat,
        "level": level,
        "workflow": {
            "generateName": f"{name}-wf-",
            "workflowtimeout": timeout,
            "resource": {"namespace": NS, "serviceAccount": sa,
                         "source": {"inline": INLINE_WF}},
        },
    }
    if remedy_sa is not None:
        spec["remedyworkflow"] = {
            "generateName": f"{name}-remedy-wf-",
            "resource": {"namespace": NS, "serviceAccount": remedy_sa,
                         "source": {"inline": INLINE_WF}},
        }
    spec.update(extra_spec or {})
    obj = {"apiVersion": API_VERSION, "kind": "HealthCheck",
           "metadata": {"name": name, "namespace": NS}, "spec": spec}
    if status:
        obj["status"] = status
    return obj


def metric_values(name):
    """Current value of the five series for both workflow labels. Every
    scenario uses its own HealthCheck name, so these are also the deltas."""
    out = {}
    for label in ("healthCheck", "remedy"):
        out[label] = {
            "success": MonitorSuccess.value(name, label),
            "error": MonitorError.value(name, label),
            "runtime": MonitorRuntime.labels(name, label)._value.get(),
            "started": MonitorStartedTime.labels(name, label)._value.get(),
            "finished": MonitorFinishedTime.labels(name, label)._value.get(),
        }
    return out


def metric_shape(values):
    """Counters exactly; gauges as written (True) or untouched (False)."""
    return {
        label: {k: (v if k in ("success", "error") else v != 0) for k, v in m.items()}
        for label, m in values.items()
    }


UNTOUCHED = {"success": 0.0, "error": 0.0, "runtime": False, "started": False,
             "finished": False}


def normalise_status(status, name):
    """Timestamps become "T" (present) — absent ones stay absent; generated
    workflow names lose their random suffix."""
    out = dict(status)
    for f in TIME_FIELDS:
        if f in out:
            assert parse_k8s_time(out[f]) is not None, (f, out[f])
            out[f] = "T"
    for f in WF_NAME_FIELDS:
        if f in out:
            for gen in (f"{name}-remedy-wf-", f"{name}-wf-"):
                if out[f].startswith(gen) and len(out[f]) > len(gen):
                    out[f] = gen + "*"
                    break
    return out


class Transcript:
    pass


async def run_cycle(hc_obj, script):
    """Create the HealthCheck, run one reconcile to completion, and collect
    everything observable about it."""
    name = hc_obj["metadata"]["name"]
    server = MemoryApiServer()
    client = ScriptedClient(server, script)
    recorder = FakeRecorder()
    r = HealthCheckReconciler(client, recorder)
    assert r.wf_hub is None
    await MemoryClient.create(client, hc_obj)
    before = dict(server.op_counts)

    result = await r.reconcile(NS, name)
    await r.drain()

    t = Transcript()
    t.result = result
    t.events = list(recorder.events)
    t.log = list(client.log)
    t.ops = {k: server.op_counts[k] - before[k] for k in before}
    t.timer_armed = r.get_timer_by_name(name, NS) is not None
    t.counts = (r.reconcile_count, r.completed_runs, r.active_watches())
    r.stop_all()
    raw = server.get(API_VERSION, "HealthCheck", NS, name)
    t.raw_status = raw.get("status") or {}
    t.status = normalise_status(t.raw_status, name)
    t.metrics = metric_values(name)
    t.remaining = sorted(
        (kind, n) for (_, kind, _, n) in server._objects
        if kind not in ("HealthCheck", "Workflow")
    )
    return t


CHECK_RBAC_CLUSTER = [
    ("create", "ServiceAccount", "check-sa"),
    ("create", "ClusterRole", "check-sa-cluster-role"),
    ("create", "ClusterRoleBinding", "check-sa-cluster-role-binding"),
]
CHECK_RBAC_LEFT_CLUSTER = [
    ("ClusterRole", "check-sa-cluster-role"),
    ("ClusterRoleBinding", "check-sa-cluster-role-binding"),
    ("ServiceAccount", "check-sa"),
]
CHECK_SUBMIT_EVENTS = [
    "Normal Normal workflow is parsed from healthcheck",
    "Normal Normal Successfully created workflow",
]
REMEDY_SUBMIT_EVENTS = [
    "Normal Normal Remedy workflow is parsed from healthcheck",
    "Normal Normal Successfully created remedyWorkflow",
]
RESCHEDULED = "Normal Normal Rescheduled workflow for next run"


# ---------------------------------------------------------------------------
# 1. check succeeds, cluster level, no remedy
# ---------------------------------------------------------------------------

def test_check_succeeds_no_remedy(run):
    name = "tr-pass"
    t = run(run_cycle(make_hc(name), {f"{name}-wf-": SUCCEEDED}))
    assert t.result.error is None and t.result.requeue_after == 0.0
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Normal Normal Workflow status is Succeeded",
        RESCHEDULED,
    ]
    assert t.log == CHECK_RBAC_CLUSTER + [("create", "Workflow", f"{name}-wf-*")]
    assert t.remaining == CHECK_RBAC_LEFT_CLUSTER
    assert t.status == {
        "status": "Succeeded",
        "startedAt": "T",
        "finishedAt": "T",
        "successCount": 1,
        "totalHealthCheckRuns": 1,
        "lastSuccessfulWorkflow": f"{name}-wf-*",
    }
    # reconcile read, 3 RBAC gets, 1 workflow poll, 1 fresh read before the write
    assert t.ops == {**NO_OPS, "get": 6, "create": 4, "update_status": 1}
    assert metric_shape(t.metrics) == {
        "healthCheck": {"success": 1.0, "error": 0.0, "runtime": True,
                        "started": True, "finished": True},
        "remedy": UNTOUCHED,
    }
    assert t.timer_armed
    assert t.counts == (1, 1, 0)


# ---------------------------------------------------------------------------
# 2. check fails, no remedy
# ---------------------------------------------------------------------------

def test_check_fails_no_remedy(run):
    name = "tr-fail"
    t = run(run_cycle(make_hc(name), {f"{name}-wf-": FAILED}))
    assert t.result.error is None
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Warning Warning Workflow status is Failed",
        RESCHEDULED,
    ]
    assert t.log == CHECK_RBAC_CLUSTER + [("create", "Workflow", f"{name}-wf-*")]
    assert t.status == {
        "status": "Failed",
        "errorMessage": "check failed",
        "startedAt": "T",
        "finishedAt": "T",
        "lastFailedAt": "T",
        "failedCount": 1,
        "totalHealthCheckRuns": 1,
        "lastFailedWorkflow": f"{name}-wf-*",
    }
    assert t.ops == {**NO_OPS, "get": 6, "create": 4, "update_status": 1}
    # a failed run leaves the runtime gauge alone
    assert metric_shape(t.metrics) == {
        "healthCheck": {"success": 0.0, "error": 1.0, "runtime": False,
                        "started": True, "finished": True},
        "remedy": UNTOUCHED,
    }
    assert t.timer_armed
    assert t.counts == (1, 1, 0)


# ---------------------------------------------------------------------------
# 3. check fails, remedy succeeds — cluster and namespace level
# ---------------------------------------------------------------------------

REMEDY_OK_STATUS = {
    "status": "Failed",
    "errorMessage": "check failed",
    "startedAt": "T",
    "finishedAt": "T",
    "lastFailedAt": "T",
    "failedCount": 1,
    "totalHealthCheckRuns": 1,
    "remedyStatus": "Succeeded",
    "remedyTriggeredAt": "T",
    "remedyFinishedAt": "T",
    "remedySuccessCount": 1,
    "remedyTotalRuns": 1,
}


@pytest.mark.parametrize("level,role,binding,role_kind,binding_kind", [
    ("cluster", "-cluster-role", "-cluster-role-binding", "ClusterRole",
     "ClusterRoleBinding"),
    ("namespace", "-ns-role", "-ns-role-binding", "Role", "RoleBinding"),
])
def test_check_fails_remedy_succeeds(run, level, role, binding, role_kind, binding_kind):
    name = f"tr-remedy-{level}"
    hc = make_hc(name, level=level, remedy_sa="remedy-sa")
    t = run(run_cycle(hc, {f"{name}-wf-": FAILED, f"{name}-remedy-wf-": SUCCEEDED}))
    assert t.result.error is None
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Warning Warning Workflow status is Failed",
    ] + REMEDY_SUBMIT_EVENTS + [
        "Normal Normal Remedy workflow status is Succeeded",
        RESCHEDULED,
    ]
    # remedy RBAC: create → use → delete; the check's RBAC stays
    assert t.log == [
        ("create", "ServiceAccount", "check-sa"),
        ("create", role_kind, "check-sa" + role),
        ("create", binding_kind, "check-sa" + binding),
        ("create", "Workflow", f"{name}-wf-*"),
        ("create", "ServiceAccount", "remedy-sa"),
        ("create", role_kind, "remedy-sa" + role),
        ("create", binding_kind, "remedy-sa" + binding),
        ("create", "Workflow", f"{name}-remedy-wf-*"),
        ("delete", "ServiceAccount", "remedy-sa"),
        ("delete", role_kind, "remedy-sa" + role),
        ("delete", binding_kind, "remedy-sa" + binding),
    ]
    assert t.remaining == sorted([
        ("ServiceAccount", "check-sa"),
        (role_kind, "check-sa" + role),
        (binding_kind, "check-sa" + binding),
    ])
    # the remedy's success overwrites nothing of the check's failure, but it
    # does claim the shared lastSuccessfulWorkflow; lastFailedWorkflow keeps
    # the check's workflow
    assert t.status == {
        **REMEDY_OK_STATUS,
        "lastFailedWorkflow": f"{name}-wf-*",
        "lastSuccessfulWorkflow": f"{name}-remedy-wf-*",
    }
    # two status writes: the remedy's, then the check's
    assert t.ops == {**NO_OPS, "get": 14, "create": 8, "update_status": 2, "delete": 3}
    assert metric_shape(t.metrics) == {
        "healthCheck": {"success": 0.0, "error": 1.0, "runtime": False,
                        "started": True, "finished": True},
        "remedy": {"success": 1.0, "error": 0.0, "runtime": True,
                   "started": True, "finished": True},
    }
    # the remedy's finished-time gauge carries the CHECK's finish epoch
    check_finished = parse_k8s_time(t.raw_status["finishedAt"]).timestamp()
    assert t.metrics["remedy"]["finished"] == int(check_finished)
    assert t.timer_armed
    assert t.counts == (1, 1, 0)


def test_remedy_finished_gauge_is_the_checks_finish_epoch(run):
    """The same quirk with the two epochs far apart: watching a succeeded
    remedy for a HealthCheck whose check finished in 2001 sets the remedy
    finished-time gauge to 2001 and the started-time gauge to now. With no
    check finish time at all the gauge falls back to now."""
    async def go():
        server = MemoryApiServer()
        client = ScriptedClient(server, {"r-": SUCCEEDED})
        r = HealthCheckReconciler(client, FakeRecorder())
        out = {}
        for name, finished in (("tr-gauge-old", "2001-01-01T00:00:00Z"),
                               ("tr-gauge-none", None)):
            obj = make_hc(name, remedy_sa="remedy-sa",
                          status={"finishedAt": finished} if finished else None)
            await MemoryClient.create(client, obj)
            wf = await client.create({"apiVersion": WF_API, "kind": "Workflow",
                                      "metadata": {"generateName": "r-", "namespace": NS}})
            await r.watch_remedy_workflow(NS, wf["metadata"]["name"],
                                          HealthCheck.from_dict(obj))
            out[name] = metric_values(name)["remedy"]
        return out

    out = run(go())
    now = parse_k8s_time(k8s_now()).timestamp()
    old = out["tr-gauge-old"]
    assert old["finished"] == parse_k8s_time("2001-01-01T00:00:00Z").timestamp()
    assert abs(old["started"] - now) < 60
    assert abs(out["tr-gauge-none"]["finished"] - now) < 60


# ---------------------------------------------------------------------------
# 4. check fails, remedy fails with a non-string message
# ---------------------------------------------------------------------------

def test_check_fails_remedy_fails_non_string_message(run):
    name = "tr-remedy-fails"
    hc = make_hc(name, remedy_sa="remedy-sa")
    t = run(run_cycle(hc, {f"{name}-wf-": FAILED,
                           f"{name}-remedy-wf-": FAILED_NON_STRING}))
    assert t.result.error is None
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Warning Warning Workflow status is Failed",
    ] + REMEDY_SUBMIT_EVENTS + [
        "Warning Warning remedy workflow status is failed",
        RESCHEDULED,
    ]
    # a non-string message is dropped (no remedyErrorMessage); the remedy's
    # name replaces the check's in the shared lastFailedWorkflow
    assert t.status == {
        "status": "Failed",
        "errorMessage": "check failed",
        "startedAt": "T",
        "finishedAt": "T",
        "lastFailedAt": "T",
        "failedCount": 1,
        "totalHealthCheckRuns": 1,
        "remedyStatus": "Failed",
        "remedyTriggeredAt": "T",
        "remedyFinishedAt": "T",
        "remedyLastFailedAt": "T",
        "remedyFailedCount": 1,
        "remedyTotalRuns": 1,
        "lastFailedWorkflow": f"{name}-remedy-wf-*",
    }
    assert t.ops == {**NO_OPS, "get": 14, "create": 8, "update_status": 2, "delete": 3}
    assert metric_shape(t.metrics) == {
        "healthCheck": {"success": 0.0, "error": 1.0, "runtime": False,
                        "started": True, "finished": True},
        "remedy": {"success": 0.0, "error": 1.0, "runtime": False,
                   "started": True, "finished": True},
    }
    assert t.remaining == CHECK_RBAC_LEFT_CLUSTER
    assert t.timer_armed
    assert t.counts == (1, 1, 0)


# ---------------------------------------------------------------------------
# 5. remedy limit reached and the reset interval elapsed: reset, then run
# ---------------------------------------------------------------------------

def test_remedy_reset_interval_elapsed_then_runs(run):
    name = "tr-reset-run"
    hc = make_hc(
        name, remedy_sa="remedy-sa",
        extra_spec={"remedyRunsLimit": 2, "remedyResetInterval": 10},
        status={"remedyTotalRuns": 2, "remedySuccessCount": 1, "remedyFailedCount": 1,
                "remedyFinishedAt": "2001-01-01T00:00:00Z",
                "remedyLastFailedAt": "2001-01-01T00:00:00Z",
                "remedyErrorMessage": "old", "remedyStatus": "Failed"},
    )
    t = run(run_cycle(hc, {f"{name}-wf-": FAILED, f"{name}-remedy-wf-": SUCCEEDED}))
    assert t.result.error is None
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Warning Warning Workflow status is Failed",
        "Normal Normal RemedyResetInterval elapsed so Remedy is reset",
    ] + REMEDY_SUBMIT_EVENTS + [
        "Normal Normal Remedy workflow status is Succeeded",
        RESCHEDULED,
    ]
    # counters restart from the reset: one run, one success, old failure gone
    assert t.status == {
        **REMEDY_OK_STATUS,
        "lastFailedWorkflow": f"{name}-wf-*",
        "lastSuccessfulWorkflow": f"{name}-remedy-wf-*",
    }
    assert t.ops == {**NO_OPS, "get": 14, "create": 8, "update_status": 2, "delete": 3}
    assert metric_shape(t.metrics)["remedy"] == {
        "success": 1.0, "error": 0.0, "runtime": True, "started": True, "finished": True}
    assert t.timer_armed
    assert t.counts == (1, 1, 0)


# ---------------------------------------------------------------------------
# 6. check passes after remedies ran: "HealthCheck Passed so Remedy is reset"
# ---------------------------------------------------------------------------

def test_check_passes_so_remedy_is_reset(run):
    name = "tr-pass-reset"
    hc = make_hc(
        name, remedy_sa="remedy-sa",
        status={"remedyTotalRuns": 1, "remedySuccessCount": 1,
                "remedyTriggeredAt": "2001-01-01T00:00:00Z",
                "remedyFinishedAt": "2001-01-01T00:00:05Z",
                "remedyStatus": "Succeeded", "failedCount": 1,
                "totalHealthCheckRuns": 1},
    )
    t = run(run_cycle(hc, {f"{name}-wf-": SUCCEEDED}))
    assert t.result.error is None
    # note the event says "passed", the status says "Passed"
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Normal Normal Workflow status is Succeeded",
        "Normal Normal HealthCheck passed so Remedy is reset",
        RESCHEDULED,
    ]
    assert t.log == CHECK_RBAC_CLUSTER + [("create", "Workflow", f"{name}-wf-*")]
    assert t.status == {
        "status": "Succeeded",
        "startedAt": "T",
        "finishedAt": "T",
        "successCount": 1,
        "failedCount": 1,
        "totalHealthCheckRuns": 2,
        "lastSuccessfulWorkflow": f"{name}-wf-*",
        "remedyStatus": "HealthCheck Passed so Remedy is reset",
    }
    assert t.ops == {**NO_OPS, "get": 6, "create": 4, "update_status": 1}
    assert metric_shape(t.metrics) == {
        "healthCheck": {"success": 1.0, "error": 0.0, "runtime": True,
                        "started": True, "finished": True},
        "remedy": UNTOUCHED,
    }
    assert t.timer_armed
    assert t.counts == (1, 1, 0)


# ---------------------------------------------------------------------------
# 7. health-check SA == remedy SA: the remedy SA is renamed "<sa>-remedy"
# ---------------------------------------------------------------------------

def test_same_service_account_renames_remedy_sa(run):
    name = "tr-same-sa"
    hc = make_hc(name, sa="shared-sa", remedy_sa="shared-sa")
    t = run(run_cycle(hc, {f"{name}-wf-": FAILED, f"{name}-remedy-wf-": SUCCEEDED}))
    assert t.result.error is None
    assert t.log == [
        ("create", "ServiceAccount", "shared-sa"),
        ("create", "ClusterRole", "shared-sa-cluster-role"),
        ("create", "ClusterRoleBinding", "shared-sa-cluster-role-binding"),
        ("create", "Workflow", f"{name}-wf-*"),
        ("create", "ServiceAccount", "shared-sa-remedy"),
        ("create", "ClusterRole", "shared-sa-remedy-cluster-role"),
        ("create", "ClusterRoleBinding", "shared-sa-remedy-cluster-role-binding"),
        ("create", "Workflow", f"{name}-remedy-wf-*"),
        ("delete", "ServiceAccount", "shared-sa-remedy"),
        ("delete", "ClusterRole", "shared-sa-remedy-cluster-role"),
        ("delete", "ClusterRoleBinding", "shared-sa-remedy-cluster-role-binding"),
    ]
    assert t.remaining == [
        ("ClusterRole", "shared-sa-cluster-role"),
        ("ClusterRoleBinding", "shared-sa-cluster-role-binding"),
        ("ServiceAccount", "shared-sa"),
    ]
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Warning Warning Workflow status is Failed",
    ] + REMEDY_SUBMIT_EVENTS + [
        "Normal Normal Remedy workflow status is Succeeded",
        RESCHEDULED,
    ]
    assert t.status == {
        **REMEDY_OK_STATUS,
        "lastFailedWorkflow": f"{name}-wf-*",
        "lastSuccessfulWorkflow": f"{name}-remedy-wf-*",
    }
    assert t.ops == {**NO_OPS, "get": 14, "create": 8, "update_status": 2, "delete": 3}
    assert t.timer_armed


# ---------------------------------------------------------------------------
# 8. the watched workflow does not exist
# ---------------------------------------------------------------------------

def test_watch_of_a_missing_workflow(run):
    """The check's watch emits its Warning and returns; the remedy's returns
    silently. Neither writes status, touches a metric, arms a timer or counts
    a completed run."""
    name = "tr-gone"
    obj = make_hc(name, remedy_sa="remedy-sa")

    async def go():
        server = MemoryApiServer()
        client = ScriptedClient(server, {})
        recorder = FakeRecorder()
        r = HealthCheckReconciler(client, recorder)
        await MemoryClient.create(client, obj)
        before = dict(server.op_counts)
        seen = []
        for watch in (r.watch_workflow_reschedule, r.watch_remedy_workflow):
            await watch(NS, "no-such-workflow", HealthCheck.from_dict(obj))
            seen.append((list(recorder.events),
                         {k: server.op_counts[k] - before[k] for k in before}))
            del recorder.events[:]
            before = dict(server.op_counts)
        raw = server.get(API_VERSION, "HealthCheck", NS, name)
        return seen, raw, r

    (check, remedy), raw, r = run(go())
    assert check == ([NOT_FOUND_EVENT], {**NO_OPS, "get": 1})
    assert remedy == ([], {**NO_OPS, "get": 1})
    assert "status" not in raw
    assert metric_shape(metric_values(name)) == {"healthCheck": UNTOUCHED,
                                                 "remedy": UNTOUCHED}
    assert r.get_timer_by_name(name, NS) is None
    assert r.completed_runs == 0


# ---------------------------------------------------------------------------
# 9. timeout: the workflow never gets a status (the one timed case, ~1 s)
# ---------------------------------------------------------------------------

def test_check_times_out(run):
    name = "tr-timeout"
    t = run(run_cycle(make_hc(name, timeout=1), {f"{name}-wf-": None}))
    assert t.result.error is None
    assert t.events == CHECK_SUBMIT_EVENTS + [
        "Warning Warning Workflow timed out",
        "Warning Warning Workflow status is Failed",
        RESCHEDULED,
    ]
    # synthesized {phase: Failed, message: Failed}
    assert t.status == {
        "status": "Failed",
        "errorMessage": "Failed",
        "startedAt": "T",
        "finishedAt": "T",
        "lastFailedAt": "T",
        "failedCount": 1,
        "totalHealthCheckRuns": 1,
        "lastFailedWorkflow": f"{name}-wf-*",
    }
    # one more get than a normal run: the workflow is polled again after the
    # deadline, and that poll's answer is replaced by the synthesized status
    assert t.ops == {**NO_OPS, "get": 7, "create": 4, "update_status": 1}
    assert metric_shape(t.metrics) == {
        "healthCheck": {"success": 0.0, "error": 1.0, "runtime": False,
                        "started": True, "finished": True},
        "remedy": UNTOUCHED,
    }
    assert t.timer_armed
    assert t.counts == (1, 1, 0)


# ---------------------------------------------------------------------------
# 10. invalid backoff parameters
# ---------------------------------------------------------------------------

def test_invalid_backoff_params_synthesize_failure_at_once(run):
    """``workflowtimeout: 0`` cannot reach the watch through ``reconcile``:
    parsing the workflow first defaults the timeout to ``repeatAfterSec``, and
    a HealthCheck with neither ``repeatAfterSec`` nor a cron schedule stops in
    the pause branch before anything is submitted. So the case is built by
    handing both watches a HealthCheck whose timeout is still 0, which is what
    the watch guards against: the backoff constructor rejects the parameters,
    and the first iteration polls once, then reports a timeout without
    sleeping — even though the workflow is merely pending."""
    async def go(name, remedy):
        obj = make_hc(name, timeout=0)
        server = MemoryApiServer()
        client = ScriptedClient(server, {"w-": None})
        recorder = FakeRecorder()
        r = HealthCheckReconciler(client, recorder)
        await MemoryClient.create(client, obj)
        wf = await client.create({"apiVersion": WF_API, "kind": "Workflow",
                                  "metadata": {"generateName": "w-", "namespace": NS}})
        hc = HealthCheck.from_dict(obj)
        assert hc.spec.workflow.timeout == 0
        before = dict(server.op_counts)
        watch = r.watch_remedy_workflow if remedy else r.watch_workflow_reschedule
        await watch(NS, wf["metadata"]["name"], hc)
        ops = {k: server.op_counts[k] - before[k] for k in before}
        armed = r.get_timer_by_name(name, NS) is not None
        r.stop_all()
        raw = server.get(API_VERSION, "HealthCheck", NS, name)
        return recorder.events, ops, armed, r.completed_runs, raw["status"]

    events, ops, armed, completed, status = run(go("tr-bad-backoff", remedy=False))
    assert events == [
        "Warning Warning Workflow timed out",
        "Warning Warning Workflow status is Failed",
        RESCHEDULED,
    ]
    # workflow poll, fresh HealthCheck read, status write
    assert ops == {**NO_OPS, "get": 2, "update_status": 1}
    assert (armed, completed) == (True, 1)
    assert normalise_status(status, "tr-bad-backoff") == {
        "status": "Failed",
        "errorMessage": "Failed",
        "startedAt": "T",
        "finishedAt": "T",
        "lastFailedAt": "T",
        "failedCount": 1,
        "totalHealthCheckRuns": 1,
        "lastFailedWorkflow": status["lastFailedWorkflow"],
    }
    assert status["lastFailedWorkflow"].startswith("w-")

    events, ops, armed, completed, status = run(go("tr-bad-backoff-remedy", remedy=True))
    assert events == [
        "Warning Warning remedy workflow is timedout",
        "Warning Warning remedy workflow status is failed",
    ]
    assert ops == {**NO_OPS, "get": 2, "update_status": 1}
    assert (armed, completed) == (False, 0)
    assert normalise_status(status, "tr-bad-backoff-remedy") == {
        "remedyStatus": "Failed",
        "remedyErrorMessage": "Failed",
        "remedyTriggeredAt": "T",
        "remedyFinishedAt": "T",
        "remedyLastFailedAt": "T",
        "remedyFailedCount": 1,
        "remedyTotalRuns": 1,
        "lastFailedWorkflow": status["lastFailedWorkflow"],
    }

"""One fixed sequence of writes against the store, in memory and journaled,
compared with a recorded transcript: every outcome (resourceVersion,
generation, warnings, or the error's type, code and message), every watch
event, the counters and the final resourceVersion. Uids and timestamps are
left out; generated names are recorded as ``<prefix>*``."""
import asyncio
import copy

from active_monitor_amd import API_VERSION
from active_monitor_amd.kube import MemoryApiServer
from active_monitor_amd.kube.errors import ApiError
from active_monitor_amd.kube.memory import healthcheck_schemas

HC = (API_VERSION, "HealthCheck")
CM = ("v1", "ConfigMap")
EVENT = ("v1", "Event")
KINDS = (HC, CM, EVENT)
MODES = ("Warn", "Strict", "Ignore")


def hc(name, ns="health", **meta):
    return {
        "apiVersion": API_VERSION, "kind": "HealthCheck",
        "metadata": {"name": name, "namespace": ns, **meta},
        "spec": {
            "repeatAfterSec": 30, "level": "cluster",
            "workflow": {"generateName": f"{name}-wf-", "resource": {
                "namespace": ns, "serviceAccount": "sa",
                "source": {"inline": "kind: Workflow\n"}}},
        },
    }


def cm(name, ns="health", **meta):
    return {"apiVersion": "v1", "kind": "ConfigMap",
            "metadata": {"name": name, "namespace": ns, **meta},
            "data": {"k": "v"}}


def event(name):
    return {"apiVersion": "v1", "kind": "Event",
            "metadata": {"name": name, "namespace": "health"}, "reason": "R"}


class Recorder:
    def __init__(self, store):
        self.store = store
        self.log = []
        self.generated = set()

    def name(self, name):
        return "gen-*" if name in self.generated else name

    def do(self, label, write):
        """Run ``write(warnings)`` and record how it ended."""
        warnings = []
        try:
            out = write(warnings)
        except ApiError as e:
            self.log.append((label, type(e).__name__, e.code, e.message))
            return None
        meta = (out or {}).get("metadata") or {}
        self.log.append((label, "ok", meta.get("resourceVersion"),
                         meta.get("generation"), tuple(warnings)))
        return out

    def event_row(self, ev):
        obj = ev["object"]
        meta = obj["metadata"]
        return (ev["type"], obj["kind"], meta.get("namespace", ""),
                self.name(meta["name"]), meta["resourceVersion"],
                meta.get("generation"))


async def transcript(store):
    """The sequence. Returns what a test compares with the literals below."""
    rec = Recorder(store)
    do, s = rec.do, store
    subs = [s.watch(av, kind) for av, kind in KINDS]
    subs.append(s.watch(*HC, "other"))

    # 1-3: create by name, by generateName, twice
    do("create", lambda w: s.create(hc("a"), warnings=w))
    do("create other ns", lambda w: s.create(hc("a", ns="other"), warnings=w))
    for n in (1, 2):
        gen = cm("", generateName="gen-")
        del gen["metadata"]["name"]
        before = {o["metadata"]["name"] for o in s.list(*CM)}
        out = s.create(gen)
        name = out["metadata"]["name"]
        assert name.startswith("gen-") and len(name) > 4 and name not in before
        rec.generated.add(name)
        rec.log.append((f"create generateName {n}", "ok",
                        out["metadata"]["resourceVersion"]))
    do("create no name", lambda w: s.create(
        {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {}}, warnings=w))
    do("create duplicate", lambda w: s.create(hc("a"), warnings=w))

    # 4-7: update
    got = s.get(*HC, "health", "a")
    stale = copy.deepcopy(got)
    stale["metadata"]["resourceVersion"] = "999"
    stale["spec"]["repeatAfterSec"] = 31
    do("update stale", lambda w: s.update(stale, warnings=w))
    do("update absent", lambda w: s.update(hc("absent"), warnings=w))
    do("update no-op", lambda w: s.update(got, warnings=w))
    got["spec"]["repeatAfterSec"] = 31
    got = do("update spec", lambda w: s.update(got, warnings=w))
    got["metadata"]["labels"] = {"tier": "1"}
    got = do("update labels", lambda w: s.update(got, warnings=w))
    got["status"] = {"status": "Succeeded"}
    out = do("update status only", lambda w: s.update(got, warnings=w))
    assert "status" not in out
    del got["status"]

    # 8-9: update_status
    do("update_status no-op", lambda w: s.update_status(got, warnings=w))
    got["status"] = {"status": "Succeeded", "successCount": 1}
    got["spec"]["repeatAfterSec"] = 99  # not a status write's to change
    out = do("update_status", lambda w: s.update_status(got, warnings=w))
    assert out["spec"]["repeatAfterSec"] == 31 and out["status"]["successCount"] == 1
    do("update_status stale", lambda w: s.update_status(got, warnings=w))
    do("update_status absent", lambda w: s.update_status(hc("absent"), warnings=w))

    # 10-13: patch
    out = do("patch", lambda w: s.patch(
        *HC, "health", "a", {"spec": {"repeatAfterSec": 40}}, warnings=w))
    assert out["spec"]["repeatAfterSec"] == 40 and out["status"]["successCount"] == 1
    out = do("patch status", lambda w: s.patch(
        *HC, "health", "a", {"status": {"successCount": 2}, "spec": {"level": "x"}},
        subresource="status", warnings=w))
    assert out["status"] == {"status": "Succeeded", "successCount": 2}
    assert out["spec"]["level"] == "cluster"
    do("patch absent", lambda w: s.patch(*HC, "health", "up", {}, warnings=w))
    do("patch upsert", lambda w: s.patch(
        *HC, "health", "up", {"spec": hc("up")["spec"]}, upsert=True, warnings=w))
    do("patch upsert cluster-scoped", lambda w: s.patch(
        "v1", "Namespace", "ignored", "ns1", {}, upsert=True, warnings=w))
    do("patch stale rv", lambda w: s.patch(
        *HC, "health", "a", {"metadata": {"resourceVersion": "1"},
                             "spec": {"repeatAfterSec": 41}}, warnings=w))
    current = s.get(*HC, "health", "a")["metadata"]["resourceVersion"]
    do("patch current rv", lambda w: s.patch(
        *HC, "health", "a", {"metadata": {"resourceVersion": current},
                             "spec": {"repeatAfterSec": 41}}, warnings=w))

    # 14: a schema violation, and an unknown field, under each mode
    for mode in MODES:
        bad = hc(f"bad-{mode}")
        bad["spec"]["repeatAfterSec"] = "sixty"
        do(f"create invalid {mode}", lambda w: s.create(
            bad, field_validation=mode, warnings=w))
        cur = s.get(*HC, "health", "a")
        cur["spec"]["repeatAfterSec"] = "sixty"
        do(f"update invalid {mode}", lambda w: s.update(
            cur, field_validation=mode, warnings=w))
        cur = s.get(*HC, "health", "a")
        cur["status"]["successCount"] = "two"
        do(f"update_status invalid {mode}", lambda w: s.update_status(
            cur, field_validation=mode, warnings=w))
        do(f"patch invalid {mode}", lambda w: s.patch(
            *HC, "health", "a", {"spec": {"repeatAfterSec": "sixty"}},
            field_validation=mode, warnings=w))
        do(f"patch status invalid {mode}", lambda w: s.patch(
            *HC, "health", "a", {"status": {"successCount": "two"}},
            subresource="status", field_validation=mode, warnings=w))

        typo = hc(f"typo-{mode}")
        typo["spec"]["repeatAfterSecs"] = 60
        do(f"create unknown {mode}", lambda w: s.create(
            typo, field_validation=mode, warnings=w))
        cur = s.get(*HC, "health", "a")
        cur["spec"]["oops"] = mode
        do(f"update unknown {mode}", lambda w: s.update(
            cur, field_validation=mode, warnings=w))
        cur = s.get(*HC, "health", "a")
        cur["status"]["typo"] = mode
        do(f"update_status unknown {mode}", lambda w: s.update_status(
            cur, field_validation=mode, warnings=w))
        do(f"patch unknown {mode}", lambda w: s.patch(
            *HC, "health", "a", {"spec": {"oops": mode, "repeatAfterSec": 50}},
            field_validation=mode, warnings=w))

    # 15: an unknown mode, for a kind with a schema and for one without
    s.create(cm("plain"))
    for label, kind, make in (("schema", HC, hc), ("no schema", CM, cm)):
        name = "a" if kind is HC else "plain"
        ops_before = dict(s.op_counts)
        do(f"create Bogus {label}", lambda w: s.create(
            make("bogus"), field_validation="Bogus", warnings=w))
        cur = s.get(*kind, "health", name)
        do(f"update Bogus {label}", lambda w: s.update(
            cur, field_validation="Bogus", warnings=w))
        do(f"update_status Bogus {label}", lambda w: s.update_status(
            cur, field_validation="Bogus", warnings=w))
        do(f"patch Bogus {label}", lambda w: s.patch(
            *kind, "health", name, {"metadata": {"labels": {"x": "y"}}},
            field_validation="Bogus", warnings=w))
        ops_before["get"] += 1
        assert s.op_counts == ops_before  # refused before anything is counted

    # 16: a finalizer holds the delete until an update removes it
    s.create(cm("fin", uid="uid-fin", finalizers=["example.com/hold"]))
    s.create(cm("fin-dep", ownerReferences=[{"uid": "uid-fin"}]))
    do("delete with finalizer", lambda w: s.delete(*CM, "health", "fin"))
    do("delete with finalizer again", lambda w: s.delete(*CM, "health", "fin"))
    held = s.get(*CM, "health", "fin")
    assert held["metadata"]["deletionTimestamp"]
    held["metadata"]["finalizers"] = []
    do("update removes finalizer", lambda w: s.update(held, warnings=w))
    do("get after finalizer", lambda w: s.get(*CM, "health", "fin"))
    do("get dependent after finalizer", lambda w: s.get(*CM, "health", "fin-dep"))

    # 17: two levels of dependents go with their owner
    s.create(cm("own", uid="uid-own"))
    s.create(cm("child", uid="uid-child", ownerReferences=[{"uid": "uid-own"}]))
    s.create(cm("grandchild", ownerReferences=[{"uid": "uid-child"}]))
    s.create(cm("bystander", ownerReferences=[{"uid": "uid-else"}]))
    do("delete owner", lambda w: s.delete(*CM, "health", "own"))
    do("delete absent", lambda w: s.delete(*CM, "health", "own"))
    do("delete cluster-scoped", lambda w: s.delete("v1", "Namespace", "x", "ns1"))
    rec.log.append(("configmaps left", sorted(
        rec.name(o["metadata"]["name"]) for o in s.list(*CM))))

    # 18: the Event cap evicts the oldest, silently
    s.max_events = 3
    for n in range(5):
        do(f"create event {n}", lambda w: s.create(event(f"ev-{n}"), warnings=w))
    rec.log.append(("events left", [o["metadata"]["name"] for o in s.list(*EVENT)]))

    # 19: replay inside the retained window, and below it
    s.history_window = 4
    do("create event 5", lambda w: s.create(event("ev-5"), warnings=w))
    rv = int(s.resource_version())
    for label, args in (
        ("inside", (*EVENT, None, str(rv - 2))),
        ("inside, namespace", (*EVENT, "health", str(rv - 2))),
        ("inside, other namespace", (*EVENT, "other", str(rv - 2))),
        ("inside, other kind", (*CM, None, str(rv - 2))),
        ("at the horizon", (*EVENT, None, str(rv - 4))),
        ("below", (*EVENT, None, str(rv - 5))),
        ("invalid", (*EVENT, None, "abc")),
    ):
        try:
            rec.log.append((f"events_since {label}",
                            [rec.event_row(ev) for ev in s.events_since(*args)]))
        except ApiError as e:
            rec.log.append((f"events_since {label}", type(e).__name__, e.code,
                            e.message))

    await asyncio.sleep(0)  # the subscriptions' queues fill on the loop
    events = []
    for sub in subs:
        sub.close()
        events.append([rec.event_row(ev) async for ev in sub])
    return {
        "log": rec.log,
        "events": dict(zip(("HealthCheck", "ConfigMap", "Event", "HealthCheck/other"),
                           events)),
        "op_counts": dict(s.op_counts),
        "rejected_writes": s.rejected_writes,
        "resource_version": s.resource_version(),
    }


def stored(store):
    return sorted(
        (o["kind"], o["metadata"].get("namespace", ""), o["metadata"]["name"],
         o["metadata"]["resourceVersion"])
        for av, kind in KINDS + (("v1", "Namespace"),) for o in store.list(av, kind))


# -- the transcript, as recorded ------------------------------------------------

CONFLICT = ("ConflictError", 409,
            'Operation cannot be fulfilled on HealthCheck "a": the object has been '
            "modified; please apply your changes to the latest version and try again")
BOGUS = ("BadRequestError", 400,
         'invalid fieldValidation "Bogus": supported values: "Warn", "Strict", "Ignore"')


def not_found(what):
    return ("NotFoundError", 404, f"{what} not found")


def invalid(name, field):
    return ("InvalidError", 422,
            f'HealthCheck.activemonitor.keikoproj.io "{name}" is invalid: {field}: '
            f'Invalid value: "string": {field} in body must be of type integer: '
            '"string"')


def strict(field):
    return ("BadRequestError", 400,
            'HealthCheck in version "v1alpha1" cannot be handled as a HealthCheck: '
            f'strict decoding error: unknown field "{field}"')


def refused_as_invalid(mode):
    return [
        (f"create invalid {mode}", *invalid(f"bad-{mode}", "spec.repeatAfterSec")),
        (f"update invalid {mode}", *invalid("a", "spec.repeatAfterSec")),
        (f"update_status invalid {mode}", *invalid("a", "status.successCount")),
        (f"patch invalid {mode}", *invalid("a", "spec.repeatAfterSec")),
        (f"patch status invalid {mode}", *invalid("a", "status.successCount")),
    ]


def added(kind, name, rv, ns="health"):
    return ("ADDED", kind, ns, name, rv, 1)


HC_HQ = "healthchecks.activemonitor.keikoproj.io"
WRITES = ("create", "update", "update_status", "patch")

EXPECTED = {
    "log": [
        ("create", "ok", "1", 1, ()),
        ("create other ns", "ok", "2", 1, ()),
        ("create generateName 1", "ok", "3"),
        ("create generateName 2", "ok", "4"),
        ("create no name", "InvalidError", 422, "name or generateName is required"),
        ("create duplicate", "AlreadyExistsError", 409,
         'HealthCheck "a" already exists'),
        ("update stale", *CONFLICT),
        ("update absent", *not_found(f'{HC_HQ} "absent"')),
        ("update no-op", "ok", "1", 1, ()),
        ("update spec", "ok", "5", 2, ()),
        ("update labels", "ok", "6", 2, ()),
        ("update status only", "ok", "6", 2, ()),
        ("update_status no-op", "ok", "6", 2, ()),
        ("update_status", "ok", "7", 2, ()),
        ("update_status stale", *CONFLICT),
        ("update_status absent", *not_found(f'{HC_HQ} "absent"')),
        ("patch", "ok", "8", 3, ()),
        ("patch status", "ok", "9", 3, ()),
        ("patch absent", *not_found(f'{HC_HQ} "up"')),
        ("patch upsert", "ok", "10", 1, ()),
        ("patch upsert cluster-scoped", "ok", "11", 1, ()),
        ("patch stale rv", *CONFLICT),
        ("patch current rv", "ok", "12", 4, ()),
        *refused_as_invalid("Warn"),
        ("create unknown Warn", "ok", "13", 1, ("spec.repeatAfterSecs",)),
        ("update unknown Warn", "ok", "12", 4, ("spec.oops",)),
        ("update_status unknown Warn", "ok", "12", 4, ("status.typo",)),
        ("patch unknown Warn", "ok", "14", 5, ("spec.oops",)),
        *refused_as_invalid("Strict"),
        ("create unknown Strict", *strict("spec.repeatAfterSecs")),
        ("update unknown Strict", *strict("spec.oops")),
        ("update_status unknown Strict", *strict("status.typo")),
        ("patch unknown Strict", *strict("spec.oops")),
        *refused_as_invalid("Ignore"),
        ("create unknown Ignore", "ok", "15", 1, ()),
        ("update unknown Ignore", "ok", "14", 5, ()),
        ("update_status unknown Ignore", "ok", "14", 5, ()),
        ("patch unknown Ignore", "ok", "14", 5, ()),
        *((f"{write} Bogus schema", *BOGUS) for write in WRITES),
        *((f"{write} Bogus no schema", *BOGUS) for write in WRITES),
        ("delete with finalizer", "ok", None, None, ()),
        ("delete with finalizer again", "ok", None, None, ()),
        ("update removes finalizer", "ok", "20", 1, ()),
        ("get after finalizer", *not_found('configmaps "fin"')),
        ("get dependent after finalizer", *not_found('configmaps "fin-dep"')),
        ("delete owner", "ok", None, None, ()),
        ("delete absent", *not_found('configmaps "own"')),
        ("delete cluster-scoped", "ok", None, None, ()),
        ("configmaps left", ["bystander", "gen-*", "gen-*", "plain"]),
        ("create event 0", "ok", "30", 1, ()),
        ("create event 1", "ok", "31", 1, ()),
        ("create event 2", "ok", "32", 1, ()),
        ("create event 3", "ok", "33", 1, ()),
        ("create event 4", "ok", "34", 1, ()),
        ("events left", ["ev-2", "ev-3", "ev-4"]),
        ("create event 5", "ok", "35", 1, ()),
        ("events_since inside",
         [added("Event", "ev-4", "34"), added("Event", "ev-5", "35")]),
        ("events_since inside, namespace",
         [added("Event", "ev-4", "34"), added("Event", "ev-5", "35")]),
        ("events_since inside, other namespace", []),
        ("events_since inside, other kind", []),
        ("events_since at the horizon",
         [added("Event", "ev-2", "32"), added("Event", "ev-3", "33"),
          added("Event", "ev-4", "34"), added("Event", "ev-5", "35")]),
        ("events_since below", "ExpiredError", 410,
         "too old resource version: 30 (31)"),
        ("events_since invalid", "ExpiredError", 410,
         "resourceVersion 'abc' is invalid"),
    ],
    "events": {
        "HealthCheck": [
            added("HealthCheck", "a", "1"),
            added("HealthCheck", "a", "2", ns="other"),
            ("MODIFIED", "HealthCheck", "health", "a", "5", 2),
            ("MODIFIED", "HealthCheck", "health", "a", "6", 2),
            ("MODIFIED", "HealthCheck", "health", "a", "7", 2),
            ("MODIFIED", "HealthCheck", "health", "a", "8", 3),
            ("MODIFIED", "HealthCheck", "health", "a", "9", 3),
            added("HealthCheck", "up", "10"),
            ("MODIFIED", "HealthCheck", "health", "a", "12", 4),
            added("HealthCheck", "typo-Warn", "13"),
            ("MODIFIED", "HealthCheck", "health", "a", "14", 5),
            added("HealthCheck", "typo-Ignore", "15"),
        ],
        "ConfigMap": [
            added("ConfigMap", "gen-*", "3"),
            added("ConfigMap", "gen-*", "4"),
            added("ConfigMap", "plain", "16"),
            added("ConfigMap", "fin", "17"),
            added("ConfigMap", "fin-dep", "18"),
            ("MODIFIED", "ConfigMap", "health", "fin", "19", 1),
            # the finalizer's removal: DELETED at the rv the update assigned
            ("DELETED", "ConfigMap", "health", "fin", "20", 1),
            ("DELETED", "ConfigMap", "health", "fin-dep", "21", 1),
            added("ConfigMap", "own", "22"),
            added("ConfigMap", "child", "23"),
            added("ConfigMap", "grandchild", "24"),
            added("ConfigMap", "bystander", "25"),
            ("DELETED", "ConfigMap", "health", "own", "26", 1),
            ("DELETED", "ConfigMap", "health", "child", "27", 1),
            ("DELETED", "ConfigMap", "health", "grandchild", "28", 1),
        ],
        # Namespace ns1 came (11) and went (29) unwatched; cap evictions
        # publish nothing
        "Event": [added("Event", f"ev-{n}", str(30 + n)) for n in range(6)],
        "HealthCheck/other": [added("HealthCheck", "a", "2", ns="other")],
    },
    "op_counts": {"get": 19, "list": 4, "create": 27, "update": 22,
                  "update_status": 14, "delete": 5},
    "rejected_writes": 19,
    "resource_version": "35",
}


def test_transcript_in_memory(run):
    store = MemoryApiServer(schemas=healthcheck_schemas())
    assert run(transcript(store)) == EXPECTED


def test_transcript_journaled_and_reopened(run, tmp_path):
    store = MemoryApiServer.open(str(tmp_path), schemas=healthcheck_schemas())
    try:
        assert run(transcript(store)) == EXPECTED
        before = stored(store)
    finally:
        store.close()
    reopened = MemoryApiServer.open(str(tmp_path), schemas=healthcheck_schemas())
    try:
        assert stored(reopened) == before
        assert reopened.resource_version() == EXPECTED["resource_version"]
    finally:
        reopened.close()

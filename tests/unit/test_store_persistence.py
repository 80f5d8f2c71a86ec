"""Durable MemoryApiServer (kube/persist.py): everything a store opened on
a data directory holds comes back after close/reopen — objects, their
order, the resourceVersion, the Event cap's eviction order — and the journal
survives torn tails and crashes inside compaction but refuses real damage."""
import asyncio
import builtins
import json
import os
import random
import shutil
import subprocess
import sys

import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.kube import MemoryApiServer
from active_monitor_amd.kube import persist
from active_monitor_amd.kube.errors import ApiError, ExpiredError
from active_monitor_amd.kube.persist import (
    JOURNAL_FILE,
    SNAPSHOT_FILE,
    SNAPSHOT_TMP_FILE,
    StoreCorruptError,
    StoreLockedError,
)

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HC = (API_VERSION, "HealthCheck")
CM = ("v1", "ConfigMap")
EV = ("v1", "Event")
WF = ("argoproj.io/v1alpha1", "Workflow")
KINDS = (HC, CM, EV, WF)
NS = "health"


def dump(server):
    """Everything observable: per-kind lists (order included) and the rv."""
    return {
        "rv": server.resource_version(),
        "lists": [server.list(av, kind) for av, kind in KINDS],
        "len": len(server),
    }


def owner_ref(owner):
    return {"apiVersion": owner["apiVersion"], "kind": owner["kind"],
            "name": owner["metadata"]["name"], "uid": owner["metadata"]["uid"]}


class Driver:
    """A seeded random walk over every mutation the store has."""

    def __init__(self, server, seed):
        self.server = server
        self.rng = random.Random(seed)
        self.n = 0

    def _pick(self, av, kind):
        items = self.server.list(av, kind, NS)
        return self.rng.choice(items) if items else None

    def create_named(self):
        self.n += 1
        self.server.create({"apiVersion": CM[0], "kind": CM[1],
                            "metadata": {"name": f"cm-{self.n}", "namespace": NS},
                            "data": {"k": str(self.rng.random())}})

    def create_generated(self):
        self.server.create({"apiVersion": HC[0], "kind": HC[1],
                            "metadata": {"generateName": "hc-", "namespace": NS},
                            "spec": {"repeatAfterSec": self.rng.randrange(1, 99)}})

    def update(self):
        obj = self._pick(*CM)
        if obj:
            obj["data"] = {"k": str(self.rng.random())}
            obj["metadata"].setdefault("labels", {})["n"] = str(self.rng.randrange(9))
            self.server.update(obj)

    def update_status(self):
        obj = self._pick(*HC)
        if obj:
            obj["status"] = {"successCount": self.rng.randrange(1000)}
            self.server.update_status(obj)

    def merge_patch(self):
        obj = self._pick(*HC)
        if obj:
            self.server.patch(*HC, NS, obj["metadata"]["name"],
                              {"spec": {"repeatAfterSec": self.rng.randrange(1, 99),
                                        "level": self.rng.choice(["cluster", None])}})

    def upsert_patch(self):
        # hits an existing object about as often as it creates one
        name = f"up-{self.rng.randrange(8)}"
        self.server.patch(*CM, NS, name, {"data": {"v": str(self.rng.random())}},
                          upsert=True)

    def delete(self):
        obj = self._pick(*CM)
        if obj and not obj["metadata"].get("finalizers"):
            self.server.delete(*CM, NS, obj["metadata"]["name"])

    def finalizer_delete(self):
        self.n += 1
        name = f"fin-{self.n}"
        self.server.create({"apiVersion": CM[0], "kind": CM[1],
                            "metadata": {"name": name, "namespace": NS,
                                         "finalizers": ["test/hold"]}})
        self.server.delete(*CM, NS, name)  # only marks it
        if self.rng.random() < 0.7:  # some stay pending across the reopen
            held = self.server.get(*CM, NS, name)
            held["metadata"]["finalizers"] = []
            self.server.update(held)

    def owner_chain(self):
        root = self.server.create({"apiVersion": HC[0], "kind": HC[1],
                                   "metadata": {"generateName": "root-", "namespace": NS},
                                   "spec": {}})
        wf = self.server.create({"apiVersion": WF[0], "kind": WF[1],
                                 "metadata": {"generateName": "wf-", "namespace": NS,
                                              "ownerReferences": [owner_ref(root)]},
                                 "spec": {}})
        self.server.create({"apiVersion": EV[0], "kind": EV[1],
                            "metadata": {"generateName": "ev-", "namespace": NS,
                                         "ownerReferences": [owner_ref(wf)]},
                            "reason": "chained"})
        if self.rng.random() < 0.6:
            self.server.delete(*HC, NS, root["metadata"]["name"])

    OPS = ("create_named", "create_generated", "update", "update_status",
           "merge_patch", "upsert_patch", "delete", "finalizer_delete",
           "owner_chain")

    def step(self, count):
        for _ in range(count):
            getattr(self, self.rng.choice(self.OPS))()


@pytest.mark.parametrize("threshold,compacts", [(25, True), (10 ** 6, False)])
def test_round_trip_of_a_random_history(tmp_path, threshold, compacts):
    d = tmp_path / "store"
    server = MemoryApiServer.open(str(d), compact_threshold=threshold)
    Driver(server, seed=7).step(400)
    before = dump(server)
    compactions = server._journal.compactions
    server.close()
    assert (compactions >= 3) if compacts else (compactions == 0)
    assert before["len"] > 20

    again = MemoryApiServer.open(str(d), compact_threshold=threshold)
    try:
        assert dump(again) == before
        # derived state: cascade GC still works off the rebuilt owner index
        for root in again.list(*HC, NS):
            if root["metadata"]["name"].startswith("root-"):
                again.delete(*HC, NS, root["metadata"]["name"])
        assert again.list(*WF) == [] and again.list(*EV) == []
    finally:
        again.close()


def test_reopening_mid_sequence_changes_nothing(tmp_path):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d, compact_threshold=40)
    driver = Driver(server, seed=11)
    cuts = random.Random(3)
    for _ in range(6):
        driver.step(cuts.randrange(20, 90))
        before = dump(server)
        server.close()
        server = driver.server = MemoryApiServer.open(d, compact_threshold=40)
        assert dump(server) == before
    server.close()


def _event(name):
    return {"apiVersion": EV[0], "kind": EV[1],
            "metadata": {"name": name, "namespace": NS}, "count": 1}


def test_event_cap_evicts_oldest_created_after_reopen(tmp_path):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    server.max_events = 5
    for i in range(9):
        server.create(_event(f"ev-{i}"))
    # updating old survivors must not make them look young
    for name in ("ev-4", "ev-5"):
        ev = server.get(*EV, NS, name)
        ev["count"] = 2
        server.update(ev)
    names = [e["metadata"]["name"] for e in server.list(*EV)]
    assert names == ["ev-4", "ev-5", "ev-6", "ev-7", "ev-8"]
    server.close()

    server = MemoryApiServer.open(d)
    server.max_events = 5
    try:
        assert [e["metadata"]["name"] for e in server.list(*EV)] == names
        server.create(_event("ev-9"))
        assert [e["metadata"]["name"] for e in server.list(*EV)] == [
            "ev-5", "ev-6", "ev-7", "ev-8", "ev-9"]
    finally:
        server.close()


def _three_configmaps(d):
    server = MemoryApiServer.open(d)
    for i in range(3):
        server.create({"apiVersion": CM[0], "kind": CM[1],
                       "metadata": {"name": f"cm-{i}", "namespace": NS}})
    state = dump(server)
    server.close()
    return state


def test_torn_tail_is_dropped_and_truncated(tmp_path):
    d = str(tmp_path / "store")
    state = _three_configmaps(d)
    journal = os.path.join(d, JOURNAL_FILE)
    good = os.path.getsize(journal)
    with open(journal, "ab") as f:
        f.write(b'{"rv":4,"op":"put","obj":{"apiVersion":"v1","ki')

    server = MemoryApiServer.open(d)
    assert dump(server) == state
    assert os.path.getsize(journal) == good
    server.create({"apiVersion": CM[0], "kind": CM[1],
                   "metadata": {"name": "after", "namespace": NS}})
    state = dump(server)
    server.close()
    server = MemoryApiServer.open(d)
    assert dump(server) == state
    server.close()


def test_unparsable_final_line_is_a_torn_tail_too(tmp_path):
    d = str(tmp_path / "store")
    state = _three_configmaps(d)
    with open(os.path.join(d, JOURNAL_FILE), "ab") as f:
        f.write(b"\x00\x00\x00garbage\n")
    server = MemoryApiServer.open(d)
    assert dump(server) == state
    server.close()


def test_garbage_in_the_middle_refuses_to_open(tmp_path):
    d = str(tmp_path / "store")
    _three_configmaps(d)
    journal = os.path.join(d, JOURNAL_FILE)
    with open(journal, "rb") as f:
        lines = f.read().split(b"\n")
    lines[1] = b"not json at all"
    with open(journal, "wb") as f:
        f.write(b"\n".join(lines))
    with pytest.raises(StoreCorruptError) as err:
        MemoryApiServer.open(d)
    assert f"{journal}:2:" in str(err.value)
    assert err.value.line == 2
    # the refusal released the directory, and discarded nothing
    with open(journal, "rb") as f:
        assert f.read().split(b"\n") == lines
    with pytest.raises(StoreCorruptError):
        MemoryApiServer.open(d)


def test_unknown_format_version_refuses_to_open(tmp_path):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d, compact_threshold=1)
    for i in range(4):  # the journal must outgrow the live objects to compact
        server.patch(*CM, NS, "cm", {"data": {"i": str(i)}}, upsert=True)
    assert server._journal.compactions >= 1
    server.close()
    snap = os.path.join(d, SNAPSHOT_FILE)
    with open(snap, "rb") as f:
        lines = f.read().split(b"\n")
    header = json.loads(lines[0])
    assert header["format"] == 1
    header["format"] = 99
    lines[0] = json.dumps(header).encode()
    with open(snap, "wb") as f:
        f.write(b"\n".join(lines))
    with pytest.raises(StoreCorruptError) as err:
        MemoryApiServer.open(d)
    assert f"{snap}:1:" in str(err.value) and "99" in str(err.value)


def test_crash_between_snapshot_rename_and_journal_reset(tmp_path):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d, compact_threshold=30)
    driver = Driver(server, seed=5)
    while server._journal.records < 25:
        driver.step(1)
    journal = os.path.join(d, JOURNAL_FILE)
    saved = str(tmp_path / "journal.saved")
    shutil.copy(journal, saved)
    at_copy = server._journal.records
    while server._journal.compactions == 0:
        driver.step(1)
    assert at_copy > 0
    state = dump(server)
    server.close()

    # the state a crash right after the rename would leave, plus whatever
    # the new journal had gained: stale records first, then the fresh ones
    with open(journal, "rb") as f:
        fresh = f.read()
    with open(saved, "rb") as f:
        stale = f.read()
    with open(journal, "wb") as f:
        f.write(stale + fresh)
    server = MemoryApiServer.open(d)
    assert dump(server) == state
    server.close()


def test_leftover_temporary_snapshot_is_removed(tmp_path):
    d = str(tmp_path / "store")
    state = _three_configmaps(d)
    tmp = os.path.join(d, SNAPSHOT_TMP_FILE)
    with open(tmp, "wb") as f:
        f.write(b'{"format":1,"rv":999,"count":1}\n{"half":')
    server = MemoryApiServer.open(d)
    assert dump(server) == state
    assert not os.path.exists(tmp)
    server.close()


def test_watch_resume_across_a_reopen(tmp_path, run):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    old_rvs = []
    for i in range(3):
        made = server.create({"apiVersion": CM[0], "kind": CM[1],
                              "metadata": {"name": f"cm-{i}", "namespace": NS}})
        old_rvs.append(int(made["metadata"]["resourceVersion"]))
    server.delete(*CM, NS, "cm-0")  # deletions consume an rv as well
    restored = server.resource_version()
    assert int(restored) == 4
    server.close()

    server = MemoryApiServer.open(d)
    try:
        assert server.resource_version() == restored
        for stale in ("0", "3"):
            with pytest.raises(ExpiredError):
                server.events_since(*CM, None, stale)
        assert server.events_since(*CM, None, restored) == []

        async def subscribe_and_write():
            sub = server.watch(*CM)
            made = server.create({"apiVersion": CM[0], "kind": CM[1],
                                  "metadata": {"name": "new", "namespace": NS}})
            ev = await asyncio.wait_for(sub.__anext__(), 5)
            sub.close()
            return made, ev

        made, live = run(subscribe_and_write())
        assert live["type"] == "ADDED" and live["object"]["metadata"]["name"] == "new"
        assert int(made["metadata"]["resourceVersion"]) > max(old_rvs + [int(restored)])
        replay = server.events_since(*CM, None, restored)
        assert [(e["type"], e["object"]["metadata"]["name"]) for e in replay] == [
            ("ADDED", "new")]
    finally:
        server.close()


_CHILD_OPEN = """
import sys
from active_monitor_amd.kube import MemoryApiServer
from active_monitor_amd.kube.persist import StoreLockedError
try:
    s = MemoryApiServer.open(sys.argv[1])
except StoreLockedError as e:
    print("LOCKED", e)
    sys.exit(3)
print("OPENED", len(s))
s.close()
"""


def test_second_process_cannot_open_a_held_directory(tmp_path):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    server.create({"apiVersion": CM[0], "kind": CM[1],
                   "metadata": {"name": "one", "namespace": NS}})

    def child():
        return subprocess.run([sys.executable, "-c", _CHILD_OPEN, d], cwd=REPO,
                              capture_output=True, text=True, timeout=60)

    held = child()
    assert held.returncode == 3, held.stderr
    assert "LOCKED" in held.stdout and d in held.stdout
    # the same process cannot open it twice either
    with pytest.raises(StoreLockedError):
        MemoryApiServer.open(d)
    server.close()
    server.close()  # idempotent
    freed = child()
    assert freed.returncode == 0, freed.stderr
    assert freed.stdout.strip() == "OPENED 1"


def test_writes_after_close_fail_loudly(tmp_path):
    server = MemoryApiServer.open(str(tmp_path / "store"))
    server.close()
    with pytest.raises(persist.StoreError):
        server.create({"apiVersion": CM[0], "kind": CM[1],
                       "metadata": {"name": "late", "namespace": NS}})


def test_store_without_a_directory_touches_no_file(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    opened = []
    real_open = builtins.open

    def spy_open(file, *a, **kw):
        opened.append(file)
        return real_open(file, *a, **kw)

    def forbidden(*a, **kw):
        raise AssertionError("the persistence module was called")

    monkeypatch.setattr(builtins, "open", spy_open)
    monkeypatch.setattr(persist, "Journal", forbidden)
    monkeypatch.setattr(persist, "_dumps", forbidden)
    monkeypatch.setattr(os, "fsync", forbidden)

    server = MemoryApiServer()
    assert server.data_dir is None
    Driver(server, seed=1).step(150)
    server.max_events = 2
    for i in range(4):
        server.create(_event(f"ev-{i}"))
    server.close()  # a no-op without a directory
    server.create(_event("still-works"))

    assert opened == []
    assert list(tmp_path.iterdir()) == []


def test_journal_record_is_on_disk_before_a_watcher_sees_the_event(tmp_path, run):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    journal = os.path.join(d, JOURNAL_FILE)
    seen = []

    class Probe:
        def _offer(self, event):
            with open(journal, "rb") as f:
                seen.append((event["object"]["metadata"]["name"], f.read()))

    server._subs.append(Probe())
    try:
        server.create({"apiVersion": CM[0], "kind": CM[1],
                       "metadata": {"name": "probe", "namespace": NS}})
    finally:
        server._subs.clear()
        server.close()
    (name, on_disk), = seen
    assert name == "probe"
    rec = json.loads(on_disk.split(b"\n")[0])
    assert rec["op"] == "put" and rec["obj"]["metadata"]["name"] == "probe"


def test_api_errors_leave_no_record(tmp_path):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    server.create({"apiVersion": CM[0], "kind": CM[1],
                   "metadata": {"name": "one", "namespace": NS}})
    with pytest.raises(ApiError):
        server.create({"apiVersion": CM[0], "kind": CM[1],
                       "metadata": {"name": "one", "namespace": NS}})
    with pytest.raises(ApiError):
        server.delete(*CM, NS, "absent")
    assert server._journal.records == 1
    server.close()


def test_journal_write_error_stops_all_further_writes(tmp_path):
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    server.create({"apiVersion": CM[0], "kind": CM[1],
                   "metadata": {"name": "kept", "namespace": NS}})
    journaled = dump(server)
    real_file = server._journal._file

    class FullDisk:
        def write(self, data):
            raise OSError(28, "No space left on device")

        def __getattr__(self, name):
            return getattr(real_file, name)

    server._journal._file = FullDisk()
    with pytest.raises(OSError):
        server.create({"apiVersion": CM[0], "kind": CM[1],
                       "metadata": {"name": "lost", "namespace": NS}})
    # the disk "recovers", but a record is missing: nothing may follow it
    server._journal._file = real_file
    with pytest.raises(persist.StoreError) as err:
        server.create({"apiVersion": CM[0], "kind": CM[1],
                       "metadata": {"name": "later", "namespace": NS}})
    assert "restart" in str(err.value) and d in str(err.value)
    server.close()

    server = MemoryApiServer.open(d)  # the restart: the last journaled state
    try:
        assert dump(server) == journaled
    finally:
        server.close()


def test_event_cap_counts_only_live_events_after_reopen(tmp_path):
    """A running store keeps the keys of deleted Events queued, so its cap
    bites earlier; a reloaded store counts the live ones (documented on
    MemoryApiServer.open)."""
    d = str(tmp_path / "store")
    server = MemoryApiServer.open(d)
    server.max_events = 4
    for i in range(4):
        server.create(_event(f"ev-{i}"))
    server.delete(*EV, NS, "ev-1")
    server.delete(*EV, NS, "ev-2")
    server.close()

    server = MemoryApiServer.open(d)
    server.max_events = 4
    try:
        assert list(server._event_keys) == [EV + (NS, "ev-0"), EV + (NS, "ev-3")]
        server.create(_event("ev-4"))
        server.create(_event("ev-5"))  # four live Events: nothing evicted yet
        names = [e["metadata"]["name"] for e in server.list(*EV)]
        assert names == ["ev-0", "ev-3", "ev-4", "ev-5"]
        server.create(_event("ev-6"))
        names = [e["metadata"]["name"] for e in server.list(*EV)]
        assert names == ["ev-3", "ev-4", "ev-5", "ev-6"]
    finally:
        server.close()


def test_new_journal_directory_entry_is_synced(tmp_path, monkeypatch):
    synced = []
    monkeypatch.setattr(persist, "_fsync_dir", synced.append)
    d = str(tmp_path / "store")
    MemoryApiServer.open(d).close()
    assert synced == [d]
    MemoryApiServer.open(d).close()  # the journal exists now
    assert synced == [d]

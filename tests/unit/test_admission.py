"""The admission policy on its own: queue order, the two limits, mutexes,
removal. No engine, no event loop, no process.
"""
import random

import pytest

from active_monitor_amd.workflow import POSTPONED_MESSAGE, engines
from active_monitor_amd.workflow.admission import Admission, mutex_names


def sync(*names):
    return {"synchronization": {"mutexes": [{"name": n} for n in names]}}


def keys(entries):
    return [e.key for e in entries]


def offer(adm, key, spec=None, created="", ns=None):
    return adm.offer(key, ns if ns is not None else key.split("/")[0], spec or {}, created)


def test_the_names_stay_importable_from_engines():
    assert engines.mutex_names is mutex_names
    assert engines.POSTPONED_MESSAGE is POSTPONED_MESSAGE
    assert engines._positive("parallelism", None) is None
    assert engines._priority({"priority": "7"}) == 7
    assert engines.QUEUE_EXPIRED_MESSAGE == "deadline exceeded while waiting to start"


@pytest.mark.parametrize("value", [0, -1, True, 1.5, "2"])
def test_limits_are_positive_integers(value):
    with pytest.raises(ValueError) as e:
        Admission(parallelism=value)
    assert str(e.value) == f"parallelism must be a positive integer, got {value!r}"
    with pytest.raises(ValueError) as e:
        Admission(namespace_parallelism=value)
    assert str(e.value) == f"namespace_parallelism must be a positive integer, got {value!r}"


def test_priority_beats_age_and_age_beats_arrival():
    adm = Admission(parallelism=1)
    offer(adm, "a/blocker")
    assert keys(adm.admit()) == ["a/blocker"]
    offer(adm, "a/young", created="2024-05-01T10:00:07Z")
    offer(adm, "a/old", created="2024-05-01T10:00:03Z")
    offer(adm, "a/urgent", {"priority": 5}, created="2024-05-01T10:00:09Z")
    offer(adm, "a/low", {"priority": -1}, created="2024-05-01T10:00:01Z")
    assert keys(adm) == ["a/urgent", "a/old", "a/young", "a/low"]
    assert len(adm) == 4
    assert adm.admit() == []


def test_equal_priority_and_timestamp_fall_back_to_arrival():
    adm = Admission(parallelism=1)
    for name in ("a/first", "a/second", "a/third"):
        offer(adm, name, {"priority": 2}, created="2024-05-01T10:00:00Z")
    assert keys(adm) == ["a/first", "a/second", "a/third"]


def test_a_priority_that_is_no_integer_counts_as_zero():
    adm = Admission(parallelism=1)
    offer(adm, "a/junk", {"priority": "high"}, created="2")
    offer(adm, "a/list", {"priority": [3]}, created="3")
    offer(adm, "a/zero", {"priority": 0}, created="1")
    offer(adm, "a/one", {"priority": 1}, created="9")
    assert keys(adm) == ["a/one", "a/zero", "a/junk", "a/list"]


def test_a_full_namespace_is_passed_over():
    adm = Admission(namespace_parallelism=1)
    a1, a2, b1 = offer(adm, "a/1"), offer(adm, "a/2"), offer(adm, "b/1")
    assert adm.admit() == [a1, b1]
    assert keys(adm) == ["a/2"]
    assert adm.blocked_by(a2) == POSTPONED_MESSAGE
    adm.release(b1)
    assert adm.admit() == []
    adm.release(a1)
    assert adm.admit() == [a2]


def test_the_entry_behind_one_that_waits_for_a_mutex_is_admitted():
    adm = Admission(parallelism=5)
    holder = offer(adm, "a/holder", sync("gpu0"))
    assert adm.admit() == [holder]
    waits = offer(adm, "a/waits", sync("gpu0"))
    free = offer(adm, "a/free", sync("gpu1"))
    elsewhere = offer(adm, "b/elsewhere", sync("gpu0"))  # a mutex is its namespace's
    assert adm.admit() == [free, elsewhere]
    assert adm.blocked_by(waits) == "Waiting for a/Mutex/gpu0 lock"
    adm.release(holder)
    assert adm.admit() == [waits]


def test_the_global_limit_ends_the_scan():
    adm = Admission(parallelism=1, namespace_parallelism=1)
    head, behind = offer(adm, "a/head"), offer(adm, "b/behind")
    assert adm.admit() == [head]
    assert adm.blocked_by(behind) == POSTPONED_MESSAGE
    assert adm.admit() == []
    adm.release(head)
    assert adm.admit() == [behind]


def test_mutexes_are_taken_all_or_none():
    adm = Admission()
    holder = offer(adm, "a/holder", sync("m2"))
    assert adm.admit() == [holder]
    both = offer(adm, "a/both", sync("m1", "m2"))
    assert adm.admit() == []
    assert adm.blocked_by(both) == "Waiting for a/Mutex/m2 lock"
    # m1 was not taken meanwhile
    first = offer(adm, "a/first", sync("m1"))
    assert adm.admit() == [first]
    adm.release(first)
    adm.release(holder)
    assert adm.admit() == [both]
    later = offer(adm, "a/later", sync("m1"))
    assert adm.admit() == []
    assert adm.blocked_by(later) == "Waiting for a/Mutex/m1 lock"
    wants_two = offer(adm, "a/two", sync("m2", "m1"))
    assert adm.blocked_by(wants_two) == "Waiting for a/Mutex/m2 lock"  # its own order


def test_removal_frees_nothing_and_admits_nothing():
    adm = Admission(parallelism=1)
    running, doomed, nxt = offer(adm, "a/running"), offer(adm, "a/doomed"), offer(adm, "a/next")
    assert adm.admit() == [running]
    assert adm.remove("a/doomed") is doomed
    assert keys(adm) == ["a/next"]
    assert adm.admit() == []
    assert adm.remove("a/doomed") is None
    assert adm.remove("a/never-seen") is None
    assert adm.remove("a/running") is None  # admitted: no longer in the queue
    assert keys(adm) == ["a/next"]
    adm.release(running)
    assert adm.admit() == [nxt]


def test_a_queued_key_offered_twice_keeps_one_entry():
    adm = Admission(parallelism=1)
    assert adm.admit() == [] and len(adm) == 0
    blocker = offer(adm, "a/blocker")
    adm.admit()
    once = offer(adm, "a/x", created="5")
    again = offer(adm, "a/x", {"priority": 9}, created="1")
    assert again is once
    assert keys(adm) == ["a/x"]
    adm.release(blocker)
    assert adm.admit() == [once]
    assert adm.admit() == []


def test_without_limits_or_mutexes_a_workflow_runs_at_once():
    adm = Admission()
    assert offer(adm, "a/x") is None
    assert offer(adm, "a/y", {"priority": 3}) is None
    assert offer(adm, "a/z", {"synchronization": {"semaphore": {}}}) is None
    assert offer(adm, "a/junk", "not a spec") is None
    assert len(adm) == 0 and adm.admit() == []


def test_without_limits_a_mutex_still_excludes():
    adm = Admission()
    one = offer(adm, "a/one", {"synchronization": {"mutex": {"name": "gpu0"}}})
    assert adm.admit() == [one]
    two = offer(adm, "a/two", sync("gpu0"))
    assert adm.admit() == []
    assert adm.blocked_by(two) == "Waiting for a/Mutex/gpu0 lock"
    assert offer(adm, "a/unbounded") is None
    adm.release(one)
    assert adm.admit() == [two]


def test_mutex_names():
    assert mutex_names({"synchronization": {
        "mutex": {"name": "a"},
        "mutexes": [{"name": "b"}, {"name": "a"}, {"name": "c"}, {"name": "b"}]}}) == ["a", "b", "c"]
    assert mutex_names({"synchronization": {"mutexes": [{"name": "z"}, {"name": 3}]}}) == ["z", "3"]
    assert mutex_names({"synchronization": {"mutex": {"name": ""}, "mutexes": "m"}}) == []
    assert mutex_names({"synchronization": {"mutex": "m", "mutexes": [None, 5, {"nome": "x"}]}}) == []
    for junk in (None, 5, "spec", [], {}, {"synchronization": None},
                 {"synchronization": ["mutex"]}, {"synchronization": "mutex"}):
        assert mutex_names(junk) == []


@pytest.mark.parametrize("seed", range(200))
def test_random_operations_keep_the_invariants(seed):
    rng = random.Random(seed)
    parallelism = rng.choice([None, 1, 2, 3])
    ns_parallelism = rng.choice([None, 1, 2])
    adm = Admission(parallelism, ns_parallelism)
    admitted = []
    serial = 0
    for _ in range(rng.randint(1, 60)):
        op = rng.choice(["offer", "offer", "release", "remove"])
        if op == "offer":
            serial += 1
            ns = rng.choice(["a", "b"])
            # now and then a key that may be queued already
            name = rng.randint(1, serial) if rng.random() < 0.1 else serial
            spec = {"priority": rng.choice([0, 0, 1, 5])}
            wanted = rng.sample(["m1", "m2"], rng.randint(0, 2))
            if wanted:
                spec.update(sync(*wanted))
            entry = adm.offer(f"{ns}/w{name}", ns, spec, f"t{rng.randint(0, 9)}")
            if entry is None:
                assert parallelism is None and ns_parallelism is None and not wanted
        elif op == "release" and admitted:
            adm.release(admitted.pop(rng.randrange(len(admitted))))
        elif op == "remove" and len(adm):
            gone = rng.choice(list(adm))
            assert adm.remove(gone.key) is gone

        before = list(adm)
        now = adm.admit()
        admitted += now

        # among those admitted in one call, queue order is kept
        assert now == [e for e in before if e in now]
        assert list(adm) == [e for e in before if e not in now]
        if parallelism is not None:
            assert len(admitted) <= parallelism
        if ns_parallelism is not None:
            for ns in ("a", "b"):
                assert sum(1 for e in admitted if e.ns == ns) <= ns_parallelism
        held = [m for e in admitted for m in e.mutexes]
        assert len(held) == len(set(held))
        assert all(ns == e.ns for e in admitted for ns, _ in e.mutexes)
        # work-conserving: short of the global limit, whatever waits is blocked
        if parallelism is None or len(admitted) < parallelism:
            assert all(adm.blocked_by(e) is not None for e in adm)
        queue = list(adm)
        assert [e.order for e in queue] == sorted(e.order for e in queue)
        assert len({e.key for e in queue}) == len(queue) == len(adm)

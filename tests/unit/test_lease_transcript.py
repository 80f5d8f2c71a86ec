"""Every read and write the two lease users make, for a fixed clock.

LeaderElector and ShardCoordinator both live on coordination.k8s.io Leases.
These tests hold the clock still and record each ``get``/``create``/``update``
on a Lease together with the spec it wrote, so the rules that decide who
drives what (expiry, the preferredHolder window, the three kinds of release)
are pinned as whole transcripts rather than as end states."""
import time

import pytest

from active_monitor_amd.engine.leader import LeaderElector
from active_monitor_amd.engine.shards import LEASE_API_VERSION, ShardCoordinator
from active_monitor_amd.kube import MemoryApiServer, MemoryClient
from active_monitor_amd.kube.errors import NotFoundError

T = 1_700_000_000.5  # the fractional half makes every age exact
NOW = "2023-11-14T22:13:20Z"  # what k8s_now() writes at T
AGO_3 = "2023-11-14T22:13:17Z"  # 3.5 s old at T
AGO_10 = "2023-11-14T22:13:10Z"  # 10.5 s old at T
AGO_11 = "2023-11-14T22:13:09Z"  # 11.5 s old at T
NS = "health"
LEADER = "689451f8.keikoproj.io"
SHARD0 = "active-monitor-shard-0-of-2"
SHARD1 = "active-monitor-shard-1-of-2"


class RecordingClient(MemoryClient):
    """Notes ``(verb, lease name, spec as written)``; a read writes nothing,
    so it records None."""

    def __init__(self, server):
        super().__init__(server)
        self.calls = []

    async def get(self, api_version, kind, namespace, name, **kw):
        if kind == "Lease":
            self.calls.append(("get", name, None))
        return await super().get(api_version, kind, namespace, name, **kw)

    async def create(self, obj, *a, **kw):
        if obj.get("kind") == "Lease":
            self.calls.append(("create", obj["metadata"]["name"], dict(obj["spec"])))
        return await super().create(obj, *a, **kw)

    async def update(self, obj, *a, **kw):
        if obj.get("kind") == "Lease":
            self.calls.append(("update", obj["metadata"]["name"], dict(obj["spec"])))
        return await super().update(obj, *a, **kw)

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture
def frozen(monkeypatch):
    monkeypatch.setattr(time, "time", lambda: T)
    monkeypatch.delenv("AM_LEADER_LEASE_SECS", raising=False)
    monkeypatch.delenv("AM_LEADER_RENEW_SECS", raising=False)


def seed(server, name, **spec):
    server.create({"apiVersion": LEASE_API_VERSION, "kind": "Lease",
                   "metadata": {"name": name, "namespace": NS}, "spec": spec})


def stored(server, name):
    return server.get(LEASE_API_VERSION, "Lease", NS, name)["spec"]


def held(holder, secs, renew=NOW, **extra):
    return {"holderIdentity": holder, "leaseDurationSeconds": secs,
            "renewTime": renew, **extra}


def elector(server, identity="me", **kw):
    client = RecordingClient(server)
    return client, LeaderElector(client, LEADER, NS, identity, **kw)


def coord(server, identity, home=0, lease=10.0):
    client = RecordingClient(server)
    return client, ShardCoordinator(
        client, namespace=NS, shard_index=home, shard_count=2, identity=identity,
        lease_duration=lease, renew_interval=0.1)


# -- leader -----------------------------------------------------------------


def test_leader_creates_an_absent_lease_then_renews_it(run, frozen):
    async def go():
        server = MemoryApiServer()
        client, el = elector(server)
        assert await el.try_acquire() is True
        assert el.is_leader is True
        assert client.take() == [("get", LEADER, None),
                                 ("create", LEADER, held("me", 15))]
        assert await el.try_acquire() is True
        assert client.take() == [("get", LEADER, None),
                                 ("update", LEADER, held("me", 15))]

    run(go(), timeout=20)


def test_leader_refuses_a_live_foreign_holder(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, LEADER, **held("other", 15))
        client, el = elector(server)
        assert await el.try_acquire() is False
        assert el.is_leader is False
        assert client.take() == [("get", LEADER, None)]
        assert stored(server, LEADER) == held("other", 15)

    run(go(), timeout=20)


def test_leader_takes_an_empty_holder_whatever_the_renew_time(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, LEADER, **held("", 15))  # renewed this very second
        client, el = elector(server)
        assert await el.try_acquire() is True
        assert el.is_leader is True
        assert client.take() == [("get", LEADER, None),
                                 ("update", LEADER, held("me", 15))]

    run(go(), timeout=20)


def test_leader_expiry_has_no_pad(run, frozen):
    """A foreign lease of 10 s that is 10.5 s old is taken: the leader's
    window is exactly ``lease_duration``."""

    async def go():
        server = MemoryApiServer()
        seed(server, LEADER, **held("other", 10, AGO_10))
        client, el = elector(server, lease_duration=10.0)
        assert await el.try_acquire() is True
        assert client.take() == [("get", LEADER, None),
                                 ("update", LEADER, held("me", 10))]

    run(go(), timeout=20)


def test_leader_release_blanks_the_holder_and_keeps_renew_time(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, LEADER, **held("me", 15, AGO_3))
        client, el = elector(server)
        el.is_leader = True
        assert await el.release() is None
        assert el.is_leader is False
        assert client.take() == [("get", LEADER, None),
                                 ("update", LEADER, held("", 15, AGO_3))]
        # not the leader any more: a second release does not even read
        await el.release()
        assert client.take() == []

    run(go(), timeout=20)


def test_leader_release_leaves_a_foreign_lease_alone(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, LEADER, **held("other", 15))
        client, el = elector(server)
        el.is_leader = True  # deposed without having noticed yet
        await el.release()
        assert el.is_leader is False
        assert client.take() == [("get", LEADER, None)]
        assert stored(server, LEADER) == held("other", 15)

    run(go(), timeout=20)


def test_leader_environment_overrides_the_arguments(run, frozen, monkeypatch):
    monkeypatch.setenv("AM_LEADER_LEASE_SECS", "7")
    monkeypatch.setenv("AM_LEADER_RENEW_SECS", "0.5")

    async def go():
        server = MemoryApiServer()
        client, el = elector(server, lease_duration=30.0, renew_interval=10.0,
                             retry_interval=2.0)
        assert (el.lease_duration, el.renew_interval, el.retry_interval) == (7.0, 0.5, 0.5)
        assert await el.try_acquire() is True
        assert client.take() == [("get", LEADER, None),
                                 ("create", LEADER, held("me", 7))]

    run(go(), timeout=20)


def test_leader_reads_durations_set_after_construction(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, LEADER, **held("other", 15, AGO_3))
        client, el = elector(server)
        assert await el.try_acquire() is False
        el.lease_duration = 3.0  # 3.5 s old: expired by the new duration
        assert await el.try_acquire() is True
        assert client.take() == [("get", LEADER, None), ("get", LEADER, None),
                                 ("update", LEADER, held("me", 3))]

    run(go(), timeout=20)


# -- shards -----------------------------------------------------------------


def test_shard_expiry_is_padded_by_one_second(run, frozen):
    """The same 10 s lease that the leader takes at 10.5 s is refused by a
    shard coordinator, and taken at 11.5 s: lease timestamps have whole-second
    resolution, so the shard window is ``lease_duration + 1``."""

    async def go():
        server = MemoryApiServer()
        seed(server, SHARD1, **held("dead", 10, AGO_10))
        client, a = coord(server, "proc-a")
        assert await a._try_acquire(1) is False
        assert client.take() == [("get", SHARD1, None)]

        lease = server.get(LEASE_API_VERSION, "Lease", NS, SHARD1)
        lease["spec"]["renewTime"] = AGO_11
        server.update(lease)
        assert await a._try_acquire(1) is True
        assert client.take() == [("get", SHARD1, None),
                                 ("update", SHARD1, held("proc-a", 10))]

    run(go(), timeout=20)


def test_shard_creates_an_absent_lease(run, frozen):
    async def go():
        server = MemoryApiServer()
        client, a = coord(server, "proc-a")
        assert await a._try_acquire(0) is True
        assert client.take() == [("get", SHARD0, None),
                                 ("create", SHARD0, held("proc-a", 10))]

    run(go(), timeout=20)


def test_preferred_holder_window_admits_only_the_preferred(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD1, **held("", 10, preferredHolder="proc-a"))
        c_client, c = coord(server, "proc-c")
        assert await c._try_acquire(1) is False
        assert c_client.take() == [("get", SHARD1, None)]

        a_client, a = coord(server, "proc-a", home=1)
        assert await a._try_acquire(1) is True
        # the preferred owner's own write clears the marker
        assert a_client.take() == [("get", SHARD1, None),
                                   ("update", SHARD1, held("proc-a", 10))]
        assert stored(server, SHARD1) == held("proc-a", 10)

    run(go(), timeout=20)


def test_third_party_keeps_a_pending_preferred_holder(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD1, **held("dead", 10, AGO_11, preferredHolder="proc-a"))
        client, c = coord(server, "proc-c")
        assert await c._try_acquire(1) is True
        assert client.take() == [
            ("get", SHARD1, None),
            ("update", SHARD1, held("proc-c", 10, preferredHolder="proc-a"))]

    run(go(), timeout=20)


def test_renew_of_an_adopted_shard_honours_a_reclaim(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD1, **held("proc-b", 10, AGO_3, preferredHolder="proc-a"))
        client, b = coord(server, "proc-b", home=0)
        b.owned.add(1)
        assert await b._renew_owned(1) is False
        # holder blanked, renewTime stamped: the preferred owner's window opens now
        assert client.take() == [
            ("get", SHARD1, None),
            ("update", SHARD1, held("", 10, NOW, preferredHolder="proc-a"))]

    run(go(), timeout=20)


def test_renew_of_the_home_shard_ignores_a_reclaim(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD0, **held("proc-a", 10, AGO_3, preferredHolder="intruder"))
        client, a = coord(server, "proc-a", home=0)
        a.owned.add(0)
        assert await a._renew_owned(0) is True
        assert client.take() == [
            ("get", SHARD0, None),
            ("update", SHARD0, held("proc-a", 10, NOW, preferredHolder="intruder"))]

    run(go(), timeout=20)


def test_renew_clears_a_satisfied_reclaim(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD0, **held("proc-a", 10, AGO_3, preferredHolder="proc-a"))
        client, a = coord(server, "proc-a", home=0)
        assert await a._renew_owned(0) is True
        assert client.take() == [("get", SHARD0, None),
                                 ("update", SHARD0, held("proc-a", 10, NOW))]

    run(go(), timeout=20)


def test_renew_of_a_lease_someone_took_writes_nothing(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD1, **held("proc-c", 10))
        client, b = coord(server, "proc-b")
        assert await b._renew_owned(1) is False
        assert client.take() == [("get", SHARD1, None)]

    run(go(), timeout=20)


def test_renew_of_a_vanished_lease_falls_through_to_acquire(run, frozen):
    async def go():
        server = MemoryApiServer()
        client, a = coord(server, "proc-a")
        assert await a._renew_owned(0) is True
        assert client.take() == [("get", SHARD0, None), ("get", SHARD0, None),
                                 ("create", SHARD0, held("proc-a", 10))]

    run(go(), timeout=20)


def test_stop_frees_every_owned_shard_at_once(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD0, **held("proc-a", 10))
        seed(server, SHARD1, **held("proc-a", 10, AGO_3, preferredHolder="proc-b"))
        client, a = coord(server, "proc-a")
        a.owned.update({0, 1})
        assert await a.stop() is None
        assert a.owned == set()
        # renewTime removed: no window, the lease is free this instant
        free = {"holderIdentity": "", "leaseDurationSeconds": 10}
        assert client.take() == [
            ("get", SHARD0, None), ("update", SHARD0, free),
            ("get", SHARD1, None),
            ("update", SHARD1, {**free, "preferredHolder": "proc-b"})]

    run(go(), timeout=20)


def test_stop_leaves_a_lease_it_no_longer_holds(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD0, **held("proc-c", 10))
        client, a = coord(server, "proc-a")
        a.owned.add(0)
        await a.stop()
        assert client.take() == [("get", SHARD0, None)]
        assert stored(server, SHARD0) == held("proc-c", 10)

    run(go(), timeout=20)


def test_request_reclaim_writes_once(run, frozen):
    async def go():
        server = MemoryApiServer()
        seed(server, SHARD0, **held("proc-b", 10, AGO_3))
        client, a = coord(server, "proc-a", home=0)
        assert await a._request_reclaim(0) is None
        assert client.take() == [
            ("get", SHARD0, None),
            ("update", SHARD0, held("proc-b", 10, AGO_3, preferredHolder="proc-a"))]
        await a._request_reclaim(0)
        assert client.take() == [("get", SHARD0, None)]
        # and on a lease that is gone it does nothing at all
        server.delete(LEASE_API_VERSION, "Lease", NS, SHARD0)
        await a._request_reclaim(0)
        assert client.take() == [("get", SHARD0, None)]
        with pytest.raises(NotFoundError):
            server.get(LEASE_API_VERSION, "Lease", NS, SHARD0)

    run(go(), timeout=20)

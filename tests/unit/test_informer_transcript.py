"""What the manager's informer puts into its cache and its queue.

A Manager without workers runs over a MemoryApiServer split in two shards, so
nothing but the informer paths (initial list, watch events, shard adoption,
shard drop, resync) touches ``queue.add``; each call is recorded in order.
Reads served from the cache in steady state, the healing of a lost DELETED
event end to end and the read-your-writes floor are pinned by
tests/integration/test_read_caching.py and are not repeated here."""
import asyncio

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.engine.reconciler import CACHE_MISS
from active_monitor_amd.engine.shards import shard_of
from active_monitor_amd.kube import MemoryApiServer, MemoryClient

NS = "health"
HC = (API_VERSION, "HealthCheck")
_names = [f"hc-{i:02d}" for i in range(40)]
S0 = [n for n in _names if shard_of(n, 2) == 0][:4]  # shard 0's names
S1 = [n for n in _names if shard_of(n, 2) == 1][:4]  # shard 1's names


def hc(name, repeat=3600):
    return {"apiVersion": API_VERSION, "kind": "HealthCheck",
            "metadata": {"name": name, "namespace": NS},
            "spec": {"repeatAfterSec": repeat, "level": "cluster"}}


def keys(*names):
    return [(NS, n) for n in names]


class ListControlClient(MemoryClient):
    """``list`` waits while ``gate`` is clear, can let exactly one call
    through (``one_shot``) and can leave named objects out of its answer."""

    def __init__(self, server):
        super().__init__(server)
        self.gate = asyncio.Event()
        self.gate.set()
        self.one_shot = False
        self.parked = 0
        self.hidden = set()

    async def list(self, *a, **kw):
        if not self.gate.is_set():
            self.parked += 1
        await self.gate.wait()
        if self.one_shot:
            self.gate.clear()
        return [o for o in await super().list(*a, **kw)
                if o["metadata"]["name"] not in self.hidden]


def manager(client, **kw):
    m = Manager(client, max_workers=0, shard_index=0, shard_count=2,
                enable_wf_hub=False, **{"resync_period": 0, **kw})
    adds = []
    real_add = m.queue.add

    async def add(key, flags=None):
        adds.append(key)
        await real_add(key, flags)

    m.queue.add = add
    return m, adds


async def until(pred, msg):
    deadline = asyncio.get_running_loop().time() + 10
    while not pred():
        assert asyncio.get_running_loop().time() < deadline, f"timed out: {msg}"
        await asyncio.sleep(0.005)


def test_static_shard_list_then_events(run):
    async def go():
        server = MemoryApiServer()
        client = ListControlClient(server)
        for name in (S0[0], S1[0], S0[1]):
            server.create(hc(name))
        m, adds = manager(client)
        client.gate.clear()
        await m.start()
        try:
            await until(lambda: client.parked == 1, "informer reaches its list")
            # the initial list has not completed: the cache cannot answer yet
            assert m._cache_lookup(NS, S0[0]) is CACHE_MISS
            assert adds == [] and m.hc_cache == {}
            # created between subscribe and list: in the list AND an event
            server.create(hc(S0[2]))
            client.gate.set()
            await until(lambda: len(adds) == 4, "list and the queued event")
            assert adds == keys(S0[0], S0[1], S0[2], S0[2])
            assert list(m.hc_cache) == keys(S0[0], S0[1], S0[2])
            assert m._cache_synced is True
            lookup = m.reconciler.hc_lookup
            assert lookup(NS, S0[0]) == server.get(*HC, NS, S0[0])
            assert lookup(NS, S1[0]) is None  # synced, and not ours
            del adds[:]

            # MODIFIED: cache replaced before the key is queued
            obj = server.get(*HC, NS, S0[0])
            obj["spec"]["repeatAfterSec"] = 60
            new = server.update(obj)
            await until(lambda: len(adds) == 1, "MODIFIED")
            assert adds == keys(S0[0])
            assert m.hc_cache[(NS, S0[0])] == new

            # DELETED: cache entry removed, key queued
            server.delete(*HC, NS, S0[0])
            await until(lambda: len(adds) == 2, "DELETED")
            assert adds == keys(S0[0], S0[0])
            assert (NS, S0[0]) not in m.hc_cache

            # events for the other shard's keys leave no trace; the owned
            # event behind them on the same stream shows they were consumed
            server.create(hc(S1[1]))
            server.delete(*HC, NS, S1[0])
            server.create(hc(S0[3]))
            await until(lambda: len(adds) == 3, "ADDED after foreign events")
            assert adds == keys(S0[0], S0[0], S0[3])
            assert list(m.hc_cache) == keys(S0[1], S0[2], S0[3])
        finally:
            await m.stop()

    run(go(), timeout=30)


def test_one_resync_pass(run):
    async def go():
        server = MemoryApiServer()
        client = ListControlClient(server)
        for name in (S0[0], S1[0], S0[1], S0[2]):
            server.create(hc(name))
        m, adds = manager(client)
        await m.start()
        task = None
        try:
            await until(lambda: m._cache_synced, "initial list")
            assert adds == keys(S0[0], S0[1], S0[2])
            del adds[:]
            # a cache entry whose DELETED event was lost ...
            m.hc_cache[(NS, "ghost")] = hc("ghost")
            # ... and a live one that the list snapshot will miss
            stale = dict(m.hc_cache[(NS, S0[2])], spec="stale")
            m.hc_cache[(NS, S0[2])] = stale
            client.hidden = {S0[2]}
            gets = server.op_counts["get"]

            client.one_shot = True  # the second pass parks at its list
            m.resync_period = 0.01
            task = asyncio.ensure_future(m._resync_loop())
            await until(lambda: client.parked == 1, "one full pass")
            # one verifying read per suspect, none for a listed key
            assert server.op_counts["get"] - gets == 2
            # live keys in list order, then the reaped key
            assert adds == keys(S0[0], S0[1], "ghost")
            assert (NS, "ghost") not in m.hc_cache
            assert m.hc_cache[(NS, S0[2])] == server.get(*HC, NS, S0[2])
            assert m.hc_cache[(NS, S0[2])] != stale
            assert (NS, S1[0]) not in m.hc_cache
        finally:
            if task is not None:
                task.cancel()
            await m.stop()

    run(go(), timeout=30)


def test_shard_ha_adopt_and_drop(run):
    async def go():
        server = MemoryApiServer()
        client = ListControlClient(server)
        for name in (S0[0], S1[0], S0[1], S1[1]):
            server.create(hc(name))
        m, adds = manager(client, shard_ha=True, leader_identity="mgr-0",
                          shard_lease_duration=1.2, shard_renew_interval=0.15)
        await m.start()
        try:
            # home shard from the initial list, then the coordinator's first
            # scan finds shard 1 unheld and adopts it through the callback
            await until(lambda: m.coordinator.owned == {0, 1} and len(adds) == 4,
                        "adoption of the unheld shard")
            assert adds == keys(S0[0], S0[1], S1[0], S1[1])
            assert sorted(m.hc_cache) == sorted(keys(S0[0], S0[1], S1[0], S1[1]))
            m.coordinator.crash()  # no more scans: the test drives the callbacks
            await asyncio.sleep(0)
            del adds[:]

            rec = m.reconciler
            watches = {}
            for name in (S0[0], S1[0], S1[1]):
                rec._arm_repeat_timer(name, NS, 3600)
                watches[name] = rec._spawn_watch((NS, name), asyncio.sleep(3600))

            # the rightful owner took shard 1 back
            m.coordinator.owned.discard(1)
            await m._drop_shard(1)
            await asyncio.sleep(0)
            assert sorted(m.hc_cache) == sorted(keys(S0[0], S0[1]))
            assert list(rec.repeat_timers_by_name) == keys(S0[0])
            assert watches[S1[0]].cancelled() and watches[S1[1]].cancelled()
            assert not watches[S0[0]].done()
            assert adds == []

            # its events are now someone else's
            obj = server.get(*HC, NS, S1[0])
            obj["spec"]["repeatAfterSec"] = 60
            server.update(obj)
            server.delete(*HC, NS, S0[1])
            await until(lambda: len(adds) == 1, "owned event after a foreign one")
            assert adds == keys(S0[1])
            assert sorted(m.hc_cache) == sorted(keys(S0[0]))
            del adds[:]

            # adoption surfaces shard 1's keys only, not what is already held
            m.coordinator.owned.add(1)
            await m._adopt_shard(1)
            assert adds == keys(S1[0], S1[1])
            assert sorted(m.hc_cache) == sorted(keys(S0[0], S1[0], S1[1]))
            assert m.hc_cache[(NS, S1[0])]["spec"]["repeatAfterSec"] == 60
        finally:
            await m.stop()

    run(go(), timeout=30)

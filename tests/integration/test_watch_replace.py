"""Replace semantics of the HTTP watch: what a re-list after 410 Gone tells
its consumer about objects that are no longer there.

client-go's reflector (which the reference gets through controller-runtime,
healthcheck_controller.go:133) turns the re-list into a Replace: a key known
before and absent from the fresh list is delivered as a deletion. These tests
make a watch miss deletions deterministically — the listener is stopped, the
store is changed directly, the event history is compacted, a new listener
starts on the same port — and read what the subscription then delivers.
"""
import asyncio
import random

from active_monitor_amd import API_VERSION
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.memory import MemoryApiServer
from active_monitor_amd.kube.server import ApiServerFrontend

from .conftest import make_hc

KIND = "HealthCheck"


class Env:
    async def __aenter__(self):
        self.server = MemoryApiServer()
        self.frontend = ApiServerFrontend(self.server)
        await self.frontend.start()
        self.port = self.frontend.port
        self.client = HttpClient(self.frontend.url, qps=0)
        await self.client.start()
        self.subs = []
        self._readers = []
        return self

    async def __aexit__(self, *exc):
        for sub in self.subs:
            sub.close()
        for task in self._readers:
            task.cancel()
        await asyncio.gather(*self._readers, return_exceptions=True)
        await self.client.close()
        await self.frontend.stop()

    def watch(self, namespace):
        """A subscription and the list its events are appended to."""
        sub = self.client.watch(API_VERSION, KIND, namespace)
        events = []

        async def read():
            async for ev in sub:
                events.append(ev)

        self.subs.append(sub)
        self._readers.append(asyncio.ensure_future(read()))
        return sub, events

    async def until(self, pred, what, timeout=15.0):
        deadline = asyncio.get_running_loop().time() + timeout
        while not pred():
            assert asyncio.get_running_loop().time() < deadline, f"timed out: {what}"
            await asyncio.sleep(0.01)

    async def outage(self, change):
        """Stop the listener, run ``change`` on the store with the history
        window at 0 (every event it makes is compacted away at once, so the
        subscriptions' resume points expire), start a new listener on the
        same port and wait until every subscription has re-listed."""
        # every subscription streams: none is between two connects, where it
        # would miss the stop and keep its connection to the store
        await self.until(lambda: len(self.frontend._live_subs) == len(self.subs),
                         "subscriptions streaming")
        before = [sub.relists for sub in self.subs]
        await self.frontend.stop()
        self.server.history_window = 0
        change()
        self.server.history_window = 4096
        self.frontend = ApiServerFrontend(self.server, port=self.port)
        await self.frontend.start()
        await self.until(
            lambda: all(s.relists > b for s, b in zip(self.subs, before)),
            "re-list after the outage")

    # direct store access: what happens while the stream is down
    def create(self, name, ns="health"):
        return self.server.create(make_hc(name=name, ns=ns))

    def delete(self, name, ns="health"):
        self.server.delete(API_VERSION, KIND, ns, name)


def _brief(events):
    return [(ev["type"], ev["object"]["metadata"]["name"]) for ev in events]


def _uid(obj):
    return obj["metadata"]["uid"]


def test_missed_deletion_and_creation_are_replaced(run):
    async def go():
        async with Env() as env:
            sub, events = env.watch("health")
            made = {n: await env.client.create(make_hc(name=n)) for n in "abc"}
            await env.until(lambda: len(events) == 3, "a, b and c seen")
            assert _brief(events) == [("ADDED", "a"), ("ADDED", "b"), ("ADDED", "c")]

            def change():
                env.delete("b")
                env.create("d")

            await env.outage(change)
            await env.client.create(make_hc(name="after"))
            await env.until(lambda: ("ADDED", "after") in _brief(events),
                            "an object created after the recovery")
            recovery = events[3:]
            brief = _brief(recovery)
            # the tombstone first, then the list, then the live stream again
            assert brief[0] == ("DELETED", "b"), brief
            assert sorted(brief[1:4]) == [("ADDED", "a"), ("ADDED", "c"), ("ADDED", "d")]
            assert brief[4:] == [("ADDED", "after")], brief
            tomb = recovery[0]
            assert tomb["synthetic"] is True
            assert tomb["object"]["apiVersion"] == API_VERSION
            assert tomb["object"]["kind"] == KIND
            meta = tomb["object"]["metadata"]
            assert (meta["namespace"], meta["name"]) == ("health", "b")
            assert meta["uid"] == _uid(made["b"])
            assert int(meta["resourceVersion"]) > int(
                made["c"]["metadata"]["resourceVersion"])
            # identities only: nothing of the lost object is made up
            assert set(tomb["object"]) == {"apiVersion", "kind", "metadata"}
            assert all("synthetic" not in ev for ev in recovery[1:])
            assert sub.relists >= 1
            assert sub.synthetic_deletes == 1

    run(go(), timeout=40)


def test_delete_and_recreate_inside_the_window(run):
    async def go():
        async with Env() as env:
            sub, events = env.watch("health")
            old = await env.client.create(make_hc(name="b"))
            await env.until(lambda: len(events) == 1, "b seen")
            new = {}

            def change():
                env.delete("b")
                new["b"] = env.create("b")
                env.create("filler")

            await env.outage(change)
            assert _uid(new["b"]) != _uid(old)
            recovery = events[1:]
            assert _brief(recovery)[0] == ("DELETED", "b"), _brief(recovery)
            assert recovery[0]["object"]["metadata"]["uid"] == _uid(old)
            assert recovery[0]["synthetic"] is True
            added = [ev for ev in recovery[1:]
                     if ev["object"]["metadata"]["name"] == "b"]
            assert [ev["type"] for ev in added] == ["ADDED"]
            assert _uid(added[0]["object"]) == _uid(new["b"])
            assert sub.synthetic_deletes == 1

    run(go(), timeout=40)


def test_delivered_deletion_is_not_announced_again(run):
    async def go():
        async with Env() as env:
            sub, events = env.watch("health")
            await env.client.create(make_hc(name="a"))
            await env.client.create(make_hc(name="b"))
            await env.client.delete(API_VERSION, KIND, "health", "b")
            await env.until(lambda: len(events) == 3, "the ordinary DELETED")
            assert _brief(events)[2] == ("DELETED", "b")
            assert "synthetic" not in events[2]

            await env.outage(lambda: env.create("filler"))
            assert sorted(_brief(events[3:])) == [("ADDED", "a"), ("ADDED", "filler")]
            assert sub.synthetic_deletes == 0

    run(go(), timeout=40)


def test_namespaced_subscription_compares_its_own_namespace(run):
    async def go():
        async with Env() as env:
            sub_ns, ev_ns = env.watch("health")
            sub_all, ev_all = env.watch(None)
            await env.client.create(make_hc(name="a", ns="health"))
            gone = await env.client.create(make_hc(name="a", ns="other"))
            await env.until(lambda: len(ev_ns) == 1 and len(ev_all) == 2,
                            "both objects seen")

            def change():
                env.delete("a", ns="other")
                env.create("filler", ns="other")

            await env.outage(change)
            assert _brief(ev_ns[1:]) == [("ADDED", "a")]
            assert sub_ns.synthetic_deletes == 0
            recovery = ev_all[2:]
            assert _brief(recovery)[0] == ("DELETED", "a")
            meta = recovery[0]["object"]["metadata"]
            assert (meta["namespace"], meta["uid"]) == ("other", _uid(gone))
            assert sorted((ev["type"], ev["object"]["metadata"]["namespace"],
                           ev["object"]["metadata"]["name"])
                          for ev in recovery[1:]) == [
                ("ADDED", "health", "a"), ("ADDED", "other", "filler")]
            assert sub_all.synthetic_deletes == 1

    run(go(), timeout=40)


def test_model_check_mirror_equals_the_store(run):
    """About 200 random creates, deletes and re-creates over 8 names with 10
    outages among them: a mirror built from nothing but the delivered events
    ends equal to the store, uids included."""

    async def go():
        rng = random.Random(0)
        names = [f"n{i}" for i in range(8)]
        async with Env() as env:
            sub, events = env.watch("health")
            live = set()

            def op():
                name = rng.choice(names)
                if name not in live:
                    env.create(name)
                    live.add(name)
                elif rng.random() < 0.5:
                    env.delete(name)
                    live.discard(name)
                else:  # re-create: a new uid under the old name
                    env.delete(name)
                    env.create(name)

            def mirror():
                held = {}
                for ev in events:
                    meta = ev["object"]["metadata"]
                    key = (meta["namespace"], meta["name"])
                    if ev["type"] == "DELETED":
                        # a deletion names the object the consumer holds
                        assert held.pop(key, meta["uid"]) == meta["uid"], ev
                    else:
                        held[key] = meta["uid"]
                return held

            def store():
                return {(o["metadata"]["namespace"], o["metadata"]["name"]): _uid(o)
                        for o in env.server.list(API_VERSION, KIND, "health")}

            total = 200
            outages = sorted(rng.sample(range(10, total - 10), 10))
            done = 0
            while done < total or outages:
                if outages and done >= outages[0]:
                    outages.pop(0)
                    burst = rng.randint(1, 8)

                    def change(n=burst):
                        for _ in range(n):
                            op()

                    await env.outage(change)
                    done += burst
                else:
                    op()
                    done += 1
                    if rng.random() < 0.2:
                        await asyncio.sleep(0)  # let some events drain
            assert sub.relists >= 10 and sub.synthetic_deletes >= 1
            await env.until(lambda: mirror() == store(), "mirror equals the store")
            n = len(events)
            await asyncio.sleep(0.2)
            assert len(events) == n, "the stream is not quiet"
            assert mirror() == store()

    run(go(), timeout=90)

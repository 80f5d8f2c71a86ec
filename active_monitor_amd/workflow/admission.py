"""Who may start, in what order, holding which mutexes.

:class:`Admission` is the bookkeeping behind the engines' ``parallelism``,
``namespace_parallelism`` and ``spec.synchronization`` mutexes: a queue ordered
by priority, then age, then arrival, the count of what was admitted, in all
and per namespace, and the mutexes held. It is synchronous and knows nothing
of Workflow objects, status writes, tasks or timers; those are the engine's
(:mod:`.engines`), which offers what it takes up, starts what :meth:`admit`
returns and releases what has ended.
"""
from __future__ import annotations

import bisect
from typing import Any, Dict, Iterator, List, Optional, Tuple

#: status.message of a Workflow that waits for one of the engine's slots
POSTPONED_MESSAGE = ("Workflow processing has been postponed because too many "
                     "workflows are already running")
#: status.message of a Workflow whose activeDeadlineSeconds ran out in the queue
QUEUE_EXPIRED_MESSAGE = "deadline exceeded while waiting to start"


def _positive(name: str, value: Any) -> Optional[int]:
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError(f"{name} must be a positive integer, got {value!r}")
    return value


def mutex_names(spec: Any) -> List[str]:
    """Names under ``spec.synchronization.mutex`` and ``.mutexes``, duplicates
    removed, order kept."""
    sync = spec.get("synchronization") if isinstance(spec, dict) else None
    if not isinstance(sync, dict):
        return []
    several = sync.get("mutexes")
    found = [sync.get("mutex")] + (several if isinstance(several, list) else [])
    return list(dict.fromkeys(
        str(m["name"]) for m in found if isinstance(m, dict) and m.get("name")
    ))


def _priority(spec: Dict[str, Any]) -> int:
    try:
        return int(spec.get("priority") or 0)
    except (TypeError, ValueError):
        return 0


class Entry:
    """A Workflow that waits to be admitted, or was. ``order`` sorts the
    queue: higher ``spec.priority``, then earlier ``creationTimestamp``, then
    arrival. ``mutexes`` are ``(namespace, name)`` in the spec's order."""

    __slots__ = ("key", "ns", "order", "mutexes")

    def __init__(self, key: str, ns: str, order: Tuple[int, str, int],
                 mutexes: List[Tuple[str, str]]):
        self.key = key
        self.ns = ns
        self.order = order
        self.mutexes = mutexes


class Admission:
    """``len()`` is the length of the queue and iteration goes over it in
    queue order; what was admitted is the caller's to keep and to
    :meth:`release`."""

    def __init__(self, parallelism: Optional[int] = None,
                 namespace_parallelism: Optional[int] = None):
        self.parallelism = _positive("parallelism", parallelism)
        self.namespace_parallelism = _positive("namespace_parallelism",
                                               namespace_parallelism)
        # without a Workflow limit only a Workflow that names a mutex is queued
        self._limited = parallelism is not None or namespace_parallelism is not None
        self._queue: List[Entry] = []  # sorted by .order
        self._queued: Dict[str, Entry] = {}
        self._arrivals = 0
        self._admitted = 0
        self._admitted_ns: Dict[str, int] = {}
        self._locked: set = set()  # (namespace, mutex name) of what was admitted

    def __len__(self) -> int:
        return len(self._queue)

    def __iter__(self) -> Iterator[Entry]:
        return iter(list(self._queue))

    def offer(self, key: str, ns: str, spec: Any, created: Any) -> Optional[Entry]:
        """None when nothing bounds the Workflow (no Workflow limit is set
        and ``spec`` names no mutex): it runs at once, uncounted. Else its
        entry, put into the queue; a key that is queued already keeps the
        entry it has."""
        names = mutex_names(spec) if isinstance(spec, dict) and "synchronization" in spec else None
        if not self._limited and not names:
            return None
        entry = self._queued.get(key)
        if entry is None:
            self._arrivals += 1
            order = (-_priority(spec if isinstance(spec, dict) else {}),
                     str(created or ""), self._arrivals)
            entry = Entry(key, ns, order, [(ns, n) for n in names or ()])
            bisect.insort(self._queue, entry, key=lambda e: e.order)
            self._queued[key] = entry
        return entry

    def blocked_by(self, entry: Entry) -> Optional[str]:
        """The ``Pending`` message for what keeps ``entry`` from starting
        now, None when nothing does."""
        if self.parallelism is not None and self._admitted >= self.parallelism:
            return POSTPONED_MESSAGE
        if (self.namespace_parallelism is not None
                and self._admitted_ns.get(entry.ns, 0) >= self.namespace_parallelism):
            return POSTPONED_MESSAGE
        for ns, name in entry.mutexes:
            if (ns, name) in self._locked:
                return f"Waiting for {ns}/Mutex/{name} lock"
        return None

    def admit(self) -> List[Entry]:
        """Take out of the queue, in its order, every entry that can start.
        One that waits for its namespace or for a mutex is passed over; the
        global limit ends the scan."""
        admitted = []
        i = 0
        while i < len(self._queue):
            if self.parallelism is not None and self._admitted >= self.parallelism:
                break
            entry = self._queue[i]
            if self.blocked_by(entry) is not None:
                i += 1
                continue
            del self._queue[i]
            del self._queued[entry.key]
            # the slot and the mutexes are taken here, all or none, before
            # the next entry is looked at
            self._admitted += 1
            self._admitted_ns[entry.ns] = self._admitted_ns.get(entry.ns, 0) + 1
            self._locked.update(entry.mutexes)
            admitted.append(entry)
        return admitted

    def release(self, entry: Entry) -> None:
        """Give back what :meth:`admit` took for ``entry``."""
        self._admitted -= 1
        left = self._admitted_ns[entry.ns] - 1
        if left:
            self._admitted_ns[entry.ns] = left
        else:
            del self._admitted_ns[entry.ns]
        self._locked.difference_update(entry.mutexes)

    def remove(self, key: str) -> Optional[Entry]:
        """Drop the queued entry of ``key``, if there is one: the Workflow
        was deleted or waited out its deadline."""
        entry = self._queued.pop(key, None)
        if entry is not None:
            self._queue.remove(entry)
        return entry

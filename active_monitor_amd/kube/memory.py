"""In-memory Kubernetes apiserver — the framework's envtest equivalent.

The reference's integration tier runs against envtest (a real kube-apiserver +
etcd, suite_test.go:67-134). This module provides the same role as a
dependency-free in-process store with the apiserver semantics the controller
exercises:

- optimistic concurrency via ``metadata.resourceVersion`` (conflict errors on
  stale writes, so the reconciler's retry-on-conflict paths are real),
- ``metadata.generateName`` server-side name generation,
- the HealthCheck status subresource (plain updates cannot touch status and
  vice versa),
- ownerReference cascade GC (Workflows vanish when their HealthCheck is
  deleted — the behavior relied on at healthcheck_controller.go:512-522),
- finalizer-driven deletionTimestamp handling,
- label-selector list filtering and watch streams (ADDED/MODIFIED/DELETED).

The core is synchronous and thread-safe; watches are asyncio queues fed via
``call_soon_threadsafe`` so any thread may mutate the store.

With a schema installed for a kind (``schemas=`` / :meth:`install_schema`,
see :mod:`.schema`) every write of that kind is validated and pruned like a
real apiserver validates a custom resource against its CRD; with none — the
default — writes are stored as given.

``MemoryApiServer()`` lives and dies with the process.
``MemoryApiServer.open(data_dir)`` is the same store journaled to a directory
(:mod:`.persist`), for standalone deployments that must survive a restart.
"""
from __future__ import annotations

import asyncio
import random
import threading
from collections import deque
from typing import Any, AsyncIterator, Dict, List, Optional, Tuple

from ..api.types import k8s_now
from ..utils.fastcopy import deep_copy, snapshot
from .errors import (
    AlreadyExistsError,
    BadRequestError,
    ConflictError,
    ExpiredError,
    InvalidError,
    NotFoundError,
)
from .registry import DEFAULT_REGISTRY, STATUS_SUBRESOURCE_KINDS, Registry

Obj = Dict[str, Any]
Key = Tuple[str, str, str, str]  # (apiVersion, kind, namespace, name)

FIELD_VALIDATION_MODES = ("Warn", "Strict", "Ignore")
_HC_SCHEMAS: Dict[Tuple[str, str], Any] = {}


def healthcheck_schemas() -> Dict[Tuple[str, str], Any]:
    """``{(apiVersion, kind): Validator}`` for the HealthCheck CRD as
    ``api.crd.healthcheck_crd()`` generates it — the ``schemas=`` argument
    of a store that validates HealthChecks. Compiled once per process."""
    if not _HC_SCHEMAS:
        from ..api.crd import healthcheck_crd
        from .schema import compile_schema

        spec = healthcheck_crd()["spec"]
        for version in spec["versions"]:
            _HC_SCHEMAS[(f'{spec["group"]}/{version["name"]}',
                         spec["names"]["kind"])] = compile_schema(
                version["schema"]["openAPIV3Schema"])
    return dict(_HC_SCHEMAS)

_SUFFIX_ALPHABET = "bcdfghjklmnpqrstvwxz2456789"  # k8s-style name suffix chars
_suffix_counter = [random.randrange(27 ** 4)]


def _rand_suffix(n: int = 5) -> str:
    """Unique k8s-style suffix: a randomly-seeded counter encoded in the
    apiserver's suffix alphabet — collision-free and far cheaper than
    per-character randomness on the create hot path."""
    _suffix_counter[0] += 1
    v = _suffix_counter[0]
    out = []
    for _ in range(n):
        v, r = divmod(v, len(_SUFFIX_ALPHABET))
        out.append(_SUFFIX_ALPHABET[r])
    return "".join(out)


def parse_label_selector(selector: Optional[str]) -> Dict[str, str]:
    """Parse an equality-based selector string ``k=v,k2=v2``."""
    if not selector:
        return {}
    out: Dict[str, str] = {}
    for part in selector.split(","):
        part = part.strip()
        if not part:
            continue
        if "=" not in part:
            raise InvalidError(f"unsupported selector term: {part!r}")
        k, _, v = part.partition("=")
        out[k.strip()] = v.lstrip("=").strip()  # tolerate '=='
    return out


def labels_match(obj: Obj, selector: Dict[str, str]) -> bool:
    labels = (obj.get("metadata") or {}).get("labels") or {}
    return all(labels.get(k) == v for k, v in selector.items())


def parse_field_selector(selector: Optional[str]) -> List[Tuple[str, str, bool]]:
    """Parse ``a.b=v,c!=w`` into (dotted-path, value, negated) terms —
    the equality-based fieldSelector subset kubectl uses (e.g. `kubectl
    describe` filters Events by involvedObject.name/namespace)."""
    if not selector:
        return []
    out: List[Tuple[str, str, bool]] = []
    for part in selector.split(","):
        part = part.strip()
        if not part:
            continue
        if "!=" in part:
            k, _, v = part.partition("!=")
            out.append((k.strip(), v.strip(), True))
        elif "=" in part:
            k, _, v = part.partition("=")
            out.append((k.strip(), v.lstrip("=").strip(), False))
        else:
            raise InvalidError(f"unsupported field selector term: {part!r}")
    return out


def fields_match(obj: Obj, terms: List[Tuple[str, str, bool]]) -> bool:
    for path, want, negated in terms:
        cur: Any = obj
        for seg in path.split("."):
            if not isinstance(cur, dict):
                cur = None
                break
            cur = cur.get(seg)
        have = "" if cur is None else str(cur)
        if (have == want) == negated:
            return False
    return True


def object_rv(obj: Obj, unparsable: int = 0) -> int:
    """``metadata.resourceVersion`` as a number (0 when there is none)."""
    try:
        return int((obj.get("metadata") or {}).get("resourceVersion", 0))
    except (TypeError, ValueError):
        return unparsable


def _selects(obj: Obj, api_version: str, kind: str, namespace: Optional[str]) -> bool:
    """Whether a watch of (apiVersion, kind[, namespace]) is told of ``obj``."""
    if obj.get("apiVersion") != api_version or obj.get("kind") != kind:
        return False
    return namespace is None or (
        (obj.get("metadata") or {}).get("namespace", "") == namespace)


class Subscription:
    """One watch stream. Async-iterate to receive ``{"type": ..., "object": ...}``."""

    def __init__(self, server: "MemoryApiServer", api_version: str, kind: str,
                 namespace: Optional[str], loop: asyncio.AbstractEventLoop):
        self._server = server
        self.api_version = api_version
        self.kind = kind
        self.namespace = namespace
        self._loop = loop
        self._queue: "asyncio.Queue[Optional[Dict[str, Any]]]" = asyncio.Queue()
        self._closed = False

    def _offer(self, event: Dict[str, Any]) -> None:
        if self._closed:
            return
        if not _selects(event["object"], self.api_version, self.kind, self.namespace):
            return
        try:
            # events carry a shared read-only snapshot (copied once at
            # publish, not per subscriber) — consumers must not mutate it
            self._loop.call_soon_threadsafe(self._queue.put_nowait, event)
        except RuntimeError:
            self._closed = True  # loop gone

    def close(self) -> None:
        if not self._closed:
            self._closed = True
            self._server._unsubscribe(self)
            try:
                self._loop.call_soon_threadsafe(self._queue.put_nowait, None)
            except RuntimeError:
                pass

    def __aiter__(self) -> AsyncIterator[Dict[str, Any]]:
        return self

    async def __anext__(self) -> Dict[str, Any]:
        ev = await self._queue.get()
        if ev is None:
            raise StopAsyncIteration
        return ev


class MemoryApiServer:
    def __init__(self, registry: Registry = DEFAULT_REGISTRY,
                 schemas: Optional[Dict[Tuple[str, str], Any]] = None):
        self.registry = registry
        # (apiVersion, kind) → compiled Validator; a kind without an entry is
        # stored unvalidated. Empty (the default) costs writes one falsy test.
        self._schemas: Dict[Tuple[str, str], Any] = {}
        #: writes refused by admission (422 Invalid, or 400 under Strict)
        self.rejected_writes = 0
        self._objects: Dict[Key, Obj] = {}
        self._rv = 0
        self._lock = threading.RLock()
        for (av, kind), schema in (schemas or {}).items():
            self.install_schema(av, kind, schema)
        self._subs: List[Subscription] = []
        # ownerReference uid → dependent keys (O(1) cascade GC)
        self._by_owner: Dict[str, set] = {}
        # Event objects are TTL'd by the real apiserver; cap them here so
        # long-running fleets don't grow the store unboundedly
        self._event_keys: deque = deque()
        self.max_events = 10000
        # counters for observability/benchmarks
        self.op_counts: Dict[str, int] = {"get": 0, "list": 0, "create": 0,
                                          "update": 0, "update_status": 0, "delete": 0}
        # bounded watch-event history: lets a resumed watch replay exactly the
        # events after its resourceVersion, and makes 410 Gone REAL — a resume
        # point older than the window raises ExpiredError, like etcd's
        # compacted-revision error surfaced by the apiserver. Tests shrink
        # history_window to force expiry deterministically.
        self._history: deque = deque()  # (rv:int, ev_type, obj snapshot)
        self.history_window = 4096
        # highest rv evicted from history — the compaction horizon; resuming
        # below it is 410 Gone
        self._compacted_rv = 0
        # on-disk journal (kube/persist.py); None unless opened with open()
        self._journal = None

    @classmethod
    def open(cls, data_dir: str, registry: Registry = DEFAULT_REGISTRY,
             sync_interval: float = 1.0,
             compact_threshold: int = 4096,
             schemas: Optional[Dict[Tuple[str, str], Any]] = None,
             ) -> "MemoryApiServer":
        """A store that survives the process: state is loaded from
        ``data_dir`` (created if missing) and every mutation is journaled
        there before it becomes visible. A kill of the process loses nothing
        acknowledged; a power loss can lose up to ``sync_interval`` seconds.
        The journal is folded into the snapshot once it holds more than
        ``compact_threshold`` records (and more than there are live objects).

        Raises :class:`~.persist.StoreLockedError` when another process holds
        the directory and :class:`~.persist.StoreCorruptError` when it cannot
        be read. Call :meth:`close` when done.

        An I/O error while journaling is raised from the mutating call; by
        then the mutation is applied in memory (visible to ``get``/``list``,
        to no watcher) but not on disk, and every later write raises
        :class:`~.persist.StoreError`. Restart the process: it reloads the
        last journaled state.

        The Event cap restarts from the live Events in creation order. A
        running store also counts Events that were deleted or cascaded away
        since (their keys stay queued until evicted), so it may start
        evicting a little earlier than the same store after a reload.

        The watch history restarts empty with the compaction horizon at the
        restored resourceVersion: a watch resuming from before the restart
        gets 410 Gone and re-lists, one resuming exactly there is valid.

        ``schemas`` applies to writes from now on: objects already in the
        directory are loaded as they are, not re-validated (a real apiserver
        does not re-validate what etcd holds either). Such an object is
        refused the next time someone writes it back unchanged."""
        from .persist import Journal

        self = cls(registry, schemas)
        journal = Journal(data_dir, sync_interval, compact_threshold)
        try:
            rv, objects = journal.load(self._key)
        except BaseException:
            journal.close()
            raise
        self._objects = objects
        for key, obj in objects.items():
            self._index_owners(key, obj)
            # dict order is creation order per key: a put keeps its place
            if key[1] == "Event":
                self._event_keys.append(key)
        self._rv = self._compacted_rv = rv
        self._journal = journal
        return self

    @property
    def data_dir(self) -> Optional[str]:
        return None if self._journal is None else self._journal.data_dir

    def close(self) -> None:
        """Flush, sync and release the data directory (idempotent; a no-op
        for a store without one). The store must not be written afterwards."""
        with self._lock:
            if self._journal is not None and not self._journal.closed:
                self._journal.close()

    # -- admission -----------------------------------------------------------

    def _enter_write(self, api_version: str, kind: str,
                     field_validation: str) -> Any:
        """What every write does on entry, before it takes the lock or counts
        itself, unless the mode is ``"Warn"`` and no schema is installed at
        all: refuse a wrong mode, whether or not anything would be pruned,
        and look up the kind's validator (None: stored as given). The write
        hands its object to :meth:`_admit` once it is named and complete."""
        if field_validation != "Warn":
            self._check_mode(field_validation)
        return self._schemas.get((api_version, kind))

    @staticmethod
    def _check_mode(field_validation: str) -> None:
        if field_validation not in FIELD_VALIDATION_MODES:
            raise BadRequestError(
                f'invalid fieldValidation "{field_validation}": supported '
                'values: ' + ", ".join(f'"{m}"' for m in FIELD_VALIDATION_MODES))

    def install_schema(self, api_version: str, kind: str,
                       openapi_schema: Any) -> None:
        """Validate and prune every later write of ``kind`` by this
        ``openAPIV3Schema`` (a dict, or one already compiled by
        :func:`.schema.compile_schema`)."""
        if isinstance(openapi_schema, dict):
            from .schema import compile_schema

            openapi_schema = compile_schema(openapi_schema)
        with self._lock:
            self._schemas[(api_version, kind)] = openapi_schema

    def _admit(self, validator: Any, obj: Obj, field_validation: str,
               warnings: Optional[List[str]], subtree: Optional[str] = None) -> None:
        """Run under the lock, before anything of the write is visible: on a
        refusal the store, the rv counter, the history and the journal are
        as they were."""
        pruned, errs = validator.admit(obj, subtree=subtree)
        if not errs and not pruned:
            return
        api_version, kind = obj.get("apiVersion", ""), obj.get("kind", "")
        group, _, version = api_version.rpartition("/")
        if errs:
            self.rejected_writes += 1
            name = (obj.get("metadata") or {}).get("name", "") or ""
            listed = errs[0] if len(errs) == 1 else "[" + ", ".join(errs) + "]"
            qualified = f"{kind}.{group}" if group else kind
            causes = [{"reason": e.reason, "message": e.detail, "field": e.field}
                      for e in errs]
            raise InvalidError(
                f'{qualified} "{name}" is invalid: {listed}', causes=causes,
                details={"name": name, "group": group, "kind": kind,
                         "causes": causes},
            )
        if field_validation == "Strict":
            self.rejected_writes += 1
            unknown = ", ".join(f'unknown field "{p}"' for p in pruned)
            raise BadRequestError(
                f'{kind} in version "{version}" cannot be handled as a {kind}: '
                f"strict decoding error: {unknown}"
            )
        if field_validation == "Warn" and warnings is not None:
            warnings.extend(pruned)

    # -- internals ---------------------------------------------------------

    def _next_rv(self) -> str:
        self._rv += 1
        return str(self._rv)

    def _key(self, obj: Obj) -> Key:
        meta = obj.get("metadata") or {}
        info = self.registry.by_kind(obj.get("apiVersion", ""), obj.get("kind", ""))
        ns = meta.get("namespace", "") if info.namespaced else ""
        return (obj.get("apiVersion", ""), obj.get("kind", ""), ns, meta.get("name", ""))

    def _resolve(self, api_version: str, kind: str, namespace: str, name: str) -> Key:
        info = self.registry.by_kind(api_version, kind)
        return (api_version, kind, namespace if info.namespaced else "", name)

    @staticmethod
    def _check_fresh(obj: Obj, meta: Obj, ex_meta: Obj) -> None:
        """Optimistic concurrency: a write that names a resourceVersion must
        name the stored one."""
        rv = meta.get("resourceVersion")
        if rv and str(rv) != str(ex_meta.get("resourceVersion")):
            raise ConflictError(
                f'Operation cannot be fulfilled on {obj.get("kind")} '
                f'"{meta.get("name")}": the object has been modified; please apply '
                f"your changes to the latest version and try again"
            )

    def _not_found(self, api_version: str, kind: str, name: str) -> NotFoundError:
        info = self.registry.by_kind(api_version, kind)
        group = api_version.split("/")[0] if "/" in api_version else ""
        full = f"{info.plural}.{group}" if group else info.plural
        return NotFoundError(f'{full} "{name}" not found')

    def _index_owners(self, key: Key, obj: Obj) -> None:
        for ref in (obj.get("metadata") or {}).get("ownerReferences") or []:
            uid = ref.get("uid")
            if uid:
                self._by_owner.setdefault(uid, set()).add(key)

    def _unindex_owners(self, key: Key, obj: Obj) -> None:
        for ref in (obj.get("metadata") or {}).get("ownerReferences") or []:
            uid = ref.get("uid")
            if uid:
                deps = self._by_owner.get(uid)
                if deps is not None:
                    deps.discard(key)
                    if not deps:
                        self._by_owner.pop(uid, None)

    def _publish(self, ev_type: str, obj: Obj) -> None:
        event = {"type": ev_type, "object": obj}
        rv = object_rv(obj, self._rv)
        if self._journal is not None:
            self._journal_event(ev_type, obj, rv)
        self._history.append((rv, ev_type, obj))
        while len(self._history) > self.history_window:
            self._compacted_rv = self._history.popleft()[0]
        for sub in list(self._subs):
            sub._offer(event)

    def _journal_event(self, ev_type: str, obj: Obj, rv: int) -> None:
        """Write-ahead of visibility: the record is in the OS before the
        event reaches the history or any watcher. Serialised here, under the
        store lock, because ``obj`` shares subtrees with the live object."""
        journal = self._journal
        if ev_type == "DELETED":
            journal.delete(rv, self._key(obj))
        else:
            journal.put(rv, obj)
        # every caller has brought _objects up to this event already, so the
        # store is exactly the journal replayed up to here
        if journal.should_compact(len(self._objects)):
            journal.compact(self._rv, self._objects.values(), len(self._objects))

    def events_since(self, api_version: str, kind: str, namespace: Optional[str],
                     resource_version: str) -> List[Dict[str, Any]]:
        """Replay retained events newer than ``resource_version`` for one
        (apiVersion, kind[, namespace]); raises :class:`ExpiredError` when the
        resume point predates the retained window (apiserver 410 semantics)."""
        try:
            since = int(resource_version)
        except (TypeError, ValueError):
            raise ExpiredError(f"resourceVersion {resource_version!r} is invalid")
        with self._lock:
            if since < self._compacted_rv:
                # events in (since, compacted_rv] are gone — the client can't
                # reconstruct the stream and must re-list
                raise ExpiredError(
                    f"too old resource version: {since} ({self._compacted_rv})"
                )
            out = []
            for rv, ev_type, obj in self._history:
                if rv > since and _selects(obj, api_version, kind, namespace):
                    out.append({"type": ev_type, "object": obj})
            return out

    def _unsubscribe(self, sub: Subscription) -> None:
        with self._lock:
            if sub in self._subs:
                self._subs.remove(sub)

    # -- public API --------------------------------------------------------

    def create(self, obj: Obj, transfer: bool = False,
               field_validation: str = "Warn",
               warnings: Optional[List[str]] = None) -> Obj:
        """``transfer=True`` lets the store take ownership of ``obj`` (no
        copy-in) and return a read-optimized snapshot (no copy-out). Only for
        callers that built the dict themselves and never touch it again —
        the controller's submit/event/RBAC paths.

        For a kind with a schema installed, here and in :meth:`update`,
        :meth:`update_status` and :meth:`patch`: an object that violates it
        raises :class:`InvalidError`; fields it does not know are pruned, and
        ``field_validation`` decides what else happens to them — ``"Strict"``
        raises :class:`BadRequestError`, ``"Warn"`` appends their paths to
        the ``warnings`` list when one is given, ``"Ignore"`` says nothing.
        Any other mode raises :class:`BadRequestError`, always."""
        validator = None
        if field_validation != "Warn" or self._schemas:
            validator = self._enter_write(
                obj.get("apiVersion", ""), obj.get("kind", ""), field_validation)
        if not transfer:
            obj = deep_copy(obj)
        meta = obj.setdefault("metadata", {})
        with self._lock:
            self.op_counts["create"] += 1
            if not meta.get("name"):
                gen = meta.get("generateName")
                if not gen:
                    raise InvalidError("name or generateName is required")
                # retry suffixes on collision, like the apiserver
                for _ in range(16):
                    candidate = gen + _rand_suffix()
                    meta["name"] = candidate
                    if self._key(obj) not in self._objects:
                        break
                else:
                    raise AlreadyExistsError(f"could not generate unique name for {gen}")
            # named first, as the apiserver does, so that a refusal can say
            # which object; nothing of the write is visible yet
            if validator is not None:
                self._admit(validator, obj, field_validation, warnings)
            key = self._key(obj)
            if key in self._objects:
                raise AlreadyExistsError(
                    f'{obj.get("kind", "object")} "{meta["name"]}" already exists'
                )
            meta["uid"] = meta.get("uid") or ("uid-" + _rand_suffix(12))
            meta["resourceVersion"] = self._next_rv()
            meta["creationTimestamp"] = meta.get("creationTimestamp") or k8s_now()
            meta["generation"] = 1
            self._objects[key] = obj
            self._index_owners(key, obj)
            if obj.get("kind") == "Event":
                self._event_keys.append(key)
                while len(self._event_keys) > self.max_events:
                    old = self._event_keys.popleft()
                    dropped = self._objects.pop(old, None)
                    if dropped is not None:
                        self._unindex_owners(old, dropped)
                        if self._journal is not None:
                            # cap evictions publish no event; they share
                            # the rv of the create that caused them
                            self._journal.delete(self._rv, old)
            out = snapshot(obj)
            self._publish("ADDED", out)
            if not transfer:
                out = deep_copy(obj)
        return out

    def get(self, api_version: str, kind: str, namespace: str, name: str,
            snapshot_read: bool = False) -> Obj:
        """``snapshot_read=True`` returns a read-optimized copy whose subtrees
        other than metadata/status are shared with the store — callers must
        treat those as read-only (the controller hot path opts in; the default
        is a fully private deep copy, safe to mutate)."""
        key = self._resolve(api_version, kind, namespace, name)
        with self._lock:
            self.op_counts["get"] += 1
            obj = self._objects.get(key)
            if obj is None:
                raise self._not_found(api_version, kind, name)
            return snapshot(obj) if snapshot_read else deep_copy(obj)

    def list(
        self,
        api_version: str,
        kind: str,
        namespace: Optional[str] = None,
        label_selector: Optional[str] = None,
        snapshot_read: bool = False,
        field_selector: Optional[str] = None,
    ) -> List[Obj]:
        selector = parse_label_selector(label_selector)
        fields = parse_field_selector(field_selector)
        copier = snapshot if snapshot_read else deep_copy
        with self._lock:
            self.op_counts["list"] += 1
            out = []
            for (av, k, ns, _), obj in self._objects.items():
                if av != api_version or k != kind:
                    continue
                if namespace is not None and ns != namespace:
                    continue
                if selector and not labels_match(obj, selector):
                    continue
                if fields and not fields_match(obj, fields):
                    continue
                out.append(copier(obj))
            return out

    def update(self, obj: Obj, field_validation: str = "Warn",
               warnings: Optional[List[str]] = None) -> Obj:
        obj = deep_copy(obj)
        key = self._key(obj)
        validator = None
        if field_validation != "Warn" or self._schemas:
            validator = self._enter_write(key[0], key[1], field_validation)
        meta = obj.setdefault("metadata", {})
        with self._lock:
            self.op_counts["update"] += 1
            existing = self._objects.get(key)
            if existing is None:
                raise self._not_found(key[0], key[1], key[3])
            ex_meta = existing["metadata"]
            self._check_fresh(obj, meta, ex_meta)
            # immutable metadata
            meta["uid"] = ex_meta.get("uid")
            meta["creationTimestamp"] = ex_meta.get("creationTimestamp")
            if ex_meta.get("deletionTimestamp"):
                meta["deletionTimestamp"] = ex_meta["deletionTimestamp"]
            # status subresource: plain update cannot change status
            if (key[0], key[1]) in STATUS_SUBRESOURCE_KINDS:
                if "status" in existing:
                    obj["status"] = deep_copy(existing["status"])
                else:
                    obj.pop("status", None)
            if validator is not None:
                self._admit(validator, obj, field_validation, warnings)
            # no-op updates don't bump the resourceVersion or emit watch
            # events (apiserver semantics — prevents self-triggering loops)
            meta["resourceVersion"] = ex_meta.get("resourceVersion")
            meta["generation"] = ex_meta.get("generation", 1)
            if obj == existing:
                return deep_copy(existing)
            if obj.get("spec") != existing.get("spec"):
                meta["generation"] = int(ex_meta.get("generation", 1)) + 1
            meta["resourceVersion"] = self._next_rv()
            self._unindex_owners(key, existing)
            self._objects[key] = obj
            self._index_owners(key, obj)
            # finalizer removal completes a pending delete
            if meta.get("deletionTimestamp") and not meta.get("finalizers"):
                # its DELETED carries the rv this update has just assigned
                self._remove(key, obj, bump_rv=False)
                return deep_copy(obj)
            self._publish("MODIFIED", snapshot(obj))
            out = deep_copy(obj)
        return out

    def update_status(self, obj: Obj, field_validation: str = "Warn",
                      warnings: Optional[List[str]] = None) -> Obj:
        obj = deep_copy(obj)
        key = self._key(obj)
        validator = None
        if field_validation != "Warn" or self._schemas:
            validator = self._enter_write(key[0], key[1], field_validation)
        meta = obj.get("metadata") or {}
        with self._lock:
            self.op_counts["update_status"] += 1
            existing = self._objects.get(key)
            if existing is None:
                raise self._not_found(key[0], key[1], key[3])
            self._check_fresh(obj, meta, existing["metadata"])
            if validator is not None:
                self._admit(validator, obj, field_validation, warnings,
                            subtree="status")
            updated = snapshot(existing)
            if "status" in obj:
                updated["status"] = deep_copy(obj["status"])
            else:
                updated.pop("status", None)
            if updated == existing:  # no-op status write (apiserver semantics)
                return deep_copy(existing)
            updated["metadata"]["resourceVersion"] = self._next_rv()
            self._objects[key] = updated
            self._publish("MODIFIED", snapshot(updated))
            out = deep_copy(updated)
        return out

    @staticmethod
    def _merge(base: Obj, patch: Obj) -> None:
        """RFC 7386 JSON merge patch: dicts merge recursively, null deletes,
        everything else replaces (strategic-merge degenerates to this for
        our types — the CRD's list fields are x-kubernetes-list-type:
        atomic)."""
        for k, v in patch.items():
            if v is None:
                base.pop(k, None)
            elif isinstance(v, dict) and isinstance(base.get(k), dict):
                MemoryApiServer._merge(base[k], v)
            else:
                base[k] = deep_copy(v) if isinstance(v, (dict, list)) else v

    def patch(self, api_version: str, kind: str, namespace: str, name: str,
              patch_obj: Obj, subresource: str = "", upsert: bool = False,
              field_validation: str = "Warn",
              warnings: Optional[List[str]] = None) -> Obj:
        """Merge-patch an object (kubectl patch / the merge half of kubectl
        apply). ``subresource='status'`` touches only status; a plain patch
        cannot touch status for kinds with the subresource (enforced by the
        update path it reuses). ``upsert=True`` creates the object when
        absent (server-side-apply shape). With a schema installed it is the
        merged result that is validated, not the patch."""
        if field_validation != "Warn":
            self._enter_write(api_version, kind, field_validation)
        key = self._resolve(api_version, kind, namespace, name)
        namespaced = self.registry.by_kind(api_version, kind).namespaced
        with self._lock:
            existing = self._objects.get(key)
            if existing is None:
                if not upsert:
                    raise self._not_found(api_version, kind, name)
                obj = deep_copy(patch_obj)
                obj.setdefault("apiVersion", api_version)
                obj.setdefault("kind", kind)
                meta = obj.setdefault("metadata", {})
                meta.setdefault("name", name)
                if namespaced:
                    meta.setdefault("namespace", namespace)
                return self.create(obj, transfer=True,
                                   field_validation=field_validation,
                                   warnings=warnings)
            merged = deep_copy(existing)
            if subresource == "status":
                status = merged.setdefault("status", {})
                patch_status = patch_obj.get("status")
                if isinstance(patch_status, dict):
                    self._merge(status, patch_status)
                return self.update_status(merged, field_validation, warnings)
            self._merge(merged, deep_copy(patch_obj))
            # identity is immutable under patch
            merged["apiVersion"], merged["kind"] = api_version, kind
            m = merged.setdefault("metadata", {})
            m["name"], m["uid"] = name, existing["metadata"].get("uid")
            if namespaced:
                m["namespace"] = key[2]
            # honor an explicit rv in the patch (optimistic concurrency);
            # otherwise patch applies to the current version
            if "resourceVersion" not in (patch_obj.get("metadata") or {}):
                m["resourceVersion"] = existing["metadata"].get("resourceVersion")
            return self.update(merged, field_validation, warnings)

    def delete(self, api_version: str, kind: str, namespace: str, name: str) -> None:
        key = self._resolve(api_version, kind, namespace, name)
        with self._lock:
            self.op_counts["delete"] += 1
            obj = self._objects.get(key)
            if obj is None:
                raise self._not_found(api_version, kind, name)
            meta = obj["metadata"]
            if meta.get("finalizers"):
                if not meta.get("deletionTimestamp"):
                    meta["deletionTimestamp"] = k8s_now()
                    meta["resourceVersion"] = self._next_rv()
                    self._publish("MODIFIED", snapshot(obj))
                return
            self._remove(key, obj)

    def _remove(self, key: Key, obj: Obj, bump_rv: bool = True) -> None:
        """Take ``obj`` out of the store and tell the watchers, then do the
        same for its dependents — background-propagation GC: objects whose
        ownerReferences name the deleted uid (the mechanism behind Workflow
        cleanup on HealthCheck delete, healthcheck_controller.go:512-522).
        O(dependents) via the owner-uid index, not a store scan."""
        del self._objects[key]
        self._unindex_owners(key, obj)
        meta = obj["metadata"]
        if bump_rv:
            # deletion bumps the rv (apiserver semantics) so a watch resuming
            # from just before the delete replays the DELETED event
            meta["resourceVersion"] = self._next_rv()
        self._publish("DELETED", snapshot(obj))
        uid = meta.get("uid")
        if uid:
            for dep_key in list(self._by_owner.pop(uid, ())):
                dependent = self._objects.get(dep_key)
                if dependent is not None:
                    self._remove(dep_key, dependent)

    def resource_version(self) -> str:
        """The store's current global resourceVersion (list metadata rv)."""
        with self._lock:
            return str(self._rv)

    def watch(self, api_version: str, kind: str, namespace: Optional[str] = None) -> Subscription:
        loop = asyncio.get_running_loop()
        sub = Subscription(self, api_version, kind, namespace, loop)
        with self._lock:
            self._subs.append(sub)
        return sub

    def __len__(self) -> int:
        with self._lock:
            return len(self._objects)

    def __bool__(self) -> bool:
        return True  # an empty store is still a store (see MemoryClient note)

"""Workflow execution engines.

The reference delegates execution to the external Argo Workflows controller
(deploy/deploy-argo.yaml; the controller only creates Workflow CRs and polls
``status.phase``, healthcheck_controller.go:525,617-624). This module provides
that role in-process:

- :class:`ScriptedWorkflowEngine` — drives submitted Workflow CRs to a phase
  decided by a policy callable. This is the integration-test linchpin: with no
  engine at all, workflows never reach a terminal phase and the IEB timeout
  forces the Failed path (the reference's envtest trick); with a
  policy, the success path — which the reference's envtest never reaches — is
  exercised too.
- :class:`LocalWorkflowEngine` — actually EXECUTES Argo-shaped workflows as
  local subprocesses (container/script leaves, ``steps`` and ``dag``
  templates, parameters, loops, ``when``, exit handlers, retries with
  backoff, ``activeDeadlineSeconds``, output parameters), so the framework
  can run health checks standalone without a cluster. The template walk
  itself lives in :mod:`.executor`, substitution and ``when`` in
  :mod:`.template`, static checks in :mod:`.validate`.
"""
from __future__ import annotations

import asyncio
import bisect
import logging
import time
from typing import Any, Callable, Dict, List, Optional, Tuple

from ..kube.client import KubeClient
from ..kube.errors import ConflictError, NotFoundError
from ..kube.registry import WF_API_VERSION, WF_KIND
from .templates import CWFT_KIND, WFT_KIND, has_references, resolve

log = logging.getLogger("active_monitor_amd.workflow")

Phase = str  # "Pending" | "Running" | "Succeeded" | "Failed"

#: status.message of a Workflow that waits for one of the engine's slots
POSTPONED_MESSAGE = ("Workflow processing has been postponed because too many "
                     "workflows are already running")
#: status.message of a Workflow whose activeDeadlineSeconds ran out in the queue
QUEUE_EXPIRED_MESSAGE = "deadline exceeded while waiting to start"

PolicyResult = Optional[Tuple[Phase, str]]
Policy = Callable[[Dict[str, Any]], PolicyResult]


def always_succeed(wf: Dict[str, Any]) -> PolicyResult:
    return ("Succeeded", "")


def always_fail(wf: Dict[str, Any]) -> PolicyResult:
    return ("Failed", "workflow failed")


def never_complete(wf: Dict[str, Any]) -> PolicyResult:
    return None


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


class _Queued:
    """A Workflow that waits to be admitted. ``order`` sorts the queue:
    higher ``spec.priority``, then earlier ``creationTimestamp``, then
    arrival. ``postponed`` is the task of its one ``Pending`` write, which
    the next write to the same Workflow waits for."""

    __slots__ = ("wf", "key", "ns", "order", "mutexes", "postponed", "expiry")

    def __init__(self, wf: Dict[str, Any], key: str, ns: str, order: Tuple[int, str, int],
                 mutexes: List[Tuple[str, str]]):
        self.wf = wf
        self.key = key
        self.ns = ns
        self.order = order
        self.mutexes = mutexes
        self.postponed: Optional["asyncio.Future[Any]"] = None
        self.expiry: Optional[asyncio.TimerHandle] = None


class _EngineBase:
    """``ttl_seconds`` deletes completed workflows after the given delay —
    the role Argo's ``ttlStrategy.secondsAfterCompletion`` plays for the
    reference (its install configures 1800s, deploy-argo.yaml:1162-1173);
    None disables (tests that inspect completed workflows).

    ``recover=True`` is for a store that outlives the engine (a durable
    data directory): ``start()`` also lists the Workflows that are already
    there. One that was never picked up runs as if just added; one left
    ``Running`` by a previous process is failed, never re-run (a remedy is
    not idempotent and a half-run DAG cannot be resumed); one already
    terminal gets its lost TTL timer re-armed for the time it has left; one
    found ``Pending`` (queued by a previous process) is admitted anew.

    ``parallelism`` and ``namespace_parallelism`` bound how many Workflows
    run at once, in all and per namespace — the Argo controller's settings of
    the same names; ``max_processes`` is for the engine that starts
    processes. None is unlimited. A Workflow that names mutexes
    (``spec.synchronization``) runs only while it holds all of them, limits
    or not. One that cannot start waits ``Pending`` in a queue ordered by
    priority, then age; docs/OPERATIONS.md, "Bounding what runs at once"."""

    DEFAULT_TTL = 1800.0
    INTERRUPTED_MESSAGE = "workflow interrupted: engine restarted"

    def __init__(self, client: KubeClient, namespace: Optional[str] = None,
                 ttl_seconds: Optional[float] = DEFAULT_TTL,
                 recover: bool = False, parallelism: Optional[int] = None,
                 namespace_parallelism: Optional[int] = None,
                 max_processes: Optional[int] = None):
        self.client = client
        self.namespace = namespace
        self.ttl_seconds = ttl_seconds
        self.recover = recover
        self.parallelism = _positive("parallelism", parallelism)
        self.namespace_parallelism = _positive("namespace_parallelism",
                                               namespace_parallelism)
        self.max_processes = _positive("max_processes", max_processes)
        # without a Workflow limit only a Workflow that names a mutex is queued
        self._limited = parallelism is not None or namespace_parallelism is not None
        self._queue: List[_Queued] = []  # sorted by .order
        self._queued: Dict[str, _Queued] = {}
        self._arrivals = 0
        self._admitted = 0
        self._admitted_ns: Dict[str, int] = {}
        self._locked: set = set()  # (namespace, mutex name) of admitted runs
        self._stopping = False
        self.postponed_total = 0
        self.expired_in_queue = 0
        # uids taken from the start-up list; their ADDED event, should the
        # watch deliver one as well, is dropped. Emptied by the first event
        # newer than everything in that list (_recovered_rv).
        self._recovered: set = set()
        self._recovered_rv = 0
        self._task: Optional[asyncio.Task] = None
        self._sub = None
        self._inflight: Dict[str, asyncio.Task] = {}
        from collections import deque

        self._ttl_handles: "deque" = deque()

    async def start(self) -> None:
        self._sub = self.client.watch(WF_API_VERSION, WF_KIND, self.namespace)
        if self.recover:
            # watch first, then list: nothing created in between is missed
            finished = []
            for wf in await self.client.list(WF_API_VERSION, WF_KIND, self.namespace):
                self._recover(wf, finished)
            # shortest remaining TTL first, so that _ttl_handles stays in
            # firing order
            finished.sort(key=lambda pair: pair[0])
            for left, wf in finished:
                self._schedule_ttl(wf, left)
            if self._queue:
                # everything the list held is in the queue: admit in order
                self._pump()
                for entry in list(self._queue):
                    self._postpone(entry)
        log.info("workflow engine limits: parallelism=%s namespace_parallelism=%s "
                 "max_processes=%s", *(
                     "unlimited" if v is None else v for v in self.limits().values()))
        self._task = asyncio.ensure_future(self._loop())

    async def stop(self) -> None:
        # what is queued stays Pending, for a restart over the same store
        self._stopping = True
        for entry in self._queue:
            if entry.expiry is not None:
                entry.expiry.cancel()
        if self._sub is not None:
            self._sub.close()
        if self._task is not None:
            self._task.cancel()
            try:
                await self._task
            except (asyncio.CancelledError, Exception):
                pass
        for t in self._inflight.values():
            t.cancel()
        for h in self._ttl_handles:
            h.cancel()
        self._ttl_handles.clear()

    async def _loop(self) -> None:
        async for ev in self._sub:
            wf = ev["object"]
            if self._recovered and self._taken_at_start(ev["type"], wf):
                continue
            if ev["type"] == "DELETED":
                if self._queued:
                    self._dequeue(wf)
                self._deleted(wf)
            if ev["type"] != "ADDED":
                continue
            if (wf.get("status") or {}).get("phase") in ("Succeeded", "Failed"):
                continue
            self._submit(wf)

    def _taken_at_start(self, ev_type: str, wf: Dict[str, Any]) -> bool:
        """True for the ADDED event of a workflow that the start-up list
        already handed to :meth:`_recover`. Events arrive in resourceVersion
        order, so the first one newer than everything in that list ends the
        overlap and the set is dropped."""
        meta = wf["metadata"]
        try:
            if int(meta.get("resourceVersion")) > self._recovered_rv:
                self._recovered.clear()
                return False
        except (TypeError, ValueError):
            pass  # opaque resourceVersion: keep matching by uid
        return ev_type == "ADDED" and meta.get("uid") in self._recovered

    def _deleted(self, wf: Dict[str, Any]) -> None:
        """The Workflow is gone: TTL, owner cascade or a user's delete."""

    def _spawn(self, wf: Dict[str, Any], coro: Any, prefix: str = "") -> "asyncio.Future[Any]":
        """``prefix`` keeps a side task (``pending:``, ``expired:``) apart
        from the run of the same Workflow."""
        key = f'{prefix}{(wf["metadata"].get("namespace", ""))}/{wf["metadata"]["name"]}'
        task = asyncio.ensure_future(coro)
        self._inflight[key] = task

        def done(t: "asyncio.Future[Any]", k: str = key) -> None:
            # a later task may have taken the key: that one stays
            if self._inflight.get(k) is t:
                del self._inflight[k]

        task.add_done_callback(done)
        return task

    # -- admission --------------------------------------------------------

    def limits(self) -> Dict[str, Optional[int]]:
        return {"parallelism": self.parallelism,
                "namespace_parallelism": self.namespace_parallelism,
                "max_processes": self.max_processes}

    def stats(self) -> Dict[str, Any]:
        """Counters for ``/statusz``. ``running`` counts the runs in flight,
        admitted or never queued; ``processes`` the leaf processes alive."""
        return {
            "running": sum(1 for key in self._inflight if ":" not in key),
            "queued": len(self._queue),
            "postponed_total": self.postponed_total,
            "expired_in_queue": self.expired_in_queue,
            "processes": self._processes(),
            "limits": self.limits(),
        }

    def _processes(self) -> int:
        return 0

    def _submit(self, wf: Dict[str, Any], recovering: bool = False) -> None:
        """Run ``wf`` now, or queue it when a limit or a mutex may stand in
        its way. ``recovering``: only queue it, start() admits once all that
        it found is queued."""
        spec = self._spec_of(wf)
        names = mutex_names(spec) if isinstance(spec, dict) and "synchronization" in spec else None
        if not self._limited and not names:
            self._spawn(wf, self._run(wf))
            return
        meta = wf["metadata"]
        ns = meta.get("namespace", "")
        key = f'{ns}/{meta["name"]}'
        if key in self._queued:
            return
        self._arrivals += 1
        order = (-_priority(spec if isinstance(spec, dict) else {}),
                 str(meta.get("creationTimestamp") or ""), self._arrivals)
        entry = _Queued(wf, key, ns, order, [(ns, n) for n in names or ()])
        bisect.insort(self._queue, entry, key=lambda e: e.order)
        self._queued[key] = entry
        if not recovering:
            self._pump()
            if key in self._queued:
                self._postpone(entry)

    def _spec_of(self, wf: Dict[str, Any]) -> Any:
        """The spec that admission reads: priority, mutexes, the deadline
        that runs in the queue."""
        return wf.get("spec")

    def _blocked_by(self, entry: _Queued) -> Optional[str]:
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

    def _pump(self) -> None:
        """Admit, in queue order, every Workflow that can start. One that
        waits for its namespace or for a mutex is passed over."""
        if self._stopping:
            return
        i = 0
        while i < len(self._queue):
            if self.parallelism is not None and self._admitted >= self.parallelism:
                break
            entry = self._queue[i]
            if self._blocked_by(entry) is not None:
                i += 1
                continue
            del self._queue[i]
            del self._queued[entry.key]
            if entry.expiry is not None:
                entry.expiry.cancel()
            # the slot and the mutexes are taken here, all or none, before
            # the next entry is looked at
            self._admitted += 1
            self._admitted_ns[entry.ns] = self._admitted_ns.get(entry.ns, 0) + 1
            self._locked.update(entry.mutexes)
            self._spawn(entry.wf, self._run_admitted(entry))

    async def _run_admitted(self, entry: _Queued) -> None:
        try:
            if entry.postponed is not None:
                await asyncio.wait([entry.postponed])  # Pending lands before Running
            await self._run(entry.wf)
        finally:
            self._admitted -= 1
            left = self._admitted_ns[entry.ns] - 1
            if left:
                self._admitted_ns[entry.ns] = left
            else:
                del self._admitted_ns[entry.ns]
            self._locked.difference_update(entry.mutexes)
            self._pump()

    def _postpone(self, entry: _Queued) -> None:
        """``entry`` stays in the queue: write ``Pending`` once and start
        the clock of its deadline."""
        self.postponed_total += 1
        wf = entry.wf
        if (wf.get("status") or {}).get("phase") != "Pending":  # else: recovered
            message = self._blocked_by(entry) or POSTPONED_MESSAGE
            entry.postponed = self._spawn(
                wf, self._set_status(wf, {"phase": "Pending", "message": message}),
                "pending:")
        spec = self._spec_of(wf)
        deadline = spec.get("activeDeadlineSeconds") if isinstance(spec, dict) else None
        try:
            deadline = float(deadline) if deadline and deadline is not True else 0.0
        except (TypeError, ValueError):
            deadline = 0.0
        if deadline > 0:
            entry.expiry = asyncio.get_event_loop().call_later(
                deadline, self._expire, entry)

    def _expire(self, entry: _Queued) -> None:
        if self._queued.get(entry.key) is not entry:
            return
        del self._queued[entry.key]
        self._queue.remove(entry)
        self.expired_in_queue += 1
        log.warning("workflow %s waited out its activeDeadlineSeconds in the "
                    "queue: failing it", entry.key)
        self._spawn(entry.wf, self._fail_expired(entry), "expired:")

    async def _fail_expired(self, entry: _Queued) -> None:
        if entry.postponed is not None:
            await asyncio.wait([entry.postponed])
        await self._set_status(entry.wf, {
            "phase": "Failed", "finishedAt": _now_iso(), "message": QUEUE_EXPIRED_MESSAGE,
        })
        self._schedule_ttl(entry.wf)

    def _dequeue(self, wf: Dict[str, Any]) -> None:
        """A DELETED Workflow leaves the queue; it never runs."""
        meta = wf["metadata"]
        entry = self._queued.pop(f'{meta.get("namespace", "")}/{meta["name"]}', None)
        if entry is not None:
            self._queue.remove(entry)
            if entry.expiry is not None:
                entry.expiry.cancel()

    def _recover(self, wf: Dict[str, Any], finished: List[Any]) -> None:
        """Handle one Workflow found at start by the state it is in; a
        terminal one is appended to ``finished`` as ``(ttl left, wf)`` for
        the caller to schedule."""
        meta = wf["metadata"]
        key = f'{meta.get("namespace", "")}/{meta["name"]}'
        if key in self._inflight:
            return
        status = wf.get("status") or {}
        phase = status.get("phase")
        if phase in ("Succeeded", "Failed", "Error"):
            if self.ttl_seconds is not None:
                finished.append((self._ttl_left(status.get("finishedAt")), wf))
            return
        if phase and phase not in ("Running", "Pending"):
            return  # a phase no local engine writes: not ours to touch
        if meta.get("uid"):
            self._recovered.add(meta["uid"])
            try:
                self._recovered_rv = max(self._recovered_rv,
                                         int(meta.get("resourceVersion")))
            except (TypeError, ValueError):
                pass
        if phase != "Running":
            log.info("recovering pending workflow %s", key)
            self._submit(wf, recovering=True)
        else:
            log.warning("workflow %s was running when the engine stopped: "
                        "failing it", key)
            self._spawn(wf, self._fail_interrupted(wf))

    def _ttl_left(self, finished_at: Any) -> float:
        """``ttl_seconds`` less the time since ``finishedAt``, floored at 0;
        a missing or unparsable ``finishedAt`` counts from now."""
        from ..api.types import parse_k8s_time

        try:
            finished = parse_k8s_time(finished_at)
        except (TypeError, ValueError):
            finished = None
        if finished is None:
            return self.ttl_seconds
        age = max(time.time() - finished.timestamp(), 0.0)
        return max(self.ttl_seconds - age, 0.0)

    async def _fail_interrupted(self, wf: Dict[str, Any]) -> None:
        status = dict(wf.get("status") or {})
        status.update(phase="Failed", finishedAt=_now_iso(),
                      message=self.INTERRUPTED_MESSAGE)
        await self._set_status(wf, status)
        self._schedule_ttl(wf)

    async def _run(self, wf: Dict[str, Any]) -> None:  # pragma: no cover - abstract
        raise NotImplementedError

    def _schedule_ttl(self, wf: Dict[str, Any], delay: Optional[float] = None) -> None:
        if self.ttl_seconds is None:
            return
        if delay is None:
            delay = self.ttl_seconds
        meta = wf["metadata"]
        ns, name = meta.get("namespace", ""), meta["name"]

        def _gc() -> None:
            async def delete() -> None:
                try:
                    await self.client.delete(WF_API_VERSION, WF_KIND, ns, name)
                except Exception:
                    pass

            task = asyncio.ensure_future(delete())
            self._inflight[f"ttl:{ns}/{name}"] = task
            task.add_done_callback(
                lambda t: self._inflight.pop(f"ttl:{ns}/{name}", None)
            )

        loop = asyncio.get_event_loop()
        self._ttl_handles.append(loop.call_later(delay, _gc))
        # handles are appended in firing order (constant ttl; start() arms
        # the remaining TTLs of recovered workflows first, shortest first,
        # and none exceeds ttl): drop spent ones from the front — O(1)
        # amortized
        now = loop.time()
        while self._ttl_handles and (
            self._ttl_handles[0].cancelled() or self._ttl_handles[0].when() <= now
        ):
            self._ttl_handles.popleft()

    async def _set_status(self, wf: Dict[str, Any], status: Dict[str, Any]) -> bool:
        """Write the Workflow status the way the Argo controller does (the
        Workflow CRD has no status subresource — a plain update). False when
        the Workflow is gone."""
        meta = wf["metadata"]
        for _ in range(5):
            try:
                fresh = await self.client.get(
                    WF_API_VERSION, WF_KIND, meta.get("namespace", ""), meta["name"]
                )
            except NotFoundError:
                return False
            fresh["status"] = status
            try:
                await self.client.update(fresh)
                return True
            except ConflictError:
                await asyncio.sleep(0.005)
        return True


class ScriptedWorkflowEngine(_EngineBase):
    def __init__(
        self,
        client: KubeClient,
        policy: Policy = always_succeed,
        delay: float = 0.0,
        namespace: Optional[str] = None,
        ttl_seconds: Optional[float] = _EngineBase.DEFAULT_TTL,
        recover: bool = False,
        parallelism: Optional[int] = None,
        namespace_parallelism: Optional[int] = None,
        max_processes: Optional[int] = None,  # accepted, starts no processes
    ):
        super().__init__(client, namespace, ttl_seconds, recover, parallelism,
                         namespace_parallelism, max_processes)
        self.policy = policy
        self.delay = delay
        self.completed = 0

    async def _run(self, wf: Dict[str, Any]) -> None:
        decision = self.policy(wf)
        if decision is None:
            return  # leave pending: the controller's IEB timeout takes over
        if self.delay > 0:
            # instant completions skip the intermediate Running write — one
            # status update (and one spurious watcher wakeup) less per run
            await self._set_status(wf, {"phase": "Running", "startedAt": _now_iso()})
            await asyncio.sleep(self.delay)
        phase, message = decision[0], decision[1]
        status: Dict[str, Any] = {"phase": phase, "finishedAt": _now_iso()}
        if message:
            status["message"] = message
        if len(decision) > 2 and decision[2]:  # type: ignore[misc]
            status["outputs"] = decision[2]  # type: ignore[misc]
        await self._set_status(wf, status)
        self._schedule_ttl(wf)
        self.completed += 1


def _now_iso() -> str:
    from ..api.types import k8s_now

    return k8s_now()


class LocalWorkflowEngine(_EngineBase):
    """Executes Argo-shaped workflows locally, one subprocess per leaf.

    Supported surface (docs/OPERATIONS.md has the full list and what is
    deliberately absent):

    - ``container`` (command+args run as a local process; ``image`` is
      informational without a container runtime) and ``script`` (source piped
      to the interpreter) leaves, with ``env`` name/value pairs; ``suspend``;
    - ``steps`` (sequential groups of parallel steps) and ``dag`` templates
      (``dependencies`` / ``depends: "a && b"``, fail-fast by default);
    - ``withItems`` / ``withParam`` fan-out and ``when`` conditions on steps
      and tasks;
    - parameters: ``spec.arguments``, template ``inputs``, ``{{item}}``,
      ``{{retries}}``, ``{{workflow.*}}`` and ``{{steps|tasks.X.outputs.*}}``,
      substituted in one pass and never re-split into argv elements;
    - outputs: ``outputs.result`` (stdout), ``valueFrom.path`` (the leaf then
      runs in a throw-away working directory), ``valueFrom.parameter`` on
      composite templates, and ``globalName`` surfacing into
      ``status.outputs.parameters`` (the custom-metrics contract,
      README.md:275-285);
    - ``retryStrategy`` with ``limit`` and ``backoff``;
    - ``spec.onExit`` with ``{{workflow.status}}``;
    - shared templates: ``templateRef`` on steps and tasks and
      ``spec.workflowTemplateRef``, resolved once per Workflow from a
      watch-fed cache of WorkflowTemplates and ClusterWorkflowTemplates, before
      admission reads the spec (:mod:`.templates`);
    - workflow-level ``activeDeadlineSeconds``. Every leaf runs in its own
      process group, which is killed when the deadline passes or the engine
      stops.

    The spec is checked by :func:`~.validate.validate_workflow_spec` before
    anything starts. Status is written twice per workflow (``Running``, then
    the terminal phase); the terminal write carries ``status.nodes``, one
    entry per step, so a user can see which task of a DAG failed.
    """

    def __init__(self, client: KubeClient, namespace: Optional[str] = None,
                 ttl_seconds: Optional[float] = _EngineBase.DEFAULT_TTL,
                 recover: bool = False, logs: Any = None,
                 parallelism: Optional[int] = None,
                 namespace_parallelism: Optional[int] = None,
                 max_processes: Optional[int] = None):
        super().__init__(client, namespace, ttl_seconds, recover, parallelism,
                         namespace_parallelism, max_processes)
        from .executor import Bound

        self.completed = 0
        #: the leaf processes of all runs; holds at most ``max_processes``
        self.process_slots = Bound(self.max_processes)
        #: a :class:`~.logs.LogStore` for what the leaves print, or None;
        #: whoever built it closes it
        self.logs = logs
        # shared templates, fed by a watch per kind: (cluster scope,
        # namespace or "", name) → object. Objects are replaced, never
        # changed in place, so a run keeps what it resolved against.
        self._templates: Dict[Tuple[bool, str, str], Dict[str, Any]] = {}
        self._template_subs: List[Any] = []
        self._template_tasks: List["asyncio.Future[Any]"] = []
        #: what :meth:`_submit` resolved, until :meth:`_run` takes it
        self._resolved: Dict[str, Any] = {}
        #: direct reads made for a name the cache did not have
        self.template_reads = 0

    async def start(self) -> None:
        # the cache is whole before the first Workflow is looked at; watch
        # first, then list, so that nothing created in between is missed
        for kind, namespace in ((WFT_KIND, self.namespace), (CWFT_KIND, None)):
            sub = self.client.watch(WF_API_VERSION, kind, namespace)
            self._template_subs.append(sub)
            for obj in await self.client.list(WF_API_VERSION, kind, namespace):
                self._cache_template(obj)
            self._template_tasks.append(asyncio.ensure_future(self._follow_templates(sub)))
        await super().start()

    @staticmethod
    def _template_key(obj: Dict[str, Any]) -> Tuple[bool, str, str]:
        meta = obj.get("metadata") or {}
        cluster = obj.get("kind") == CWFT_KIND
        return cluster, "" if cluster else meta.get("namespace", ""), meta.get("name", "")

    def _cache_template(self, obj: Dict[str, Any]) -> None:
        """Keep ``obj`` unless what is cached is newer (a direct read and
        the watch may deliver the same object in either order)."""
        key = self._template_key(obj)
        have = self._templates.get(key)
        if have is not None:
            try:
                if (int(have["metadata"]["resourceVersion"])
                        > int(obj["metadata"]["resourceVersion"])):
                    return
            except (KeyError, TypeError, ValueError):
                pass  # opaque resourceVersion: the later arrival stands
        self._templates[key] = obj

    async def _follow_templates(self, sub: Any) -> None:
        async for ev in sub:
            if ev["type"] == "DELETED":
                self._templates.pop(self._template_key(ev["object"]), None)
            elif ev["type"] in ("ADDED", "MODIFIED"):
                self._cache_template(ev["object"])

    def _resolve(self, wf: Dict[str, Any]) -> Any:
        """``wf``'s spec resolved against the cache; namespaced names are
        looked up in the Workflow's namespace."""
        ns = wf["metadata"].get("namespace", "")
        return resolve(wf["spec"], lambda cluster, name: self._templates.get(
            (cluster, "" if cluster else ns, name)))

    def cached_templates(self) -> List[str]:
        """What the cache holds, sorted: ``namespaced/NAMESPACE/NAME`` and
        ``cluster/NAME``."""
        return sorted(f"cluster/{name}" if cluster else f"namespaced/{ns}/{name}"
                      for cluster, ns, name in self._templates)

    def cached_template(self, name: str, namespace: str = "",
                        cluster: bool = False) -> Optional[Dict[str, Any]]:
        """The cached object of that name, None when there is none; read-only."""
        return self._templates.get((cluster, "" if cluster else namespace, name))

    def _submit(self, wf: Dict[str, Any], recovering: bool = False) -> None:
        # this runs in the watch loop: whatever one Workflow's spec holds,
        # the Workflows after it are still looked at
        try:
            found = self._resolve(wf) if has_references(wf.get("spec")) else None
        except Exception:
            log.exception("workflow %s/%s: references not resolved, taken as it is",
                          wf["metadata"].get("namespace", ""), wf["metadata"].get("name"))
            found = None
        if found is None:
            super()._submit(wf, recovering)
            return
        if found.missing:
            self._spawn(wf, self._confirm_missing(wf, found), "resolve:")
            return
        self._take_up(wf, found, recovering)

    def _take_up(self, wf: Dict[str, Any], found: Any, recovering: bool = False) -> None:
        meta = wf["metadata"]
        self._resolved[f'{meta.get("namespace", "")}/{meta["name"]}'] = found
        if found.errors:
            self._spawn(wf, self._run(wf))  # fails at once: nothing to wait for
        else:
            super()._submit(wf, recovering)

    async def _confirm_missing(self, wf: Dict[str, Any], found: Any) -> None:
        """A name the cache lacks is read once from the apiserver before the
        Workflow is failed for it: a template applied in the same instant as
        its user may not have come down the watch yet. The task is cancelled
        when the Workflow is deleted meanwhile (:meth:`_deleted`).

        A Workflow recovered at start that comes through here is admitted
        when its reads are done, not in the ordered pass over what start()
        found; the cache was primed by a list just before, so this takes a
        template created in that very moment."""
        ns = wf["metadata"].get("namespace", "")
        asked: set = set()
        while True:
            wanted = [m for m in found.missing if m not in asked]
            if not wanted:
                break
            for cluster, name in wanted:
                asked.add((cluster, name))
                self.template_reads += 1
                try:
                    self._cache_template(await self.client.get(
                        WF_API_VERSION, CWFT_KIND if cluster else WFT_KIND,
                        "" if cluster else ns, name))
                except NotFoundError:
                    pass
            found = self._resolve(wf)
        if not self._stopping:
            self._take_up(wf, found)

    def _spec_of(self, wf: Dict[str, Any]) -> Any:
        meta = wf["metadata"]
        found = self._resolved.get(f'{meta.get("namespace", "")}/{meta["name"]}')
        return found.spec if found is not None else wf.get("spec")

    def _processes(self) -> int:
        return self.process_slots.held

    def _deleted(self, wf: Dict[str, Any]) -> None:
        meta = wf["metadata"]
        key = f'{meta.get("namespace", "")}/{meta["name"]}'
        self._resolved.pop(key, None)
        confirming = self._inflight.get(f"resolve:{key}")
        if confirming is not None:
            confirming.cancel()  # not taken up: there is nothing to run any more
        if self.logs is not None:
            self.logs.discard(meta.get("namespace", ""), meta["name"])

    async def _fail_expired(self, entry: _Queued) -> None:
        self._resolved.pop(entry.key, None)
        await super()._fail_expired(entry)

    async def stop(self) -> None:
        inflight = list(self._inflight.values())
        for sub in self._template_subs:
            sub.close()
        for task in self._template_tasks:
            task.cancel()
        await asyncio.gather(*self._template_tasks, return_exceptions=True)
        self._template_subs, self._template_tasks = [], []
        await super().stop()
        # cancelled runs kill and reap their process groups before they end
        if inflight:
            await asyncio.gather(*inflight, return_exceptions=True)

    async def _run(self, wf: Dict[str, Any]) -> None:
        from .executor import WorkflowRun
        from .validate import ignored_synchronization, validate_workflow_spec

        meta = wf["metadata"]
        ns, name = meta.get("namespace", ""), meta["name"]
        # resolved once, when the Workflow was taken up: the run reads this
        # snapshot, whatever happens to the shared templates meanwhile
        found = self._resolved.pop(f"{ns}/{name}", None)
        spec = (found.spec if found is not None else wf.get("spec")) or {}
        recorded: Dict[str, Any] = {}
        if found is not None and not found.errors:
            if found.stored_spec is not None:
                recorded["storedWorkflowTemplateSpec"] = found.stored_spec
            if found.stored:
                recorded["storedTemplates"] = found.stored
        logs = self.logs
        if logs is not None:
            try:
                logs.start_run(ns, name)
            except (OSError, ValueError) as e:
                log.warning("no logs kept for workflow %s/%s: %s", ns, name, e)
                logs = None
        await self._set_status(wf, {"phase": "Running", "startedAt": _now_iso(), **recorded})
        nodes: Dict[str, Any] = {}
        outputs: List[Dict[str, Any]] = []
        if found is not None and found.errors:
            problems = [found.errors[0][1]]
        else:
            problems = validate_workflow_spec(spec, found)
        if problems:
            phase, message = "Failed", problems[0]
        else:
            ignored = ignored_synchronization(spec, found)
            if ignored:
                log.warning("workflow %s/%s: %s not supported and ignored",
                            ns, name, " and ".join(ignored))
            run = WorkflowRun(spec, name, ns, logs=logs, process_slots=self.process_slots,
                              templates=found.scopes if found is not None else None)
            try:
                phase, message, timed_out = await self._run_phases(run, spec)
            except asyncio.CancelledError:
                run.terminate("engine stopped")
                if logs is not None:
                    logs.finish_run(ns, name)
                raise
            nodes = run.nodes
            if not timed_out:  # a run that was cut short publishes no outputs
                outputs = run.global_outputs
        status: Dict[str, Any] = {"phase": phase, "finishedAt": _now_iso(), **recorded}
        if message:
            status["message"] = message
        if outputs:
            status["outputs"] = {"parameters": outputs}
        if nodes:
            status["nodes"] = nodes
        exists = True
        try:
            exists = await self._set_status(wf, status)
        finally:
            if logs is not None:
                logs.finish_run(ns, name)
                if not exists:
                    # deleted while it ran: its DELETED event came before
                    # the last nodes wrote
                    logs.discard(ns, name)
        self._schedule_ttl(wf)
        self.completed += 1

    async def _run_phases(self, run: Any, spec: Dict[str, Any]) -> Tuple[Phase, str, bool]:
        """The entrypoint, then the exit handler. Each gets the workflow's
        ``activeDeadlineSeconds`` as a budget of its own, so the handler
        still runs after the entrypoint used up the deadline. Returns
        ``(phase, message, timed_out)``."""
        phase, message, timed_out = await self._bounded(
            run, run.run_entrypoint(), spec, "deadline exceeded"
        )
        if spec.get("onExit"):
            exit_phase, exit_message, exit_timed_out = await self._bounded(
                run, run.run_exit_handler(phase), spec, "exit handler: deadline exceeded"
            )
            timed_out = timed_out or exit_timed_out
            if exit_phase == "Failed":
                if phase != "Failed":
                    message = exit_message
                phase = "Failed"
        return phase, message, timed_out

    @staticmethod
    async def _bounded(run: Any, coro: Any, spec: Dict[str, Any],
                       timeout_message: str) -> Tuple[Phase, str, bool]:
        deadline = spec.get("activeDeadlineSeconds")
        try:
            if deadline:
                phase, message = await asyncio.wait_for(coro, float(deadline))
            else:
                phase, message = await coro
            return phase, message, False
        except asyncio.TimeoutError:
            run.terminate(timeout_message)
            return "Failed", timeout_message, True
        except asyncio.CancelledError:
            raise
        except Exception as e:
            coro.close()  # no-op unless it never started (bad deadline value)
            run.terminate(str(e))
            return "Failed", str(e), False

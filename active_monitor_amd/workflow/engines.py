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

Who may start, and in what order, is decided by :mod:`.admission`; the shared
templates are kept by :mod:`.template_cache`. What is here is the life of one
Workflow: its status writes, its timers and its tasks.
"""
from __future__ import annotations

import asyncio
import functools
import logging
import time
from collections import deque
from typing import Any, Callable, Dict, List, Optional, Tuple

from ..api.types import k8s_now, parse_k8s_time
from ..kube.client import KubeClient
from ..kube.errors import ConflictError, NotFoundError
from ..kube.registry import WF_API_VERSION, WF_KIND
from .admission import (  # noqa: F401 - the names were born here and stay importable
    POSTPONED_MESSAGE,
    QUEUE_EXPIRED_MESSAGE,
    Admission,
    Entry,
    _positive,
    _priority,
    mutex_names,
)
from .template_cache import TemplateCache
from .templates import has_references, resolve

log = logging.getLogger("active_monitor_amd.workflow")

Phase = str  # "Pending" | "Running" | "Succeeded" | "Failed"

PolicyResult = Optional[Tuple[Phase, str]]
Policy = Callable[[Dict[str, Any]], PolicyResult]


def always_succeed(wf: Dict[str, Any]) -> PolicyResult:
    return ("Succeeded", "")


def always_fail(wf: Dict[str, Any]) -> PolicyResult:
    return ("Failed", "workflow failed")


def never_complete(wf: Dict[str, Any]) -> PolicyResult:
    return None


def _key(wf: Dict[str, Any]) -> str:
    meta = wf["metadata"]
    return f'{meta.get("namespace", "")}/{meta["name"]}'


class _Record:
    """A Workflow the engine has taken up, from its ``ADDED`` event (or the
    start-up list) until its run has ended, or it was deleted or has expired
    before it ran. Each task is None before it is started.

    ``found``       the spec resolved against the shared templates, if it
                    refers to any: the snapshot that admission and the run read
    ``entry``       its place in the admission queue, while it waits there
    ``pending``     its one ``Pending`` write, which the next write to the
                    same Workflow waits for
    ``expiry``      the timer of its deadline in the queue
    ``confirming``  the direct reads of templates the cache lacks
    ``run``         its run
    """

    __slots__ = ("wf", "key", "found", "entry", "pending", "expiry", "confirming", "run")

    def __init__(self, wf: Dict[str, Any], key: str):
        self.wf = wf
        self.key = key
        self.found: Any = None
        self.entry: Optional[Entry] = None
        self.pending: Optional["asyncio.Future[Any]"] = None
        self.expiry: Optional[asyncio.TimerHandle] = None
        self.confirming: Optional["asyncio.Future[Any]"] = None
        self.run: Optional["asyncio.Future[Any]"] = None

    @property
    def spec(self) -> Any:
        """The spec that admission reads: priority, mutexes, the deadline
        that runs in the queue."""
        return self.found.spec if self.found is not None else self.wf.get("spec")


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
        self._admission = Admission(parallelism, namespace_parallelism)
        self.parallelism = self._admission.parallelism
        self.namespace_parallelism = self._admission.namespace_parallelism
        self.max_processes = _positive("max_processes", max_processes)
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
        # by key: the newest Workflow of that name. A run outlives its
        # Workflow's deletion, so the run of an earlier one may still be
        # going; its record is reachable from its task alone.
        self._records: Dict[str, _Record] = {}
        #: every task started and not yet done, whatever it is for
        self._tasks: set = set()
        self._running = 0
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
            if len(self._admission):
                # everything the list held is in the queue: admit in order
                self._pump()
                for entry in self._admission:
                    self._postpone(self._records[entry.key])
        log.info("workflow engine limits: parallelism=%s namespace_parallelism=%s "
                 "max_processes=%s", *(
                     "unlimited" if v is None else v for v in self.limits().values()))
        self._task = asyncio.ensure_future(self._loop())

    async def stop(self) -> None:
        # what is queued stays Pending, for a restart over the same store
        self._stopping = True
        for rec in self._records.values():
            if rec.expiry is not None:
                rec.expiry.cancel()
        if self._sub is not None:
            self._sub.close()
        if self._task is not None:
            self._task.cancel()
            try:
                await self._task
            except (asyncio.CancelledError, Exception):
                pass
        for t in self._tasks:
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
        """The Workflow is gone: TTL, owner cascade or a user's delete. One
        that has not started never runs; a run goes on until it ends."""
        rec = self._records.get(_key(wf))
        if rec is None or rec.run is not None:
            return
        del self._records[rec.key]
        if rec.entry is not None:
            self._admission.remove(rec.key)
            rec.entry = None
        if rec.expiry is not None:
            rec.expiry.cancel()
        if rec.confirming is not None:
            rec.confirming.cancel()  # not taken up: there is nothing to run any more

    def _spawn(self, coro: Any, run_of: Optional[_Record] = None) -> "asyncio.Future[Any]":
        """Every task starts here. ``run_of``: the task is that record's run."""
        task = asyncio.ensure_future(coro)
        self._tasks.add(task)
        if run_of is None:
            task.add_done_callback(self._tasks.discard)
        else:
            self._running += 1
            run_of.run = task
            task.add_done_callback(functools.partial(self._ended, run_of))
        return task

    def _ended(self, rec: _Record, run: Any) -> None:
        self._tasks.discard(run)
        self._running -= 1
        # a Workflow created since under the same name has a record of its own
        if self._records.get(rec.key) is rec:
            del self._records[rec.key]

    def limits(self) -> Dict[str, Optional[int]]:
        return {"parallelism": self.parallelism,
                "namespace_parallelism": self.namespace_parallelism,
                "max_processes": self.max_processes}

    def stats(self) -> Dict[str, Any]:
        """Counters for ``/statusz``. ``running`` counts the runs in flight,
        admitted or never queued; ``processes`` the leaf processes alive."""
        return {
            "running": self._running,
            "queued": len(self._admission),
            "postponed_total": self.postponed_total,
            "expired_in_queue": self.expired_in_queue,
            "processes": self._processes(),
            "limits": self.limits(),
        }

    def _processes(self) -> int:
        return 0

    # -- one Workflow, from its ADDED event to the end of its run ------------

    def _submit(self, wf: Dict[str, Any], recovering: bool = False) -> None:
        """``recovering``: only queue it, start() admits once all that it
        found is queued."""
        key = _key(wf)
        have = self._records.get(key)
        if have is not None and have.run is None:
            return  # queued already, or its templates are being read
        rec = self._records[key] = _Record(wf, key)
        self._take_up(rec, recovering)

    def _take_up(self, rec: _Record, recovering: bool = False) -> None:
        """Run ``rec`` now, or queue it when a limit or a mutex may stand in
        its way."""
        meta = rec.wf["metadata"]
        rec.entry = self._admission.offer(rec.key, meta.get("namespace", ""), rec.spec,
                                          meta.get("creationTimestamp"))
        if rec.entry is None:
            self._spawn(self._run(rec), rec)
        elif not recovering:
            self._pump()
            if rec.entry is not None:
                self._postpone(rec)

    def _pump(self) -> None:
        """Start every Workflow that admission lets through."""
        if self._stopping:
            return
        for entry in self._admission.admit():
            rec = self._records[entry.key]
            rec.entry = None
            if rec.expiry is not None:
                rec.expiry.cancel()
            self._spawn(self._run_admitted(rec, entry), rec)

    async def _run_admitted(self, rec: _Record, entry: Entry) -> None:
        try:
            if rec.pending is not None:
                await asyncio.wait([rec.pending])  # Pending lands before Running
            await self._run(rec)
        finally:
            self._admission.release(entry)
            self._pump()

    def _postpone(self, rec: _Record) -> None:
        """``rec`` stays in the queue: write ``Pending`` once and start the
        clock of its deadline."""
        self.postponed_total += 1
        wf = rec.wf
        if (wf.get("status") or {}).get("phase") != "Pending":  # else: recovered
            message = self._admission.blocked_by(rec.entry) or POSTPONED_MESSAGE
            rec.pending = self._spawn(
                self._set_status(wf, {"phase": "Pending", "message": message}))
        spec = rec.spec
        deadline = spec.get("activeDeadlineSeconds") if isinstance(spec, dict) else None
        try:
            deadline = float(deadline) if deadline and deadline is not True else 0.0
        except (TypeError, ValueError):
            deadline = 0.0
        if deadline > 0:
            rec.expiry = asyncio.get_event_loop().call_later(deadline, self._expire, rec)

    def _expire(self, rec: _Record) -> None:
        if rec.entry is None:
            return
        self._admission.remove(rec.key)
        rec.entry = None
        del self._records[rec.key]
        self.expired_in_queue += 1
        log.warning("workflow %s waited out its activeDeadlineSeconds in the "
                    "queue: failing it", rec.key)
        self._spawn(self._fail_expired(rec))

    async def _fail_expired(self, rec: _Record) -> None:
        if rec.pending is not None:
            await asyncio.wait([rec.pending])
        await self._set_status(rec.wf, {
            "phase": "Failed", "finishedAt": k8s_now(), "message": QUEUE_EXPIRED_MESSAGE,
        })
        self._schedule_ttl(rec.wf)

    def _recover(self, wf: Dict[str, Any], finished: List[Any]) -> None:
        """Handle one Workflow found at start by the state it is in; a
        terminal one is appended to ``finished`` as ``(ttl left, wf)`` for
        the caller to schedule."""
        meta = wf["metadata"]
        key = _key(wf)
        rec = self._records.get(key)
        if rec is not None and rec.run is not None:
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
            self._spawn(self._fail_interrupted(wf))

    def _ttl_left(self, finished_at: Any) -> float:
        """``ttl_seconds`` less the time since ``finishedAt``, floored at 0;
        a missing or unparsable ``finishedAt`` counts from now."""
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
        status.update(phase="Failed", finishedAt=k8s_now(),
                      message=self.INTERRUPTED_MESSAGE)
        await self._set_status(wf, status)
        self._schedule_ttl(wf)

    async def _run(self, rec: _Record) -> None:  # pragma: no cover - abstract
        raise NotImplementedError

    def _schedule_ttl(self, wf: Dict[str, Any], delay: Optional[float] = None) -> None:
        if self.ttl_seconds is None:
            return
        if delay is None:
            delay = self.ttl_seconds
        meta = wf["metadata"]
        loop = asyncio.get_event_loop()
        # no closure here: whatever the timer holds lives as long as the TTL
        self._ttl_handles.append(loop.call_later(
            delay, self._ttl_over, meta.get("namespace", ""), meta["name"]))
        # handles are appended in firing order (constant ttl; start() arms
        # the remaining TTLs of recovered workflows first, shortest first,
        # and none exceeds ttl): drop spent ones from the front — O(1)
        # amortized
        now = loop.time()
        while self._ttl_handles and (
            self._ttl_handles[0].cancelled() or self._ttl_handles[0].when() <= now
        ):
            self._ttl_handles.popleft()

    def _ttl_over(self, ns: str, name: str) -> None:
        self._spawn(self._delete(ns, name))

    async def _delete(self, ns: str, name: str) -> None:
        try:
            await self.client.delete(WF_API_VERSION, WF_KIND, ns, name)
        except Exception:
            pass

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

    async def _run(self, rec: _Record) -> None:
        wf = rec.wf
        decision = self.policy(wf)
        if decision is None:
            return  # leave pending: the controller's IEB timeout takes over
        if self.delay > 0:
            # instant completions skip the intermediate Running write — one
            # status update (and one spurious watcher wakeup) less per run
            await self._set_status(wf, {"phase": "Running", "startedAt": k8s_now()})
            await asyncio.sleep(self.delay)
        phase, message = decision[0], decision[1]
        status: Dict[str, Any] = {"phase": phase, "finishedAt": k8s_now()}
        if message:
            status["message"] = message
        if len(decision) > 2 and decision[2]:  # type: ignore[misc]
            status["outputs"] = decision[2]  # type: ignore[misc]
        await self._set_status(wf, status)
        self._schedule_ttl(wf)
        self.completed += 1


class LocalWorkflowEngine(_EngineBase):
    """Executes Argo-shaped workflows locally: one subprocess per container
    or script leaf, one socket per ``http`` leaf.

    Supported surface (docs/OPERATIONS.md has the full list and what is
    deliberately absent):

    - ``container`` (command+args run as a local process; ``image`` is
      informational without a container runtime) and ``script`` (source piped
      to the interpreter) leaves, with ``env`` name/value pairs; ``suspend``;
    - ``http`` leaves: one request sent from the event loop itself, without
      a process (:mod:`.httpprobe`), judged by its status or by a
      ``successCondition`` (:mod:`.expr`); at most ``HTTP_MAX_IN_FLIGHT``
      over all runs, and none of them counts against ``max_processes``;
    - ``steps`` (sequential groups of parallel steps) and ``dag`` templates
      (``dependencies`` / ``depends: "a && b"``, fail-fast by default);
    - ``withItems`` / ``withParam`` / ``withSequence`` fan-out, ``when``
      conditions and ``continueOn: {failed: true}`` on steps and tasks;
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
      admission reads the spec (:mod:`.templates`, :mod:`.template_cache`);
    - workflow-level ``activeDeadlineSeconds``. Every leaf runs in its own
      process group, which is killed when the deadline passes or the engine
      stops;
    - per-step deadlines, cut the same way: a template's
      ``activeDeadlineSeconds`` bounds one attempt of a ``container`` or
      ``script`` leaf from the start of its process, its ``timeout`` a
      ``container``, ``script``, ``http`` or ``suspend`` node as a whole,
      slot waits, retries and backoff waits included.

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
        from .executor import HTTP_MAX_IN_FLIGHT, Bound

        self.completed = 0
        #: the leaf processes of all runs; holds at most ``max_processes``
        self.process_slots = Bound(self.max_processes)
        #: the HTTP probes of all runs; they are no processes and are not
        #: counted in :meth:`stats`
        self.http_slots = Bound(HTTP_MAX_IN_FLIGHT)
        #: a :class:`~.logs.LogStore` for what the leaves print, or None;
        #: whoever built it closes it
        self.logs = logs
        self._templates = TemplateCache(client, namespace)

    async def start(self) -> None:
        # the cache is whole before the first Workflow is looked at
        await self._templates.start()
        await super().start()

    @property
    def template_reads(self) -> int:
        """Direct reads made for a name the cache did not have."""
        return self._templates.reads

    def cached_templates(self) -> List[str]:
        """What the cache holds, sorted: ``namespaced/NAMESPACE/NAME`` and
        ``cluster/NAME``."""
        return self._templates.names()

    def cached_template(self, name: str, namespace: str = "",
                        cluster: bool = False) -> Optional[Dict[str, Any]]:
        """The cached object of that name, None when there is none; read-only."""
        return self._templates.get(name, namespace, cluster)

    def _take_up(self, rec: _Record, recovering: bool = False) -> None:
        # this runs in the watch loop: whatever one Workflow's spec holds,
        # the Workflows after it are still looked at
        wf = rec.wf
        try:
            found = resolve(wf["spec"], self._templates.lookup(
                wf["metadata"].get("namespace", ""))) if has_references(wf.get("spec")) else None
        except Exception:
            log.exception("workflow %s/%s: references not resolved, taken as it is",
                          wf["metadata"].get("namespace", ""), wf["metadata"].get("name"))
            found = None
        if found is not None and found.missing:
            rec.confirming = self._spawn(self._confirm_missing(rec, found))
        else:
            self._take_up_resolved(rec, found, recovering)

    def _take_up_resolved(self, rec: _Record, found: Any, recovering: bool = False) -> None:
        rec.found = found
        if found is not None and found.errors:
            self._spawn(self._run(rec), rec)  # fails at once: nothing to wait for
        else:
            super()._take_up(rec, recovering)

    async def _confirm_missing(self, rec: _Record, found: Any) -> None:
        """A name the cache lacks is read once from the apiserver before the
        Workflow is failed for it: a template applied in the same instant as
        its user may not have come down the watch yet. The task is cancelled
        when the Workflow is deleted meanwhile (:meth:`_deleted`).

        A Workflow recovered at start that comes through here is admitted
        when its reads are done, not in the ordered pass over what start()
        found; the cache was primed by a list just before, so this takes a
        template created in that very moment."""
        wf = rec.wf
        found = await self._templates.read_missing(
            wf["spec"], wf["metadata"].get("namespace", ""), found)
        rec.confirming = None
        if not self._stopping:
            self._take_up_resolved(rec, found)

    def _processes(self) -> int:
        return self.process_slots.held

    def _deleted(self, wf: Dict[str, Any]) -> None:
        super()._deleted(wf)
        if self.logs is not None:
            self.logs.discard(wf["metadata"].get("namespace", ""), wf["metadata"]["name"])

    async def stop(self) -> None:
        await self._templates.stop()
        await super().stop()
        # cancelled runs kill and reap their process groups before they end
        await asyncio.gather(*self._tasks, return_exceptions=True)

    async def _run(self, rec: _Record) -> None:
        from .executor import WorkflowRun
        from .validate import ignored_synchronization, validate_workflow_spec

        wf = rec.wf
        meta = wf["metadata"]
        ns, name = meta.get("namespace", ""), meta["name"]
        # resolved once, when the Workflow was taken up: the run reads this
        # snapshot, whatever happens to the shared templates meanwhile
        found = rec.found
        spec = rec.spec or {}
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
        await self._set_status(wf, {"phase": "Running", "startedAt": k8s_now(), **recorded})
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
                              templates=found.scopes if found is not None else None,
                              http_slots=self.http_slots)
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
        status: Dict[str, Any] = {"phase": phase, "finishedAt": k8s_now(), **recorded}
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

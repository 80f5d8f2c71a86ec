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
import logging
import time
from typing import Any, Callable, Dict, List, Optional, Tuple

from ..kube.client import KubeClient
from ..kube.errors import ConflictError, NotFoundError
from ..kube.registry import WF_API_VERSION, WF_KIND

log = logging.getLogger("active_monitor_amd.workflow")

Phase = str  # "Running" | "Succeeded" | "Failed"

PolicyResult = Optional[Tuple[Phase, str]]
Policy = Callable[[Dict[str, Any]], PolicyResult]


def always_succeed(wf: Dict[str, Any]) -> PolicyResult:
    return ("Succeeded", "")


def always_fail(wf: Dict[str, Any]) -> PolicyResult:
    return ("Failed", "workflow failed")


def never_complete(wf: Dict[str, Any]) -> PolicyResult:
    return None


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
    terminal gets its lost TTL timer re-armed for the time it has left."""

    DEFAULT_TTL = 1800.0
    INTERRUPTED_MESSAGE = "workflow interrupted: engine restarted"

    def __init__(self, client: KubeClient, namespace: Optional[str] = None,
                 ttl_seconds: Optional[float] = DEFAULT_TTL,
                 recover: bool = False):
        self.client = client
        self.namespace = namespace
        self.ttl_seconds = ttl_seconds
        self.recover = recover
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
        self._task = asyncio.ensure_future(self._loop())

    async def stop(self) -> None:
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
                self._deleted(wf)
            if ev["type"] != "ADDED":
                continue
            if (wf.get("status") or {}).get("phase") in ("Succeeded", "Failed"):
                continue
            self._spawn(wf, self._run(wf))

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

    def _spawn(self, wf: Dict[str, Any], coro: Any) -> None:
        key = f'{(wf["metadata"].get("namespace", ""))}/{wf["metadata"]["name"]}'
        task = asyncio.ensure_future(coro)
        self._inflight[key] = task
        task.add_done_callback(lambda t, k=key: self._inflight.pop(k, None))

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
        if phase and phase != "Running":
            return  # a phase no local engine writes: not ours to touch
        if meta.get("uid"):
            self._recovered.add(meta["uid"])
            try:
                self._recovered_rv = max(self._recovered_rv,
                                         int(meta.get("resourceVersion")))
            except (TypeError, ValueError):
                pass
        if not phase:
            log.info("recovering pending workflow %s", key)
            self._spawn(wf, self._run(wf))
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
    ):
        super().__init__(client, namespace, ttl_seconds, recover)
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
                 recover: bool = False, logs: Any = None):
        super().__init__(client, namespace, ttl_seconds, recover)
        self.completed = 0
        #: a :class:`~.logs.LogStore` for what the leaves print, or None;
        #: whoever built it closes it
        self.logs = logs

    def _deleted(self, wf: Dict[str, Any]) -> None:
        if self.logs is not None:
            meta = wf["metadata"]
            self.logs.discard(meta.get("namespace", ""), meta["name"])

    async def stop(self) -> None:
        inflight = list(self._inflight.values())
        await super().stop()
        # cancelled runs kill and reap their process groups before they end
        if inflight:
            await asyncio.gather(*inflight, return_exceptions=True)

    async def _run(self, wf: Dict[str, Any]) -> None:
        from .executor import WorkflowRun
        from .validate import validate_workflow_spec

        spec = wf.get("spec") or {}
        meta = wf["metadata"]
        ns, name = meta.get("namespace", ""), meta["name"]
        logs = self.logs
        if logs is not None:
            try:
                logs.start_run(ns, name)
            except (OSError, ValueError) as e:
                log.warning("no logs kept for workflow %s/%s: %s", ns, name, e)
                logs = None
        await self._set_status(wf, {"phase": "Running", "startedAt": _now_iso()})
        nodes: Dict[str, Any] = {}
        outputs: List[Dict[str, Any]] = []
        problems = validate_workflow_spec(spec)
        if problems:
            phase, message = "Failed", problems[0]
        else:
            run = WorkflowRun(spec, name, ns, logs=logs)
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
        status: Dict[str, Any] = {"phase": phase, "finishedAt": _now_iso()}
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

"""The HealthCheck reconciler — the heart of the framework.

Re-implements every behavior of the reference's 1,485-line reconciler
(internal/controllers/healthcheck_controller.go) with one deliberate
architectural change (SURVEY.md §7 "the single biggest architectural
decision"): the workflow watch never blocks a reconcile worker — it runs as a
detached asyncio task — and repeat timers feed back through the workqueue, so
``MaxConcurrentReconciles`` genuinely bounds reconcile work and repeats are
reconcile-driven (picking up fresh spec, recomputing cron intervals every
cycle — the reference's bare ``time.AfterFunc`` repeats re-use stale values,
:479-500,:746-755).

Behavior contracts kept bit-for-bit:

- schedule branches: pause → ``Stopped`` + explanatory ErrorMessage (:238-250),
  cron → ``RepeatAfterSec = int(next−now)+1`` (:251-263), already-scheduled
  dedup (:264-267),
- RBAC provision → parse → submit (ownerRef, generateName, instance-id label,
  podGC, activeDeadlineSeconds) → watch with inverse-exponential backoff →
  status mutation + metrics → remedy state machine → re-arm timer,
- IEB timeout synthesizes ``{phase: Failed, message: Failed}`` (:627-632),
- remedy RunsLimit/ResetInterval state machine with the exact RemedyStatus
  strings and counter-zeroing sets (:649-660, :677-721),
- remedy RBAC create → use → delete cycle (:759-786),
- timers stopped on CR deletion (:180-184).
"""
from __future__ import annotations

import asyncio
import logging
import time
from dataclasses import dataclass
from typing import Any, Awaitable, Dict, Optional, Set, Tuple

from .. import API_VERSION
from ..api.runrequest import (
    RUN_HANDLED_ANNOTATION,
    RUN_REQUEST_ANNOTATION,
    RUN_WORKFLOW_ANNOTATION,
    pending_run_request,
)
from ..api.types import HealthCheck, k8s_now, parse_k8s_time
from ..kube.client import EventRecorder, KubeClient
from ..kube.errors import ConflictError, NotFoundError, is_storage_error
from ..kube.registry import WF_API_VERSION, WF_KIND
from ..metrics import (
    MonitorError,
    MonitorFinishedTime,
    MonitorRuntime,
    MonitorStartedTime,
    MonitorSuccess,
    create_dynamic_prometheus_metric,
    forget_healthcheck,
)
from .backoff import IEBTimeoutError, InverseExponentialBackoff, compute_backoff_params
from .cronx import CronParseError, load_zone, seconds_until_next
from .parse import parse_from_healthcheck_async
from .rbac import RBACProvisioner
from .workqueue import WorkQueue

log = logging.getLogger("active_monitor_amd.reconciler")

HC_KIND = "HealthCheck"
SUCC_STR = "Succeeded"
FAIL_STR = "Failed"
REMEDY = "remedy"
HEALTHCHECK = "healthCheck"
TIMER_FLAG = "timer"

#: sentinel returned by an informer-cache lookup that cannot answer (cache
#: not yet synced); distinct from None, which means "synced and not found"
CACHE_MISS = object()


@dataclass
class ReconcileResult:
    requeue_after: float = 0.0
    error: Optional[BaseException] = None


@dataclass
class RepeatTimer:
    """Entry in RepeatTimersByName. Like the reference's expired ``time.Timer``
    values (:746-755), a fired entry stays in the map so the already-scheduled
    dedup check keeps holding during the run it triggered."""

    handle: Optional[asyncio.TimerHandle] = None
    fired: bool = False

    def stop(self) -> None:
        if self.handle is not None:
            self.handle.cancel()


class HealthCheckReconciler:
    def __init__(
        self,
        client: KubeClient,
        recorder: EventRecorder,
        max_parallel: int = 10,
        queue: Optional[WorkQueue] = None,
        cron_time_zone: Optional[str] = None,
    ):
        self.client = client
        self.recorder = recorder
        self.max_parallel = max_parallel
        # NB: not `queue or WorkQueue()` — an empty WorkQueue is falsy (__len__)
        self.queue = queue if queue is not None else WorkQueue()
        self.rbac = RBACProvisioner(client, recorder)
        # zone for cron schedules that carry no TZ=/CRON_TZ= prefix; None (or
        # "Local") reads them on the controller's own clock. A bad name
        # raises CronParseError here, at start-up, not per CR later.
        self.cron_time_zone = cron_time_zone if cron_time_zone != "Local" else None
        self._cron_zone = load_zone(cron_time_zone) if cron_time_zone else None
        # optional WorkflowWatchHub (set by the Manager): event-driven wakeups
        # for workflow completion; None falls back to pure IEB polling
        self.wf_hub = None
        # optional informer-cache lookup (set by the Manager): serves
        # HealthCheck reads from the watch-fed cache like controller-runtime's
        # cached client (healthcheck_controller.go:133 reads through the
        # informer cache, not the wire). Returns a dict, None (synced and
        # absent ⇒ NotFound) or CACHE_MISS (not synced / not covered).
        self.hc_lookup = None
        # read-your-writes floor per key: the rv our last status write
        # produced. A cache entry older than this is our own write's event
        # still in flight — reading it would lose the update (a stale
        # success/failed count rewritten over the real one). Cache reads
        # below the floor fall through to a direct GET. This closes a
        # lost-update race controller-runtime's cached client actually has.
        self._written_rv: Dict[Tuple[str, str], int] = {}
        self.repeat_timers_by_name: Dict[Tuple[str, str], RepeatTimer] = {}
        self._watch_tasks: Dict[str, Set[asyncio.Task]] = {}
        # uid of the object each key's run and timer were started for: a
        # HealthCheck deleted and re-created under its name is another object
        self._driven_uid: Dict[Tuple[str, str], str] = {}
        # name -> namespaces whose check of that name has emitted metrics;
        # the series carry the name alone, so they go with the last of them
        self._metric_namespaces: Dict[str, Set[str]] = {}
        # run requests (api/runrequest.py). A submitted run whose
        # acknowledgement is not written yet: key -> (token, workflow name,
        # uid), so that a failed ack write is retried without resubmitting
        self._run_acks: Dict[Tuple[str, str], Tuple[str, str, str]] = {}
        # keys whose reconcile was put off because a run was in flight; they
        # are queued again when the last watch task of the key is done
        self._rerun_after_watch: Set[Tuple[str, str]] = set()
        # paused (manual-only) checks with an on-demand run in flight
        self._manual_runs: Set[Tuple[str, str]] = set()
        # observability for benchmarks/tests
        self.reconcile_count = 0
        self.completed_runs = 0
        self.on_demand_runs = 0

    # ------------------------------------------------------------------
    # timers
    # ------------------------------------------------------------------

    def get_timer_by_name(self, name: str, namespace: str = "") -> Optional[RepeatTimer]:
        """Timers are keyed (namespace, name) — the reference keys by name
        alone (:139), making same-name CRs in different namespaces fight over
        one timer slot; fixed here with no other visible change. The
        name-only form falls back to any-namespace lookup for API parity."""
        if namespace:
            return self.repeat_timers_by_name.get((namespace, name))
        for (ns, n), entry in self.repeat_timers_by_name.items():
            if n == name:
                return entry
        return None

    def _arm_repeat_timer(self, name: str, namespace: str, delay: float) -> None:
        key = (namespace, name)
        old = self.repeat_timers_by_name.get(key)
        if old is not None:
            old.stop()
        entry = RepeatTimer()
        loop = asyncio.get_running_loop()
        entry.handle = loop.call_later(
            max(0.0, delay), self._on_timer_fired, entry, name, namespace
        )
        self.repeat_timers_by_name[key] = entry

    def _on_timer_fired(self, entry: RepeatTimer, name: str, namespace: str) -> None:
        entry.fired = True
        # repeats flow through the workqueue (bounded by max_parallel); the
        # TIMER flag bypasses only the already-scheduled dedup branch.
        # Synchronous enqueue — no fire-and-forget task to lose.
        self.queue.add_nowait((namespace, name), {TIMER_FLAG})

    def _stop_timer(self, name: str, namespace: str = "") -> bool:
        entry = self.repeat_timers_by_name.pop((namespace, name), None)
        if entry is not None:
            entry.stop()
            return True
        return False

    # ------------------------------------------------------------------
    # watch-task registry
    # ------------------------------------------------------------------

    def _spawn_watch(self, key, coro) -> asyncio.Task:
        task = asyncio.get_running_loop().create_task(coro)
        self._watch_tasks.setdefault(key, set()).add(task)

        def _done(t: asyncio.Task, key=key) -> None:
            tasks = self._watch_tasks.get(key)
            if tasks is not None:
                tasks.discard(t)
                if not tasks:
                    self._watch_tasks.pop(key, None)
            if (self._rerun_after_watch or self._manual_runs) and not self._watch_tasks.get(key):
                self._manual_runs.discard(key)
                if key in self._rerun_after_watch:
                    # a reconcile the in-flight guard put off: only now, with
                    # the task gone from the registry, can it get past it
                    self._rerun_after_watch.discard(key)
                    self.queue.add_nowait(key)
            if not t.cancelled() and t.exception() is not None:
                log.error("watch task for %s failed: %s", key, t.exception())

        task.add_done_callback(_done)
        return task

    def _cancel_watches(self, key) -> None:
        for t in list(self._watch_tasks.get(key, ())):
            t.cancel()

    def forget(self, namespace: str, name: str) -> bool:
        """Stop driving a key: its repeat timer is stopped and its in-flight
        watches are cancelled. True when there was a timer to stop."""
        stopped = self._stop_timer(name, namespace)
        key = (namespace, name)
        self._run_acks.pop(key, None)
        self._rerun_after_watch.discard(key)
        self._manual_runs.discard(key)
        self._cancel_watches(key)
        return stopped

    def active_watches(self) -> int:
        return sum(len(v) for v in self._watch_tasks.values())

    async def drain(self, timeout: float = 30.0) -> None:
        """Await all in-flight watch tasks (test/shutdown helper)."""
        deadline = time.monotonic() + timeout
        while self._watch_tasks and time.monotonic() < deadline:
            tasks = [t for ts in self._watch_tasks.values() for t in ts]
            if not tasks:
                break
            await asyncio.wait(tasks, timeout=min(1.0, deadline - time.monotonic()))

    # ------------------------------------------------------------------
    # events
    # ------------------------------------------------------------------

    async def _event(self, hc: HealthCheck, ev_type: str, message: str) -> None:
        # the recorder only reads object identity — don't serialize the spec
        involved = {
            "apiVersion": API_VERSION,
            "kind": HC_KIND,
            "metadata": {
                "name": hc.metadata.name,
                "namespace": hc.metadata.namespace,
                "uid": hc.metadata.uid,
            },
        }
        await self.recorder.event(involved, ev_type, ev_type, message)

    # ------------------------------------------------------------------
    # Reconcile entry (reference :170-223)
    # ------------------------------------------------------------------

    @staticmethod
    def _rv_of(obj: Optional[Dict[str, Any]]) -> int:
        try:
            return int((obj.get("metadata") or {}).get("resourceVersion", 0))
        except (TypeError, ValueError, AttributeError):
            return -1  # opaque rv: cannot order, treat as unusable floor

    def note_written(self, namespace: str, name: str, obj: Optional[Dict[str, Any]]) -> None:
        """Record the rv a write of ours produced (read-your-writes floor)."""
        rv = self._rv_of(obj)
        if rv > 0:
            key = (namespace, name)
            if rv > self._written_rv.get(key, 0):
                self._written_rv[key] = rv

    async def _get_hc(self, namespace: str, name: str) -> Dict[str, Any]:
        """Read a HealthCheck through the informer cache when one is synced,
        else over the wire. Cache hits return a shallow top-level copy so the
        caller may replace top-level keys (the status-update path does)
        without corrupting the shared cached object. Entries older than our
        own last write (the event is still in flight) are not served — the
        read goes direct instead, so a timer-fired repeat can never observe
        pre-write counters and lose the update."""
        lk = self.hc_lookup
        if lk is not None:
            hit = lk(namespace, name)
            if hit is None:
                self._written_rv.pop((namespace, name), None)
                raise NotFoundError(
                    f'healthchecks.activemonitor.keikoproj.io "{name}" not found'
                )
            if hit is not CACHE_MISS:
                floor = self._written_rv.get((namespace, name), 0)
                if floor == 0 or 0 < floor <= self._rv_of(hit):
                    return dict(hit)
        return await self.client.get(API_VERSION, HC_KIND, namespace, name,
                                     snapshot_read=True)

    async def reconcile(
        self, namespace: str, name: str, flags: Optional[Set[str]] = None
    ) -> ReconcileResult:
        flags = flags or set()
        self.reconcile_count += 1
        try:
            obj = await self._get_hc(namespace, name)
        except NotFoundError:
            await self._deleted(namespace, name)
            return ReconcileResult()
        driven = self._driven_uid.get((namespace, name))
        if driven and driven != ((obj.get("metadata") or {}).get("uid") or driven):
            # deleted and re-created before this key was reconciled in
            # between (the queue holds a key once): what is held belongs to
            # the old object and must not outlive it, nor may its in-flight
            # run pass for a run of the new one
            await self._deleted(namespace, name)
            self._watch_tasks.pop((namespace, name), None)
        hc = HealthCheck.from_dict(obj)
        return await self._process_or_recover(hc, from_timer=TIMER_FLAG in flags)

    async def _deleted(self, namespace: str, name: str) -> None:
        """The CR is gone: stop the repeat timer so self-scheduling halts
        (:180-184) and cancel the in-flight watches proactively (the
        reference lets them die on workflow NotFound after GC) — first, so
        that no late completion can re-create a series — then drop the
        name's metric series once no namespace has a check of that name
        left (the series are labelled by name alone, as in the reference)."""
        stopped = self.forget(namespace, name)
        self._driven_uid.pop((namespace, name), None)
        spaces = self._metric_namespaces.get(name)
        if spaces is not None:
            spaces.discard(namespace)
        if not spaces:
            self._metric_namespaces.pop(name, None)
            forget_healthcheck(name)
        if stopped:
            log.info("cancelled rescheduled workflow for deleted healthcheck %s", name)
            await self.recorder.event(
                {"apiVersion": API_VERSION, "kind": HC_KIND,
                 "metadata": {"name": name, "namespace": namespace}},
                "Normal", "Normal",
                "Cancelling workflow for this healthcheck due to deletion",
            )

    async def _process_or_recover(self, hc: HealthCheck, from_timer: bool) -> ReconcileResult:
        """Panic guard + error policy (reference :190-223). The reference's
        trailing full-object Update (:208-215) is omitted: with the status
        subresource enabled it can persist neither status nor the in-memory
        spec mutations of the fresh object it writes — a pure no-op write per
        reconcile. Status persistence happens where it matters, in the watch
        completion paths (:734,:858) and the pause branch (:246)."""
        try:
            return await self._process_healthcheck(hc, from_timer)
        except asyncio.CancelledError:
            raise
        except Exception as e:  # recover() equivalent — never crash a worker
            if is_storage_error(e):
                return ReconcileResult()
            log.warning("healthcheck %s process error: %s", hc.name, e)
            return ReconcileResult(requeue_after=1.0, error=e)

    # ------------------------------------------------------------------
    # Scheduler (reference :225-291)
    # ------------------------------------------------------------------

    async def _process_healthcheck(self, hc: HealthCheck, from_timer: bool) -> ReconcileResult:
        spec = hc.spec
        if spec.workflow.resource is None:
            return ReconcileResult()
        wf_namespace = spec.workflow.resource.namespace
        key = (hc.namespace, hc.name)
        # the one lookup a check nobody asks to run pays for run requests
        run_token = pending_run_request(hc.metadata) if hc.metadata.annotations else None
        unacked = self._run_acks.get(key) if self._run_acks else None
        if unacked is not None:
            if unacked[0] == run_token and unacked[2] == hc.metadata.uid:
                # the run is submitted and only its acknowledgement failed:
                # repeat the write, not the run
                await self._ack_run_request(key)
                return ReconcileResult()
            del self._run_acks[key]  # withdrawn, replaced, or another object

        finished_unix = 0.0
        t = parse_k8s_time(hc.status.finished_at)
        if t is not None:
            finished_unix = t.timestamp()

        paused = spec.repeat_after_sec <= 0 and spec.schedule.cron == ""
        if paused and run_token is None:
            if key in self._manual_runs:
                # an on-demand run of this paused check is in flight: a
                # Stopped written from what this reconcile read could land
                # after the run's result and take its counts back
                self._rerun_after_watch.add(key)
                return ReconcileResult()
            # pause branch (:238-250) — exact status strings
            hc.status.status = "Stopped"
            hc.status.error_message = (
                "workflow execution is stopped; either spec.RepeatAfterSec or "
                "spec.Schedule must be provided. spec.RepeatAfterSec set to "
                f"{spec.repeat_after_sec}. spec.Schedule set to {spec.schedule.go_string()}"
            )
            hc.status.finished_at = k8s_now()
            await self._event(
                hc,
                "Warning",
                "Workflow execution is stopped; either spec.RepeatAfterSec or "
                "spec.Schedule must be provided",
            )
            await self.update_healthcheck_status(hc)
            return ReconcileResult()
        if self._watch_tasks.get(key) and (
            not from_timer or key not in self.repeat_timers_by_name
        ):
            # a run for this CR is already in flight: spurious reconciles
            # (informer list/watch overlap at startup, spec edits mid-run)
            # must not submit a duplicate workflow. The reference double-
            # submits here and parks a second blocked goroutine per duplicate
            # (SURVEY.md §2.3.1); the clean rebuild closes that hole. A timer
            # tick whose timer is gone is the tick an on-demand run replaced.
            if run_token is not None:
                # the run in flight started before the request and does not
                # serve it: the request is served when that run is done
                self._rerun_after_watch.add(key)
            return ReconcileResult()
        if spec.repeat_after_sec <= 0 and not paused:
            # cron branch (:251-263): +1s compensates integer truncation
            try:
                spec.repeat_after_sec = seconds_until_next(
                    spec.schedule.cron, default_zone=self._cron_zone
                )
            except CronParseError as e:
                log.warning("healthcheck %s: fail to parse cron %r: %s",
                            hc.name, spec.schedule.cron, e)
                await self._event(hc, "Warning", "Fail to parse cron")
                raise
        # already executed recently and a repeat is scheduled (:264-267). The
        # reference's elif chain exempts cron CRs from this dedup, so every
        # status write re-submits them in a tight loop until the blocking
        # watch throttles it; here it applies to them too, with the freshly
        # computed interval
        if (
            not from_timer
            and run_token is None
            and int(time.time() - finished_unix) < spec.repeat_after_sec
            and self.get_timer_by_name(hc.name, hc.namespace) is not None
        ):
            return ReconcileResult()

        if run_token is not None:
            # never two runs at once: the run that serves the request takes
            # the place of the pending tick, and its completion arms the
            # timer again by the usual rule
            self._stop_timer(hc.name, hc.namespace)
            self.on_demand_runs += 1
            await self._event(hc, "Normal", "Workflow run requested on demand")

        try:
            await self.rbac.create_rbac_for_workflow(hc, HEALTHCHECK)
        except Exception:
            await self._event(hc, "Warning", "Error creating RBAC for HealthCheckWorkflow")
            raise

        generated_name = await self.create_submit_workflow(hc, run_token)
        self._driven_uid[key] = hc.metadata.uid
        if run_token is not None and paused:
            self._manual_runs.add(key)
        # non-blocking watch: the reconcile worker is freed immediately
        self._spawn_watch(
            key,
            self.watch_workflow_reschedule(
                wf_namespace, generated_name, hc, on_demand=run_token is not None
            ),
        )
        if run_token is not None:
            self._run_acks[key] = (run_token, generated_name, hc.metadata.uid)
            await self._ack_run_request(key)
        return ReconcileResult()

    async def _ack_run_request(self, key: Tuple[str, str]) -> None:
        """Write ``run-handled`` and ``run-workflow`` for the run remembered
        in ``_run_acks``, in one merge patch. An error leaves the memory in
        place and propagates: the reconcile is requeued and repeats only
        this write. The guarantee is at-least-once: a controller that dies
        between the submit and this write serves the request again."""
        token, wf_name, uid = self._run_acks[key]
        namespace, name = key
        try:
            out = await self.client.patch(
                API_VERSION, HC_KIND, namespace, name,
                {"metadata": {"annotations": {
                    RUN_HANDLED_ANNOTATION: token,
                    RUN_WORKFLOW_ANNOTATION: wf_name,
                }}},
            )
        except NotFoundError:
            self._run_acks.pop(key, None)  # deleted meanwhile: nothing to tell
            return
        self._run_acks.pop(key, None)
        if not uid or ((out.get("metadata") or {}).get("uid") or uid) == uid:
            # read-your-writes: a cached read from before this write would
            # show the request as still pending
            self.note_written(namespace, name, out)

    # ------------------------------------------------------------------
    # Submit (reference :502-571)
    # ------------------------------------------------------------------

    def _owner_reference(self, hc: HealthCheck) -> Dict[str, Any]:
        return {
            "kind": HC_KIND,
            "apiVersion": API_VERSION,
            "name": hc.name,
            "uid": hc.metadata.uid,
            "controller": True,
        }

    #: (parse/submit error, parsed, created) event texts; the remedy's
    #: spellings are the reference's (:515-568)
    _SUBMIT_EVENTS = (
        "Error creating or submitting workflow",
        "workflow is parsed from healthcheck",
        "Successfully created workflow",
    )
    _REMEDY_SUBMIT_EVENTS = (
        "Error creating or submitting remedyworkflow",
        "Remedy workflow is parsed from healthcheck",
        "Successfully created remedyWorkflow",
    )

    async def _create_submit(self, hc: HealthCheck, remedy: bool,
                             run_token: Optional[str] = None) -> str:
        """Parse ``spec.workflow`` (or ``spec.remedyworkflow``) and create the
        Workflow; returns its generated name. ``run_token`` marks the check
        Workflow that serves a run request."""
        wf_spec = hc.spec.remedy_workflow if remedy else hc.spec.workflow
        if remedy and wf_spec.resource is None:
            raise ValueError("RemedyWorkflow Resource is nil")
        failed, parsed, created_ok = (
            self._REMEDY_SUBMIT_EVENTS if remedy else self._SUBMIT_EVENTS
        )
        try:
            spec, labels = await parse_from_healthcheck_async(hc, remedy)
        except Exception:
            await self._event(hc, "Warning", failed)
            raise
        await self._event(hc, "Normal", parsed)
        wf = {
            "apiVersion": WF_API_VERSION,
            "kind": WF_KIND,
            "metadata": {
                "generateName": wf_spec.generate_name,
                "namespace": wf_spec.resource.namespace,
                "labels": labels,
                "ownerReferences": [self._owner_reference(hc)],
            },
            "spec": spec,
        }
        if run_token is not None:
            wf["metadata"]["annotations"] = {RUN_REQUEST_ANNOTATION: run_token}
        created = await self.client.create(wf, transfer=True)
        await self._event(hc, "Normal", created_ok)
        return created["metadata"]["name"]

    def create_submit_workflow(
        self, hc: HealthCheck, run_token: Optional[str] = None
    ) -> Awaitable[str]:
        return self._create_submit(hc, remedy=False, run_token=run_token)

    def create_submit_remedy_workflow(self, hc: HealthCheck) -> Awaitable[str]:
        return self._create_submit(hc, remedy=True)

    # ------------------------------------------------------------------
    # Watch (reference :607-757 health check, :788-874 remedy)
    # ------------------------------------------------------------------

    _POLL_RETRIES = 3

    async def _poll_workflow(
        self, namespace: str, name: str, via_cache: bool = False
    ) -> Optional[Dict[str, Any]]:
        """One status poll. NotFound propagates (ends the watch, :618-622);
        transient apiserver errors are retried briefly and then treated as a
        missed poll — the reference aborts the whole watch on any error,
        stalling the CR until an external reconcile.

        ``via_cache=True`` reads from the watch hub's last-event cache (the
        watch payload already carried the full Workflow) instead of a GET
        round-trip — the informer-cache read discipline of controller-runtime.
        A cache miss means no event reached the hub yet, i.e. the freshly
        submitted workflow has no status — reported as such without touching
        the wire. The IEB fallback polls (hub wait timed out) always go
        direct, so a lost watch event costs one poll interval, never
        correctness."""
        if via_cache and self.wf_hub is not None:
            hit = self.wf_hub.cached(namespace, name)
            if hit is not None:
                ev_type, obj = hit
                if ev_type == "DELETED":
                    raise NotFoundError(f'workflow "{name}" not found (deleted)')
                status = obj.get("status")
                return status if isinstance(status, dict) else None
            return None
        last: Optional[BaseException] = None
        for attempt in range(self._POLL_RETRIES):
            try:
                wf = await self.client.get(WF_API_VERSION, WF_KIND, namespace, name,
                                           snapshot_read=True)
                status = wf.get("status")
                return status if isinstance(status, dict) else None
            except NotFoundError:
                raise
            except asyncio.CancelledError:
                raise
            except Exception as e:
                last = e
                await asyncio.sleep(0.05 * (attempt + 1))
        log.warning("workflow poll %s/%s failed transiently: %s", namespace, name, last)
        return None  # missed poll; the IEB deadline still bounds the watch

    async def _wait_next_poll(
        self, ieb: InverseExponentialBackoff, namespace: str, name: str, since: Optional[int]
    ) -> bool:
        """Wait until the next poll is due. With a watch hub the wait ends the
        moment the workflow changes (ms-scale completion detection); without
        one this is exactly the reference's IEB sleep. Raises IEBTimeoutError
        past the deadline either way — the synthesized-failure semantics are
        identical. Returns True when a watch event (not a timeout) ended the
        wait, i.e. the hub cache holds the fresh object and the next poll may
        read it without a wire round-trip."""
        if self.wf_hub is None:
            await ieb.next()
            return False
        ieb.check_deadline()
        interval = ieb.peek_interval()
        ieb.decay()
        changed = await self.wf_hub.wait_change(namespace, name, interval, since=since)
        ieb.check_deadline()
        return changed is not None

    async def _watch_until_terminal(
        self, hc: HealthCheck, wf_namespace: str, wf_name: str,
        backoff: Tuple[float, float, float, float], timeout_event: str,
    ) -> Optional[Dict[str, Any]]:
        """Poll a workflow until it is Succeeded or Failed and return its
        status, or None once it no longer exists (:618-622). ``backoff`` is
        ``(max, min, timeout, factor)`` in seconds; past the timeout the
        status is synthesized as ``{phase: Failed, message: Failed}`` and
        ``timeout_event`` is emitted (:627-632)."""
        ieb: Optional[InverseExponentialBackoff] = None
        timed_out = False
        try:
            ieb = InverseExponentialBackoff(*backoff)
        except ValueError:
            # invalid params (e.g. timeout 0): the reference's loop sees a
            # constructor error on its first iteration and synthesizes Failed
            timed_out = True

        # the first poll may read the hub cache (a just-submitted workflow has
        # no status until an event lands); timed-out waits force direct polls
        via_cache = self.wf_hub is not None
        while True:
            # pre-poll change counter: any event landing between this poll and
            # the wait below is detected immediately (no lost wakeups)
            seq = self.wf_hub.seq(wf_namespace, wf_name) if self.wf_hub else None
            try:
                status = await self._poll_workflow(wf_namespace, wf_name,
                                                   via_cache=via_cache)
            except NotFoundError:
                status = None
                break
            if timed_out:
                status = {"phase": FAIL_STR, "message": FAIL_STR}
                await self._event(hc, "Warning", timeout_event)
                break
            if status is not None and status.get("phase") in (SUCC_STR, FAIL_STR):
                break
            # not terminal yet: wait for the next poll (hub-accelerated)
            try:
                via_cache = await self._wait_next_poll(ieb, wf_namespace, wf_name, seq)
            except IEBTimeoutError:
                timed_out = True
        # this watch is done with the workflow forever (names are unique):
        # release its hub cache/seq entry now rather than waiting for the
        # server-side TTL delete (RSS leak at fleet rates otherwise)
        if self.wf_hub is not None:
            self.wf_hub.forget(wf_namespace, wf_name)
        return status

    async def watch_workflow_reschedule(
        self, wf_namespace: str, wf_name: str, hc: HealthCheck,
        on_demand: bool = False,
    ) -> None:
        then = k8s_now()
        then_unix = time.time()
        repeat_after_sec = hc.spec.repeat_after_sec
        max_t, min_t, factor, timeout = compute_backoff_params(
            hc.spec.backoff_max, hc.spec.backoff_min, hc.spec.backoff_factor,
            hc.spec.workflow.timeout,
        )
        status = await self._watch_until_terminal(
            hc, wf_namespace, wf_name, (max_t, min_t, timeout, factor),
            "Workflow timed out",
        )
        if status is None:
            # parent healthcheck likely deleted; don't reschedule (:618-622)
            await self._event(
                hc,
                "Warning",
                "Error attempting to find workflow for healthcheck. This may "
                "indicate that either the healthcheck was removed or the Workflow "
                "was GC'd before active-monitor could obtain the status",
            )
            if on_demand and repeat_after_sec > 0:
                # the run took the pending tick's place (its timer was
                # stopped): without a result to re-arm from, the schedule
                # is put back here, so the check is never left unscheduled
                fresh = await self._get_live_hc(hc)
                if fresh is not None:
                    self._arm_repeat_timer(
                        hc.name, hc.namespace,
                        self._next_delay(fresh, repeat_after_sec))
            return
        await self._apply_check_result(hc, wf_name, status, then, then_unix)
        try:
            await self._finish_and_reschedule(hc, repeat_after_sec)
        finally:
            self.completed_runs += 1

    async def watch_remedy_workflow(
        self, wf_namespace: str, wf_name: str, hc: HealthCheck
    ) -> None:
        """Remedy watch (reference :788-874): backoff params derive from the
        *health-check* workflow's timeout with factor fixed at 0.5 (:791-801),
        a reference quirk kept for behavioral parity. A vanished remedy
        workflow ends the watch silently."""
        then = k8s_now()
        then_unix = time.time()
        max_t, min_t, _factor, timeout = compute_backoff_params(
            0, 0, "", hc.spec.workflow.timeout
        )
        status = await self._watch_until_terminal(
            hc, wf_namespace, wf_name, (max_t, min_t, timeout, 0.5),
            "remedy workflow is timedout",
        )
        if status is None:
            return
        await self._apply_remedy_result(hc, wf_name, status, then, then_unix)
        # persist remedy status promptly (reference :856-871); the check's
        # own write follows when its watch finishes
        fresh = await self._get_live_hc(hc)
        if fresh is not None:
            await self.update_healthcheck_status(hc, fresh=fresh)

    # ------------------------------------------------------------------
    # Status + metric mutations for a terminal workflow: check, then remedy
    # ------------------------------------------------------------------

    def _note_metrics(self, hc: HealthCheck) -> None:
        spaces = self._metric_namespaces.get(hc.name)
        if spaces is None:
            spaces = self._metric_namespaces[hc.name] = set()
        spaces.add(hc.namespace)

    async def _apply_check_result(
        self, hc: HealthCheck, wf_name: str, status: Dict[str, Any],
        then: str, then_unix: float,
    ) -> None:
        """Reference :634-727. Only the check registers custom metrics,
        resets the remedy on a pass and triggers it on a failure."""
        st = hc.status
        now = k8s_now()
        now_unix = time.time()
        self._note_metrics(hc)
        if status.get("phase") == SUCC_STR:
            await self._event(hc, "Normal", "Workflow status is Succeeded")
            st.status = SUCC_STR
            st.started_at = then
            st.finished_at = now
            st.success_count += 1
            st.total_healthcheck_runs = st.success_count + st.failed_count
            st.last_successful_workflow = wf_name
            MonitorSuccess.labels(hc.name, HEALTHCHECK).inc()
            MonitorRuntime.labels(hc.name, HEALTHCHECK).set(now_unix - then_unix)
            MonitorStartedTime.labels(hc.name, HEALTHCHECK).set(int(then_unix))
            MonitorFinishedTime.labels(hc.name, HEALTHCHECK).set(int(now_unix))
            # custom metrics from workflow output parameters — the
            # reference documents this (README.md:275-285) but never
            # wires it; here the documented feature is real.
            create_dynamic_prometheus_metric(hc.name, status)
            if not hc.spec.remedy_workflow.is_empty() and st.remedy_total_runs >= 1:
                st.reset_remedy()
                st.remedy_status = "HealthCheck Passed so Remedy is reset"
                await self._event(hc, "Normal", "HealthCheck passed so Remedy is reset")
        else:
            await self._event(hc, "Warning", "Workflow status is Failed")
            st.status = FAIL_STR
            st.started_at = then
            st.finished_at = now
            st.last_failed_at = now
            msg = status.get("message")
            st.error_message = msg if isinstance(msg, str) else ""
            st.failed_count += 1
            st.total_healthcheck_runs = st.success_count + st.failed_count
            st.last_failed_workflow = wf_name
            MonitorError.labels(hc.name, HEALTHCHECK).inc()
            MonitorStartedTime.labels(hc.name, HEALTHCHECK).set(int(then_unix))
            MonitorFinishedTime.labels(hc.name, HEALTHCHECK).set(int(now_unix))
            try:
                await self._maybe_run_remedy(hc, now_unix)
            except asyncio.CancelledError:
                raise
            except Exception as e:
                # a remedy failure must not lose the health-check
                # status or the repeat schedule (the reference aborts
                # the whole watch here, stalling the CR — :686-688)
                log.warning("remedy for %s failed: %s", hc.name, e)
                await self._event(hc, "Warning", "Error executing RemedyWorkflow")

    async def _apply_remedy_result(
        self, hc: HealthCheck, wf_name: str, status: Dict[str, Any],
        then: str, then_unix: float,
    ) -> None:
        """Reference :819-855. The remedy_* twins of the check's fields —
        except the two reference quirks marked below."""
        st = hc.status
        now = k8s_now()
        now_unix = time.time()
        self._note_metrics(hc)
        if status.get("phase") == SUCC_STR:
            await self._event(hc, "Normal", "Remedy workflow status is Succeeded")
            st.remedy_status = SUCC_STR
            st.remedy_started_at = then
            st.remedy_finished_at = now
            st.remedy_success_count += 1
            st.remedy_total_runs = st.remedy_success_count + st.remedy_failed_count
            # reference quirk kept: remedy watch writes the shared
            # last*Workflow fields with the remedy name (:830)
            st.last_successful_workflow = wf_name
            MonitorSuccess.labels(hc.name, REMEDY).inc()
            MonitorRuntime.labels(hc.name, REMEDY).set(now_unix - then_unix)
            MonitorStartedTime.labels(hc.name, REMEDY).set(int(then_unix))
            # reference quirk kept: finished-time gauge carries the
            # HEALTH-CHECK finish epoch, not the remedy's (:834)
            hc_fin = parse_k8s_time(st.finished_at)
            MonitorFinishedTime.labels(hc.name, REMEDY).set(
                int(hc_fin.timestamp()) if hc_fin else int(now_unix)
            )
        else:
            await self._event(hc, "Warning", "remedy workflow status is failed")
            st.remedy_status = FAIL_STR
            st.remedy_started_at = then
            st.remedy_finished_at = now
            st.remedy_last_failed_at = now
            msg = status.get("message")
            st.remedy_error_message = msg if isinstance(msg, str) else ""
            st.remedy_failed_count += 1
            st.remedy_total_runs = st.remedy_success_count + st.remedy_failed_count
            st.last_failed_workflow = wf_name
            MonitorError.labels(hc.name, REMEDY).inc()
            MonitorStartedTime.labels(hc.name, REMEDY).set(int(then_unix))
            MonitorFinishedTime.labels(hc.name, REMEDY).set(int(now_unix))

    async def _finish_and_reschedule(self, hc: HealthCheck, repeat_after_sec: float) -> None:
        """Persist status and re-arm the repeat timer (reference :729-757).

        The timer is armed BEFORE the status write so the MODIFIED event the
        write triggers always observes an armed timer in the dedup branch —
        closing a duplicate-submission race the reference leaves open by
        updating first (:734) and arming after (:746)."""
        fresh = await self._get_live_hc(hc)
        if fresh is None:
            return
        repeat_after_sec = self._next_delay(fresh, repeat_after_sec)
        # <= 0: the on-demand run of a paused (manual-only) check, which has
        # no next run to arm — not even a zero-delay one
        armed = repeat_after_sec > 0
        if armed:
            self._arm_repeat_timer(hc.name, hc.namespace, repeat_after_sec)
        try:
            await self.update_healthcheck_status(hc, fresh=fresh)
        except NotFoundError:
            self._stop_timer(hc.name, hc.namespace)
            return
        except Exception:
            await self._event(hc, "Warning", "Error updating healthcheck resource")
            self._stop_timer(hc.name, hc.namespace)
            raise
        if armed:
            await self._event(hc, "Normal", "Rescheduled workflow for next run")

    def _next_delay(self, fresh: Dict[str, Any], repeat_after_sec: float) -> float:
        """Cron CRs: recompute the delay at completion time so the next run
        lands on the cron tick, not submit-time + interval (the reference
        re-arms with the stale submit-time value, drifting by the run's
        duration — :746-752)."""
        fresh_spec = fresh.get("spec") or {}
        cron = ((fresh_spec.get("schedule") or {}).get("cron")) or ""
        if int(fresh_spec.get("repeatAfterSec", 0) or 0) <= 0 and cron:
            try:
                return seconds_until_next(cron, default_zone=self._cron_zone)
            except CronParseError:
                pass  # keep the submit-time value
        return repeat_after_sec

    # ------------------------------------------------------------------
    # Remedy (reference :677-721, :759-786)
    # ------------------------------------------------------------------

    async def _maybe_run_remedy(self, hc: HealthCheck, now_unix: float) -> None:
        """The remedy trigger state machine (reference :677-721)."""
        if hc.spec.remedy_workflow.is_empty():
            return
        limit = hc.spec.remedy_runs_limit
        reset_interval = hc.spec.remedy_reset_interval
        if limit != 0 and reset_interval != 0:
            if limit > hc.status.remedy_total_runs:
                await self.process_remedy_workflow(hc)
            else:
                rf = parse_k8s_time(hc.status.remedy_finished_at)
                since_last = int(now_unix - rf.timestamp()) if rf is not None else reset_interval + 1
                if reset_interval >= since_last:
                    log.info(
                        "skipping remedy for %s: remedy limit met, will run after reset interval",
                        hc.name,
                    )
                else:
                    hc.status.reset_remedy()
                    hc.status.remedy_status = "RemedyResetInterval elapsed so Remedy is reset"
                    await self._event(
                        hc, "Normal", "RemedyResetInterval elapsed so Remedy is reset"
                    )
                    await self.process_remedy_workflow(hc)
        else:
            await self.process_remedy_workflow(hc)

    async def process_remedy_workflow(self, hc: HealthCheck) -> None:
        """create remedy RBAC → submit → watch → delete remedy RBAC
        (reference :759-786)."""
        await self.rbac.create_rbac_for_workflow(hc, REMEDY)
        generated_name = await self.create_submit_remedy_workflow(hc)
        # watch in the remedy's own namespace — the reference watches in the
        # health-check workflow's namespace (:773), which mis-targets when the
        # two differ; fixed here with no CR-visible change for the common case
        remedy_ns = hc.spec.remedy_workflow.resource.namespace
        await self.watch_remedy_workflow(remedy_ns, generated_name, hc)
        await self.rbac.delete_rbac_for_workflow(hc)

    # ------------------------------------------------------------------
    # Status persistence (reference :1445-1462)
    # ------------------------------------------------------------------

    async def _get_live_hc(self, hc: HealthCheck) -> Optional[Dict[str, Any]]:
        """Fresh read for a status write; None when the CR is gone, being
        deleted, or another object of the same name (deleted and re-created
        while the run was in flight), in which case nothing is written."""
        try:
            fresh = await self._get_hc(hc.namespace, hc.name)
        except NotFoundError:
            return None
        meta = fresh.get("metadata") or {}
        if meta.get("deletionTimestamp"):
            return None
        if hc.metadata.uid and meta.get("uid") and meta["uid"] != hc.metadata.uid:
            return None
        return fresh

    async def update_healthcheck_status(
        self, hc: HealthCheck, retries: int = 5,
        fresh: Optional[Dict[str, Any]] = None,
    ) -> None:
        """Fresh Get + status-subresource update with conflict retry.
        ``fresh`` lets callers that just read the object donate that read for
        the first attempt (one round-trip saved per completed run)."""
        last: Optional[BaseException] = None
        for attempt in range(retries):
            if fresh is None:
                fresh = await self.client.get(API_VERSION, HC_KIND, hc.namespace,
                                              hc.name, snapshot_read=True)
            fresh["status"] = hc.status.to_dict()
            try:
                out = await self.client.update_status(fresh)
                # read-your-writes: later cache reads must be ≥ this version
                self.note_written(hc.namespace, hc.name, out)
                return
            except ConflictError as e:
                last = e
                fresh = None  # stale: re-read on the next attempt
                await asyncio.sleep(0.01 * (attempt + 1))
        raise last if last else RuntimeError("status update failed")

    # ------------------------------------------------------------------
    # Shutdown
    # ------------------------------------------------------------------

    def stop_all(self) -> None:
        for (ns, name) in list(self.repeat_timers_by_name):
            self._stop_timer(name, ns)
        for key in list(self._watch_tasks):
            self._cancel_watches(key)

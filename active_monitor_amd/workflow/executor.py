"""One local run of an Argo-shaped workflow.

:class:`WorkflowRun` walks the template tree of a validated spec, runs leaf
templates as local subprocesses and records a node per step, Argo-style.
:class:`~.engines.LocalWorkflowEngine` owns the Workflow object and its status
writes; everything between the two writes happens here.
"""
from __future__ import annotations

import asyncio
import collections
import logging
import os
import shutil
import signal
import tempfile
import time
from typing import Any, Awaitable, Dict, List, Optional, Tuple

from ..api.types import k8s_now
from .expr import ExprError
from .expr import parse as parse_expr
from .expr import render as render_expr
from .template import (
    TemplateError,
    UnresolvedReference,
    active_deadline,
    eval_when,
    expand_sequence,
    item_display_name,
    item_scope,
    parse_duration,
    parse_with_param,
    step_timeout,
    substitute,
    substitute_list,
    to_str,
)
from .templates import OWN_SCOPE, scope_key, shown_ref
from .validate import HTTP_DEFAULT_TIMEOUT_SECONDS, task_dependencies

#: ``outputs.result`` keeps at most this many bytes of a leaf's stdout
RESULT_MAX_BYTES = 64 * 1024
#: a failed leaf's message ends with this many characters of its output
MESSAGE_TAIL_CHARS = 500
#: bytes of each stream's end kept for that message: a character is at most
#: four bytes, and a decoder that starts inside one is back in step within
#: three more, so the last MESSAGE_TAIL_CHARS characters of the kept bytes
#: are those of the whole stream
_TAIL_BYTES = 4 * MESSAGE_TAIL_CHARS + 8
#: one read of a leaf's pipe takes at most this much
_PIPE_CHUNK = 64 * 1024
#: after its group was killed a leaf's pipes reach EOF at once, unless a
#: process that left the group still holds them; it is not waited for longer
_KILL_DRAIN_SECONDS = 1.0
#: a killed member of the group that was not the leaf's own child (its parent
#: exited first) is reaped by whoever adopted it, init as a rule, and stays
#: in the process table until then; the kill path waits this long for the
#: group to be empty, so that a workflow reported Failed has left nothing
_KILL_REAP_SECONDS = 5.0
#: a leaf attempt that outran its template's ``activeDeadlineSeconds``
#: (Argo's wording for the pod it would have been, from memory)
POD_DEADLINE_MESSAGE = "Pod was active on the node longer than the specified deadline"
#: a node that outran its template's ``timeout``, retries and waits included
STEP_DEADLINE_MESSAGE = "Step exceeded its deadline"
#: HTTP probes in flight at once, over all runs of an engine
HTTP_MAX_IN_FLIGHT = 64

log = logging.getLogger("active_monitor_amd.workflow")

Scope = Dict[str, str]
Outputs = Dict[str, Any]  # {"result": str, "parameters": {name: value}}
#: (phase, message, outputs); outputs is None for skipped / fanned-out calls
Result = Tuple[str, str, Optional[Outputs]]
#: the template a call names: (scope, template name, the ``templateRef`` its
#: node shows or None for a ``template:`` call); scopes as in :mod:`.templates`
Target = Tuple[str, Any, Optional[Dict[str, Any]]]


class Bound:
    """At most ``limit`` holders at a time, served in arrival order; None
    bounds nothing. ``held`` counts the holders either way. A waiter that is
    cancelled gives up its place, or the slot it was just handed.

    ``fail_fast`` is set by a DAG that fails fast: its first child to fail
    sets ``closed`` before it hands its slot on, and a child that gets a
    slot afterwards does not start."""

    __slots__ = ("limit", "held", "fail_fast", "closed", "_waiters")

    def __init__(self, limit: Optional[int] = None):
        self.limit = limit
        self.held = 0
        self.fail_fast = False
        self.closed = False
        self._waiters: "collections.deque[asyncio.Future[None]]" = collections.deque()

    async def acquire(self) -> None:
        if self.limit is None or (self.held < self.limit and not self._waiters):
            self.held += 1
            return
        fut: "asyncio.Future[None]" = asyncio.get_running_loop().create_future()
        self._waiters.append(fut)
        try:
            await fut
        except asyncio.CancelledError:
            if fut.cancelled():
                try:
                    self._waiters.remove(fut)
                except ValueError:
                    pass  # release() passed it over already
            else:
                self.release()  # handed over as the cancellation arrived
            raise

    def release(self) -> None:
        self.held -= 1
        while self._waiters and self.held < self.limit:
            fut = self._waiters.popleft()
            if not fut.done():
                self.held += 1
                fut.set_result(None)


def _continues(call: Dict[str, Any]) -> bool:
    """Whether the caller of a step or task goes on when it failed. Only
    ``continueOn.failed`` counts: no node here ever ends in ``Error``."""
    on = call.get("continueOn")
    return isinstance(on, dict) and on.get("failed") is True


def _parallelism_bound(tmpl: Dict[str, Any]) -> Optional[Bound]:
    """A new bound for a spec, or for one invocation of a ``steps`` or
    ``dag`` template, that sets ``parallelism``; None when it does not."""
    limit = tmpl.get("parallelism")
    return Bound(limit) if limit is not None else None


class WorkflowRun:
    def __init__(self, spec: Dict[str, Any], name: str, namespace: str,
                 logs: Any = None, process_slots: Optional[Bound] = None,
                 templates: Optional[Dict[str, Dict[Any, Dict[str, Any]]]] = None,
                 http_slots: Optional[Bound] = None):
        """``spec`` is the effective spec; ``templates`` the shared templates
        it reaches, by scope (:attr:`.templates.Resolved.scopes`)."""
        self.spec = spec
        #: an HTTP probe holds one slot of this, the engine's bound over the
        #: probes of all runs, and none of ``_process_bounds``: it is no process
        self._http_slots = http_slots
        # a leaf process holds one slot of each, taken in this order:
        # spec.parallelism, then the engine's bound over all of its runs
        self._process_bounds = [
            b for b in (_parallelism_bound(spec), process_slots) if b is not None
        ]
        self.name = name
        self.namespace = namespace
        #: a :class:`~.logs.LogStore`, or None: leaf output is then drained
        #: and dropped
        self.logs = logs
        self.templates = {t.get("name"): t for t in spec.get("templates") or []}
        self._scopes = {**(templates or {}), OWN_SCOPE: self.templates}
        self.nodes: Dict[str, Dict[str, Any]] = {}
        self.global_outputs: List[Dict[str, str]] = []
        self._procs: Dict[int, asyncio.subprocess.Process] = {}
        self.base_scope: Scope = {"workflow.name": name, "workflow.namespace": namespace}
        self.arguments: Dict[str, str] = {}
        for p in (spec.get("arguments") or {}).get("parameters") or []:
            if isinstance(p, dict) and p.get("name") is not None and p.get("value") is not None:
                self.arguments[str(p["name"])] = to_str(p["value"])
                self.base_scope[f"workflow.parameters.{p['name']}"] = to_str(p["value"])

    # -- entry points -----------------------------------------------------

    async def run_entrypoint(self) -> Tuple[str, str]:
        return await self._run_root(self.spec.get("entrypoint"), self.name, self.base_scope)

    async def run_exit_handler(self, status: str) -> Tuple[str, str]:
        scope = dict(self.base_scope)
        scope["workflow.status"] = status
        return await self._run_root(self.spec["onExit"], f"{self.name}.onExit", scope)

    async def _run_root(self, template: str, node_id: str, scope: Scope) -> Tuple[str, str]:
        phase, message, _ = await self._run_template(
            (OWN_SCOPE, template, None), self.arguments, node_id, node_id, None, scope
        )
        return phase, message

    def terminate(self, reason: str) -> None:
        """After a cancellation: kill whatever is still alive and close the
        nodes that were cut short."""
        for proc in list(self._procs.values()):
            _kill_group(proc)
        now = k8s_now()
        for node in self.nodes.values():
            if "phase" not in node:
                node.update(phase="Failed", message=reason, finishedAt=now)

    # -- nodes ------------------------------------------------------------

    @staticmethod
    def _target(call: Dict[str, Any], tscope: str) -> Target:
        """What a step or task of a template of scope ``tscope`` names."""
        ref = call.get("templateRef")
        if isinstance(ref, dict):
            return (scope_key(ref.get("clusterScope") is True, ref.get("name")),
                    ref.get("template"), shown_ref(ref))
        return tscope, call.get("template"), None

    def _open(self, node_id: str, display: str, type_: str, target: Optional[Target],
              parent: Optional[str]) -> Dict[str, Any]:
        node: Dict[str, Any] = {
            "id": node_id, "displayName": display, "type": type_,
            "startedAt": k8s_now(), "children": [],
        }
        if target is not None:
            tscope, template, ref = target
            if ref is not None:
                node["templateRef"] = ref
            elif template is not None:
                node["templateName"] = template
            if tscope:
                node["templateScope"] = tscope
        self.nodes[node_id] = node
        if parent is not None and parent in self.nodes:
            self.nodes[parent]["children"].append(node_id)
        return node

    @staticmethod
    def _close(node: Dict[str, Any], phase: str, message: str = "",
               outputs: Optional[Outputs] = None) -> None:
        node["phase"] = phase
        node["message"] = message
        node["finishedAt"] = k8s_now()
        if outputs:
            shown: Dict[str, Any] = {}
            if outputs.get("result") is not None:
                shown["result"] = outputs["result"]
            if outputs.get("parameters"):
                shown["parameters"] = [
                    {"name": k, "value": v} for k, v in outputs["parameters"].items()
                ]
            if shown:
                node["outputs"] = shown

    def _mark(self, node_id: str, display: str, target: Optional[Target],
              parent: Optional[str], phase: str, message: str) -> None:
        """A node that never ran: ``Skipped`` (false ``when``) or ``Omitted``."""
        self._close(self._open(node_id, display, "Skipped", target, parent), phase, message)

    # -- templates --------------------------------------------------------

    def _inputs(self, tmpl: Dict[str, Any], args: Dict[str, str], scope: Scope) -> Scope:
        """Template scope: workflow-level variables plus ``inputs.parameters``
        (caller's argument, else ``value``, else ``default``)."""
        out = {k: v for k, v in scope.items() if k.startswith("workflow.")}
        for p in (tmpl.get("inputs") or {}).get("parameters") or []:
            if not isinstance(p, dict) or p.get("name") is None:
                continue
            name = str(p["name"])
            if name in args:
                value = args[name]
            elif p.get("value") is not None:
                value = substitute(to_str(p["value"]), out)
            elif p.get("default") is not None:
                value = substitute(to_str(p["default"]), out)
            else:
                raise TemplateError(
                    f"inputs.parameters.{name} was not supplied and has no default"
                )
            out[f"inputs.parameters.{name}"] = value
        return out

    async def _run_template(self, target: Target, args: Dict[str, str], node_id: str,
                            display: str, parent: Optional[str], wf_scope: Scope) -> Result:
        tmpl = (self._scopes.get(target[0]) or {}).get(target[1]) or {}
        if not tmpl.get("timeout"):  # none, 0 or "": nothing is put around it
            return await self._run_attempts(tmpl, target, args, node_id, display, parent,
                                            wf_scope)
        try:
            written = tmpl["timeout"]
            budget = step_timeout(written, self._inputs(tmpl, args, wf_scope)
                                  if isinstance(written, str) and "{{" in written else {})
        except TemplateError as e:
            message = f"invalid timeout: {e}"
            self._mark(node_id, display, target, parent, "Failed", message)
            return "Failed", message, None
        attempts = self._run_attempts(tmpl, target, args, node_id, display, parent, wf_scope)
        if budget is None:
            return await attempts
        try:
            # the node as a whole: waits for a slot, every attempt and every
            # backoff wait. On expiry the running attempt is cancelled and
            # awaited, so its group is killed and reaped, its slots, directory
            # and log writer are given back, before the node is reported
            return await asyncio.wait_for(attempts, budget)
        except asyncio.TimeoutError:
            if node_id in self.nodes:
                self._cut(node_id, STEP_DEADLINE_MESSAGE)
            else:  # over before the first attempt could open it
                self._mark(node_id, display, target, parent, "Failed", STEP_DEADLINE_MESSAGE)
            return "Failed", STEP_DEADLINE_MESSAGE, None

    def _cut(self, node_id: str, message: str) -> None:
        """Close ``node_id`` and what is still open below it as ``Failed``."""
        node = self.nodes.get(node_id)
        if node is None:
            return
        for child in node["children"]:
            self._cut(child, message)
        if "phase" not in node:
            self._close(node, "Failed", message)

    async def _run_attempts(self, tmpl: Dict[str, Any], target: Target, args: Dict[str, str],
                            node_id: str, display: str, parent: Optional[str],
                            wf_scope: Scope) -> Result:
        retry = tmpl.get("retryStrategy")
        if not isinstance(retry, dict):
            return await self._run_once(tmpl, target, args, node_id, display, parent,
                                        wf_scope, None)

        node = self._open(node_id, display, "Retry", target, parent)
        try:
            limit = int(str(substitute(retry.get("limit") or 0, wf_scope)).strip() or 0)
            backoff = retry.get("backoff") if isinstance(retry.get("backoff"), dict) else None
            wait = parse_duration(backoff.get("duration", 0)) if backoff else 0.0
            factor = float(backoff.get("factor") or 1) if backoff else 1.0
            max_duration = (
                parse_duration(backoff["maxDuration"])
                if backoff and backoff.get("maxDuration") is not None else None
            )
        except (TemplateError, ValueError) as e:
            msg = f"invalid retryStrategy: {e}"
            self._close(node, "Failed", msg)
            return "Failed", msg, None
        started = time.monotonic()
        attempt = 0
        while True:
            phase, message, outputs = await self._run_once(
                tmpl, target, args, f"{node_id}({attempt})", f"{display}({attempt})",
                node_id, wf_scope, attempt,
            )
            if phase == "Succeeded" or attempt >= limit:
                break
            attempt += 1
            delay = wait * factor ** (attempt - 1)
            # a retry that would start later than maxDuration after the first
            # attempt began never starts — so do not wait for it either
            if max_duration is not None and time.monotonic() - started + delay > max_duration:
                break
            if delay > 0:
                await asyncio.sleep(delay)
        self._close(node, phase, message, outputs)
        return phase, message, outputs

    async def _run_once(self, tmpl: Dict[str, Any], target: Target, args: Dict[str, str],
                        node_id: str, display: str, parent: Optional[str], wf_scope: Scope,
                        attempt: Optional[int]) -> Result:
        tscope = target[0]
        if "steps" in tmpl:
            type_ = "Steps"
        elif "dag" in tmpl:
            type_ = "DAG"
        elif "suspend" in tmpl:
            type_ = "Suspend"
        elif "http" in tmpl:
            type_ = "HTTP"
        else:
            type_ = "Pod"
        node = self._open(node_id, display, type_, (tscope, tmpl.get("name"), target[2]), parent)
        outputs: Optional[Outputs] = None
        try:
            scope = self._inputs(tmpl, args, wf_scope)
            if attempt is not None:
                scope["retries"] = str(attempt)
            if type_ == "Steps":
                ok, message = await self._run_steps(tmpl, node_id, scope, tscope)
            elif type_ == "DAG":
                ok, message = await self._run_dag(tmpl, node_id, scope, tscope)
            elif type_ == "Suspend":
                duration = substitute((tmpl["suspend"] or {}).get("duration", 0) or 0, scope)
                await asyncio.sleep(parse_duration(duration))
                ok, message = True, ""
            elif type_ == "HTTP":
                ok, message, outputs = await self._run_http(tmpl, scope, node)
            elif "container" in tmpl or "script" in tmpl:
                ok, message, outputs = await self._run_leaf(tmpl, scope, node)
            else:
                ok, message = False, "unsupported template type"
            if ok and type_ in ("Steps", "DAG"):
                outputs = self._composite_outputs(tmpl, scope)
        except TemplateError as e:
            ok, message, outputs = False, str(e), None
        if ok and outputs:
            self._export_globals(tmpl, outputs, leaf=type_ in ("Pod", "HTTP"))
        phase = "Succeeded" if ok else "Failed"
        self._close(node, phase, message, outputs)
        return phase, message, outputs if ok else None

    def _export_globals(self, tmpl: Dict[str, Any], outputs: Outputs, leaf: bool) -> None:
        """Surface output parameters into ``status.outputs.parameters`` (the
        custom-metrics contract). Leaf parameters surface under ``globalName``
        or, lacking one, their own name; composite templates only re-export
        what carries a ``globalName``."""
        for p in (tmpl.get("outputs") or {}).get("parameters") or []:
            if not isinstance(p, dict) or p.get("name") not in outputs["parameters"]:
                continue
            if leaf or p.get("globalName"):
                self.global_outputs.append({
                    "name": p.get("globalName") or p["name"],
                    "value": outputs["parameters"][p["name"]],
                })

    def _composite_outputs(self, tmpl: Dict[str, Any], scope: Scope) -> Optional[Outputs]:
        params: Dict[str, str] = {}
        for p in (tmpl.get("outputs") or {}).get("parameters") or []:
            if not isinstance(p, dict) or p.get("name") is None:
                continue
            value_from = p.get("valueFrom") if isinstance(p.get("valueFrom"), dict) else {}
            if p.get("value") is not None:
                params[p["name"]] = substitute(to_str(p["value"]), scope)
            elif value_from.get("parameter") is not None:
                try:
                    params[p["name"]] = substitute(to_str(value_from["parameter"]), scope)
                except UnresolvedReference:
                    if value_from.get("default") is None:
                        raise
                    params[p["name"]] = to_str(value_from["default"])
            elif value_from.get("default") is not None:
                params[p["name"]] = to_str(value_from["default"])
        return {"result": None, "parameters": params} if params else None

    # -- steps and DAGs ---------------------------------------------------

    async def _run_steps(self, tmpl: Dict[str, Any], node_id: str, scope: Scope,
                         tscope: str = OWN_SCOPE) -> Tuple[bool, str]:
        bound = _parallelism_bound(tmpl)
        for i, group in enumerate(tmpl["steps"] or []):
            steps = [s for s in (group if isinstance(group, list) else [group])
                     if isinstance(s, dict)]
            gid = f"{node_id}[{i}]"
            gnode = self._open(gid, f"[{i}]", "StepGroup", None, node_id)
            results = await _gather([
                self._run_call(s, "steps", gid, f"{gid}.{s.get('name')}", scope, bound, tscope)
                for s in steps
            ])
            failed = [msg for phase, msg, _ in results if phase == "Failed"]
            self._close(gnode, "Failed" if failed else "Succeeded", failed[0] if failed else "")
            if failed:
                return False, failed[0]
        return True, ""

    async def _run_dag(self, tmpl: Dict[str, Any], node_id: str, scope: Scope,
                       tscope: str = OWN_SCOPE) -> Tuple[bool, str]:
        dag = tmpl["dag"] or {}
        tasks = {t.get("name"): t for t in dag.get("tasks") or [] if isinstance(t, dict)}
        deps = {name: task_dependencies(t) for name, t in tasks.items()}
        fail_fast = dag.get("failFast", True) is not False
        bound = _parallelism_bound(tmpl)
        if bound is not None:
            bound.fail_fast = fail_fast
        phases: Dict[str, str] = {}
        running: Dict["asyncio.Future[Result]", str] = {}
        first_failure: Optional[str] = None

        def omit(name: str, why: str) -> None:
            phases[name] = "Omitted"
            self._mark(f"{node_id}.{name}", name, self._target(tasks[name], tscope), node_id,
                       "Omitted", why)

        try:
            while True:
                for name in tasks:
                    if name in phases or name in running.values():
                        continue
                    if first_failure is not None and fail_fast:
                        continue
                    states = [phases.get(d) for d in deps[name]]
                    if any(s in ("Failed", "Omitted") for s in states):
                        omit(name, "omitted: a dependency did not succeed")
                    elif all(s in ("Succeeded", "Skipped") for s in states):
                        fut = asyncio.ensure_future(self._run_call(
                            tasks[name], "tasks", node_id, f"{node_id}.{name}", scope, bound,
                            tscope,
                        ))
                        running[fut] = name
                if not running:
                    break
                done, _ = await asyncio.wait(running, return_when=asyncio.FIRST_COMPLETED)
                for fut in sorted(done, key=lambda f: list(running).index(f)):
                    name = running.pop(fut)
                    phase, message, _ = fut.result()
                    phases[name] = phase
                    if phase == "Failed" and first_failure is None:
                        first_failure = message
        finally:
            await _cancel_all(list(running))
        for name in tasks:
            if name not in phases:
                omit(name, "omitted: the DAG failed before this task could start")
        if first_failure is not None:
            return False, first_failure
        return True, ""

    async def _run_call(self, call: Dict[str, Any], kind: str, parent: str, node_id: str,
                        scope: Scope, bound: Optional[Bound] = None,
                        tscope: str = OWN_SCOPE) -> Result:
        """One step or DAG task: loop expansion, ``when``, arguments, then
        the template it names. Publishes ``steps.NAME.*`` / ``tasks.NAME.*``
        into the caller's scope when it ran exactly once. ``bound`` is the
        calling template's ``parallelism``: the call, or each item of its
        loop, holds one slot of it from start to end. ``tscope`` is the
        calling template's scope, where a ``template:`` of the call is looked
        up. A failure under ``continueOn: {failed: true}`` is published as
        ``Failed`` and returned as a success."""
        name = str(call.get("name"))
        target = self._target(call, tscope)
        # a failure that is continued past keeps its nodes and its status
        # Failed, and reads as a success to the caller alone
        continued: Result = ("Succeeded", "", None)
        try:
            if "withItems" in call or "withParam" in call or "withSequence" in call:
                if "withItems" in call:
                    items = call["withItems"]
                    if not isinstance(items, list):
                        raise TemplateError("withItems is not a list")
                elif "withSequence" in call:
                    items = expand_sequence(call["withSequence"], scope)
                else:
                    items = parse_with_param(substitute(to_str(call["withParam"]), scope))
                results = await _gather([
                    self._run_expanded(
                        call, target, parent, f"{parent}.{item_display_name(name, i, item)}",
                        item_display_name(name, i, item), {**scope, **item_scope(item)},
                        bound,
                    )
                    for i, item in enumerate(items)
                ])
                failed = [msg for phase, msg, _ in results if phase == "Failed"]
                if failed:
                    phase = "Failed"
                elif any(phase == "Omitted" for phase, _, _ in results):
                    phase = "Omitted"
                else:
                    phase = "Succeeded"
                scope[f"{kind}.{name}.status"] = phase
                if failed and _continues(call):
                    return continued
                return phase, failed[0] if failed else "", None
            phase, message, outputs = await self._run_expanded(
                call, target, parent, node_id, name, scope, bound)
        except TemplateError as e:
            self._mark(node_id, name, target, parent, "Failed", str(e))
            return "Failed", str(e), None
        scope[f"{kind}.{name}.status"] = phase
        if phase == "Failed" and _continues(call):
            return continued
        if phase == "Succeeded" and outputs:
            if outputs.get("result") is not None:
                scope[f"{kind}.{name}.outputs.result"] = outputs["result"]
            for k, v in (outputs.get("parameters") or {}).items():
                scope[f"{kind}.{name}.outputs.parameters.{k}"] = v
        return phase, message, outputs

    async def _run_expanded(self, call: Dict[str, Any], target: Target, parent: str,
                            node_id: str, display: str, scope: Scope,
                            bound: Optional[Bound] = None) -> Result:
        if bound is None:
            return await self._run_child(call, target, parent, node_id, display, scope)
        await bound.acquire()
        try:
            if bound.closed:
                message = "omitted: the DAG failed before this task could start"
                self._mark(node_id, display, target, parent, "Omitted", message)
                return "Omitted", message, None
            result = await self._run_child(call, target, parent, node_id, display, scope)
            if result[0] == "Failed" and bound.fail_fast and not _continues(call):
                bound.closed = True  # before the slot goes to the next in line
            return result
        finally:
            bound.release()

    async def _run_child(self, call: Dict[str, Any], target: Target, parent: str,
                         node_id: str, display: str, scope: Scope) -> Result:
        try:
            if call.get("when") is not None:
                expr = substitute(to_str(call["when"]), scope)
                if not eval_when(expr):
                    message = f"when {expr!r} evaluated false"
                    self._mark(node_id, display, target, parent, "Skipped", message)
                    return "Skipped", message, None
            args: Dict[str, str] = {}
            for p in (call.get("arguments") or {}).get("parameters") or []:
                if isinstance(p, dict) and p.get("name") is not None and p.get("value") is not None:
                    args[str(p["name"])] = substitute(to_str(p["value"]), scope)
        except TemplateError as e:
            self._mark(node_id, display, target, parent, "Failed", str(e))
            return "Failed", str(e), None
        return await self._run_template(target, args, node_id, display, parent, scope)

    # -- leaves -----------------------------------------------------------

    async def _run_leaf(self, tmpl: Dict[str, Any], scope: Scope,
                        node: Dict[str, Any]) -> Tuple[bool, str, Optional[Outputs]]:
        stdin: Optional[bytes] = None
        try:
            deadline = active_deadline(tmpl.get("activeDeadlineSeconds"), scope)
        except TemplateError as e:
            return False, f"invalid activeDeadlineSeconds: {e}", None
        if "container" in tmpl:
            body = tmpl["container"] or {}
            cmd = substitute_list(body.get("command"), scope) + substitute_list(
                body.get("args"), scope
            )
            if not cmd:
                return False, "container template has no command", None
        else:
            body = tmpl["script"] or {}
            cmd = substitute_list(body.get("command"), scope) or ["sh"]
            stdin = str(substitute(body.get("source", "") or "", scope)).encode()
        env = None
        for e in body.get("env") or []:
            # valueFrom sources (secrets, field refs) have no local equivalent
            if isinstance(e, dict) and e.get("name") is not None and e.get("value") is not None:
                if env is None:
                    env = dict(os.environ)
                env[str(e["name"])] = str(substitute(to_str(e["value"]), scope))

        out_params = [
            p for p in (tmpl.get("outputs") or {}).get("parameters") or []
            if isinstance(p, dict) and p.get("name") is not None
        ]
        needs_dir = any(
            isinstance(p.get("valueFrom"), dict) and p["valueFrom"].get("path") is not None
            for p in out_params
        )
        workdir = tempfile.mkdtemp(prefix="am-wf-") if needs_dir else None
        try:
            held: List[Bound] = []
            try:
                # around the process only; a cancellation while waiting, or
                # while running, unwinds through here and frees what is held
                for bound in self._process_bounds:
                    await bound.acquire()
                    held.append(bound)
                if deadline is None:
                    ok, message, stdout = await self._exec(cmd, stdin, env, workdir, node)
                else:
                    # the clock of one attempt starts with its process, not
                    # with the wait for a slot. The cancellation that expiry
                    # sends takes the kill path of _exec and is awaited, so
                    # the group is gone and the log closed when this returns
                    try:
                        ok, message, stdout = await asyncio.wait_for(
                            self._exec(cmd, stdin, env, workdir, node), deadline)
                    except asyncio.TimeoutError:
                        ok, message, stdout = False, POD_DEADLINE_MESSAGE, b""
            finally:
                for bound in reversed(held):
                    bound.release()
            if not ok:
                return False, message, None
            params: Dict[str, str] = {}
            for p in out_params:
                value_from = p.get("valueFrom") if isinstance(p.get("valueFrom"), dict) else {}
                value: Any = None
                if p.get("value") is not None:
                    value = substitute(to_str(p["value"]), scope)
                elif value_from.get("path") is not None:
                    path = os.path.join(workdir or "", str(substitute(value_from["path"], scope)))
                    try:
                        with open(path, "rb") as f:
                            value = f.read(RESULT_MAX_BYTES).decode(errors="replace")
                        if value.endswith("\n"):
                            value = value[:-1]
                    except OSError:
                        if value_from.get("default") is None:
                            return False, (
                                f"output parameter {p['name']!r}: "
                                f"{value_from['path']} not found and no default given"
                            ), None
                        value = to_str(value_from["default"])
                elif value_from.get("default") is not None:
                    value = to_str(value_from["default"])
                if value is not None:
                    params[str(p["name"])] = value
            result = stdout[:RESULT_MAX_BYTES].decode(errors="replace")
            if result.endswith("\n"):
                result = result[:-1]
            return True, "", {"result": result, "parameters": params}
        finally:
            if workdir is not None:
                shutil.rmtree(workdir, ignore_errors=True)

    async def _run_http(self, tmpl: Dict[str, Any], scope: Scope,
                        node: Dict[str, Any]) -> Tuple[bool, str, Optional[Outputs]]:
        """One HTTP probe on the event loop: no process, so no slot of
        ``spec.parallelism`` or of the engine's process bound. A cancellation
        unwinds through the probe, which closes its socket first."""
        from .httpprobe import ProbeError, Request, probe

        body = tmpl["http"] or {}
        url = str(substitute(to_str(body.get("url") or ""), scope))
        method = str(substitute(to_str(body.get("method") or "GET"), scope))
        headers = tuple(
            (str(h["name"]), str(substitute(to_str(h["value"]), scope)))
            for h in body.get("headers") or []
            if isinstance(h, dict) and h.get("name") is not None and h.get("value") is not None
        )
        sent = body.get("body")
        if sent is not None:
            sent = str(substitute(to_str(sent), scope))
        timeout = body.get("timeoutSeconds") or HTTP_DEFAULT_TIMEOUT_SECONDS
        condition = None
        if body.get("successCondition") is not None:
            text = str(substitute(to_str(body["successCondition"]), scope))
            try:
                condition = parse_expr(text)
            except ExprError as e:
                return False, f"invalid successCondition: {e}", None

        writer = self._log_writer(node)

        def say(line: str) -> None:
            if writer is not None:
                writer.write(line.encode(errors="replace") + b"\n")

        try:
            if self._http_slots is not None:
                await self._http_slots.acquire()
            try:
                response = await probe(Request(url, method, headers, sent),
                                       timeout=float(timeout),
                                       insecure=body.get("insecureSkipVerify") is True, log=say)
            except ProbeError as e:
                say(f"! {e}")
                return False, str(e), None
            finally:
                if self._http_slots is not None:
                    self._http_slots.release()
            if writer is not None and response.body:
                writer.write(response.body)
        finally:
            if writer is not None:
                writer.close()

        result = response.body.decode(errors="replace")
        env = {"response": {"statusCode": response.status, "body": result,
                            "headers": response.headers}}
        if condition is None:
            if response.status >= 300:
                return False, f"received non-2xx response code: {response.status}", None
        else:
            try:
                met = condition.evaluate_bool(env)
            except ExprError as e:
                return False, f"invalid successCondition: {e}", None
            if not met:
                return False, (f"successCondition {condition.text!r} evaluated false "
                               f"(status {response.status})"), None
        params: Dict[str, str] = {}
        for p in (tmpl.get("outputs") or {}).get("parameters") or []:
            if not isinstance(p, dict) or p.get("name") is None:
                continue
            value_from = p.get("valueFrom") if isinstance(p.get("valueFrom"), dict) else {}
            default = value_from.get("default")
            value: Any = None
            if p.get("value") is not None:
                value = substitute(to_str(p["value"]), scope)
            elif value_from.get("expression") is not None:
                try:
                    found = parse_expr(
                        str(substitute(to_str(value_from["expression"]), scope))
                    ).evaluate(env)
                    if found is None:
                        raise ExprError("the value is nil")
                    value = render_expr(found)
                except ExprError as e:
                    if default is None:
                        return False, f"output parameter {p['name']!r}: {e}", None
                    value = to_str(default)
            elif default is not None:
                value = to_str(default)
            if value is not None:
                params[str(p["name"])] = value
        return True, "", {"result": result, "parameters": params}

    def _log_writer(self, node: Optional[Dict[str, Any]]) -> Any:
        """The log writer of a leaf's node, or None: without a store, or when
        the store cannot take this run (the leaf runs all the same)."""
        if self.logs is None or node is None:
            return None
        try:
            return self.logs.writer(self.namespace, self.name, node["id"],
                                    node["displayName"])
        except (OSError, ValueError) as e:
            log.warning("no log kept for %s/%s node %s: %s",
                        self.namespace, self.name, node["id"], e)
            return None

    async def _exec(self, cmd: List[str], stdin: Optional[bytes], env: Optional[Dict[str, str]],
                    cwd: Optional[str],
                    node: Optional[Dict[str, Any]] = None) -> Tuple[bool, str, bytes]:
        """Run one process in a session of its own, so that the whole group
        — shells and whatever they started — can be killed on cancellation.
        Its output goes to the node's log as it is read; what is returned is
        the first ``RESULT_MAX_BYTES`` of stdout."""
        spawn = asyncio.ensure_future(asyncio.create_subprocess_exec(
            *cmd,
            stdin=asyncio.subprocess.PIPE if stdin is not None else None,
            stdout=asyncio.subprocess.PIPE,
            stderr=asyncio.subprocess.PIPE,
            env=env, cwd=cwd, start_new_session=True,
        ))
        try:
            proc = await asyncio.shield(spawn)
        except asyncio.CancelledError:
            # cancelled in the middle of the spawn: let it finish, so that
            # the child is known and can be killed like any other
            try:
                late = await spawn
            except BaseException:
                late = None
            if late is not None:
                _kill_group(late)
                await late.wait()
            raise
        except (OSError, ValueError) as e:
            return False, str(e), b""
        self._procs[proc.pid] = proc
        writer = self._log_writer(node)
        out = _Kept(RESULT_MAX_BYTES)
        err = _Kept(0)
        pumps = [
            asyncio.ensure_future(_pump(proc.stdout, out, writer)),
            asyncio.ensure_future(_pump(proc.stderr, err, writer)),
        ]
        if stdin is not None:
            pumps.append(asyncio.ensure_future(_feed(proc.stdin, stdin)))
        # shielded: a cancellation must not stop the pumps before the kill,
        # they still have to read what the group wrote until then
        drained = asyncio.gather(*pumps)
        drained.add_done_callback(lambda f: f.cancelled() or f.exception())
        try:
            # both pipes at EOF (every holder of them gone), then the leader
            await asyncio.shield(drained)
            await proc.wait()
        except BaseException:
            _kill_group(proc)
            try:
                await proc.wait()
                await asyncio.wait([drained], timeout=_KILL_DRAIN_SECONDS)
                await _group_gone(proc.pid)
            except asyncio.CancelledError:
                pass
            raise
        finally:
            self._procs.pop(proc.pid, None)
            drained.cancel()
            if writer is not None:
                writer.close()
        if proc.returncode != 0:
            tail = (err.tail or out.tail).decode(errors="replace")[-MESSAGE_TAIL_CHARS:]
            return False, f"exit code {proc.returncode}: {tail}", out.head
        return True, "", out.head


class _Kept:
    """What of one stream stays in memory: its first ``head_max`` bytes and
    its last ``_TAIL_BYTES``."""

    __slots__ = ("head", "head_max", "tail")

    def __init__(self, head_max: int):
        self.head = b""
        self.head_max = head_max
        self.tail = b""

    def add(self, chunk: bytes) -> None:
        if len(self.head) < self.head_max:
            self.head += chunk[:self.head_max - len(self.head)]
        if len(chunk) >= _TAIL_BYTES:
            self.tail = chunk[-_TAIL_BYTES:]
        else:
            self.tail = (self.tail + chunk)[-_TAIL_BYTES:]


async def _pump(stream: "asyncio.StreamReader", kept: _Kept, writer: Any) -> None:
    """Drain one pipe to EOF, a chunk at a time."""
    while True:
        chunk = await stream.read(_PIPE_CHUNK)
        if not chunk:
            return
        kept.add(chunk)
        if writer is not None:
            writer.write(chunk)


async def _feed(stdin: "asyncio.StreamWriter", data: bytes) -> None:
    """Write a script to its interpreter and close the pipe; one that does
    not read all of it is no error."""
    try:
        stdin.write(data)
        await stdin.drain()
    except (BrokenPipeError, ConnectionResetError):
        pass
    try:
        stdin.close()
    except (BrokenPipeError, ConnectionResetError):
        pass


def _kill_group(proc: "asyncio.subprocess.Process") -> None:
    """SIGKILL the process group led by ``proc``.

    The leader may already have exited and been reaped — a shell that put a
    child in the background and returned — while that child keeps the
    leaf's stdout open and so keeps the leaf "running"; the group is
    signalled all the same. This is only called for a leaf whose pipes are
    still open, i.e. while some member of the group is still there, and as
    long as one is, the kernel cannot hand the group id to anyone else. An
    empty group is ESRCH, which is ignored."""
    try:
        os.killpg(proc.pid, signal.SIGKILL)
    except (ProcessLookupError, PermissionError):
        pass


async def _group_gone(pgid: int) -> None:
    """After :func:`_kill_group`: wait, for ``_KILL_REAP_SECONDS`` at the
    most, until the group has no member left, zombies included. The group
    id stays taken for as long as it has one."""
    loop = asyncio.get_running_loop()
    give_up = loop.time() + _KILL_REAP_SECONDS
    while loop.time() < give_up:
        try:
            os.killpg(pgid, 0)
        except (ProcessLookupError, PermissionError):
            return
        await asyncio.sleep(0.05)


async def _cancel_all(tasks: List["asyncio.Future[Any]"]) -> None:
    for t in tasks:
        t.cancel()
    if tasks:
        await asyncio.gather(*tasks, return_exceptions=True)


async def _gather(coros: List[Awaitable[Result]]) -> List[Result]:
    """Run ``coros`` concurrently and return their results in order. If the
    caller is cancelled, every child is cancelled and awaited first, so no
    subprocess outlives its workflow."""
    tasks = [asyncio.ensure_future(c) for c in coros]
    try:
        if tasks:
            await asyncio.wait(tasks)
    finally:
        await _cancel_all([t for t in tasks if not t.done()])
    return [t.result() for t in tasks]

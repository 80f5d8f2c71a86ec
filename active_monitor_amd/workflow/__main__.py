"""Offline workflow tools: ``python -m active_monitor_amd.workflow``.

``lint FILE... [--templates PATH ...]``
    Check Workflow, HealthCheck, WorkflowTemplate or ClusterWorkflowTemplate
    YAML against the surface the local executor supports. The template
    documents of all files given, and of every ``--templates`` file or
    directory of YAML, are what ``templateRef`` and ``workflowTemplateRef``
    are looked up in, by kind and name (a namespace means nothing offline); a
    reference to none of them is a problem. A template document is itself
    checked as a library: every template in it, ``entrypoint`` optional,
    workflow parameters not required to be declared. A HealthCheck is first
    held against the CRD schema the way a strict ``apply`` would (``invalid
    HealthCheck: spec.repeatAfterSec: ...``, ``invalid HealthCheck: unknown
    field "spec.x"``); a cron schedule the controller would use is parsed
    (``invalid HealthCheck: spec.schedule.cron: ...``); then its inline check
    and remedy workflows are linted. Prints one line per problem; exit status
    1 when there are any.

``run FILE [-p name=value ...] [--remedy] [--logs] [--templates PATH ...]``
    Execute one workflow with the local executor against a throw-away
    in-memory store and print the phase and a node table: the first Workflow
    or HealthCheck workflow of FILE. The template documents of FILE and of
    ``--templates`` are put into that store first. For a HealthCheck the
    check workflow runs (``--remedy``: the remedy workflow). ``--logs`` adds
    what every leaf printed, stdout and stderr, under a ``--- NODE ---`` line
    each; for an ``http`` leaf that is its request line, the response's
    status line and the body that was kept. Exit status 0 for ``Succeeded``,
    1 for ``Failed``.

``next (FILE | --cron SPEC) [-n N] [--from RFC3339] [--time-zone ZONE]``
    Print the next N (default 5) activations of a cron schedule, one per
    line: the instant in the schedule's zone, the same instant in UTC, and
    the ``RepeatAfterSec`` the controller would derive at ``--from`` (default
    now). For a FILE, every HealthCheck's ``spec.schedule.cron`` is shown.
    ``--time-zone`` plays the role of the controller's ``--cron-time-zone``.
    A schedule that does not parse prints ``error: ...``; exit status 1.

None of them needs a server.
"""
from __future__ import annotations

import argparse
import asyncio
import os
import sys
from datetime import datetime, timezone
from typing import Any, Dict, Iterator, List, Optional, Tuple

import yaml

from ..api.types import HealthCheck
from ..engine.cronx import CronParseError, parse_standard
from ..engine.parse import (
    WorkflowParseError,
    parse_remedy_workflow_from_healthcheck,
    parse_workflow_from_healthcheck,
)
from ..kube import MemoryApiServer, MemoryClient
from ..kube.errors import NotFoundError
from ..kube.registry import WF_API_VERSION, WF_KIND
from . import LocalWorkflowEngine, validate_workflow_spec
from .logs import LogStore
from .templates import CWFT_KIND, TEMPLATE_KINDS, lookup_in
from .validate import validate_template_library

Templates = Dict[Tuple[bool, str], Dict[str, Any]]


def _inline(wf: Any) -> bool:
    return (
        wf is not None and wf.resource is not None
        and wf.resource.source is not None
        and wf.resource.source.inline is not None
    )


def _schema_problems(doc: Dict[str, Any]) -> List[str]:
    """What an apiserver holding the HealthCheck CRD would refuse under
    strict field validation: schema errors, then unknown fields."""
    import copy

    from ..kube.memory import healthcheck_schemas

    validator = healthcheck_schemas().get((doc.get("apiVersion"), "HealthCheck"))
    if validator is None:
        return []  # another apiVersion: HealthCheck.from_dict has the say
    pruned, errs = validator.admit(copy.deepcopy(doc))
    if errs:
        return [f"invalid HealthCheck: {e}" for e in errs]
    return [f'invalid HealthCheck: unknown field "{p}"' for p in pruned]


def _load(path: str) -> List[Any]:
    with open(path) as f:
        return [d for d in yaml.safe_load_all(f) if d is not None]


def _template_set(files: List[str], extra: List[str]) -> Templates:
    """Every template document of ``files`` and of ``extra`` (files, or
    directories whose ``*.yaml`` / ``*.yml`` are read), by (cluster scope,
    name). A file that cannot be read is skipped here: as one of ``files``
    it is reported when it is linted itself."""
    paths = list(files)
    for p in extra:
        if os.path.isdir(p):
            paths += sorted(os.path.join(p, n) for n in os.listdir(p)
                            if n.endswith((".yaml", ".yml")))
        else:
            paths.append(p)
    found: Templates = {}
    for path in paths:
        try:
            docs = _load(path)
        except (OSError, yaml.YAMLError):
            continue
        for doc in docs:
            if isinstance(doc, dict) and doc.get("kind") in TEMPLATE_KINDS:
                name = (doc.get("metadata") or {}).get("name")
                if isinstance(name, str):
                    found[(doc["kind"] == CWFT_KIND, name)] = doc
    return found


def _specs(path: str, templates: Optional[Templates] = None
           ) -> Iterator[Tuple[str, Optional[Dict[str, Any]], List[str]]]:
    """``(label, spec, problems)`` for every workflow found in ``path``; a
    template document yields its problems as a library and no spec."""
    try:
        docs = _load(path)
    except (OSError, yaml.YAMLError) as e:
        yield path, None, [str(e)]
        return
    for i, doc in enumerate(docs):
        label = path if len(docs) == 1 else f"{path}[{i}]"
        kind = doc.get("kind") if isinstance(doc, dict) else None
        if kind == "Workflow":
            spec = doc.get("spec")
            yield label, spec, [] if isinstance(spec, dict) else ["invalid workflow, missing spec"]
        elif kind == "HealthCheck":
            problems = _schema_problems(doc)
            if problems:
                yield label, None, problems
                continue
            try:
                hc = HealthCheck.from_dict(doc)
            except Exception as e:
                yield label, None, [f"invalid HealthCheck: {e}"]
                continue
            if hc.spec.repeat_after_sec <= 0 and hc.spec.schedule.cron:
                try:
                    parse_standard(hc.spec.schedule.cron)
                except CronParseError as e:
                    yield label, None, [f"invalid HealthCheck: spec.schedule.cron: {e}"]
                    continue
            found = False
            for what, wf, parse in (
                ("workflow", hc.spec.workflow, parse_workflow_from_healthcheck),
                ("remedyworkflow", hc.spec.remedy_workflow,
                 parse_remedy_workflow_from_healthcheck),
            ):
                if not _inline(wf):
                    continue
                found = True
                try:
                    spec, _ = parse(hc)
                    yield f"{label} ({what})", spec, []
                except WorkflowParseError as e:
                    yield f"{label} ({what})", None, [str(e)]
            if not found:
                yield label, None, []  # file/URL sources: nothing to lint offline
        elif kind in TEMPLATE_KINDS:
            yield label, None, validate_template_library(
                doc, lookup_in(templates) if templates is not None else None)
        else:
            yield label, None, [
                "expected kind Workflow, HealthCheck, WorkflowTemplate or "
                f"ClusterWorkflowTemplate, found {kind!r}"]


def lint(paths: List[str], templates: Optional[List[str]] = None) -> int:
    library = _template_set(paths, templates or [])
    bad = 0
    for path in paths:
        for label, spec, problems in _specs(path, library):
            if spec is not None and not problems:
                problems = validate_workflow_spec(spec, lookup_in(library))
            for p in problems:
                print(f"{label}: {p}")
            bad += len(problems)
    if not bad:
        print("ok")
    return 1 if bad else 0


async def _execute(spec: Dict[str, Any], name: str, logs: Optional[LogStore] = None,
                   templates: Optional[Templates] = None) -> Dict[str, Any]:
    client = MemoryClient(MemoryApiServer())
    for doc in (templates or {}).values():
        # offline a template's namespace means nothing: it goes where the
        # Workflow goes
        await client.create({**doc, "metadata": {
            "name": doc["metadata"]["name"], "namespace": "local"}})
    engine = LocalWorkflowEngine(client, ttl_seconds=None, logs=logs)
    sub = client.watch(WF_API_VERSION, WF_KIND, "local")
    await engine.start()
    try:
        await client.create({
            "apiVersion": WF_API_VERSION, "kind": WF_KIND,
            "metadata": {"name": name, "namespace": "local"}, "spec": spec,
        })
        async for ev in sub:
            status = ev["object"].get("status") or {}
            if status.get("phase") in ("Succeeded", "Failed"):
                return status
    finally:
        sub.close()
        await engine.stop()
    raise RuntimeError("workflow watch ended before the workflow did")


def _print_nodes(status: Dict[str, Any]) -> None:
    nodes = status.get("nodes") or {}
    if not nodes:
        return
    child_ids = {c for n in nodes.values() for c in n.get("children", [])}
    rows: List[Tuple[str, str, str, str]] = []

    def walk(node_id: str, depth: int) -> None:
        n = nodes[node_id]
        rows.append(("  " * depth + n["displayName"], n["type"], n.get("phase", ""),
                     " ".join((n.get("message") or "").split())[:100]))
        for c in n.get("children", []):
            if c in nodes:
                walk(c, depth + 1)

    for node_id in nodes:
        if node_id not in child_ids:
            walk(node_id, 0)
    width = max(len(r[0]) for r in rows + [("NODE", "", "", "")])
    print(f"{'NODE':<{width}}  {'TYPE':<9}  {'PHASE':<9}  MESSAGE")
    for name, type_, phase, message in rows:
        print(f"{name:<{width}}  {type_:<9}  {phase:<9}  {message}".rstrip())


async def _execute_with_logs(spec: Dict[str, Any], name: str,
                             templates: Optional[Templates] = None
                             ) -> Tuple[Dict[str, Any], bytes]:
    """``_execute`` over a temporary log store; also returns the log of
    every Pod and HTTP node, in start order, under a ``--- displayName ---``
    line."""
    logs = LogStore()
    try:
        status = await _execute(spec, name, logs, templates)
        out: List[bytes] = []
        for node in (status.get("nodes") or {}).values():
            if node.get("type") not in ("Pod", "HTTP") or not logs.has_run("local", name):
                continue
            out.append(f"--- {node['displayName']} ---\n".encode())
            try:
                text = b"".join([c async for c in logs.read("local", name, node["id"])])
            except NotFoundError:
                text = b""
            out.append(text if not text or text.endswith(b"\n") else text + b"\n")
        return status, b"".join(out)
    finally:
        logs.close()


def run(path: str, params: List[str], remedy: bool, logs: bool = False,
        templates: Optional[List[str]] = None) -> int:
    wanted = "(remedyworkflow)" if remedy else "(workflow)"
    found: List[Tuple[str, Dict[str, Any]]] = []
    library = _template_set([path], templates or [])
    for label, spec, problems in _specs(path, library):
        if problems:
            print(f"{label}: {problems[0]}")
            return 1
        if spec is not None:
            found.append((label, spec))
    # a HealthCheck yields "(workflow)" / "(remedyworkflow)"; a bare Workflow
    # document has no suffix and is only eligible without --remedy
    matching = [s for label, s in found if label.endswith(wanted)]
    if not matching and not remedy:
        matching = [s for _, s in found]
    if not matching:
        print(f"{path}: no inline {'remedy ' if remedy else ''}workflow found")
        return 1
    chosen = matching[0]
    overrides = {}
    for p in params:
        name, sep, value = p.partition("=")
        if not sep:
            print(f"-p expects name=value, got {p!r}")
            return 2
        overrides[name] = value
    if overrides:
        args = chosen.setdefault("arguments", {})
        declared = [q for q in args.get("parameters") or []
                    if isinstance(q, dict) and q.get("name") not in overrides]
        args["parameters"] = declared + [{"name": k, "value": v} for k, v in overrides.items()]
    log_text = b""
    if logs:
        status, log_text = asyncio.run(_execute_with_logs(chosen, "run", library))
    else:
        status = asyncio.run(_execute(chosen, "run", templates=library))
    print(f"phase: {status['phase']}")
    if status.get("message"):
        print(f"message: {status['message']}")
    for p in (status.get("outputs") or {}).get("parameters") or []:
        print(f"output {p['name']}: {p['value']}")
    _print_nodes(status)
    if log_text:
        sys.stdout.flush()
        sys.stdout.buffer.write(log_text)
        sys.stdout.buffer.flush()
    return 0 if status["phase"] == "Succeeded" else 1


def _crons(path: str) -> List[Tuple[str, str]]:
    """``(label, spec.schedule.cron)`` for every HealthCheck in ``path``."""
    with open(path) as f:
        docs = [d for d in yaml.safe_load_all(f) if isinstance(d, dict)]
    out = []
    for doc in docs:
        if doc.get("kind") != "HealthCheck":
            continue
        name = (doc.get("metadata") or {}).get("name") or path
        cron = ((doc.get("spec") or {}).get("schedule") or {}).get("cron")
        if not cron:
            raise CronParseError(f"{name}: no spec.schedule.cron")
        out.append((name, str(cron)))
    if not out:
        raise CronParseError(f"{path}: no HealthCheck found")
    return out


def next_activations(path: Optional[str], cron: Optional[str], count: int,
                     start: Optional[str], time_zone: Optional[str]) -> int:
    try:
        if start is None:
            now = datetime.now(timezone.utc).replace(microsecond=0)
        else:
            now = datetime.fromisoformat(start[:-1] + "+00:00" if start[-1:] in "Zz" else start)
            if now.tzinfo is None:
                raise ValueError(f"--from needs a UTC offset or Z: {start!r}")
        crons = [("", cron)] if cron is not None else _crons(path)
        for label, spec in crons:
            sched = parse_standard(spec, default_zone=time_zone)
            # a schedule without any zone runs on the controller's own clock
            t = now if sched.zone is not None else now.astimezone()
            if label:
                print(f"{label}: {spec}")
            for _ in range(count):
                nxt = sched.next(t)
                shown = nxt.astimezone(sched.zone) if sched.zone is not None else nxt
                print(f"{shown.isoformat()}  {nxt.astimezone(timezone.utc):%Y-%m-%dT%H:%M:%SZ}"
                      f"  RepeatAfterSec={int((nxt - now).total_seconds()) + 1}")
                t = nxt
    except (OSError, ValueError, yaml.YAMLError) as e:  # CronParseError is a ValueError
        print(f"error: {e}")
        return 1
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(
        prog="python -m active_monitor_amd.workflow",
        description="Lint or run workflows with the local executor; no server needed.",
    )
    sub = ap.add_subparsers(dest="cmd", required=True)
    p_lint = sub.add_parser(
        "lint", help="check Workflow / HealthCheck / WorkflowTemplate YAML")
    p_lint.add_argument("files", nargs="+", metavar="FILE")
    shared = dict(action="append", default=[], metavar="PATH",
                  help="a file, or a directory of YAML, whose WorkflowTemplates and "
                       "ClusterWorkflowTemplates references are looked up in (repeatable)")
    p_lint.add_argument("--templates", **shared)
    p_run = sub.add_parser("run", help="execute one workflow locally")
    p_run.add_argument("file", metavar="FILE")
    p_run.add_argument("-p", "--parameter", action="append", default=[], metavar="name=value",
                       help="set or override a spec.arguments parameter")
    p_run.add_argument("--remedy", action="store_true",
                       help="for a HealthCheck, run its remedy workflow instead of the check")
    p_run.add_argument("--logs", action="store_true",
                       help="after the node table, print what each leaf printed")
    p_run.add_argument("--templates", **shared)
    p_next = sub.add_parser("next", help="print a cron schedule's next activations")
    what = p_next.add_mutually_exclusive_group(required=True)
    what.add_argument("file", nargs="?", metavar="FILE",
                      help="HealthCheck YAML; its spec.schedule.cron is used")
    what.add_argument("--cron", metavar="SPEC", help="a cron schedule, e.g. "
                      "'CRON_TZ=Europe/Berlin 0 9 * * MON-FRI'")
    p_next.add_argument("-n", type=int, default=5, metavar="N",
                        help="how many activations (default 5)")
    p_next.add_argument("--from", dest="start", default=None, metavar="RFC3339",
                        help="start after this instant (default: now)")
    p_next.add_argument("--time-zone", default=None, metavar="ZONE",
                        help="zone for a schedule without a TZ=/CRON_TZ= prefix, "
                             "as the controller's --cron-time-zone")
    args = ap.parse_args(argv)
    if args.cmd == "lint":
        return lint(args.files, args.templates)
    if args.cmd == "next":
        return next_activations(args.file, args.cron, args.n, args.start, args.time_zone)
    return run(args.file, args.parameter, args.remedy, args.logs, args.templates)


if __name__ == "__main__":
    sys.exit(main())

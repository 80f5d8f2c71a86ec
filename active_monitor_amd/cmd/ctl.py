"""amctl — operator CLI for the HealthCheck API.

The reference's operator UX is kubectl against the CRD (shortnames hc/hcs,
printcolumns — healthcheck_types.go:68-76); amctl provides the same surface
against any server speaking the Kubernetes REST API, including this
framework's standalone ``--serve-api`` endpoint:

    amctl --server http://127.0.0.1:8001 get hc -n health
    amctl --server ... describe hc inline-hello -n health
    amctl --server ... apply -f examples/inline-hello.yaml
    amctl --server ... delete hc inline-hello -n health
    amctl --server ... logs hc inline-hello -n health
    amctl --server ... run hc inline-hello -n health --wait
    amctl --server ... get wftmpl -n health
    amctl --server ... get cwft

``run`` asks the controller to run a check now (docs/OPERATIONS.md, "Running
a check on demand"); it is ``kubectl annotate --overwrite`` with a fresh
token, plus the waiting. ``logs`` and ``run --logs`` need the standalone apiserver: on a cluster the output of a
workflow is the logs of its pods (``kubectl logs``, ``argo logs``).
"""
from __future__ import annotations

import argparse
import asyncio
import sys
import time
from datetime import datetime, timezone
from typing import Any, Dict, List, Optional

import yaml

from .. import API_VERSION
from ..api.runrequest import (
    RUN_HANDLED_ANNOTATION,
    RUN_REQUESTED_ANNOTATION,
    RUN_WORKFLOW_ANNOTATION,
    new_run_token,
)
from ..api.types import parse_k8s_time
from ..kube.config import get_config
from ..kube.errors import (
    AlreadyExistsError,
    BadRequestError,
    ConflictError,
    InvalidError,
    NotFoundError,
)
from ..kube.http import HttpClient
from ..kube.registry import WF_API_VERSION

ALIASES = {
    "hc": (API_VERSION, "HealthCheck"),
    "hcs": (API_VERSION, "HealthCheck"),
    "healthcheck": (API_VERSION, "HealthCheck"),
    "healthchecks": (API_VERSION, "HealthCheck"),
    "wf": (WF_API_VERSION, "Workflow"),
    "workflow": (WF_API_VERSION, "Workflow"),
    "workflows": (WF_API_VERSION, "Workflow"),
    "events": ("v1", "Event"),
    "event": ("v1", "Event"),
    "wftmpl": (WF_API_VERSION, "WorkflowTemplate"),
    "workflowtemplate": (WF_API_VERSION, "WorkflowTemplate"),
    "workflowtemplates": (WF_API_VERSION, "WorkflowTemplate"),
    # cluster-scoped: -n is ignored
    "cwft": (WF_API_VERSION, "ClusterWorkflowTemplate"),
    "cwftmpl": (WF_API_VERSION, "ClusterWorkflowTemplate"),
    "clusterworkflowtemplate": (WF_API_VERSION, "ClusterWorkflowTemplate"),
    "clusterworkflowtemplates": (WF_API_VERSION, "ClusterWorkflowTemplate"),
}


def _age(creation: Optional[str]) -> str:
    t = parse_k8s_time(creation)
    if t is None:
        return "<unknown>"
    delta = datetime.now(timezone.utc) - t
    secs = int(delta.total_seconds())
    if secs < 120:
        return f"{secs}s"
    if secs < 7200:
        return f"{secs // 60}m"
    if secs < 172800:
        return f"{secs // 3600}h"
    return f"{secs // 86400}d"


def _table(headers: List[str], rows: List[List[str]]) -> str:
    widths = [max(len(h), *(len(r[i]) for r in rows)) if rows else len(h)
              for i, h in enumerate(headers)]
    out = ["   ".join(h.ljust(w) for h, w in zip(headers, widths)).rstrip()]
    for r in rows:
        out.append("   ".join(c.ljust(w) for c, w in zip(r, widths)).rstrip())
    return "\n".join(out)


def _hc_row(o: Dict[str, Any]) -> List[str]:
    st = o.get("status") or {}
    return [
        o["metadata"]["name"],
        st.get("status", "") or "<none>",
        str(st.get("successCount", 0)),
        str(st.get("failedCount", 0)),
        str(st.get("remedySuccessCount", 0)),
        str(st.get("remedyFailedCount", 0)),
        _age(o["metadata"].get("creationTimestamp")),
    ]


async def cmd_get(client: HttpClient, args) -> int:
    av, kind = ALIASES[args.resource]
    if args.name:
        objs = [await client.get(av, kind, args.namespace, args.name)]
    else:
        objs = await client.list(av, kind, args.namespace or None)
    if args.output == "yaml":
        print(yaml.safe_dump_all(objs, sort_keys=False).rstrip())
        return 0
    if kind == "HealthCheck":
        # the CRD's printcolumns (healthcheck_types.go:71-76)
        print(_table(
            ["NAME", "LATEST STATUS", "SUCCESS CNT", "FAIL CNT",
             "REMEDY SUCCESS CNT", "REMEDY FAIL CNT", "AGE"],
            [_hc_row(o) for o in objs],
        ))
    elif kind == "Workflow":
        print(_table(
            ["NAME", "STATUS", "AGE"],
            [[o["metadata"]["name"],
              (o.get("status") or {}).get("phase", "") or "<pending>",
              _age(o["metadata"].get("creationTimestamp"))] for o in objs],
        ))
    elif kind in ("WorkflowTemplate", "ClusterWorkflowTemplate"):
        print(_table(
            ["NAME", "TEMPLATES", "AGE"],
            [[o["metadata"]["name"],
              str(len((o.get("spec") or {}).get("templates") or [])),
              _age(o["metadata"].get("creationTimestamp"))] for o in objs],
        ))
    else:
        print(_table(
            ["NAME", "TYPE", "REASON", "MESSAGE"],
            [[o["metadata"]["name"], o.get("type", ""), o.get("reason", ""),
              (o.get("message", "") or "")[:80]] for o in objs],
        ))
    return 0


async def cmd_describe(client: HttpClient, args) -> int:
    av, kind = ALIASES[args.resource]
    o = await client.get(av, kind, args.namespace, args.name)
    print(yaml.safe_dump(o, sort_keys=False).rstrip())
    return 0


async def _apply_one(client: HttpClient, doc: Dict[str, Any], mode: str) -> None:
    meta = doc.get("metadata") or {}
    name = meta.get("name", "")
    try:
        await client.create(doc, field_validation=mode)
        print(f'{doc.get("kind", "object").lower()}/{name} created')
    except (AlreadyExistsError, ConflictError):
        # exists: update with a fresh resourceVersion
        current = await client.get(
            doc.get("apiVersion", ""), doc.get("kind", ""),
            meta.get("namespace", ""), name,
        )
        doc.setdefault("metadata", {})["resourceVersion"] = (
            current["metadata"]["resourceVersion"]
        )
        await client.update(doc, field_validation=mode)
        print(f'{doc.get("kind", "object").lower()}/{name} configured')


async def cmd_apply(client: HttpClient, args) -> int:
    with open(args.filename) as f:
        docs = [d for d in yaml.safe_load_all(f) if d]
    # kubectl's --validate values, as the fieldValidation the server reads
    mode = args.validate.capitalize()
    rc = 0
    for doc in docs:
        try:
            await _apply_one(client, doc, mode)
        except (InvalidError, BadRequestError) as e:
            # a refused document does not stop the ones after it
            print(f"error: {e.message}", file=sys.stderr)
            rc = 1
        while client.warnings:
            print(f"Warning: {client.warnings.popleft()}", file=sys.stderr)
    return rc


async def cmd_delete(client: HttpClient, args) -> int:
    av, kind = ALIASES[args.resource]
    await client.delete(av, kind, args.namespace, args.name)
    print(f"{args.resource}/{args.name} deleted")
    return 0


class _LogsError(Exception):
    """``amctl logs`` cannot show anything; the message says why."""


async def _hc_workflow(client: HttpClient, args) -> Dict[str, Any]:
    """The Workflow whose log ``logs hc NAME`` shows: the last failed run
    of a check that stands Failed, else the last successful one."""
    hc = await client.get(API_VERSION, "HealthCheck", args.namespace, args.name)
    status = hc.get("status") or {}
    if args.failed:
        which = "lastFailedWorkflow"
    elif args.succeeded:
        which = "lastSuccessfulWorkflow"
    else:
        which = ("lastFailedWorkflow" if status.get("status") == "Failed"
                 else "lastSuccessfulWorkflow")
    wf_name = status.get(which)
    if not wf_name:
        if not status.get("lastFailedWorkflow") and not status.get("lastSuccessfulWorkflow"):
            raise _LogsError(f"healthcheck {args.name} has not run yet")
        kind = "failed" if which == "lastFailedWorkflow" else "successful"
        raise _LogsError(f"healthcheck {args.name} has no {kind} workflow yet")
    # the check and the remedy name a namespace each; the HealthCheck's own
    # is where a workflow without one goes
    spec = hc.get("spec") or {}
    namespaces: List[str] = []
    for key in ("workflow", "remedyworkflow"):
        ns = ((spec.get(key) or {}).get("resource") or {}).get("namespace")
        if ns and ns not in namespaces:
            namespaces.append(ns)
    if args.namespace not in namespaces:
        namespaces.append(args.namespace)
    for ns in namespaces:
        try:
            return await client.get(WF_API_VERSION, "Workflow", ns, wf_name)
        except NotFoundError:
            continue
    raise _LogsError(
        f"workflow {wf_name} of healthcheck {args.name} is gone: a workflow "
        "and its logs are deleted together once the engine TTL has passed")


async def cmd_logs(client: HttpClient, args) -> int:
    try:
        if ALIASES[args.resource][1] == "HealthCheck":
            wf = await _hc_workflow(client, args)
        else:
            wf = await client.get(WF_API_VERSION, "Workflow", args.namespace, args.name)
        meta = wf["metadata"]
        phase = (wf.get("status") or {}).get("phase", "") or "Pending"
        print(f'==> workflow {meta["name"]} ({phase}) <==', file=sys.stderr, flush=True)
        out = sys.stdout.buffer
        try:
            async for chunk in client.logs(
                meta.get("namespace", ""), meta["name"], node=args.node,
                follow=args.follow, tail_lines=args.tail,
                prefix=not (args.no_prefix or args.node is not None),
            ):
                out.write(chunk)
                out.flush()
        except NotFoundError as e:
            raise _LogsError(
                f'{e.message} (workflow {meta["name"]}: a workflow and its logs '
                "are deleted together once the engine TTL has passed)")
    except _LogsError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    return 0


class _RunTimeout(Exception):
    """``amctl run --wait`` ran out of time; the message names the stage."""


_RUN_POLL_SECS = 0.1
_TERMINAL = ("Succeeded", "Failed")


async def _run_handled(client: HttpClient, namespace: str, name: str,
                       token: str, deadline: float) -> Dict[str, Any]:
    """Wait until the controller has acknowledged ``token``; the HealthCheck
    as it stood then."""
    while True:
        hc = await client.get(API_VERSION, "HealthCheck", namespace, name)
        annotations = hc["metadata"].get("annotations") or {}
        if annotations.get(RUN_HANDLED_ANNOTATION) == token:
            return hc
        if time.monotonic() >= deadline:
            raise _RunTimeout("no controller handled the request: is one "
                              "running, and does it own this check?")
        await asyncio.sleep(_RUN_POLL_SECS)


async def _run_verdict(client: HttpClient, namespace: str, name: str,
                       wf_namespace: str, wf_name: str, deadline: float) -> str:
    """Wait until the Workflow that served the request is Succeeded or
    Failed. One that is gone already (TTL) has left its verdict in the
    HealthCheck's status."""
    while True:
        try:
            wf = await client.get(WF_API_VERSION, "Workflow", wf_namespace, wf_name)
            phase = (wf.get("status") or {}).get("phase")
        except NotFoundError:
            hc = await client.get(API_VERSION, "HealthCheck", namespace, name)
            status = hc.get("status") or {}
            phase = None
            if status.get("lastSuccessfulWorkflow") == wf_name:
                phase = "Succeeded"
            elif status.get("lastFailedWorkflow") == wf_name:
                phase = "Failed"
        if phase in _TERMINAL:
            return phase
        if time.monotonic() >= deadline:
            raise _RunTimeout(f"workflow {wf_name} is still running")
        await asyncio.sleep(_RUN_POLL_SECS)


async def _run_follow_logs(client: HttpClient, wf_namespace: str, wf_name: str,
                           deadline: float) -> None:
    async def follow() -> None:
        out = sys.stdout.buffer
        async for chunk in client.logs(wf_namespace, wf_name, follow=True, prefix=True):
            out.write(chunk)
            out.flush()

    try:
        await asyncio.wait_for(follow(), max(0.0, deadline - time.monotonic()))
    except asyncio.TimeoutError:
        raise _RunTimeout(f"workflow {wf_name} is still running")
    except NotFoundError as e:
        raise _LogsError(
            f"{e.message} (workflow {wf_name}: a workflow and its logs "
            "are deleted together once the engine TTL has passed)")


async def cmd_run(client: HttpClient, args) -> int:
    wait = args.wait or args.logs
    if args.all and args.names:
        print("error: --all takes every healthcheck of the namespace: give "
              "no names with it", file=sys.stderr)
        return 2
    if not args.all and not args.names:
        print("error: name a healthcheck, or give --all", file=sys.stderr)
        return 2
    if args.logs and (args.all or len(args.names) != 1):
        print("error: --logs follows one run: give a single name", file=sys.stderr)
        return 2
    names = list(args.names)
    if args.all:
        names = [o["metadata"]["name"] for o in
                 await client.list(API_VERSION, "HealthCheck", args.namespace)]
    requested = []
    for name in names:
        token = new_run_token()
        await client.patch(
            API_VERSION, "HealthCheck", args.namespace, name,
            {"metadata": {"annotations": {RUN_REQUESTED_ANNOTATION: token}}})
        print(f"healthcheck/{name} run requested ({token})", flush=True)
        requested.append((name, token))
    if not wait:
        return 0
    deadline = time.monotonic() + args.timeout
    rc = 0
    for name, token in requested:
        try:
            hc = await _run_handled(client, args.namespace, name, token, deadline)
            wf_name = hc["metadata"]["annotations"].get(RUN_WORKFLOW_ANNOTATION, "")
            resource = ((hc.get("spec") or {}).get("workflow") or {}).get("resource") or {}
            wf_namespace = resource.get("namespace") or args.namespace
            print(f"healthcheck/{name} running as workflow {wf_name}", flush=True)
            if args.logs:
                await _run_follow_logs(client, wf_namespace, wf_name, deadline)
            phase = await _run_verdict(client, args.namespace, name,
                                       wf_namespace, wf_name, deadline)
        except _RunTimeout as e:
            print(f"error: healthcheck/{name}: {e}", file=sys.stderr)
            rc = 2
            continue
        except _LogsError as e:
            print(f"Error: {e}", file=sys.stderr)
            rc = max(rc, 1)
            continue
        print(f"healthcheck/{name} {phase} (workflow {wf_name})", flush=True)
        if phase != "Succeeded":
            rc = max(rc, 1)
    return rc


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="amctl", description=__doc__.splitlines()[0])
    p.add_argument("--server", required=True, help="apiserver URL")
    p.add_argument("--token", default="")
    p.add_argument("--token-file", default=None,
                   help="read the bearer token from this file")
    p.add_argument("--insecure-skip-tls-verify", action="store_true")
    sub = p.add_subparsers(dest="command", required=True)

    g = sub.add_parser("get")
    g.add_argument("resource", choices=sorted(ALIASES))
    g.add_argument("name", nargs="?", default="")
    g.add_argument("-n", "--namespace", default="health")
    g.add_argument("-o", "--output", choices=["table", "yaml"], default="table")

    d = sub.add_parser("describe")
    d.add_argument("resource", choices=sorted(ALIASES))
    d.add_argument("name")
    d.add_argument("-n", "--namespace", default="health")

    a = sub.add_parser("apply")
    a.add_argument("-f", "--filename", required=True)
    a.add_argument("--validate", choices=["strict", "warn", "ignore"],
                   default="strict",
                   help="what the server does with fields its schema does "
                        "not know: strict refuses the document, warn stores "
                        "it without them and says so, ignore stores it "
                        "without them silently (default: strict, as kubectl)")

    rm = sub.add_parser("delete")
    rm.add_argument("resource", choices=sorted(ALIASES))
    rm.add_argument("name")
    rm.add_argument("-n", "--namespace", default="health")

    lg = sub.add_parser(
        "logs", help="what a workflow's leaves printed (standalone apiserver)")
    lg.add_argument("resource", choices=sorted(
        a for a, (_, kind) in ALIASES.items() if kind in ("HealthCheck", "Workflow")))
    lg.add_argument("name")
    lg.add_argument("-n", "--namespace", default="health")
    lg.add_argument("--node", default=None,
                    help="one node, by id or display name (default: all)")
    lg.add_argument("-f", "--follow", action="store_true",
                    help="keep printing until the workflow finishes")
    lg.add_argument("--tail", type=int, default=None, metavar="N",
                    help="only the last N lines of each node")
    which = lg.add_mutually_exclusive_group()
    which.add_argument("--failed", action="store_true",
                       help="hc: the last failed workflow, whatever the status")
    which.add_argument("--succeeded", action="store_true",
                       help="hc: the last successful workflow")
    lg.add_argument("--no-prefix", action="store_true",
                    help="do not put the node's display name before each line")

    rn = sub.add_parser(
        "run", help="ask the controller to run healthchecks now")
    rn.add_argument("resource", choices=sorted(
        a for a, (_, kind) in ALIASES.items() if kind == "HealthCheck"))
    rn.add_argument("names", nargs="*", metavar="NAME")
    rn.add_argument("-n", "--namespace", default="health")
    rn.add_argument("--all", action="store_true",
                    help="every healthcheck of the namespace")
    rn.add_argument("--wait", action="store_true",
                    help="wait for the run: exit 0 when all succeeded, 1 when "
                         "any failed, 2 when --timeout passed")
    rn.add_argument("--timeout", type=float, default=300.0, metavar="SECS",
                    help="how long --wait waits, in all (default: 300)")
    rn.add_argument("--logs", action="store_true",
                    help="follow the run's output (implies --wait; one name; "
                         "standalone apiserver)")
    return p


async def run(args) -> int:
    client = get_config(
        server=args.server, token=args.token,
        insecure=args.insecure_skip_tls_verify,
        token_file=getattr(args, "token_file", None),
    ).make_client()
    await client.start()
    try:
        handler = {"get": cmd_get, "describe": cmd_describe,
                   "apply": cmd_apply, "delete": cmd_delete,
                   "logs": cmd_logs, "run": cmd_run}[args.command]
        return await handler(client, args)
    except NotFoundError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    finally:
        await client.close()


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    return asyncio.run(run(args))


if __name__ == "__main__":
    sys.exit(main())

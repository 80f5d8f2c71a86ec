"""Standalone local apiserver process.

Runs a MemoryApiServer behind the Kubernetes-REST ApiServerFrontend in its
own process, optionally with an in-"cluster" workflow engine playing the
Argo workflow-controller role (completing submitted Workflows the way the
real controller at deploy/deploy-argo.yaml would).

Two consumers:

- ``bench.py``'s default real-wire regime: the controller under test runs in
  a *different* process and reaches this one over 127.0.0.1 HTTP, so the
  measured reconcile path crosses the same process/serialization/TCP boundary
  the reference crosses to kube-apiserver — no shared event loop, no shared
  memory, no zero-RTT self-play.
- a kubectl-able local dev apiserver (``python -m active_monitor_amd.kube.standalone``).

Prints one ``READY {json}`` line on stdout once serving; runs until
SIGTERM/SIGINT.
"""
from __future__ import annotations

import argparse
import asyncio
import json
import os
import signal
import sys

from .memory import healthcheck_schemas
from .server import ApiServerFrontend


#: where the workflow logs live in a data directory; the journal
#: (kube/persist.py) knows its own files only and leaves it alone
LOGS_SUBDIR = "logs"


def bench_policy(remedy_frac: float):
    """The bench fleet's workflow outcomes, decodable from workflow names
    (bench.py make_cr): CR ``hc-NNNNN`` fails its checks iff NNNNN%100 <
    remedy_frac*100; remedy workflows always succeed."""
    cut = remedy_frac * 100.0

    def policy(wf):
        name = (wf.get("metadata") or {}).get("name", "")
        if "-remedy-wf-" in name:
            return ("Succeeded", "")
        base = name.split("-wf-")[0]
        parts = base.split("-")
        if len(parts) == 2 and parts[0] == "hc" and parts[1].isdigit():
            if int(parts[1]) % 100 < cut:
                return ("Failed", "synthetic failure")
        return ("Succeeded", "")

    return policy


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="active-monitor-apiserver")
    p.add_argument("--host", default="127.0.0.1")
    p.add_argument("--port", type=int, default=0, help="0 = ephemeral")
    p.add_argument("--engine", choices=["scripted-bench", "local", "none"],
                   default="none",
                   help="in-cluster workflow engine: scripted-bench completes "
                        "workflows per the bench policy, local executes them "
                        "as subprocesses, none leaves them pending")
    p.add_argument("--remedy-frac", type=float, default=0.2,
                   help="scripted-bench: fraction of CRs whose checks fail")
    p.add_argument("--engine-delay", type=float, default=0.0,
                   help="scripted-bench: simulated workflow runtime (s)")
    p.add_argument("--engine-ttl", type=float, default=60.0,
                   help="completed-workflow TTL seconds (Argo ttlStrategy "
                        "equivalent; bounds server memory at fleet rates)")
    p.add_argument("--token-file", default=None, metavar="FILE",
                   help="require 'Authorization: Bearer <token>' on every "
                        "request but the health probes and /version; FILE "
                        "holds one accepted token per line, read at start "
                        "(default: no authentication)")
    p.add_argument("--data-dir", default=None, metavar="DIR",
                   help="keep the store in DIR (snapshot + journal) so a "
                        "restart finds every object again; one process per "
                        "directory (default: memory only)")
    p.add_argument("--no-schema-validation", dest="schema_validation",
                   action="store_false",
                   help="store HealthChecks as given instead of validating "
                        "and pruning them by the CRD schema (also: "
                        "AM_SCHEMA_VALIDATION=0 in the environment)")
    add_log_flags(p)
    add_limit_flags(p, "engine")
    args = p.parse_args(argv)
    check_log_flags(p, args)
    check_limit_flags(p, args, "engine")
    return args


def add_log_flags(p: argparse.ArgumentParser) -> None:
    """The flags of the workflow log store, for both entry points."""
    p.add_argument("--log-max-bytes", type=int, default=None, metavar="N",
                   help="local engine: keep at most N bytes of output per "
                        "workflow node, the newest (default: 1 MiB)")
    p.add_argument("--log-max-total-bytes", type=int, default=None, metavar="N",
                   help="local engine: keep at most N bytes of workflow "
                        "output in all; beyond it whole finished runs are "
                        "dropped, oldest first (default: 256 MiB)")
    p.add_argument("--no-workflow-logs", dest="workflow_logs",
                   action="store_false",
                   help="local engine: keep no workflow output")


def check_log_flags(p: argparse.ArgumentParser, args) -> None:
    for flag, value in (("--log-max-bytes", args.log_max_bytes),
                        ("--log-max-total-bytes", args.log_max_total_bytes)):
        if value is not None and value < 2:
            p.error(f"{flag} must be 2 or more")


#: engine option -> flag suffix, for ``--engine-*`` here and ``--workflow-*``
#: on the controller
LIMIT_FLAGS = (("parallelism", "parallelism"),
               ("namespace_parallelism", "namespace-parallelism"),
               ("max_processes", "max-processes"))


def add_limit_flags(p: argparse.ArgumentParser, prefix: str) -> None:
    """The flags that bound what the workflow engine runs at once, as
    ``--<prefix>-parallelism`` and so on, for both entry points."""
    for (_, suffix), text in zip(LIMIT_FLAGS, (
            "run at most N workflows at once; the rest wait Pending, "
            "higher spec.priority first, then older first",
            "run at most N workflows of one namespace at once",
            "local engine: at most N workflow processes alive at once, "
            "over all workflows")):
        p.add_argument(f"--{prefix}-{suffix}", type=int, default=None, metavar="N",
                       help=f"{text} (default: unlimited)")


def limit_options(args, prefix: str) -> dict:
    """The limits that were given, as options for :func:`build_engine`."""
    given = {}
    for option, suffix in LIMIT_FLAGS:
        value = getattr(args, f"{prefix}_{suffix}".replace("-", "_"))
        if value is not None:
            given[option] = value
    return given


def check_limit_flags(p: argparse.ArgumentParser, args, prefix: str) -> None:
    for option, value in limit_options(args, prefix).items():
        if value < 1:
            p.error(f"--{prefix}-{option.replace('_', '-')} must be a positive integer")


def open_logs(args, engine_kind: str, server, info=None):
    """The workflow log store of a standalone process: ``<data-dir>/logs``,
    or a temporary directory without ``--data-dir``. None, and ``workflow
    logs: off``, unless the local engine runs here and logs are wanted. What
    an earlier process left is served again, less the runs whose Workflow is
    no longer in ``server``."""
    from ..workflow import logs
    from .registry import WF_API_VERSION, WF_KIND

    info = info or _to_stderr
    if engine_kind != "local" or not args.workflow_logs:
        info("workflow logs: off")
        return None
    caps = {}
    if args.log_max_bytes is not None:
        caps["max_node_bytes"] = args.log_max_bytes
    if args.log_max_total_bytes is not None:
        caps["max_total_bytes"] = args.log_max_total_bytes
    if args.data_dir:
        live = [
            ((wf["metadata"].get("namespace", "")), wf["metadata"]["name"])
            for wf in server.list(WF_API_VERSION, WF_KIND)
        ]
        store = logs.LogStore.open(
            os.path.join(args.data_dir, LOGS_SUBDIR), live=live, **caps)
    else:
        store = logs.LogStore(**caps)
    info(f"workflow logs: {store.describe()}")
    return store


def standalone_schemas(enabled: bool = True):
    """``(schemas, log line)`` for a standalone store: the HealthCheck CRD
    schema, unless ``enabled`` is false or AM_SCHEMA_VALIDATION=0 is set."""
    if not enabled or os.environ.get("AM_SCHEMA_VALIDATION") == "0":
        return None, "schema validation: off"
    schemas = healthcheck_schemas()
    kinds = ", ".join(f"{kind} ({av})" for av, kind in schemas)
    return schemas, f"schema validation: {kinds}"


def read_accepted_tokens(path: str) -> set:
    with open(path, "r") as f:
        tokens = {line.strip() for line in f if line.strip()}
    if not tokens:
        raise SystemExit(f"--token-file {path}: no tokens in file")
    return tokens


def _to_stderr(message: str) -> None:
    print(message, file=sys.stderr, flush=True)


def open_durable_store(data_dir: str, schemas=None, info=_to_stderr, error=_to_stderr):
    """Open the store kept in ``data_dir`` and say what was found; on a
    locked or unreadable directory say the reason and return None — the
    caller exits 1 and never starts an empty store over it."""
    from . import MemoryApiServer  # looked up late, see open_store
    from .persist import StoreError

    try:
        server = MemoryApiServer.open(data_dir, schemas=schemas)
    except (StoreError, OSError) as e:
        error(f"cannot open data directory: {e}")
        return None
    info(f"data directory {server.data_dir}: loaded {len(server)} objects, "
         f"resourceVersion {server.resource_version()}")
    return server


def open_store(data_dir, schema_validation: bool = True,
               info=_to_stderr, error=_to_stderr):
    """The store of a standalone process, for both entry points (this module
    and ``cmd.main --backend memory``): says which schemas validate, then
    opens ``data_dir`` — or, without one, starts an empty store. Returns None
    when the directory cannot be used. ``info``/``error`` take one message."""
    # the class is looked up on the package when called, not bound at import:
    # tests substitute a recording subclass there
    from . import MemoryApiServer

    schemas, schema_line = standalone_schemas(schema_validation)
    info(schema_line)
    if data_dir:
        return open_durable_store(data_dir, schemas, info, error)
    return MemoryApiServer(schemas=schemas)


def build_engine(kind: str, client, data_dir, logs=None, **options):
    """The workflow engine that runs inside a standalone process, or None for
    ``"none"``. Over a data directory it recovers what the last process left
    (a workflow found Running is failed as interrupted, never run again).
    ``logs`` is the local engine's log store."""
    from ..workflow import LocalWorkflowEngine, ScriptedWorkflowEngine

    if kind == "none":
        return None
    if kind == "local":
        options["logs"] = logs
    cls = {"local": LocalWorkflowEngine, "scripted-bench": ScriptedWorkflowEngine}[kind]
    return cls(client, recover=bool(data_dir), **options)


def stop_on_signals(stop: asyncio.Event) -> asyncio.Event:
    """Have SIGINT and SIGTERM set ``stop`` on the running loop."""
    loop = asyncio.get_running_loop()
    for sig in (signal.SIGINT, signal.SIGTERM):
        try:
            loop.add_signal_handler(sig, stop.set)
        except (NotImplementedError, RuntimeError):  # pragma: no cover - non-unix
            pass
    return stop


async def amain(args) -> int:
    from .client import MemoryClient

    server = open_store(args.data_dir, args.schema_validation)
    if server is None:
        return 1
    accepted = read_accepted_tokens(args.token_file) if args.token_file else None
    logs = open_logs(args, args.engine, server)
    frontend = ApiServerFrontend(server, args.host, args.port,
                                 accepted_tokens=accepted, logs=logs)
    await frontend.start()

    options = {"ttl_seconds": args.engine_ttl, **limit_options(args, "engine")}
    if args.engine == "scripted-bench":
        options.update(policy=bench_policy(args.remedy_frac), delay=args.engine_delay)
    engine = build_engine(args.engine, MemoryClient(server), args.data_dir,
                          logs=logs, **options)
    if engine is not None:
        await engine.start()

    print("READY " + json.dumps({"url": frontend.url, "port": frontend.port}),
          flush=True)
    await stop_on_signals(asyncio.Event()).wait()

    if engine is not None:
        await engine.stop()
    await frontend.stop()
    if logs is not None:
        logs.close()
    server.close()
    return 0


def main(argv=None) -> int:
    return asyncio.run(amain(parse_args(argv)))


if __name__ == "__main__":
    sys.exit(main())

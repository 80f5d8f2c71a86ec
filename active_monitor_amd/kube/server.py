"""HTTP apiserver frontend: serves the in-memory store over the Kubernetes
REST API.

This is the framework's envtest-style local apiserver: the HttpClient (and
kubectl-shaped tooling) can talk to a MemoryApiServer over real HTTP —
typed paths, status subresource, label selectors, resourceVersion watch
resume with real 410 Gone semantics, and streaming watches (JSON lines).

Implementation note: the server is a hand-rolled asyncio HTTP/1.1 protocol
(keep-alive, Content-Length framing; watch streams use Connection: close
framing) rather than an aiohttp web app — at fleet rates the apiserver
process is request-bound and the web-framework dispatch chain cost ~200µs
of the ~300µs per request. The wire format is unchanged; the full HTTP test
suite (CRUD, discovery, error paths, watch conformance, kubectl-ability)
runs against this server.
"""
from __future__ import annotations

import asyncio
import hmac
import logging
from typing import List, Optional, Set, Tuple

from ..utils import wirecodec
from ..utils.wirecodec import EXPECT_CONTINUE, WANT_TABLE
from .errors import (
    ApiError,
    BadRequestError,
    ExpiredError,
    InvalidError,
    NotFoundError,
    UnauthorizedError,
)
from .memory import (
    MemoryApiServer,
    fields_match,
    labels_match,
    object_rv,
    parse_field_selector,
    parse_label_selector,
)
from .registry import WF_API_VERSION, WF_KIND

log = logging.getLogger("active_monitor_amd.kube.server")

_REASONS = {
    200: "OK", 201: "Created", 400: "Bad Request", 401: "Unauthorized",
    404: "Not Found",
    405: "Method Not Allowed", 409: "Conflict", 410: "Gone",
    422: "Unprocessable Entity", 500: "Internal Server Error",
}


#: status line + Content-Type of a JSON response, per status code; the
#: Content-Length line and the payload are appended by wirecodec.frame
_JSON_PREFIX = {
    code: (f"HTTP/1.1 {code} {reason}\r\n"
           f"Content-Type: application/json\r\n").encode("latin-1")
    for code, reason in _REASONS.items()
}
_UNAUTHORIZED_PREFIX = (
    b"HTTP/1.1 401 Unauthorized\r\nContent-Type: application/json\r\n"
    b"WWW-Authenticate: Bearer\r\n"
)


def _json_prefix(status: int) -> bytes:
    prefix = _JSON_PREFIX.get(status)
    if prefix is None:  # a code without a reason phrase of its own
        prefix = _JSON_PREFIX[status] = (
            f"HTTP/1.1 {status} OK\r\n"
            f"Content-Type: application/json\r\n"
        ).encode("latin-1")
    return prefix


def _status_body(err: ApiError) -> dict:
    body = {
        "kind": "Status",
        "apiVersion": "v1",
        "status": "Failure",
        "message": err.message,
        "reason": err.reason,
        "code": err.code,
    }
    details = getattr(err, "details", None)
    if details:  # a schema rejection: name, group, kind and the causes
        body["details"] = details
    return body


def _failure(err: ApiError, status: Optional[int] = None) -> Tuple[int, dict]:
    """``(status, Status body)`` of a refusal; the HTTP status is the error's
    own code unless the route gives it another."""
    return status or err.code, _status_body(err)


def _route(path: str) -> Optional[Tuple[str, str, str, str, str]]:
    """``(api_version, namespace, plural, name, subresource)`` of a resource
    path, ``""`` for what it does not name; None for any other path.

        /api/v1/...  or  /apis/{group}/{version}/...  followed by
        {plural}[/{name}[/{subresource}]]
        namespaces/{ns}/{plural}[/{name}[/{subresource}]]

    ``namespaces/{ns}`` is a namespace prefix only with a plural after it:
    /api/v1/namespaces[/{name}] is the Namespace resource itself."""
    segs = [seg for seg in path.split("/") if seg]
    if len(segs) >= 2 and segs[0] == "api":
        api_version, parts = segs[1], segs[2:]
    elif len(segs) >= 3 and segs[0] == "apis":
        api_version, parts = f"{segs[1]}/{segs[2]}", segs[3:]
    else:
        return None
    namespace = ""
    if len(parts) >= 3 and parts[0] == "namespaces":
        namespace, parts = parts[1], parts[2:]
    plural, name, subresource = (parts + ["", "", ""])[:3]
    return api_version, namespace, plural, name, subresource


class _MethodNotAllowed(ApiError):
    code = 405
    reason = "MethodNotAllowed"


class _Warned:
    """A response object that goes out with ``Warning`` headers: what a write
    returns when fields were pruned under ``fieldValidation=Warn``. Every
    other JSON response is a plain dict, and the writer tells the two apart
    by the one type test it made before there were warnings."""

    __slots__ = ("obj", "paths")

    def __init__(self, obj: dict, paths: list):
        self.obj = obj
        self.paths = paths

    @staticmethod
    def _header_text(path: str) -> str:
        """``path`` as it may stand in a quoted header value. Its keys are
        the client's own JSON keys, so anything but printable ASCII — CR and
        LF above all — goes out percent-encoded (as does ``%`` itself), and
        backslash and double quote are backslash-escaped."""
        out = []
        for byte in path.encode("utf-8", "surrogatepass"):
            if byte in (0x22, 0x5C):
                out.append("\\" + chr(byte))
            elif 0x20 <= byte <= 0x7E and byte != 0x25:
                out.append(chr(byte))
            else:
                out.append(f"%{byte:02X}")
        return "".join(out)

    def prefix(self, status: int) -> bytes:
        lines = "".join(
            f'Warning: 299 - "unknown field \\"{self._header_text(p)}\\""\r\n'
            for p in self.paths
        )
        return _json_prefix(status) + lines.encode("ascii")


#: served without credentials, as on a real apiserver
_OPEN_PATHS = frozenset({
    "/healthz", "/livez", "/readyz", "/version", "/version/",
})


class ApiServerFrontend:
    def __init__(self, server: MemoryApiServer, host: str = "127.0.0.1", port: int = 0,
                 accepted_tokens: Optional[Set[str]] = None, logs=None):
        self.server = server
        #: the workflow.logs.LogStore behind the Workflows' ``log``
        #: subresource, or None: every such request is then a 404
        self.logs = logs
        self.host = host
        self.port = port
        #: None = open to everyone. A set = bearer-token authn: every request
        #: but the health probes and /version must carry one of these tokens.
        #: The set is consulted per request and may be changed while serving
        #: (that is how tests rotate credentials).
        self.accepted_tokens = accepted_tokens
        #: requests answered 401
        self.unauthorized_count = 0
        self._srv: Optional[asyncio.AbstractServer] = None
        self._live_subs: list = []

    @property
    def url(self) -> str:
        return f"http://{self.host}:{self.port}"

    async def start(self) -> None:
        self._srv = await asyncio.start_server(self._handle_conn, self.host, self.port)
        if self.port == 0:
            self.port = self._srv.sockets[0].getsockname()[1]

    async def stop(self) -> None:
        self.kick_watches()
        if self._srv is not None:
            self._srv.close()
            try:
                await asyncio.wait_for(self._srv.wait_closed(), 2.0)
            except asyncio.TimeoutError:
                pass

    def kick_watches(self) -> None:
        """Terminate every open watch stream and every followed log (server
        stays up). Clients see a clean end-of-stream and reconnect with their
        resourceVersion — the fault-injection hook for RV-expiry/resume
        conformance tests."""
        for sub in list(self._live_subs):
            sub.close()

    # -- authn --------------------------------------------------------------

    def _authorized(self, path: str, authorization: bytes) -> bool:
        if path in _OPEN_PATHS:
            return True
        ok = False
        scheme, _, presented = authorization.partition(b" ")
        if scheme.lower() == b"bearer":
            presented = presented.strip()
            # every candidate is compared, in constant time each
            for tok in list(self.accepted_tokens or ()):
                if hmac.compare_digest(presented, tok.encode("utf-8")):
                    ok = True
        if not ok:
            self.unauthorized_count += 1
        return ok

    @staticmethod
    def _unauthorized_response() -> bytes:
        return wirecodec.frame(
            _UNAUTHORIZED_PREFIX, _status_body(UnauthorizedError("Unauthorized"))
        )

    # -- HTTP protocol ------------------------------------------------------

    async def _handle_conn(self, reader: asyncio.StreamReader,
                           writer: asyncio.StreamWriter) -> None:
        try:
            while True:
                # one read for the whole head (it ends at CRLF CRLF) and one
                # parse of it: utils/wirecodec.py
                head = await reader.readuntil(b"\r\n\r\n")
                parsed = wirecodec.parse_request_head(head)
                if parsed is None:
                    return
                (method, path, query, content_length, content_type, flags,
                 authorization) = parsed
                if flags & EXPECT_CONTINUE:
                    writer.write(b"HTTP/1.1 100 Continue\r\n\r\n")
                    await writer.drain()
                body = await reader.readexactly(content_length) if content_length else b""

                if (self.accepted_tokens is not None
                        and not self._authorized(path, authorization)):
                    # the body was consumed above, so keep-alive survives
                    writer.write(self._unauthorized_response())
                    await writer.drain()
                    continue
                if query.get("watch") in ("true", "1"):
                    await self._serve_watch(writer, path, query)
                    return  # watch streams own the connection
                if path.endswith("/log") and self._is_log_route(path):
                    if await self._serve_log(writer, method, path, query):
                        return  # so does a followed log
                    continue
                status, obj = self._serve_unary(method, path, query, body,
                                                content_type)
                if (flags & WANT_TABLE and method == "GET" and status == 200
                        and isinstance(obj, dict)):
                    obj = self._to_table(obj)
                if type(obj) is dict or not isinstance(obj, (_Warned, str)):
                    writer.write(wirecodec.frame(_json_prefix(status), obj))
                elif isinstance(obj, _Warned):
                    writer.write(wirecodec.frame(obj.prefix(status), obj.obj))
                else:  # health probes are plain text
                    payload = obj.encode()
                    writer.write(
                        (
                            f"HTTP/1.1 {status} {_REASONS.get(status, 'OK')}\r\n"
                            f"Content-Type: text/plain\r\n"
                            f"Content-Length: {len(payload)}\r\n\r\n"
                        ).encode("latin-1") + payload
                    )
                await writer.drain()
        except (ConnectionError, asyncio.IncompleteReadError,
                asyncio.LimitOverrunError, asyncio.CancelledError):
            # LimitOverrunError: a head longer than the reader's limit
            pass
        except Exception:  # defensive: never kill the accept loop
            log.exception("frontend connection handler failed")
        finally:
            try:
                writer.close()
            except Exception:
                pass

    # -- routing ------------------------------------------------------------

    def _serve_unary(self, method: str, path: str, query: dict,
                     body: bytes, content_type: str = "") -> Tuple[int, Optional[dict]]:
        # discovery endpoints (enough for kubectl --server=<url>)
        if path in ("/api", "/api/"):
            return 200, {"kind": "APIVersions", "versions": ["v1"]}
        if path in ("/apis", "/apis/"):
            return 200, self._discovery_apis()
        if path in ("/version", "/version/"):
            from .. import __version__

            return 200, {
                "major": "1", "minor": "33",
                "gitVersion": f"v1.33.0-active-monitor-amd+{__version__}",
            }
        if path in ("/healthz", "/readyz", "/livez"):
            return 200, "ok"  # apiserver health probes (kubectl checks these)
        route = _route(path)
        if route is None:
            return _failure(ApiError(f"the server could not find {path}"), 404)
        if not route[2]:  # /api/v1 or /apis/g/v → resource discovery
            return 200, self._resource_list(route[0])
        return self._dispatch(method, route, query, body, content_type)

    def _discovery_apis(self) -> dict:
        groups_map: dict = {}
        for (av, _), info in self.server.registry.kinds():
            if "/" in av:
                g, v = av.split("/", 1)
                groups_map.setdefault(g, set()).add(v)
        groups = []
        for g, versions in sorted(groups_map.items()):
            gv = sorted({f"{g}/{v}" for v in versions})
            groups.append({
                "name": g,
                "versions": [{"groupVersion": x, "version": x.split("/", 1)[1]} for x in gv],
                "preferredVersion": {"groupVersion": gv[0], "version": gv[0].split("/", 1)[1]},
            })
        return {"kind": "APIGroupList", "apiVersion": "v1", "groups": groups}

    def _resource_list(self, api_version: str) -> dict:
        resources = []
        for (av, kind), info in sorted(self.server.registry.kinds()):
            if av != api_version:
                continue
            resources.append({
                "name": info.plural,
                "singularName": kind.lower(),
                "namespaced": info.namespaced,
                "kind": kind,
                "verbs": ["create", "delete", "get", "list", "patch", "update", "watch"],
            })
            if (av, kind) == (WF_API_VERSION, WF_KIND):
                resources.append({
                    "name": f"{info.plural}/log",
                    "singularName": "",
                    "namespaced": True,
                    "kind": kind,
                    "verbs": ["get"],
                })
            if (av, kind) == ("activemonitor.keikoproj.io/v1alpha1", "HealthCheck"):
                resources[-1]["shortNames"] = ["hc", "hcs"]
                resources.append({
                    "name": f"{info.plural}/status",
                    "singularName": "",
                    "namespaced": True,
                    "kind": kind,
                    "verbs": ["get", "update", "patch"],
                })
        return {"kind": "APIResourceList", "apiVersion": "v1",
                "groupVersion": api_version, "resources": resources}

    def _dispatch(self, method: str, route: Tuple[str, str, str, str, str],
                  query: dict, body: bytes,
                  content_type: str = "") -> Tuple[int, Optional[dict]]:
        api_version, namespace, plural, name, subresource = route
        try:
            kind = self.server.registry.by_plural(api_version, plural).kind
        except KeyError:
            return _failure(ApiError(f"unknown resource {plural}"), 404)

        try:
            if method == "GET" and not name:
                items = self.server.list(
                    api_version, kind, namespace or None, query.get("labelSelector"),
                    field_selector=query.get("fieldSelector"),
                )
                return 200, {
                    "apiVersion": api_version, "kind": kind + "List",
                    "metadata": {"resourceVersion": self.server.resource_version()},
                    "items": items,
                }
            if method == "GET":
                return 200, self.server.get(api_version, kind, namespace, name)
            if method == "POST":
                obj = self._parse_body(body)
                meta = obj.setdefault("metadata", {})
                if namespace and not meta.get("namespace"):
                    meta["namespace"] = namespace
                return self._write(201, query, self.server.create, obj)
            if method == "PUT":
                obj = self._parse_body(body)
                if subresource == "status":
                    return self._write(200, query, self.server.update_status, obj)
                return self._write(200, query, self.server.update, obj)
            if method == "DELETE" and not name:
                # deletecollection (kubectl delete --all / -l selector)
                victims = self.server.list(
                    api_version, kind, namespace or None, query.get("labelSelector")
                )
                for obj in victims:
                    m = obj.get("metadata") or {}
                    try:
                        self.server.delete(api_version, kind,
                                           m.get("namespace", ""), m.get("name", ""))
                    except ApiError:
                        pass  # raced another delete / cascade GC
                return 200, {"apiVersion": api_version, "kind": kind + "List",
                             "items": victims}
            if method == "DELETE":
                self.server.delete(api_version, kind, namespace, name)
                return 200, {"kind": "Status", "status": "Success"}
            if method == "PATCH":
                ct = content_type.split(";")[0].strip().lower()
                if ct == "application/json-patch+json":
                    # RFC 6902 op lists are not supported; kubectl defaults
                    # to strategic/merge for CRDs anyway
                    return _failure(
                        InvalidError("json-patch is not supported; use merge-patch"),
                        415)
                if ct == "application/apply-patch+yaml":
                    import yaml as _yaml

                    try:
                        patch_obj = _yaml.safe_load(body)
                    except _yaml.YAMLError:
                        raise InvalidError("request body is not valid JSON")
                    if not isinstance(patch_obj, dict):
                        raise InvalidError("request body is not valid JSON")
                    upsert = True  # server-side apply creates when absent
                else:  # merge-patch / strategic-merge-patch
                    patch_obj = self._parse_body(body)
                    upsert = False
                return self._write(
                    200, query, self.server.patch,
                    api_version, kind, namespace, name, patch_obj,
                    subresource=subresource, upsert=upsert,
                )
        except InvalidError as e:
            return _failure(
                e, 400 if e.message == "request body is not valid JSON" else None)
        except ApiError as e:
            return _failure(e)
        return _failure(ApiError(f"unsupported method {method}"), 405)

    @staticmethod
    def _write(status: int, query: dict, write, *args, **kwargs):
        """Run one store write under the request's ``fieldValidation`` (absent
        means Warn, as in Kubernetes 1.27 and later). Pruned paths come back
        in ``warnings`` only under Warn, with a schema installed for the
        kind; the usual answer is the plain object."""
        mode = query.get("fieldValidation")
        if mode is None:
            mode = "Warn"  # any other value is checked by the store
        warnings: list = []
        out = write(*args, field_validation=mode, warnings=warnings, **kwargs)
        if warnings:
            return status, _Warned(out, warnings)
        return status, out

    @staticmethod
    def _parse_body(body: bytes) -> dict:
        try:
            obj = wirecodec.loads_strict(body)
            if not isinstance(obj, dict):
                raise ValueError
            return obj
        except (ValueError, TypeError):
            raise InvalidError("request body is not valid JSON")

    # -- Table responses (kubectl get) --------------------------------------

    #: printcolumns per kind, mirroring the CRD's additionalPrinterColumns
    #: (api/crd.py; reference healthcheck_types.go:71-76 printcolumn markers)
    _PRINTCOLUMNS = {
        "HealthCheck": [
            ("LATEST STATUS", "string", ("status", "status")),
            ("SUCCESS CNT  ", "string", ("status", "successCount")),
            ("FAIL CNT", "string", ("status", "failedCount")),
            ("REMEDY SUCCESS CNT  ", "string", ("status", "remedySuccessCount")),
            ("REMEDY FAIL CNT", "string", ("status", "remedyFailedCount")),
            ("Age", "date", ("metadata", "creationTimestamp")),
        ],
        "Workflow": [
            ("Status", "string", ("status", "phase")),
            ("Age", "date", ("metadata", "creationTimestamp")),
        ],
    }
    _DEFAULT_COLUMNS = [("Age", "date", ("metadata", "creationTimestamp"))]

    def _to_table(self, obj: dict) -> dict:
        """meta.k8s.io/v1 Table transform — what kubectl get requests via
        Accept: ...;as=Table. Rows carry PartialObjectMetadata objects."""
        if obj.get("kind", "").endswith("List"):
            items = obj.get("items", [])
            kind = obj.get("kind", "")[:-4]
            meta = obj.get("metadata", {})
        elif obj.get("kind") and obj.get("metadata") is not None:
            items = [obj]
            kind = obj.get("kind", "")
            meta = {}
        else:
            return obj  # Status bodies etc. pass through
        cols = self._PRINTCOLUMNS.get(kind, self._DEFAULT_COLUMNS)
        defs = [{"name": "Name", "type": "string", "format": "name"}] + [
            {"name": n, "type": t} for (n, t, _) in cols
        ]
        rows = []
        for it in items:
            cells = [((it.get("metadata") or {}).get("name", ""))]
            for _, _, path in cols:
                cur = it
                for seg in path:
                    cur = cur.get(seg) if isinstance(cur, dict) else None
                    if cur is None:
                        break
                cells.append("" if cur is None else cur)
            rows.append({
                "cells": cells,
                "object": {
                    "kind": "PartialObjectMetadata",
                    "apiVersion": "meta.k8s.io/v1",
                    "metadata": it.get("metadata", {}),
                },
            })
        return {
            "kind": "Table",
            "apiVersion": "meta.k8s.io/v1",
            "metadata": meta,
            "columnDefinitions": defs,
            "rows": rows,
        }

    # -- workflow logs ------------------------------------------------------

    def _is_log_route(self, path: str) -> bool:
        route = _route(path)
        if route is None or route[4] != "log" or route[0] != WF_API_VERSION:
            return False
        try:
            return self.server.registry.by_plural(route[0], route[2]).kind == WF_KIND
        except KeyError:
            return False

    async def _serve_log(self, writer: asyncio.StreamWriter, method: str,
                         path: str, query: dict) -> bool:
        """``GET .../workflows/{name}/log``: what the workflow's leaves
        printed, as text/plain. With ``follow=true`` the response is chunked
        and ends when the run does (or with kick_watches/stop); True is then
        returned and the connection is not used again."""
        _, namespace, _, name, _ = _route(path)
        try:
            if method != "GET":
                raise _MethodNotAllowed(f"unsupported method {method}")
            numbers = {}
            for key in ("tailLines", "limitBytes"):
                if query.get(key) is not None:
                    try:
                        numbers[key] = int(query[key])
                    except ValueError:
                        raise BadRequestError(
                            f"{key} must be an integer, not {query[key]!r}")
            # NotFound: the Workflow does not exist
            self.server.get(WF_API_VERSION, WF_KIND, namespace, name)
            if self.logs is None:
                raise NotFoundError(
                    f"workflow {namespace}/{name} has no logs: this server "
                    "keeps no workflow logs")
            if not self.logs.has_run(namespace, name):
                raise NotFoundError(
                    f"workflow {namespace}/{name} has no logs: it was not run "
                    "by the local executor, or its logs were dropped for the "
                    "total size cap")
            follow = query.get("follow") in ("true", "1")
            stream = self.logs.read(
                namespace, name, node=query.get("node") or None, follow=follow,
                tail_lines=numbers.get("tailLines"),
                limit_bytes=numbers.get("limitBytes"),
                prefix=query.get("prefix") in ("true", "1"),
            )  # NotFound: the node is unknown
        except ApiError as e:
            status, body = _failure(e)
            writer.write(wirecodec.frame(_json_prefix(status), body))
            await writer.drain()
            return False
        if not follow:
            payload = b"".join([chunk async for chunk in stream])
            writer.write(
                b"HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\n"
                b"Content-Length: %d\r\n\r\n" % len(payload) + payload
            )
            await writer.drain()
            return False
        self._live_subs.append(stream)
        try:
            writer.write(
                b"HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\n"
                b"Transfer-Encoding: chunked\r\nConnection: close\r\n\r\n"
            )
            await writer.drain()
            async for chunk in stream:
                writer.write(b"%x\r\n%s\r\n" % (len(chunk), chunk))
                await writer.drain()
            writer.write(b"0\r\n\r\n")
            await writer.drain()
        except (ConnectionError, asyncio.CancelledError):
            pass
        finally:
            await stream.aclose()
            if stream in self._live_subs:
                self._live_subs.remove(stream)
        return True

    # -- watch --------------------------------------------------------------

    @staticmethod
    async def _refuse_watch(writer: asyncio.StreamWriter, err: ApiError,
                            status: int) -> None:
        status, body = _failure(err, status)
        writer.write(wirecodec.frame(_json_prefix(status), body))
        await writer.drain()

    async def _serve_watch(self, writer: asyncio.StreamWriter, path: str,
                           query: dict) -> None:
        """Watch with real resourceVersion semantics: a resume rv replays the
        retained event history after that rv (410 Gone when it predates the
        window — the client must re-list); no rv replays current state as
        ADDED. The live subscription is opened before the replay snapshot is
        taken and overlap is deduplicated by rv, so no event can fall between
        replay and stream. Framing: Connection: close (read-until-EOF)."""
        route = _route(path)
        if route is None:
            return await self._refuse_watch(
                writer, ApiError(f"the server could not find {path}"), 404)
        api_version, namespace, plural = route[:3]  # a name is not looked at
        namespace = namespace or None
        try:
            kind = self.server.registry.by_plural(api_version, plural).kind
        except KeyError:
            # a watch names all that follows the version, not the plural alone
            tail = [seg for seg in path.split("/") if seg][api_version.count("/") + 2:]
            return await self._refuse_watch(
                writer, ApiError("unknown resource " + "/".join(tail)), 404)

        rv_param = query.get("resourceVersion")
        # a selector that does not parse leaves the watch unfiltered
        selector: dict = {}
        fields: List[tuple] = []
        try:
            selector = parse_label_selector(query.get("labelSelector"))
        except ApiError:
            pass
        try:
            fields = parse_field_selector(query.get("fieldSelector"))
        except ApiError:
            pass
        sub = self.server.watch(api_version, kind, namespace)
        self._live_subs.append(sub)
        try:
            replay = []
            last_rv = 0
            if rv_param:
                try:
                    replay = self.server.events_since(api_version, kind, namespace, rv_param)
                except ExpiredError as e:
                    return await self._refuse_watch(writer, e, 410)
                try:
                    last_rv = int(rv_param)
                except ValueError:
                    last_rv = 0
            else:
                last_rv = int(self.server.resource_version())
                replay = [
                    {"type": "ADDED", "object": obj}
                    for obj in self.server.list(api_version, kind, namespace)
                ]
            writer.write(
                b"HTTP/1.1 200 OK\r\n"
                b"Content-Type: application/json;stream=watch\r\n"
                b"Connection: close\r\n\r\n"
            )

            def _matches(obj: dict) -> bool:
                if selector and not labels_match(obj, selector):
                    return False
                if fields and not fields_match(obj, fields):
                    return False
                return True

            for ev in replay:
                last_rv = max(last_rv, object_rv(ev.get("object") or {}))
                if not _matches(ev.get("object") or {}):
                    continue
                writer.write(wirecodec.dumpb(ev) + b"\n")
            await writer.drain()
            # watch budget: like a real apiserver, an expiring watch ends
            # with a clean stream close and the client resumes from its rv
            # (kubectl sends timeoutSeconds by default; reflectors resume).
            # Implemented as one timer that closes the subscription — the
            # event loop stays free of per-event wait_for wrappers.
            budget_handle = None
            if query.get("timeoutSeconds"):
                try:
                    budget_handle = asyncio.get_running_loop().call_later(
                        float(query["timeoutSeconds"]), sub.close
                    )
                except ValueError:
                    pass
            try:
                async for ev in sub:
                    if object_rv(ev.get("object") or {}) <= last_rv:
                        continue  # already covered by the replay snapshot
                    if not _matches(ev.get("object") or {}):
                        continue
                    writer.write(wirecodec.dumpb(ev) + b"\n")
                    await writer.drain()
            finally:
                if budget_handle is not None:
                    budget_handle.cancel()
        except (ConnectionError, asyncio.CancelledError):
            pass
        finally:
            sub.close()
            if sub in self._live_subs:
                self._live_subs.remove(sub)

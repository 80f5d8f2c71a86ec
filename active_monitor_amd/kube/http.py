"""HTTP Kubernetes client — the real-apiserver backend.

Implements the same async KubeClient facade the reconciler programs against
(kube/client.py), over the Kubernetes REST API: typed/namespaced paths,
status subresource writes, label selectors, and streaming watches with
reconnect — the role client-go's typed + dynamic clients play in the
reference (healthcheck_controller.go:133-137).
"""
from __future__ import annotations

import asyncio
import json
import logging
import re
import ssl
import time
from collections import deque
from typing import Any, AsyncIterator, Dict, List, Optional, Tuple
from urllib.parse import urlencode, urlsplit

import aiohttp

from ..utils import wirecodec
from .auth import Credential, CredentialSource
from .errors import (
    AlreadyExistsError,
    ApiError,
    BadRequestError,
    ConflictError,
    InvalidError,
    NotFoundError,
    UnauthorizedError,
)
from .registry import DEFAULT_REGISTRY, WF_API_VERSION, WF_KIND, Registry

log = logging.getLogger("active_monitor_amd.kube.http")

Obj = Dict[str, Any]


def _error_for(status: int, raw: bytes) -> ApiError:
    body = raw.decode("utf-8", "replace")
    reason = ""
    message = body
    details = None
    try:
        parsed = json.loads(body)
        reason = parsed.get("reason", "")
        message = parsed.get("message", body)
        details = parsed.get("details")
    except (ValueError, TypeError, AttributeError):
        pass
    if status == 404:
        return NotFoundError(message)
    if status == 401:
        return UnauthorizedError(message)
    if status == 409:
        if reason == "AlreadyExists":
            return AlreadyExistsError(message)
        return ConflictError(message)
    if status == 422:
        if isinstance(details, dict):
            return InvalidError(message, causes=details.get("causes"),
                                details=details)
        return InvalidError(message)
    if status == 400 and reason == "BadRequest":
        return BadRequestError(message)
    err = ApiError(message)
    err.code = status
    return err


_WARNING_HEADER = re.compile(r'^\s*\d{3}\s+\S+\s+"((?:[^"\\]|\\.)*)"')


def _warning_text(header: str) -> str:
    """The warn-text of an RFC 7234 ``Warning`` header value
    (``299 - "text"``), unquoted; the raw value when it is not one."""
    m = _WARNING_HEADER.match(header)
    if m is None:
        return header.strip()
    return re.sub(r"\\(.)", r"\1", m.group(1))


def _fv_params(field_validation: Optional[str]) -> Optional[Dict[str, str]]:
    return {"fieldValidation": field_validation} if field_validation else None


class _Expired(Exception):
    """The watch's resourceVersion is too old (HTTP 410 / ERROR event)."""


class _WatchUnauthorized(Exception):
    """The watch connect was refused with 401 and the client has a
    credential source to ask for a newer credential."""


class HttpSubscription:
    """Streaming watch with automatic reconnect (resourceVersion resume).

    Conformance with client-go's reflector (which the reference inherits via
    controller-runtime, healthcheck_controller.go:133-137):

    - a 410 Gone response or a watch ``ERROR`` event (code 410 or otherwise)
      clears the stored resourceVersion, **re-lists** the collection and
      delivers the list as a *Replace*: first a synthetic ``DELETED`` for
      every object the consumer was told about that the list no longer holds
      (or holds under another uid: deleted and re-created inside the expiry
      window), then a synthetic ``ADDED`` per live object — so consumers
      miss neither the changes nor the deletions that happened inside the
      window — and resumes watching from the list's resourceVersion,
    - ``allowWatchBookmarks`` is requested and BOOKMARK events advance the
      resume point without being delivered,
    - frames are read with an incremental buffer, so a watch event larger
      than aiohttp's 64 KB readline limit cannot wedge the stream.

    For the Replace the subscription remembers what it has delivered, as
    ``(namespace, name) -> uid``: identities only, never objects, so the
    memory is proportional to the number of live objects. The first connect
    carries no resourceVersion and the server replays the current state as
    ``ADDED``, so the map is complete without a list of its own. The last
    state of an object whose deletion was missed is therefore not known, and
    a synthetic ``DELETED`` carries a tombstone instead (client-go's
    ``DeletedFinalStateUnknown``): ``apiVersion``, ``kind`` and a ``metadata``
    of ``namespace``, ``name``, ``uid`` and the list's ``resourceVersion``,
    with a top-level ``"synthetic": true`` beside ``type`` and ``object``.
    Consumers read only ``metadata`` of a ``DELETED`` event's object.
    """

    def __init__(self, client: "HttpClient", api_version: str, kind: str,
                 namespace: Optional[str]):
        self._client = client
        self.api_version = api_version
        self.kind = kind
        self.namespace = namespace
        self._closed = False
        self._resource_version: Optional[str] = None
        self._queue: "asyncio.Queue[Optional[Dict[str, Any]]]" = asyncio.Queue()
        self._task = asyncio.ensure_future(self._pump())
        #: test/telemetry counter: completed re-list recoveries
        self.relists = 0
        #: synthetic DELETED events those re-lists produced
        self.synthetic_deletes = 0
        # what the consumer has been told exists: (namespace, name) -> uid
        self._known: Dict[Tuple[str, str], str] = {}
        # a 401 on connect earns one immediate reconnect with a fresh
        # credential; re-armed by the next connect that is accepted
        self._auth_retry_armed = True

    async def _pump(self) -> None:
        while not self._closed:
            try:
                await self._stream_once()
            except asyncio.CancelledError:
                return
            except _Expired:
                if self._closed:
                    return
                log.warning(
                    "watch resourceVersion expired (%s/%s); re-listing",
                    self.api_version, self.kind,
                )
                self._resource_version = None
                # retried until it succeeds: a connect without a
                # resourceVersion would replay the live objects but, unlike
                # the re-list, could not say which ones are gone
                while not self._closed:
                    try:
                        await self._relist()
                        break
                    except asyncio.CancelledError:
                        return
                    except Exception as e:
                        log.warning("re-list after watch expiry failed: %s", e)
                        await asyncio.sleep(1.0)
            except _WatchUnauthorized as e:
                if self._closed:
                    return
                if self._auth_retry_armed:
                    self._auth_retry_armed = False
                    log.info("watch refused with 401 (%s/%s); reconnecting with "
                             "a fresh credential", self.api_version, self.kind)
                    continue
                log.warning("watch stream error (%s/%s): %s; reconnecting",
                            self.api_version, self.kind, e)
                await asyncio.sleep(1.0)
            except Exception as e:
                if self._closed:
                    return
                log.warning("watch stream error (%s/%s): %s; reconnecting",
                            self.api_version, self.kind, e)
                await asyncio.sleep(1.0)

    async def _relist(self) -> None:
        """Reflector-style recovery: list the collection, deliver it as a
        Replace and resume the watch from the list's resourceVersion. The
        deletions come first — a consumer must drop what it holds for an
        object that was deleted and re-created before it sees the new one —
        then every live object as a synthetic ADDED (consumers treat events
        as level triggers)."""
        path = self._client._collection_path(self.api_version, self.kind, self.namespace)
        out = await self._client._request("GET", path)
        if self._closed:
            return
        rv = (out.get("metadata") or {}).get("resourceVersion")
        if rv:
            self._resource_version = str(rv)
        items = out.get("items", [])
        listed: Dict[Tuple[str, str], str] = {}
        for obj in items:
            meta = obj.get("metadata") or {}
            listed[(meta.get("namespace", ""), meta.get("name", ""))] = meta.get("uid", "")
        for key, uid in self._known.items():
            if listed.get(key) != uid:
                self._queue.put_nowait(self._tombstone(key, uid, rv))
                self.synthetic_deletes += 1
        for obj in items:
            self._queue.put_nowait({"type": "ADDED", "object": obj})
        self._known = listed
        self.relists += 1

    def _tombstone(self, key: Tuple[str, str], uid: str, rv: Any) -> Dict[str, Any]:
        meta: Dict[str, Any] = {"namespace": key[0], "name": key[1], "uid": uid}
        if rv:
            meta["resourceVersion"] = str(rv)
        return {
            "type": "DELETED",
            "object": {"apiVersion": self.api_version, "kind": self.kind,
                       "metadata": meta},
            "synthetic": True,
        }

    #: server-side watch budget (client-go reflectors use 5-10 min): bounds
    #: how long a half-open TCP connection can silently starve the informer
    WATCH_TIMEOUT_SECS = 300

    async def _stream_once(self) -> None:
        params = {"watch": "true", "allowWatchBookmarks": "true",
                  "timeoutSeconds": str(self.WATCH_TIMEOUT_SECS)}
        if self._resource_version:
            params["resourceVersion"] = self._resource_version
        path = self._client._collection_path(self.api_version, self.kind, self.namespace)
        source = self._client._credentials
        cred = await source.get() if source is not None else None
        async with self._client._session.get(
            self._client.base_url + path, params=params,
            headers=self._client._session_auth(cred),
            # sock_read is the client-side safety net behind the server
            # budget: a connection that goes dead-quiet past it is aborted
            # and the reconnect/resume path takes over
            timeout=aiohttp.ClientTimeout(
                total=None, sock_read=self.WATCH_TIMEOUT_SECS + 60
            ),
        ) as resp:
            if resp.status == 410:
                await resp.read()
                raise _Expired()
            if resp.status == 401 and source is not None:
                source.invalidate(cred)
                raise _WatchUnauthorized(_error_for(401, await resp.read()))
            if resp.status >= 400:
                raise _error_for(resp.status, await resp.read())
            self._auth_retry_armed = True
            # incremental framing: newline-delimited JSON without readline's
            # line-length ceiling (a >64 KB Workflow event must not wedge the
            # stream in a reconnect-replay loop)
            buf = bytearray()
            while True:
                chunk = await resp.content.readany()
                if not chunk:
                    return  # server closed the stream; reconnect with RV
                buf.extend(chunk)
                while True:
                    nl = buf.find(b"\n")
                    if nl < 0:
                        break
                    line = bytes(buf[:nl]).strip()
                    del buf[: nl + 1]
                    if not line:
                        continue
                    self._handle_event(wirecodec.loads_strict(line))
                    if self._closed:
                        return

    def _handle_event(self, ev: Dict[str, Any]) -> None:
        etype = ev.get("type")
        obj = ev.get("object") or {}
        if etype == "ERROR":
            # a watch ERROR carries a metav1.Status; 410 (or anything else —
            # the stream is unusable either way) triggers re-list recovery
            raise _Expired()
        meta = obj.get("metadata") or {}
        rv = meta.get("resourceVersion")
        if rv:
            self._resource_version = str(rv)
        if etype == "BOOKMARK":
            return  # resume-point advance only, never delivered
        if etype == "DELETED":
            self._known.pop((meta.get("namespace", ""), meta.get("name", "")), None)
        elif etype in ("ADDED", "MODIFIED"):
            self._known[(meta.get("namespace", ""), meta.get("name", ""))] = meta.get("uid", "")
        else:
            return
        self._queue.put_nowait({"type": etype, "object": obj})

    def close(self) -> None:
        self._closed = True
        self._task.cancel()
        self._queue.put_nowait(None)

    def __aiter__(self) -> AsyncIterator[Dict[str, Any]]:
        return self

    async def __anext__(self) -> Dict[str, Any]:
        ev = await self._queue.get()
        if ev is None:
            raise StopAsyncIteration
        return ev


class _TokenBucket:
    """Client-side request rate limiter (client-go flowcontrol equivalent —
    the reference inherits controller-runtime's default 20 QPS / burst 30).
    Waiters are serialized, so throttled requests drain in FIFO order."""

    def __init__(self, qps: float, burst: int):
        self.qps = qps
        self.burst = float(burst)
        self.tokens = float(burst)
        self.last = time.monotonic()
        self._lock = asyncio.Lock()

    async def acquire(self) -> None:
        if self.qps <= 0:
            return
        async with self._lock:
            now = time.monotonic()
            self.tokens = min(self.burst, self.tokens + (now - self.last) * self.qps)
            self.last = now
            if self.tokens >= 1.0:
                self.tokens -= 1.0
                return
            wait = (1.0 - self.tokens) / self.qps
            self.tokens = 0.0
            await asyncio.sleep(wait)
            self.last = time.monotonic()


class _ConnPool:
    """Persistent plain-HTTP/1.1 connections for the unary hot path.

    aiohttp's client spends ~100µs of framework machinery per request
    (middlewares, tracing, CIMultiDict headers, timer contexts); at fleet
    rates the controller loop is request-bound, so the ~5 unary calls per
    reconcile cycle go over raw asyncio streams with keep-alive instead.
    Watches (streaming) and HTTPS targets stay on aiohttp."""

    def __init__(self, host: str, port: int, max_conns: int = 32):
        self.host = host
        self.port = port
        self.max_conns = max_conns
        self._free: List[Tuple[asyncio.StreamReader, asyncio.StreamWriter]] = []
        self._count = 0
        self._waiters: "deque[asyncio.Future]" = deque()
        self._closed = False

    async def _acquire(self):
        while True:
            while self._free:
                reader, writer = self._free.pop()
                if writer.is_closing():
                    self._count -= 1
                    continue
                return reader, writer
            if self._count < self.max_conns:
                self._count += 1
                try:
                    return await asyncio.open_connection(self.host, self.port)
                except Exception:
                    self._count -= 1
                    raise
            fut = asyncio.get_running_loop().create_future()
            self._waiters.append(fut)
            await fut

    def _release(self, conn, reusable: bool) -> None:
        if reusable and not self._closed and not conn[1].is_closing():
            self._free.append(conn)
        else:
            self._count -= 1
            try:
                conn[1].close()
            except Exception:
                pass
        while self._waiters:
            fut = self._waiters.popleft()
            if not fut.done():
                fut.set_result(None)
                break

    async def request(self, method: str, target: str, headers: str,
                      body: Optional[bytes]) -> Tuple[int, bytes]:
        head = (
            f"{method} {target} HTTP/1.1\r\nHost: {self.host}:{self.port}\r\n"
            f"{headers}Content-Length: {len(body) if body else 0}\r\n\r\n"
        ).encode("latin-1")
        return await self._roundtrip(head + body if body else head)

    async def request_json(self, method: str, target: str, headers: str,
                           obj: Optional[Obj]) -> Tuple[int, bytes]:
        """``request`` with a JSON body (None: no body), head and payload
        framed into one buffer by the wire codec."""
        prefix = (
            f"{method} {target} HTTP/1.1\r\nHost: {self.host}:{self.port}\r\n"
            f"{headers}"
        ).encode("latin-1")
        return await self._roundtrip(wirecodec.frame(prefix, obj))

    async def _roundtrip(self, data: bytes) -> Tuple[int, bytes]:
        conn = await self._acquire()
        reader, writer = conn
        ok = False
        try:
            writer.write(data)
            await writer.drain()

            try:
                head = await reader.readuntil(b"\r\n\r\n")
            except asyncio.IncompleteReadError as e:
                if not e.partial:
                    raise ConnectionResetError("server closed connection") from None
                raise
            status, content_length, chunked, keep_alive = (
                wirecodec.parse_response_head(head)
            )
            if chunked:
                chunks = []
                while True:
                    size_line = await reader.readline()
                    size = int(size_line.strip().split(b";")[0], 16)
                    if size == 0:
                        await reader.readline()  # trailing CRLF
                        break
                    chunks.append(await reader.readexactly(size))
                    await reader.readexactly(2)  # CRLF after each chunk
                payload = b"".join(chunks)
            else:
                payload = await reader.readexactly(content_length) if content_length else b""
            ok = keep_alive
            return status, payload
        finally:
            self._release(conn, ok)

    def close(self) -> None:
        self._closed = True
        for _, writer in self._free:
            try:
                writer.close()
            except Exception:
                pass
        self._free.clear()
        while self._waiters:  # fail queued acquirers instead of hanging them
            fut = self._waiters.popleft()
            if not fut.done():
                fut.set_exception(ConnectionError("connection pool closed"))


class HttpClient:
    def __init__(
        self,
        base_url: str,
        token: Optional[str] = None,
        verify: bool = True,
        ca_cert: Optional[str] = None,
        registry: Registry = DEFAULT_REGISTRY,
        qps: float = 20.0,
        burst: int = 30,
        credentials: Optional[CredentialSource] = None,
    ):
        self.base_url = base_url.rstrip("/")
        self.token = token
        # a credential source supersedes ``token``: the Authorization header
        # is then resolved per request instead of being fixed in start()
        self._credentials = credentials
        self.verify = verify
        self.ca_cert = ca_cert
        self.registry = registry
        #: optional (cert_path, key_path) for client-certificate auth
        self.client_cert: tuple = (None, None)
        self._session: Optional[aiohttp.ClientSession] = None
        # plain-HTTP unary fast path (see _ConnPool); None for https targets
        self._pool: Optional[_ConnPool] = None
        self._pool_headers = ""
        # pool path with a source: the header block rendered for _hdr_cred
        self._hdr_cred: Optional[Credential] = None
        self._hdr_block = ""
        # qps<=0 disables throttling (benchmarks measuring the raw wire)
        self._limiter = _TokenBucket(qps, burst)
        #: unary requests issued (observability/bench; watch streams excluded)
        self.request_count = 0
        #: the latest apiserver warnings (``Warning`` response headers, e.g.
        #: ``unknown field "spec.x"``). Only requests sent with
        #: ``field_validation`` set see response headers and add here.
        self.warnings: "deque[str]" = deque(maxlen=256)

    async def start(self) -> None:
        headers = {"Content-Type": "application/json"}
        if self.token and self._credentials is None:
            headers["Authorization"] = f"Bearer {self.token}"
        ssl_ctx: Any = None
        if self.base_url.startswith("https"):
            if not self.verify:
                ssl_ctx = ssl.create_default_context()
                ssl_ctx.check_hostname = False
                ssl_ctx.verify_mode = ssl.CERT_NONE
            elif self.ca_cert:
                ssl_ctx = ssl.create_default_context(cafile=self.ca_cert)
            cert, key = self.client_cert
            if cert:
                if ssl_ctx is None:
                    ssl_ctx = ssl.create_default_context()
                ssl_ctx.load_cert_chain(cert, key)
        self._session = aiohttp.ClientSession(
            headers=headers, connector=aiohttp.TCPConnector(ssl=ssl_ctx)
        )
        if self.base_url.startswith("http://"):
            parts = urlsplit(self.base_url)
            self._pool = _ConnPool(parts.hostname or "127.0.0.1", parts.port or 80)
            self._pool_headers = "Content-Type: application/json\r\n" + (
                f"Authorization: Bearer {self.token}\r\n"
                if self.token and self._credentials is None else ""
            )

    async def close(self) -> None:
        if self._pool is not None:
            self._pool.close()
        if self._session is not None:
            await self._session.close()

    async def ping(self) -> None:
        """Fail fast when the apiserver is unreachable (used at startup, the
        run()-returns-error-for-invalid-config contract of the reference's
        cmd/main_test.go:35-49)."""
        await self._request("GET", "/version")

    # -- paths --------------------------------------------------------------

    def _collection_path(self, api_version: str, kind: str, namespace: Optional[str]) -> str:
        info = self.registry.by_kind(api_version, kind)
        prefix = f"/api/{api_version}" if "/" not in api_version else f"/apis/{api_version}"
        if info.namespaced and namespace:
            return f"{prefix}/namespaces/{namespace}/{info.plural}"
        return f"{prefix}/{info.plural}"

    def _object_path(self, api_version: str, kind: str, namespace: str, name: str) -> str:
        return f"{self._collection_path(api_version, kind, namespace or None)}/{name}"

    # -- requests -----------------------------------------------------------

    async def _request(self, method: str, path: str, body: Optional[Obj] = None,
                       params: Optional[Dict[str, str]] = None, *,
                       content_type: Optional[str] = None,
                       via_session: bool = False) -> Obj:
        """Every unary request: rate limit, count, credential, send, map an
        error status to its exception, decode. With a credential source a 401
        means the request was not processed, so for any verb: invalidate what
        was used, fetch a fresh credential, send once more (a request of its
        own to the limiter and the counter). The second answer stands,
        whatever it is. A fixed ``token=`` is not retried."""
        if self._session is None:
            raise RuntimeError("HttpClient.start() must be called before requests")
        await self._limiter.acquire()
        self.request_count += 1
        source = self._credentials
        cred = await source.get() if source is not None else None
        status, raw = await self._send(method, path, body, params, cred,
                                       content_type, via_session)
        if status == 401 and source is not None:
            source.invalidate(cred)
            cred = await source.get()
            await self._limiter.acquire()
            self.request_count += 1
            status, raw = await self._send(method, path, body, params, cred,
                                           content_type, via_session)
        if status >= 400:
            raise _error_for(status, raw)
        return wirecodec.loads_lenient(raw) if raw else {}

    def _auth_block(self, cred: Credential) -> str:
        if cred is not self._hdr_cred:
            self._hdr_block = (
                f"{self._pool_headers}Authorization: Bearer {cred.token}\r\n"
            )
            self._hdr_cred = cred
        return self._hdr_block

    @staticmethod
    def _session_auth(cred: Optional[Credential]) -> Dict[str, str]:
        """Per-request headers for the aiohttp session; without a source's
        credential the session's own (a fixed token, or none) stand."""
        return {} if cred is None else {"Authorization": f"Bearer {cred.token}"}

    async def _send(self, method: str, path: str, body: Optional[Obj],
                    params: Optional[Dict[str, str]], cred: Optional[Credential],
                    content_type: Optional[str],
                    via_session: bool) -> Tuple[int, bytes]:
        """One round trip, over the pool, or over the aiohttp session for
        https targets and for ``via_session`` requests: those set their own
        Content-Type and have their ``Warning`` response headers collected."""
        if self._pool is not None and not via_session:
            target = path + ("?" + urlencode(params) if params else "")
            headers = self._pool_headers if cred is None else self._auth_block(cred)
            try:
                return await self._pool.request_json(method, target, headers, body)
            except (ConnectionError, asyncio.IncompleteReadError, OSError):
                # stale keep-alive connection: one clean retry on a fresh one
                return await self._pool.request_json(method, target, headers, body)
        headers = self._session_auth(cred)
        if content_type:
            headers["Content-Type"] = content_type
        async with self._session.request(
            method, self.base_url + path, params=params, headers=headers,
            data=wirecodec.dumpb(body) if body is not None else None,
        ) as resp:
            if via_session:
                for value in resp.headers.getall("Warning", ()):
                    text = _warning_text(value)
                    log.warning("apiserver warning: %s", text)
                    self.warnings.append(text)
            return resp.status, await resp.read()

    async def get(self, api_version: str, kind: str, namespace: str, name: str,
                  snapshot_read: bool = False) -> Obj:
        # snapshot_read is a memory-backend optimization; wire responses are
        # always private copies
        return await self._request("GET", self._object_path(api_version, kind, namespace, name))

    async def list(
        self, api_version: str, kind: str,
        namespace: Optional[str] = None, label_selector: Optional[str] = None,
        snapshot_read: bool = False, field_selector: Optional[str] = None,
    ) -> List[Obj]:
        params = {}
        if label_selector:
            params["labelSelector"] = label_selector
        if field_selector:
            params["fieldSelector"] = field_selector
        out = await self._request(
            "GET", self._collection_path(api_version, kind, namespace), params=params
        )
        return out.get("items", [])

    # ``field_validation`` ("Strict", "Warn" or "Ignore") is sent as the
    # ``fieldValidation`` query parameter. None — what the controller sends —
    # leaves it out (the apiserver then warns) and stays on the pooled path,
    # which does not look at response headers.

    async def create(self, obj: Obj, transfer: bool = False,
                     field_validation: Optional[str] = None) -> Obj:
        # transfer is a memory-backend optimization; ignored on the wire
        meta = obj.get("metadata") or {}
        path = self._collection_path(
            obj.get("apiVersion", ""), obj.get("kind", ""), meta.get("namespace")
        )
        return await self._request("POST", path, obj, _fv_params(field_validation),
                                   via_session=field_validation is not None)

    def _path_of(self, obj: Obj) -> str:
        meta = obj.get("metadata") or {}
        return self._object_path(
            obj.get("apiVersion", ""), obj.get("kind", ""),
            meta.get("namespace", ""), meta.get("name", ""),
        )

    async def update(self, obj: Obj, field_validation: Optional[str] = None) -> Obj:
        return await self._request("PUT", self._path_of(obj), obj,
                                   _fv_params(field_validation),
                                   via_session=field_validation is not None)

    async def update_status(self, obj: Obj,
                            field_validation: Optional[str] = None) -> Obj:
        return await self._request("PUT", self._path_of(obj) + "/status", obj,
                                   _fv_params(field_validation),
                                   via_session=field_validation is not None)

    async def patch(self, api_version: str, kind: str, namespace: str, name: str,
                    patch: Obj, subresource: str = "",
                    field_validation: Optional[str] = None) -> Obj:
        """JSON merge-patch (kubectl patch semantics). Not on the reconcile
        hot path — goes through the full aiohttp session for header control."""
        path = self._object_path(api_version, kind, namespace, name)
        if subresource:
            path += f"/{subresource}"
        return await self._request("PATCH", path, patch, _fv_params(field_validation),
                                   content_type="application/merge-patch+json",
                                   via_session=True)

    async def delete(self, api_version: str, kind: str, namespace: str, name: str) -> None:
        await self._request("DELETE", self._object_path(api_version, kind, namespace, name))

    async def logs(self, namespace: str, name: str, node: Optional[str] = None,
                   follow: bool = False, tail_lines: Optional[int] = None,
                   limit_bytes: Optional[int] = None,
                   prefix: bool = False) -> AsyncIterator[bytes]:
        """The ``log`` subresource of a Workflow (a standalone apiserver's
        stand-in for the logs of the workflow's pods), as it arrives. With
        ``follow`` it ends when the server ends it: the run has finished.
        Credentials as for every request, with one refresh-and-retry on 401;
        a stream that breaks is not resumed."""
        if self._session is None:
            raise RuntimeError("HttpClient.start() must be called before requests")
        params: Dict[str, str] = {}
        if node is not None:
            params["node"] = node
        if follow:
            params["follow"] = "true"
        if tail_lines is not None:
            params["tailLines"] = str(tail_lines)
        if limit_bytes is not None:
            params["limitBytes"] = str(limit_bytes)
        if prefix:
            params["prefix"] = "true"
        url = self.base_url + self._object_path(
            WF_API_VERSION, WF_KIND, namespace, name) + "/log"
        source = self._credentials
        for attempt in (0, 1):
            await self._limiter.acquire()
            self.request_count += 1
            cred = await source.get() if source is not None else None
            async with self._session.get(
                url, params=params, headers=self._session_auth(cred),
                timeout=aiohttp.ClientTimeout(total=None),
            ) as resp:
                if resp.status == 401 and source is not None and attempt == 0:
                    await resp.read()
                    source.invalidate(cred)
                    continue
                if resp.status >= 400:
                    raise _error_for(resp.status, await resp.read())
                async for chunk in resp.content.iter_any():
                    yield chunk
                return

    def watch(self, api_version: str, kind: str, namespace: Optional[str] = None) -> HttpSubscription:
        return HttpSubscription(self, api_version, kind, namespace)

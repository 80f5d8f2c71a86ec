"""One HTTP exchange over asyncio streams: what an ``http`` template runs.

:func:`probe` sends one request, follows redirects the way Go's client does
(Argo's behaviour as remembered, not diffed) and returns the status, the
headers and the start of the body. It starts no thread and no process of its
own; the one thing asyncio itself hands to a thread is the lookup of a host
name that is not an address. Every hop has a connection of its own, which is
closed, and waited for, before :func:`probe` returns or raises, a timeout or
a cancellation included.
"""
from __future__ import annotations

import asyncio
import socket
import ssl
import time
from typing import Callable, List, NamedTuple, Optional, Tuple
from urllib.parse import urljoin, urlsplit

from ..utils import wirecodec
from .executor import RESULT_MAX_BYTES
from .expr import Headers
from .template import TemplateError

#: a response head, interim ones included, is at most this long
HEAD_MAX_BYTES = 64 * 1024
MAX_REDIRECTS = 10
#: interim (1xx) responses tolerated before the final one
_MAX_INTERIM = 8
_READ_CHUNK = 16 * 1024
_SENSITIVE = ("authorization", "cookie")
_NO_BODY_METHODS = ("GET", "HEAD")

Log = Callable[[str], None]


class ProbeError(TemplateError):
    """The exchange failed; the message is one line."""

    def __init__(self, detail: str):
        super().__init__("http request failed: " + " ".join(str(detail).split()))


class Request(NamedTuple):
    url: str
    method: str = "GET"
    headers: Tuple[Tuple[str, str], ...] = ()
    body: Optional[str] = None


class Response(NamedTuple):
    status: int
    reason: str
    headers: Headers
    #: the first ``RESULT_MAX_BYTES`` of the body
    body: bytes
    #: the body was longer than what was kept; the rest was never read
    truncated: bool
    #: where the response came from, after redirects
    url: str


def _seconds(value: float) -> str:
    return f"{value:g}s"


async def probe(request: Request, *, timeout: float, insecure: bool = False,
                log: Optional[Log] = None) -> Response:
    """``timeout`` bounds all of it: name lookup, connect, TLS, every
    redirect and the body. ``insecure`` turns off the verification of the
    server's certificate chain and name. ``log`` gets a ``> METHOD URL`` line
    per hop and a ``< STATUS REASON (N bytes, T ms)`` line per response;
    header values are never passed to it."""
    try:
        return await asyncio.wait_for(_exchange(request, insecure, log), timeout)
    except asyncio.TimeoutError:
        raise ProbeError(f"timed out after {_seconds(timeout)}") from None


def _check_line(what: str, text: str) -> str:
    if "\r" in text or "\n" in text:
        raise TemplateError(f"http {what} holds a line break")
    return text


async def _exchange(request: Request, insecure: bool, log: Optional[Log]) -> Response:
    method = _check_line("method", request.method or "GET").upper()
    headers = [(_check_line("header name", str(n)), _check_line("header value", str(v)))
               for n, v in request.headers]
    body = request.body.encode() if request.body is not None else None
    url = request.url
    origin = _netloc(url)
    for hop in range(MAX_REDIRECTS + 1):
        sent = headers
        if _netloc(url) != origin:
            sent = [(n, v) for n, v in headers if n.lower() not in _SENSITIVE]
        response = await _one_hop(url, method, sent, body, insecure, log)
        location = response.headers.first("Location")
        if response.status not in (301, 302, 303, 307, 308) or location is None:
            return response
        if hop == MAX_REDIRECTS:
            raise ProbeError(f"stopped after {MAX_REDIRECTS} redirects")
        if response.status in (301, 302, 303) and method not in _NO_BODY_METHODS:
            method, body = "GET", None
        url = urljoin(url, location)
    raise AssertionError("unreachable")  # pragma: no cover


def _split(url: str) -> Tuple[str, str, int, str]:
    """(scheme, host, port, request target) of an absolute URL."""
    try:
        parts = urlsplit(_check_line("url", url))
        port = parts.port
    except ValueError as e:
        raise TemplateError(f"invalid http url {url!r}: {e}") from None
    scheme = parts.scheme.lower()
    if scheme not in ("http", "https"):
        raise TemplateError(
            f"unsupported url scheme {parts.scheme!r} in {url!r}: only http and https")
    if not parts.hostname:
        raise TemplateError(f"invalid http url {url!r}: no host")
    target = parts.path or "/"
    if parts.query:
        target += "?" + parts.query
    return scheme, parts.hostname, port or (443 if scheme == "https" else 80), target


def _netloc(url: str) -> Tuple[str, int]:
    _, host, port, _ = _split(url)
    return host.lower(), port


def _tls_context(insecure: bool) -> ssl.SSLContext:
    ctx = ssl.create_default_context()
    if insecure:
        ctx.check_hostname = False
        ctx.verify_mode = ssl.CERT_NONE
    return ctx


def _failure(e: BaseException) -> ProbeError:
    if isinstance(e, asyncio.IncompleteReadError):
        return ProbeError("malformed response: body cut short")
    if isinstance(e, ssl.SSLCertVerificationError):
        return ProbeError(f"certificate verify failed: {e.verify_message}")
    if isinstance(e, ssl.SSLError):
        return ProbeError(f"tls: {e.reason or e}")
    if isinstance(e, ConnectionRefusedError):
        return ProbeError("connection refused")
    if isinstance(e, socket.gaierror):
        return ProbeError(f"no such host: {e.strerror or e}")
    if isinstance(e, (ConnectionResetError, BrokenPipeError)):
        return ProbeError("connection reset by peer")
    if isinstance(e, OSError) and getattr(e, "exceptions", None):
        # several addresses were tried: the last one's failure speaks for all
        return _failure(e.exceptions[-1])
    return ProbeError(getattr(e, "strerror", None) or str(e) or type(e).__name__)


async def _one_hop(url: str, method: str, headers: List[Tuple[str, str]],
                   body: Optional[bytes], insecure: bool, log: Optional[Log]) -> Response:
    scheme, host, port, target = _split(url)
    if log is not None:
        log(f"> {method} {url}")
    started = time.monotonic()
    default_port = port == (443 if scheme == "https" else 80)
    shown_host = f"[{host}]" if ":" in host else host
    given = {n.lower() for n, _ in headers}
    lines = [f"{method} {target} HTTP/1.1"]
    if "host" not in given:
        lines.append(f"Host: {shown_host}" if default_port else f"Host: {shown_host}:{port}")
    if "user-agent" not in given:
        from .. import __version__

        lines.append(f"User-Agent: active-monitor-amd/{__version__}")
    lines += [f"{n}: {v}" for n, v in headers
              if n.lower() not in ("connection", "content-length")]
    lines.append("Connection: close")
    payload = b""
    if method not in _NO_BODY_METHODS:
        payload = body or b""
        lines.append(f"Content-Length: {len(payload)}")
    try:
        wire = ("\r\n".join(lines) + "\r\n\r\n").encode("latin-1") + payload
    except UnicodeEncodeError:
        raise TemplateError("http headers hold characters outside Latin-1") from None

    writer: Optional[asyncio.StreamWriter] = None
    graceful = False
    try:
        try:
            reader, writer = await asyncio.open_connection(
                host, port, limit=HEAD_MAX_BYTES,
                ssl=_tls_context(insecure) if scheme == "https" else None)
            writer.write(wire)
            await writer.drain()
            status, reason, found, length, chunked = await _read_head(reader)
            if method == "HEAD" or status in (204, 304):
                kept, truncated = b"", False
            elif chunked:
                kept, truncated = await _read_chunked(reader)
            else:
                kept, truncated = await _read_plain(reader, length)
            graceful = not truncated and scheme == "http"
        except (OSError, asyncio.IncompleteReadError) as e:
            raise _failure(e) from None
        if log is not None:
            ms = int((time.monotonic() - started) * 1000)
            more = "+" if truncated else ""
            log(f"< {status} {reason} ({len(kept)}{more} bytes, {ms} ms)".replace("  ", " "))
        return Response(status, reason, found, kept, truncated, url)
    finally:
        if writer is not None:
            await _close(writer, graceful)


async def _close(writer: asyncio.StreamWriter, graceful: bool) -> None:
    """Close the connection and wait until the transport is gone. Anything
    but a whole plain exchange is aborted: what the peer still sends is of no
    interest, and a TLS shutdown would wait for its answer."""
    if graceful:
        writer.close()
    else:
        writer.transport.abort()
    try:
        await writer.wait_closed()
    except (OSError, asyncio.IncompleteReadError):
        pass


async def _read_head(reader: asyncio.StreamReader
                     ) -> Tuple[int, str, Headers, Optional[int], bool]:
    """(status, reason, headers, content length or None, chunked) of the
    final response; interim ones are read and passed over."""
    for _ in range(_MAX_INTERIM + 1):
        try:
            head = await reader.readuntil(b"\r\n\r\n")
        except asyncio.LimitOverrunError:
            raise ProbeError(
                f"malformed response: head longer than {HEAD_MAX_BYTES} bytes") from None
        except asyncio.IncompleteReadError as e:
            if not e.partial:
                raise ProbeError("connection closed before a response") from None
            raise ProbeError("malformed response: head cut short") from None
        if not head.startswith(b"HTTP/1."):
            raise ProbeError("malformed response")
        try:
            status, length, chunked, _ = wirecodec.parse_response_head(head)
        except (ValueError, IndexError, ConnectionError):
            raise ProbeError("malformed response") from None
        if not 100 <= status <= 599 or length < 0:
            raise ProbeError("malformed response")
        if status >= 200 or status == 101:
            break
    else:
        raise ProbeError(f"malformed response: more than {_MAX_INTERIM} interim responses")
    lines = head.decode("latin-1").split("\r\n")
    reason = lines[0].split(" ", 2)[2].strip() if lines[0].count(" ") >= 2 else ""
    found = Headers()
    for line in lines[1:]:
        name, sep, value = line.partition(":")
        if sep and name.strip():
            found.add(name.strip(), value.strip())
    return (status, reason, found,
            length if found.lookup("Content-Length") is not None else None, chunked)


async def _read_plain(reader: asyncio.StreamReader,
                      length: Optional[int]) -> Tuple[bytes, bool]:
    """A body of ``length`` bytes, or up to the close when None: its first
    ``RESULT_MAX_BYTES``, and whether there was more. One byte past what is
    kept is asked for, to tell; nothing after that."""
    want = RESULT_MAX_BYTES + 1 if length is None else min(length, RESULT_MAX_BYTES + 1)
    chunks: List[bytes] = []
    have = 0
    while have < want:
        chunk = await reader.read(min(_READ_CHUNK, want - have))
        if not chunk:
            if length is not None:
                raise ProbeError(
                    f"malformed response: body ended after {have} of {length} bytes")
            break
        chunks.append(chunk)
        have += len(chunk)
    data = b"".join(chunks)
    return data[:RESULT_MAX_BYTES], len(data) > RESULT_MAX_BYTES


async def _read_chunked(reader: asyncio.StreamReader) -> Tuple[bytes, bool]:
    chunks: List[bytes] = []
    have = 0
    try:
        while have <= RESULT_MAX_BYTES:
            size_line = await reader.readline()
            try:
                size = int(size_line.split(b";")[0].strip(), 16)
            except ValueError:
                raise ProbeError("malformed response: bad chunk size") from None
            if size < 0:
                raise ProbeError("malformed response: bad chunk size")
            if size == 0:
                break  # trailers, if any, are of no interest
            take = min(size, RESULT_MAX_BYTES + 1 - have)
            while take:
                piece = await reader.read(min(_READ_CHUNK, take))
                if not piece:
                    raise ProbeError("malformed response: chunk cut short")
                chunks.append(piece)
                have += len(piece)
                take -= len(piece)
                size -= len(piece)
            if size:
                break  # the cap fell inside this chunk
            if await reader.readexactly(2) != b"\r\n":
                raise ProbeError("malformed response: chunk without its line end")
    except asyncio.LimitOverrunError:
        raise ProbeError("malformed response: bad chunk size") from None
    except ValueError:
        # readline() on a line longer than the reader's limit
        raise ProbeError("malformed response: bad chunk size") from None
    data = b"".join(chunks)
    return data[:RESULT_MAX_BYTES], len(data) > RESULT_MAX_BYTES

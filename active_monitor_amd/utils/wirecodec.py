"""The wire codec: HTTP/1.1 head parsing and JSON to/from bytes.

Everything the apiserver frontend (kube/server.py) and the HTTP client
(kube/http.py) do to turn bytes into requests/objects and back lives here,
once. Like ``utils/fastcopy.py`` there are two layers:

- the pure-Python implementations (``_py_*``) are the expressions both files
  used inline before: ``json.dumps(obj, separators=(",", ":")).encode()``,
  ``json.loads``, the header ``if``-chains and the ``urllib`` target split.
  They define the behaviour.
- when the native extension is built (``native/wirejson.c``,
  ``native/wirehead.c``), its functions run first. Each handles exactly the
  shapes this wire carries — plain dict/list/str/int/float/bool/None trees,
  CRLF heads with plain targets — and answers ``NotImplemented`` for anything
  else, on which the ``_py_*`` function runs unchanged. The fast path never
  guesses, so values *and* exceptions are the stdlib's.

Switches: ``AM_REQUIRE_NATIVE=1`` makes a missing native codec fatal (GPU
boxes: no silent fallback). ``AM_WIRE_NATIVE=0`` forces the Python layer even
when the extension is there — a diagnostic; child processes inherit it, so
one variable switches the controller and a spawned apiserver together.

Heads are parsed whole: the caller reads up to the blank line
(``readuntil(b"\\r\\n\\r\\n")``) and hands the bytes over.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, Iterator, Optional, Tuple
from urllib.parse import parse_qsl, unquote, urlsplit

#: bits of the ``flags`` element of a parsed request head
EXPECT_CONTINUE = 1
WANT_TABLE = 2

RequestHead = Tuple[str, str, Dict[str, str], int, str, int, bytes]
ResponseHead = Tuple[int, int, bool, bool]


# -- pure-Python layer --------------------------------------------------------

def _py_dumpb(obj: Any) -> bytes:
    return json.dumps(obj, separators=(",", ":")).encode()


def _py_frame(prefix: bytes, obj: Any) -> bytes:
    payload = json.dumps(obj, separators=(",", ":")).encode() if obj is not None else b""
    return prefix + (
        f"Content-Length: {len(payload)}\r\n\r\n"
    ).encode("latin-1") + payload


def _py_loads_strict(data: bytes) -> Any:
    """The server's decode: the stdlib on the bytes as received."""
    return json.loads(data)


def _py_loads_lenient(data: bytes) -> Any:
    """The client's decode: undecodable bytes become U+FFFD first."""
    return json.loads(data.decode("utf-8", "replace"))


def _head_lines(head: bytes) -> Iterator[bytes]:
    """The lines ``StreamReader.readline`` would have returned."""
    pos = 0
    while pos < len(head):
        nl = head.find(b"\n", pos)
        end = len(head) if nl < 0 else nl + 1
        yield head[pos:end]
        pos = end


def _py_parse_request_head(head: bytes) -> Optional[RequestHead]:
    """(method, path, query, content_length, content_type, flags,
    authorization), or None for an empty or malformed request line (the
    connection is then closed)."""
    lines = _head_lines(head)
    request_line = next(lines, b"")
    if not request_line or request_line in (b"\r\n", b"\n"):
        return None
    try:
        method, target, _ = request_line.decode("latin-1").split(" ", 2)
    except ValueError:
        return None
    content_length = 0
    content_type = ""
    expect_continue = False
    want_table = False
    authorization = b""
    for line in lines:
        if line in (b"\r\n", b"\n", b""):
            break
        lower = line.lower()
        if lower.startswith(b"content-length:"):
            content_length = int(line.split(b":", 1)[1])
        elif lower.startswith(b"content-type:"):
            content_type = line.split(b":", 1)[1].strip().decode("latin-1")
        elif lower.startswith(b"expect:") and b"100-continue" in lower:
            expect_continue = True  # curl sends this for big bodies
        elif lower.startswith(b"accept:") and b"as=table" in lower:
            want_table = True
        elif lower.startswith(b"authorization:"):
            authorization = line.split(b":", 1)[1].strip()

    parts = urlsplit(target)
    path = unquote(parts.path)
    query = dict(parse_qsl(parts.query))
    flags = ((EXPECT_CONTINUE if expect_continue else 0)
             | (WANT_TABLE if want_table else 0))
    return (method, path, query, content_length, content_type, flags,
            authorization)


def _py_parse_response_head(head: bytes) -> ResponseHead:
    """(status, content_length, chunked, keep_alive)."""
    lines = _head_lines(head)
    status_line = next(lines, b"")
    if not status_line:
        raise ConnectionResetError("server closed connection")
    status = int(status_line.split(b" ", 2)[1])
    content_length = 0
    chunked = False
    keep_alive = True
    for line in lines:
        if line in (b"\r\n", b"\n", b""):
            break
        lower = line.lower()
        if lower.startswith(b"content-length:"):
            content_length = int(line.split(b":", 1)[1])
        elif lower.startswith(b"transfer-encoding:") and b"chunked" in lower:
            chunked = True
        elif lower.startswith(b"connection:") and b"close" in lower:
            keep_alive = False
    return status, content_length, chunked, keep_alive


# -- native layer ---------------------------------------------------------------

try:
    from active_monitor_amd import _amcore  # native/_amcore.c + wire*.c

    _json_dumpb = _amcore.json_dumpb
    _json_frame = _amcore.json_frame
    _json_loadb = _amcore.json_loadb
    _parse_request_head = _amcore.parse_request_head
    _parse_response_head = _amcore.parse_response_head
    HAVE_NATIVE = True
except (ImportError, AttributeError):  # pragma: no cover - toolchain-less installs
    if os.environ.get("AM_REQUIRE_NATIVE") == "1":
        raise ImportError(
            "the native wire codec in active_monitor_amd._amcore is required "
            "(AM_REQUIRE_NATIVE=1) but not built; run "
            "`python setup.py build_ext --inplace`"
        )
    HAVE_NATIVE = False

if HAVE_NATIVE:
    def _native_dumpb(obj: Any) -> bytes:
        out = _json_dumpb(obj)
        if out is NotImplemented:
            return _py_dumpb(obj)
        return out

    def _native_frame(prefix: bytes, obj: Any) -> bytes:
        out = _json_frame(prefix, obj)
        if out is NotImplemented:
            return _py_frame(prefix, obj)
        return out

    def _native_loads_strict(data: bytes) -> Any:
        out = _json_loadb(data)
        if out is NotImplemented:
            return _py_loads_strict(data)
        return out

    def _native_loads_lenient(data: bytes) -> Any:
        out = _json_loadb(data)
        if out is NotImplemented:
            return _py_loads_lenient(data)
        return out

    def _native_parse_request_head(head: bytes) -> Optional[RequestHead]:
        out = _parse_request_head(head)
        if out is NotImplemented:
            return _py_parse_request_head(head)
        return out

    def _native_parse_response_head(head: bytes) -> ResponseHead:
        out = _parse_response_head(head)
        if out is NotImplemented:
            return _py_parse_response_head(head)
        return out


#: True when the functions below start with the native fast path
NATIVE = HAVE_NATIVE and os.environ.get("AM_WIRE_NATIVE") != "0"

if NATIVE:
    dumpb = _native_dumpb
    frame = _native_frame
    loads_strict = _native_loads_strict
    loads_lenient = _native_loads_lenient
    parse_request_head = _native_parse_request_head
    parse_response_head = _native_parse_response_head
else:
    dumpb = _py_dumpb
    frame = _py_frame
    loads_strict = _py_loads_strict
    loads_lenient = _py_loads_lenient
    parse_request_head = _py_parse_request_head
    parse_response_head = _py_parse_response_head

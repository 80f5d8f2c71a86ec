"""One HTTP exchange over asyncio streams, against a scripted loopback
server: body framings, the body cap, redirects, failures, and that no
connection outlives a probe, however it ends."""
import asyncio
import shutil
import socket
import ssl
import time

import pytest

from active_monitor_amd import __version__
from active_monitor_amd.workflow.executor import RESULT_MAX_BYTES
from active_monitor_amd.workflow.httpprobe import ProbeError, Request, probe
from active_monitor_amd.workflow.template import TemplateError
from tests.probeserver import ProbeServer, Route

BIG = bytes(range(256)) * (RESULT_MAX_BYTES // 256) + b"!"  # one byte over the cap


def test_body_by_content_length_chunked_and_to_close(run):
    async def go():
        routes = {
            "/length": Route(body=b"plain body", headers=[("X-Kind", "a"), ("x-kind", "b")]),
            "/chunked": Route(body=b"0123456789" * 250, chunked=True, chunk_size=999),
            "/close": Route(body=b"until the end", to_close=True),
            "/empty": Route(204, "No Content"),
            "/interim": Route(body=b"after 100", interim=True),
        }
        async with ProbeServer(routes) as srv:
            lines = []
            got = {p: await probe(Request(srv.url + p), timeout=5, log=lines.append)
                   for p in routes}
            assert await srv.settled()
            return srv, got, lines

    srv, got, lines = run(go())
    assert got["/length"].status == 200 and got["/length"].reason == "OK"
    assert got["/length"].body == b"plain body" and not got["/length"].truncated
    assert got["/length"].headers.lookup("X-KIND") == ["a", "b"]
    assert got["/length"].headers["Content-Length"] == ["10"]
    assert got["/chunked"].body == b"0123456789" * 250 and not got["/chunked"].truncated
    assert got["/close"].body == b"until the end" and not got["/close"].truncated
    assert got["/empty"].status == 204 and got["/empty"].body == b""
    assert got["/interim"].status == 200 and got["/interim"].body == b"after 100"
    assert srv.closed_early == [] and srv.connections == 5
    first = srv.requests[0]
    assert first.method == "GET" and first.target == "/length"
    assert first.headers["host"] == f"127.0.0.1:{srv.port}"
    assert first.headers["connection"] == "close"
    assert first.headers["user-agent"] == f"active-monitor-amd/{__version__}"
    assert "accept-encoding" not in first.headers and "content-length" not in first.headers
    assert lines[0] == f"> GET {srv.url}/length"
    assert lines[1].startswith("< 200 OK (10 bytes, ") and lines[1].endswith(" ms)")
    assert len(lines) == 10


def test_request_method_headers_and_body(run):
    async def go():
        async with ProbeServer({"/in": Route(201, "Created", body=b"ok")}) as srv:
            await probe(Request(srv.url + "/in?a=1&b=2", "POST",
                                (("Content-Type", "application/json"), ("User-Agent", "mine")),
                                '{"k": "é"}'), timeout=5)
            await probe(Request(srv.url + "/in", "DELETE"), timeout=5)
            got = await probe(Request(srv.url + "/in", "HEAD", (), "ignored"), timeout=5)
            return srv, got

    srv, got = run(go())
    post, delete, head = srv.requests
    assert post.method == "POST" and post.target == "/in?a=1&b=2"
    assert post.body == '{"k": "é"}'.encode() and post.headers["content-length"] == "11"
    assert post.headers["content-type"] == "application/json"
    assert post.headers["user-agent"] == "mine"
    assert delete.headers["content-length"] == "0" and delete.body == b""
    # HEAD: no body sent, none read although Content-Length announces one
    assert head.method == "HEAD" and "content-length" not in head.headers
    assert got.status == 201 and got.body == b"" and not got.truncated
    assert got.headers.first("content-length") == "2"


@pytest.mark.parametrize("how", ["length", "chunked", "to_close"])
def test_a_body_one_byte_over_the_cap_is_cut_there(run, how):
    route = Route(body=BIG, chunked=how == "chunked", chunk_size=4093,
                  to_close=how == "to_close")

    async def go():
        async with ProbeServer({"/big": route, "/fits": Route(body=BIG[:-1])}) as srv:
            big = await probe(Request(srv.url + "/big"), timeout=5)
            fits = await probe(Request(srv.url + "/fits"), timeout=5)
            assert await srv.settled()
            return big, fits

    big, fits = run(go())
    assert len(BIG) == RESULT_MAX_BYTES + 1
    assert big.body == BIG[:RESULT_MAX_BYTES] and big.truncated
    assert fits.body == BIG[:-1] and not fits.truncated


def test_an_endless_body_ends_at_the_cap_and_the_server_sees_the_close(run):
    async def go():
        async with ProbeServer({"/stream": Route(endless=True)}) as srv:
            began = time.monotonic()
            got = await probe(Request(srv.url + "/stream"), timeout=8)
            took = time.monotonic() - began
            assert await srv.settled()
            return srv, got, took

    srv, got, took = run(go())
    assert got.body == b"x" * RESULT_MAX_BYTES and got.truncated
    assert srv.closed_early == ["/stream"]
    assert took < 8  # it returned, it did not time out


def test_redirects_as_go_follows_them(run):
    async def go():
        async with ProbeServer({"/end": Route(body=b"there")}) as other:
            routes = {
                "/302": Route(302, "Found", redirect="/end"),
                "/303": Route(303, "See Other", redirect="/end"),
                "/307": Route(307, "Temporary Redirect", redirect="/end?kept=1"),
                "/308": Route(308, "Permanent Redirect", redirect="/end"),
                "/away": Route(301, "Moved", redirect=other.url + "/end"),
                "/bare": Route(302, "Found", body=b"no location"),
                "/end": Route(body=b"here"),
            }
            async with ProbeServer(routes) as srv:
                auth = (("Authorization", "Bearer s3cret"), ("Cookie", "c=1"), ("X-Trace", "t"))
                out = {}
                for path, method in [("/302", "POST"), ("/303", "PUT"), ("/307", "POST"),
                                     ("/308", "PATCH"), ("/302", "HEAD"), ("/away", "GET"),
                                     ("/bare", "GET")]:
                    before = len(srv.requests), len(other.requests)
                    lines = []
                    resp = await probe(
                        Request(srv.url + path, method, auth,
                                "payload" if method not in ("GET", "HEAD") else None),
                        timeout=5, log=lines.append)
                    out[path, method] = (resp, srv.requests[before[0]:],
                                         other.requests[before[1]:], lines)
                assert await srv.settled() and await other.settled()
                return srv, other, out

    srv, other, out = run(go())
    for (path, method), last_method, last_body in [
            (("/302", "POST"), "GET", b""), (("/303", "PUT"), "GET", b""),
            (("/307", "POST"), "POST", b"payload"), (("/308", "PATCH"), "PATCH", b"payload"),
            (("/302", "HEAD"), "HEAD", b"")]:
        resp, here, there, lines = out[path, method]
        assert resp.status == 200 and resp.url.startswith(srv.url + "/end"), (path, method)
        first, last = here
        assert (first.method, first.body) == (method, b"" if method == "HEAD" else b"payload")
        assert (last.method, last.body) == (last_method, last_body), (path, method)
        assert ("content-length" in last.headers) == (last_method not in ("GET", "HEAD"))
        # the same host: credentials travel along
        assert last.headers["authorization"] == "Bearer s3cret"
        assert [ln.split()[0] for ln in lines] == [">", "<", ">", "<"]
    assert out["/307", "POST"][1][1].target == "/end?kept=1"

    resp, here, there, lines = out["/away", "GET"]
    assert resp.body == b"there" and resp.url == other.url + "/end"
    assert here[0].headers["authorization"] == "Bearer s3cret"
    (arrived,) = there  # another port is another host
    assert "authorization" not in arrived.headers and "cookie" not in arrived.headers
    assert arrived.headers["x-trace"] == "t"
    assert arrived.headers["host"] == f"127.0.0.1:{other.port}"
    assert not any("s3cret" in ln for ln in lines)

    resp, here, _, _ = out["/bare", "GET"]  # nowhere to go: the answer as it is
    assert resp.status == 302 and resp.body == b"no location" and len(here) == 1


def test_ten_redirects_are_followed_the_eleventh_fails(run):
    async def go():
        ten = {f"/r{i}": Route(302, "Found", redirect=f"/r{i + 1}") for i in range(10)}
        ten["/r10"] = Route(body=b"made it")
        eleven = {f"/r{i}": Route(302, "Found", redirect=f"/r{i + 1}") for i in range(11)}
        eleven["/r11"] = Route(body=b"never seen")
        async with ProbeServer(ten) as a, ProbeServer(eleven) as b:
            ok = await probe(Request(a.url + "/r0"), timeout=5)
            with pytest.raises(ProbeError) as e:
                await probe(Request(b.url + "/r0"), timeout=5)
            assert await a.settled() and await b.settled()
            return ok, a.paths(), str(e.value), b.paths()

    ok, a_paths, error, b_paths = run(go())
    assert ok.body == b"made it" and a_paths == [f"/r{i}" for i in range(11)]
    assert error == "http request failed: stopped after 10 redirects"
    assert b_paths == [f"/r{i}" for i in range(11)]  # the 11th Location is not followed


def test_a_refused_connection(run):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]  # bound, not listening: connecting is refused

        async def go():
            with pytest.raises(ProbeError) as e:
                await probe(Request(f"http://127.0.0.1:{port}/"), timeout=5)
            return str(e.value)

        assert run(go()) == "http request failed: connection refused"


def test_malformed_responses_and_other_schemes(run):
    async def go():
        routes = {
            "/garbage": Route(raw=b"SSH-2.0-OpenSSH_9.6\r\n\r\n"),
            "/nostatus": Route(raw=b"HTTP/1.1 abc Nope\r\n\r\n"),
            "/silent": Route(raw=b""),
            "/longhead": Route(raw=b"HTTP/1.1 200 OK\r\nX: " + b"y" * (65 * 1024) + b"\r\n\r\n"),
            "/short": Route(raw=b"HTTP/1.1 200 OK\r\nContent-Length: 10\r\n\r\nabc"),
            "/badchunk": Route(raw=b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\nzz\r\n"),
        }
        errors = {}
        async with ProbeServer(routes) as srv:
            for path in routes:
                with pytest.raises(ProbeError) as e:
                    await probe(Request(srv.url + path), timeout=5)
                errors[path] = str(e.value)
            assert await srv.settled()
            for url in ("ftp://127.0.0.1/x", "file:///etc/passwd", "127.0.0.1/x", "http:///x"):
                with pytest.raises(TemplateError) as e:
                    await probe(Request(url), timeout=5)
                assert not isinstance(e.value, ProbeError), url
            with pytest.raises(TemplateError):
                await probe(Request(srv.url + "/x", headers=(("X", "a\r\nEvil: 1"),)), timeout=5)
            return errors, len(srv.requests)

    errors, seen = run(go())
    assert seen == 6  # nothing was sent for the refused URLs and header
    assert errors["/silent"] == "http request failed: connection closed before a response"
    for path in ("/garbage", "/nostatus", "/longhead", "/short", "/badchunk"):
        assert errors[path].startswith("http request failed: malformed response"), errors
        assert "\n" not in errors[path]


def test_the_timeout_bounds_the_exchange_and_closes_the_socket(run):
    async def go():
        async with ProbeServer({"/slow": Route(delay=30, body=b"late")}) as srv:
            began = time.monotonic()
            with pytest.raises(ProbeError) as e:
                await probe(Request(srv.url + "/slow"), timeout=1)
            took = time.monotonic() - began
            settled = await srv.settled()
            return str(e.value), took, settled, srv.closed_early

    error, took, settled, closed_early = run(go())
    assert error == "http request failed: timed out after 1s"
    # far below the server's 30 s: the bound follows from that gap
    assert 1.0 <= took < 10.0
    assert settled and closed_early == ["/slow"]


def test_a_cancelled_probe_leaves_no_open_transport(run):
    async def go():
        async with ProbeServer({"/slow": Route(delay=30)}) as srv:
            task = asyncio.ensure_future(probe(Request(srv.url + "/slow"), timeout=60))
            for _ in range(500):
                if srv.requests:
                    break
                await asyncio.sleep(0.01)
            assert srv.requests, "the request never arrived"
            task.cancel()
            with pytest.raises(asyncio.CancelledError):
                await task
            settled = await srv.settled()
            return settled, srv.closed_early

    settled, closed_early = run(go())
    assert settled and closed_early == ["/slow"]


@pytest.mark.skipif(shutil.which("openssl") is None, reason="needs the openssl CLI")
def test_tls_is_verified_unless_told_otherwise(run, tmp_path):
    from active_monitor_amd.engine.endpoints import generate_self_signed_cert

    cert, key = generate_self_signed_cert(str(tmp_path))
    ctx = ssl.SSLContext(ssl.PROTOCOL_TLS_SERVER)
    ctx.load_cert_chain(cert, key)

    async def go():
        async with ProbeServer({"/ok": Route(body=b"over tls")}, ssl=ctx) as srv:
            assert srv.url.startswith("https://")
            with pytest.raises(ProbeError) as e:
                await probe(Request(srv.url + "/ok"), timeout=5)
            seen_before = len(srv.requests)
            got = await probe(Request(srv.url + "/ok"), timeout=5, insecure=True)
            assert await srv.settled()
            return str(e.value), seen_before, got

    error, seen_before, got = run(go())
    assert error.startswith("http request failed: certificate verify failed: "), error
    assert "self" in error and "signed" in error  # the reason OpenSSL gives
    assert seen_before == 0  # no request went over the unverified connection
    assert got.status == 200 and got.body == b"over tls"

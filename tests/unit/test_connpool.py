"""Unit tests for the plain-HTTP connection pool behind HttpClient's unary
fast path (kube/http.py _ConnPool): keep-alive reuse, concurrency cap with
FIFO waiters, chunked framing, stale-connection retry at the client layer,
and fail-fast on close."""
import asyncio

import pytest

from active_monitor_amd.kube.http import _ConnPool
from tests.miniserver import MiniServer


def test_keepalive_reuses_one_connection(run):
    async def go():
        async with MiniServer() as srv:
            pool = _ConnPool("127.0.0.1", srv.port)
            for _ in range(20):
                status, body = await pool.request("GET", "/x", "", None)
                assert status == 200 and body == b'{"ok":true}'
            pool.close()
            assert srv.connections == 1, srv.connections
            assert srv.requests == 20

    run(go(), timeout=20)


def test_chunked_framing(run):
    async def go():
        async with MiniServer(chunked=True) as srv:
            pool = _ConnPool("127.0.0.1", srv.port)
            status, body = await pool.request("GET", "/x", "", None)
            assert status == 200 and body == b'{"ok":true}'
            pool.close()

    run(go(), timeout=20)


def test_concurrency_cap_with_fifo_waiters(run):
    async def go():
        async with MiniServer(delay=0.05) as srv:
            pool = _ConnPool("127.0.0.1", srv.port, max_conns=2)
            results = await asyncio.gather(
                *(pool.request("GET", f"/{i}", "", None) for i in range(6))
            )
            assert all(s == 200 for s, _ in results)
            assert srv.connections <= 2, srv.connections
            pool.close()

    run(go(), timeout=20)


def test_server_close_surfaces_as_connection_error(run):
    """A connection the server closed mid-keep-alive raises; HttpClient's
    layer above retries once on a fresh connection (covered end-to-end by
    the apiserver-outage test)."""

    async def go():
        async with MiniServer(close_after=1) as srv:
            pool = _ConnPool("127.0.0.1", srv.port)
            status, _ = await pool.request("GET", "/a", "", None)
            assert status == 200
            with pytest.raises((ConnectionError, asyncio.IncompleteReadError)):
                await pool.request("GET", "/b", "", None)
            # and a fresh request after the failure works (new connection)
            status, _ = await pool.request("GET", "/c", "", None)
            assert status == 200
            pool.close()

    run(go(), timeout=20)


def test_close_fails_queued_waiters(run):
    async def go():
        async with MiniServer(delay=0.2) as srv:
            pool = _ConnPool("127.0.0.1", srv.port, max_conns=1)
            t1 = asyncio.ensure_future(pool.request("GET", "/1", "", None))
            await asyncio.sleep(0.05)  # t1 holds the only connection
            t2 = asyncio.ensure_future(pool.request("GET", "/2", "", None))
            await asyncio.sleep(0.05)  # t2 queued
            pool.close()
            with pytest.raises(ConnectionError):
                await t2
            await t1  # in-flight request completes normally

    run(go(), timeout=20)

"""A scriptable HTTP/1.1 server for the tests of ``http`` templates: what a
path answers is set per path, what arrived is recorded as it was seen."""
import asyncio


class Route:
    """What one path answers. ``redirect`` sets a ``Location`` header;
    ``chunked`` frames ``body`` in chunks of ``chunk_size``; ``to_close``
    sends no framing at all, the body ends with the connection; ``endless``
    never stops sending; ``delay`` waits before anything is sent, and ends
    early when the peer goes away; ``interim`` sends a ``100 Continue``
    first; ``raw`` replaces the whole response."""

    def __init__(self, status=200, reason="OK", headers=(), body=b"", delay=0.0,
                 chunked=False, chunk_size=1000, to_close=False, redirect=None,
                 endless=False, interim=False, raw=None):
        self.status = status
        self.reason = reason
        self.headers = list(headers)
        self.body = body.encode() if isinstance(body, str) else body
        self.delay = delay
        self.chunked = chunked
        self.chunk_size = chunk_size
        self.to_close = to_close
        self.redirect = redirect
        self.endless = endless
        self.interim = interim
        self.raw = raw


class Seen:
    def __init__(self, method, target, headers, body):
        self.method = method
        self.target = target
        #: lower-case name -> value, as sent
        self.headers = headers
        self.body = body


class ProbeServer:
    """``routes``: path -> Route, or a list of Routes served one after the
    other, the last one for good. Any other path answers 404.

    ``requests`` holds every request in arrival order; ``closed_early`` the
    paths whose peer closed before the response was all sent; ``peak`` the
    most requests that were being served at once; ``open`` the connections
    not yet closed on this side."""

    def __init__(self, routes=None, ssl=None):
        self.routes = {k: list(v) if isinstance(v, (list, tuple)) else [v]
                       for k, v in (routes or {}).items()}
        self._ssl = ssl
        self.requests = []
        self.closed_early = []
        self.connections = 0
        self.open = 0
        self.active = 0
        self.peak = 0
        self._handlers = set()

    async def __aenter__(self):
        self._srv = await asyncio.start_server(self._accept, "127.0.0.1", 0, ssl=self._ssl)
        self.port = self._srv.sockets[0].getsockname()[1]
        scheme = "https" if self._ssl is not None else "http"
        self.url = f"{scheme}://127.0.0.1:{self.port}"
        return self

    async def __aexit__(self, *exc):
        self._srv.close()
        for task in list(self._handlers):
            task.cancel()
        await asyncio.gather(*self._handlers, return_exceptions=True)

    async def settled(self, timeout=5.0):
        """Wait until every connection accepted so far has been closed."""
        loop = asyncio.get_running_loop()
        end = loop.time() + timeout
        while self.open and loop.time() < end:
            await asyncio.sleep(0.005)
        return self.open == 0

    def paths(self):
        return [r.target for r in self.requests]

    async def _accept(self, reader, writer):
        task = asyncio.current_task()
        self._handlers.add(task)
        self.connections += 1
        self.open += 1
        try:
            await self._serve(reader, writer)
            writer.close()  # sends what is still buffered first
            await asyncio.wait_for(writer.wait_closed(), 2.0)
        except (OSError, asyncio.IncompleteReadError, asyncio.TimeoutError,
                asyncio.CancelledError):
            writer.transport.abort()
        finally:
            self._handlers.discard(task)
            self.open -= 1

    async def _serve(self, reader, writer):
        try:
            head = await reader.readuntil(b"\r\n\r\n")
        except asyncio.IncompleteReadError:
            return  # a TLS handshake that failed, a port scan
        lines = head.decode("latin-1").split("\r\n")
        method, target, _ = lines[0].split(" ", 2)
        headers = {}
        for line in lines[1:]:
            name, sep, value = line.partition(":")
            if sep:
                headers[name.strip().lower()] = value.strip()
        length = int(headers.get("content-length", 0))
        body = await reader.readexactly(length) if length else b""
        self.requests.append(Seen(method, target, headers, body))
        path = target.split("?", 1)[0]
        queue = self.routes.get(path)
        if queue is None:
            route = Route(404, "Not Found", body=b"no such path\n")
        else:
            route = queue.pop(0) if len(queue) > 1 else queue[0]
        self.active += 1
        self.peak = max(self.peak, self.active)
        try:
            await self._answer(route, path, method, reader, writer)
        except ConnectionError:
            self.closed_early.append(path)
        finally:
            self.active -= 1

    async def _answer(self, route, path, method, reader, writer):
        if route.delay:
            # nothing more is due from the peer: a read that ends means it left
            gone = asyncio.ensure_future(reader.read(1))
            try:
                await asyncio.wait([gone], timeout=route.delay)
            finally:
                gone.cancel()
            await asyncio.wait([gone])  # the reader is free again only then
            if not gone.cancelled():
                gone.exception()  # a reset says the same as an end of stream
                self.closed_early.append(path)
                return
        if route.raw is not None:
            writer.write(route.raw)
            await writer.drain()
            return
        if route.interim:
            writer.write(b"HTTP/1.1 100 Continue\r\n\r\n")
        head = [f"HTTP/1.1 {route.status} {route.reason}"]
        head += [f"{n}: {v}" for n, v in route.headers]
        if route.redirect is not None:
            head.append(f"Location: {route.redirect}")
        if route.endless or route.chunked:
            head.append("Transfer-Encoding: chunked")
        elif not route.to_close:
            head.append(f"Content-Length: {len(route.body)}")
        writer.write(("\r\n".join(head) + "\r\n\r\n").encode("latin-1"))
        if method == "HEAD":
            await writer.drain()
            return
        if route.endless:
            piece = b"2000\r\n" + b"x" * 0x2000 + b"\r\n"
            for _ in range(16 * 1024):  # 128 MiB: nobody should read that far
                writer.write(piece)
                await writer.drain()
            return
        if route.chunked:
            for at in range(0, len(route.body), route.chunk_size):
                piece = route.body[at:at + route.chunk_size]
                writer.write(f"{len(piece):x}\r\n".encode() + piece + b"\r\n")
            writer.write(b"0\r\n\r\n")
        else:
            writer.write(route.body)
        await writer.drain()
        if writer.can_write_eof() and self._ssl is None:
            # a whole response: let the peer read it and close in its time
            writer.write_eof()
            await reader.read()

"""A scriptable HTTP/1.1 server for tests of the client's transports."""
import asyncio


class MiniServer:
    """Counts connections and requests, answers every request 200 with
    ``body``; can close a connection after N responses and can answer
    chunked."""

    def __init__(self, close_after=None, chunked=False, delay=0.0,
                 body=b'{"ok":true}'):
        self.close_after = close_after
        self.chunked = chunked
        self.delay = delay
        self.body = body
        self.connections = 0
        self.requests = 0

    async def __aenter__(self):
        self._srv = await asyncio.start_server(self._handle, "127.0.0.1", 0)
        self.port = self._srv.sockets[0].getsockname()[1]
        return self

    async def __aexit__(self, *exc):
        self._srv.close()

    async def _handle(self, reader, writer):
        self.connections += 1
        served = 0
        try:
            while True:
                line = await reader.readline()
                if not line or line in (b"\r\n", b"\n"):
                    return
                length = 0
                while True:
                    h = await reader.readline()
                    if h in (b"\r\n", b"\n", b""):
                        break
                    if h.lower().startswith(b"content-length:"):
                        length = int(h.split(b":", 1)[1])
                if length:
                    await reader.readexactly(length)
                self.requests += 1
                if self.delay:
                    await asyncio.sleep(self.delay)
                body = self.body
                if self.chunked:
                    writer.write(
                        b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
                        + hex(len(body))[2:].encode() + b"\r\n" + body + b"\r\n0\r\n\r\n"
                    )
                else:
                    writer.write(
                        b"HTTP/1.1 200 OK\r\nContent-Length: "
                        + str(len(body)).encode() + b"\r\n\r\n" + body
                    )
                await writer.drain()
                served += 1
                if self.close_after is not None and served >= self.close_after:
                    return
        except (ConnectionError, asyncio.IncompleteReadError):
            pass
        finally:
            writer.close()

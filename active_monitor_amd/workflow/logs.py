"""What the leaves of locally executed workflows printed.

:class:`LogStore` keeps the output of every Pod node of a run in files of a
bounded size, serves it (optionally following a run that is still going) and
drops it with the Workflow. It is the standalone stand-in for ``kubectl
logs`` / ``argo logs``: there are no pods whose logs a kubelet would keep.

Layout, under the store's directory::

    <namespace>/<workflow>/index      one JSON line per node, in start order
    <namespace>/<workflow>/<n>.<off>  a segment of node n; <off> is the offset
                                      of its first byte in what the node wrote

File names are generated. A node id comes from user YAML (``withItems:
["/", "../x"]`` is legal) and appears only inside ``index``; namespace and
workflow name must be single path segments.

A node is written in segments of half its cap. When a third would begin, the
oldest is removed, so the node never holds more than the cap and, once it has
written more, always at least the newest half of it. The lowest ``<off>``
left is the exact number of bytes dropped, which is how a reader — also one
in a later process — words ``[log truncated: N bytes dropped]``.

Everything runs on the event loop: writes are appends followed by a flush
(in the OS, so they survive a kill of the process), reads are of at most one
node's cap at a time.
"""
from __future__ import annotations

import asyncio
import json
import logging
import os
import shutil
import tempfile
from collections import deque
from typing import AsyncIterator, Dict, Iterable, List, Optional, Set, Tuple

from ..kube.errors import NotFoundError

log = logging.getLogger("active_monitor_amd.workflow.logs")

DEFAULT_MAX_NODE_BYTES = 1024 * 1024
DEFAULT_MAX_TOTAL_BYTES = 256 * 1024 * 1024
#: a line longer than this is stored in pieces; a partial line is flushed
#: once it passes it
MAX_LINE_BYTES = 16 * 1024
#: what a follower that does not keep up may have waiting before records are
#: skipped for it (and counted)
FOLLOW_BACKLOG_BYTES = 4 * 1024 * 1024
INDEX_FILE = "index"
#: the directory of the namespace ``""``; no namespace name starts with ``_``
NO_NAMESPACE_DIR = "_"

RunKey = Tuple[str, str]


def _segment(value: str, what: str) -> str:
    """``value`` if it can be one path segment, else ValueError."""
    if (not isinstance(value, str) or not value or value in (".", "..")
            or "/" in value or "\\" in value or "\0" in value):
        raise ValueError(f"{what} {value!r} is not a single path segment")
    return value


def _run_dirs(namespace: str, name: str) -> Tuple[str, str]:
    ns_dir = NO_NAMESPACE_DIR if namespace == "" else _segment(namespace, "namespace")
    if namespace == NO_NAMESPACE_DIR:
        raise ValueError(f"namespace {namespace!r} is reserved")
    return ns_dir, _segment(name, "workflow name")


class _Node:
    __slots__ = ("seq", "id", "display", "segments", "writer")

    def __init__(self, seq: int, node_id: str, display: str):
        self.seq = seq
        self.id = node_id
        self.display = display
        #: [offset of the first byte, bytes held], oldest first
        self.segments: List[List[int]] = []
        self.writer: Optional["LogWriter"] = None

    @property
    def dropped(self) -> int:
        return self.segments[0][0] if self.segments else 0

    @property
    def end(self) -> int:
        """How many bytes the node has written so far."""
        return sum(self.segments[-1]) if self.segments else 0


class _Run:
    __slots__ = ("namespace", "name", "path", "nodes", "finished", "size",
                 "followers")

    def __init__(self, namespace: str, name: str, path: str):
        self.namespace = namespace
        self.name = name
        self.path = path
        self.nodes: List[_Node] = []
        self.finished = False
        self.size = 0
        self.followers: List["_Follower"] = []

    def select(self, node: Optional[str]) -> List[_Node]:
        if node is None:
            return list(self.nodes)
        return ([n for n in self.nodes if n.id == node]
                or [n for n in self.nodes if n.display == node])


class _Follower:
    """The live end of one ``follow`` read: records of the selected nodes in
    the order they were written, in a backlog of bounded size."""

    def __init__(self, node: Optional[str]):
        self.node = node
        #: (node, lines, node.end after them)
        self.records: "deque[Tuple[_Node, bytes, int]]" = deque()
        self.backlog = 0
        self.skipped = 0
        self.done = False
        self.wake = asyncio.Event()

    def wants(self, n: _Node) -> bool:
        return self.node is None or self.node in (n.id, n.display)

    def push(self, n: _Node, data: bytes, upto: int) -> None:
        if self.backlog + len(data) > FOLLOW_BACKLOG_BYTES:
            self.skipped += len(data)
            return
        self.records.append((n, data, upto))
        self.backlog += len(data)
        self.wake.set()

    def end(self) -> None:
        self.done = True
        self.wake.set()


class LogStream:
    """What :meth:`LogStore.read` returns: an async iterator of ``bytes``.
    ``close()`` ends a following read once it has served what is waiting."""

    def __init__(self, gen: AsyncIterator[bytes], follower: Optional[_Follower]):
        self._gen = gen
        self._follower = follower

    def __aiter__(self) -> "LogStream":
        return self

    def __anext__(self):
        return self._gen.__anext__()

    def close(self) -> None:
        if self._follower is not None:
            self._follower.end()

    def aclose(self):
        return self._gen.aclose()


class LogWriter:
    """The write end of one node. ``write`` takes chunks as they were read
    from the leaf's pipes; ``close`` flushes a last partial line."""

    def __init__(self, store: "LogStore", run: _Run, node: _Node):
        self._store = store
        self._run = run
        self._node = node
        self._partial = bytearray()
        self._file = None
        self._closed = False
        self._failed = False
        self._segment_done = False

    def write(self, chunk: bytes) -> None:
        if self._closed or not chunk:
            return
        buf = self._partial
        buf += chunk
        end = buf.rfind(b"\n") + 1
        if end:
            self._records(bytes(buf[:end]))
            del buf[:end]
        if len(buf) > MAX_LINE_BYTES:
            self._records(bytes(buf))
            buf.clear()

    def close(self) -> None:
        if self._closed:
            return
        if self._partial:
            self._records(bytes(self._partial))
            self._partial.clear()
        self._closed = True
        self._close_file()
        self._node.writer = None

    def _close_file(self) -> None:
        if self._file is not None:
            try:
                self._file.close()
            except OSError:
                pass
            self._file = None

    def _records(self, data: bytes) -> None:
        """Append whole lines. A segment ends at a line end unless one line
        (or forced piece) alone is longer than what is left of it."""
        store, node = self._store, self._node
        if self._run.path is None:  # the run was discarded under the writer
            return
        half = store.segment_bytes
        pos, total = 0, len(data)
        while pos < total:
            if self._segment_done or not node.segments:
                self._rotate()
            seg = node.segments[-1]
            room = half - seg[1]
            if total - pos <= room:
                end = total
            else:
                self._segment_done = True
                # as many whole lines as fit
                end = data.rfind(b"\n", pos, pos + room) + 1
                if end <= pos:
                    line_end = data.find(b"\n", pos) + 1 or total
                    if seg[1] and line_end - pos <= min(half, MAX_LINE_BYTES):
                        continue  # the next segment takes the line whole
                    # longer than a segment, or than any stored line: cut
                    end = pos + room
            piece = data[pos:end]
            self._append(piece)
            seg[1] += len(piece)
            self._run.size += len(piece)
            store.total_bytes += len(piece)
            pos = end
        if self._run.followers:
            upto = node.end
            for f in self._run.followers:
                if f.wants(node):
                    f.push(node, data, upto)
        if store.total_bytes > store.max_total_bytes:
            store._evict()

    def _rotate(self) -> None:
        """Begin the next segment; of three, remove the oldest."""
        store, node, run = self._store, self._node, self._run
        self._close_file()
        self._segment_done = False
        offset = node.end
        while len(node.segments) >= 2:
            first = node.segments.pop(0)
            try:
                os.unlink(store._segment_path(run, node, first[0]))
            except OSError:
                pass
            run.size -= first[1]
            store.total_bytes -= first[1]
        node.segments.append([offset, 0])
        if self._failed:
            return
        try:
            self._file = open(store._segment_path(run, node, offset), "ab")
        except OSError as e:
            self._fail(e)

    def _append(self, piece: bytes) -> None:
        if self._failed or self._file is None:
            return
        try:
            self._file.write(piece)
            self._file.flush()  # in the OS: survives a kill of this process
        except (OSError, ValueError) as e:
            self._fail(e)

    def _fail(self, e: Exception) -> None:
        if not self._failed:
            log.warning("workflow log %s/%s node %s: %s; the rest of its "
                        "output is not kept", self._run.namespace,
                        self._run.name, self._node.id, e)
        self._failed = True
        self._close_file()


class LogStore:
    def __init__(self, directory: Optional[str] = None,
                 max_node_bytes: int = DEFAULT_MAX_NODE_BYTES,
                 max_total_bytes: int = DEFAULT_MAX_TOTAL_BYTES):
        if max_node_bytes < 2 or max_total_bytes < 1:
            raise ValueError("log caps must be positive")
        self._own_directory = directory is None
        if directory is None:
            directory = tempfile.mkdtemp(prefix="am-logs-")
        else:
            os.makedirs(directory, exist_ok=True)
        self.directory = os.path.abspath(directory)
        self.max_node_bytes = int(max_node_bytes)
        self.max_total_bytes = int(max_total_bytes)
        self.segment_bytes = self.max_node_bytes // 2
        self.total_bytes = 0
        #: runs in the order they were started (recovered ones: by age)
        self._runs: Dict[RunKey, _Run] = {}
        #: finished runs, the first to be dropped first
        self._finished: "deque[RunKey]" = deque()
        self._closed = False

    # -- lifetime ---------------------------------------------------------

    @classmethod
    def open(cls, directory: str, live: Optional[Iterable[RunKey]] = None,
             max_node_bytes: int = DEFAULT_MAX_NODE_BYTES,
             max_total_bytes: int = DEFAULT_MAX_TOTAL_BYTES) -> "LogStore":
        """The store over what an earlier process left in ``directory``.
        Every run found is finished as far as this store goes: it is served
        as it is and never appended to. ``live`` is the ``(namespace, name)``
        of the Workflows that exist; with it, every other run directory is
        removed."""
        store = cls(directory, max_node_bytes, max_total_bytes)
        keep: Optional[Set[RunKey]] = None if live is None else set(live)
        found: List[Tuple[float, _Run]] = []
        for ns_dir in sorted(os.listdir(store.directory)):
            ns_path = os.path.join(store.directory, ns_dir)
            if not os.path.isdir(ns_path) or os.path.islink(ns_path):
                continue
            namespace = "" if ns_dir == NO_NAMESPACE_DIR else ns_dir
            for name in sorted(os.listdir(ns_path)):
                path = os.path.join(ns_path, name)
                if not os.path.isdir(path) or os.path.islink(path):
                    continue
                if keep is not None and (namespace, name) not in keep:
                    shutil.rmtree(path, ignore_errors=True)
                    continue
                run = store._load_run(namespace, name, path)
                try:
                    age = os.path.getmtime(os.path.join(path, INDEX_FILE))
                except OSError:
                    age = 0.0
                found.append((age, run))
            _remove_if_empty(ns_path)
        found.sort(key=lambda pair: pair[0])
        for _, run in found:
            key = (run.namespace, run.name)
            store._runs[key] = run
            store._finished.append(key)
            store.total_bytes += run.size
        if store.total_bytes > store.max_total_bytes:
            store._evict()
        return store

    def _load_run(self, namespace: str, name: str, path: str) -> _Run:
        run = _Run(namespace, name, path)
        run.finished = True
        by_seq: Dict[int, _Node] = {}
        try:
            with open(os.path.join(path, INDEX_FILE), "rb") as f:
                index = f.read()
        except OSError:
            index = b""
        run.size = len(index)
        lines = index.split(b"\n")
        for raw in lines:
            try:  # a torn last line (killed while writing it) is dropped
                rec = json.loads(raw)
                node = _Node(int(rec["seq"]), str(rec["id"]), str(rec["displayName"]))
            except (ValueError, TypeError, KeyError):
                continue
            if node.seq not in by_seq:
                by_seq[node.seq] = node
                run.nodes.append(node)
        for entry in os.listdir(path):
            seq, dot, offset = entry.partition(".")
            if not (dot and seq.isdigit() and offset.isdigit()):
                continue
            node = by_seq.get(int(seq))
            if node is None:
                continue
            try:
                held = os.path.getsize(os.path.join(path, entry))
            except OSError:
                continue
            node.segments.append([int(offset), held])
            run.size += held
        for node in run.nodes:
            node.segments.sort()
        return run

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        for run in self._runs.values():
            for f in list(run.followers):
                f.end()
            for node in run.nodes:
                if node.writer is not None:
                    node.writer.close()
        if self._own_directory:
            shutil.rmtree(self.directory, ignore_errors=True)

    def describe(self) -> str:
        """``DIR (N runs, B bytes)``, for the line logged at start."""
        return f"{self.directory} ({len(self._runs)} runs, {self.total_bytes} bytes)"

    # -- runs -------------------------------------------------------------

    def has_run(self, namespace: str, name: str) -> bool:
        return (namespace, name) in self._runs

    def runs(self) -> List[RunKey]:
        return list(self._runs)

    def start_run(self, namespace: str, name: str) -> None:
        """Begin (or begin again) the run of this Workflow. ValueError when
        namespace or name cannot be a path segment."""
        ns_dir, name_dir = _run_dirs(namespace, name)
        if self._closed:
            raise ValueError("the log store is closed")
        self.discard(namespace, name)
        path = os.path.join(self.directory, ns_dir, name_dir)
        if os.path.lexists(path):  # left by a process this store never read
            shutil.rmtree(path, ignore_errors=True)
        os.makedirs(path)
        # the index exists from the start: an empty run is still a run
        with open(os.path.join(path, INDEX_FILE), "ab"):
            pass
        self._runs[(namespace, name)] = _Run(namespace, name, path)

    def writer(self, namespace: str, name: str, node_id: str,
               display_name: Optional[str] = None) -> LogWriter:
        """The writer of one Pod node; the run is begun if it has not been.
        ValueError as for :meth:`start_run`; OSError when the run's
        directory cannot be written."""
        run = self._runs.get((namespace, name))
        if run is None or run.finished:
            self.start_run(namespace, name)
            run = self._runs[(namespace, name)]
        node = _Node(len(run.nodes), node_id,
                     node_id if display_name is None else display_name)
        line = json.dumps({"seq": node.seq, "id": node.id,
                           "displayName": node.display}).encode() + b"\n"
        with open(os.path.join(run.path, INDEX_FILE), "ab") as f:
            f.write(line)
        run.size += len(line)
        self.total_bytes += len(line)
        run.nodes.append(node)
        node.writer = LogWriter(self, run, node)
        for f in run.followers:
            f.wake.set()
        return node.writer

    def finish_run(self, namespace: str, name: str) -> None:
        """No more is written to this run: followers end once they have
        served what there is, and the run may be dropped for the total cap."""
        run = self._runs.get((namespace, name))
        if run is None or run.finished:
            return
        for node in run.nodes:
            if node.writer is not None:
                node.writer.close()
        run.finished = True
        self._finished.append((namespace, name))
        for f in list(run.followers):
            f.end()
        if self.total_bytes > self.max_total_bytes:
            self._evict()

    def discard(self, namespace: str, name: str) -> None:
        """Remove the run's files, if it has any."""
        run = self._runs.pop((namespace, name), None)
        if run is None:
            return
        for f in list(run.followers):
            f.end()
        for node in run.nodes:
            if node.writer is not None:
                node.writer._close_file()
        self.total_bytes -= run.size
        path, run.path = run.path, None
        try:
            self._finished.remove((namespace, name))
        except ValueError:
            pass
        shutil.rmtree(path, ignore_errors=True)
        _remove_if_empty(os.path.dirname(path))

    def _evict(self) -> None:
        """Over the total cap: drop whole finished runs, oldest first."""
        while self.total_bytes > self.max_total_bytes and self._finished:
            namespace, name = self._finished[0]
            log.info("workflow logs over %d bytes: dropping %s/%s",
                     self.max_total_bytes, namespace, name)
            self.discard(namespace, name)

    # -- files ------------------------------------------------------------

    @staticmethod
    def _segment_path(run: _Run, node: _Node, offset: int) -> str:
        return os.path.join(run.path, f"{node.seq}.{offset}")

    def _node_bytes(self, run: _Run, node: _Node) -> Tuple[int, bytes]:
        """``(bytes dropped, what is held)`` of one node: at most its cap."""
        parts: List[bytes] = []
        dropped = node.dropped
        for seg in node.segments:
            try:
                with open(self._segment_path(run, node, seg[0]), "rb") as f:
                    parts.append(f.read())
            except OSError:
                pass
        return dropped, b"".join(parts)

    # -- read -------------------------------------------------------------

    def read(self, namespace: str, name: str, node: Optional[str] = None,
             follow: bool = False, tail_lines: Optional[int] = None,
             limit_bytes: Optional[int] = None,
             prefix: bool = False) -> LogStream:
        """The log of a run, or of the nodes of it that ``node`` names (by
        id, else by ``displayName``), as an async iterator of ``bytes``, each
        of whole lines. NotFoundError — raised here, not at the first
        ``__anext__`` — for a run or a node the store does not have; a run
        that is still going may be followed for a node that has yet to
        start."""
        run = self._runs.get((namespace, name))
        if run is None:
            raise NotFoundError(f"no logs for workflow {namespace}/{name}")
        if node is not None and not run.select(node) and (run.finished or not follow):
            raise NotFoundError(
                f"workflow {namespace}/{name} has no node {node!r}")
        follower = _Follower(node) if follow else None
        return LogStream(
            self._read(run, node, follower, tail_lines, limit_bytes, prefix),
            follower)

    async def _read(self, run: _Run, node: Optional[str],
                    follower: Optional[_Follower], tail_lines: Optional[int],
                    limit_bytes: Optional[int], prefix: bool) -> AsyncIterator[bytes]:
        left = limit_bytes
        # what each node had written when its stored part was served: a
        # follower's record at or below it has been served already
        served: Dict[int, int] = {}
        if follower is not None:
            # subscribed in the step that lists the nodes to serve from the
            # files: every record is in the files by then, or comes through
            # the follower, or both (and `served` tells)
            if run.finished or run.path is None:
                follower.done = True
            else:
                run.followers.append(follower)
        try:
            for n in run.select(node):
                if run.path is None:
                    return
                data = self._render(run, n, tail_lines, prefix)
                served[n.seq] = n.end
                if left is not None:
                    data = data[:max(left, 0)]
                    left -= len(data)
                if data:
                    yield data
                if left is not None and left <= 0:
                    return
            if follower is None:
                return
            # whether each node stands at a line start, so that a prefix goes
            # in front of lines, not of the pieces a long line is stored in
            line_start: Dict[int, bool] = {}
            while True:
                while follower.records:
                    n, data, upto = follower.records.popleft()
                    follower.backlog -= len(data)
                    if upto <= served.get(n.seq, 0):
                        continue
                    if prefix:
                        data = _prefixed(data, n.display.encode() + b": ",
                                         line_start.get(n.seq, True))
                        line_start[n.seq] = data.endswith(b"\n")
                    if left is not None:
                        data = data[:max(left, 0)]
                        left -= len(data)
                    if data:
                        yield data
                    if left is not None and left <= 0:
                        return
                if follower.skipped:
                    skipped, follower.skipped = follower.skipped, 0
                    yield (b"[log follow: %d bytes skipped, reader too slow]\n"
                           % skipped)
                if follower.done and not follower.records:
                    return
                follower.wake.clear()
                await follower.wake.wait()
        finally:
            if follower is not None and follower in run.followers:
                run.followers.remove(follower)

    def _render(self, run: _Run, node: _Node, tail_lines: Optional[int],
                prefix: bool) -> bytes:
        dropped, data = self._node_bytes(run, node)
        whole = True
        if tail_lines is not None:
            tail_lines = max(tail_lines, 0)
            lines = data.splitlines(keepends=True)
            whole = tail_lines >= len(lines)
            data = b"".join(lines[len(lines) - tail_lines:]) if tail_lines else b""
        if dropped and whole:
            data = b"[log truncated: %d bytes dropped]\n" % dropped + data
        if prefix and data:
            data = _prefixed(data, node.display.encode() + b": ", True)
        return data


def _prefixed(data: bytes, prefix: bytes, at_line_start: bool) -> bytes:
    lines = data.splitlines(keepends=True)
    out = []
    for i, line in enumerate(lines):
        out.append(line if i == 0 and not at_line_start else prefix + line)
    return b"".join(out)


def _remove_if_empty(path: str) -> None:
    try:
        os.rmdir(path)
    except OSError:
        pass

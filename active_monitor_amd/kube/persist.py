"""On-disk journal for :class:`~.memory.MemoryApiServer` (opt-in).

A data directory holds three files:

- ``snapshot.jsonl`` — a header line ``{"format": 1, "rv": N, "count": M}``
  followed by the M objects, one per line, in store iteration order;
- ``journal.jsonl`` — append-only, one record per line:
  ``{"rv": N, "op": "put", "obj": {...}}`` or
  ``{"rv": N, "op": "del", "key": [apiVersion, kind, namespace, name]}``;
- ``lock`` — held with ``flock`` for the life of the store, so one process
  owns a directory.

Durability. Every record is written and flushed to the OS before the store
makes the mutation visible (write-ahead of visibility), so a process kill
(SIGKILL, OOM) loses nothing a caller or watcher has seen. ``fsync`` runs at
most once per ``sync_interval`` (a background thread syncs a dirty journal),
at compaction and on close, so a power loss or kernel crash can lose up to
one sync interval of writes.

An I/O error while journaling (disk full, EIO) is raised to the caller of the
mutation, and every later write is refused with :class:`StoreError`: the
store has applied that mutation in memory but it is not on disk, so the
process has to be restarted — it comes back with the last journaled state.

Loading reads the snapshot and replays the journal records whose rv is above
the snapshot's; older records are skipped, which makes a crash between
"snapshot renamed into place" and "journal reset" harmless. An incomplete or
unparsable LAST journal line is a torn tail from a crash mid-write: it is
dropped and the file truncated there. Damage anywhere else refuses to open
(:class:`StoreCorruptError`) — the middle of a journal is never discarded
silently.
"""
from __future__ import annotations

import fcntl
import json
import os
import threading
import time
from typing import Any, Callable, Dict, Iterable, Optional, Tuple

FORMAT_VERSION = 1
SNAPSHOT_FILE = "snapshot.jsonl"
SNAPSHOT_TMP_FILE = SNAPSHOT_FILE + ".tmp"
JOURNAL_FILE = "journal.jsonl"
LOCK_FILE = "lock"

Obj = Dict[str, Any]
Key = Tuple[str, str, str, str]


class StoreError(Exception):
    """Base class for data-directory failures."""


class StoreLockedError(StoreError):
    """Another process holds the data directory."""


class StoreCorruptError(StoreError):
    """A snapshot or journal that cannot be loaded; names the file and line."""

    def __init__(self, path: str, line: int, reason: str):
        super().__init__(f"{path}:{line}: {reason}")
        self.path = path
        self.line = line
        self.reason = reason


def _dumps(value: Any) -> bytes:
    return json.dumps(value, separators=(",", ":")).encode("utf-8") + b"\n"


def _fsync_dir(path: str) -> None:
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


class Journal:
    """The open data directory: lock, loader, appender, compactor."""

    def __init__(self, data_dir: str, sync_interval: float = 1.0,
                 compact_threshold: int = 4096):
        self.data_dir = os.path.abspath(data_dir)
        self.sync_interval = float(sync_interval)
        self.compact_threshold = int(compact_threshold)
        self.records = 0  # records in the journal file
        self.compactions = 0
        self.last_compaction_seconds = 0.0
        self._snapshot_path = os.path.join(self.data_dir, SNAPSHOT_FILE)
        self._tmp_path = os.path.join(self.data_dir, SNAPSHOT_TMP_FILE)
        self._journal_path = os.path.join(self.data_dir, JOURNAL_FILE)
        self._file = None
        self._failed: Optional[BaseException] = None  # first write error
        self._dirty = False
        self._io_lock = threading.Lock()  # file handle vs. the syncer thread
        self._stop = threading.Event()
        self._syncer: Optional[threading.Thread] = None

        os.makedirs(self.data_dir, exist_ok=True)
        self._lock_fd = os.open(os.path.join(self.data_dir, LOCK_FILE),
                                os.O_RDWR | os.O_CREAT, 0o644)
        try:
            fcntl.flock(self._lock_fd, fcntl.LOCK_EX | fcntl.LOCK_NB)
        except OSError:
            os.close(self._lock_fd)
            self._lock_fd = -1
            raise StoreLockedError(
                f"data directory {self.data_dir} is in use by another process"
            )

    # -- load --------------------------------------------------------------

    def load(self, key_of: Callable[[Obj], Key]) -> Tuple[int, Dict[Key, Obj]]:
        """Return ``(rv, objects)``; ``objects`` iterates in store order (a
        put of an existing key keeps its place, a new key appends). Opens the
        journal for appending afterwards."""
        try:
            os.unlink(self._tmp_path)  # a compaction that never finished
        except FileNotFoundError:
            pass
        objects: Dict[Key, Obj] = {}
        rv = self._load_snapshot(objects, key_of)
        rv = self._replay_journal(objects, key_of, rv)
        created = not os.path.exists(self._journal_path)
        self._file = open(self._journal_path, "ab")
        if created:
            # make the new directory entry durable too; fsync of the file
            # alone does not promise that on every filesystem
            _fsync_dir(self.data_dir)
        if self.sync_interval > 0:
            self._syncer = threading.Thread(
                target=self._sync_loop, name="store-journal-sync", daemon=True
            )
            self._syncer.start()
        return rv, objects

    def _load_snapshot(self, objects: Dict[Key, Obj],
                       key_of: Callable[[Obj], Key]) -> int:
        path = self._snapshot_path
        try:
            f = open(path, "rb")
        except FileNotFoundError:
            return 0
        with f:
            lines = f.read().split(b"\n")
        try:
            header = json.loads(lines[0])
            if not isinstance(header, dict):
                raise ValueError("header is not an object")
        except ValueError as e:
            raise StoreCorruptError(path, 1, f"unreadable snapshot header: {e}")
        if header.get("format") != FORMAT_VERSION:
            raise StoreCorruptError(
                path, 1, f"unknown format version {header.get('format')!r} "
                         f"(this build reads {FORMAT_VERSION})")
        rv, count = header.get("rv"), header.get("count")
        if not isinstance(rv, int) or not isinstance(count, int):
            raise StoreCorruptError(path, 1, "snapshot header lacks rv/count")
        if len(lines) < count + 1:
            raise StoreCorruptError(
                path, len(lines), f"snapshot ends after {len(lines) - 1} of "
                                  f"{count} objects")
        for n in range(1, count + 1):
            try:
                obj = json.loads(lines[n])
                if not isinstance(obj, dict):
                    raise ValueError("not an object")
            except ValueError as e:
                raise StoreCorruptError(path, n + 1, f"unreadable object: {e}")
            objects[key_of(obj)] = obj
        return rv

    @staticmethod
    def _parse_record(raw: bytes) -> Tuple[int, str, Any]:
        rec = json.loads(raw)
        if not isinstance(rec, dict):
            raise ValueError("record is not an object")
        rv, op = rec.get("rv"), rec.get("op")
        if not isinstance(rv, int) or isinstance(rv, bool):
            raise ValueError("record has no integer rv")
        if op == "put":
            if not isinstance(rec.get("obj"), dict):
                raise ValueError("put record has no object")
            return rv, op, rec["obj"]
        if op == "del":
            key = rec.get("key")
            if not isinstance(key, list) or len(key) != 4:
                raise ValueError("del record has no key")
            return rv, op, tuple(key)
        raise ValueError(f"unknown op {op!r}")

    def _replay_journal(self, objects: Dict[Key, Obj],
                        key_of: Callable[[Obj], Key], snapshot_rv: int) -> int:
        path = self._journal_path
        try:
            f = open(path, "rb")
        except FileNotFoundError:
            return snapshot_rv
        with f:
            data = f.read()
        lines = data.split(b"\n")
        # data ending in "\n" leaves one empty trailing element; anything
        # else there is a record whose write never completed
        tail = lines.pop()
        torn = bool(tail)
        good_bytes = len(data) - len(tail)
        rv = snapshot_rv
        self.records = 0
        for n, raw in enumerate(lines, start=1):
            try:
                rec_rv, op, payload = self._parse_record(raw)
            except ValueError as e:
                if n == len(lines) and not torn:
                    # unparsable final line: torn tail as well
                    good_bytes -= len(raw) + 1
                    torn = True
                    break
                raise StoreCorruptError(path, n, f"unreadable record: {e}")
            self.records += 1
            if rec_rv <= snapshot_rv:
                continue  # already in the snapshot
            if op == "put":
                objects[key_of(payload)] = payload
            else:
                objects.pop(payload, None)
            if rec_rv > rv:
                rv = rec_rv
        if torn:
            with open(path, "r+b") as f:
                f.truncate(good_bytes)
                f.flush()
                os.fsync(f.fileno())
        return rv

    # -- append ------------------------------------------------------------

    def put(self, rv: int, obj: Obj) -> None:
        self._append(_dumps({"rv": rv, "op": "put", "obj": obj}))

    def delete(self, rv: int, key: Key) -> None:
        self._append(_dumps({"rv": rv, "op": "del", "key": list(key)}))

    def _append(self, line: bytes) -> None:
        with self._io_lock:
            f = self._file
            if f is None:
                raise StoreError(f"data directory {self.data_dir} is closed")
            if self._failed is not None:
                raise StoreError(
                    f"data directory {self.data_dir}: an earlier write failed "
                    f"({self._failed}); restart the process")
            try:
                f.write(line)
                f.flush()  # in the OS: survives a kill of this process
                if self.sync_interval <= 0:
                    os.fsync(f.fileno())
            except OSError as e:
                # the record may be missing or half written: nothing may
                # follow it, or a restart would replay a history with a hole
                self._failed = e
                raise
            self.records += 1
            if self.sync_interval > 0:
                self._dirty = True

    def _sync_loop(self) -> None:
        while not self._stop.wait(self.sync_interval):
            if not self._dirty:
                continue
            with self._io_lock:
                if self._file is None:
                    return
                self._dirty = False
                try:
                    os.fsync(self._file.fileno())
                except OSError as e:
                    self._failed = e  # the next write reports it
                    return

    # -- compaction --------------------------------------------------------

    def should_compact(self, live_objects: int) -> bool:
        """Rewriting the snapshot costs one line per live object, so it is
        due only once the journal is longer than both the threshold and the
        snapshot it would write — amortised O(1) per mutation however large
        the fleet."""
        return self.records > self.compact_threshold and self.records > live_objects

    def compact(self, rv: int, objects: Iterable[Obj], count: int) -> None:
        """Snapshot to a temporary file, fsync, rename over the old snapshot,
        then start a fresh journal. A crash after the rename leaves the old
        journal beside the new snapshot; its records are skipped by rv."""
        started = time.monotonic()
        try:
            self._compact(rv, objects, count)
        except OSError as e:
            self._failed = e  # no telling how far it got: stop writing
            raise
        self.compactions += 1
        self.last_compaction_seconds = time.monotonic() - started

    def _compact(self, rv: int, objects: Iterable[Obj], count: int) -> None:
        with open(self._tmp_path, "wb") as f:
            f.write(_dumps({"format": FORMAT_VERSION, "rv": rv, "count": count}))
            for obj in objects:
                f.write(_dumps(obj))
            f.flush()
            os.fsync(f.fileno())
        os.replace(self._tmp_path, self._snapshot_path)
        _fsync_dir(self.data_dir)
        with self._io_lock:
            self._file.truncate(0)  # append mode: the next write lands at 0
            os.fsync(self._file.fileno())
            self._dirty = False
            self.records = 0

    # -- close -------------------------------------------------------------

    @property
    def closed(self) -> bool:
        return self._lock_fd < 0

    def close(self) -> None:
        self._stop.set()
        with self._io_lock:
            f, self._file = self._file, None
            if f is not None:
                f.flush()
                os.fsync(f.fileno())
                f.close()
        if self._syncer is not None and self._syncer is not threading.current_thread():
            self._syncer.join(timeout=5)
            self._syncer = None
        if self._lock_fd >= 0:
            fcntl.flock(self._lock_fd, fcntl.LOCK_UN)
            os.close(self._lock_fd)
            self._lock_fd = -1

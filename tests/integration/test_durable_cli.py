"""``--data-dir`` on the two command lines: a standalone apiserver finds its
objects again after a restart, and a directory that is held or unreadable
stops the process instead of starting an empty store over it."""
import asyncio
import json
import os
import subprocess
import sys

import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.kube import MemoryApiServer
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.persist import JOURNAL_FILE

from .conftest import make_hc

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STANDALONE = [sys.executable, "-m", "active_monitor_amd.kube.standalone"]


async def start_standalone(data_dir):
    proc = await asyncio.create_subprocess_exec(
        *STANDALONE, "--data-dir", data_dir, "--engine", "none",
        stdout=asyncio.subprocess.PIPE, stderr=asyncio.subprocess.PIPE, cwd=REPO,
    )
    line = await asyncio.wait_for(proc.stdout.readline(), 60)
    assert line.startswith(b"READY "), (line, await proc.stderr.read())
    return proc, json.loads(line[len(b"READY "):])["url"]


async def sigterm(proc):
    proc.terminate()
    try:
        _, err = await asyncio.wait_for(proc.communicate(), 20)
    except asyncio.TimeoutError:
        proc.kill()
        await proc.wait()
        raise AssertionError("standalone did not stop on SIGTERM")
    return proc.returncode, err.decode()


async def restart_round_trip(data_dir):
    """Create a HealthCheck over HTTP, SIGTERM the server, start it again on
    the same directory and read the HealthCheck back."""
    proc, url = await start_standalone(data_dir)
    try:
        client = HttpClient(url, qps=0)
        await client.start()
        try:
            made = await asyncio.wait_for(client.create(make_hc(name="kept")), 10)
        finally:
            await client.close()
    finally:
        rc, first_log = await sigterm(proc)
    assert rc == 0, first_log
    assert "loaded 0 objects, resourceVersion 0" in first_log

    proc, url = await start_standalone(data_dir)
    try:
        client = HttpClient(url, qps=0)
        await client.start()
        try:
            back = await asyncio.wait_for(
                client.get(API_VERSION, "HealthCheck", "health", "kept"), 10)
        finally:
            await client.close()
    finally:
        rc, second_log = await sigterm(proc)
    assert rc == 0, second_log
    assert os.path.abspath(data_dir) in second_log
    assert "loaded 1 objects, resourceVersion 1" in second_log
    assert back["metadata"]["uid"] == made["metadata"]["uid"]
    assert back["spec"] == made["spec"]
    assert back == made


def test_standalone_keeps_a_healthcheck_across_a_restart(tmp_path, run):
    run(restart_round_trip(str(tmp_path / "data")), timeout=120)


def test_controller_rejects_data_dir_with_http_backend(tmp_path):
    out = subprocess.run(
        [sys.executable, "-m", "active_monitor_amd.cmd.main", "--backend", "http",
         "--server", "http://127.0.0.1:1", "--data-dir", str(tmp_path / "data")],
        capture_output=True, text=True, timeout=60, cwd=REPO,
    )
    assert out.returncode == 2, out.stderr  # argparse's argument-error status
    assert "--data-dir" in out.stderr and "usage:" in out.stderr
    assert not (tmp_path / "data").exists()


def test_held_directory_stops_a_second_standalone(tmp_path):
    d = str(tmp_path / "data")
    holder = MemoryApiServer.open(d)
    try:
        out = subprocess.run(STANDALONE + ["--data-dir", d, "--engine", "none"],
                             capture_output=True, text=True, timeout=60, cwd=REPO)
    finally:
        holder.close()
    assert out.returncode == 1, out.stderr
    assert d in out.stderr and "in use" in out.stderr
    assert "READY" not in out.stdout


def _corrupt_directory(tmp_path):
    d = str(tmp_path / "data")
    server = MemoryApiServer.open(d)
    for i in range(3):
        server.create({"apiVersion": "v1", "kind": "ConfigMap",
                       "metadata": {"name": f"cm-{i}", "namespace": "health"}})
    server.close()
    journal = os.path.join(d, JOURNAL_FILE)
    with open(journal, "rb") as f:
        lines = f.read().split(b"\n")
    lines[1] = b"{{{{"
    with open(journal, "wb") as f:
        f.write(b"\n".join(lines))
    return d, journal


def test_corrupt_directory_stops_standalone(tmp_path):
    d, journal = _corrupt_directory(tmp_path)
    out = subprocess.run(STANDALONE + ["--data-dir", d, "--engine", "none"],
                         capture_output=True, text=True, timeout=60, cwd=REPO)
    assert out.returncode == 1, out.stderr
    assert f"{journal}:2:" in out.stderr
    assert "READY" not in out.stdout


@pytest.mark.parametrize("problem", ["corrupt", "held"])
def test_controller_exits_1_on_an_unusable_directory(tmp_path, problem):
    holder = None
    if problem == "corrupt":
        d, journal = _corrupt_directory(tmp_path)
        expect = f"{journal}:2:"
    else:
        d = str(tmp_path / "data")
        holder = MemoryApiServer.open(d)
        expect = d
    try:
        out = subprocess.run(
            [sys.executable, "-m", "active_monitor_amd.cmd.main", "--data-dir", d,
             "--metrics-bind-address", "0", "--health-probe-bind-address", "0"],
            capture_output=True, text=True, timeout=60, cwd=REPO,
        )
    finally:
        if holder is not None:
            holder.close()
    assert out.returncode == 1, out.stderr
    assert expect in out.stderr


# -- what both entry points say and do at start ------------------------------

CONTROLLER = [sys.executable, "-m", "active_monitor_amd.cmd.main", "--backend", "memory",
              "--metrics-bind-address", "0", "--health-probe-bind-address", "0"]
ENTRY_POINTS = {
    "controller": CONTROLLER + ["--serve-api", "127.0.0.1:0"],
    "standalone": STANDALONE + ["--engine", "local"],
}
SCHEMA_ON = "schema validation: HealthCheck (activemonitor.keikoproj.io/v1alpha1)"
WF = ("argoproj.io/v1alpha1", "Workflow")


def _clean_env():
    return {k: v for k, v in os.environ.items() if k != "AM_SCHEMA_VALIDATION"}


def _said(which, log, level, message):
    """Index of the log line that carries exactly ``message``: the standalone
    apiserver prints it bare, the controller through its ``main`` logger."""
    lines = log.splitlines()
    if which == "standalone":
        hits = [i for i, l in enumerate(lines) if l == message]
    else:
        tail = f" {level} active_monitor_amd.main {message}"
        hits = [i for i, l in enumerate(lines) if l.endswith(tail)]
    assert len(hits) == 1, (message, log)
    return hits[0]


async def _start_entry_point(which, *argv):
    """Start the process and read up to the line that names its URL."""
    proc = await asyncio.create_subprocess_exec(
        *ENTRY_POINTS[which], *argv, cwd=REPO, env=_clean_env(),
        stdout=asyncio.subprocess.PIPE, stderr=asyncio.subprocess.PIPE,
    )
    if which == "standalone":
        line = await asyncio.wait_for(proc.stdout.readline(), 60)
        assert line.startswith(b"READY "), (line, await proc.stderr.read())
        return proc, json.loads(line[len(b"READY "):])["url"], ""
    head = b""
    while True:
        line = await asyncio.wait_for(proc.stderr.readline(), 60)
        assert line, head  # end of stream: it died before serving
        head += line
        if b" serving Kubernetes REST API at " in line:
            return proc, line.split()[-1].decode(), head.decode()


@pytest.mark.parametrize("which", ["controller", "standalone"])
def test_entry_point_on_an_existing_directory(tmp_path, run, which):
    """The schema line, the count of what was loaded, and an engine built
    with ``recover=True``: a workflow the last process left Running is failed
    as interrupted, not run again."""
    d = str(tmp_path / "data")
    left = MemoryApiServer.open(d)
    left.create({"apiVersion": "v1", "kind": "ConfigMap",
                 "metadata": {"name": "cm", "namespace": "health"}})
    left.create({"apiVersion": WF[0], "kind": WF[1],
                 "metadata": {"name": "cut-off", "namespace": "health"},
                 "spec": {"entrypoint": "main", "templates": [
                     {"name": "main", "container": {"command": ["true"]}}]},
                 "status": {"phase": "Running", "startedAt": "2024-01-01T00:00:00Z"}})
    left.close()

    async def go():
        proc, url, head = await _start_entry_point(which, "--data-dir", d)
        try:
            client = HttpClient(url, qps=0)
            await client.start()
            try:
                deadline = asyncio.get_running_loop().time() + 10
                while True:
                    wf = await asyncio.wait_for(client.get(*WF, "health", "cut-off"), 10)
                    if wf["status"]["phase"] != "Running":
                        break
                    assert asyncio.get_running_loop().time() < deadline, wf
                    await asyncio.sleep(0.02)
            finally:
                await client.close()
        finally:
            rc, rest = await sigterm(proc)
        assert rc == 0, rest
        return wf, head + rest

    wf, log = run(go(), timeout=120)
    assert wf["status"]["phase"] == "Failed"
    assert wf["status"]["message"] == "workflow interrupted: engine restarted"
    first = _said(which, log, "INFO", SCHEMA_ON)
    second = _said(which, log, "INFO",
                   f"data directory {d}: loaded 2 objects, resourceVersion 2")
    assert first < second


@pytest.mark.parametrize("which", ["controller", "standalone"])
def test_entry_point_on_a_held_directory(tmp_path, which):
    d = str(tmp_path / "data")
    holder = MemoryApiServer.open(d)
    try:
        out = subprocess.run(
            ENTRY_POINTS[which] + ["--data-dir", d, "--no-schema-validation"],
            capture_output=True, text=True, timeout=60, cwd=REPO, env=_clean_env())
    finally:
        holder.close()
    assert out.returncode == 1, out.stderr
    first = _said(which, out.stderr, "INFO", "schema validation: off")
    second = _said(which, out.stderr, "ERROR",
                   f"cannot open data directory: data directory {d} "
                   "is in use by another process")
    assert first < second
    assert "loaded" not in out.stderr
    assert "READY" not in out.stdout and "serving" not in out.stderr

"""The wire path with the native codec and with the Python one must be the
same wire: a small bench-mix fleet run through HttpClient and
ApiServerFrontend persists identical status counters either way, and the
special paths of the HTTP handler (401 with keep-alive, Expect/100-continue,
Table, an over-long head, watch replay) answer identically.

Each mode runs in a fresh subprocess, because ``AM_WIRE_NATIVE`` is read when
``utils/wirecodec.py`` is imported. Run as a script, this file is that
subprocess: it prints one JSON line of observations."""
import asyncio
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NS = "health"
TOKEN = "parity-token"
# bench.py's mix (make_cr decides by index % 100): 20% failing-with-remedy,
# 30% cron, 50% repeatAfterSec
FLEET = list(range(0, 6)) + list(range(20, 29)) + list(range(50, 65))
WAVES = 2


# -- the subprocess -------------------------------------------------------------

async def _read_response(reader):
    head = await reader.readuntil(b"\r\n\r\n")
    lines = head.decode("latin-1").split("\r\n")
    status = int(lines[0].split(" ")[1])
    headers = {k.lower(): v.strip() for k, v in
               (ln.split(":", 1) for ln in lines[1:] if ln)}
    body = await reader.readexactly(int(headers.get("content-length", 0)))
    return status, headers, body


async def _special_paths(frontend, client, hc_path):
    port = frontend.port
    auth = f"Authorization: Bearer {TOKEN}\r\n"
    seen = {}

    # 401, then an authorized request on the same connection
    r, w = await asyncio.open_connection("127.0.0.1", port)
    w.write(f"GET {hc_path} HTTP/1.1\r\nHost: x\r\nContent-Length: 2\r\n\r\n{{}}".encode())
    status, headers, body = await _read_response(r)
    seen["unauthorized"] = [status, headers.get("www-authenticate"),
                            json.loads(body)["reason"]]
    w.write(f"GET {hc_path}/hc-00000 HTTP/1.1\r\nHost: x\r\n{auth}\r\n".encode())
    status, headers, body = await _read_response(r)
    seen["after_401_same_connection"] = [status, json.loads(body)["metadata"]["name"]]
    seen["unauthorized_count"] = frontend.unauthorized_count

    # Expect: 100-continue on the still-open connection (curl-style names)
    doc = json.dumps({"apiVersion": "v1", "kind": "ConfigMap",
                      "metadata": {"name": "big", "namespace": NS},
                      "data": {"k": "v" * 2000}}, indent=2).encode()
    w.write((f"POST /api/v1/namespaces/{NS}/configmaps HTTP/1.1\r\nhost: x\r\n"
             f"authorization: Bearer {TOKEN}\r\ncontent-type: application/json\r\n"
             f"content-length: {len(doc)}\r\nEXPECT: 100-continue\r\n\r\n").encode())
    interim = await r.readuntil(b"\r\n\r\n")
    w.write(doc)
    status, headers, body = await _read_response(r)
    seen["expect_continue"] = [interim.decode(), status,
                               len(json.loads(body)["data"]["k"])]

    # Table
    w.write((f"GET {hc_path}?limit=500 HTTP/1.1\r\nHost: x\r\n{auth}"
             "Accept: application/json;as=Table;v=v1;g=meta.k8s.io,application/json\r\n"
             "\r\n").encode())
    status, headers, body = await _read_response(r)
    table = json.loads(body)
    seen["table"] = [status, table["kind"], len(table["rows"]),
                     [c["name"] for c in table["columnDefinitions"]][:3],
                     table["rows"][0]["cells"][0]]
    w.close()

    # a 70 KB head: the connection is closed without an answer
    r, w = await asyncio.open_connection("127.0.0.1", port)
    w.write(f"GET {hc_path} HTTP/1.1\r\nHost: x\r\n{auth}X-Pad: ".encode()
            + b"a" * 70_000 + b"\r\n\r\n")
    try:
        answer = await asyncio.wait_for(r.read(), 10)
    except ConnectionError:
        answer = b""
    seen["long_head"] = answer.decode("latin-1")
    w.close()

    # watch: replay of current state, then resume from a resourceVersion
    r, w = await asyncio.open_connection("127.0.0.1", port)
    w.write(f"GET {hc_path}?watch=true HTTP/1.1\r\nHost: x\r\n{auth}\r\n".encode())
    head = await r.readuntil(b"\r\n\r\n")
    events = [json.loads(await r.readline()) for _ in FLEET]
    seen["watch_replay"] = [
        head.decode(), sorted({e["type"] for e in events}),
        sorted(e["object"]["metadata"]["name"] for e in events)
        == sorted(f"hc-{i:05d}" for i in FLEET)]
    w.close()
    listing = await client._request("GET", hc_path)
    rv = listing["metadata"]["resourceVersion"]
    import bench

    extra, _ = bench.make_cr(99, NS, 0.3, 0.2)
    await client.create(extra)
    r, w = await asyncio.open_connection("127.0.0.1", port)
    w.write((f"GET {hc_path}?watch=true&resourceVersion={rv} HTTP/1.1\r\n"
             f"Host: x\r\n{auth}\r\n").encode())
    await r.readuntil(b"\r\n\r\n")
    ev = json.loads(await r.readline())
    seen["watch_resume"] = [ev["type"], ev["object"]["metadata"]["name"]]
    w.close()
    return seen


async def _fleet():
    import bench
    from active_monitor_amd.engine import Manager
    from active_monitor_amd.kube import MemoryApiServer, MemoryClient
    from active_monitor_amd.kube.http import HttpClient
    from active_monitor_amd.kube.server import ApiServerFrontend
    from active_monitor_amd.kube.standalone import bench_policy
    from active_monitor_amd.utils import wirecodec
    from active_monitor_amd.workflow import ScriptedWorkflowEngine

    server = MemoryApiServer()
    frontend = ApiServerFrontend(server, accepted_tokens={TOKEN})
    await frontend.start()
    engine = ScriptedWorkflowEngine(MemoryClient(server), policy=bench_policy(0.2))
    await engine.start()
    client = HttpClient(frontend.url, token=TOKEN, qps=0)
    await client.start()
    manager = Manager(client, max_workers=4)
    await manager.start()

    names = []
    for i in FLEET:
        cr, _ = bench.make_cr(i, NS, 0.3, 0.2)
        names.append(cr["metadata"]["name"])
        await client.create(cr)
    rec = manager.reconciler
    done = len(FLEET)  # creation-triggered first runs
    for wave in range(WAVES + 1):
        if wave:
            for name in names:
                manager.queue.add_nowait((NS, name), {"timer"})
            done += len(FLEET)
        while rec.completed_runs < done:
            await asyncio.sleep(0.005)
    await manager.stop()

    objs = await client.list("activemonitor.keikoproj.io/v1alpha1", "HealthCheck", NS)
    objs.sort(key=lambda o: o["metadata"]["name"])
    rows = [[o["metadata"]["name"]]
            + [(o.get("status") or {}).get(col) or 0 for col in bench.STATUS_COLUMNS]
            + [(o.get("status") or {}).get(key) == want
               for key, want in bench.STATUS_STRINGS]
            for o in objs]
    hc_path = client._collection_path(
        "activemonitor.keikoproj.io/v1alpha1", "HealthCheck", NS)
    special = await _special_paths(frontend, client, hc_path)
    await client.close()
    await engine.stop()
    await frontend.stop()
    print(json.dumps({"native": wirecodec.NATIVE, "rows": rows, "special": special}))


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    asyncio.run(asyncio.wait_for(_fleet(), 90))
    sys.exit(0)


# -- the tests ------------------------------------------------------------------

_RESULTS = {}


def _observed(mode: str) -> dict:
    """One subprocess run per codec mode, shared by the tests below."""
    if mode not in _RESULTS:
        out = subprocess.run(
            [sys.executable, os.path.abspath(__file__)], cwd=REPO,
            capture_output=True, text=True, timeout=120,
            env=dict(os.environ, AM_WIRE_NATIVE=mode, AM_REQUIRE_NATIVE="1"),
        )
        assert out.returncode == 0, out.stderr[-3000:]
        _RESULTS[mode] = json.loads(out.stdout.strip().splitlines()[-1])
    return _RESULTS[mode]


def test_each_mode_runs_the_codec_it_says():
    assert _observed("0")["native"] is False
    assert _observed("1")["native"] is True


def test_persisted_status_counters_are_identical():
    py, native = _observed("0"), _observed("1")
    assert native["rows"] == py["rows"]
    rows = {r[0]: r[1:] for r in native["rows"]}
    assert len(rows) == len(FLEET)
    # successCount, failedCount, remedySuccessCount, remedyFailedCount,
    # remedyTotalRuns, totalHealthCheckRuns, status ok, remedyStatus ok
    runs = WAVES + 1
    assert rows["hc-00000"] == [0, runs, runs, 0, runs, runs, False, True]
    assert rows["hc-00020"] == [runs, 0, 0, 0, 0, runs, True, False]
    assert rows["hc-00050"] == [runs, 0, 0, 0, 0, runs, True, False]


def test_special_paths_answer_identically():
    py, native = _observed("0")["special"], _observed("1")["special"]
    assert native == py
    assert native["unauthorized"] == [401, "Bearer", "Unauthorized"]
    assert native["after_401_same_connection"] == [200, "hc-00000"]
    assert native["unauthorized_count"] == 1
    assert native["expect_continue"] == ["HTTP/1.1 100 Continue\r\n\r\n", 201, 2000]
    assert native["table"] == [200, "Table", len(FLEET),
                               ["Name", "LATEST STATUS", "SUCCESS CNT  "], "hc-00000"]
    assert native["long_head"] == ""
    assert native["watch_replay"] == [
        "HTTP/1.1 200 OK\r\nContent-Type: application/json;stream=watch\r\n"
        "Connection: close\r\n\r\n", ["ADDED"], True]
    assert native["watch_resume"] == ["ADDED", "hc-00099"]

"""GPU-box validation of exec credential plugins.

Like the other test_gpu_host files this validates the host, not a kernel:
credential plugins are child processes of the controller's event loop, and
this makes sure they start and are reaped normally there. It is the
revoked-token round trip against a ``standalone --token-file`` apiserver in
its own process: the server accepts only ``tok-2``, the plugin's first answer
``tok-1`` is refused, the client refreshes once and the create goes through.
Nothing here touches the device.
"""
import asyncio
import json
import os
import sys

import pytest

from active_monitor_amd.kube.auth import ExecPluginSource
from active_monitor_amd.kube.config import load_kubeconfig
from active_monitor_amd.kube.errors import UnauthorizedError
from active_monitor_amd.kube.http import HttpClient
from tests.credplugin import exec_stanza, runs, write_kubeconfig, write_plugin

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_exec_plugin_round_trip_on_gpu_host(run, tmp_path):
    accepted = tmp_path / "accepted-tokens"
    accepted.write_text("tok-2\n\nsome-other-client\n")
    counter = tmp_path / "counter"
    pidfile = tmp_path / "plugin-pid"

    async def go():
        server = await asyncio.create_subprocess_exec(
            sys.executable, "-m", "active_monitor_amd.kube.standalone",
            "--token-file", str(accepted),
            stdout=asyncio.subprocess.PIPE, cwd=REPO,
        )
        client = None
        try:
            line = await asyncio.wait_for(server.stdout.readline(), 20)
            assert line.startswith(b"READY "), line
            url = json.loads(line[len(b"READY "):])["url"]

            cfg = load_kubeconfig(write_kubeconfig(
                tmp_path,
                {"exec": exec_stanza(write_plugin(tmp_path), counter,
                                     env={"FAKE_PIDFILE": pidfile})},
                server=url,
            ))
            assert isinstance(cfg.credential_source, ExecPluginSource)
            cfg.credential_source.timeout = 10.0
            client = cfg.make_client()
            await client.start()

            anon = HttpClient(url, qps=0)
            await anon.start()
            try:
                await asyncio.wait_for(anon.ping(), 5)  # /version is open
                with pytest.raises(UnauthorizedError):
                    await asyncio.wait_for(anon.list("v1", "ConfigMap", "health"), 5)
            finally:
                await anon.close()

            made = await asyncio.wait_for(client.create({
                "apiVersion": "v1", "kind": "ConfigMap",
                "metadata": {"name": "authed", "namespace": "health"},
            }), 20)
            assert made["metadata"]["name"] == "authed"
            assert runs(counter) == 2
            items = await asyncio.wait_for(client.list("v1", "ConfigMap", "health"), 5)
            assert [i["metadata"]["name"] for i in items] == ["authed"]
            assert runs(counter) == 2
        finally:
            if client is not None:
                await client.close()
            server.terminate()
            try:
                await asyncio.wait_for(server.wait(), 5)
            except asyncio.TimeoutError:
                server.kill()
                await server.wait()

    run(go(), timeout=60)
    # the last plugin child was reaped, not left as a zombie
    with pytest.raises(ProcessLookupError):
        os.kill(int(pidfile.read_text()), 0)

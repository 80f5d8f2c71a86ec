"""GPU-box validation of the watch's Replace after a re-list.

Like the other test_gpu_host files this validates the host, not a kernel:
restarting a loopback listener on a fixed port and the timing of the watch's
reconnect are what depends on the host, so the missed-deletion scenario of
test_deleted_healthcheck.py runs once on the benchmark host, over the native
wire codec. Nothing here touches the device.
"""
import asyncio

import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.utils import wirecodec

from .conftest import make_hc
from .test_deleted_healthcheck import KIND, WireEnv

pytestmark = pytest.mark.gpu


def test_missed_deletion_does_not_resurrect_on_gpu_host(run):
    assert wirecodec.NATIVE, "the wire path must run on the C codec here"

    async def go():
        async with WireEnv() as env:
            created = await env.client.create(make_hc(name="gpu-ghost", repeat=1))
            uid = created["metadata"]["uid"]
            await env.until(lambda: env.rec.completed_runs >= 1, "the first run")
            assert ("health", "gpu-ghost") in env.manager.hc_cache

            await env.outage(
                lambda: env.store.delete(API_VERSION, KIND, "health", "gpu-ghost"))

            await env.until(
                lambda: ("health", "gpu-ghost") not in env.manager.hc_cache
                and env.rec.get_timer_by_name("gpu-ghost", "health") is None,
                "the cache entry and the repeat timer to go", timeout=5.0)
            assert env.manager._sub.synthetic_deletes == 1
            # the repeat interval is 1 s: a check still driven submits again
            # (a workflow submitted for an owner that is gone is not
            # garbage-collected with it, so it would stay to be counted)
            first = len(env.owned_workflows(uid))
            reconciles = env.rec.reconcile_count
            await asyncio.sleep(2.5)
            assert len(env.owned_workflows(uid)) == first
            assert env.rec.reconcile_count == reconciles
            assert env.rec.active_watches() == 0

    run(go(), timeout=30)

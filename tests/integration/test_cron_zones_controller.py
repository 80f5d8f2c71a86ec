"""Cron time zones through the controller: a ``CRON_TZ=`` schedule runs and
re-arms, the controller-wide default zone reaches both places that derive
``RepeatAfterSec``, and a bad zone is a per-CR parse failure in a spec but a
start-up error on the command line."""
import asyncio
import json
import socket
import urllib.request

import pytest

from active_monitor_amd.cmd.main import build_parser
from active_monitor_amd.cmd.main import main as cli_main
from active_monitor_amd.cmd.main import run as cli_run
from active_monitor_amd.engine import CronParseError, Manager, seconds_until_next
from active_monitor_amd.workflow import always_succeed

from .conftest import Env, make_hc

EVENT = ("v1", "Event")


class ZonedEnv(Env):
    """``Env`` whose Manager is given a controller-wide cron time zone."""

    def __init__(self, cron_time_zone=None, **kw):
        super().__init__(**kw)
        self.manager = Manager(self.client, max_workers=4, cron_time_zone=cron_time_zone)

    async def event_messages(self, ns="health"):
        await self.manager.recorder.flush()
        return [e.get("message") for e in await self.client.list(*EVENT, ns)]

    def armed_delay(self, name, ns="health"):
        timer = self.manager.reconciler.get_timer_by_name(name, ns)
        assert timer is not None and timer.handle is not None and not timer.fired
        return timer.handle.when() - asyncio.get_running_loop().time()


async def first_success(env, name):
    async def succeeded():
        hc = await env.get_hc(name)
        return hc.status.success_count >= 1 and hc

    return await env.wait_for(succeeded, msg=f"first successful run of {name}")


def test_prefixed_schedule_runs_and_rearms(run):
    async def go():
        async with ZonedEnv(policy=always_succeed) as env:
            await env.create_hc(make_hc(name="tokyo", repeat=0,
                                        cron="CRON_TZ=Asia/Tokyo * * * * *"))
            hc = await first_success(env, "tokyo")
            assert hc.status.status == "Succeeded"
            assert hc.status.success_count == 1
            assert 0 < env.armed_delay("tokyo") <= 61
            assert "Fail to parse cron" not in await env.event_messages()
            assert len(await env.workflows()) == 1

    run(go(), timeout=30)


def test_controller_wide_zone_applies_to_a_bare_schedule(run):
    async def go():
        async with ZonedEnv(cron_time_zone="Asia/Kolkata", policy=always_succeed) as env:
            assert env.manager.reconciler.cron_time_zone == "Asia/Kolkata"
            await env.create_hc(make_hc(name="nine", repeat=0, cron="0 9 * * *"))
            await first_success(env, "nine")
            # armed at completion (_finish_and_reschedule), moments ago
            want = seconds_until_next("0 9 * * *", default_zone="Asia/Kolkata")
            assert abs(env.armed_delay("nine") - want) <= 2.0
            # 09:00 in Kolkata is not 09:00 on a clock 5h30 away from it
            assert abs(want - seconds_until_next("CRON_TZ=UTC 0 9 * * *")) > 3600

    run(go(), timeout=30)


def test_a_prefix_beats_the_controller_wide_zone(run):
    async def go():
        async with ZonedEnv(cron_time_zone="Asia/Kolkata", policy=always_succeed) as env:
            await env.create_hc(make_hc(name="tokyo9", repeat=0,
                                        cron="CRON_TZ=Asia/Tokyo 0 9 * * *"))
            await first_success(env, "tokyo9")
            want = seconds_until_next("CRON_TZ=Asia/Tokyo 0 9 * * *")
            assert abs(env.armed_delay("tokyo9") - want) <= 2.0

    run(go(), timeout=30)


def test_bad_location_in_a_spec_is_a_parse_failure_for_that_cr(run, caplog):
    async def go():
        async with ZonedEnv(policy=always_succeed) as env:
            await env.create_hc(make_hc(name="mars", repeat=0,
                                        cron="CRON_TZ=Mars/Olympus * * * * *"))

            async def warned():
                return "Fail to parse cron" in await env.event_messages()

            await env.wait_for(warned, msg="Fail to parse cron event")
            assert await env.workflows() == []
            hc = await env.get_hc("mars")
            assert hc.status.success_count == 0 and hc.status.failed_count == 0

    with caplog.at_level("WARNING", logger="active_monitor_amd.reconciler"):
        run(go(), timeout=30)
    assert any("provided bad location Mars/Olympus" in r.getMessage()
               for r in caplog.records)


def test_manager_refuses_an_unknown_zone():
    with pytest.raises(CronParseError) as e:
        ZonedEnv(cron_time_zone="Mars/Olympus")
    assert "Mars/Olympus" in str(e.value)
    assert ZonedEnv(cron_time_zone="Local").manager.reconciler.cron_time_zone is None
    assert ZonedEnv().manager.reconciler.cron_time_zone is None


def test_flag_with_an_unknown_zone_is_an_argument_error(capsys):
    with pytest.raises(SystemExit) as e:
        cli_main(["--cron-time-zone", "Mars/Olympus"])
    assert e.value.code == 2
    assert "Mars/Olympus" in capsys.readouterr().err


def test_flag_defaults_to_the_environment(monkeypatch):
    monkeypatch.delenv("AM_CRON_TIME_ZONE", raising=False)
    assert build_parser().parse_args([]).cron_time_zone is None
    monkeypatch.setenv("AM_CRON_TIME_ZONE", "Europe/London")
    assert build_parser().parse_args([]).cron_time_zone == "Europe/London"
    assert build_parser().parse_args(
        ["--cron-time-zone", "Asia/Tokyo"]).cron_time_zone == "Asia/Tokyo"
    monkeypatch.setenv("AM_CRON_TIME_ZONE", "Mars/Olympus")
    with pytest.raises(SystemExit) as e:
        cli_main([])
    assert e.value.code == 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _statusz(port):
    with urllib.request.urlopen(f"http://127.0.0.1:{port}/statusz", timeout=5) as r:
        return json.loads(r.read())


@pytest.mark.parametrize("flags,want", [
    (["--cron-time-zone", "Asia/Kolkata"], "Asia/Kolkata"),
    ([], None),
], ids=["set", "unset"])
def test_statusz_reports_the_zone(run, monkeypatch, flags, want):
    monkeypatch.delenv("AM_CRON_TIME_ZONE", raising=False)

    async def go():
        port = _free_port()
        args = build_parser().parse_args([
            "--backend", "memory", "--workflow-engine", "none",
            "--metrics-bind-address", f"127.0.0.1:{port}", "--no-metrics-secure",
            "--health-probe-bind-address", "0", *flags,
        ])
        stop = asyncio.Event()
        task = asyncio.ensure_future(cli_run(args, stop))
        loop = asyncio.get_running_loop()
        try:
            deadline = loop.time() + 10
            stats = None
            while stats is None:
                try:
                    stats = await loop.run_in_executor(None, _statusz, port)
                except OSError:
                    assert loop.time() < deadline, "statusz never answered"
                    await asyncio.sleep(0.05)
            assert "cron_time_zone" in stats
            assert stats["cron_time_zone"] == want
        finally:
            stop.set()
            assert await asyncio.wait_for(task, 15) == 0

    run(go(), timeout=40)

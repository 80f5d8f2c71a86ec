"""Cron schedules in a named time zone: the TZ=/CRON_TZ= prefix grammar and
the zone-aware ``Schedule.next`` across daylight-saving changes, held against
pinned instants and an independent minute-by-minute oracle."""
import time
from datetime import datetime, timedelta, timezone
from zoneinfo import ZoneInfo

import pytest

from active_monitor_amd.engine.cronx import (
    CronParseError,
    parse_standard,
    seconds_until_next,
)
from tests.cron_zone_cases import PINNED, ZONES, instant

UTC = timezone.utc


# ---------------------------------------------------------------------------
# pinned instants
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec,after,expected", PINNED)
def test_pinned_instant(spec, after, expected):
    after = instant(after)
    got = parse_standard(spec).next(after)
    assert got == instant(expected), got.astimezone(UTC).isoformat()
    assert got.tzinfo is after.tzinfo
    assert got.second == 0 and got.microsecond == 0


def test_result_keeps_a_zoneinfo_tzinfo():
    tokyo = ZoneInfo("Asia/Tokyo")
    after = datetime(2026, 6, 1, 12, 0, tzinfo=tokyo)
    got = parse_standard("CRON_TZ=Asia/Tokyo @daily").next(after)
    assert got.tzinfo is tokyo
    assert got == datetime(2026, 6, 2, 0, 0, tzinfo=tokyo)  # midnight in Tokyo
    assert got.astimezone(UTC) == datetime(2026, 6, 1, 15, 0, tzinfo=UTC)


# ---------------------------------------------------------------------------
# agreement with a minute-by-minute oracle that has its own field sets
# ---------------------------------------------------------------------------

EVERY_DAY = None
#: spec -> (minutes, hours, cron days of week or EVERY_DAY); all fire at least
#: every day the day-of-week field admits
SCHEDULES = {
    "*/15 * * * *": ({0, 15, 30, 45}, set(range(24)), EVERY_DAY),
    "30 2 * * *": ({30}, {2}, EVERY_DAY),
    "0 0 * * *": ({0}, {0}, EVERY_DAY),
    "45 23 * * MON-FRI": ({45}, {23}, {1, 2, 3, 4, 5}),
    "0 1,2,3 * * *": ({0}, {1, 2, 3}, EVERY_DAY),
    "59 23 * * *": ({59}, {23}, EVERY_DAY),
    "0 */6 * * *": ({0}, {0, 6, 12, 18}, EVERY_DAY),
    "*/20 0-4 * * *": ({0, 20, 40}, {0, 1, 2, 3, 4}, EVERY_DAY),
}

#: the two instants of 2026 at which each zone changes its offset (Kolkata has
#: none: any two instants)
TRANSITIONS = {
    "America/New_York": ("2026-03-08T07:00:00+00:00", "2026-11-01T06:00:00+00:00"),
    "Europe/London": ("2026-03-29T01:00:00+00:00", "2026-10-25T01:00:00+00:00"),
    "Australia/Lord_Howe": ("2026-04-04T15:00:00+00:00", "2026-10-03T15:30:00+00:00"),
    "America/Havana": ("2026-03-08T05:00:00+00:00", "2026-11-01T05:00:00+00:00"),
    "Asia/Kolkata": ("2026-01-01T00:00:00+00:00", "2026-07-01T12:00:00+00:00"),
}

#: twelve start instants around each transition, some off the whole minute
AROUND = tuple(timedelta(**kw) for kw in (
    dict(hours=-49), dict(hours=-25, seconds=17), dict(hours=-3),
    dict(minutes=-61), dict(minutes=-31, seconds=30), dict(minutes=-1),
    dict(), dict(minutes=1), dict(minutes=29, seconds=59), dict(minutes=59),
    dict(hours=2), dict(hours=26, microseconds=5),
))


def starts(zone):
    return [instant(t) + d for t in TRANSITIONS[zone] for d in AROUND]


def oracle_next(fields, zone, after):
    """First whole minute strictly after ``after`` whose wall clock in
    ``zone`` matches; one zone conversion per minute, no skipping."""
    minutes, hours, days = fields
    t = after.replace(second=0, microsecond=0) + timedelta(minutes=1)
    for _ in range(8 * 24 * 60):
        w = t.astimezone(zone)
        if (w.minute in minutes and w.hour in hours
                and (days is EVERY_DAY or w.isoweekday() % 7 in days)):
            return t
        t += timedelta(minutes=1)
    raise AssertionError("oracle found nothing within eight days")


def test_transition_fixture_is_right():
    for name, pair in TRANSITIONS.items():
        zone = ZoneInfo(name)
        for text in pair:
            t = instant(text)
            before = (t - timedelta(minutes=1)).astimezone(zone).utcoffset()
            changed = before != t.astimezone(zone).utcoffset()
            assert changed == (name != "Asia/Kolkata"), (name, text)
        assert len(starts(name)) == 24


@pytest.mark.parametrize("zone_name", ZONES)
def test_agrees_with_minute_scan_oracle(zone_name):
    zone = ZoneInfo(zone_name)
    checked = 0
    for spec, fields in SCHEDULES.items():
        sched = parse_standard(f"CRON_TZ={zone_name} {spec}")
        for after in starts(zone_name):
            want = oracle_next(fields, zone, after)
            got = sched.next(after)
            assert got == want, (
                f"{zone_name} {spec!r} after {after.isoformat()}: "
                f"got {got.isoformat()}, oracle {want.isoformat()}"
            )
            checked += 1
    assert checked == 8 * 24


def test_oracle_covers_all_zones_and_schedules():
    assert set(TRANSITIONS) == set(ZONES) and len(ZONES) == 5
    assert len(SCHEDULES) == 8


# ---------------------------------------------------------------------------
# grammar
# ---------------------------------------------------------------------------

def test_both_prefixes_and_extra_spaces():
    after = datetime(2026, 1, 1, tzinfo=UTC)
    want = datetime(2026, 1, 1, 3, 30, tzinfo=UTC)
    for spec in ("TZ=Asia/Kolkata 0 9 * * *", "CRON_TZ=Asia/Kolkata 0 9 * * *",
                 "CRON_TZ=Asia/Kolkata    0 9 * * *", "  TZ=Asia/Kolkata \t 0 9 * * *  "):
        sched = parse_standard(spec)
        assert sched.zone == ZoneInfo("Asia/Kolkata")
        assert sched.next(after) == want


def test_descriptor_and_every_with_prefix():
    daily = parse_standard("CRON_TZ=Asia/Tokyo @daily")
    assert daily.next(datetime(2026, 1, 1, tzinfo=UTC)) == datetime(2026, 1, 1, 15, tzinfo=UTC)
    every = parse_standard("CRON_TZ=Asia/Tokyo @every 90s")
    assert every.every == 90.0
    now = datetime(2026, 1, 1, 0, 0, 7, tzinfo=UTC)
    assert every.next(now) == now + timedelta(seconds=90)
    assert seconds_until_next("TZ=Asia/Tokyo @every 90s", now) == 91


def test_utc_empty_and_local_names():
    after = datetime(2026, 7, 1, 10, 30, tzinfo=timezone(timedelta(hours=3)))  # 07:30Z
    for spec in ("CRON_TZ=UTC 0 9 * * *", "CRON_TZ= 0 9 * * *", "TZ= 0 9 * * *"):
        sched = parse_standard(spec)
        assert sched.zone is not None
        assert sched.next(after) == datetime(2026, 7, 1, 9, 0, tzinfo=UTC)
    local = parse_standard("CRON_TZ=Local 0 9 * * *")
    assert local.zone is None
    assert local == parse_standard("0 9 * * *")
    # no zone: today's behaviour, the fields are read on after's own clock
    assert local.next(after) == after.replace(day=2, hour=9, minute=0)
    assert local.next(datetime(2026, 7, 1, 10, 30)) == datetime(2026, 7, 2, 9, 0)


@pytest.mark.parametrize("bad", [
    "cron_tz=UTC * * * * *",
    "tz=UTC * * * * *",
    "CRON_TZ=UTC",
    "CRON_TZ=UTC   ",
    "TZ=",
    "CRON_TZ=Mars/Olympus * * * * *",
    "CRON_TZ=../etc/passwd * * * * *",
    "CRON_TZ=/etc/passwd * * * * *",
    "CRON_TZ=America * * * * *",
    "CRON_TZ=UTC * * * *",
])
def test_bad_prefixed_specs_are_parse_errors(bad):
    with pytest.raises(CronParseError):
        parse_standard(bad)


def test_unknown_zone_uses_robfigs_wording():
    with pytest.raises(CronParseError) as e:
        parse_standard("CRON_TZ=Mars/Olympus * * * * *")
    assert str(e.value).startswith("provided bad location Mars/Olympus")
    with pytest.raises(CronParseError) as e:
        parse_standard("* * * * *", default_zone="Mars/Olympus")
    assert str(e.value).startswith("provided bad location Mars/Olympus")


def test_default_zone_applies_without_a_prefix_and_loses_to_one():
    after = datetime(2026, 1, 1, tzinfo=UTC)
    bare = parse_standard("0 9 * * *")
    assert bare.zone is None
    by_name = parse_standard("0 9 * * *", default_zone="Asia/Kolkata")
    by_tzinfo = parse_standard("0 9 * * *", default_zone=ZoneInfo("Asia/Kolkata"))
    assert by_name == by_tzinfo
    assert by_name.next(after) == datetime(2026, 1, 1, 3, 30, tzinfo=UTC)
    prefixed = parse_standard("CRON_TZ=Asia/Tokyo 0 9 * * *", default_zone="Asia/Kolkata")
    assert prefixed.zone == ZoneInfo("Asia/Tokyo")
    assert prefixed.next(after) == datetime(2026, 1, 2, 0, 0, tzinfo=UTC)
    assert parse_standard("CRON_TZ=Local 0 9 * * *", default_zone="Asia/Kolkata").zone is None


def test_naive_after_with_a_zone_is_a_value_error():
    sched = parse_standard("CRON_TZ=America/New_York 0 9 * * *")
    with pytest.raises(ValueError) as e:
        sched.next(datetime(2026, 1, 1))
    assert not isinstance(e.value, CronParseError)


def test_seconds_until_next_across_the_skipped_day():
    now = datetime(2026, 3, 8, 6, 0, tzinfo=UTC)
    assert seconds_until_next("CRON_TZ=America/New_York 30 2 * * *", now=now) == int(24.5 * 3600) + 1
    assert seconds_until_next("0 9 * * *", now=datetime(2026, 1, 1, tzinfo=UTC),
                              default_zone="Asia/Kolkata") == int(3.5 * 3600) + 1


def test_seconds_until_next_takes_utc_now_for_a_zoned_schedule():
    got = seconds_until_next("CRON_TZ=Asia/Tokyo * * * * *")
    assert 1 <= got <= 61


# ---------------------------------------------------------------------------
# skipping by field, not minute by minute
# ---------------------------------------------------------------------------

def test_rare_schedule_is_found_by_skipping_fields():
    """2 s is a gross-error bound: skipping by field is about a thousand
    steps a call, a minute scan about a million zone conversions a call."""
    sched = parse_standard("CRON_TZ=America/New_York 0 0 29 2 *")
    after = datetime(2026, 3, 1, tzinfo=UTC)
    t0 = time.monotonic()
    for _ in range(50):
        got = sched.next(after)
    elapsed = time.monotonic() - t0
    assert got == datetime(2028, 2, 29, 5, 0, tzinfo=UTC)
    assert elapsed < 2.0, elapsed


def test_five_year_give_up_is_kept():
    with pytest.raises(CronParseError):
        parse_standard("CRON_TZ=Europe/London 0 0 31 2 *").next(datetime(2026, 1, 1, tzinfo=UTC))

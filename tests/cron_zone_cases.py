"""Cases shared by the cron time-zone tests: the pinned instants and the zones.

The expected instants were computed with a minute-by-minute scan over
``zoneinfo`` (never with ``Schedule.next``) and are compared as instants.
"""
from datetime import datetime

ZONES = (
    "America/New_York", "Europe/London", "Australia/Lord_Howe",
    "Asia/Kolkata", "America/Havana",
)

#: (spec, after, expected next) as RFC 3339 strings
PINNED = (
    # 02:30 does not exist on the 8th (02:00 -> 03:00): next is the 9th
    ("CRON_TZ=America/New_York 30 2 * * *",
     "2026-03-08T00:00:00-05:00", "2026-03-09T06:30:00+00:00"),
    # 01:30 happens twice on 1 November (02:00 EDT -> 01:00 EST)
    ("TZ=America/New_York 30 1 * * *",
     "2026-11-01T01:00:00-04:00", "2026-11-01T05:30:00+00:00"),
    ("TZ=America/New_York 30 1 * * *",
     "2026-11-01T05:30:00+00:00", "2026-11-01T06:30:00+00:00"),
    # hourly keeps firing every absolute hour: 01:00 EST -> 03:00 EDT
    ("CRON_TZ=America/New_York 0 * * * *",
     "2026-03-08T01:00:00-05:00", "2026-03-08T07:00:00+00:00"),
    ("CRON_TZ=Asia/Kolkata 0 9 * * *",
     "2026-01-01T00:00:00+00:00", "2026-01-01T03:30:00+00:00"),
    ("CRON_TZ=America/New_York @daily",
     "2026-03-08T12:00:00+00:00", "2026-03-09T04:00:00+00:00"),
    # a 30-minute gap (02:00 -> 02:30) skips 02:15 on the 4th locally
    ("CRON_TZ=Australia/Lord_Howe 15 2 * * *",
     "2026-10-03T12:00:00+00:00", "2026-10-04T15:15:00+00:00"),
    # 1 April 00:00 BST
    ("CRON_TZ=Europe/London 0 0 1 * *",
     "2026-03-29T00:30:00+00:00", "2026-03-31T23:00:00+00:00"),
)


def instant(text: str) -> datetime:
    return datetime.fromisoformat(text)

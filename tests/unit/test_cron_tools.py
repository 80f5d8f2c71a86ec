"""The offline tools and cron time zones: ``lint`` parses a HealthCheck's
cron schedule, ``next`` previews a schedule's activations."""
import pathlib

import yaml

from active_monitor_amd.workflow.__main__ import main

REPO = pathlib.Path(__file__).parents[2]
EXAMPLE = REPO / "examples" / "cron-timezone.yaml"


def healthcheck(cron, repeat=None):
    doc = yaml.safe_load(EXAMPLE.read_text())
    doc["spec"]["schedule"]["cron"] = cron
    if repeat is not None:
        doc["spec"]["repeatAfterSec"] = repeat
    return doc


def test_lint_reports_a_bad_location(tmp_path, capsys):
    bad = tmp_path / "mars.yaml"
    bad.write_text(yaml.safe_dump(healthcheck("CRON_TZ=Mars/Olympus 0 9 * * *")))
    assert main(["lint", str(bad)]) == 1
    out = capsys.readouterr().out
    assert (f"{bad}: invalid HealthCheck: spec.schedule.cron: "
            "provided bad location Mars/Olympus") in out


def test_lint_reports_any_cron_the_controller_would_refuse(tmp_path, capsys):
    bad = tmp_path / "six.yaml"
    bad.write_text(yaml.safe_dump(healthcheck("0 0 9 * * *")))
    assert main(["lint", str(bad)]) == 1
    assert "spec.schedule.cron: expected exactly 5 fields" in capsys.readouterr().out


def test_lint_leaves_a_cron_alone_that_repeat_after_sec_overrides(tmp_path, capsys):
    unused = tmp_path / "unused.yaml"
    unused.write_text(yaml.safe_dump(healthcheck("CRON_TZ=Mars/Olympus 0 9 * * *", repeat=60)))
    assert main(["lint", str(unused)]) == 0
    assert capsys.readouterr().out.strip() == "ok"


def test_lint_accepts_the_shipped_example(capsys):
    assert main(["lint", str(EXAMPLE)]) == 0
    assert capsys.readouterr().out.strip() == "ok"


def test_next_shows_a_repeated_wall_time_twice(capsys):
    assert main(["next", "--cron", "CRON_TZ=America/New_York 30 1 * * *",
                 "--from", "2026-11-01T04:00:00Z", "-n", "3"]) == 0
    rows = [line.split() for line in capsys.readouterr().out.splitlines()]
    assert len(rows) == 3
    assert [r[0] for r in rows] == [
        "2026-11-01T01:30:00-04:00", "2026-11-01T01:30:00-05:00", "2026-11-02T01:30:00-05:00"]
    assert [r[1] for r in rows] == [
        "2026-11-01T05:30:00Z", "2026-11-01T06:30:00Z", "2026-11-02T06:30:00Z"]
    assert rows[0][2] == f"RepeatAfterSec={90 * 60 + 1}"


def test_next_defaults_to_five_and_takes_a_default_zone(capsys):
    assert main(["next", "--cron", "0 9 * * *", "--time-zone", "Asia/Kolkata",
                 "--from", "2026-01-01T00:00:00+00:00"]) == 0
    rows = [line.split() for line in capsys.readouterr().out.splitlines()]
    assert [r[1] for r in rows] == [f"2026-01-0{d}T03:30:00Z" for d in range(1, 6)]
    assert rows[0][0] == "2026-01-01T09:00:00+05:30"


def test_next_reads_a_healthcheck_file(capsys):
    assert main(["next", str(EXAMPLE), "-n", "2", "--from", "2026-03-06T12:00:00Z"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "cron-timezone: CRON_TZ=America/New_York 0 9 * * MON-FRI"
    # Friday 09:00 EST, then Monday 09:00 EDT: the change falls on the weekend
    assert [line.split()[1] for line in lines[1:]] == [
        "2026-03-06T14:00:00Z", "2026-03-09T13:00:00Z"]


def test_next_prints_parse_errors(tmp_path, capsys):
    assert main(["next", "--cron", "CRON_TZ=Mars/Olympus 0 9 * * *"]) == 1
    assert capsys.readouterr().out.startswith("error: provided bad location Mars/Olympus")
    assert main(["next", "--cron", "0 9 * * *", "--time-zone", "Mars/Olympus"]) == 1
    assert capsys.readouterr().out.startswith("error: provided bad location Mars/Olympus")
    assert main(["next", str(tmp_path / "missing.yaml")]) == 1
    assert capsys.readouterr().out.startswith("error: ")

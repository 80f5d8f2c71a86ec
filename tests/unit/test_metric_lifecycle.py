"""Metric series end with the HealthCheck they describe
(metrics.forget_healthcheck); the reference keeps every series for ever
(collector.go:55-60)."""
import json
import threading

from prometheus_client import CollectorRegistry

from active_monitor_amd.metrics import (
    MonitorError,
    MonitorFinishedTime,
    MonitorRuntime,
    MonitorStartedTime,
    MonitorSuccess,
    create_dynamic_prometheus_metric,
    custom_gauge_metrics,
    exposition,
    forget_healthcheck,
)
from active_monitor_amd.metrics.collector import _ExactNameCounter


def _status(*metrics):
    return {"outputs": {"parameters": [
        {"name": "m", "value": json.dumps({"metrics": list(metrics)})}]}}


def _metric(name, value, help_text="help"):
    return {"name": name, "value": value, "metrictype": "gauge", "help": help_text}


def _lines(name, registry=None):
    text = (exposition(registry) if registry is not None else exposition()).decode()
    return [ln for ln in text.splitlines()
            if not ln.startswith("#") and f'healthcheck_name="{name}"' in ln]


def test_exact_name_counter_remove():
    c = _ExactNameCounter("lc_counter", "help", ("healthcheck_name", "workflow"))
    c.labels("a", "healthCheck").inc()
    c.labels("a", "remedy").inc(2)
    c.labels("b", "healthCheck").inc()
    c.remove("a", "healthCheck")
    assert c.value("a", "healthCheck") == 0.0
    assert c.value("a", "remedy") == 2.0
    assert c.value("b", "healthCheck") == 1.0
    samples = c.collect()[0].samples
    assert sorted(s.labels["healthcheck_name"] + "/" + s.labels["workflow"]
                  for s in samples) == ["a/remedy", "b/healthCheck"]
    # absent label sets: silent, and nothing else is touched
    c.remove("a", "healthCheck")
    c.remove("never", "seen")
    assert len(c.collect()[0].samples) == 2
    # a removed label set starts again from zero
    c.labels("a", "healthCheck").inc()
    assert c.value("a", "healthCheck") == 1.0


def test_forget_healthcheck_counts_what_it_removed():
    name = "lc-count"
    MonitorSuccess.labels(name, "healthCheck").inc()
    MonitorRuntime.labels(name, "healthCheck").set(1.5)
    MonitorStartedTime.labels(name, "healthCheck").set(10)
    MonitorFinishedTime.labels(name, "healthCheck").set(12)
    MonitorError.labels(name, "remedy").inc()
    MonitorStartedTime.labels(name, "remedy").set(11)
    MonitorFinishedTime.labels(name, "remedy").set(12)
    create_dynamic_prometheus_metric(name, _status(_metric("x", 1), _metric("y", 2)))
    assert len(_lines(name)) == 9
    assert forget_healthcheck(name) == 9
    assert _lines(name) == []
    assert "lc_count_x" not in custom_gauge_metrics
    assert "lc_count_y" not in custom_gauge_metrics
    assert "lc_count_" not in exposition().decode()
    assert forget_healthcheck(name) == 0


def test_forget_healthcheck_is_silent_on_unknown_names():
    before = exposition()
    assert forget_healthcheck("lc-never-seen") == 0
    assert forget_healthcheck("") == 0
    assert exposition() == before


def test_other_checks_keep_their_series():
    MonitorSuccess.labels("lc-keep", "healthCheck").inc()
    MonitorSuccess.labels("lc-drop", "healthCheck").inc()
    assert forget_healthcheck("lc-drop") == 1
    assert MonitorSuccess.value("lc-keep", "healthCheck") == 1.0
    assert MonitorSuccess.value("lc-drop", "healthCheck") == 0.0
    assert forget_healthcheck("lc-keep") == 1


def test_shared_gauge_stays_while_another_check_has_a_child():
    """``a-b`` and ``a_b`` map to one gauge name."""
    registry = CollectorRegistry()
    create_dynamic_prometheus_metric("lc-a-b", _status(_metric("m", 1, "first")), registry)
    create_dynamic_prometheus_metric("lc_a_b", _status(_metric("m", 2, "ignored")), registry)
    assert len(_lines("lc-a-b", registry)) == len(_lines("lc_a_b", registry)) == 1

    assert forget_healthcheck("lc-a-b", registry) == 1
    assert "lc_a_b_m" in custom_gauge_metrics
    assert _lines("lc-a-b", registry) == []
    assert _lines("lc_a_b", registry) == ['lc_a_b_m{healthcheck_name="lc_a_b"} 2.0']

    assert forget_healthcheck("lc_a_b", registry) == 1
    assert "lc_a_b_m" not in custom_gauge_metrics
    assert "lc_a_b_m" not in exposition(registry).decode()

    # the name is free again: registered anew, with the new help text
    create_dynamic_prometheus_metric("lc-a-b", _status(_metric("m", 3, "second")), registry)
    text = exposition(registry).decode()
    assert "# HELP lc_a_b_m second" in text
    assert 'lc_a_b_m{healthcheck_name="lc-a-b"} 3.0' in text
    assert forget_healthcheck("lc-a-b", registry) == 1


def test_forget_while_another_thread_increments():
    """One thread hammers ``labels(...).inc()`` and the dynamic gauge while
    another forgets the name: no exception, no lost lock, and once both are
    done one last forget leaves nothing behind."""
    name = "lc-race"
    registry = CollectorRegistry()
    errs = []
    N = 3000
    removed = []

    def emit():
        try:
            for i in range(N):
                MonitorSuccess.labels(name, "healthCheck").inc()
                MonitorError.labels(name, "remedy").inc()
                MonitorRuntime.labels(name, "healthCheck").set(i)
                if i % 10 == 0:
                    create_dynamic_prometheus_metric(
                        name, _status(_metric("m", i)), registry)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    def forget():
        try:
            for _ in range(N):
                removed.append(forget_healthcheck(name, registry))
                exposition(registry)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=emit), threading.Thread(target=forget)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert errs == []
    assert all(0 <= n <= 4 for n in removed)
    forget_healthcheck(name, registry)
    assert forget_healthcheck(name, registry) == 0
    assert _lines(name) == []
    assert _lines(name, registry) == []
    assert "lc_race_m" not in custom_gauge_metrics
    # the counters still count after all that
    MonitorSuccess.labels(name, "healthCheck").inc()
    assert MonitorSuccess.value(name, "healthCheck") == 1.0
    assert forget_healthcheck(name, registry) == 1

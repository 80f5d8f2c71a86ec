"""Prometheus collectors (reference: internal/metrics/collector.go).

Exact series-name parity with the reference's 5 static collectors:

- ``healthcheck_success_count``   (counter)  :18-24
- ``healthcheck_error_count``     (counter)  :25-30
- ``healthcheck_runtime_seconds`` (gauge)    :31-36
- ``healthcheck_starttime``       (gauge)    :37-42 (Unix-seconds epoch despite
  the "Time taken" help string — a reference quirk kept for scrape parity)
- ``healthcheck_finishedtime``    (gauge)    :43-48

all labeled ``{healthcheck_name, workflow}`` with workflow ∈ {"healthCheck",
"remedy"} (collector.go:14-15; controller constants
healthcheck_controller.go:60-61).

The Go prometheus client exposes counters under the exact configured name,
while prometheus_client appends ``_total``; to keep the wire format identical a
small custom collector is used for the two counters.

Custom metrics from workflow output parameters
(``workflow.status.outputs.parameters`` JSON of shape
``{"metrics": [{name, value, metrictype, help}]}``, README.md:275-285) are
registered dynamically by :func:`create_dynamic_prometheus_metric`
(collector.go:68-115) — and, unlike the reference (which documents the feature
but never calls it — SURVEY.md §2.3, quirk list), the reconciler here invokes
it on the workflow-success path.

Series end with the HealthCheck they describe: :func:`forget_healthcheck`
removes every label set of a name, static and dynamic. The reference never
removes one (collector.go:55-60), so its ``/metrics`` grows with every
HealthCheck that ever existed.
"""
from __future__ import annotations

import json
import logging
import threading
from typing import Any, Dict, Iterable, List, Optional, Set, Tuple

from prometheus_client import CollectorRegistry, Gauge, generate_latest
from prometheus_client.core import Metric

log = logging.getLogger("active_monitor_amd.metrics")

HC_NAME_LABEL = "healthcheck_name"
WF_LABEL = "workflow"

# The framework's own registry — the equivalent of controller-runtime's
# metrics.Registry (collector.go:62-65); served by the Manager's metrics
# endpoint.
REGISTRY = CollectorRegistry()


class _ExactNameCounter:
    """CounterVec exposed under its exact name (no ``_total`` suffix), matching
    the Go client's exposition of the reference series."""

    def __init__(self, name: str, help_text: str, labelnames: Tuple[str, ...]):
        self._name = name
        self._help = help_text
        self._labelnames = labelnames
        self._values: Dict[Tuple[str, ...], float] = {}
        self._lock = threading.Lock()

    def labels(self, *labelvalues: str) -> "_ExactNameCounterChild":
        if len(labelvalues) != len(self._labelnames):
            raise ValueError(f"{self._name}: expected {len(self._labelnames)} labels")
        return _ExactNameCounterChild(self, tuple(labelvalues))

    def _inc(self, key: Tuple[str, ...], amount: float) -> None:
        if amount < 0:
            raise ValueError("counters can only increase")
        with self._lock:
            self._values[key] = self._values.get(key, 0.0) + amount

    def value(self, *labelvalues: str) -> float:
        with self._lock:
            return self._values.get(tuple(labelvalues), 0.0)

    def remove(self, *labelvalues: str) -> bool:
        """Drop one label set; silent (False) when it is not there."""
        with self._lock:
            return self._values.pop(tuple(labelvalues), None) is not None

    def collect(self) -> Iterable[Metric]:
        # An 'untyped' family keeps both the family name and sample names
        # exactly as configured (prometheus_client would append '_total' to a
        # counter-typed family, diverging from the Go client's exposition).
        fam = Metric(self._name, self._help, "untyped")
        with self._lock:
            for key, val in sorted(self._values.items()):
                fam.add_sample(self._name, dict(zip(self._labelnames, key)), val)
        return [fam]

    def describe(self) -> Iterable[Metric]:
        return [Metric(self._name, self._help, "untyped")]


class _ExactNameCounterChild:
    def __init__(self, parent: _ExactNameCounter, key: Tuple[str, ...]):
        self._parent = parent
        self._key = key

    def inc(self, amount: float = 1.0) -> None:
        self._parent._inc(self._key, amount)


class _TrackedGauge(Gauge):
    """A Gauge that keeps the label sets it has handed out, so that removing
    one can say whether it was there — prometheus_client keeps that to
    itself, and whether ``remove`` raises on an absent label set depends on
    its version. Label values are positional, as everywhere in this
    package."""

    def __init__(self, *args: Any, **kwargs: Any):
        super().__init__(*args, **kwargs)
        self._label_sets: Set[Tuple[str, ...]] = set()
        self._label_sets_lock = threading.Lock()

    def labels(self, *labelvalues: Any, **labelkwargs: Any) -> Any:
        # on the reconciler's hot path (three calls per run): a label set
        # seen before costs one set lookup, without the lock. A remove()
        # that slips in between that lookup and the child's re-creation
        # leaves a child the set does not know; remove() therefore always
        # removes the child as well, so the next one clears it.
        if labelvalues in self._label_sets:
            return super().labels(*labelvalues)
        if labelkwargs:
            raise ValueError("label values are given by position here")
        with self._label_sets_lock:
            child = super().labels(*labelvalues)
            self._label_sets.add(tuple(str(v) for v in labelvalues))
        return child

    def remove(self, *labelvalues: Any) -> bool:  # type: ignore[override]
        """Drop one label set; silent when it is not there. True when it
        was (exact unless the same label set is being written meanwhile)."""
        key = tuple(str(v) for v in labelvalues)
        with self._label_sets_lock:
            known = key in self._label_sets
            self._label_sets.discard(key)
            try:
                super().remove(*key)
            except KeyError:
                pass
        return known

    def label_sets(self) -> int:
        with self._label_sets_lock:
            return len(self._label_sets)


_LABELS = (HC_NAME_LABEL, WF_LABEL)

MonitorSuccess = _ExactNameCounter(
    "healthcheck_success_count", "The total number of successful healthcheck resources", _LABELS
)
MonitorError = _ExactNameCounter(
    "healthcheck_error_count", "The total number of errored healthcheck resources", _LABELS
)
MonitorRuntime = _TrackedGauge(
    "healthcheck_runtime_seconds",
    "Time taken for the workflow to complete.",
    _LABELS,
    registry=REGISTRY,
)
MonitorStartedTime = _TrackedGauge(
    "healthcheck_starttime",
    "Time taken for the workflow to complete.",
    _LABELS,
    registry=REGISTRY,
)
MonitorFinishedTime = _TrackedGauge(
    "healthcheck_finishedtime",
    "Time taken for the workflow to complete.",
    _LABELS,
    registry=REGISTRY,
)

REGISTRY.register(MonitorSuccess)  # type: ignore[arg-type]
REGISTRY.register(MonitorError)  # type: ignore[arg-type]

# Dynamic custom-metric gauges, guarded by an RW-ish lock (the reference fixed
# a data race here with an RWMutex — collector.go:50-51,92-109, issue #288).
custom_gauge_metrics: Dict[str, _TrackedGauge] = {}
_custom_lock = threading.Lock()
# HealthCheck name -> the dynamic gauges it has a child in ("a-b" and "a_b"
# share their gauges), so that forgetting a name does not walk every gauge
_custom_owned: Dict[str, Set[str]] = {}


def create_dynamic_prometheus_metric(
    name: str,
    workflow_status: Optional[Dict[str, Any]],
    registry: CollectorRegistry = REGISTRY,
) -> List[str]:
    """Parse ``workflow.status.outputs.parameters`` into dynamically registered
    gauges named ``<hc_name_with_underscores>_<metric name>`` labeled
    ``{healthcheck_name}`` (collector.go:68-115).

    ``workflow_status`` is the unstructured ``status`` dict of a Workflow.
    Returns the list of metric names updated (for tests/observability).
    """
    updated: List[str] = []
    if not workflow_status:
        return updated
    outputs = workflow_status.get("outputs")
    if not isinstance(outputs, dict):
        return updated
    parameters = outputs.get("parameters")
    if not isinstance(parameters, list):
        return updated

    for parameter in parameters:
        if not isinstance(parameter, dict):
            continue
        raw = parameter.get("value")
        if not isinstance(raw, str):
            continue
        try:
            json_map = json.loads(raw)
        except (ValueError, TypeError):
            # The reference ignores unmarshal errors (collector.go:76) and
            # iterates an empty map; mirror that leniency.
            continue
        if not isinstance(json_map, dict):
            continue
        for metric_raw in json_map.get("metrics", []) or []:
            if not isinstance(metric_raw, dict):
                log.error("Failed to decode metric for %s: %r", name, metric_raw)
                continue
            # mapstructure.Decode is case-insensitive on keys (collector.go:81).
            lowered = {str(k).lower(): v for k, v in metric_raw.items()}
            metric_name = str(lowered.get("name", "") or "")
            if metric_name == "":
                log.error("Skipping metric collection. Invalid metric %s: %r", name, metric_raw)
                continue
            try:
                value = float(lowered.get("value", 0) or 0)
            except (TypeError, ValueError):
                log.error("Failed to decode metric for %s: %r", name, metric_raw)
                continue
            help_text = str(lowered.get("help", "") or "")
            # '-' → '_' for Prometheus-friendly names (collector.go:90).
            full_name = name.replace("-", "_") + "_" + metric_name
            with _custom_lock:
                gauge = custom_gauge_metrics.get(full_name)
                if gauge is None:
                    try:
                        gauge = _TrackedGauge(full_name, help_text, (HC_NAME_LABEL,),
                                              registry=registry)
                        custom_gauge_metrics[full_name] = gauge
                    except ValueError as e:
                        log.error("Error registering %s metric %s", full_name, e)
                        continue
                gauge.labels(name).set(value)
                _custom_owned.setdefault(name, set()).add(full_name)
            updated.append(full_name)
            log.info("Successfully collected metric for %s, metric: %s=%s", name, full_name, value)
    return updated


_STATIC_SERIES = (MonitorSuccess, MonitorError, MonitorRuntime,
                  MonitorStartedTime, MonitorFinishedTime)
_WORKFLOW_LABELS = ("healthCheck", "remedy")


def forget_healthcheck(name: str, registry: CollectorRegistry = REGISTRY) -> int:
    """Remove every series of the HealthCheck ``name``: its ``healthCheck``
    and ``remedy`` label sets of the five static series, and its child of
    every dynamic gauge. A dynamic gauge left without any child is
    unregistered from ``registry`` and dropped from ``custom_gauge_metrics``,
    so a later check of that name registers it afresh, help text included;
    one that still has another check's child (``a-b`` and ``a_b`` share
    their gauges) stays. Unknown names are not an error. Returns the number
    of label sets removed."""
    removed = 0
    for series in _STATIC_SERIES:
        for wf_label in _WORKFLOW_LABELS:
            if series.remove(name, wf_label):
                removed += 1
    with _custom_lock:
        for full_name in _custom_owned.pop(name, ()):
            gauge = custom_gauge_metrics.get(full_name)
            if gauge is None:
                continue
            if gauge.remove(name):
                removed += 1
            if gauge.label_sets() == 0:
                del custom_gauge_metrics[full_name]
                try:
                    registry.unregister(gauge)
                except KeyError:
                    pass  # registered with another registry than this one
    return removed


def exposition(registry: CollectorRegistry = REGISTRY) -> bytes:
    """Text exposition of the registry (for the manager's /metrics endpoint)."""
    return generate_latest(registry)

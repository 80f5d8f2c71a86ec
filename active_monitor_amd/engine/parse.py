"""Workflow YAML parsing + field injection.

Re-implements the reference's parseWorkflowFromHealthcheck /
parseRemedyWorkflowFromHealthcheck (healthcheck_controller.go:876-1125):

- read the definition through the artifact store,
- YAML-decode; non-map documents and missing/non-map ``spec`` are errors with
  the reference's messages,
- label handling: workflow-defined ``metadata.labels`` are used (values
  stringified), the Argo instance-id label
  ``workflows.argoproj.io/controller-instanceid: activemonitor-workflows``
  is guaranteed as a default. Unlike the reference — whose shared
  ``workflowLabels`` map leaks labels across HealthChecks —
  labels here are scoped per submission,
- inject ``spec.podGC = {strategy: OnPodCompletion}`` when unset (:953-977),
- inject ``spec.serviceAccountName`` from the resource (:988-991),
- ``spec.activeDeadlineSeconds`` defaulting: health-check workflows default to
  ``Workflow.Timeout``, itself defaulted to ``RepeatAfterSec`` (a spec mutation
  that later feeds the backoff computation, :980-995); remedy workflows default
  to ``RepeatAfterSec`` and round-trip an existing numeric deadline back into
  ``RemedyWorkflow.Timeout`` (:1108-1120).
"""
from __future__ import annotations

import asyncio
from typing import Any, Dict, Optional, Tuple

import yaml

from ..api.types import HealthCheck
from ..store import ArtifactReadError, get_artifact_reader

WF_INSTANCE_ID_LABEL_KEY = "workflows.argoproj.io/controller-instanceid"
WF_INSTANCE_ID = "activemonitor-workflows"
POD_GC_ON_POD_COMPLETION = "OnPodCompletion"


class WorkflowParseError(Exception):
    pass


def _extract_labels(data: Dict[str, Any]) -> Dict[str, str]:
    """Per-submission label derivation with the instance-id default."""
    labels: Dict[str, str] = {}
    metadata = data.get("metadata")
    if isinstance(metadata, dict):
        raw = metadata.get("labels")
        if isinstance(raw, dict):
            for k, v in raw.items():
                labels[str(k)] = str(v)
    labels.setdefault(WF_INSTANCE_ID_LABEL_KEY, WF_INSTANCE_ID)
    return labels


# libyaml loader when available (~10x faster than the pure-Python one)
_Loader = getattr(yaml, "CSafeLoader", yaml.SafeLoader)

# Workflow definitions are re-parsed every cycle (reference :894); fleets
# re-submit the same YAML thousands of times, so cache parses by content.
_PARSE_CACHE: Dict[bytes, Dict[str, Any]] = {}
_PARSE_CACHE_MAX = 2048


def _decode(content: bytes) -> Dict[str, Any]:
    from ..utils.fastcopy import deep_copy

    cached = _PARSE_CACHE.get(content)
    if cached is not None:
        return deep_copy(cached)
    try:
        data = yaml.load(content, Loader=_Loader)
    except yaml.YAMLError as e:
        raise WorkflowParseError(f"Invalid spec file passed: {e}") from e
    if data is None:
        data = {}
    if not isinstance(data, dict):
        raise WorkflowParseError("Invalid spec file passed: not a mapping")
    if len(_PARSE_CACHE) >= _PARSE_CACHE_MAX:
        _PARSE_CACHE.clear()  # simple bound; refill costs one parse per doc
    _PARSE_CACHE[content] = deep_copy(data)
    return data


def _validated_spec(data: Dict[str, Any], remedy: bool) -> Dict[str, Any]:
    spec_raw = data.get("spec")
    if spec_raw is None:
        raise WorkflowParseError(
            "Invalid remedy workflow, missing spec" if remedy else "invalid workflow, missing spec"
        )
    if not isinstance(spec_raw, dict):
        raise WorkflowParseError(
            "invalid remedy workflow, spec is not a map"
            if remedy
            else "invalid workflow, spec is not a map"
        )
    return spec_raw


#: ceiling on one offloaded artifact read before the reconcile errors out
ARTIFACT_READ_TIMEOUT = 35.0


def _source_blocks(resource) -> bool:
    """URL and file sources do real I/O; inline is a memory read."""
    src = getattr(resource, "source", None)
    return src is not None and (src.url is not None or src.file is not None)


async def _read_source_async(resource) -> bytes:
    """Read an artifact source without blocking the event loop.

    The reference's URL fetch blocks only its own goroutine (url.go:20-57);
    a single-loop design must offload it. Inline sources stay on-loop (pure
    memory); URL/file reads run on a worker thread under a hard timeout so one
    hung source cannot stall other CRs' reconciles, watches or timers."""
    if resource is None:
        return b""
    reader = get_artifact_reader(resource.source)
    if not _source_blocks(resource):
        return reader.read()
    try:
        return await asyncio.wait_for(asyncio.to_thread(reader.read), ARTIFACT_READ_TIMEOUT)
    except asyncio.TimeoutError:
        raise ArtifactReadError(
            f"artifact read timed out after {ARTIFACT_READ_TIMEOUT:.0f}s"
        ) from None


def parse_from_healthcheck(
    hc: HealthCheck, remedy: bool, content: Optional[bytes] = None
) -> Tuple[Dict[str, Any], Dict[str, str]]:
    """Returns ``(spec_dict, labels)`` for the health-check workflow or, with
    ``remedy``, the remedy workflow. The two differ only in the error strings
    and in the deadline rule at the end. ``content`` short-circuits the
    artifact read (used by the async variant, which offloads blocking sources
    to a thread)."""
    wf = hc.spec.remedy_workflow if remedy else hc.spec.workflow
    if content is None:
        content = b""
        if wf.resource is not None:
            content = get_artifact_reader(wf.resource.source).read()
    data = _decode(content)
    labels = _extract_labels(data)
    spec = _validated_spec(data, remedy)

    if spec.get("podGC") is None:
        spec["podGC"] = {"strategy": POD_GC_ON_POD_COMPLETION}
    if wf.resource is not None and wf.resource.service_account:
        spec["serviceAccountName"] = wf.resource.service_account

    deadline = spec.get("activeDeadlineSeconds")
    if not remedy:
        # Workflow.Timeout defaults from RepeatAfterSec — a spec mutation that
        # later feeds the backoff computation (reference :980-995)
        if wf.timeout == 0:
            wf.timeout = hc.spec.repeat_after_sec
        if deadline is None:
            spec["activeDeadlineSeconds"] = wf.timeout
    else:
        # the deadline defaults from RepeatAfterSec; an existing numeric one
        # round-trips into RemedyWorkflow.Timeout (reference :1108-1120)
        timeout = hc.spec.repeat_after_sec
        if deadline is None:
            spec["activeDeadlineSeconds"] = timeout
        elif isinstance(deadline, (int, float)) and not isinstance(deadline, bool):
            timeout = int(deadline)
        wf.timeout = timeout
    return spec, labels


async def parse_from_healthcheck_async(
    hc: HealthCheck, remedy: bool
) -> Tuple[Dict[str, Any], Dict[str, str]]:
    """Event-loop-safe variant: blocking sources (URL/file) are read on a
    worker thread with a timeout before the pure-CPU parse runs on-loop."""
    wf = hc.spec.remedy_workflow if remedy else hc.spec.workflow
    content = await _read_source_async(wf.resource)
    return parse_from_healthcheck(hc, remedy, content)


def parse_workflow_from_healthcheck(
    hc: HealthCheck, content: Optional[bytes] = None
) -> Tuple[Dict[str, Any], Dict[str, str]]:
    """Health-check workflow (reference :876-1000); mutates
    ``hc.spec.workflow.timeout`` when it defaults from RepeatAfterSec."""
    return parse_from_healthcheck(hc, False, content)


def parse_remedy_workflow_from_healthcheck(
    hc: HealthCheck, content: Optional[bytes] = None
) -> Tuple[Dict[str, Any], Dict[str, str]]:
    """Remedy workflow (reference :1002-1125); sets
    ``hc.spec.remedy_workflow.timeout``."""
    return parse_from_healthcheck(hc, True, content)


async def parse_workflow_from_healthcheck_async(
    hc: HealthCheck,
) -> Tuple[Dict[str, Any], Dict[str, str]]:
    return await parse_from_healthcheck_async(hc, False)


async def parse_remedy_workflow_from_healthcheck_async(
    hc: HealthCheck,
) -> Tuple[Dict[str, Any], Dict[str, str]]:
    return await parse_from_healthcheck_async(hc, True)

"""The run-request contract: asking for a HealthCheck to run now.

Three annotations on the HealthCheck, none of them in ``status`` (the CRD
and its 18 status fields stay as they are, so a cluster carrying the
reference's CRD prunes nothing):

- ``run-requested``: written by the user (``amctl run``, ``kubectl annotate
  --overwrite``). An opaque non-empty token, by convention an RFC 3339 UTC
  time to the microsecond; a new value is a new request.
- ``run-handled``: written by the controller, the last token it served.
- ``run-workflow``: written by the controller, the generated name of the
  check Workflow that served it.

The Workflow that serves a request carries ``run-request: <token>``.
"""
from __future__ import annotations

from datetime import datetime, timezone
from typing import Any, Optional

from .. import GROUP

RUN_REQUESTED_ANNOTATION = f"{GROUP}/run-requested"
RUN_HANDLED_ANNOTATION = f"{GROUP}/run-handled"
RUN_WORKFLOW_ANNOTATION = f"{GROUP}/run-workflow"
#: on the Workflow, not on the HealthCheck
RUN_REQUEST_ANNOTATION = f"{GROUP}/run-request"


def pending_run_request(metadata: Any) -> Optional[str]:
    """The token of the request that waits to be served, or None.

    A request is pending when ``run-requested`` is a non-empty string and
    differs from ``run-handled``. ``metadata`` is an object's metadata as a
    dict or as an :class:`ObjectMeta`."""
    if isinstance(metadata, dict):
        annotations = metadata.get("annotations")
    else:
        annotations = getattr(metadata, "annotations", None)
    if not annotations or not isinstance(annotations, dict):
        return None
    token = annotations.get(RUN_REQUESTED_ANNOTATION)
    if not token or not isinstance(token, str):
        return None
    if annotations.get(RUN_HANDLED_ANNOTATION) == token:
        return None
    return token


def new_run_token() -> str:
    """A fresh token by the convention: now, in UTC, to the microsecond."""
    return datetime.now(timezone.utc).strftime("%Y-%m-%dT%H:%M:%S.%fZ")

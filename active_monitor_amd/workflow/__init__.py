"""Workflow execution backends (Argo-CR driven, scripted fake, local executor)."""
from .engines import (
    POSTPONED_MESSAGE,
    QUEUE_EXPIRED_MESSAGE,
    LocalWorkflowEngine,
    ScriptedWorkflowEngine,
    always_fail,
    always_succeed,
    never_complete,
)
from .logs import LogStore
from .validate import validate_template_library, validate_workflow_spec

__all__ = [
    "POSTPONED_MESSAGE",
    "QUEUE_EXPIRED_MESSAGE",
    "LocalWorkflowEngine",
    "LogStore",
    "ScriptedWorkflowEngine",
    "always_fail",
    "always_succeed",
    "never_complete",
    "validate_template_library",
    "validate_workflow_spec",
]

"""RBAC provisioning for health-check and remedy workflows.

Re-implements the reference's SA/Role/ClusterRole/Binding lifecycle
(healthcheck_controller.go:302-474, 1127-1443):

- default least-privilege rule sets: read-only for health checks, scoped CRUD
  for remedies (:85-120), overridable per-CR via ``spec.*.rbacRules`` (:124-129),
- derived names ``<sa>-cluster-role``, ``<sa>-cluster-role-binding``,
  ``<sa>-ns-role``, ``<sa>-ns-role-binding`` (:306-309,321-324),
- get-then-create idempotency (existing objects are reused, never updated),
- every created object labeled ``workflows.argoproj.io/managed-by:
  active-monitor``; deletes only touch objects carrying that label
  (:1169,1242,1317,1375,1433),
- remedy SA collision rename ``<sa>-remedy`` when it matches the health-check
  SA (:316-319).
"""
from __future__ import annotations

import os
import time
from typing import Any, Callable, Dict, List, Optional

from ..api.types import HealthCheck, PolicyRule
from ..kube.client import EventRecorder, KubeClient
from ..kube.errors import AlreadyExistsError, NotFoundError

RBAC_API_VERSION = "rbac.authorization.k8s.io/v1"

WF_MANAGED_BY_LABEL_KEY = "workflows.argoproj.io/managed-by"
WF_MANAGED_BY_VALUE = "active-monitor"

CLUSTER_LEVEL = "cluster"
NAMESPACE_LEVEL = "namespace"

# spec.level → (role kind, suffix of the role name derived from the SA); the
# binding is "<role kind>Binding" named "<role name>-binding" (:306-309,321-324)
_ROLE_BY_LEVEL = {
    CLUSTER_LEVEL: ("ClusterRole", "-cluster-role"),
    NAMESPACE_LEVEL: ("Role", "-ns-role"),
}

# Least-privilege read-only rules for monitoring workflows
# (healthcheck_controller.go:85-101).
DEFAULT_HEALTHCHECK_RULES: List[PolicyRule] = [
    PolicyRule(
        api_groups=[""],
        resources=["pods", "nodes", "events", "services", "configmaps", "namespaces", "endpoints"],
        verbs=["get", "list", "watch"],
    ),
    PolicyRule(
        api_groups=["apps"],
        resources=["deployments", "replicasets", "statefulsets", "daemonsets"],
        verbs=["get", "list", "watch"],
    ),
    PolicyRule(
        api_groups=["argoproj.io"],
        resources=["workflows"],
        verbs=["get", "list", "watch"],
    ),
]

# Scoped write rules for remedy workflows (healthcheck_controller.go:104-120).
DEFAULT_REMEDY_RULES: List[PolicyRule] = [
    PolicyRule(
        api_groups=[""],
        resources=["pods", "events", "services", "configmaps", "endpoints"],
        verbs=["get", "list", "watch", "create", "update", "patch", "delete"],
    ),
    PolicyRule(
        api_groups=["apps"],
        resources=["deployments", "replicasets", "statefulsets"],
        verbs=["get", "list", "watch", "create", "update", "patch", "delete"],
    ),
    PolicyRule(
        api_groups=["argoproj.io"],
        resources=["workflows"],
        verbs=["get", "list", "watch", "create", "update", "patch", "delete"],
    ),
]


def resolve_rbac_rules(
    custom: List[PolicyRule], defaults: List[PolicyRule]
) -> List[PolicyRule]:
    """Custom rules win when non-empty (healthcheck_controller.go:124-129)."""
    return custom if custom else defaults


def _managed_labels() -> Dict[str, str]:
    return {WF_MANAGED_BY_LABEL_KEY: WF_MANAGED_BY_VALUE}


def _is_managed(obj: Dict[str, Any]) -> bool:
    labels = (obj.get("metadata") or {}).get("labels") or {}
    return labels.get(WF_MANAGED_BY_LABEL_KEY) == WF_MANAGED_BY_VALUE


class RBACProvisioner:
    """Creates and deletes the workflow RBAC objects through a KubeClient
    (the reference threads a typed clientset through each helper so unit
    tests can pass a fake — here the client itself is injectable)."""

    #: how long a successful ensure suppresses re-checking the same object.
    #: The reference re-gets every RBAC object on every cycle (:333-408); with
    #: a fleet at 1 Hz that is ~4 redundant apiserver round-trips per cycle.
    #: External deletions are still repaired within this window; 0 disables.
    ENSURE_TTL = 30.0

    def __init__(self, client: KubeClient, recorder: Optional[EventRecorder] = None,
                 ensure_ttl: Optional[float] = None):
        self.client = client
        self.recorder = recorder
        if ensure_ttl is None:
            env = os.environ.get("AM_RBAC_ENSURE_TTL")
            ensure_ttl = float(env) if env else self.ENSURE_TTL
        self.ensure_ttl = ensure_ttl
        self._ensured: Dict[tuple, float] = {}

    def _fresh(self, key: tuple) -> bool:
        if self.ensure_ttl <= 0:
            return False
        exp = self._ensured.get(key)
        return exp is not None and exp > time.monotonic()

    def _mark(self, key: tuple) -> None:
        if self.ensure_ttl > 0:
            if len(self._ensured) > 50000:
                now = time.monotonic()
                self._ensured = {k: v for k, v in self._ensured.items() if v > now}
            self._ensured[key] = time.monotonic() + self.ensure_ttl

    async def _event(self, hc_obj: Dict[str, Any], ev_type: str, message: str) -> None:
        if self.recorder is not None:
            await self.recorder.event(hc_obj, ev_type, ev_type, message)

    async def _ensure(
        self, api_version: str, kind: str, namespace: str, name: str,
        body_fn: Optional[Callable[[], Dict[str, Any]]] = None,
    ) -> None:
        """Get-then-create, reusing the object if present. ``namespace`` is ""
        for cluster-scoped kinds; ``body_fn`` builds the fields beyond
        metadata and runs only when the object has to be created."""
        cache_key = (kind, namespace, name)
        if self._fresh(cache_key):
            return
        try:
            await self.client.get(api_version, kind, namespace, name)
        except NotFoundError:
            metadata: Dict[str, Any] = {"name": name}
            if namespace:
                metadata["namespace"] = namespace
            metadata["labels"] = _managed_labels()
            obj = {"apiVersion": api_version, "kind": kind, "metadata": metadata}
            if body_fn is not None:
                obj.update(body_fn())
            try:
                await self.client.create(obj, transfer=True)
            except AlreadyExistsError:
                # concurrent reconciles sharing an SA race get-then-create;
                # losing the race means the object exists — reuse it
                pass
        self._mark(cache_key)

    async def _delete_if_managed(self, api_version: str, kind: str, namespace: str, name: str) -> None:
        """Drop the TTL-cache entry, then delete the object if it carries the
        managed-by label."""
        self._ensured.pop((kind, namespace, name), None)
        # Already-gone objects count as deleted. (The reference propagates the
        # Get error here (:1164-1166), which makes concurrent remedy teardowns
        # of a shared SA fail each other — an availability fix, not a
        # semantic change.)
        try:
            obj = await self.client.get(api_version, kind, namespace, name)
        except NotFoundError:
            return
        if _is_managed(obj):
            try:
                await self.client.delete(api_version, kind, namespace, name)
            except NotFoundError:
                return

    # -- orchestration ------------------------------------------------------

    async def create_rbac_for_workflow(self, hc: HealthCheck, workflow_type: str) -> None:
        """``workflow_type`` ∈ {"healthCheck", "remedy"}
        (healthcheck_controller.go:302-415). May rename the remedy SA on
        collision — a spec mutation visible for the rest of the reconcile,
        as in the reference (:316-319). The remedy is validated (and renamed)
        whichever of the two is being provisioned."""
        check, remedy = hc.spec.workflow, hc.spec.remedy_workflow
        sa, ns = check.resource.service_account, check.resource.namespace
        rules = resolve_rbac_rules(check.rbac_rules, DEFAULT_HEALTHCHECK_RULES)

        remedy_sa = remedy_ns = ""
        if not remedy.is_empty():
            if remedy.resource is None:
                await self._event(hc.to_dict(), "Warning",
                                  "RemedyWorkflow is set but Resource is nil")
                raise ValueError("RemedyWorkflow is set but Resource is nil")
            if remedy.resource.service_account == "":
                await self._event(
                    hc.to_dict(), "Warning",
                    "ServiceAccount for the RemedyWorkflow is not specified"
                )
                raise ValueError("ServiceAccount for the RemedyWorkflow is not specified")
            if sa == remedy.resource.service_account:
                remedy.resource.service_account = sa + "-remedy"
            remedy_sa, remedy_ns = remedy.resource.service_account, remedy.resource.namespace

        if workflow_type == "remedy":
            sa, ns = remedy_sa, remedy_ns
            rules = resolve_rbac_rules(remedy.rbac_rules, DEFAULT_REMEDY_RULES)

        # the SA is created before an unset level is reported (:333-345)
        await self._ensure("v1", "ServiceAccount", ns, sa)
        role = _ROLE_BY_LEVEL.get(hc.spec.level)
        if role is None:
            await self._event(hc.to_dict(), "Warning", "level is not set")
            raise ValueError("level is not set")
        role_kind, suffix = role
        role_ns = "" if role_kind == "ClusterRole" else ns
        await self._ensure(
            RBAC_API_VERSION, role_kind, role_ns, sa + suffix,
            lambda: {"rules": [r.to_dict() for r in rules]},
        )
        await self._ensure(
            RBAC_API_VERSION, role_kind + "Binding", role_ns, sa + suffix + "-binding",
            lambda: {
                "roleRef": {
                    "apiGroup": "rbac.authorization.k8s.io",
                    "kind": role_kind,
                    "name": sa + suffix,
                },
                "subjects": [{"kind": "ServiceAccount", "name": sa, "namespace": ns}],
            },
        )

    async def delete_rbac_for_workflow(self, hc: HealthCheck) -> None:
        """Tear down the remedy RBAC after a remedy run
        (healthcheck_controller.go:417-474). Only remedy objects are deleted,
        and only when labeled managed-by active-monitor."""
        if hc.spec.remedy_workflow.resource is None:
            return
        sa = hc.spec.remedy_workflow.resource.service_account
        ns = hc.spec.remedy_workflow.resource.namespace
        await self._delete_if_managed("v1", "ServiceAccount", ns, sa)
        role = _ROLE_BY_LEVEL.get(hc.spec.level)
        if role is None:
            await self._event(hc.to_dict(), "Warning", "level is not set")
            raise ValueError("level is not set")
        role_kind, suffix = role
        role_ns = "" if role_kind == "ClusterRole" else ns
        await self._delete_if_managed(RBAC_API_VERSION, role_kind, role_ns, sa + suffix)
        await self._delete_if_managed(
            RBAC_API_VERSION, role_kind + "Binding", role_ns, sa + suffix + "-binding")

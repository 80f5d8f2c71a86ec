"""Shared templates: ``WorkflowTemplate`` and ``ClusterWorkflowTemplate``.

:func:`resolve` turns a Workflow spec that refers to shared templates — by
``spec.workflowTemplateRef``, or by ``templateRef`` on a step or DAG task —
into a :class:`Resolved` bundle: the effective spec and every referenced
template, each under the scope it came from. The bundle is a snapshot: the
executor, the validator and the status writes all read it, and nothing in it
changes when the shared template is edited afterwards.

A scope is a string: ``""`` for the Workflow's own templates,
``namespaced/NAME`` for those of a WorkflowTemplate and ``cluster/NAME`` for
those of a ClusterWorkflowTemplate. Inside a scoped template ``template: X``
means X of the same scope, never the Workflow's own X.

Semantics follow Argo's documented behaviour with one simplification:
``arguments.parameters`` and ``templates`` of a ``workflowTemplateRef`` are
merged by ``name`` with the Workflow's entry replacing the template's whole
(Argo merges such entries field by field).
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Tuple

WFT_KIND = "WorkflowTemplate"
WFT_PLURAL = "workflowtemplates"
CWFT_KIND = "ClusterWorkflowTemplate"
CWFT_PLURAL = "clusterworkflowtemplates"
TEMPLATE_KINDS = (WFT_KIND, CWFT_KIND)

#: ``(cluster_scope, name)`` → the template object, or None when there is none
Lookup = Callable[[bool, str], Optional[Dict[str, Any]]]

OWN_SCOPE = ""


def scope_key(cluster: bool, name: Any) -> str:
    return f"{'cluster' if cluster else 'namespaced'}/{name}"


def scope_label(scope: str) -> str:
    """``WorkflowTemplate 'net-checks'`` for ``namespaced/net-checks``."""
    where, _, name = scope.partition("/")
    return f"{CWFT_KIND if where == 'cluster' else WFT_KIND} {name!r}"


def template_where(name: Any, scope: str = OWN_SCOPE) -> str:
    """How a problem names a template: ``template 'probe'``, or ``template
    'probe' of WorkflowTemplate 'net-checks'`` for a shared one."""
    if scope:
        return f"template {name!r} of {scope_label(scope)}"
    return f"template {name!r}"


def not_found_message(cluster: bool, name: Any) -> str:
    return f'{CWFT_PLURAL if cluster else WFT_PLURAL}.argoproj.io "{name}" not found'


def _name_of(entry: Any) -> Any:
    """The ``name`` of a list entry when it can serve as one (a scalar),
    else None. A Workflow is stored without schema admission, so any JSON
    may stand where a name is expected."""
    name = entry.get("name") if isinstance(entry, dict) else None
    return name if isinstance(name, (str, int, float)) else None


def calls_of(tmpl: Dict[str, Any]) -> List[Dict[str, Any]]:
    """The steps or DAG tasks of a composite template, flattened. What is
    not shaped like one (``dag: [...]``, ``steps: 5``) holds no calls."""
    if "steps" in tmpl:
        out = []
        steps = tmpl["steps"]
        for group in steps if isinstance(steps, list) else []:
            for s in group if isinstance(group, list) else [group]:
                if isinstance(s, dict):
                    out.append(s)
        return out
    if "dag" in tmpl:
        dag = tmpl["dag"]
        tasks = dag.get("tasks") if isinstance(dag, dict) else None
        return [t for t in tasks if isinstance(t, dict)] if isinstance(tasks, list) else []
    return []


def call_kind(tmpl: Dict[str, Any]) -> str:
    return "task" if "dag" in tmpl else "step"


def templates_by_name(spec: Any) -> Dict[Any, Dict[str, Any]]:
    templates = spec.get("templates") if isinstance(spec, dict) else None
    if not isinstance(templates, list):
        return {}
    return {_name_of(t): t for t in templates if _name_of(t) is not None}


def has_references(spec: Any) -> bool:
    """Whether ``spec`` names a shared template anywhere. Like everything
    here it raises for nothing a stored spec may hold."""
    if not isinstance(spec, dict):
        return False
    if "workflowTemplateRef" in spec:
        return True
    templates = spec.get("templates")
    for tmpl in templates if isinstance(templates, list) else []:
        if isinstance(tmpl, dict) and ("steps" in tmpl or "dag" in tmpl):
            for call in calls_of(tmpl):
                if "templateRef" in call:
                    return True
    return False


def well_formed_ref(ref: Any) -> bool:
    return (isinstance(ref, dict) and isinstance(ref.get("name"), str) and bool(ref["name"])
            and isinstance(ref.get("template"), str) and bool(ref["template"]))


def shown_ref(ref: Dict[str, Any]) -> Dict[str, Any]:
    """The ``templateRef`` a node carries."""
    out: Dict[str, Any] = {"name": ref.get("name"), "template": ref.get("template")}
    if ref.get("clusterScope") is True:
        out["clusterScope"] = True
    return out


def _merge_named(base: Any, over: Any) -> List[Any]:
    """Two lists of ``{name: ...}`` entries merged by name: an entry of
    ``over`` replaces the one of ``base`` where it stands, new ones follow."""
    out = list(base) if isinstance(base, list) else []
    at = {_name_of(e): i for i, e in enumerate(out)}
    for e in over if isinstance(over, list) else []:
        name = _name_of(e)
        if name is not None and name in at:
            out[at[name]] = e
        else:
            if name is not None:
                at[name] = len(out)
            out.append(e)
    return out


def merge_specs(template_spec: Dict[str, Any], workflow_spec: Dict[str, Any]) -> Dict[str, Any]:
    """The effective spec of a Workflow that has a ``workflowTemplateRef``:
    the template's spec overlaid by the Workflow's. For every top-level field
    the Workflow's value wins when present; ``arguments.parameters`` and
    ``templates`` are merged by ``name``, whole entries. ``workflowTemplateRef``
    itself is dropped. Neither input is changed."""
    out = dict(template_spec)
    out.pop("workflowTemplateRef", None)
    for key, value in workflow_spec.items():
        if key == "workflowTemplateRef" or value is None:
            continue
        if key == "templates":
            out[key] = _merge_named(out.get(key), value)
        elif key == "arguments" and isinstance(value, dict) and isinstance(out.get(key), dict):
            merged = {**out[key], **value}
            if "parameters" in out[key] or "parameters" in value:
                merged["parameters"] = _merge_named(out[key].get("parameters"),
                                                    value.get("parameters"))
            out[key] = merged
        else:
            out[key] = value
    return out


class Resolved:
    """What :func:`resolve` found.

    ``spec``         the effective spec, ``workflowTemplateRef`` merged in
    ``stored_spec``  the same, but None unless ``workflowTemplateRef`` was used
    ``scopes``       scope → {template name → template}; ``""`` is the
                     Workflow's own (the effective spec's) templates
    ``stored``       ``namespaced/NAME/TEMPLATE`` / ``cluster/NAME/TEMPLATE`` →
                     every template reached through a ``templateRef``, in the
                     order met
    ``errors``       ``(where, message)`` of every reference that does not
                     resolve; ``message`` alone is what fails a Workflow
    ``missing``      ``(cluster_scope, name)`` the lookup did not have
    """

    __slots__ = ("spec", "stored_spec", "scopes", "stored", "errors", "missing")

    def __init__(self) -> None:
        self.spec: Dict[str, Any] = {}
        self.stored_spec: Optional[Dict[str, Any]] = None
        self.scopes: Dict[str, Dict[Any, Dict[str, Any]]] = {}
        self.stored: Dict[str, Dict[str, Any]] = {}
        self.errors: List[Tuple[str, str]] = []
        self.missing: List[Tuple[bool, str]] = []

    def stored_in(self, scope: str) -> List[Dict[str, Any]]:
        """The reached templates of one scope, in the order met."""
        prefix = scope + "/"
        return [t for key, t in self.stored.items() if key.startswith(prefix)]

    def problems(self) -> List[str]:
        return [f"{where}: {message}" for where, message in self.errors]


class _Walk:
    """Collects each (scope, template) once, so reference loops terminate."""

    def __init__(self, lookup: Lookup, found: Resolved):
        self.lookup = lookup
        self.found = found
        self._objects: Dict[str, Optional[Dict[str, Any]]] = {}
        self._todo: List[Tuple[Dict[str, Any], str]] = []

    def library(self, cluster: bool, name: str) -> Optional[Dict[str, Any]]:
        key = scope_key(cluster, name)
        if key not in self._objects:
            obj = self.lookup(cluster, name)
            self._objects[key] = obj
            if obj is None:
                self.found.missing.append((cluster, name))
            else:
                self.found.scopes[key] = templates_by_name(obj.get("spec"))
        return self._objects[key]

    def calls(self, tmpl: Dict[str, Any], scope: str) -> None:
        where = template_where(tmpl.get("name"), scope)
        for call in calls_of(tmpl):
            ref = call.get("templateRef")
            if ref is None:
                local = call.get("template")
                if scope and isinstance(local, str) and local in self.found.scopes[scope]:
                    self.reach(scope, local)
                continue  # an unknown local name is the validator's to report
            if call.get("template") is not None or not well_formed_ref(ref):
                continue  # so is a malformed call
            cwhere = f"{where}: {call_kind(tmpl)} {call.get('name')!r}"
            cluster = ref.get("clusterScope") is True
            if self.library(cluster, ref["name"]) is None:
                self.found.errors.append((cwhere, not_found_message(cluster, ref["name"])))
                continue
            target = scope_key(cluster, ref["name"])
            if ref["template"] not in self.found.scopes[target]:
                self.found.errors.append((
                    cwhere, f"template reference {ref['name']}.{ref['template']} not found"))
                continue
            self.reach(target, ref["template"])

    def reach(self, scope: str, name: Any) -> None:
        key = f"{scope}/{name}"
        if key not in self.found.stored:
            tmpl = self.found.scopes[scope][name]
            self.found.stored[key] = tmpl
            self._todo.append((tmpl, scope))

    def drain(self) -> None:
        while self._todo:
            tmpl, scope = self._todo.pop(0)
            self.calls(tmpl, scope)


def resolve(spec: Dict[str, Any], lookup: Lookup) -> Resolved:
    """Resolve every reference of ``spec``. Never raises for what a spec may
    hold: what does not resolve is in ``errors``."""
    found = Resolved()
    walk = _Walk(lookup, found)
    found.spec = spec
    if "workflowTemplateRef" in spec:
        ref = spec["workflowTemplateRef"]
        if not isinstance(ref, dict) or not isinstance(ref.get("name"), str) or not ref["name"]:
            found.errors.append(("spec.workflowTemplateRef", "needs a name"))
            return found
        cluster = ref.get("clusterScope") is True
        obj = walk.library(cluster, ref["name"])
        if obj is None:
            found.errors.append(("spec.workflowTemplateRef",
                                 not_found_message(cluster, ref["name"])))
            return found
        tspec = obj.get("spec")
        found.spec = found.stored_spec = merge_specs(
            tspec if isinstance(tspec, dict) else {}, spec)
        arguments = found.spec.get("arguments")
        params = arguments.get("parameters") if isinstance(arguments, dict) else None
        if isinstance(params, list):
            # a parameter left to its ``default`` runs with it
            params = [
                {**p, "value": p["default"]} if isinstance(p, dict) and p.get("value") is None
                and p.get("default") is not None else p for p in params]
            # a new map: the one at hand may be the template's own
            found.spec["arguments"] = {**arguments, "parameters": params}
        for p in params if isinstance(params, list) else []:
            if _name_of(p) is not None and p.get("value") is None:
                found.errors.append((
                    "spec.arguments",
                    f"parameter {p['name']!r} has no value in "
                    f"{scope_label(scope_key(cluster, ref['name']))} "
                    "and the Workflow does not supply one"))
    found.scopes[OWN_SCOPE] = templates_by_name(found.spec)
    for tmpl in found.scopes[OWN_SCOPE].values():
        walk.calls(tmpl, OWN_SCOPE)
    walk.drain()
    return found


def library_scope(obj: Dict[str, Any]) -> str:
    return scope_key(obj.get("kind") == CWFT_KIND, (obj.get("metadata") or {}).get("name"))


def resolve_library(obj: Dict[str, Any], lookup: Lookup) -> Tuple[str, Resolved]:
    """A template document checked on its own: every template it holds
    counts as reached. Returns its scope and what its references lead to."""
    scope = library_scope(obj)
    found = Resolved()
    walk = _Walk(lookup, found)
    found.scopes[scope] = templates_by_name(obj.get("spec"))
    walk._objects[scope] = obj
    for name in found.scopes[scope]:
        walk.reach(scope, name)
    walk.drain()
    return scope, found


def lookup_in(objects: Dict[Tuple[bool, str], Dict[str, Any]]) -> Lookup:
    return lambda cluster, name: objects.get((cluster, name))

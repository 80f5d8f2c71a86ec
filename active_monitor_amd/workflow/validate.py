"""Static checks for the workflow surface the local executor runs.

:func:`validate_workflow_spec` returns human-readable problems, in a stable
order, without starting anything. The engine calls it before the first
process and fails the workflow with the first problem; the ``lint`` command
prints all of them.
"""
from __future__ import annotations

import re
from typing import Any, Dict, List, Optional, Set

from .expr import FUNCTIONS, ExprError
from .expr import parse as parse_expr
from .template import (
    REF_RE,
    TemplateError,
    active_deadline,
    expand_sequence,
    find_refs,
    find_strings,
    step_timeout,
)
from .templates import (
    OWN_SCOPE,
    Lookup,
    Resolved,
    calls_of,
    library_scope,
    resolve,
    resolve_library,
    scope_label,
    template_where,
    well_formed_ref,
)

#: template body types the local executor runs
BODY_TYPES = ("container", "script", "steps", "dag", "suspend", "http")
#: body types Argo knows that have no local equivalent
UNSUPPORTED_BODY_TYPES = ("resource", "data", "containerSet", "plugin")

HTTP_METHODS = ("GET", "HEAD", "POST", "PUT", "PATCH", "DELETE", "OPTIONS")
#: ``timeoutSeconds`` of an ``http`` template that sets none (Argo's default,
#: from memory)
HTTP_DEFAULT_TIMEOUT_SECONDS = 30
_HTTP_KEYS = ("url", "method", "headers", "body", "timeoutSeconds", "successCondition",
              "insecureSkipVerify")
#: what an expression of an ``http`` template may name
_HTTP_EXPR_NAMES = ("response", "response.statusCode", "response.body", "response.headers")

_WORKFLOW_VARS = {"workflow.name", "workflow.namespace", "workflow.status"}
_DEPENDS_RE = re.compile(r"^[A-Za-z0-9_\-]+(\s*&&\s*[A-Za-z0-9_\-]+)*$")


def parse_depends(expr: Any) -> Optional[List[str]]:
    """Task names of a ``depends`` that is only bare names joined by ``&&``;
    None for anything else (``A.Failed``, ``||``, ``!``, parentheses)."""
    if not isinstance(expr, str) or not _DEPENDS_RE.match(expr.strip()):
        return None
    return [p.strip() for p in expr.split("&&")]


def task_dependencies(task: Dict[str, Any]) -> List[str]:
    """Dependencies of one DAG task (``dependencies`` list and/or a
    supported ``depends``), duplicates removed, order kept."""
    deps: List[str] = []
    raw = task.get("dependencies")
    if isinstance(raw, list):
        deps.extend(str(d) for d in raw)
    if task.get("depends"):
        deps.extend(parse_depends(task["depends"]) or [])
    return list(dict.fromkeys(deps))


def _param_names(params: Any) -> Set[str]:
    return {
        str(p["name"]) for p in (params or []) if isinstance(p, dict) and p.get("name") is not None
    }


def _find_cycle(deps: Dict[str, List[str]]) -> Optional[str]:
    """Name of a task that sits on a dependency cycle, or None."""
    WHITE, GREY, BLACK = 0, 1, 2
    color = {n: WHITE for n in deps}
    for root in deps:
        if color[root] != WHITE:
            continue
        stack = [(root, iter(deps[root]))]
        color[root] = GREY
        while stack:
            node, it = stack[-1]
            for nxt in it:
                if nxt not in color:
                    continue
                if color[nxt] == GREY:
                    return nxt
                if color[nxt] == WHITE:
                    color[nxt] = GREY
                    stack.append((nxt, iter(deps[nxt])))
                    break
            else:
                color[node] = BLACK
                stack.pop()
    return None


def _check_refs(where: str, obj: Any, inputs: Set[str], wf_params: Optional[Set[str]],
                call_names: Set[str], kind: str, problems: List[str],
                in_loop: bool = False) -> None:
    """``in_loop``: ``obj`` is a step or task that carries ``withItems``,
    ``withParam`` or ``withSequence`` — the only place where ``{{item}}``
    means anything.
    ``wf_params`` None: workflow parameters are not known here (a template
    document checked on its own) and any name passes."""
    for text in find_strings(obj):
        if "{{=" in text.replace(" ", ""):
            problems.append(f"{where}: expression tags ({{{{=...}}}}) are not supported")
            break
    for ref in dict.fromkeys(find_refs(obj)):
        head, _, rest = ref.partition(".")
        if head == "inputs":
            if not rest.startswith("parameters."):
                problems.append(f"{where}: unsupported reference {{{{{ref}}}}}")
            elif rest[len("parameters."):] not in inputs:
                problems.append(
                    f"{where}: {{{{{ref}}}}} refers to an undeclared input parameter"
                )
        elif head == "workflow":
            if rest.startswith("parameters."):
                if wf_params is not None and rest[len("parameters."):] not in wf_params:
                    problems.append(
                        f"{where}: {{{{{ref}}}}} refers to an undeclared workflow parameter"
                    )
            elif ref not in _WORKFLOW_VARS:
                problems.append(f"{where}: unsupported reference {{{{{ref}}}}}")
        elif head in ("steps", "tasks"):
            if head != kind:
                problems.append(
                    f"{where}: {{{{{ref}}}}} is not available in this template"
                )
            # task names may contain dots only in theory; match the longest
            elif not any(rest == n or rest.startswith(n + ".") for n in call_names):
                problems.append(f"{where}: {{{{{ref}}}}} refers to an unknown {head[:-1]}")
        elif head == "item":
            if not in_loop:
                problems.append(
                    f"{where}: {{{{{ref}}}}} is only available in a step or task "
                    "with withItems or withParam"
                )
        elif head == "retries":
            if rest:
                problems.append(f"{where}: unsupported reference {{{{{ref}}}}}")
        else:
            problems.append(f"{where}: unknown variable namespace in {{{{{ref}}}}}")


def _positive_int(value: Any) -> bool:
    return isinstance(value, int) and not isinstance(value, bool) and value >= 1


def ignored_synchronization(spec: Dict[str, Any],
                            templates: Optional[Resolved] = None) -> List[str]:
    """What of ``synchronization`` the local engine does not act on, for one
    warning: semaphores (they are backed by a ConfigMap) and anything at
    template level, in the spec's own templates and, with ``templates``, in
    the shared ones it reaches. Mutexes at ``spec`` level are honoured by
    the engine."""
    found: List[str] = []
    sync = spec.get("synchronization")
    if isinstance(sync, dict) and ("semaphore" in sync or "semaphores" in sync):
        found.append("spec.synchronization semaphores are")
    names = [str(t.get("name")) for t in spec.get("templates") or []
             if isinstance(t, dict) and "synchronization" in t]
    if templates is not None:
        names += [key for key, t in templates.stored.items() if "synchronization" in t]
    if names:
        found.append(f"template-level synchronization ({', '.join(names)}) is")
    return found


def _check_expression(where: str, what: str, text: Any, problems: List[str]) -> None:
    """An expression of an ``http`` template: it parses and names only what
    the executor gives it. One that still holds ``{{...}}`` is judged when it
    runs; its references are checked like everywhere else."""
    if not isinstance(text, str) or not text.strip():
        problems.append(f"{where}: {what} must be a non-empty string")
        return
    if "{{" in text:
        return
    try:
        names = parse_expr(text).names()
    except ExprError as e:
        problems.append(f"{where}: invalid {what}: {e}")
        return
    for name in sorted(names.identifiers):
        if name not in _HTTP_EXPR_NAMES and not name.startswith("response.headers."):
            problems.append(f"{where}: {what} uses the unknown name {name!r}")
    for fn in sorted(names.functions - set(FUNCTIONS)):
        problems.append(f"{where}: {what} calls the unknown function {fn!r}")


def _check_http(where: str, tmpl: Dict[str, Any], problems: List[str]) -> None:
    body = tmpl.get("http")
    if not isinstance(body, dict):
        problems.append(f"{where}: http is not a map")
        return
    if not isinstance(body.get("url"), str) or not body["url"].strip():
        problems.append(f"{where}: http.url must be a non-empty string")
    method = body.get("method")
    if method is not None and "{{" not in str(method) and method not in HTTP_METHODS:
        problems.append(
            f"{where}: http.method {method!r} is not one of {', '.join(HTTP_METHODS)}")
    headers = body.get("headers")
    if headers is not None and not isinstance(headers, list):
        problems.append(f"{where}: http.headers is not a list")
    for h in headers if isinstance(headers, list) else []:
        if isinstance(h, dict) and "valueFrom" in h:
            problems.append(
                f"{where}: http header {h.get('name')!r} has a valueFrom: "
                "secret references have no local equivalent")
        elif (not isinstance(h, dict) or not isinstance(h.get("name"), str) or not h["name"]
              or not isinstance(h.get("value"), str) or set(h) - {"name", "value"}):
            problems.append(f"{where}: http.headers entries must be {{name, value}} strings")
    if "body" in body and not isinstance(body["body"], str):
        problems.append(f"{where}: http.body must be a string")
    if "timeoutSeconds" in body and not _positive_int(body["timeoutSeconds"]):
        problems.append(f"{where}: http.timeoutSeconds must be a positive integer")
    if "insecureSkipVerify" in body and not isinstance(body["insecureSkipVerify"], bool):
        problems.append(f"{where}: http.insecureSkipVerify must be true or false")
    for key in body:
        if key not in _HTTP_KEYS:
            problems.append(f"{where}: http.{key} is not supported")
    if "successCondition" in body:
        _check_expression(where, "successCondition", body["successCondition"], problems)
    for p in (tmpl.get("outputs") or {}).get("parameters") or []:
        value_from = p.get("valueFrom") if isinstance(p, dict) else None
        if isinstance(value_from, dict) and "expression" in value_from:
            _check_expression(where, f"outputs.parameters.{p.get('name')} expression",
                              value_from["expression"], problems)


_LOOP_KEYS = ("withItems", "withParam", "withSequence")


def _check_sequence(where: str, seq: Any, problems: List[str]) -> None:
    """Expand it once, with a zero in place of every ``{{...}}``: a number
    that is a reference is judged when it runs, the shape and whatever is
    written out are judged here. A ``format`` with a reference is left out."""
    if isinstance(seq, dict):
        seq = {k: REF_RE.sub("0", v) if isinstance(v, str) else v for k, v in seq.items()
               if not (k == "format" and isinstance(v, str) and "{{" in v)}
    try:
        expand_sequence(seq)
    except TemplateError as e:
        problems.append(f"{where}: {e}")


def _check_continue_on(where: str, on: Any, problems: List[str]) -> None:
    if not isinstance(on, dict):
        problems.append(f"{where}: continueOn is not a map")
        return
    for key, value in on.items():
        if key not in ("failed", "error"):
            problems.append(f"{where}: continueOn.{key} is not supported (failed, error)")
        elif not isinstance(value, bool):
            problems.append(f"{where}: continueOn.{key} must be true or false")


def _check_deadlines(where: str, tmpl: Dict[str, Any], problems: List[str]) -> None:
    """``timeout`` and ``activeDeadlineSeconds`` of a template. A value that
    holds ``{{...}}`` is judged when it runs."""
    if "timeout" in tmpl:
        value = tmpl["timeout"]
        if "steps" in tmpl or "dag" in tmpl:
            problems.append(f"{where}: timeout is not supported on steps and dag templates")
        elif not (isinstance(value, str) and "{{" in value):
            try:
                step_timeout(value)
            except TemplateError as e:
                problems.append(f"{where}: invalid timeout: {e}")
    value = tmpl.get("activeDeadlineSeconds")
    if not (isinstance(value, str) and "{{" in value):
        try:
            active_deadline(value)
        except TemplateError as e:
            problems.append(f"{where}: invalid activeDeadlineSeconds: {e}")


UNRESOLVABLE = "cannot be resolved here: no WorkflowTemplates were given"


def _check_template(where: str, tmpl: Dict[str, Any], local: Dict[Any, Dict[str, Any]],
                    resolvable: bool, wf_params: Optional[Set[str]],
                    problems: List[str]) -> None:
    """One template in its own scope: ``local`` holds the templates that a
    ``template: X`` of its calls may name. ``resolvable``: a ``templateRef``
    has been followed already and what it lacks is reported elsewhere."""
    if "templateRef" in tmpl:
        problems.append(f"{where}: templateRef is not supported")
    bodies = [b for b in BODY_TYPES if b in tmpl]
    foreign = [b for b in UNSUPPORTED_BODY_TYPES if b in tmpl]
    if foreign:
        problems.append(f"{where}: {foreign[0]} templates are not supported")
    elif not bodies and "templateRef" not in tmpl:  # that one is its (refused) body
        problems.append(
            f"{where}: no body (expected one of {', '.join(BODY_TYPES)})"
        )
    if len(bodies) + len(foreign) > 1:
        problems.append(
            f"{where}: several bodies ({', '.join(bodies + foreign)}); expected exactly one"
        )

    if "http" in tmpl:
        _check_http(where, tmpl, problems)

    if tmpl.get("parallelism") is not None and not _positive_int(tmpl["parallelism"]):
        problems.append(f"{where}: parallelism must be a positive integer")
    _check_deadlines(where, tmpl, problems)

    calls = calls_of(tmpl)
    kind = "tasks" if "dag" in tmpl else ("steps" if "steps" in tmpl else "")
    seen: Set[str] = set()
    for call in calls:
        cname = call.get("name")
        cwhere = f"{where}: {kind[:-1]} {cname!r}"
        if cname is None:
            problems.append(f"{where}: a {kind[:-1]} has no name")
        elif cname in seen:
            problems.append(f"{cwhere} is defined more than once")
        seen.add(cname)
        if "templateRef" in call:
            if call.get("template") is not None:
                problems.append(f"{cwhere}: template and templateRef are mutually exclusive")
            elif not well_formed_ref(call["templateRef"]):
                problems.append(f"{cwhere}: templateRef needs a name and a template")
            elif not resolvable:
                problems.append(f"{cwhere}: templateRef {UNRESOLVABLE}")
        elif call.get("template") not in local:
            problems.append(f"{cwhere}: template {call.get('template')!r} not found")
        loops = [key for key in _LOOP_KEYS if key in call]
        if len(loops) > 1:
            problems.append(f"{cwhere}: {' and '.join(loops)} are mutually exclusive")
        if "withSequence" in call:
            _check_sequence(cwhere, call["withSequence"], problems)
        if "continueOn" in call:
            _check_continue_on(cwhere, call["continueOn"], problems)
        if "withItems" in call and not isinstance(call["withItems"], list):
            problems.append(f"{cwhere}: withItems is not a list")

    if kind == "tasks":
        deps: Dict[str, List[str]] = {}
        for task in calls:
            tname = task.get("name")
            twhere = f"{where}: task {tname!r}"
            if task.get("depends") and parse_depends(task["depends"]) is None:
                problems.append(
                    f"{twhere}: unsupported depends expression {task['depends']!r} "
                    "(only task names joined by && are supported)"
                )
            if "dependencies" in task and not isinstance(task["dependencies"], list):
                problems.append(f"{twhere}: dependencies is not a list")
            deps[tname] = task_dependencies(task)
            for d in deps[tname]:
                if d not in seen:
                    problems.append(f"{twhere}: depends on unknown task {d!r}")
        cyc = _find_cycle(deps)
        if cyc is not None:
            problems.append(f"{where}: dependency cycle through task {cyc!r}")

    inputs = _param_names((tmpl.get("inputs") or {}).get("parameters"))
    names = {str(n) for n in seen if n is not None}
    # the template's own fields first, then each step or task on its own:
    # {{item}} is valid only inside one that loops
    body = {k: v for k, v in tmpl.items() if k not in ("steps", "dag")}
    _check_refs(where, body, inputs, wf_params, names, kind, problems)
    for call in calls:
        _check_refs(f"{where}: {kind[:-1]} {call.get('name')!r}", call, inputs, wf_params,
                    names, kind, problems,
                    in_loop=any(key in call for key in _LOOP_KEYS))


def _named_templates(spec: Dict[str, Any], where: str,
                     problems: List[str]) -> Dict[Any, Dict[str, Any]]:
    templates: Dict[Any, Dict[str, Any]] = {}
    listed = spec.get("templates") or []
    if not isinstance(listed, list):
        problems.append(f"spec.templates{where} is not a list")
        return templates
    for t in listed:
        if not isinstance(t, dict) or not isinstance(t.get("name"), (str, int, float)):
            problems.append(f"a template{where} has no name")
            continue
        if t["name"] in templates:
            problems.append(f"template {t['name']!r}{where} is defined more than once")
        templates[t["name"]] = t
    return templates


def _check_shared(found: Resolved, skip: str, wf_params: Optional[Set[str]],
                  problems: List[str]) -> None:
    """Every shared template that was reached, in its own scope; those of
    scope ``skip`` have been checked by the caller."""
    for key, tmpl in found.stored.items():
        scope = key[:key.rindex("/")]
        if scope != skip:
            _check_template(template_where(tmpl.get("name"), scope), tmpl,
                            found.scopes[scope], True, wf_params, problems)


def validate_workflow_spec(spec: Any, templates: Any = None) -> List[str]:
    """Problems that would stop ``spec`` from running locally; ``[]`` when
    it is clean.

    ``templates`` gives the shared templates: a lookup ``(cluster_scope,
    name) -> object or None``, or the :class:`~.templates.Resolved` bundle of
    a spec that was resolved already. The effective whole is then checked:
    ``workflowTemplateRef`` merged in, every reachable shared template in its
    own scope, every ``{{workflow.parameters.X}}`` against the effective
    arguments. A reference that does not resolve is reported alone: the rest
    cannot be judged without it. Without ``templates`` each reference is one
    problem that says so."""
    if not isinstance(spec, dict):
        return ["workflow spec is not a map"]
    found: Optional[Resolved] = None
    if templates is not None:
        found = templates if isinstance(templates, Resolved) else resolve(spec, templates)
        if found.errors:
            return found.problems()
        spec = found.spec
    elif "workflowTemplateRef" in spec:
        return [f"spec.workflowTemplateRef {UNRESOLVABLE}"]
    problems: List[str] = []
    own = _named_templates(spec, "", problems)

    entry = spec.get("entrypoint")
    if entry not in own:
        problems.append(f"entrypoint {entry!r} not found")
    on_exit = spec.get("onExit")
    if on_exit is not None and on_exit not in own:
        problems.append(f"onExit template {on_exit!r} not found")

    if spec.get("parallelism") is not None and not _positive_int(spec["parallelism"]):
        problems.append("spec.parallelism must be a positive integer")
    priority = spec.get("priority")
    if priority is not None and (isinstance(priority, bool) or not isinstance(priority, int)):
        problems.append("spec.priority must be an integer")

    wf_params = _param_names((spec.get("arguments") or {}).get("parameters"))
    _check_refs("spec.arguments", spec.get("arguments"), set(), wf_params, set(), "", problems)

    for name, tmpl in own.items():
        _check_template(template_where(name), tmpl, own, found is not None,
                        wf_params, problems)
    if found is not None:
        _check_shared(found, OWN_SCOPE, wf_params, problems)
    return problems


def validate_template_library(obj: Any, templates: Optional[Lookup] = None) -> List[str]:
    """Problems of one ``WorkflowTemplate`` / ``ClusterWorkflowTemplate``
    document, checked as a library: every template it holds, in its own
    scope. ``entrypoint`` is optional and workflow parameters need not be
    declared, since the Workflow that uses it may bring them."""
    if not isinstance(obj, dict) or not isinstance(obj.get("spec"), dict):
        return ["invalid workflow template, missing spec"]
    if not isinstance((obj.get("metadata") or {}).get("name"), str):
        return ["invalid workflow template, missing metadata.name"]
    spec = obj["spec"]
    if templates is not None:
        scope, found = resolve_library(obj, templates)
    else:
        scope, found = library_scope(obj), Resolved()
    if found.errors:
        return found.problems()
    problems: List[str] = []
    of = f" of {scope_label(scope)}"
    local = _named_templates(spec, of, problems)
    for key in ("entrypoint", "onExit"):
        if spec.get(key) is not None and spec[key] not in local:
            problems.append(f"{key} {spec[key]!r}{of} not found")
    for name, tmpl in local.items():
        _check_template(template_where(name, scope), tmpl, local, templates is not None,
                        None, problems)
    _check_shared(found, scope, None, problems)
    return problems

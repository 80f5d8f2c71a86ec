"""Structural-schema validation and pruning for custom resources.

A real apiserver checks every write of a custom resource against the CRD's
``openAPIV3Schema``: values of the wrong type are refused with 422, fields
the schema does not know are pruned. :func:`compile_schema` turns such a
schema into a :class:`Validator` once per kind; :meth:`Validator.admit` is
what the store (kube/memory.py) runs per write.

Compilation resolves every keyword into per-node tables and a per-node
``ok`` closure, so admitting an object never looks at the schema dict again.
``ok`` answers "valid, nothing to prune, no null to drop" without building a
path or an error; only an object that fails it is walked a second time by
the reporting pass, which prunes, drops nulls and words the errors.

Keywords outside the supported set (``default``, ``oneOf``/``anyOf``/
``allOf``/``not``, ``x-kubernetes-validations``, ...) raise ``ValueError`` at
compile time: nothing in a schema is silently left unenforced.

The error strings follow the format apiextensions-apiserver documents
(``field.Error`` rendering); they have not been compared against a live
cluster.
"""
from __future__ import annotations

import json
import re
from datetime import datetime
from typing import Any, Callable, Dict, List, Optional, Tuple

TYPE_INVALID = "FieldValueTypeInvalid"
REQUIRED = "FieldValueRequired"
NOT_SUPPORTED = "FieldValueNotSupported"
INVALID = "FieldValueInvalid"

_TYPES = ("object", "array", "string", "integer", "number", "boolean")

_SUPPORTED = frozenset({
    "type", "properties", "required", "items", "additionalProperties",
    "enum", "minimum", "maximum", "minLength", "maxLength", "pattern",
    "minItems", "maxItems", "format", "nullable",
    "x-kubernetes-preserve-unknown-fields", "x-kubernetes-int-or-string",
    "x-kubernetes-list-type", "description",
})

#: never pruned or type-checked (beyond "metadata is an object"): the
#: apiserver validates these against ObjectMeta/TypeMeta, not the CRD schema
_ROOT_EXEMPT = frozenset({"apiVersion", "kind", "metadata"})

_RFC3339 = re.compile(
    r"^(\d{4})-(\d{2})-(\d{2})[Tt](\d{2}):(\d{2}):(\d{2})(\.\d+)?"
    r"([Zz]|[+-]\d{2}:\d{2})$"
)


class SchemaError(str):
    """One validation error: the apiserver-style string, plus the cause
    ``reason`` and ``field`` a Status body's ``details.causes`` carries."""

    reason: str
    field: str

    def __new__(cls, field: str, reason: str, detail: str) -> "SchemaError":
        self = super().__new__(cls, f"{field}: {detail}")
        self.field = field
        self.reason = reason
        self.detail = detail
        return self


#: timestamps found valid: a fleet's status writes carry the same few
#: second-precision strings over and over
_DATE_TIMES_SEEN: set = set()


def _is_date_time(value: str) -> bool:
    if value in _DATE_TIMES_SEEN:
        return True
    if not _parse_date_time(value):
        return False
    if len(_DATE_TIMES_SEEN) > 4096:
        _DATE_TIMES_SEEN.clear()
    _DATE_TIMES_SEEN.add(value)
    return True


def _parse_date_time(value: str) -> bool:
    m = _RFC3339.match(value)
    if m is None:
        return False
    y, mo, d, h, mi, s = (int(x) for x in m.groups()[:6])
    zone = m.group(8)
    if zone not in ("Z", "z") and (int(zone[1:3]) > 23 or int(zone[4:6]) > 59):
        return False
    if h > 23 or mi > 59 or s > 60:  # 60: a leap second
        return False
    try:
        datetime(y, mo, d)
    except ValueError:
        return False
    return True


def _json_type(value: Any) -> str:
    if value is None:
        return "null"
    t = type(value)
    if t is bool:
        return "boolean"
    if t is int:
        return "integer"
    if t is float:
        return "number"
    if t is str:
        return "string"
    if t is dict:
        return "object"
    if t is list:
        return "array"
    return t.__name__


_NUMBERS = (int, float)


def _same(a: Any, b: Any) -> bool:
    """JSON equality: numbers by value (``1.0`` is ``1``, as ``integer``
    accepts ``60.0``), everything else by type too — ``True`` is not ``1``."""
    ta, tb = type(a), type(b)
    if ta is tb:
        return a == b
    return ta in _NUMBERS and tb in _NUMBERS and a == b


def _join(path: str, key: str) -> str:
    return f"{path}.{key}" if path else key


class _Node:
    """One compiled schema node. ``ok`` is the no-report check; the tables
    below it feed :meth:`walk`, the reporting and pruning pass."""

    __slots__ = (
        "type", "nullable", "props", "required", "additional", "keep_unknown",
        "items", "enum", "minimum", "maximum", "min_length", "max_length",
        "pattern", "pattern_src", "min_items", "max_items", "date_time",
        "int_or_string", "ok",
    )

    # -- the reporting pass --------------------------------------------------

    def _type_ok(self, v: Any) -> bool:
        t = type(v)
        want = self.type
        if self.int_or_string:
            return t is int or t is str
        if want is None:
            return True
        if want == "string":
            return t is str
        if want == "integer":
            return t is int or (t is float and v.is_integer())
        if want == "number":
            return t is int or t is float
        if want == "boolean":
            return t is bool
        if want == "object":
            return t is dict
        return t is list

    def walk(self, v: Any, path: str, errs: List[SchemaError],
             pruned: List[str]) -> None:
        """Validate ``v`` (not None unless nullable), pruning in place."""
        if v is None and self.nullable:
            return
        if not self._type_ok(v):
            want = "integer or string" if self.int_or_string else self.type
            got = _json_type(v)
            errs.append(SchemaError(
                path, TYPE_INVALID,
                f'Invalid value: "{got}": {path} in body must be of type '
                f'{want}: "{got}"'))
            return
        if self.enum is not None and not any(_same(v, e) for e in self.enum):
            allowed = ", ".join(json.dumps(e) for e in self.enum)
            errs.append(SchemaError(
                path, NOT_SUPPORTED,
                f"Unsupported value: {json.dumps(v)}: supported values: {allowed}"))
        t = type(v)
        if t is dict:
            self._walk_object(v, path, errs, pruned)
        elif t is list:
            self._walk_array(v, path, errs, pruned)
        elif t is str:
            self._walk_string(v, path, errs)
        elif t is int or t is float:
            if self.minimum is not None and v < self.minimum:
                self._invalid(errs, path, v, "should be greater than or equal to "
                              f"{json.dumps(self.minimum)}")
            if self.maximum is not None and v > self.maximum:
                self._invalid(errs, path, v, "should be less than or equal to "
                              f"{json.dumps(self.maximum)}")

    @staticmethod
    def _invalid(errs: List[SchemaError], path: str, v: Any, what: str) -> None:
        errs.append(SchemaError(
            path, INVALID, f"Invalid value: {json.dumps(v)}: {path} in body {what}"))

    def _walk_string(self, v: str, path: str, errs: List[SchemaError]) -> None:
        if self.min_length is not None and len(v) < self.min_length:
            self._invalid(errs, path, v,
                          f"should be at least {self.min_length} chars long")
        if self.max_length is not None and len(v) > self.max_length:
            self._invalid(errs, path, v,
                          f"should be at most {self.max_length} chars long")
        if self.pattern is not None and self.pattern.search(v) is None:
            self._invalid(errs, path, v, f"should match '{self.pattern_src}'")
        if self.date_time and not _is_date_time(v):
            self._invalid(errs, path, v,
                          f"must be of type date-time: {json.dumps(v)}")

    def _walk_object(self, v: Dict[str, Any], path: str,
                     errs: List[SchemaError], pruned: List[str]) -> None:
        props = self.props
        for key in list(v):
            child = props.get(key)
            known = child is not None
            if not known:
                child = self.additional
                if child is None:
                    if not self.keep_unknown:
                        del v[key]
                        pruned.append(_join(path, key))
                    continue
                if child is True:
                    continue
            val = v[key]
            if val is None and not child.nullable:
                del v[key]  # dropped like the apiserver drops it: not "pruned"
                continue
            child.walk(val, _join(path, key), errs, pruned)
        for key in self.required:
            if key not in v:
                errs.append(SchemaError(_join(path, key), REQUIRED, "Required value"))

    def _walk_array(self, v: List[Any], path: str, errs: List[SchemaError],
                    pruned: List[str]) -> None:
        if self.min_items is not None and len(v) < self.min_items:
            self._invalid(errs, path, v,
                          f"should have at least {self.min_items} items")
        if self.max_items is not None and len(v) > self.max_items:
            self._invalid(errs, path, v,
                          f"should have at most {self.max_items} items")
        item = self.items
        if item is not None:
            for i, x in enumerate(v):
                item.walk(x, f"{path}[{i}]", errs, pruned)


def _scalar_ok(node: _Node) -> Callable[[Any], bool]:
    """The ``ok`` closure of a non-container node, specialised for the
    unconstrained cases a CRD is mostly made of."""
    want = node.type
    plain = (node.enum is None and node.minimum is None and node.maximum is None
             and node.min_length is None and node.max_length is None
             and node.pattern is None and not node.date_time
             and not node.nullable and not node.int_or_string)
    if plain and want == "string":
        return lambda v: type(v) is str
    if plain and want == "integer":
        return lambda v: type(v) is int or (type(v) is float and v.is_integer())
    if plain and want == "boolean":
        return lambda v: type(v) is bool
    if plain and want == "number":
        return lambda v: type(v) is int or type(v) is float
    if (want == "string" and node.date_time and not node.nullable
            and node.enum is None and node.min_length is None
            and node.max_length is None and node.pattern is None):
        return lambda v: type(v) is str and _is_date_time(v)

    def ok(v: Any) -> bool:  # the general case: run the reporting pass dry
        errs: List[SchemaError] = []
        node.walk(v, "", errs, [])
        return not errs

    return ok


def _object_ok(node: _Node) -> Callable[[Any], bool]:
    props = {k: c.ok for k, c in node.props.items()}
    required = tuple(node.required)
    additional = node.additional
    keep_unknown = node.keep_unknown
    nullable = node.nullable
    enum = node.enum
    extra_ok = None if additional in (None, True) else additional.ok

    def ok(v: Any) -> bool:
        if type(v) is not dict:
            return v is None and nullable
        for key, val in v.items():
            child = props.get(key)
            if child is None:
                if extra_ok is not None:
                    child = extra_ok
                elif additional is True or keep_unknown:
                    continue
                else:
                    return False  # to be pruned
            if not child(val):
                return False
        for key in required:
            if key not in v:
                return False
        return enum is None or any(_same(v, e) for e in enum)

    return ok


def _array_ok(node: _Node) -> Callable[[Any], bool]:
    item = None if node.items is None else node.items.ok
    lo, hi = node.min_items, node.max_items
    nullable = node.nullable
    enum = node.enum

    def ok(v: Any) -> bool:
        if type(v) is not list:
            return v is None and nullable
        if lo is not None and len(v) < lo:
            return False
        if hi is not None and len(v) > hi:
            return False
        if item is not None:
            for x in v:
                if not item(x):
                    return False
        return enum is None or any(_same(v, e) for e in enum)

    return ok


def _compile(schema: Any, path: str) -> _Node:
    where = path or "<root>"
    if not isinstance(schema, dict):
        raise ValueError(f"schema at {where} is not an object")
    for kw in schema:
        if kw not in _SUPPORTED:
            raise ValueError(f"unsupported schema keyword {kw!r} at {where}")
    node = _Node()
    node.type = schema.get("type")
    node.int_or_string = bool(schema.get("x-kubernetes-int-or-string"))
    node.keep_unknown = bool(schema.get("x-kubernetes-preserve-unknown-fields"))
    if node.type is None:
        if not (node.int_or_string or node.keep_unknown):
            raise ValueError(f"schema at {where} has no type")
    elif node.type not in _TYPES:
        raise ValueError(f"unsupported type {node.type!r} at {where}")
    node.nullable = bool(schema.get("nullable"))
    node.props = {
        key: _compile(sub, _join(path, key))
        for key, sub in (schema.get("properties") or {}).items()
    }
    node.required = list(schema.get("required") or [])
    extra = schema.get("additionalProperties")
    if extra is None or extra is False:
        node.additional = None
    elif extra is True:
        node.additional = True
    else:
        node.additional = _compile(extra, _join(path, "*"))
    node.items = (
        _compile(schema["items"], f"{path}[]") if "items" in schema else None
    )
    node.enum = list(schema["enum"]) if "enum" in schema else None
    node.minimum = schema.get("minimum")
    node.maximum = schema.get("maximum")
    node.min_length = schema.get("minLength")
    node.max_length = schema.get("maxLength")
    node.min_items = schema.get("minItems")
    node.max_items = schema.get("maxItems")
    node.pattern_src = schema.get("pattern")
    try:
        node.pattern = (
            None if node.pattern_src is None else re.compile(node.pattern_src)
        )
    except re.error as e:
        raise ValueError(f"invalid pattern {node.pattern_src!r} at {where}: {e}")
    # formats other than date-time are ignored, as the apiserver ignores
    # the formats it does not know
    node.date_time = schema.get("format") == "date-time"
    if node.type == "object" or (node.type is None and node.keep_unknown):
        node.ok = _object_ok(node) if node.type == "object" else (lambda v: True)
    elif node.type == "array":
        node.ok = _array_ok(node)
    else:
        node.ok = _scalar_ok(node)
    return node


class Validator:
    """A compiled ``openAPIV3Schema``; see :func:`compile_schema`."""

    def __init__(self, root: _Node):
        self._root = root
        self._status = root.props.get("status")
        # the root as admit() checks it: the schema's own entries for
        # apiVersion/kind/metadata are not applied
        self._fields = {k: c for k, c in root.props.items()
                        if k not in _ROOT_EXEMPT}
        self._fields_ok = {k: c.ok for k, c in self._fields.items()}
        self._required = tuple(root.required)

    def _clean(self, obj: Dict[str, Any]) -> bool:
        fields = self._fields_ok
        keep = self._root.keep_unknown or self._root.additional is True
        for key, val in obj.items():
            child = fields.get(key)
            if child is None:
                if key == "metadata":
                    if type(val) is not dict:
                        return False
                elif key != "apiVersion" and key != "kind" and not keep:
                    return False
            elif not child(val):
                return False
        for key in self._required:
            if key not in obj:
                return False
        return True

    def admit(self, obj: Dict[str, Any], *,
              subtree: Optional[str] = None) -> Tuple[List[str], List[SchemaError]]:
        """Validate the caller's private copy ``obj`` and prune it in place.

        Returns ``(pruned_paths, errors)``: the sorted dotted paths of the
        unknown fields that were removed, and the validation errors in
        document order. With any error the content of ``obj`` is unspecified
        and must not be stored. ``subtree="status"`` looks at ``.status``
        only (a status-subresource write)."""
        errs: List[SchemaError] = []
        pruned: List[str] = []
        if subtree is not None:
            if subtree != "status":
                raise ValueError(f"unsupported subtree {subtree!r}")
            if "status" not in obj:
                return pruned, errs
            node = self._status
            val = obj["status"]
            if node is None:
                del obj["status"]
                if val is not None:
                    pruned.append("status")
            elif val is None and not node.nullable:
                del obj["status"]
            elif not node.ok(val):
                node.walk(val, "status", errs, pruned)
                pruned.sort()
            return pruned, errs
        if self._clean(obj):
            return pruned, errs
        root = self._root
        keep = root.keep_unknown or root.additional is True
        for key in list(obj):
            val = obj[key]
            if key == "metadata":
                if type(val) is not dict:
                    got = _json_type(val)
                    errs.append(SchemaError(
                        "metadata", TYPE_INVALID,
                        f'Invalid value: "{got}": metadata in body must be of '
                        f'type object: "{got}"'))
                continue
            if key == "apiVersion" or key == "kind":
                continue
            child = self._fields.get(key)
            if child is None:
                if not keep:
                    del obj[key]
                    pruned.append(key)
                continue
            if val is None and not child.nullable:
                del obj[key]
                continue
            child.walk(val, key, errs, pruned)
        for key in self._required:
            if key not in obj:
                errs.append(SchemaError(key, REQUIRED, "Required value"))
        pruned.sort()
        return pruned, errs


def compile_schema(openapi_v3_schema: Dict[str, Any]) -> Validator:
    """Compile a CRD version's ``openAPIV3Schema`` once; raises ``ValueError``
    naming the keyword and its path for anything it would not enforce."""
    root = _compile(openapi_v3_schema, "")
    if root.type != "object":
        raise ValueError("the root of a custom resource schema must be of type object")
    return Validator(root)

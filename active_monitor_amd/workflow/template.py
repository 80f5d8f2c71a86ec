"""Argo-style ``{{...}}`` substitution, durations and ``when`` expressions.

Pure functions used by the local executor and the validator — nothing here
starts a process or touches the API.

Substitution works on a *flat* scope: a dict whose keys are the full dotted
references (``"inputs.parameters.msg"``, ``"item"``, ``"item.host"``,
``"steps.probe.outputs.result"`` ...) and whose values are strings. It is a
single pass: a substituted value is never scanned again, so a parameter whose
value happens to contain ``{{workflow.name}}`` comes out literally.

Only tags that look like a dotted reference (``{{ a.b-c.d }}``) are
recognised. Anything else between double braces — Go templates such as
``{{.State.Running}}``, or Argo's ``{{=expr}}`` tags, which the local engine
does not implement — is left untouched by :func:`substitute` (the validator
reports ``{{=`` tags as unsupported).
"""
from __future__ import annotations

import json
import re
from typing import Any, Dict, Iterator, List, Mapping, Optional, Tuple

REF_RE = re.compile(r"\{\{\s*([A-Za-z_][A-Za-z0-9_.\-]*)\s*\}\}")


class TemplateError(Exception):
    """A template could not be rendered or evaluated."""


class UnresolvedReference(TemplateError):
    def __init__(self, ref: str):
        self.ref = ref
        super().__init__("failed to resolve {{%s}}" % ref)


class WhenError(TemplateError):
    def __init__(self, expr: str, detail: str):
        super().__init__(f"invalid when expression {expr!r}: {detail}")


def to_str(value: Any) -> str:
    """Parameter values are strings on the wire; render YAML scalars and
    structures the way Argo does (JSON for non-strings)."""
    if isinstance(value, str):
        return value
    return json.dumps(value)


def substitute(text: Any, scope: Mapping[str, str]) -> Any:
    """Replace every ``{{ref}}`` in ``text``; non-strings pass through."""
    if not isinstance(text, str) or "{{" not in text:
        return text

    def repl(m: "re.Match[str]") -> str:
        ref = m.group(1)
        if ref not in scope:
            raise UnresolvedReference(ref)
        return scope[ref]

    return REF_RE.sub(repl, text)


def substitute_list(values: Any, scope: Mapping[str, str]) -> List[str]:
    """Render an argv-style list. Each element stays exactly one element —
    values are never split or joined."""
    return [str(substitute(v, scope)) for v in (values or [])]


def find_refs(obj: Any) -> Iterator[str]:
    """Every reference mentioned anywhere inside ``obj`` (strings, lists,
    dict values)."""
    if isinstance(obj, str):
        for m in REF_RE.finditer(obj):
            yield m.group(1)
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from find_refs(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from find_refs(v)


def find_strings(obj: Any) -> Iterator[str]:
    if isinstance(obj, str):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from find_strings(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from find_strings(v)


# -- loops ----------------------------------------------------------------


def item_scope(item: Any) -> Dict[str, str]:
    """``{{item}}`` (and ``{{item.KEY}}`` for map items)."""
    scope = {"item": to_str(item)}
    if isinstance(item, dict):
        for k, v in item.items():
            scope[f"item.{k}"] = to_str(v)
    return scope


def item_display_name(name: str, index: int, item: Any) -> str:
    if isinstance(item, (dict, list)):
        return f"{name}({index})"
    return f"{name}({index}:{to_str(item)})"


def parse_with_param(text: str) -> List[Any]:
    try:
        items = json.loads(text)
    except (TypeError, ValueError):
        items = None
    if not isinstance(items, list):
        shown = text if len(text) <= 80 else text[:77] + "..."
        raise TemplateError(f"withParam value is not a JSON list: {shown!r}")
    return items


#: a ``withSequence`` longer than this is refused: every item becomes a task
#: at once, and a count this large on the machine under check is a typo
SEQUENCE_MAX_ITEMS = 10_000
_SEQUENCE_KEYS = ("count", "start", "end", "format")
_INTEGER = re.compile(r"[+-]?\d+$")
#: literal text, one verb out of d x X o with an optional zero-padded width,
#: literal text
_SEQUENCE_FORMAT = re.compile(r"([^%]*)%((?:0\d+)?[dxXo])([^%]*)$")


def _sequence_int(key: str, value: Any) -> int:
    if isinstance(value, int) and not isinstance(value, bool):
        return value
    if isinstance(value, str) and _INTEGER.match(value.strip()):
        return int(value.strip())
    raise TemplateError(f"withSequence.{key} {value!r} is not an integer")


def expand_sequence(seq: Any, scope: Mapping[str, str] = {}) -> List[str]:
    """The items of a ``withSequence``, as strings: ``count`` of them from
    ``start`` (default 0) upwards, or ``start`` to ``end`` inclusive, counting
    down when ``end`` is the smaller. ``{{...}}`` in a field is resolved in
    ``scope`` first. ``format`` is checked against the one shape it may have
    and is never handed to ``%`` as it came."""
    if not isinstance(seq, dict):
        raise TemplateError("withSequence is not a map")
    for key in seq:
        if key not in _SEQUENCE_KEYS:
            raise TemplateError(f"withSequence.{key} is not supported")
    given = {k: substitute(v, scope) for k, v in seq.items() if v is not None}
    if "count" in given and "end" in given:
        raise TemplateError("withSequence takes count or end, not both")
    if "count" not in given and "end" not in given:
        raise TemplateError("withSequence needs count or end")
    start = _sequence_int("start", given["start"]) if "start" in given else 0
    if "count" in given:
        count = _sequence_int("count", given["count"])
        if count < 0:
            raise TemplateError(f"withSequence.count {count} is negative")
        step = 1
    else:
        end = _sequence_int("end", given["end"])
        count = abs(end - start) + 1
        step = 1 if end >= start else -1
    if count > SEQUENCE_MAX_ITEMS:
        raise TemplateError(
            f"withSequence expands to {count} items, more than the cap of "
            f"{SEQUENCE_MAX_ITEMS}")
    prefix, verb, suffix = "", "d", ""
    if "format" in given:
        m = _SEQUENCE_FORMAT.match(given["format"]) if isinstance(given["format"], str) else None
        if m is None:
            raise TemplateError(
                f"withSequence.format {given['format']!r} is not one of %d, %x, %X, %o "
                "(with an optional zero-padded width) inside literal text")
        prefix, verb, suffix = m.groups()
    return [prefix + format(start + i * step, verb) + suffix for i in range(count)]


# -- durations ------------------------------------------------------------

_DURATION_PART = re.compile(r"(\d+(?:\.\d*)?|\.\d+)(ms|s|m|h)")
_UNIT_SECONDS = {"ms": 0.001, "s": 1.0, "m": 60.0, "h": 3600.0}


def parse_duration(value: Any) -> float:
    """Seconds from ``500ms`` / ``2s`` / ``1m`` / ``1h`` / ``1m30s`` or a bare
    number of seconds (int, float or numeric string)."""
    if isinstance(value, bool):
        raise TemplateError(f"invalid duration {value!r}")
    if isinstance(value, (int, float)):
        seconds = float(value)
    else:
        text = str(value).strip() if value is not None else ""
        try:
            seconds = float(text)
        except ValueError:
            pos, seconds = 0, 0.0
            while pos < len(text):
                m = _DURATION_PART.match(text, pos)
                if m is None:
                    raise TemplateError(f"invalid duration {value!r}") from None
                seconds += float(m.group(1)) * _UNIT_SECONDS[m.group(2)]
                pos = m.end()
            if not text:
                raise TemplateError(f"invalid duration {value!r}") from None
    if seconds < 0 or seconds != seconds or seconds == float("inf"):
        raise TemplateError(f"invalid duration {value!r}")
    return seconds


def step_timeout(value: Any, scope: Mapping[str, str] = {}) -> Optional[float]:
    """Seconds of a template's ``timeout``; None when it sets none, which is
    how zero and the empty string read as well. A ``{{...}}`` reference is
    resolved in ``scope`` and then has to give a positive duration."""
    if value is None or value == "" or (not isinstance(value, bool) and value == 0):
        return None
    resolved = substitute(value, scope)
    seconds = parse_duration(resolved)
    if seconds > 0:
        return seconds
    if resolved is value:
        return None  # zero in another spelling: 0s
    raise TemplateError(f"{resolved!r} is not a positive duration")


def active_deadline(value: Any, scope: Mapping[str, str] = {}) -> Optional[float]:
    """Seconds of a template's ``activeDeadlineSeconds``; None when it sets
    none. A positive integer, as a number or as a string, once a ``{{...}}``
    reference is resolved in ``scope``."""
    if value is None:
        return None
    resolved = substitute(value, scope)
    if isinstance(resolved, str) and _INTEGER.match(resolved.strip()):
        resolved = int(resolved.strip())
    if isinstance(resolved, bool) or not isinstance(resolved, int) or resolved < 1:
        raise TemplateError(f"{resolved!r} is not a positive integer")
    return float(resolved)


# -- when -----------------------------------------------------------------
#
#   expr    := and ( '||' and )*
#   and     := primary ( '&&' primary )*
#   primary := '(' expr ')' | operand [ cmp operand ]
#   cmp     := == != < <= > >=
#   operand := 'quoted' | "quoted" | bare word
#
# A primary without a comparison must be the word true or false. The
# expression is only ever tokenised and walked — nothing is executed.

_NUMBER = re.compile(r"[+-]?(?:\d+(?:\.\d*)?|\.\d+)(?:[eE][+-]?\d+)?$")
_TOKEN = re.compile(
    r"""\s*(?:
        (?P<op>==|!=|<=|>=|<|>|&&|\|\||\(|\))
      | '(?P<sq>[^']*)'
      | "(?P<dq>[^"]*)"
      | (?P<word>[^\s()=!<>&|'"]+)
    )""",
    re.VERBOSE,
)
_CMP = ("==", "!=", "<", "<=", ">", ">=")

Token = Tuple[str, str]  # ("op" | "str" | "word", text)


def _tokenize(expr: str) -> List[Token]:
    tokens: List[Token] = []
    pos = 0
    end = len(expr.rstrip())
    while pos < end:
        m = _TOKEN.match(expr, pos)
        if m is None:
            raise WhenError(expr, f"unexpected character at offset {pos}")
        if m.group("op") is not None:
            tokens.append(("op", m.group("op")))
        elif m.group("sq") is not None:
            tokens.append(("str", m.group("sq")))
        elif m.group("dq") is not None:
            tokens.append(("str", m.group("dq")))
        else:
            tokens.append(("word", m.group("word")))
        pos = m.end()
    return tokens


def _compare(left: str, op: str, right: str) -> bool:
    a: Any = left
    b: Any = right
    if _NUMBER.match(left) and _NUMBER.match(right):
        a, b = float(left), float(right)
    if op == "==":
        return a == b
    if op == "!=":
        return a != b
    if op == "<":
        return a < b
    if op == "<=":
        return a <= b
    if op == ">":
        return a > b
    return a >= b


class _WhenParser:
    def __init__(self, expr: str):
        self.expr = expr
        self.tokens = _tokenize(expr)
        self.pos = 0

    def peek(self) -> Token:
        if self.pos < len(self.tokens):
            return self.tokens[self.pos]
        return ("end", "")

    def take(self) -> Token:
        tok = self.peek()
        self.pos += 1
        return tok

    def parse(self) -> bool:
        if not self.tokens:
            raise WhenError(self.expr, "empty expression")
        value = self.expr_()
        if self.peek()[0] != "end":
            raise WhenError(self.expr, f"unexpected {self.peek()[1]!r}")
        return value

    def expr_(self) -> bool:
        value = self.and_()
        while self.peek() == ("op", "||"):
            self.take()
            rhs = self.and_()
            value = value or rhs
        return value

    def and_(self) -> bool:
        value = self.primary()
        while self.peek() == ("op", "&&"):
            self.take()
            rhs = self.primary()
            value = value and rhs
        return value

    def operand(self) -> Token:
        tok = self.take()
        if tok[0] not in ("str", "word"):
            raise WhenError(self.expr, f"expected a value, found {tok[1] or 'end of input'!r}")
        return tok

    def primary(self) -> bool:
        if self.peek() == ("op", "("):
            self.take()
            value = self.expr_()
            if self.take() != ("op", ")"):
                raise WhenError(self.expr, "missing ')'")
            return value
        left = self.operand()
        kind, text = self.peek()
        if kind == "op" and text in _CMP:
            self.take()
            right = self.operand()
            return _compare(left[1], text, right[1])
        if left == ("word", "true"):
            return True
        if left == ("word", "false"):
            return False
        raise WhenError(self.expr, f"expected a comparison after {left[1]!r}")


def eval_when(expr: Any) -> bool:
    """Evaluate an already-substituted ``when`` expression."""
    if isinstance(expr, bool):
        return expr
    return _WhenParser(str(expr)).parse()

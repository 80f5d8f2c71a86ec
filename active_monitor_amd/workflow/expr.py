"""A typed evaluator for the expressions of ``http`` templates.

``successCondition`` and ``outputs.parameters[].valueFrom.expression`` are
written in a subset of the expr language Argo uses. An expression is
tokenised, parsed into a tree and walked; it is never handed to ``eval``,
reads nothing but the environment it is given and does no I/O.

    or      := and ( ('||' | 'or') and )*
    and     := eq ( ('&&' | 'and') eq )*
    eq      := rel ( ('==' | '!=') rel )*
    rel     := word ( ('<' | '<=' | '>' | '>=') word )*
    word    := range ( ('in' | 'contains' | 'startsWith' | 'endsWith'
                        | 'matches') range )*
    range   := unary [ '..' unary ]
    unary   := ('!' | 'not' | '-') unary | postfix
    postfix := primary ( '.' NAME | '[' or ']' )*
    primary := NUMBER | STRING | 'true' | 'false' | 'nil' | NAME
             | NAME '(' [ or (',' or)* ] ')' | '(' or ')' | '[' [ or (',' or)* ] ']'

Values are int, float, string, bool, nil, lists of those, and whatever
``jsonpath`` finds in a JSON document (maps included). Typing is strict,
unlike ``when``: ``200 == "200"`` is false, ``200 < "3"`` is an error, ``&&``
and ``||`` take bools only and do not look at their right side when the left
one decides. ``matches`` is Python's ``re.search``; Argo's is RE2, so a
pattern that uses look-arounds or back-references runs here and not there.
"""
from __future__ import annotations

import json
import re
from typing import Any, Callable, Dict, FrozenSet, List, NamedTuple, Optional, Tuple

from .template import TemplateError


class ExprError(TemplateError):
    """An expression that does not parse (``offset`` is where) or cannot be
    evaluated (``offset`` is None; the message names the operator or function
    and the types it was given)."""

    def __init__(self, message: str, offset: Optional[int] = None):
        self.offset = offset
        super().__init__(message if offset is None else f"{message} at offset {offset}")


class Headers(dict):
    """Response headers as Go's ``http.Header``: canonical name to the list
    of its values. ``lookup`` ignores the case of the name and gives None for
    one that is absent."""

    @staticmethod
    def canonical(name: str) -> str:
        return "-".join(p[:1].upper() + p[1:].lower() for p in name.split("-"))

    def add(self, name: str, value: str) -> None:
        self.setdefault(self.canonical(name), []).append(value)

    def lookup(self, name: str) -> Optional[List[str]]:
        return self.get(self.canonical(name))

    def first(self, name: str) -> Optional[str]:
        values = self.lookup(name)
        return values[0] if values else None


class Names(NamedTuple):
    """What an expression mentions: identifiers with the member names that
    follow them directly (``response.statusCode``), and the functions it
    calls."""

    identifiers: FrozenSet[str]
    functions: FrozenSet[str]


def type_name(value: Any) -> str:
    if value is None:
        return "nil"
    if isinstance(value, bool):
        return "bool"
    if isinstance(value, int):
        return "int"
    if isinstance(value, float):
        return "float"
    if isinstance(value, str):
        return "string"
    if isinstance(value, (list, tuple, range)):
        return "list"
    if isinstance(value, dict):
        return "map"
    return type(value).__name__


def _is_number(value: Any) -> bool:
    return isinstance(value, (int, float)) and not isinstance(value, bool)


def _operands(op: str, a: Any, b: Any) -> ExprError:
    return ExprError(f"{op}: invalid operand types {type_name(a)} and {type_name(b)}")


def _argument(fn: str, *args: Any) -> ExprError:
    return ExprError(f"{fn}(): invalid argument types ({', '.join(map(type_name, args))})")


# -- tokens -------------------------------------------------------------------

_TOKEN = re.compile(
    r"""(?P<float>\d+\.\d+(?:[eE][+-]?\d+)?)
      | (?P<int>\d+)
      | (?P<name>[A-Za-z_][A-Za-z0-9_]*)
      | (?P<op>\|\||&&|==|!=|<=|>=|\.\.|[<>!()\[\],.\-])
      | (?P<quote>['"])
    """,
    re.VERBOSE,
)
_ESCAPES = {"\\": "\\", "'": "'", '"': '"', "n": "\n", "t": "\t"}
_WORD_OPS = {"or": "||", "and": "&&", "not": "!"}
_INFIX_WORDS = ("in", "contains", "startsWith", "endsWith", "matches")

Token = Tuple[str, Any, int]  # (kind, value, offset); kind: int float str name op end


def _string(text: str, start: int) -> Tuple[str, int]:
    """The string literal whose opening quote is at ``start``; returns its
    value and the offset after the closing quote."""
    quote = text[start]
    out: List[str] = []
    pos = start + 1
    while pos < len(text):
        c = text[pos]
        if c == quote:
            return "".join(out), pos + 1
        if c == "\\":
            nxt = text[pos + 1:pos + 2]
            if nxt not in _ESCAPES:
                raise ExprError(f"unknown escape '\\{nxt}'", pos)
            out.append(_ESCAPES[nxt])
            pos += 2
        else:
            out.append(c)
            pos += 1
    raise ExprError("unterminated string", start)


def _tokenize(text: str) -> List[Token]:
    tokens: List[Token] = []
    pos = 0
    while pos < len(text):
        if text[pos].isspace():
            pos += 1
            continue
        m = _TOKEN.match(text, pos)
        if m is None:
            raise ExprError(f"unexpected character {text[pos]!r}", pos)
        if m.group("quote"):
            value, end = _string(text, pos)
            tokens.append(("str", value, pos))
            pos = end
            continue
        if m.group("float"):
            tokens.append(("float", float(m.group("float")), pos))
        elif m.group("int"):
            tokens.append(("int", int(m.group("int")), pos))
        elif m.group("name"):
            word = m.group("name")
            if word in _WORD_OPS:
                tokens.append(("op", _WORD_OPS[word], pos))
            else:
                tokens.append(("name", word, pos))
        else:
            tokens.append(("op", m.group("op"), pos))
        pos = m.end()
    tokens.append(("end", "", len(text)))
    return tokens


# -- tree ---------------------------------------------------------------------
#
# A node is a tuple whose first element says what it is:
#   ("lit", value)  ("name", ident)  ("list", [nodes])  ("call", fn, [nodes])
#   ("member", node, name)  ("index", node, node)  ("not", node)  ("neg", node)
#   ("and", a, b)  ("or", a, b)  ("bin", op, a, b)

Node = Tuple[Any, ...]


class _Parser:
    def __init__(self, text: str):
        self.tokens = _tokenize(text)
        self.pos = 0

    def peek(self) -> Token:
        return self.tokens[self.pos]

    def take(self) -> Token:
        tok = self.tokens[self.pos]
        if tok[0] != "end":
            self.pos += 1
        return tok

    def at_op(self, *ops: str) -> bool:
        kind, value, _ = self.peek()
        return kind == "op" and value in ops

    def expect(self, op: str) -> None:
        kind, value, offset = self.take()
        if kind != "op" or value != op:
            raise ExprError(f"expected {op!r}, found {self._shown(kind, value)}", offset)

    @staticmethod
    def _shown(kind: str, value: Any) -> str:
        return "end of expression" if kind == "end" else repr(value)

    def parse(self) -> Node:
        if self.peek()[0] == "end":
            raise ExprError("empty expression", 0)
        node = self.or_()
        kind, value, offset = self.peek()
        if kind != "end":
            raise ExprError(f"unexpected {self._shown(kind, value)}", offset)
        return node

    def or_(self) -> Node:
        node = self.and_()
        while self.at_op("||"):
            self.take()
            node = ("or", node, self.and_())
        return node

    def and_(self) -> Node:
        node = self.eq()
        while self.at_op("&&"):
            self.take()
            node = ("and", node, self.eq())
        return node

    def eq(self) -> Node:
        node = self.rel()
        while self.at_op("==", "!="):
            op = self.take()[1]
            node = ("bin", op, node, self.rel())
        return node

    def rel(self) -> Node:
        node = self.word()
        while self.at_op("<", "<=", ">", ">="):
            op = self.take()[1]
            node = ("bin", op, node, self.word())
        return node

    def word(self) -> Node:
        node = self.range_()
        while self.peek()[0] == "name" and self.peek()[1] in _INFIX_WORDS:
            op = self.take()[1]
            node = ("bin", op, node, self.range_())
        return node

    def range_(self) -> Node:
        node = self.unary()
        if self.at_op(".."):
            self.take()
            node = ("bin", "..", node, self.unary())
        return node

    def unary(self) -> Node:
        if self.at_op("!"):
            self.take()
            return ("not", self.unary())
        if self.at_op("-"):
            self.take()
            return ("neg", self.unary())
        return self.postfix()

    def postfix(self) -> Node:
        node = self.primary()
        while True:
            if self.at_op("."):
                self.take()
                kind, value, offset = self.take()
                if kind != "name":
                    raise ExprError(
                        f"expected a member name, found {self._shown(kind, value)}", offset)
                node = ("member", node, value)
            elif self.at_op("["):
                self.take()
                index = self.or_()
                self.expect("]")
                node = ("index", node, index)
            else:
                return node

    def items(self, close: str) -> List[Node]:
        found: List[Node] = []
        if self.at_op(close):
            self.take()
            return found
        while True:
            found.append(self.or_())
            if self.at_op(","):
                self.take()
                continue
            self.expect(close)
            return found

    def primary(self) -> Node:
        kind, value, offset = self.take()
        if kind in ("int", "float", "str"):
            return ("lit", value)
        if kind == "name":
            if value in _INFIX_WORDS:
                raise ExprError(f"unexpected {value!r}", offset)
            if value == "true":
                return ("lit", True)
            if value == "false":
                return ("lit", False)
            if value == "nil":
                return ("lit", None)
            if self.at_op("("):
                self.take()
                return ("call", value, self.items(")"))
            return ("name", value)
        if kind == "op" and value == "(":
            node = self.or_()
            self.expect(")")
            return node
        if kind == "op" and value == "[":
            return ("list", self.items("]"))
        raise ExprError(f"expected a value, found {self._shown(kind, value)}", offset)


# -- functions ----------------------------------------------------------------

_JSONPATH_SEGMENT = re.compile(
    r"""\.(?P<name>[A-Za-z_][A-Za-z0-9_\-]*)
      | \[\s*(?P<index>-?\d+)\s*\]
      | \[\s*(?P<q>['"])(?P<key>.*?)(?P=q)\s*\]
    """,
    re.VERBOSE,
)


def _jsonpath(text: Any, path: Any) -> Any:
    if not isinstance(text, str) or not isinstance(path, str):
        raise _argument("jsonpath", text, path)
    if not path.startswith("$"):
        raise ExprError(f"jsonpath(): path {path!r} does not start with $")
    segments: List[Any] = []
    pos = 1
    while pos < len(path):
        m = _JSONPATH_SEGMENT.match(path, pos)
        if m is None:
            raise ExprError(
                f"jsonpath(): path {path!r} is not supported from offset {pos} on "
                "(only .name, [\"name\"] and [index] segments are)")
        if m.group("name") is not None:
            segments.append(m.group("name"))
        elif m.group("index") is not None:
            segments.append(int(m.group("index")))
        else:
            segments.append(m.group("key"))
        pos = m.end()
    try:
        value = json.loads(text)
    except ValueError:
        raise ExprError("jsonpath(): the text is not JSON") from None
    for seg in segments:
        if isinstance(seg, int):
            if not isinstance(value, list) or not 0 <= seg < len(value):
                raise ExprError(f"jsonpath(): {path} leads nowhere ([{seg}] is missing)")
            value = value[seg]
        else:
            if not isinstance(value, dict) or seg not in value:
                raise ExprError(f"jsonpath(): {path} leads nowhere ({seg!r} is missing)")
            value = value[seg]
    return value


def _len(value: Any) -> int:
    if isinstance(value, (str, list, tuple, range, dict)):
        return len(value)
    raise _argument("len", value)


def _int(value: Any) -> int:
    if _is_number(value):
        try:
            return int(value)
        except (ValueError, OverflowError):
            raise ExprError(f"int(): {value!r} has no integer value") from None
    if isinstance(value, str):
        try:
            return int(value.strip())
        except ValueError:
            raise ExprError(f"int(): {value!r} is not an integer") from None
    raise _argument("int", value)


def _float(value: Any) -> float:
    if _is_number(value):
        return float(value)
    if isinstance(value, str):
        try:
            return float(value.strip())
        except ValueError:
            raise ExprError(f"float(): {value!r} is not a number") from None
    raise _argument("float", value)


def render(value: Any) -> str:
    """A value as text: a string as it is, the rest as JSON, nil as ``nil``."""
    if isinstance(value, str):
        return value
    if value is None:
        return "nil"
    if isinstance(value, (range, tuple)):
        value = list(value)
    return json.dumps(value)


def _on_string(name: str, fn: Callable[[str], str]) -> Callable[[Any], str]:
    def call(value: Any) -> str:
        if not isinstance(value, str):
            raise _argument(name, value)
        return fn(value)
    return call


#: name -> (number of arguments, implementation)
FUNCTIONS: Dict[str, Tuple[int, Callable[..., Any]]] = {
    "len": (1, _len),
    "int": (1, _int),
    "float": (1, _float),
    "string": (1, render),
    "lower": (1, _on_string("lower", str.lower)),
    "upper": (1, _on_string("upper", str.upper)),
    "trim": (1, _on_string("trim", str.strip)),
    "jsonpath": (2, _jsonpath),
}


# -- evaluation ---------------------------------------------------------------


def _equal(a: Any, b: Any) -> bool:
    if _is_number(a) and _is_number(b):
        return a == b
    if isinstance(a, (list, tuple, range)) and isinstance(b, (list, tuple, range)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_equal(v, b[k]) for k, v in a.items())
    if type_name(a) != type_name(b):
        return False
    return a == b


def _binary(op: str, a: Any, b: Any) -> Any:
    if op == "==":
        return _equal(a, b)
    if op == "!=":
        return not _equal(a, b)
    if op in ("<", "<=", ">", ">="):
        if not (_is_number(a) and _is_number(b)) and not (
                isinstance(a, str) and isinstance(b, str)):
            raise _operands(op, a, b)
        if op == "<":
            return a < b
        if op == "<=":
            return a <= b
        if op == ">":
            return a > b
        return a >= b
    if op == "..":
        if type_name(a) != "int" or type_name(b) != "int":
            raise _operands(op, a, b)
        return range(a, b + 1)
    if op == "in":
        if isinstance(b, range):
            return type_name(a) == "int" and a in b
        if isinstance(b, (list, tuple)):
            return any(_equal(a, x) for x in b)
        if isinstance(b, dict) and isinstance(a, str):
            return b.lookup(a) is not None if isinstance(b, Headers) else a in b
        raise _operands(op, a, b)
    # contains, startsWith, endsWith, matches
    if not isinstance(a, str) or not isinstance(b, str):
        raise _operands(op, a, b)
    if op == "contains":
        return b in a
    if op == "startsWith":
        return a.startswith(b)
    if op == "endsWith":
        return a.endswith(b)
    try:
        return re.search(b, a) is not None
    except re.error as e:
        raise ExprError(f"matches: invalid pattern {b!r}: {e}") from None


def _evaluate(node: Node, env: Dict[str, Any]) -> Any:
    kind = node[0]
    if kind == "lit":
        return node[1]
    if kind == "name":
        if node[1] not in env:
            raise ExprError(f"unknown name {node[1]!r}")
        return env[node[1]]
    if kind == "list":
        return [_evaluate(n, env) for n in node[1]]
    if kind in ("and", "or"):
        op = "&&" if kind == "and" else "||"
        left = _evaluate(node[1], env)
        if not isinstance(left, bool):
            raise ExprError(f"{op}: invalid operand type {type_name(left)}, expected bool")
        if left is (kind == "or"):
            return left
        right = _evaluate(node[2], env)
        if not isinstance(right, bool):
            raise ExprError(f"{op}: invalid operand type {type_name(right)}, expected bool")
        return right
    if kind == "not":
        value = _evaluate(node[1], env)
        if not isinstance(value, bool):
            raise ExprError(f"!: invalid operand type {type_name(value)}, expected bool")
        return not value
    if kind == "neg":
        value = _evaluate(node[1], env)
        if not _is_number(value):
            raise ExprError(f"-: invalid operand type {type_name(value)}, expected a number")
        return -value
    if kind == "bin":
        return _binary(node[1], _evaluate(node[2], env), _evaluate(node[3], env))
    if kind == "member":
        obj = _evaluate(node[1], env)
        if not isinstance(obj, dict):
            raise ExprError(f".{node[2]}: invalid operand type {type_name(obj)}, expected map")
        return obj.lookup(node[2]) if isinstance(obj, Headers) else obj.get(node[2])
    if kind == "index":
        obj = _evaluate(node[1], env)
        key = _evaluate(node[2], env)
        if isinstance(obj, dict) and isinstance(key, str):
            return obj.lookup(key) if isinstance(obj, Headers) else obj.get(key)
        if isinstance(obj, (list, tuple, range, str)) and type_name(key) == "int":
            if not -len(obj) <= key < len(obj):
                raise ExprError(
                    f"[]: index {key} out of range for a {type_name(obj)} of length {len(obj)}")
            return obj[key]
        raise _operands("[]", obj, key)
    # call
    name, arg_nodes = node[1], node[2]
    if name not in FUNCTIONS:
        raise ExprError(f"unknown function {name!r}")
    arity, fn = FUNCTIONS[name]
    if len(arg_nodes) != arity:
        raise ExprError(f"{name}(): takes {arity} argument{'s' if arity != 1 else ''}, "
                        f"{len(arg_nodes)} given")
    return fn(*[_evaluate(n, env) for n in arg_nodes])


def _collect(node: Node, identifiers: set, functions: set) -> None:
    kind = node[0]
    if kind == "lit":
        return
    if kind in ("name", "member"):
        chain: List[str] = []
        at = node
        while at[0] == "member":
            chain.append(at[2])
            at = at[1]
        if at[0] == "name":
            identifiers.add(".".join([at[1]] + chain[::-1]))
        else:
            _collect(at, identifiers, functions)
        return
    if kind == "call":
        functions.add(node[1])
    for part in node[1:]:
        if isinstance(part, tuple):
            _collect(part, identifiers, functions)
        elif isinstance(part, list):
            for n in part:
                _collect(n, identifiers, functions)


class Expr:
    """A parsed expression."""

    __slots__ = ("text", "_root")

    def __init__(self, text: str, root: Node):
        self.text = text
        self._root = root

    def evaluate(self, env: Dict[str, Any]) -> Any:
        try:
            return _evaluate(self._root, env)
        except RecursionError:
            raise ExprError("expression is nested too deeply") from None

    def evaluate_bool(self, env: Dict[str, Any]) -> bool:
        """The value of a condition: anything but a bool is an error."""
        value = self.evaluate(env)
        if not isinstance(value, bool):
            raise ExprError(f"the value is {type_name(value)}, expected bool")
        return value

    def names(self) -> Names:
        identifiers: set = set()
        functions: set = set()
        _collect(self._root, identifiers, functions)
        return Names(frozenset(identifiers), frozenset(functions))


def parse(text: Any) -> Expr:
    if not isinstance(text, str):
        raise ExprError(f"expression is {type_name(text)}, expected string", 0)
    try:
        return Expr(text, _Parser(text).parse())
    except RecursionError:
        raise ExprError("expression is nested too deeply", 0) from None

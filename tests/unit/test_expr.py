"""The typed expression evaluator of ``http`` templates: precedence, strict
typing, short-circuit, ranges, header lookup, ``jsonpath`` and the errors."""
import pytest

from active_monitor_amd.workflow.expr import ExprError, Headers, Names, parse
from active_monitor_amd.workflow.template import TemplateError


def env(status=200, body='{"status":"ok","items":[{"n":1},{"n":2}],"depth":17}', headers=None):
    found = Headers()
    for name, value in headers or [("content-type", "application/json"),
                                   ("Set-Cookie", "a=1"), ("set-cookie", "b=2")]:
        found.add(name, value)
    return {"response": {"statusCode": status, "body": body, "headers": found}}


def ev(text, **kw):
    return parse(text).evaluate(env(**kw))


@pytest.mark.parametrize("text,want", [
    # literals
    ("200", 200), ("1.5", 1.5), ("'x'", "x"), ('"x"', "x"), ("true", True),
    ("false", False), ("nil", None), ("[200, 204]", [200, 204]), ("[]", []),
    (r"'a\'b'", "a'b"), (r'"a\"b\\c"', 'a"b\\c'), (r"'l1\nl2\tend'", "l1\nl2\tend"),
    ("-3", -3),
    # precedence: || below && below == below < below in below !
    ("true || false && false", True),
    ("(true || false) && false", False),
    ("false && false || true", True),
    ("1 < 2 == true", True),
    ("1 == 1 && 2 == 2", True),
    ("2 in [1, 2] == true", True),
    ("!false && true", True),
    ("!(1 == 2)", True),
    ("not false and true or false", True),
    ("1 < 2 && 2 <= 2 && 3 > 2 && 3 >= 3 && 1 != 2", True),
    ("'a' < 'b'", True), ("'b' <= 'a'", False),
    ("1 < 1.5", True),
    # strict typing
    ('200 == "200"', False), ('200 != "200"', True), ("1 == 1.0", True),
    ("true == 1", False), ("nil == false", False), ("nil == nil", True),
    ("[1, 'a'] == [1, 'a']", True), ("[1] == [1.5]", False),
    # short-circuit: the right side is not looked at
    ('false && (1 < "x")', False),
    ('true || (1 < "x")', True),
    # ranges and in
    ("200 in 200..299", True), ("299 in 200..299", True), ("300 in 200..299", False),
    ("'200' in 200..299", False), ("len(200..299)", 100), ("(1..3)[2]", 3),
    ("204 in [200, 204]", True), ("'204' in [200, 204]", False),
    ("response.statusCode in 200..299", True),
    # strings
    ("'health ok' contains 'ok'", True), ("'health' startsWith 'hea'", True),
    ("'health' endsWith 'th'", True), ("'health' endsWith 'he'", False),
    (r"'v1.22.3' matches '^v\\d+\\.'", True), ("'abc' matches 'b'", True),
    ("'abc' matches '^b'", False),
    ("'abc'[1]", "b"), ("[5, 6][0]", 5),
    # functions
    ("len('abc')", 3), ("len([1, 2])", 2), ("int('42')", 42), ("int(1.9)", 1),
    ("float('1.5')", 1.5), ("float(2)", 2.0), ("string(200)", "200"),
    ("string(true)", "true"), ("string([1, 'a'])", '[1, "a"]'),
    ("lower('AbC')", "abc"), ("upper('AbC')", "ABC"), ("trim('  x \n')", "x"),
    # the environment
    ("response.statusCode", 200),
    ("response.statusCode == 200 && response.body contains 'ok'", True),
    ('response.headers["content-type"]', ["application/json"]),
    ('response.headers["Content-Type"][0]', "application/json"),
    ('response.headers["CONTENT-TYPE"][0] startsWith "application/"', True),
    ('response.headers["set-cookie"]', ["a=1", "b=2"]),
    ('len(response.headers["Set-Cookie"])', 2),
    ('response.headers["x-missing"]', None),
    ('response.headers["x-missing"] == nil', True),
    ('"Content-type" in response.headers', True),
    # jsonpath
    ('jsonpath(response.body, "$.status")', "ok"),
    ('jsonpath(response.body, "$.status") == "ok"', True),
    ('jsonpath(response.body, "$.depth") < 500', True),
    ('jsonpath(response.body, "$.items[1].n")', 2),
    ('jsonpath(response.body, "$[\\"items\\"][0][\'n\']")', 1),
    ('jsonpath(response.body, "$.items")', [{"n": 1}, {"n": 2}]),
    ('len(jsonpath(response.body, "$"))', 3),
    ('jsonpath(response.body, "$.items[0]").n', 1),
    ('jsonpath("[1, 2]", "$[1]")', 2),
])
def test_values(text, want):
    got = ev(text)
    assert got == want and type(got) is type(want), (text, got)


@pytest.mark.parametrize("text,needles", [
    ('200 < "3"', ["<", "int", "string"]),
    ('"a" > 1', [">", "string", "int"]),
    ("true < false", ["<", "bool"]),
    ("1 && true", ["&&", "int", "bool"]),
    ("true && 'x'", ["&&", "string"]),
    ("nil || true", ["||", "nil"]),
    ("!1", ["!", "int"]),
    ("-'x'", ["-", "string"]),
    ("1 in 2", ["in", "int"]),
    ("'a' in 'abc'", ["in", "string"]),
    ("1 contains 1", ["contains", "int"]),
    ("'abc' matches 1", ["matches", "string", "int"]),
    ("'abc' matches '('", ["matches", "pattern"]),
    ("'a'..3", ["..", "string", "int"]),
    ("[1, 2][2]", ["index", "out of range"]),
    ("'abc'[3]", ["index", "out of range"]),
    ("[1]['a']", ["[]", "list", "string"]),
    ("response.statusCode.x", [".x", "int"]),
    ("len(1)", ["len()", "int"]),
    ("len()", ["len()", "1 argument"]),
    ("lower(1)", ["lower()", "int"]),
    ("int('x')", ["int()"]),
    ("int(nil)", ["int()", "nil"]),
    ("float('x')", ["float()"]),
    ("jsonpath(1, '$')", ["jsonpath()", "int", "string"]),
    ("jsonpath(response.body, '$.nope')", ["jsonpath()", "nowhere", "nope"]),
    ("jsonpath(response.body, '$.items[2]')", ["jsonpath()", "nowhere"]),
    ("jsonpath(response.body, '$.status.deeper')", ["jsonpath()", "nowhere"]),
    ("jsonpath(response.body, 'status')", ["jsonpath()", "$"]),
    ("jsonpath(response.body, '$..status')", ["jsonpath()", "not supported"]),
    ("jsonpath(response.body, '$.items[*]')", ["jsonpath()", "not supported"]),
    ("jsonpath('<html>', '$.status')", ["jsonpath()", "not JSON"]),
    ("nosuch(1)", ["unknown function", "nosuch"]),
    ("status == 200", ["unknown name", "status"]),
])
def test_evaluation_errors_name_the_operator_and_the_types(text, needles):
    with pytest.raises(ExprError) as e:
        ev(text)
    assert e.value.offset is None
    for needle in needles:
        assert needle in str(e.value), (text, str(e.value))


def test_an_error_is_a_template_error():
    assert issubclass(ExprError, TemplateError)
    with pytest.raises(TemplateError):
        ev('200 < "3"')


@pytest.mark.parametrize("text,offset", [
    ("", 0),
    ("   ", 0),
    ("1 +", 2),
    ("1 == ", 5),
    ("(1 == 1", 7),
    ("1 == 1)", 6),
    ("[1, 2", 5),
    ("'abc", 0),
    (r"'a\qb'", 2),
    ("a b", 2),
    ("1 2", 2),
    ("response.", 9),
    ("response.'x'", 9),
    ("len(1,)", 6),
    ("1 = 1", 2),
    ("1 & 1", 2),
    ("== 1", 0),
    ("in [1]", 0),
    ("$x", 0),
    ("1; 2", 1),
])
def test_syntax_errors_carry_the_offset(text, offset):
    with pytest.raises(ExprError) as e:
        parse(text)
    assert e.value.offset == offset, str(e.value)
    assert f"offset {offset}" in str(e.value)


def test_a_condition_must_be_a_bool():
    assert parse("response.statusCode == 200").evaluate_bool(env()) is True
    assert parse("response.statusCode == 200").evaluate_bool(env(status=500)) is False
    for text, kind in [("response.statusCode", "int"), ("response.body", "string"),
                       ("nil", "nil"), ("[true]", "list"), ("1.5", "float")]:
        with pytest.raises(ExprError) as e:
            parse(text).evaluate_bool(env())
        assert kind in str(e.value) and "bool" in str(e.value)


def test_nothing_is_ever_executed():
    """What would be code to ``eval`` is a call of an unknown function, an
    unknown name or a syntax error here."""
    with pytest.raises(ExprError) as e:
        parse("__import__('os').system('true')")  # there are no methods to call
    assert e.value.offset == 23
    called = parse("__import__('os').system")
    assert called.names().functions == {"__import__"}
    with pytest.raises(ExprError, match="unknown function '__import__'"):
        called.evaluate(env())
    with pytest.raises(ExprError, match="unknown name '__import__'"):
        parse("__import__").evaluate(env())
    with pytest.raises(ExprError, match="unknown name '__builtins__'"):
        parse("__builtins__.open").evaluate(env())
    with pytest.raises(ExprError, match="unknown function 'open'"):
        parse("open('/etc/passwd')").evaluate(env())
    # attribute access never reaches Python attributes
    assert ev("response.__class__") is None
    with pytest.raises(ExprError):
        ev("response.body.__class__")
    with pytest.raises(ExprError) as e:
        parse("lambda: 1")
    assert e.value.offset is not None


def test_names_for_lint():
    names = parse(
        'response.statusCode in 200..299 && len(response.headers["x"]) > 0 '
        '&& jsonpath(response.body, "$.a") == other.thing && lower(x) == "y"'
    ).names()
    assert isinstance(names, Names)
    assert names.identifiers == {
        "response.statusCode", "response.headers", "response.body", "other.thing", "x"}
    assert names.functions == {"len", "jsonpath", "lower"}
    assert parse("1 == 1").names() == (frozenset(), frozenset())


def test_deep_nesting_is_an_error_not_a_crash():
    with pytest.raises(ExprError):
        parse("(" * 5000 + "1" + ")" * 5000)

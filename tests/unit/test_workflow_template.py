"""Substitution, durations and ``when`` expressions (workflow/template.py):
pure functions, no subprocess."""
import pytest

from active_monitor_amd.workflow.template import (
    TemplateError,
    UnresolvedReference,
    WhenError,
    eval_when,
    find_refs,
    item_display_name,
    item_scope,
    parse_duration,
    parse_with_param,
    substitute,
    substitute_list,
)

SCOPE = {
    "workflow.name": "wf-1",
    "workflow.namespace": "health",
    "workflow.status": "Failed",
    "workflow.parameters.site": "rack-7",
    "inputs.parameters.msg": "hello world",
    "retries": "2",
    "steps.probe.outputs.result": "17",
    "steps.probe.outputs.parameters.lag": "3ms",
    "tasks.build.outputs.result": "ok",
    "tasks.build.outputs.parameters.sha": "abc",
    **item_scope({"host": "db-1", "port": 5432}),
}


@pytest.mark.parametrize("ref,value", [
    ("workflow.name", "wf-1"),
    ("workflow.namespace", "health"),
    ("workflow.status", "Failed"),
    ("workflow.parameters.site", "rack-7"),
    ("inputs.parameters.msg", "hello world"),
    ("retries", "2"),
    ("steps.probe.outputs.result", "17"),
    ("steps.probe.outputs.parameters.lag", "3ms"),
    ("tasks.build.outputs.result", "ok"),
    ("tasks.build.outputs.parameters.sha", "abc"),
    ("item.host", "db-1"),
    ("item.port", "5432"),
])
def test_each_namespace_resolves(ref, value):
    assert substitute("<{{%s}}>" % ref, SCOPE) == f"<{value}>"


def test_scalar_and_map_items():
    assert substitute("{{item}}", item_scope("a")) == "a"
    assert substitute("{{item}}", item_scope(3)) == "3"
    assert substitute("{{item}}", item_scope({"k": 1})) == '{"k": 1}'
    assert item_display_name("s", 1, "b") == "s(1:b)"
    assert item_display_name("s", 0, 7) == "s(0:7)"
    assert item_display_name("s", 2, {"k": 1}) == "s(2)"


def test_spacing_inside_braces_is_accepted():
    assert substitute("{{ item }}/{{  workflow.name}}/{{retries  }}",
                      {**SCOPE, "item": "x"}) == "x/wf-1/2"


def test_substitution_is_single_pass():
    scope = {"inputs.parameters.x": "{{workflow.name}}", "workflow.name": "wf-1"}
    assert substitute("a {{inputs.parameters.x}} b", scope) == "a {{workflow.name}} b"


def test_argv_elements_are_never_split():
    scope = {"inputs.parameters.x": "a b; touch /tmp/pwned"}
    assert substitute_list(["echo", "{{inputs.parameters.x}}", 3], scope) == [
        "echo", "a b; touch /tmp/pwned", "3",
    ]


def test_unresolved_reference_message():
    with pytest.raises(UnresolvedReference) as e:
        substitute("x {{ steps.gone.outputs.result }} y", SCOPE)
    assert str(e.value) == "failed to resolve {{steps.gone.outputs.result}}"
    assert isinstance(e.value, TemplateError)


def test_non_reference_braces_and_non_strings_pass_through():
    assert substitute("docker inspect -f '{{.State.Running}}'", {}) == (
        "docker inspect -f '{{.State.Running}}'"
    )
    assert substitute(5, {}) == 5
    assert substitute(None, {}) is None


def test_find_refs_walks_structures():
    obj = {"a": ["{{ item }}", {"b": "{{inputs.parameters.x}} {{workflow.name}}"}], "c": 1}
    assert sorted(find_refs(obj)) == ["inputs.parameters.x", "item", "workflow.name"]


def test_with_param_must_be_a_json_list():
    assert parse_with_param('[1, "a", {"k": 2}]') == [1, "a", {"k": 2}]
    for bad in ('{"a": 1}', "nope", "3", ""):
        with pytest.raises(TemplateError, match="not a JSON list"):
            parse_with_param(bad)


@pytest.mark.parametrize("text,seconds", [
    ("500ms", 0.5), ("2s", 2.0), ("1m", 60.0), ("1h", 3600.0), ("3", 3.0), (3, 3.0),
    ("0.2s", 0.2), (0.25, 0.25), ("1m30s", 90.0),
])
def test_durations(text, seconds):
    assert parse_duration(text) == pytest.approx(seconds)


@pytest.mark.parametrize("text", ["garbage", "", None, "5 parsecs", "-1", "s", "1x", True, "nan"])
def test_bad_durations(text):
    with pytest.raises(TemplateError, match="invalid duration"):
        parse_duration(text)


@pytest.mark.parametrize("expr,expected", [
    # numeric when both sides are numbers ...
    ("10 > 9", True),
    ("10 < 9", False),
    ("1.0 == 1", True),
    ("'10' > '9'", True),
    ("2 >= 2", True),
    ("2 <= 1", False),
    ("3 != 3.0", False),
    # ... string otherwise ("10" sorts before "9a")
    ("10 > 9a", False),
    ("abc == abc", True),
    ("abc != abd", True),
    ("abc < abd", True),
    # quotes
    ("Failed == 'Failed'", True),
    ('"a b" == \'a b\'', True),
    ("'' == ''", True),
    ("Succeeded == Failed", False),
    # literals
    ("true", True),
    ("false", False),
    ("true == true", True),
    # combination and precedence: && binds tighter than ||
    ("1 == 1 && 2 == 2", True),
    ("1 == 1 && 2 == 3", False),
    ("1 == 2 || 2 == 2", True),
    ("1 == 1 || 1 == 2 && 1 == 3", True),
    ("(1 == 1 || 1 == 2) && 1 == 3", False),
    ("((a == a))", True),
    ("  a==a&&b!=c  ", True),
])
def test_when_table(expr, expected):
    assert eval_when(expr) is expected


@pytest.mark.parametrize("expr", [
    "", "==", "a ==", "== a", "a b", "a == b c", "(a == b", "a == b)", "a && b",
    "a == b &&", "a = b", "a == 'b", "maybe", "a == b || ", "!a",
])
def test_when_malformed(expr):
    with pytest.raises(WhenError, match="invalid when expression"):
        eval_when(expr)


def test_when_never_executes_code(tmp_path, monkeypatch):
    marker = tmp_path / "executed"
    calls = []
    monkeypatch.setattr("os.system", lambda cmd: calls.append(cmd))
    for expr in (
        "__import__('os').system('x') == 1",
        f"__import__('os').system('touch {marker}') == 0",
        f"open('{marker}', 'w') == 1",
    ):
        with pytest.raises(WhenError, match="invalid when expression"):
            eval_when(expr)
    assert calls == []
    assert not marker.exists()

"""The structural-schema compiler and ``Validator.admit`` (kube/schema.py):
every supported keyword passing and failing, the apiserver-style error
strings, pruning, null handling, and the keywords that refuse to compile."""
import copy

import pytest

from active_monitor_amd.kube.schema import (
    INVALID,
    NOT_SUPPORTED,
    REQUIRED,
    TYPE_INVALID,
    compile_schema,
)


def crd(spec_props, **spec_extra):
    """A custom-resource root whose ``spec`` holds the properties under test."""
    return {
        "type": "object",
        "properties": {
            "apiVersion": {"type": "string"},
            "kind": {"type": "string"},
            "metadata": {"type": "object"},
            "spec": dict({"type": "object", "properties": spec_props}, **spec_extra),
            "status": {
                "type": "object",
                "properties": {
                    "successCount": {"type": "integer"},
                    "startedAt": {"type": "string", "format": "date-time"},
                },
            },
        },
    }


def admit(schema, spec, **top):
    obj = dict({"apiVersion": "g/v1", "kind": "K",
                "metadata": {"name": "n", "labels": {"a": "b"}},
                "spec": spec}, **top)
    pruned, errs = compile_schema(schema).admit(obj)
    return obj, pruned, [str(e) for e in errs]


INT = {"type": "integer"}
STR = {"type": "string"}

# (id, property schema, value, expected error or None)
KEYWORD_CASES = [
    ("string-ok", STR, "a", None),
    ("string-bad", STR, 1,
     'spec.f: Invalid value: "integer": spec.f in body must be of type string: "integer"'),
    ("integer-ok", INT, 60, None),
    ("integer-bad", INT, "sixty",
     'spec.f: Invalid value: "string": spec.f in body must be of type integer: "string"'),
    ("integer-integral-float", INT, 60.0, None),
    ("integer-fractional-float", INT, 60.5,
     'spec.f: Invalid value: "number": spec.f in body must be of type integer: "number"'),
    ("integer-not-bool", INT, True,
     'spec.f: Invalid value: "boolean": spec.f in body must be of type integer: "boolean"'),
    ("number-ok", {"type": "number"}, 1.5, None),
    ("number-int-ok", {"type": "number"}, 2, None),
    ("number-not-bool", {"type": "number"}, False,
     'spec.f: Invalid value: "boolean": spec.f in body must be of type number: "boolean"'),
    ("boolean-ok", {"type": "boolean"}, False, None),
    ("boolean-bad", {"type": "boolean"}, 0,
     'spec.f: Invalid value: "integer": spec.f in body must be of type boolean: "integer"'),
    ("object-ok", {"type": "object", "properties": {"a": STR}}, {"a": "x"}, None),
    ("object-bad", {"type": "object", "properties": {"a": STR}}, [],
     'spec.f: Invalid value: "array": spec.f in body must be of type object: "array"'),
    ("array-ok", {"type": "array", "items": STR}, ["a", "b"], None),
    ("array-bad", {"type": "array", "items": STR}, {},
     'spec.f: Invalid value: "object": spec.f in body must be of type array: "object"'),
    ("items-bad", {"type": "array", "items": STR}, ["a", 2],
     'spec.f[1]: Invalid value: "integer": spec.f[1] in body must be of type string: "integer"'),
    ("required-ok", {"type": "object", "required": ["a"], "properties": {"a": STR}},
     {"a": "x"}, None),
    ("required-bad", {"type": "object", "required": ["a"], "properties": {"a": STR}},
     {}, "spec.f.a: Required value"),
    ("additional-schema-ok", {"type": "object", "additionalProperties": INT},
     {"x": 1, "y": 2}, None),
    ("additional-schema-bad", {"type": "object", "additionalProperties": INT},
     {"x": "1"},
     'spec.f.x: Invalid value: "string": spec.f.x in body must be of type integer: "string"'),
    ("additional-true", {"type": "object", "additionalProperties": True},
     {"x": {"deep": [1]}}, None),
    ("enum-ok", {"type": "string", "enum": ["a", "b"]}, "a", None),
    ("enum-bad", {"type": "string", "enum": ["a", "b"]}, "x",
     'spec.f: Unsupported value: "x": supported values: "a", "b"'),
    ("minimum-ok", {"type": "integer", "minimum": 1}, 1, None),
    ("minimum-bad", {"type": "integer", "minimum": 1}, 0,
     "spec.f: Invalid value: 0: spec.f in body should be greater than or equal to 1"),
    ("maximum-ok", {"type": "number", "maximum": 2.5}, 2.5, None),
    ("maximum-bad", {"type": "number", "maximum": 2.5}, 3,
     "spec.f: Invalid value: 3: spec.f in body should be less than or equal to 2.5"),
    ("minLength-ok", {"type": "string", "minLength": 2}, "ab", None),
    ("minLength-bad", {"type": "string", "minLength": 2}, "a",
     'spec.f: Invalid value: "a": spec.f in body should be at least 2 chars long'),
    ("maxLength-ok", {"type": "string", "maxLength": 2}, "ab", None),
    ("maxLength-bad", {"type": "string", "maxLength": 2}, "abc",
     'spec.f: Invalid value: "abc": spec.f in body should be at most 2 chars long'),
    ("pattern-ok", {"type": "string", "pattern": "^a+$"}, "aaa", None),
    ("pattern-bad", {"type": "string", "pattern": "^a+$"}, "ab",
     "spec.f: Invalid value: \"ab\": spec.f in body should match '^a+$'"),
    ("minItems-ok", {"type": "array", "items": INT, "minItems": 1}, [1], None),
    ("minItems-bad", {"type": "array", "items": INT, "minItems": 1}, [],
     "spec.f: Invalid value: []: spec.f in body should have at least 1 items"),
    ("maxItems-ok", {"type": "array", "items": INT, "maxItems": 1}, [1], None),
    ("maxItems-bad", {"type": "array", "items": INT, "maxItems": 1}, [1, 2],
     "spec.f: Invalid value: [1, 2]: spec.f in body should have at most 1 items"),
    ("date-time-ok", {"type": "string", "format": "date-time"},
     "2026-01-02T03:04:05Z", None),
    ("date-time-offset-ok", {"type": "string", "format": "date-time"},
     "2026-01-02T03:04:05.25+01:00", None),
    ("date-time-bad", {"type": "string", "format": "date-time"}, "yesterday",
     'spec.f: Invalid value: "yesterday": spec.f in body must be of type '
     'date-time: "yesterday"'),
    ("date-time-bad-day", {"type": "string", "format": "date-time"},
     "2026-02-30T03:04:05Z",
     'spec.f: Invalid value: "2026-02-30T03:04:05Z": spec.f in body must be of '
     'type date-time: "2026-02-30T03:04:05Z"'),
    ("unknown-format-ignored", {"type": "string", "format": "hostname"}, "!!", None),
    ("nullable-kept", {"type": "string", "nullable": True}, None, None),
    ("int-or-string-int", {"x-kubernetes-int-or-string": True}, 8080, None),
    ("int-or-string-str", {"x-kubernetes-int-or-string": True}, "http", None),
    ("int-or-string-bad", {"x-kubernetes-int-or-string": True}, 1.5,
     'spec.f: Invalid value: "number": spec.f in body must be of type integer '
     'or string: "number"'),
    ("list-type-and-description-ignored",
     {"type": "array", "items": STR, "x-kubernetes-list-type": "atomic",
      "description": "words"}, ["a"], None),
]


@pytest.mark.parametrize("schema,value,want", [c[1:] for c in KEYWORD_CASES],
                         ids=[c[0] for c in KEYWORD_CASES])
def test_keyword(schema, value, want):
    obj, pruned, errs = admit(crd({"f": schema}), {"f": copy.deepcopy(value)})
    assert pruned == []
    assert errs == ([] if want is None else [want])
    if want is None:
        assert obj["spec"] == {"f": value}  # stored as given (60.0 stays 60.0)
        assert type(obj["spec"]["f"]) is type(value)


def test_error_reasons_and_fields():
    schema = crd({
        "n": INT,
        "level": {"type": "string", "enum": ["a", "b"]},
        "size": {"type": "integer", "minimum": 1},
        "wf": {"type": "object", "required": ["source"], "properties": {"source": STR}},
    })
    obj = {"spec": {"n": "x", "level": "c", "size": 0, "wf": {}}}
    _, errs = compile_schema(schema).admit(obj)
    assert [(e.field, e.reason) for e in errs] == [
        ("spec.n", TYPE_INVALID),
        ("spec.level", NOT_SUPPORTED),
        ("spec.size", INVALID),
        ("spec.wf.source", REQUIRED),
    ]
    assert errs[3].detail == "Required value"
    assert str(errs[3]) == "spec.wf.source: Required value"


def test_nested_and_list_index_paths():
    rule = {"type": "object", "required": ["verbs"],
            "properties": {"verbs": {"type": "array", "items": STR}}}
    schema = crd({
        "repeatAfterSec": INT,
        "workflow": {"type": "object", "properties": {
            "rbacRules": {"type": "array", "items": rule},
            "resource": {"type": "object", "required": ["namespace", "source"],
                         "properties": {"namespace": STR,
                                        "source": {"type": "object",
                                                   "properties": {"inline": STR}}}},
        }},
    })
    _, _, errs = admit(schema, {
        "repeatAfterSec": "sixty",
        "workflow": {"resource": {"namespace": "health"},
                     "rbacRules": [{"verbs": ["get"]}, {}]},
    })
    assert errs == [
        'spec.repeatAfterSec: Invalid value: "string": spec.repeatAfterSec in '
        'body must be of type integer: "string"',
        "spec.workflow.resource.source: Required value",
        "spec.workflow.rbacRules[1].verbs: Required value",
    ]


def test_two_errors_in_document_order():
    schema = crd({"a": INT, "b": INT, "c": INT})
    _, _, errs = admit(schema, {"c": "x", "b": 2, "a": "y"})
    assert [e.split(":")[0] for e in errs] == ["spec.c", "spec.a"]


def test_null_is_dropped_without_being_reported():
    schema = crd({"a": STR, "b": {"type": "string", "nullable": True},
                  "o": {"type": "object", "properties": {"x": INT}}})
    obj, pruned, errs = admit(schema, {"a": None, "b": None, "o": {"x": None}})
    assert (pruned, errs) == ([], [])
    assert obj["spec"] == {"b": None, "o": {}}


def test_null_for_a_required_field_is_a_missing_field():
    schema = crd({"a": STR}, required=["a"])
    _, _, errs = admit(schema, {"a": None})
    assert errs == ["spec.a: Required value"]


def test_unknown_fields_are_pruned_sorted_and_metadata_is_left_alone():
    schema = crd({
        "known": STR,
        "list": {"type": "array", "items": {"type": "object", "properties": {"k": STR}}},
        "bare": {"type": "object"},
    })
    obj = {
        "apiVersion": "g/v1", "kind": "K",
        "metadata": {"name": "n", "anything": {"goes": [1, None]}},
        "zzz": 1,
        "spec": {"known": "x", "typo": 1,
                 "list": [{"k": "a"}, {"k": "b", "z": 1, "a": 2}],
                 "bare": {"x": 1}},
    }
    pruned, errs = compile_schema(schema).admit(obj)
    assert errs == []
    assert pruned == ["spec.bare.x", "spec.list[1].a", "spec.list[1].z",
                      "spec.typo", "zzz"]
    assert pruned == sorted(pruned)
    assert obj == {
        "apiVersion": "g/v1", "kind": "K",
        "metadata": {"name": "n", "anything": {"goes": [1, None]}},
        "spec": {"known": "x", "list": [{"k": "a"}, {"k": "b"}], "bare": {}},
    }


def test_preserve_unknown_fields_keeps_keys():
    schema = crd({
        "free": {"type": "object", "x-kubernetes-preserve-unknown-fields": True,
                 "properties": {"n": INT}},
        "any": {"x-kubernetes-preserve-unknown-fields": True},
    })
    spec = {"free": {"n": 1, "other": {"deep": [None, {"x": 1}]}},
            "any": [1, {"a": None}]}
    obj, pruned, errs = admit(schema, copy.deepcopy(spec))
    assert (pruned, errs) == ([], [])
    assert obj["spec"] == spec
    # the properties it does name are still checked
    _, _, errs = admit(schema, {"free": {"n": "1", "other": 2}})
    assert errs == ['spec.free.n: Invalid value: "string": spec.free.n in body '
                    'must be of type integer: "string"']


def test_metadata_must_be_an_object_and_is_not_otherwise_checked():
    schema = crd({"a": STR})
    obj = {"apiVersion": 7, "kind": None, "metadata": "n", "spec": {"a": "x"}}
    pruned, errs = compile_schema(schema).admit(obj)
    assert pruned == []
    assert [str(e) for e in errs] == [
        'metadata: Invalid value: "string": metadata in body must be of type '
        'object: "string"']


def test_status_subtree_only():
    v = compile_schema(crd({"a": STR}, required=["a"]))
    # spec is wrong in every way, and not looked at
    obj = {"metadata": {"name": "n"}, "spec": {"a": 1, "typo": 2},
           "status": {"successCount": 3, "startedAt": "2026-01-02T03:04:05Z",
                      "extra": 1}}
    pruned, errs = v.admit(obj, subtree="status")
    assert (pruned, errs) == (["status.extra"], [])
    assert obj["spec"] == {"a": 1, "typo": 2}
    assert obj["status"] == {"successCount": 3, "startedAt": "2026-01-02T03:04:05Z"}

    _, errs = v.admit({"status": {"successCount": "3"}}, subtree="status")
    assert [str(e) for e in errs] == [
        'status.successCount: Invalid value: "string": status.successCount in '
        'body must be of type integer: "string"']
    _, errs = v.admit({"status": {"startedAt": "yesterday"}}, subtree="status")
    assert [str(e) for e in errs] == [
        'status.startedAt: Invalid value: "yesterday": status.startedAt in body '
        'must be of type date-time: "yesterday"']
    assert v.admit({"spec": {"a": 1}}, subtree="status") == ([], [])
    obj = {"status": {"successCount": None}}
    assert v.admit(obj, subtree="status") == ([], []) and obj == {"status": {}}
    obj = {"status": None}
    assert v.admit(obj, subtree="status") == ([], []) and obj == {}
    with pytest.raises(ValueError):
        v.admit({}, subtree="spec")


def test_a_valid_object_is_left_untouched():
    schema = crd({"a": STR, "l": {"type": "array", "items": INT}}, required=["a"])
    spec = {"a": "x", "l": [1, 2.0]}
    obj, pruned, errs = admit(schema, copy.deepcopy(spec),
                              status={"successCount": 1})
    assert (pruned, errs) == ([], [])
    assert obj["spec"] == spec and obj["status"] == {"successCount": 1}


@pytest.mark.parametrize("keyword,value,path", [
    ("default", 5, "spec.f"),
    ("oneOf", [{"type": "integer"}], "spec.f"),
    ("anyOf", [{"type": "integer"}], "spec.f"),
    ("allOf", [{"type": "integer"}], "spec.f"),
    ("not", {"type": "integer"}, "spec.f"),
    ("x-kubernetes-validations", [{"rule": "self > 0"}], "spec.f"),
])
def test_unsupported_keywords_refuse_to_compile(keyword, value, path):
    schema = crd({"f": {"type": "integer", keyword: value}})
    with pytest.raises(ValueError) as e:
        compile_schema(schema)
    assert keyword in str(e.value) and path in str(e.value)


def test_unsupported_keyword_paths_inside_lists_and_at_the_root():
    schema = crd({"l": {"type": "array",
                        "items": {"type": "object",
                                  "properties": {"k": {"type": "string", "default": "x"}}}}})
    with pytest.raises(ValueError, match=r"'default' at spec\.l\[\]\.k"):
        compile_schema(schema)
    with pytest.raises(ValueError, match="'oneOf' at <root>"):
        compile_schema({"type": "object", "oneOf": []})
    with pytest.raises(ValueError, match="spec.f"):
        compile_schema(crd({"f": {"type": "null"}}))
    with pytest.raises(ValueError, match="spec.f"):
        compile_schema(crd({"f": {"description": "typeless"}}))


def test_enum_compares_numbers_by_value_and_nothing_else_across_types():
    schema = crd({"n": {"type": "integer", "enum": [1, 2]},
                  "x": {"type": "number", "enum": [1.5, 2.0]},
                  "s": {"type": "string", "enum": ["1"]}})
    # 1.0 is the integer 1, as 60.0 satisfies `integer`; 2 is the number 2.0
    assert admit(schema, {"n": 1.0, "x": 2, "s": "1"})[1:] == ([], [])
    _, _, errs = admit(schema, {"n": 3.0, "x": 1})
    assert errs == [
        "spec.n: Unsupported value: 3.0: supported values: 1, 2",
        "spec.x: Unsupported value: 1: supported values: 1.5, 2.0",
    ]
    # a boolean is no number: True is not 1
    flags = crd({"b": {"enum": [1], "x-kubernetes-int-or-string": True},
                 "t": {"type": "boolean", "enum": [True]}})
    assert admit(flags, {"b": 1, "t": True})[1:] == ([], [])
    _, _, errs = admit(flags, {"t": False})
    assert errs == ["spec.t: Unsupported value: false: supported values: true"]

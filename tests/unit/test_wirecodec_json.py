"""wirecodec JSON tests: every implementation must equal the stdlib
expressions it replaces — ``json.dumps(obj, separators=(",", ":")).encode()``
byte for byte, ``json.loads`` value for value and type for type — and where
the stdlib raises, raise an exception of the same class."""
import json
import os
import random
import subprocess
import sys
from collections import OrderedDict

import pytest

from active_monitor_amd.utils import wirecodec as wc

IMPLS = [("python", wc._py_dumpb, wc._py_frame, wc._py_loads_strict,
          wc._py_loads_lenient)]
if wc.HAVE_NATIVE:
    IMPLS.append(("native", wc._native_dumpb, wc._native_frame,
                  wc._native_loads_strict, wc._native_loads_lenient))
IDS = [i[0] for i in IMPLS]

def ref_dumpb(obj):
    return json.dumps(obj, separators=(",", ":")).encode()


def ref_strict(data):
    return json.loads(data)


def ref_lenient(data):
    return json.loads(data.decode("utf-8", "replace"))


def same(a, b):
    """Equal, with equal types at every node (floats by repr: -0.0, nan)."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return (list(a.keys()) == list(b.keys())
                and all(type(k) is str for k in a)
                and all(same(a[k], b[k]) for k in a))
    if isinstance(a, list):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return repr(a) == repr(b)
    return a == b


def outcome(fn, *args):
    try:
        return ("value", fn(*args))
    except Exception as e:  # the class is what is compared
        return ("raises", type(e))


def same_outcome(got, want):
    if got[0] != want[0]:
        return False
    if got[0] == "raises":
        return got[1] is want[1]
    if isinstance(want[1], bytes):
        return got[1] == want[1] and type(got[1]) is bytes
    return same(got[1], want[1])


# -- plain corpus -------------------------------------------------------------

INLINE_WF = """\
apiVersion: argoproj.io/v1alpha1
kind: Workflow
spec:
  entrypoint: start
  templates:
    - name: start
      container:
        image: busybox
        command: [echo, check]
"""

HEALTHCHECK = {
    "apiVersion": "activemonitor.keikoproj.io/v1alpha1",
    "kind": "HealthCheck",
    "metadata": {"name": "hc-00001", "namespace": "health", "uid": "u-1",
                 "resourceVersion": "1234", "generation": 1,
                 "creationTimestamp": "2026-01-01T00:00:00Z"},
    "spec": {
        "level": "namespace", "repeatAfterSec": 3600,
        "workflow": {
            "generateName": "hc-00001-wf-", "workflowtimeout": 30,
            "resource": {"namespace": "health", "serviceAccount": "bench-sa-1",
                         "source": {"inline": INLINE_WF}},
        },
    },
    "status": {"status": "Succeeded", "successCount": 12, "failedCount": 0,
               "totalHealthCheckRuns": 12, "lastFailedWorkflow": "",
               "startedAt": "2026-01-01T00:00:01Z",
               "finishedAt": "2026-01-01T00:00:02Z"},
}
WORKFLOW = {
    "apiVersion": "argoproj.io/v1alpha1", "kind": "Workflow",
    "metadata": {"name": "hc-00001-wf-abcde", "namespace": "health",
                 "labels": {"workflows.argoproj.io/controller-instanceid":
                            "activemonitor-workflows"},
                 "ownerReferences": [{"apiVersion":
                                      "activemonitor.keikoproj.io/v1alpha1",
                                      "kind": "HealthCheck", "name": "hc-00001",
                                      "uid": "u-1", "controller": True}]},
    "spec": {"entrypoint": "start", "activeDeadlineSeconds": 30,
             "ttlStrategy": {"secondsAfterCompletion": 60.5},
             "templates": [{"name": "start", "container": {
                 "image": "busybox", "command": ["echo", "check"]}}]},
    "status": {"phase": "Succeeded", "progress": "1/1", "message": None},
}
EVENT = {
    "apiVersion": "v1", "kind": "Event", "type": "Normal",
    "metadata": {"name": "hc-00001.17a", "namespace": "health"},
    "involvedObject": {"kind": "HealthCheck", "name": "hc-00001"},
    "reason": "Normal", "message": "Successfully \"ran\" workflow\n",
    "count": 3, "firstTimestamp": "2026-01-01T00:00:00Z",
}
STATUS = {"kind": "Status", "apiVersion": "v1", "status": "Failure",
          "message": "healthchecks \"x\" not found", "reason": "NotFound",
          "code": 404}
LIST = {"apiVersion": "activemonitor.keikoproj.io/v1alpha1",
        "kind": "HealthCheckList", "metadata": {"resourceVersion": "77"},
        "items": [HEALTHCHECK, HEALTHCHECK, HEALTHCHECK]}

_ALPHABETS = [
    "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_./ ",
    "\"\\/",
    "".join(chr(c) for c in range(0x20)) + "\x7f",
    "\x80\xa0\xe9\xfc\xff",
    "中文日本語 ￿",
    "\U0001f600\U0001f680\U00010000\U0010ffff",
]


def _rand_str(rng):
    n = rng.choice((0, 1, 3, 8, 8, 20, 40))
    kinds = rng.sample(_ALPHABETS, rng.randint(1, 3))
    return "".join(rng.choice(rng.choice(kinds)) for _ in range(n))


def _rand_tree(rng, depth):
    roll = rng.random()
    if depth <= 0 or roll < 0.45:
        leaf = rng.randrange(7)
        if leaf == 0:
            return _rand_str(rng)
        if leaf == 1:
            return rng.randint(-2**63, 2**63)
        if leaf == 2:
            return rng.randint(-1000, 1000)
        if leaf == 3:
            return rng.choice((rng.uniform(-1e6, 1e6), rng.random(),
                               rng.uniform(-1, 1) * 10.0 ** rng.randint(-300, 300),
                               float(rng.randint(-5, 5))))
        return rng.choice((True, False, None, _rand_str(rng)))
    if roll < 0.75:
        return {_rand_str(rng): _rand_tree(rng, depth - 1)
                for _ in range(rng.randint(0, 4))}
    return [_rand_tree(rng, depth - 1) for _ in range(rng.randint(0, 4))]


def _plain_corpus():
    rng = random.Random(20260101)
    corpus = [HEALTHCHECK, WORKFLOW, EVENT, STATUS, LIST, {}, [],
              {"a": {}, "b": [], "c": [[], {}, [{}]], "d": {"e": {"f": {}}}},
              {"big": "xéy\n" * 50_000}]  # 250 KB: forces buffer growth
    corpus += [_rand_tree(rng, 6) for _ in range(2000)]
    return corpus


PLAIN = _plain_corpus()
PLAIN_BYTES = [ref_dumpb(o) for o in PLAIN]  # the reference, computed once


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_plain_encode_is_byte_identical(name, dumpb, frame, strict, lenient):
    for obj, want in zip(PLAIN, PLAIN_BYTES):
        got = dumpb(obj)
        assert type(got) is bytes and got == want, obj


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_plain_decode_is_equal_and_type_equal(name, dumpb, frame, strict, lenient):
    for raw in PLAIN_BYTES:
        want = json.loads(raw)
        assert same(strict(raw), want), raw[:200]
        assert same(lenient(raw), want), raw[:200]
        assert same(strict(bytearray(raw)), want)


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_plain_decode_of_indented_and_tuple_input(name, dumpb, frame, strict, lenient):
    for obj in PLAIN[:200]:
        pretty = json.dumps(obj, indent=2, ensure_ascii=False).encode("utf-8")
        assert same(strict(b"\r\n\t " + pretty + b" \n"), json.loads(pretty))
    assert dumpb((1, ("a", [2.5]), {"k": ()})) == b'[1,["a",[2.5]],{"k":[]}]'


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_frame(name, dumpb, frame, strict, lenient):
    prefix = b"HTTP/1.1 200 OK\r\nContent-Type: application/json\r\n"
    for obj, payload in list(zip(PLAIN, PLAIN_BYTES))[:300]:
        if obj is None:  # "no body", not the document null: checked below
            continue
        assert frame(prefix, obj) == (
            prefix + b"Content-Length: %d\r\n\r\n" % len(payload) + payload)
    assert frame(b"", {}) == b"Content-Length: 2\r\n\r\n{}"
    assert frame(prefix, None) == prefix + b"Content-Length: 0\r\n\r\n"


def test_native_handles_the_whole_plain_corpus_itself():
    """Without this the tests above could pass with the fast path never
    taken: on plain input the C functions must not answer NotImplemented."""
    assert wc.HAVE_NATIVE, "run `python setup.py build_ext --inplace`"
    from active_monitor_amd import _amcore

    for obj, raw in zip(PLAIN, PLAIN_BYTES):
        assert _amcore.json_dumpb(obj) is not NotImplemented, obj
        assert _amcore.json_frame(b"x\r\n", obj) is not NotImplemented, obj
        assert _amcore.json_loadb(raw) is not NotImplemented, raw[:200]


# -- hostile corpus -----------------------------------------------------------

class _Str(str):
    pass


class _Int(int):
    pass


def _deep_list(depth):
    top = cur = []
    for _ in range(depth):
        nxt = []
        cur.append(nxt)
        cur = nxt
    return top


def _unlink(top):
    # take the chain apart iteratively so dropping it cannot recurse
    while top:
        top = top.pop()


def _hostile_objects():
    cyc = []
    cyc.append(cyc)
    cyc_d = {}
    cyc_d["self"] = cyc_d
    return [
        {1: "a"}, {1.5: "a"}, {True: "a"}, {None: "a"}, {"ok": {2: 3}},
        {(1, 2): "tuple key"},
        OrderedDict([("b", 1), ("a", 2)]), {"k": OrderedDict(a=1)},
        _Str("sub"), {_Str("subkey"): 1}, _Int(7), [_Int(7)],
        float("inf"), float("-inf"), float("nan"), [1.0, float("nan")],
        -0.0, 5e-324, 1e22, 1e16, 1e-7, 1.7976931348623157e308, 0.1 + 0.2,
        2**63, -2**63 - 1, 10**40, -10**40, 2**63 - 1, -2**63,
        "\ud800", "a\udfffb", {"\ud800": "\udc00\ud800"}, "😀",
        b"bytes", {"a": b"bytes"}, {1, 2}, object(), [object()],
        cyc, cyc_d, 3 + 4j,
    ]


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_hostile_encode_matches_stdlib(name, dumpb, frame, strict, lenient):
    for obj in _hostile_objects():
        want = outcome(ref_dumpb, obj)
        assert same_outcome(outcome(dumpb, obj), want), repr(obj)[:80]
        got = outcome(frame, b"p", obj)
        if want[0] == "value":
            assert got == ("value", b"pContent-Length: %d\r\n\r\n%s"
                           % (len(want[1]), want[1]))
        else:
            assert same_outcome(got, want), repr(obj)[:80]


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_depth_100000_encode(name, dumpb, frame, strict, lenient):
    deep = _deep_list(100_000)
    try:
        want = outcome(ref_dumpb, deep)
        assert want == ("raises", RecursionError)
        assert outcome(dumpb, deep) == want
        assert outcome(frame, b"", deep) == want
    finally:
        _unlink(deep)


DOC_300 = ref_dumpb({"kind": "Status", "items": [1, -2.5e3, True, None,
                     "é\U0001f600\\\"", {"a": {"b": []}}],
                     "pad": "x" * 173, "esc": "😀 é \n"})

HOSTILE_DOCS = [
    b'"\\ud800"', b'{"a":"\\ud800"}', b'"\\udc00\\ud800"', b'"\\ud800\\u0041"',
    b'"\\ud83d\\ude00"', b'"\\uD83D\\uDE00"', b'"\\ud83d\\ude0"', b'"\\ud83d\\uzz00"',
    b'"\\u00e9\\u4E2D\\/\\b\\f\\n\\r\\t\\"\\\\"', b'"\\x41"', b'"\\"', b'"\\',
    b'{"a":1,"a":2}', b'{"a":1,"b":2,"a":{"a":3,"a":4}}',
    b"-0", b"1E5", b"1.0", b"-0.0", b"1e400", b"-1e400", b"1e-400", b"0.1e1",
    b"01", b"-", b"-a", b"1.", b"1.e5", b"1e", b"1e+", b".5", b"+1", b"0x10",
    b"9223372036854775807", b"9223372036854775808", b"-9223372036854775809",
    b"1" * 50, b"-" + b"7" * 400, b"1" * 5000,
    b"123456789012345678", b"1234567890123456789", b"0.5" + b"0" * 100,
    b"  \n\t{\r\n \"a\" : [ 1 , 2 ] , \"b\" : { } }  \n",
    json.dumps({"a": [1, {"b": None}], "c": "d"}, indent=2).encode(),
    b"\xef\xbb\xbf{}", b"\xef\xbb\xbf", b'{"a":"\xff"}', b'"\xc0\xaf"',
    b'"\xed\xa0\x80"', b'"\xf4\x90\x80\x80"', b'"\xe2\x82"', b'{"\xe9":1}',
    "é中\U0001f600".join('""').encode("utf-8"),
    b'{"a":1} x', b'{"a":1}{', b"[1,2]]", b"[1,]", b"[,1]", b"{,}", b'{"a"}',
    b'{"a":}', b'{"a":1,}', b"{a:1}", b"{1:1}", b"[1 2]", b"nul", b"nullx",
    b"true", b"false", b"null", b"tru", b"NaN", b"Infinity", b"-Infinity",
    b"[NaN]", b'"a\nb"', b'"a\x00b"', b'"tab\there"', b'"\x7f"', b"\x00",
    b"", b"  ", b"[", b"]", b"{", b'{"', b"[[]", b"'a'",
    '{"a":"﻿"}'.encode("utf-8"),
    '[1,"é"]'.encode("utf-16"), '{"a":1}'.encode("utf-16-le"),
    '{"a":1}'.encode("utf-32-be"),
    b"[" * 100_000, b"[" * 100_000 + b"]" * 100_000,
    b'{"a":' * 100_000, b"[" * 150 + b"]" * 150,
] + [DOC_300[:i] for i in range(len(DOC_300))] + [
    DOC_300 + b"x", DOC_300 + b" ", DOC_300 * 2,
]


def test_hostile_prefix_document_is_300_bytes():
    assert len(DOC_300) == 300


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_hostile_decode_matches_stdlib(name, dumpb, frame, strict, lenient):
    for raw in HOSTILE_DOCS:
        assert same_outcome(outcome(strict, raw), outcome(ref_strict, raw)), raw[:80]
        assert same_outcome(outcome(lenient, raw), outcome(ref_lenient, raw)), raw[:80]


def test_native_never_answers_for_what_the_stdlib_rejects():
    """The fast path never guesses: whatever ``json.loads`` refuses, or reads
    through another encoding than UTF-8, is NotImplemented to the C parser."""
    assert wc.HAVE_NATIVE, "run `python setup.py build_ext --inplace`"
    from active_monitor_amd import _amcore

    for raw in HOSTILE_DOCS:
        got = _amcore.json_loadb(raw)
        want = outcome(ref_strict, raw)
        if want[0] == "raises":
            assert got is NotImplemented, raw[:80]
        elif got is not NotImplemented:
            assert same(got, want[1]), raw[:80]
    assert _amcore.json_loadb("[1]") is NotImplemented  # str: not bytes-like


# -- key cache ----------------------------------------------------------------

KEY_CACHE_SLOTS = 2048  # native/wirejson.h


def _slot(key: bytes) -> int:
    h = 2166136261
    for b in key:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h % KEY_CACHE_SLOTS


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_parsed_documents_are_independent(name, dumpb, frame, strict, lenient):
    raw = ref_dumpb(HEALTHCHECK)
    a, b = strict(raw), strict(raw)
    assert same(a, b) and same(a, HEALTHCHECK)
    a["metadata"]["name"] = "changed"
    a["status"]["extra"] = [1]
    del a["spec"]["workflow"]
    assert same(b, HEALTHCHECK)
    assert same(strict(raw), HEALTHCHECK)


@pytest.mark.parametrize("name,dumpb,frame,strict,lenient", IMPLS, ids=IDS)
def test_colliding_keys_round_trip(name, dumpb, frame, strict, lenient):
    seen = {}
    pair = None
    for i in range(100_000):
        key = b"key%d" % i
        other = seen.setdefault(_slot(key), key)
        if other is not key:
            pair = (other.decode(), key.decode())
            break
    assert pair is not None
    k1, k2 = pair
    raw = ref_dumpb({k1: 1, k2: 2, "nested": {k2: [k1], k1: {k2: k1}}})
    for _ in range(3):  # each parse evicts the other key again
        got = strict(raw)
        assert same(got, {k1: 1, k2: 2, "nested": {k2: [k1], k1: {k2: k1}}})
    many = {"k%05d" % i: i for i in range(10_000)}  # far more keys than slots
    many["x" * 32] = "at the length limit"
    many["y" * 33] = "past it"
    assert same(strict(ref_dumpb(many)), many)
    assert same(strict(ref_dumpb(many)), many)


# -- switches -----------------------------------------------------------------

def test_wire_native_switch_forces_the_python_layer():
    assert wc.HAVE_NATIVE, "run `python setup.py build_ext --inplace`"
    repo = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    code = ("from active_monitor_amd.utils import wirecodec as w;"
            "print(w.NATIVE, w.HAVE_NATIVE, w.dumpb is w._py_dumpb)")
    for value, want in (("0", "False True True"), ("1", "True True False")):
        out = subprocess.run(
            [sys.executable, "-c", code], cwd=repo, capture_output=True,
            text=True, timeout=60, env=dict(os.environ, AM_WIRE_NATIVE=value),
        )
        assert out.returncode == 0, out.stderr[-2000:]
        assert out.stdout.strip() == want


def test_native_codec_is_built_in_tree():
    assert wc.HAVE_NATIVE, "run `python setup.py build_ext --inplace`"

"""Driver for native/check/check_json (see check_json.c): runs the JSON corpus
of tests/unit/test_wirecodec_json.py through the sanitizer-built codec that
is compiled into that executable. Passing means: no sanitizer report, and
every answer is the stdlib's or NotImplemented."""
import os
import sys

import _amcore  # the built-in, sanitizer-built copy

assert "_amcore" in sys.builtin_module_names, "run this with native/check/check_json"

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

import active_monitor_amd  # noqa: E402

# the package's own import of the extension must find the sanitized copy
sys.modules["active_monitor_amd._amcore"] = _amcore
active_monitor_amd._amcore = _amcore

from active_monitor_amd.utils import wirecodec  # noqa: E402

assert wirecodec._json_dumpb is _amcore.json_dumpb

from tests.unit import test_wirecodec_json as corpus  # noqa: E402

n = 0
for obj, raw in zip(corpus.PLAIN, corpus.PLAIN_BYTES):
    assert _amcore.json_dumpb(obj) == raw
    framed = _amcore.json_frame(b"HTTP/1.1 200 OK\r\n", obj)
    assert framed.endswith(b"\r\n\r\n" + (b"" if obj is None else raw))
    assert corpus.same(_amcore.json_loadb(raw), corpus.ref_strict(raw))
    assert corpus.same(_amcore.json_loadb(bytearray(raw)), corpus.ref_strict(raw))
    n += 1

for obj in corpus._hostile_objects():
    want = corpus.outcome(corpus.ref_dumpb, obj)
    for got in (_amcore.json_dumpb(obj), _amcore.json_frame(b"", obj)):
        assert got is NotImplemented or (want[0] == "value" and got.endswith(want[1]))
    n += 1

deep = corpus._deep_list(100_000)
assert _amcore.json_dumpb(deep) is NotImplemented
corpus._unlink(deep)

for raw in corpus.HOSTILE_DOCS:
    want = corpus.outcome(corpus.ref_strict, raw)
    got = _amcore.json_loadb(raw)
    assert got is NotImplemented or (want[0] == "value" and corpus.same(got, want[1])), raw[:80]
    n += 1

for impl in corpus.IMPLS:
    corpus.test_parsed_documents_are_independent(*impl)
    corpus.test_colliding_keys_round_trip(*impl)

print(f"check_json: {n} documents through the sanitized codec, no report")

"""The run-request predicate: when is a request to run a check pending."""
from datetime import datetime

import pytest

from active_monitor_amd import api
from active_monitor_amd.api import (
    RUN_HANDLED_ANNOTATION,
    RUN_REQUEST_ANNOTATION,
    RUN_REQUESTED_ANNOTATION,
    RUN_WORKFLOW_ANNOTATION,
    ObjectMeta,
    new_run_token,
    pending_run_request,
)

T1 = "2026-01-02T03:04:05.000006Z"
T2 = "2026-01-02T03:04:06.000000Z"


def test_the_keys_are_under_the_group():
    assert RUN_REQUESTED_ANNOTATION == "activemonitor.keikoproj.io/run-requested"
    assert RUN_HANDLED_ANNOTATION == "activemonitor.keikoproj.io/run-handled"
    assert RUN_WORKFLOW_ANNOTATION == "activemonitor.keikoproj.io/run-workflow"
    assert RUN_REQUEST_ANNOTATION == "activemonitor.keikoproj.io/run-request"
    for name in ("RUN_REQUESTED_ANNOTATION", "RUN_HANDLED_ANNOTATION",
                 "RUN_WORKFLOW_ANNOTATION", "pending_run_request"):
        assert name in api.__all__


@pytest.mark.parametrize("metadata", [
    {},
    {"name": "x"},
    {"annotations": None},
    {"annotations": {}},
    {"annotations": {"other": "value"}},
    {"annotations": {RUN_HANDLED_ANNOTATION: T1}},  # handled alone asks nothing
], ids=["empty", "no-annotations", "null", "none-set", "other-key", "handled-only"])
def test_absent_annotation_is_no_request(metadata):
    assert pending_run_request(metadata) is None


def test_empty_annotation_is_no_request():
    assert pending_run_request({"annotations": {RUN_REQUESTED_ANNOTATION: ""}}) is None
    # not even when it differs from what was handled
    assert pending_run_request({"annotations": {
        RUN_REQUESTED_ANNOTATION: "", RUN_HANDLED_ANNOTATION: T1}}) is None


def test_requested_equal_to_handled_is_served():
    assert pending_run_request({"annotations": {
        RUN_REQUESTED_ANNOTATION: T1, RUN_HANDLED_ANNOTATION: T1,
        RUN_WORKFLOW_ANNOTATION: "wf-abc"}}) is None


def test_requested_different_from_handled_is_pending():
    assert pending_run_request({"annotations": {RUN_REQUESTED_ANNOTATION: T1}}) == T1
    assert pending_run_request({"annotations": {
        RUN_REQUESTED_ANNOTATION: T2, RUN_HANDLED_ANNOTATION: T1}}) == T2
    # the token is opaque: an earlier time, or no time at all, is a request too
    assert pending_run_request({"annotations": {
        RUN_REQUESTED_ANNOTATION: T1, RUN_HANDLED_ANNOTATION: T2}}) == T1
    assert pending_run_request({"annotations": {
        RUN_REQUESTED_ANNOTATION: "again please", RUN_HANDLED_ANNOTATION: T2}}) == "again please"
    assert pending_run_request({"annotations": {
        RUN_REQUESTED_ANNOTATION: T1, RUN_HANDLED_ANNOTATION: ""}}) == T1


@pytest.mark.parametrize("value", [1, 1.5, True, ["x"], {"a": "b"}, None])
def test_non_string_request_is_no_request(value):
    assert pending_run_request({"annotations": {RUN_REQUESTED_ANNOTATION: value}}) is None


@pytest.mark.parametrize("handled", [1, True, ["x"], None])
def test_non_string_handled_never_equals_a_token(handled):
    assert pending_run_request({"annotations": {
        RUN_REQUESTED_ANNOTATION: T1, RUN_HANDLED_ANNOTATION: handled}}) == T1


@pytest.mark.parametrize("annotations", ["text", 3, ["a"]])
def test_annotations_of_another_type_are_no_request(annotations):
    assert pending_run_request({"annotations": annotations}) is None


def test_parsed_metadata_is_read_the_same_way():
    raw = {"name": "x", "annotations": {RUN_REQUESTED_ANNOTATION: T2,
                                        RUN_HANDLED_ANNOTATION: T1}}
    assert pending_run_request(ObjectMeta.from_dict(raw)) == T2
    raw["annotations"][RUN_HANDLED_ANNOTATION] = T2
    assert pending_run_request(ObjectMeta.from_dict(raw)) is None
    assert pending_run_request(ObjectMeta()) is None


def test_a_fresh_token_is_an_rfc3339_utc_time_to_the_microsecond():
    token = new_run_token()
    assert len(token) == len(T1) and token.endswith("Z") and token[19] == "."
    assert datetime.strptime(token, "%Y-%m-%dT%H:%M:%S.%fZ").year >= 2024
    assert pending_run_request({"annotations": {RUN_REQUESTED_ANNOTATION: token}}) == token


def test_statusz_reports_on_demand_runs_next_to_completed_runs(run):
    import asyncio
    import json
    import urllib.request

    from active_monitor_amd.engine.endpoints import serve_endpoints

    class FakeRec:
        reconcile_count = 9
        completed_runs = 5
        on_demand_runs = 2
        repeat_timers_by_name = {}

        def active_watches(self):
            return 0

    class FakeManager:
        ready = True
        queue = []
        reconciler = FakeRec()

    def fetch(url):
        with urllib.request.urlopen(url, timeout=5) as r:
            return json.loads(r.read())

    async def go():
        servers = await serve_endpoints(FakeManager(), health=("127.0.0.1", 0))
        try:
            port = servers[0].sockets[0].getsockname()[1]
            stats = await asyncio.get_running_loop().run_in_executor(
                None, fetch, f"http://127.0.0.1:{port}/statusz")
        finally:
            for s in servers:
                s.close()
        keys = list(stats)
        assert stats["on_demand_runs"] == 2 and stats["completed_runs"] == 5
        assert keys.index("on_demand_runs") == keys.index("completed_runs") + 1

    run(go())

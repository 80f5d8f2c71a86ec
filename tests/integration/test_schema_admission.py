"""Admission by the CRD schema in the store and over the REST frontend:
what is refused, what is pruned, what the three field-validation modes do,
and that a refused write leaves no trace."""
import asyncio
import copy
import json
import os
import time

import aiohttp
import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.engine import Manager
from active_monitor_amd.kube import (
    BadRequestError,
    InvalidError,
    MemoryApiServer,
    MemoryClient,
)
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.memory import healthcheck_schemas
from active_monitor_amd.kube.persist import JOURNAL_FILE
from active_monitor_amd.kube.server import ApiServerFrontend
from active_monitor_amd.workflow import ScriptedWorkflowEngine

from .conftest import make_hc

HC = (API_VERSION, "HealthCheck")
COLLECTION = f"/apis/{API_VERSION}/namespaces/health/healthchecks"
TYPE_ERR = ('spec.repeatAfterSec: Invalid value: "string": spec.repeatAfterSec '
            'in body must be of type integer: "string"')
JSON = {"Content-Type": "application/json"}
MERGE = {"Content-Type": "application/merge-patch+json"}


class ValidatingEnv:
    """The frontend over a store that validates HealthChecks, an HttpClient,
    and a raw aiohttp session for looking at status codes and headers."""

    def __init__(self, server=None):
        self.server = server or MemoryApiServer(schemas=healthcheck_schemas())
        self.frontend = ApiServerFrontend(self.server)

    async def __aenter__(self):
        await self.frontend.start()
        self.client = HttpClient(self.frontend.url, qps=0)
        await self.client.start()
        self.raw = aiohttp.ClientSession()
        return self

    async def __aexit__(self, *exc):
        await self.raw.close()
        await self.client.close()
        await self.frontend.stop()
        self.server.close()

    async def send(self, method, path, body, headers=JSON, **params):
        """(status, decoded body, Warning header values)."""
        data = body if isinstance(body, (bytes, str)) else json.dumps(body)
        async with self.raw.request(method, self.frontend.url + path, data=data,
                                    headers=headers, params=params) as resp:
            return (resp.status, json.loads(await resp.text()),
                    resp.headers.getall("Warning", []))

    def stored(self, name):
        return self.server.get(*HC, "health", name)

    def absent(self, name):
        with pytest.raises(Exception) as e:
            self.stored(name)
        return e.value.code == 404


def invalid_hc(name="bad"):
    hc = make_hc(name=name)
    hc["spec"]["repeatAfterSec"] = "sixty"
    return hc


def typo_hc(name="typo"):
    hc = make_hc(name=name, repeat=0)
    hc["spec"]["repeatAfterSecs"] = 60
    return hc


async def next_event(sub, timeout=10):
    return await asyncio.wait_for(sub.__anext__(), timeout)


# -- 1: create ---------------------------------------------------------------

def test_invalid_create_is_422_with_the_full_status_body(run):
    async def go():
        async with ValidatingEnv() as env:
            status, body, warnings = await env.send("POST", COLLECTION, invalid_hc())
            assert status == 422 and warnings == []
            assert body == {
                "kind": "Status", "apiVersion": "v1", "status": "Failure",
                "reason": "Invalid", "code": 422,
                "message": 'HealthCheck.activemonitor.keikoproj.io "bad" is '
                           f"invalid: {TYPE_ERR}",
                "details": {
                    "name": "bad", "group": "activemonitor.keikoproj.io",
                    "kind": "HealthCheck",
                    "causes": [{
                        "reason": "FieldValueTypeInvalid",
                        "message": TYPE_ERR.split(": ", 1)[1],
                        "field": "spec.repeatAfterSec",
                    }],
                },
            }
            assert env.absent("bad")
            assert env.server.rejected_writes == 1
            assert env.server.resource_version() == "0"

            # several errors are listed in brackets; the client carries the causes
            two = invalid_hc("two")
            del two["spec"]["workflow"]["resource"]["source"]
            with pytest.raises(InvalidError) as e:
                await env.client.create(two)
            assert e.value.message == (
                'HealthCheck.activemonitor.keikoproj.io "two" is invalid: '
                f"[spec.workflow.resource.source: Required value, {TYPE_ERR}]")
            assert [c["field"] for c in e.value.causes] == [
                "spec.workflow.resource.source", "spec.repeatAfterSec"]
            assert [c["reason"] for c in e.value.causes] == [
                "FieldValueRequired", "FieldValueTypeInvalid"]
            assert env.server.rejected_writes == 2

    run(go())


# -- 2: update and patch leave no trace ----------------------------------------

async def refused_writes_leave_no_trace(env, journal=None):
    made = await env.client.create(make_hc(name="good"))
    rv = made["metadata"]["resourceVersion"]
    path = f"{COLLECTION}/good"
    sub = env.client.watch(*HC, "health")
    try:
        first = await next_event(sub)
        assert first["type"] == "ADDED"
        size = os.path.getsize(journal) if journal else None
        history = len(env.server._history)

        broken = copy.deepcopy(made)
        broken["spec"]["repeatAfterSec"] = "sixty"
        status, body, _ = await env.send("PUT", path, broken)
        assert status == 422 and TYPE_ERR in body["message"]
        status, body, _ = await env.send(
            "PATCH", path, {"spec": {"repeatAfterSec": "sixty"}}, headers=MERGE)
        assert status == 422 and TYPE_ERR in body["message"]
        with pytest.raises(InvalidError):
            await env.client.patch(*HC, "health", "good",
                                   {"spec": {"workflow": {"resource": {"source": None}}}})

        assert env.server.rejected_writes == 3
        assert await env.client.get(*HC, "health", "good") == made
        assert env.server.resource_version() == rv
        assert len(env.server._history) == history
        if journal:
            assert os.path.getsize(journal) == size

        # the next thing the watch sees is the next accepted write
        await env.client.patch(*HC, "health", "good", {"spec": {"repeatAfterSec": 5}})
        ev = await next_event(sub)
        assert ev["type"] == "MODIFIED"
        assert ev["object"]["spec"]["repeatAfterSec"] == 5
        assert int(ev["object"]["metadata"]["resourceVersion"]) == int(rv) + 1
        if journal:
            assert os.path.getsize(journal) > size
    finally:
        sub.close()


def test_refused_update_and_patch_leave_no_trace(run):
    async def go():
        async with ValidatingEnv() as env:
            await refused_writes_leave_no_trace(env)

    run(go())


def test_refused_update_and_patch_leave_the_journal_alone(run, tmp_path):
    d = str(tmp_path / "data")

    async def go():
        server = MemoryApiServer.open(d, schemas=healthcheck_schemas())
        async with ValidatingEnv(server) as env:
            await refused_writes_leave_no_trace(env, os.path.join(d, JOURNAL_FILE))

    run(go())


# -- 3: the status subresource -------------------------------------------------

def test_status_writes_are_checked_on_the_status_subtree(run):
    async def go():
        async with ValidatingEnv() as env:
            made = await env.client.create(make_hc(name="st"))
            path = f"{COLLECTION}/st/status"
            for status_doc, field, kind in (
                ({"successCount": "3"}, "status.successCount", "integer"),
                ({"startedAt": "yesterday"}, "status.startedAt", "date-time"),
            ):
                obj = dict(made, status=status_doc)
                code, body, _ = await env.send("PUT", path, obj)
                assert code == 422
                assert body["details"]["causes"][0]["field"] == field
                assert f"{field} in body must be of type {kind}" in body["message"]
                with pytest.raises(InvalidError):
                    await env.client.patch(*HC, "health", "st", {"status": status_doc},
                                           subresource="status")
            assert "status" not in env.stored("st")
            assert env.server.rejected_writes == 4

            # the spec of a status write is not looked at, as it is not stored
            obj = dict(made, spec={"repeatAfterSec": "sixty"},
                       status={"successCount": 3,
                               "startedAt": "2026-01-02T03:04:05Z", "extra": 1})
            code, body, warnings = await env.send("PUT", path, obj)
            assert code == 200
            assert warnings == ['299 - "unknown field \\"status.extra\\""']
            assert body["status"] == {"successCount": 3,
                                      "startedAt": "2026-01-02T03:04:05Z"}
            assert body["spec"] == made["spec"]

    run(go())


# -- 4: unknown fields and the three modes ---------------------------------------

def test_unknown_field_under_warn_strict_and_ignore(run):
    async def go():
        async with ValidatingEnv() as env:
            sub = env.client.watch(*HC, "health")
            try:
                # absent means Warn
                status, body, warnings = await env.send("POST", COLLECTION, typo_hc())
                assert status == 201
                assert warnings == ['299 - "unknown field \\"spec.repeatAfterSecs\\""']
                assert "repeatAfterSecs" not in body["spec"]
                got = await env.client.get(*HC, "health", "typo")
                assert "repeatAfterSecs" not in got["spec"]
                ev = await next_event(sub)
                assert ev["type"] == "ADDED"
                assert ev["object"]["metadata"]["name"] == "typo"
                assert "repeatAfterSecs" not in ev["object"]["spec"]
            finally:
                sub.close()

            status, body, warnings = await env.send(
                "POST", COLLECTION, typo_hc("strict"), fieldValidation="Strict")
            assert status == 400 and warnings == []
            assert body["reason"] == "BadRequest" and body["code"] == 400
            assert body["message"] == (
                'HealthCheck in version "v1alpha1" cannot be handled as a '
                'HealthCheck: strict decoding error: unknown field '
                '"spec.repeatAfterSecs"')
            assert env.absent("strict")

            two = typo_hc("strict2")
            two["spec"]["workflow"]["timeout"] = 3
            with pytest.raises(BadRequestError) as e:
                await env.client.create(two, field_validation="Strict")
            assert e.value.message.endswith(
                'strict decoding error: unknown field "spec.repeatAfterSecs", '
                'unknown field "spec.workflow.timeout"')
            assert env.absent("strict2")

            status, body, warnings = await env.send(
                "POST", COLLECTION, typo_hc("ignore"), fieldValidation="Ignore")
            assert status == 201 and warnings == []
            assert "repeatAfterSecs" not in env.stored("ignore")["spec"]

            status, body, _ = await env.send(
                "POST", COLLECTION, make_hc(name="bogus"), fieldValidation="bogus")
            assert status == 400 and body["reason"] == "BadRequest"
            assert "fieldValidation" in body["message"]
            assert env.absent("bogus")

            # a valid object answers as it always did: no header
            status, _, warnings = await env.send(
                "POST", COLLECTION, make_hc(name="fine"), fieldValidation="Strict")
            assert status == 201 and warnings == []

    run(go())


def test_http_client_collects_warnings(run, caplog):
    async def go():
        async with ValidatingEnv() as env:
            made = await env.client.create(typo_hc("w"), field_validation="Warn")
            assert "repeatAfterSecs" not in made["spec"]
            assert list(env.client.warnings) == ['unknown field "spec.repeatAfterSecs"']
            made["spec"]["oops"] = {"a": 1}
            await env.client.update(made, field_validation="Warn")
            assert list(env.client.warnings)[-1] == 'unknown field "spec.oops"'
            await env.client.update(made, field_validation="Ignore")
            assert len(env.client.warnings) == 2
            # unset: the pooled path, which does not look at response headers
            made["spec"]["again"] = 1
            out = await env.client.update(made)
            assert "again" not in out["spec"] and len(env.client.warnings) == 2

    with caplog.at_level("WARNING", logger="active_monitor_amd.kube.http"):
        run(go())
    assert 'apiserver warning: unknown field "spec.oops"' in caplog.text


def test_memory_client_passes_mode_and_warnings_through(run):
    async def go():
        client = MemoryClient(MemoryApiServer(schemas=healthcheck_schemas()))
        warnings = []
        made = await client.create(typo_hc("m"), warnings=warnings)
        assert warnings == ["spec.repeatAfterSecs"]
        assert "repeatAfterSecs" not in made["spec"]
        made["spec"]["x"] = 1
        with pytest.raises(BadRequestError):
            await client.update(made, field_validation="Strict")
        quiet = []
        await client.update(made, field_validation="Ignore", warnings=quiet)
        assert quiet == []
        with pytest.raises(InvalidError):
            await client.patch(*HC, "health", "m", {"status": {"failedCount": "1"}},
                               subresource="status")
        made["status"] = {"failedCount": 1, "typo": 2}
        out = await client.update_status(made, warnings=warnings)
        assert warnings == ["spec.repeatAfterSecs", "status.typo"]
        assert out["status"] == {"failedCount": 1}
        assert client.server.rejected_writes == 2

    run(go())


# -- 5: server-side apply ----------------------------------------------------------

def test_apply_patch_upsert_of_an_invalid_object_is_422(run):
    async def go():
        async with ValidatingEnv() as env:
            apply = {"Content-Type": "application/apply-patch+yaml"}
            status, body, _ = await env.send(
                "PATCH", f"{COLLECTION}/up", json.dumps(invalid_hc("up")), headers=apply)
            assert status == 422 and TYPE_ERR in body["message"]
            assert body["details"]["name"] == "up"
            assert env.absent("up") and env.server.rejected_writes == 1
            status, body, _ = await env.send(
                "PATCH", f"{COLLECTION}/up", json.dumps(make_hc(name="up")), headers=apply)
            assert status == 200 and env.stored("up")["spec"]["repeatAfterSec"] == 1

    run(go())


# -- 6: the default is unchanged -----------------------------------------------------

def test_a_bare_store_still_stores_anything(run):
    async def go():
        async with ValidatingEnv(MemoryApiServer()) as env:
            hc = invalid_hc("anything")
            hc["spec"]["repeatAfterSecs"] = 60
            status, body, warnings = await env.send(
                "POST", COLLECTION, hc, fieldValidation="Strict")
            assert status == 201 and warnings == []
            assert env.stored("anything")["spec"] == hc["spec"]
            assert env.server.rejected_writes == 0

    run(go())


def test_a_schema_can_be_installed_later_and_only_for_its_kind():
    server = MemoryApiServer()
    server.create(invalid_hc("before"))
    server.install_schema(*HC, healthcheck_schemas()[HC])
    with pytest.raises(InvalidError):
        server.create(invalid_hc("after"))
    # other kinds are stored as given
    server.create({"apiVersion": "v1", "kind": "ConfigMap",
                   "metadata": {"name": "cm", "namespace": "health"},
                   "data": 7, "whatever": None})
    # a dict is compiled on the way in, and refused if it cannot be enforced
    with pytest.raises(ValueError, match="default"):
        server.install_schema("v1", "ConfigMap", {
            "type": "object",
            "properties": {"data": {"type": "object", "default": {}}}})


# -- 7: stored objects are not re-validated ---------------------------------------------

def test_objects_in_a_data_dir_are_not_revalidated_on_load(tmp_path):
    d = str(tmp_path / "data")
    server = MemoryApiServer.open(d)
    server.create(invalid_hc("old"))
    server.close()

    server = MemoryApiServer.open(d, schemas=healthcheck_schemas())
    try:
        old = server.get(*HC, "health", "old")
        assert old["spec"]["repeatAfterSec"] == "sixty"
        with pytest.raises(InvalidError):
            server.update(dict(old, metadata=dict(old["metadata"], labels={"a": "b"})))
        assert server.get(*HC, "health", "old") == old
        # mending it is a write like any other
        old["spec"]["repeatAfterSec"] = 60
        assert server.update(old)["spec"]["repeatAfterSec"] == 60
    finally:
        server.close()


# -- 8: the controller's own writes satisfy its own CRD -----------------------------------

def test_controller_runs_over_a_validating_store(run):
    def policy(wf):
        name = wf["metadata"]["name"]
        if name.startswith("sick-wf-"):
            return ("Failed", "check failed")
        return ("Succeeded", "")

    async def go():
        server = MemoryApiServer(schemas=healthcheck_schemas())
        client = MemoryClient(server)
        manager = Manager(client, max_workers=4)
        engine = ScriptedWorkflowEngine(client, policy=policy)
        await engine.start()
        await manager.start()
        try:
            await client.create(make_hc(name="well", repeat=1))
            sick = make_hc(name="sick", repeat=1, remedy=True)
            sick["spec"]["remedyRunsLimit"] = 1000
            sick["spec"]["remedyResetInterval"] = 3600
            await client.create(sick)

            deadline = time.monotonic() + 30
            while True:
                well = (await client.get(*HC, "health", "well")).get("status") or {}
                ill = (await client.get(*HC, "health", "sick")).get("status") or {}
                if (well.get("successCount", 0) >= 3 and ill.get("failedCount", 0) >= 3
                        and ill.get("remedyTotalRuns", 0) >= 3):
                    break
                assert time.monotonic() < deadline, (well, ill)
                await asyncio.sleep(0.05)
            assert well["status"] == "Succeeded" and ill["status"] == "Failed"
            assert ill["remedySuccessCount"] >= 1
        finally:
            await manager.stop()
            await engine.stop()
        assert server.rejected_writes == 0
        assert server.op_counts["update_status"] > 6

    run(go(), timeout=45)


# -- details ----------------------------------------------------------------------------

def test_warning_headers_carry_nothing_but_printable_ascii(run):
    """Pruned paths are made of the client's own JSON keys: one with CR LF in
    it must not start a header line of its own, and no raw non-ASCII byte
    goes into the head."""
    async def go():
        async with ValidatingEnv() as env:
            hc = make_hc(name="inject")
            hc["spec"]["a\r\nX-Injected: yes\r\n\r\nbody"] = 1
            hc["spec"]["grüße"] = 1
            hc["spec"]['q"uo\\te'] = 1
            hc["spec"]["100%"] = 1
            async with env.raw.post(env.frontend.url + COLLECTION, data=json.dumps(hc),
                                    headers=JSON) as resp:
                assert resp.status == 201
                assert "X-Injected" not in resp.headers
                warnings = resp.headers.getall("Warning")
                body = json.loads(await resp.text())
            assert body["spec"] == make_hc(name="inject")["spec"]
            assert sorted(warnings) == sorted([
                '299 - "unknown field \\"spec.a%0D%0AX-Injected: yes%0D%0A%0D%0Abody\\""',
                '299 - "unknown field \\"spec.gr%C3%BC%C3%9Fe\\""',
                '299 - "unknown field \\"spec.q\\"uo\\\\te\\""',
                '299 - "unknown field \\"spec.100%25\\""',
            ])
            for w in warnings:
                assert all(0x20 <= ord(c) <= 0x7E for c in w)
            # the connection is still in step: the next request is answered
            assert (await env.client.get(*HC, "health", "inject"))["spec"] == body["spec"]

    run(go())


def test_a_refused_generate_name_object_is_named_in_the_message():
    server = MemoryApiServer(schemas=healthcheck_schemas())
    hc = invalid_hc()
    del hc["metadata"]["name"]
    hc["metadata"]["generateName"] = "gen-"
    with pytest.raises(InvalidError) as e:
        server.create(hc)
    name = e.value.details["name"]
    assert name.startswith("gen-") and len(name) == len("gen-") + 5
    assert e.value.message.startswith(
        f'HealthCheck.activemonitor.keikoproj.io "{name}" is invalid: ')
    assert len(server) == 0 and server.resource_version() == "0"
    assert server.rejected_writes == 1


@pytest.mark.parametrize("schemas", [None, "healthcheck"], ids=["bare", "validating"])
def test_an_unknown_mode_is_refused_on_entry_whatever_the_object(run, schemas):
    """Not only when something was pruned, and not only with a schema."""
    server = MemoryApiServer(schemas=healthcheck_schemas() if schemas else None)
    made = server.create(make_hc(name="clean"))
    rv = server.resource_version()
    calls = [
        lambda: server.create(make_hc(name="other"), field_validation="bogus"),
        lambda: server.update(dict(made, spec=dict(made["spec"], repeatAfterSec=9)),
                              field_validation="strict"),
        lambda: server.update_status(dict(made, status={"successCount": 1}),
                                     field_validation=""),
        lambda: server.patch(*HC, "health", "clean", {"spec": {"repeatAfterSec": 9}},
                             field_validation="bogus"),
        lambda: server.patch(*HC, "health", "new", make_hc(name="new"), upsert=True,
                             field_validation="bogus"),
    ]
    for call in calls:
        with pytest.raises(BadRequestError) as e:
            call()
        assert "fieldValidation" in e.value.message
    assert server.resource_version() == rv and len(server) == 1
    assert server.get(*HC, "health", "clean") == made

    async def through_the_client():
        with pytest.raises(BadRequestError):
            await MemoryClient(server).create(make_hc(name="other"),
                                              field_validation="bogus")

    run(through_the_client())

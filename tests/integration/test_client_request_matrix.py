"""HttpClient's unary requests, over both transports and with each kind of
credential: what is counted, what a 401 costs, how every error status comes
back, which requests collect warnings, and the stale keep-alive retry."""
import pytest

from active_monitor_amd import API_VERSION
from active_monitor_amd.kube import MemoryApiServer
from active_monitor_amd.kube.auth import Credential, CredentialSource
from active_monitor_amd.kube.errors import ApiError
from active_monitor_amd.kube.http import HttpClient
from active_monitor_amd.kube.memory import healthcheck_schemas
from active_monitor_amd.kube.server import ApiServerFrontend
from tests.miniserver import MiniServer

from .conftest import make_hc

HC = (API_VERSION, "HealthCheck")
CM = ("v1", "ConfigMap")
TRANSPORTS = ("pool", "aiohttp")
CREDENTIALS = ("none", "token", "source")
matrix = pytest.mark.parametrize(
    "transport,credential", [(t, c) for t in TRANSPORTS for c in CREDENTIALS])


def configmap(name):
    return {"apiVersion": "v1", "kind": "ConfigMap",
            "metadata": {"name": name, "namespace": "health"}, "data": {"k": "v"}}


class Tokens(CredentialSource):
    """Hands out ``tokens[0]``, then ``tokens[1]``, ... one per refresh."""

    def __init__(self, *tokens):
        super().__init__()
        self.tokens = list(tokens)
        self.refreshes = 0

    async def _refresh(self):
        self.refreshes += 1
        return Credential(self.tokens[min(self.refreshes, len(self.tokens)) - 1])


async def start_client(url, transport, credential, tokens=("good",)):
    kwargs = {"token": tokens[0]} if credential == "token" else (
        {"credentials": Tokens(*tokens)} if credential == "source" else {})
    client = HttpClient(url, qps=0, **kwargs)
    await client.start()
    if transport == "aiohttp":
        client._pool = None  # the unary path https targets take
    client.limiter_passes = 0
    acquire = client._limiter.acquire

    async def counted():
        client.limiter_passes += 1
        await acquire()

    client._limiter.acquire = counted
    return client


class Wire:
    """A validating store behind a frontend that wants the token ``good``
    (from a client that has one), and the client under test."""

    def __init__(self, transport, credential, tokens=("good",)):
        self.store = MemoryApiServer(schemas=healthcheck_schemas())
        self.frontend = ApiServerFrontend(
            self.store, accepted_tokens=None if credential == "none" else {"good"})
        self.args = (transport, credential, tokens)

    async def __aenter__(self):
        await self.frontend.start()
        self.client = await start_client(self.frontend.url, *self.args)
        return self

    async def __aexit__(self, *exc):
        await self.client.close()
        await self.frontend.stop()


def the_four(client):
    """A GET, a POST, a PUT that names its field validation, and a PATCH, as
    ``(label, coroutine function)``; run in this order against a store that
    holds ConfigMap ``there``."""
    return [
        ("GET", lambda: client.get(*CM, "health", "there")),
        ("POST", lambda: client.create(configmap("made"))),
        ("PUT strict", lambda: client.update(configmap("there"),
                                             field_validation="Strict")),
        ("PATCH", lambda: client.patch(*CM, "health", "there", {"data": {"k": "p"}})),
    ]


@matrix
def test_requests_are_counted_once(run, transport, credential):
    async def go():
        async with Wire(transport, credential) as w:
            w.store.create(configmap("there"))
            c = w.client
            for label, call in the_four(c):
                before = c.request_count
                out = await call()
                assert out["kind"] == "ConfigMap", label
                assert c.request_count == c.limiter_passes == before + 1, label
            assert c.request_count == 4
            assert w.frontend.unauthorized_count == 0
            assert w.store.get(*CM, "health", "there")["data"] == {"k": "p"}
            if credential == "source":
                assert c._credentials.refreshes == 1

    run(go(), timeout=30)


@matrix
def test_a_401_is_final_without_a_source_and_retried_once_with_one(
        run, transport, credential):
    async def go():
        # a fixed token is stale for good; a source's next one is accepted
        tokens = ("good",) if credential == "source" else ("stale",)
        async with Wire(transport, credential, tokens) as w:
            w.frontend.accepted_tokens = {"good"}
            w.store.create(configmap("there"))
            c = w.client
            for label, call in the_four(c):
                if credential == "source":
                    c._credentials._cached = Credential("stale")
                requests, refused = c.request_count, w.frontend.unauthorized_count
                if credential == "source":
                    assert (await call())["kind"] == "ConfigMap", label
                    assert c.request_count == requests + 2, label
                    assert c.limiter_passes == c.request_count, label
                else:
                    with pytest.raises(ApiError) as exc:
                        await call()
                    assert type(exc.value).__name__ == "UnauthorizedError", label
                    assert (exc.value.code, exc.value.message) == (401, "Unauthorized")
                    assert c.request_count == requests + 1, label
                    assert c.limiter_passes == c.request_count, label
                assert w.frontend.unauthorized_count == refused + 1, label

    run(go(), timeout=30)


@pytest.mark.parametrize("transport", TRANSPORTS)
def test_a_source_whose_fresh_token_is_refused_too_gives_up_after_two(run, transport):
    async def go():
        async with Wire(transport, "source", tokens=("stale", "staler")) as w:
            w.store.create(configmap("there"))
            c = w.client
            for n, (label, call) in enumerate(the_four(c), 1):
                with pytest.raises(ApiError) as exc:
                    await call()
                assert (type(exc.value).__name__, exc.value.code,
                        exc.value.message) == ("UnauthorizedError", 401, "Unauthorized")
                assert c.request_count == c.limiter_passes == 2 * n, label
                assert w.frontend.unauthorized_count == 2 * n, label

    run(go(), timeout=30)


TYPE_ERR = ('spec.repeatAfterSec: Invalid value: "string": spec.repeatAfterSec '
            'in body must be of type integer: "string"')
CAUSES = [{"reason": "FieldValueTypeInvalid",
           "message": 'Invalid value: "string": spec.repeatAfterSec in body must be '
                      'of type integer: "string"',
           "field": "spec.repeatAfterSec"}]
NO_HC = 'healthchecks.activemonitor.keikoproj.io "absent" not found'
CONFLICT = ('Operation cannot be fulfilled on HealthCheck "there": the object has '
            "been modified; please apply your changes to the latest version and "
            "try again")
STRICT = ('HealthCheck in version "v1alpha1" cannot be handled as a HealthCheck: '
          'strict decoding error: unknown field "spec.oops"')


def invalid(name):
    return ("InvalidError", 422,
            f'HealthCheck.activemonitor.keikoproj.io "{name}" is invalid: {TYPE_ERR}',
            CAUSES, {"name": name, "group": "activemonitor.keikoproj.io",
                     "kind": "HealthCheck", "causes": CAUSES})


def error_cases(client):
    """``(label, coroutine function, (type, code, message, causes, details))``
    against a store that holds HealthCheck ``there`` at resourceVersion 1.
    Every status is provoked once by a request that stays on the pooled path
    and once by one that names its field validation or is a patch."""
    def hc(name="there", rv=None, **spec):
        obj = make_hc(name=name)
        obj["spec"].update(spec)
        if rv:
            obj["metadata"]["resourceVersion"] = rv
        return obj

    c = client
    return [
        ("404 GET", lambda: c.get(*HC, "health", "absent"),
         ("NotFoundError", 404, NO_HC, None, None)),
        ("404 PATCH", lambda: c.patch(*HC, "health", "absent", {"spec": {}}),
         ("NotFoundError", 404, NO_HC, None, None)),
        ("404 DELETE", lambda: c.delete(*HC, "health", "absent"),
         ("NotFoundError", 404, NO_HC, None, None)),
        ("409 AlreadyExists POST", lambda: c.create(hc()),
         ("AlreadyExistsError", 409, 'HealthCheck "there" already exists', None, None)),
        ("409 AlreadyExists POST Warn",
         lambda: c.create(hc(), field_validation="Warn"),
         ("AlreadyExistsError", 409, 'HealthCheck "there" already exists', None, None)),
        ("409 Conflict PUT", lambda: c.update(hc(rv="99")),
         ("ConflictError", 409, CONFLICT, None, None)),
        ("409 Conflict PUT status Ignore",
         lambda: c.update_status(hc(rv="99"), field_validation="Ignore"),
         ("ConflictError", 409, CONFLICT, None, None)),
        ("422 POST", lambda: c.create(hc("bad", repeatAfterSec="sixty")),
         invalid("bad")),
        ("422 PUT Strict",
         lambda: c.update(hc(repeatAfterSec="sixty"), field_validation="Strict"),
         invalid("there")),
        ("422 PATCH",
         lambda: c.patch(*HC, "health", "there", {"spec": {"repeatAfterSec": "sixty"}}),
         invalid("there")),
        ("400 strict PUT",
         lambda: c.update(hc(oops=1), field_validation="Strict"),
         ("BadRequestError", 400, STRICT, None, None)),
        ("400 strict PATCH",
         lambda: c.patch(*HC, "health", "there", {"spec": {"oops": 1}},
                         field_validation="Strict"),
         ("BadRequestError", 400, STRICT, None, None)),
        ("400 unknown mode POST",
         lambda: c.create(hc("other"), field_validation="Bogus"),
         ("BadRequestError", 400, 'invalid fieldValidation "Bogus": supported '
          'values: "Warn", "Strict", "Ignore"', None, None)),
        ("500 GET", lambda: c.list("v1", "Secret", "health"),
         ("ApiError", 500, "etcd is sad", None, None)),
        ("500 PATCH", lambda: c.patch("v1", "Secret", "health", "s", {}),
         ("ApiError", 500, "etcd is sad", None, None)),
    ]


@matrix
def test_every_error_status_comes_back_as_its_exception(run, transport, credential):
    async def go():
        async with Wire(transport, credential) as w:
            w.store.create(make_hc(name="there"))
            real_list, real_patch = w.store.list, w.store.patch

            def sad(real):
                def call(api_version, kind, *args, **kwargs):
                    if kind == "Secret":
                        raise ApiError("etcd is sad")
                    return real(api_version, kind, *args, **kwargs)
                return call

            w.store.list, w.store.patch = sad(real_list), sad(real_patch)
            for n, (label, call, want) in enumerate(error_cases(w.client), 1):
                with pytest.raises(ApiError) as exc:
                    await call()
                e = exc.value
                got = (type(e).__name__, e.code, e.message,
                       getattr(e, "causes", None) or None, getattr(e, "details", None))
                assert got == want, label
                assert w.client.request_count == w.client.limiter_passes == n, label
            assert w.store.get(*HC, "health", "there")["metadata"]["resourceVersion"] == "1"

    run(go(), timeout=30)


@matrix
def test_warnings_come_only_from_requests_that_look_at_headers(
        run, transport, credential):
    async def go():
        async with Wire(transport, credential) as w:
            c = w.client

            def typo(name):
                obj = make_hc(name=name)
                obj["spec"]["oops"] = name
                return obj

            made = await c.create(typo("quiet"))
            assert "oops" not in made["spec"] and list(c.warnings) == []
            made = await c.update(
                dict(made, spec=dict(made["spec"], oops=2, repeatAfterSec=7)))
            await c.update_status(dict(made, status={"typo": 1}))
            await c.get(*HC, "health", "quiet")
            assert list(c.warnings) == []

            await c.create(typo("loud"), field_validation="Warn")
            assert list(c.warnings) == ['unknown field "spec.oops"']
            await c.create(typo("ignored"), field_validation="Ignore")
            assert len(c.warnings) == 1  # asked for, and none sent
            loud = await c.get(*HC, "health", "loud")
            loud = await c.update(
                dict(loud, spec=dict(loud["spec"], oops2=2, repeatAfterSec=7)),
                field_validation="Warn")
            await c.update_status(dict(loud, status={"typo": 1}),
                                  field_validation="Warn")
            await c.patch(*HC, "health", "loud", {"spec": {"oops3": 3, "level": "x"}})
            await c.patch(*HC, "health", "loud", {"status": {"typo4": 4}},
                          subresource="status")
            assert list(c.warnings) == [
                'unknown field "spec.oops"', 'unknown field "spec.oops2"',
                'unknown field "status.typo"', 'unknown field "spec.oops3"',
                'unknown field "status.typo4"']

    run(go(), timeout=30)


@matrix
def test_an_empty_200_body_decodes_to_an_empty_object(run, transport, credential):
    async def go():
        async with MiniServer(body=b"") as srv:
            client = await start_client(
                f"http://127.0.0.1:{srv.port}", transport, credential)
            try:
                assert await client._request("GET", "/x") == {}
                assert await client.update(configmap("x")) == {}
                assert await client.update(configmap("x"), field_validation="Warn") == {}
                assert await client.patch(*CM, "health", "x", {"data": None}) == {}
                assert await client.delete(*CM, "health", "x") is None
                assert client.request_count == srv.requests == 5
            finally:
                await client.close()

    run(go(), timeout=30)


@pytest.mark.parametrize("credential", CREDENTIALS)
def test_a_closed_keep_alive_connection_costs_one_retry(run, credential):
    async def go():
        async with MiniServer(close_after=1) as srv:
            client = await start_client(
                f"http://127.0.0.1:{srv.port}", "pool", credential)
            try:
                assert await client._request("GET", "/a") == {"ok": True}
                assert (srv.connections, srv.requests) == (1, 1)
                # the pool's one connection is closed at the far end by now:
                # the request fails on it, and goes again on a fresh one
                assert await client.create(configmap("x")) == {"ok": True}
                assert (srv.connections, srv.requests) == (2, 2)
                assert client.request_count == client.limiter_passes == 2
            finally:
                await client.close()

    run(go(), timeout=30)

"""Client credential sources: static tokens, rotating token files and
client-go exec credential plugins.

What the reference inherits from ``ctrl.GetConfigOrDie()`` (cmd/main.go:70)
and client-go's transport: a bearer token that is looked up per request from
a *source* instead of being baked into the connection for the life of the
process. Three sources:

- :class:`StaticToken` — a literal token,
- :class:`TokenFileSource` — a file that something else rewrites (the
  projected service-account token, kubeconfig ``tokenFile``); re-read once a
  minute like client-go does,
- :class:`ExecPluginSource` — a ``users[].user.exec`` stanza, the
  ``client.authentication.k8s.io`` ExecCredential contract every managed
  cluster (EKS, GKE, AKS, OIDC helpers) uses.

Only token-issuing plugins are supported. A plugin that answers with
``clientCertificateData``/``clientKeyData`` alone raises
:class:`CredentialError`.
"""
from __future__ import annotations

import asyncio
import base64
import calendar
import json
import logging
import os
import re
import shutil
import time
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional

from .errors import ConfigError

log = logging.getLogger("active_monitor_amd.kube.auth")

EXEC_API_VERSIONS = (
    "client.authentication.k8s.io/v1",
    "client.authentication.k8s.io/v1beta1",
)
#: name of the cluster ``extensions`` entry handed to plugins as spec.cluster.config
EXEC_EXTENSION = "client.authentication.k8s.io/exec"
#: client-go re-reads a token file once its cached value is this old
TOKEN_FILE_PERIOD = 60.0


class CredentialError(ConfigError):
    """A credential source could not produce a credential."""


@dataclass(frozen=True)
class Credential:
    token: str
    #: epoch seconds; None = valid until invalidated
    expiry: Optional[float] = None


class CredentialSource:
    """Cached, single-flight credential lookup.

    ``get()`` answers from the cache while :meth:`_fresh` holds. Concurrent
    callers that find the cache cold share one :meth:`_refresh`.
    ``invalidate(seen)`` drops the cache only when ``seen`` is still the
    cached object, so N requests that were all refused with the same
    credential cause one refresh, not N.
    """

    def __init__(self, now: Callable[[], float] = time.time):
        self._now = now
        self._cached: Optional[Credential] = None
        self._lock: Optional[asyncio.Lock] = None
        self._lock_loop: Optional[asyncio.AbstractEventLoop] = None

    def _flight_lock(self) -> asyncio.Lock:
        # a source may outlive an event loop (config is loaded before
        # asyncio.run); a Lock may not
        loop = asyncio.get_running_loop()
        if self._lock is None or self._lock_loop is not loop:
            self._lock, self._lock_loop = asyncio.Lock(), loop
        return self._lock

    async def get(self) -> Credential:
        cred = self._cached
        if cred is not None and self._fresh(cred):
            return cred
        async with self._flight_lock():
            cred = self._cached
            if cred is not None and self._fresh(cred):
                return cred
            cred = await self._refresh()
            self._cached = cred
            return cred

    def invalidate(self, seen: Credential) -> None:
        if self._cached is seen:
            self._cached = None

    def expire(self) -> None:
        """Refresh on the next ``get()`` whatever is cached."""
        self._cached = None

    def _fresh(self, cred: Credential) -> bool:
        return cred.expiry is None or self._now() < cred.expiry

    async def _refresh(self) -> Credential:
        raise NotImplementedError


class StaticToken(CredentialSource):
    def __init__(self, token: str):
        super().__init__()
        self._static = Credential(token)
        self._cached = self._static

    async def _refresh(self) -> Credential:
        return self._static


class TokenFileSource(CredentialSource):
    """A bearer token kept in a file that is rewritten behind our back.

    The file is re-read once the cached value is ``period`` seconds old, or
    at the next ``get()`` after ``invalidate()``. A read that fails or finds
    the file empty keeps the previous token; it is an error only while there
    has never been one. ``initial`` seeds the source with a value that is
    used until the first read is due.
    """

    def __init__(self, path: str, initial: Optional[str] = None,
                 period: float = TOKEN_FILE_PERIOD,
                 now: Callable[[], float] = time.time):
        super().__init__(now)
        self.path = str(path)
        self.period = period
        self._read_at = now()
        self._last: Optional[Credential] = Credential(initial) if initial else None
        self._cached = self._last

    def _fresh(self, cred: Credential) -> bool:
        return self._now() - self._read_at < self.period

    async def _refresh(self) -> Credential:
        # a few hundred bytes from a tmpfs projection: read inline, as the
        # cost of a thread hop would dwarf it
        problem = ""
        token = ""
        try:
            with open(self.path, "r") as f:
                token = f.read().strip()
            if not token:
                problem = "file is empty"
        except OSError as e:
            problem = str(e)
        self._read_at = self._now()
        if problem:
            if self._last is None:
                raise CredentialError(f"cannot read token file {self.path}: {problem}")
            log.warning("cannot read token file %s: %s; keeping the previous token",
                        self.path, problem)
            return self._last
        if self._last is None or token != self._last.token:
            self._last = Credential(token)
        return self._last


_RFC3339 = re.compile(
    r"^(\d{4})-(\d{2})-(\d{2})[Tt ](\d{2}):(\d{2}):(\d{2})(\.\d+)?"
    r"([Zz]|[+-]\d{2}:\d{2})$"
)


def parse_rfc3339(value: str) -> float:
    """RFC 3339 timestamp → epoch seconds (``Z`` and numeric offsets)."""
    m = _RFC3339.match(value.strip()) if isinstance(value, str) else None
    if m is None:
        raise ValueError(f"not an RFC 3339 timestamp: {value!r}")
    y, mo, d, h, mi, s = (int(m.group(i)) for i in range(1, 7))
    epoch = float(calendar.timegm((y, mo, d, h, mi, s, 0, 0, 0)))
    if m.group(7):
        epoch += float(m.group(7))
    zone = m.group(8)
    if zone not in ("Z", "z"):
        sign = 1 if zone[0] == "+" else -1
        epoch -= sign * (int(zone[1:3]) * 3600 + int(zone[4:6]) * 60)
    return epoch


def _default_timeout() -> float:
    # the project's existing bound for "an external thing we wait on"
    from ..engine.parse import ARTIFACT_READ_TIMEOUT

    return ARTIFACT_READ_TIMEOUT


class ExecPluginSource(CredentialSource):
    """``users[].user.exec``: run a credential plugin, use the token it prints.

    The stanza is validated on construction (kubeconfig load time); the
    plugin runs on the first ``get()`` and again once its credential has
    expired (``now >= expiry``, client-go's rule) or was invalidated after a
    401. The plugin is a child process of the event loop with stdin at
    /dev/null and a hard timeout; it is killed and reaped when that passes.
    """

    def __init__(self, spec: Dict[str, Any], cluster: Optional[Dict[str, Any]] = None,
                 kubeconfig_dir: Optional[str] = None, timeout: Optional[float] = None,
                 now: Callable[[], float] = time.time):
        super().__init__(now)
        if not isinstance(spec, dict):
            raise ConfigError("exec credential stanza must be a mapping")
        self.command = spec.get("command") or ""
        if not isinstance(self.command, str) or not self.command:
            raise ConfigError("exec credential stanza has no command")
        self.api_version = spec.get("apiVersion") or ""
        if self.api_version not in EXEC_API_VERSIONS:
            raise ConfigError(
                f"exec plugin {self.command}: unsupported apiVersion "
                f"{self.api_version!r} (supported: {', '.join(EXEC_API_VERSIONS)})"
            )
        mode = spec.get("interactiveMode")
        if mode is None:
            if self.api_version.endswith("/v1"):
                raise ConfigError(
                    f"exec plugin {self.command}: interactiveMode must be set "
                    f"for {self.api_version}"
                )
        elif mode == "Always":
            raise ConfigError(
                f"exec plugin {self.command}: interactiveMode Always needs a "
                f"terminal, which a controller does not have"
            )
        elif mode not in ("Never", "IfAvailable"):
            raise ConfigError(
                f"exec plugin {self.command}: unknown interactiveMode {mode!r}"
            )
        self.args: List[str] = [str(a) for a in (spec.get("args") or [])]
        self.env: Dict[str, str] = {}
        for entry in spec.get("env") or []:
            if not isinstance(entry, dict) or "name" not in entry:
                raise ConfigError(
                    f"exec plugin {self.command}: env entries must be "
                    f"{{name, value}} mappings"
                )
            self.env[str(entry["name"])] = str(entry.get("value", ""))
        self.install_hint: str = spec.get("installHint") or ""
        self.provide_cluster_info = bool(spec.get("provideClusterInfo"))
        self.cluster = dict(cluster or {})
        self.kubeconfig_dir = kubeconfig_dir or os.getcwd()
        self.timeout = float(timeout) if timeout is not None else _default_timeout()
        #: completed plugin runs (observability/tests)
        self.runs = 0

    # -- request document ---------------------------------------------------

    def _exec_info(self) -> str:
        spec: Dict[str, Any] = {"interactive": False}
        if self.provide_cluster_info:
            spec["cluster"] = self._cluster_info()
        return json.dumps({
            "apiVersion": self.api_version,
            "kind": "ExecCredential",
            "spec": spec,
        })

    def _cluster_info(self) -> Dict[str, Any]:
        c = self.cluster
        info: Dict[str, Any] = {"server": c.get("server", "")}
        ca_data = c.get("certificate-authority-data")
        if not ca_data and c.get("certificate-authority"):
            # client-go hands plugins the CA bytes whichever way they were configured
            try:
                with open(c["certificate-authority"], "rb") as f:
                    ca_data = base64.b64encode(f.read()).decode()
            except OSError as e:
                log.warning("exec plugin %s: cannot read certificate-authority %s: %s",
                            self.command, c["certificate-authority"], e)
        if ca_data:
            info["certificate-authority-data"] = ca_data
        if c.get("insecure-skip-tls-verify"):
            info["insecure-skip-tls-verify"] = True
        if c.get("tls-server-name"):
            info["tls-server-name"] = c["tls-server-name"]
        for ext in c.get("extensions") or []:
            if isinstance(ext, dict) and ext.get("name") == EXEC_EXTENSION:
                info["config"] = ext.get("extension")
                break
        return info

    # -- running the plugin -------------------------------------------------

    def _not_found(self, detail: str) -> CredentialError:
        msg = f"exec plugin {self.command}: {detail}"
        if self.install_hint:
            msg += f"\n{self.install_hint}"
        return CredentialError(msg)

    def _resolve(self, env: Dict[str, str]) -> str:
        cmd = self.command
        seps = (os.sep,) + ((os.altsep,) if os.altsep else ())
        if any(s in cmd for s in seps):
            if not os.path.isabs(cmd):
                cmd = os.path.join(self.kubeconfig_dir, cmd)
            if not os.path.isfile(cmd):
                raise self._not_found(f"command not found: {cmd}")
            return cmd
        found = shutil.which(cmd, path=env.get("PATH"))
        if found is None:
            raise self._not_found("command not found on PATH")
        return found

    async def _refresh(self) -> Credential:
        env = dict(os.environ)
        env.update(self.env)
        env["KUBERNETES_EXEC_INFO"] = self._exec_info()
        program = self._resolve(env)
        try:
            proc = await asyncio.create_subprocess_exec(
                program, *self.args,
                stdin=asyncio.subprocess.DEVNULL,
                stdout=asyncio.subprocess.PIPE,
                stderr=asyncio.subprocess.PIPE,
                env=env,
            )
        except FileNotFoundError as e:
            raise self._not_found(f"command not found: {e}") from e
        except OSError as e:
            raise CredentialError(f"exec plugin {self.command}: cannot start: {e}") from e
        try:
            stdout, stderr = await asyncio.wait_for(proc.communicate(), self.timeout)
        except asyncio.TimeoutError:
            raise CredentialError(
                f"exec plugin {self.command}: timed out after {self.timeout:g}s"
            ) from None
        finally:
            # timeout or cancellation: never leave the child running or unreaped
            if proc.returncode is None:
                try:
                    proc.kill()
                except ProcessLookupError:
                    pass
                await proc.wait()
        self.runs += 1
        if proc.returncode != 0:
            tail = "\n".join(stderr.decode("utf-8", "replace").strip().splitlines()[-5:])
            raise CredentialError(
                f"exec plugin {self.command}: exited with status "
                f"{proc.returncode}" + (f": {tail}" if tail else "")
            )
        return self._parse(stdout)

    def _parse(self, stdout: bytes) -> Credential:
        try:
            doc = json.loads(stdout)
        except ValueError as e:
            raise CredentialError(
                f"exec plugin {self.command}: output is not JSON: {e}"
            ) from None
        if not isinstance(doc, dict) or doc.get("kind") != "ExecCredential":
            kind = doc.get("kind") if isinstance(doc, dict) else type(doc).__name__
            raise CredentialError(
                f"exec plugin {self.command}: expected kind ExecCredential, got {kind!r}"
            )
        if doc.get("apiVersion") != self.api_version:
            raise CredentialError(
                f"exec plugin {self.command}: answered with apiVersion "
                f"{doc.get('apiVersion')!r}, the kubeconfig asks for {self.api_version!r}"
            )
        status = doc.get("status")
        if not isinstance(status, dict):
            status = {}
        token = status.get("token")
        if not token or not isinstance(token, str):
            if status.get("clientCertificateData") and status.get("clientKeyData"):
                raise CredentialError(
                    f"exec plugin {self.command}: certificate-issuing exec plugins "
                    f"are not supported (the plugin returned clientCertificateData "
                    f"and no token)"
                )
            raise CredentialError(
                f"exec plugin {self.command}: status carries neither a token "
                f"nor certificate data"
            )
        expiry = None
        stamp = status.get("expirationTimestamp")
        if stamp:
            try:
                expiry = parse_rfc3339(stamp)
            except ValueError as e:
                raise CredentialError(f"exec plugin {self.command}: {e}") from None
        return Credential(token, expiry)

"""Cluster connection config: kubeconfig + in-cluster service account.

The role of the reference's ``ctrl.GetConfigOrDie()`` (cmd/main.go:70): find
apiserver coordinates and credentials from, in order,

1. an explicit server URL (flags),
2. the in-cluster service-account mount
   (``/var/run/secrets/kubernetes.io/serviceaccount``),
3. ``$KUBECONFIG`` / ``~/.kube/config`` (current-context; bearer token,
   ``tokenFile``, ``exec`` credential plugin or client-certificate auth,
   cluster CA, insecure-skip-tls-verify).

Credentials that can change while the process runs (the projected
service-account token, ``tokenFile``, ``exec``) travel as a
``CredentialSource`` (kube/auth.py) that the client consults per request.
Not supported: exec plugins that issue client certificates, and the legacy
``auth-provider`` stanza (a warning says to migrate to ``exec``).
"""
from __future__ import annotations

import base64
import logging
import os
import tempfile
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import yaml

from .auth import CredentialSource, ExecPluginSource, TokenFileSource
from .errors import ConfigError  # noqa: F401  (public here)

log = logging.getLogger("active_monitor_amd.kube.config")

SA_DIR = Path("/var/run/secrets/kubernetes.io/serviceaccount")


@dataclass
class ClusterConfig:
    server: str
    token: Optional[str] = None
    ca_cert_path: Optional[str] = None
    client_cert_path: Optional[str] = None
    client_key_path: Optional[str] = None
    verify: bool = True
    #: where ``token`` came from, when a file that is rewritten in place
    token_file: Optional[str] = None
    #: rotating credentials; None = ``token`` (or nothing) for good
    credential_source: Optional[CredentialSource] = None

    def make_client(self):
        from .http import HttpClient

        client = HttpClient(
            self.server,
            token=self.token,
            verify=self.verify,
            ca_cert=self.ca_cert_path,
            credentials=self.credential_source,
        )
        client.client_cert = (self.client_cert_path, self.client_key_path)
        return client


def in_cluster_config() -> Optional[ClusterConfig]:
    host = os.environ.get("KUBERNETES_SERVICE_HOST")
    token_file = SA_DIR / "token"
    if not host or not token_file.exists():
        return None
    port = os.environ.get("KUBERNETES_SERVICE_PORT", "443")
    ca = SA_DIR / "ca.crt"
    token = token_file.read_text().strip()
    return ClusterConfig(
        server=f"https://{host}:{port}",
        token=token,
        ca_cert_path=str(ca) if ca.exists() else None,
        token_file=str(token_file),
        # bound service-account tokens rotate; the kubelet rewrites the file
        credential_source=TokenFileSource(str(token_file), initial=token or None),
    )


def _materialize(data_b64: Optional[str], path: Optional[str], suffix: str) -> Optional[str]:
    """kubeconfig allows inline base64 ``*-data`` or file paths."""
    if path:
        return path
    if not data_b64:
        return None
    f = tempfile.NamedTemporaryFile(
        mode="wb", suffix=suffix, prefix="amkube-", delete=False
    )
    f.write(base64.b64decode(data_b64))
    f.close()
    return f.name


def _file_source(path: str, stopgap: Optional[str]) -> TokenFileSource:
    """Token file configured by hand (kubeconfig ``tokenFile``, --token-file):
    the file is the credential, so the first ``get()`` reads it; a literal
    token given next to it only serves while the file cannot be read."""
    source = TokenFileSource(path, initial=stopgap)
    source.expire()
    return source


def load_kubeconfig(path: Optional[str] = None, context: Optional[str] = None) -> ClusterConfig:
    cfg_path = path or os.environ.get("KUBECONFIG") or os.path.expanduser("~/.kube/config")
    try:
        doc = yaml.safe_load(Path(cfg_path).read_text())
    except OSError as e:
        raise ConfigError(f"cannot read kubeconfig {cfg_path}: {e}") from e
    if not isinstance(doc, dict):
        raise ConfigError(f"invalid kubeconfig {cfg_path}")

    ctx_name = context or doc.get("current-context")
    contexts = {c.get("name"): c.get("context", {}) for c in doc.get("contexts", []) or []}
    if ctx_name not in contexts:
        raise ConfigError(f"context {ctx_name!r} not found in {cfg_path}")
    ctx = contexts[ctx_name]

    clusters = {c.get("name"): c.get("cluster", {}) for c in doc.get("clusters", []) or []}
    users = {u.get("name"): u.get("user", {}) for u in doc.get("users", []) or []}
    cluster = clusters.get(ctx.get("cluster"))
    if cluster is None:
        raise ConfigError(f"cluster {ctx.get('cluster')!r} not found in {cfg_path}")
    user = users.get(ctx.get("user"), {})

    server = cluster.get("server", "")
    if not server:
        raise ConfigError(f"cluster {ctx.get('cluster')!r} has no server")

    # credential precedence (client-go): tokenFile, then token, then exec
    token = user.get("token")
    token_file = user.get("tokenFile")
    source: Optional[CredentialSource] = None
    cfg_dir = os.path.dirname(os.path.abspath(cfg_path))
    if token_file:
        if not os.path.isabs(token_file):
            token_file = os.path.join(cfg_dir, token_file)
        # a literal token next to tokenFile only bridges the time to the
        # first successful read, so the first get() goes to the file
        source = _file_source(token_file, token or None)
    elif not token and user.get("exec"):
        source = ExecPluginSource(user["exec"], cluster=cluster, kubeconfig_dir=cfg_dir)
    if user.get("auth-provider"):
        log.warning(
            "kubeconfig user %r uses the legacy auth-provider stanza (%s), which "
            "is not supported and is ignored; migrate to an exec credential plugin",
            ctx.get("user"), (user["auth-provider"] or {}).get("name", "unnamed"),
        )

    return ClusterConfig(
        server=server,
        token=token,
        token_file=token_file,
        credential_source=source,
        ca_cert_path=_materialize(
            cluster.get("certificate-authority-data"),
            cluster.get("certificate-authority"),
            ".crt",
        ),
        client_cert_path=_materialize(
            user.get("client-certificate-data"), user.get("client-certificate"), ".crt"
        ),
        client_key_path=_materialize(
            user.get("client-key-data"), user.get("client-key"), ".key"
        ),
        verify=not cluster.get("insecure-skip-tls-verify", False),
    )


def get_config(server: str = "", token: str = "", insecure: bool = False,
               kubeconfig: Optional[str] = None,
               token_file: Optional[str] = None) -> ClusterConfig:
    """GetConfigOrDie-style resolution (explicit > in-cluster > kubeconfig).

    ``token_file`` goes with an explicit ``server``: the bearer token is read
    from that file and re-read as it rotates; ``token``, if also given, is
    used until the first successful read."""
    if server:
        if token_file:
            return ClusterConfig(
                server=server, token=token or None, verify=not insecure,
                token_file=token_file,
                credential_source=_file_source(token_file, token or None),
            )
        return ClusterConfig(server=server, token=token or None, verify=not insecure)
    in_cluster = in_cluster_config()
    if in_cluster is not None:
        return in_cluster
    return load_kubeconfig(kubeconfig)

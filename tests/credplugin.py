"""A fake client-go exec credential plugin for the credential tests.

``write_plugin`` drops a small Python script into a directory. Every run of
the script appends a line to a counter file and prints an ExecCredential
whose token is ``tok-<run number>``; its kubeconfig ``env`` entries steer it
into the other behaviours the tests need (see PLUGIN_SOURCE).
"""
import base64
import os
import stat
import sys

import yaml

PLUGIN_SOURCE = '''\
#!{python}
import json, os, sys, time

env = os.environ
with open(env["FAKE_COUNTER"], "a") as f:
    f.write("run\\n")
with open(env["FAKE_COUNTER"]) as f:
    n = len(f.readlines())
if env.get("FAKE_PIDFILE"):
    with open(env["FAKE_PIDFILE"], "w") as f:
        f.write(str(os.getpid()))
info = json.loads(env.get("KUBERNETES_EXEC_INFO") or "{{}}")
if env.get("FAKE_DUMP"):
    with open(env["FAKE_DUMP"], "w") as f:
        json.dump({{"argv": sys.argv[1:], "env": dict(env), "exec_info": info,
                   "stdin": sys.stdin.read()}}, f)
if env.get("FAKE_SLEEP"):
    time.sleep(float(env["FAKE_SLEEP"]))
if env.get("FAKE_FAIL"):
    sys.stderr.write(env.get("FAKE_STDERR", "") + "\\n")
    sys.exit(int(env["FAKE_FAIL"]))
mode = env.get("FAKE_OUTPUT", "")
if mode == "notjson":
    print("Welcome! please log in at https://example.invalid/")
    sys.exit(0)
doc = {{
    "apiVersion": info.get("apiVersion"),
    "kind": "ExecCredential",
    "status": {{"token": env.get("FAKE_TOKEN") or "tok-%d" % n}},
}}
if env.get("FAKE_EXPIRY"):
    doc["status"]["expirationTimestamp"] = env["FAKE_EXPIRY"]
if mode == "wrongkind":
    doc["kind"] = "TokenReview"
elif mode == "wrongversion":
    doc["apiVersion"] = "client.authentication.k8s.io/v1alpha1"
elif mode == "empty":
    doc["status"] = {{}}
elif mode == "certonly":
    doc["status"] = {{"clientCertificateData": "CERT", "clientKeyData": "KEY"}}
print(json.dumps(doc))
'''


def write_plugin(directory, name="fake-plugin"):
    """Write the plugin into ``directory``; return its path."""
    path = os.path.join(str(directory), name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(PLUGIN_SOURCE.format(python=sys.executable))
    os.chmod(path, stat.S_IRWXU | stat.S_IRGRP | stat.S_IXGRP | stat.S_IROTH | stat.S_IXOTH)
    return path


def runs(counter) -> int:
    """How many times the plugin has run."""
    try:
        with open(str(counter)) as f:
            return len(f.readlines())
    except FileNotFoundError:
        return 0


def exec_stanza(command, counter, api_version="client.authentication.k8s.io/v1",
                interactive_mode="Never", args=None, env=None, **extra):
    stanza = {"apiVersion": api_version, "command": str(command)}
    if interactive_mode is not None:
        stanza["interactiveMode"] = interactive_mode
    if args:
        stanza["args"] = list(args)
    entries = {"FAKE_COUNTER": str(counter)}
    entries.update(env or {})
    stanza["env"] = [{"name": k, "value": str(v)} for k, v in entries.items()]
    stanza.update(extra)
    return stanza


def write_kubeconfig(directory, user, server="https://api.example:6443",
                     cluster_extra=None, name="config"):
    cluster = {
        "server": server,
        "certificate-authority-data": base64.b64encode(b"CA PEM").decode(),
    }
    cluster.update(cluster_extra or {})
    doc = {
        "apiVersion": "v1",
        "kind": "Config",
        "current-context": "dev",
        "contexts": [{"name": "dev", "context": {"cluster": "c1", "user": "u1"}}],
        "clusters": [{"name": "c1", "cluster": cluster}],
        "users": [{"name": "u1", "user": user}],
    }
    path = os.path.join(str(directory), name)
    with open(path, "w") as f:
        f.write(yaml.safe_dump(doc))
    return path


class Clock:
    """Injectable ``now``."""

    def __init__(self, t=1_700_000_000.0):
        self.t = t

    def __call__(self):
        return self.t

    def advance(self, dt):
        self.t += dt

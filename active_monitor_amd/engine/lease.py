"""One coordination.k8s.io/v1 Lease as seen by one identity.

Leader election (engine/leader.py) and shard ownership (engine/shards.py)
both decide who drives what by the same few operations on a Lease: read it,
test whether its holder's window has run out, write it under the
resourceVersion that was read, and give it up. They live here once; the
policies that differ (who may take a lease, and when) stay with the callers.
"""
from __future__ import annotations

import time
from typing import Optional

from ..api.types import k8s_now, parse_k8s_time
from ..kube.client import KubeClient
from ..kube.errors import AlreadyExistsError, ConflictError, NotFoundError

LEASE_API_VERSION = "coordination.k8s.io/v1"

# what release() does to renewTime — the choice carries meaning:
KEEP = "keep"    # leave it: the lease reads as it did, minus its holder
DROP = "drop"    # remove it: free this instant, no window for anyone
STAMP = "stamp"  # set it to now: opens the preferredHolder's priority window


class Lease:
    def __init__(self, client: KubeClient, namespace: str, name: str,
                 identity: str, duration: float, expiry_pad: float = 0.0):
        self.client = client
        self.namespace = namespace
        self.name = name
        self.identity = identity
        self.duration = duration
        # renewTime has whole-second resolution; a caller that must never see
        # a freshly renewed lease as expired pads the window by that second
        self.expiry_pad = expiry_pad

    def _held_spec(self) -> dict:
        return {
            "holderIdentity": self.identity,
            "leaseDurationSeconds": int(self.duration),
            "renewTime": k8s_now(),
        }

    async def read(self) -> Optional[dict]:
        """The Lease object, or None when there is none."""
        try:
            return await self.client.get(
                LEASE_API_VERSION, "Lease", self.namespace, self.name)
        except NotFoundError:
            return None

    def expired(self, spec: dict) -> bool:
        """True once ``renewTime`` is older than the window (or missing)."""
        renew = parse_k8s_time(spec.get("renewTime"))
        return renew is None or (
            time.time() - renew.timestamp()) > self.duration + self.expiry_pad

    async def create(self) -> bool:
        """Create the lease held by this identity; False if someone was first."""
        try:
            await self.client.create({
                "apiVersion": LEASE_API_VERSION,
                "kind": "Lease",
                "metadata": {"name": self.name, "namespace": self.namespace},
                "spec": self._held_spec(),
            })
            return True
        except AlreadyExistsError:
            return False

    async def write(self, lease: dict) -> bool:
        """Update under the resourceVersion that was read; False when the
        lease changed or vanished in between (someone else acted first)."""
        try:
            await self.client.update(lease)
            return True
        except (ConflictError, NotFoundError):
            return False

    async def take(self, lease: dict, **extra) -> bool:
        """Replace the spec of a lease just read with a fresh one held by
        this identity (plus ``extra`` fields) and write it."""
        lease["spec"] = {**self._held_spec(), **extra}
        return await self.write(lease)

    async def release(self, renew_time: str, lease: Optional[dict] = None) -> None:
        """Blank the holder if it is this identity, treating ``renewTime`` as
        ``renew_time`` says (KEEP, DROP or STAMP). ``lease`` is the object if
        the caller has just read it."""
        if lease is None:
            lease = await self.read()
        spec = (lease or {}).get("spec") or {}
        if spec.get("holderIdentity") != self.identity:
            return
        spec["holderIdentity"] = ""
        if renew_time == DROP:
            spec.pop("renewTime", None)
        elif renew_time == STAMP:
            spec["renewTime"] = k8s_now()
        await self.write(lease)

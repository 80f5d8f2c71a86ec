"""Lease-based leader election (cmd/main.go:87-88 equivalent).

A single active replica holds a coordination.k8s.io/v1 Lease named with the
reference's LeaderElectionID ``689451f8.keikoproj.io``; others block in
``acquire()`` until the holder's lease expires.
"""
from __future__ import annotations

import asyncio
import logging
import os

from ..kube.client import KubeClient
from .lease import KEEP, Lease

log = logging.getLogger("active_monitor_amd.leader")


class LeaderElector:
    def __init__(
        self,
        client: KubeClient,
        name: str,
        namespace: str,
        identity: str,
        lease_duration: float = 15.0,
        renew_interval: float = 5.0,
        retry_interval: float = 2.0,
    ):
        # ops/test override for failover latency (mirrors controller-runtime's
        # LeaseDuration/RenewDeadline tunables the reference inherits)
        env_lease = os.environ.get("AM_LEADER_LEASE_SECS")
        env_renew = os.environ.get("AM_LEADER_RENEW_SECS")
        if env_lease:
            lease_duration = float(env_lease)
        if env_renew:
            renew_interval = float(env_renew)
            retry_interval = min(retry_interval, renew_interval)
        self.client = client
        self.name = name
        self.namespace = namespace
        self.identity = identity
        self.lease_duration = lease_duration
        self.renew_interval = renew_interval
        self.retry_interval = retry_interval
        self.is_leader = False

    def _lease(self) -> Lease:
        # built per action, not in __init__: lease_duration may be set on the
        # elector after construction and must be the one in force
        return Lease(self.client, self.namespace, self.name, self.identity,
                     self.lease_duration)

    async def try_acquire(self) -> bool:
        handle = self._lease()
        lease = await handle.read()
        if lease is None:
            ok = await handle.create()
        else:
            spec = lease.get("spec") or {}
            holder = spec.get("holderIdentity")
            expired = handle.expired(spec)  # exactly lease_duration, no pad
            if holder and holder != self.identity and not expired:
                return False
            ok = await handle.take(lease)
        if ok:
            self.is_leader = True
        return ok

    async def acquire(self) -> None:
        while not await self.try_acquire():
            await asyncio.sleep(self.retry_interval)
        log.info("acquired leadership as %s", self.identity)

    async def renew_loop(self) -> None:
        while True:
            await asyncio.sleep(self.renew_interval)
            if not await self.try_acquire():
                # lost the lease — in the reference losing leadership is fatal
                # for the replica; raise so the manager's task group surfaces it
                self.is_leader = False
                raise RuntimeError(f"lost leadership lease {self.name}")

    async def release(self) -> None:
        if not self.is_leader:
            return
        try:
            await self._lease().release(KEEP)
        except Exception:
            pass
        self.is_leader = False

"""The shared templates an engine resolves against, kept by a watch per kind.

:class:`TemplateCache` holds every WorkflowTemplate (of one namespace, or of
all) and ClusterWorkflowTemplate the apiserver has. Objects are replaced,
never changed in place, so a run keeps what it resolved against.
"""
from __future__ import annotations

import asyncio
from typing import Any, Dict, List, Optional, Tuple

from ..kube.errors import NotFoundError
from ..kube.registry import WF_API_VERSION
from .templates import CWFT_KIND, WFT_KIND, Lookup, Resolved, resolve


class TemplateCache:
    def __init__(self, client: Any, namespace: Optional[str] = None):
        self.client = client
        self.namespace = namespace
        # (cluster scope, namespace or "", name) → object
        self._objects: Dict[Tuple[bool, str, str], Dict[str, Any]] = {}
        self._subs: List[Any] = []
        self._tasks: List["asyncio.Future[Any]"] = []
        #: direct reads made for a name the cache did not have
        self.reads = 0

    async def start(self) -> None:
        """Returns with the cache whole. Watch first, then list, so that
        nothing created in between is missed."""
        for kind, namespace in ((WFT_KIND, self.namespace), (CWFT_KIND, None)):
            sub = self.client.watch(WF_API_VERSION, kind, namespace)
            self._subs.append(sub)
            for obj in await self.client.list(WF_API_VERSION, kind, namespace):
                self._keep(obj)
            self._tasks.append(asyncio.ensure_future(self._follow(sub)))

    async def stop(self) -> None:
        for sub in self._subs:
            sub.close()
        for task in self._tasks:
            task.cancel()
        await asyncio.gather(*self._tasks, return_exceptions=True)
        self._subs, self._tasks = [], []

    @staticmethod
    def _key(obj: Dict[str, Any]) -> Tuple[bool, str, str]:
        meta = obj.get("metadata") or {}
        cluster = obj.get("kind") == CWFT_KIND
        return cluster, "" if cluster else meta.get("namespace", ""), meta.get("name", "")

    def _keep(self, obj: Dict[str, Any]) -> None:
        """Keep ``obj`` unless what is cached is newer (a direct read and
        the watch may deliver the same object in either order)."""
        key = self._key(obj)
        have = self._objects.get(key)
        if have is not None:
            try:
                if (int(have["metadata"]["resourceVersion"])
                        > int(obj["metadata"]["resourceVersion"])):
                    return
            except (KeyError, TypeError, ValueError):
                pass  # opaque resourceVersion: the later arrival stands
        self._objects[key] = obj

    async def _follow(self, sub: Any) -> None:
        async for ev in sub:
            if ev["type"] == "DELETED":
                self._objects.pop(self._key(ev["object"]), None)
            elif ev["type"] in ("ADDED", "MODIFIED"):
                self._keep(ev["object"])

    def names(self) -> List[str]:
        """What the cache holds, sorted: ``namespaced/NAMESPACE/NAME`` and
        ``cluster/NAME``."""
        return sorted(f"cluster/{name}" if cluster else f"namespaced/{ns}/{name}"
                      for cluster, ns, name in self._objects)

    def get(self, name: str, namespace: str = "",
            cluster: bool = False) -> Optional[Dict[str, Any]]:
        """The cached object of that name, None when there is none; read-only."""
        return self._objects.get((cluster, "" if cluster else namespace, name))

    def lookup(self, namespace: str) -> Lookup:
        """For a Workflow of ``namespace``: namespaced names are looked up
        there."""
        return lambda cluster, name: self.get(name, namespace, cluster)

    async def read_missing(self, spec: Dict[str, Any], namespace: str,
                           found: Resolved) -> Resolved:
        """Each name that ``found``, ``spec`` resolved for a Workflow of
        ``namespace``, lists as missing is read once from the apiserver; then
        ``spec`` is resolved anew, until that names nothing not yet asked
        for. Returns the last resolution."""
        asked: set = set()
        while True:
            wanted = [m for m in found.missing if m not in asked]
            if not wanted:
                return found
            for cluster, name in wanted:
                asked.add((cluster, name))
                self.reads += 1
                try:
                    self._keep(await self.client.get(
                        WF_API_VERSION, CWFT_KIND if cluster else WFT_KIND,
                        "" if cluster else namespace, name))
                except NotFoundError:
                    pass
            found = resolve(spec, self.lookup(namespace))

"""The HealthCheck CRD schema against the project's own documents: every
shipped example and sample admits untouched, the committed CRD manifest
compiles, and so do the objects the benchmark builds."""
import copy
import glob
import os
import sys

import pytest
import yaml

from active_monitor_amd import API_VERSION
from active_monitor_amd.kube.memory import healthcheck_schemas
from active_monitor_amd.kube.schema import compile_schema

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CRD_FILE = os.path.join(
    REPO, "config", "crd", "bases", "activemonitor.keikoproj.io_healthchecks.yaml")


def _healthcheck_documents():
    files = sorted(
        glob.glob(os.path.join(REPO, "examples", "**", "*.y*ml"), recursive=True)
        + glob.glob(os.path.join(REPO, "config", "samples", "*.y*ml"))
    )
    found = []
    for path in files:
        with open(path) as f:
            for i, doc in enumerate(yaml.safe_load_all(f)):
                if isinstance(doc, dict) and doc.get("kind") == "HealthCheck":
                    found.append(pytest.param(
                        doc, id=f"{os.path.relpath(path, REPO)}[{i}]"))
    return found


DOCUMENTS = _healthcheck_documents()


@pytest.fixture(scope="module")
def validator():
    return healthcheck_schemas()[(API_VERSION, "HealthCheck")]


def test_the_examples_were_found():
    assert len(DOCUMENTS) >= 20


@pytest.mark.parametrize("doc", DOCUMENTS)
def test_shipped_healthcheck_admits_untouched(validator, doc):
    obj = copy.deepcopy(doc)
    pruned, errs = validator.admit(obj)
    assert errs == []
    assert pruned == []
    assert obj == doc


def test_committed_crd_manifest_compiles_and_is_the_generated_schema():
    with open(CRD_FILE) as f:
        crd = yaml.safe_load(f)
    versions = crd["spec"]["versions"]
    assert [v["name"] for v in versions] == ["v1alpha1"]
    schema = versions[0]["schema"]["openAPIV3Schema"]
    committed = compile_schema(schema)
    from active_monitor_amd.api.crd import healthcheck_crd

    assert schema == healthcheck_crd()["spec"]["versions"][0]["schema"]["openAPIV3Schema"]
    bad = {"spec": {"repeatAfterSec": "sixty", "workflow": {}}}
    _, errs = committed.admit(bad)
    assert [e.field for e in errs] == ["spec.repeatAfterSec"]


@pytest.mark.parametrize("i", [0, 25, 60])  # remedy, cron, interval
def test_bench_objects_admit_untouched(validator, i):
    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)
    cr, is_remedy = bench.make_cr(i, "health", 0.3, 0.2)
    assert is_remedy == (i == 0)
    assert ("schedule" in cr["spec"]) == (i == 25)
    before = copy.deepcopy(cr)
    assert validator.admit(cr) == ([], [])
    assert cr == before

"""GPU-box validation of the native wire codec.

Like the other test_gpu_host files this validates the host, not a kernel:
on the benchmark host the wire path must run on the C codec (no silent
Python fallback), and a short bench run over it must produce the contract
line. Nothing here touches the device beyond what bench.py itself does.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_native_wire_codec_loaded_on_gpu_host():
    out = subprocess.run(
        [sys.executable, "-c",
         "from active_monitor_amd.utils import wirecodec as w;"
         "print(w.NATIVE, w.dumpb({'a': [1]}), w.loads_strict(b'{\"a\": [1]}'))"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
        env=dict(os.environ, AM_REQUIRE_NATIVE="1"),
    )
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip() == "True b'{\"a\":[1]}' {'a': [1]}"


def test_short_bench_over_the_native_codec():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--crs", "50", "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
        env=dict(os.environ, AM_REQUIRE_NATIVE="1"),
    )
    assert out.returncode == 0, out.stderr[-2000:]
    data = json.loads(out.stdout.strip().splitlines()[-1])
    assert data["metric"] == "sustained_healthcheck_cycles_per_sec"
    assert data["value"] > 0

"""GPU-box validation of the durable standalone mode.

Like the other test_gpu_host files this validates the host, not a kernel:
the data directory relies on ``flock``, ``fsync`` and atomic rename on the
benchmark host's filesystem, and on SIGTERM reaching a child process. It is
the standalone restart round trip — create a HealthCheck over HTTP, SIGTERM
the apiserver process, start it again on the same directory, read the same
object back. Nothing here touches the device.
"""
import pytest

from .test_durable_cli import restart_round_trip

pytestmark = pytest.mark.gpu


def test_standalone_restart_round_trip_on_gpu_host(run, tmp_path):
    run(restart_round_trip(str(tmp_path / "data")), timeout=120)

import os
import sys

# Before anything imports torch: MKL (torch's CPU log / exp / tanh and GEMMs) picks its code branch by CPU vendor and ISA,
# and the branches round differently, so the bit-exact pins against tests/golden/ (recorded with this setting by
# tests/golden/make_golden.py) would hold on one host and not another.  COMPATIBLE is the branch MKL keeps identical
# on every x86 processor.
os.environ["MKL_CBWR"] = "COMPATIBLE"

import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP device); run with -m gpu on the GPU box")


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="session")
def hip_lib():
    """Build (if needed) and load the C-ABI library."""
    from snn_for_object_detection_amd import _build, _hip
    _build.build()
    return _hip.load()

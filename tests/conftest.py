import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: builds the 1.03 G-parameter headline model on the CPU (~10 s, 4 GB)")


@pytest.fixture(scope="session", autouse=True)
def _built_library():
    """The .so is built in-tree; (re)build when sources are newer (hipcc cross-compiles without a GPU)."""
    from shasta_amd import build
    try:
        build.build(verbose=False)
    except Exception as e:  # noqa: BLE001
        if not os.path.exists(build.LIB):
            raise
        print("warning: rebuild failed, using existing library:", e)
    yield

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def reference():
    """The compiled reference's answers as recorded under tests/golden/refcalls (tests/refcalls.py).
    NEM_REFERENCE_RECORD=1 calls the compiled reference instead and records what it returns
    (tests/golden/make_refcalls.py)."""
    from tests.refcalls import RecordedReference
    if os.environ.get("NEM_REFERENCE_RECORD") == "1":
        from oracle import pyoracle
        return RecordedReference(live=pyoracle.Reference())
    return RecordedReference()


@pytest.fixture(scope="session")
def gpu_lib():
    from pangenomenem_amd import build, engine
    build.build()
    lib = engine.load_library()
    if engine.device_count() <= 0:
        pytest.fail("no HIP device visible: the gpu tests must run on the GPU box")
    return lib

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle_port():
    """Our C restatement of cmatrices.c (test infrastructure)."""
    from oracle import binding
    if not os.path.exists(binding.PORT_SO):
        binding.build()
    return binding.port()


@pytest.fixture(scope="session")
def oracle_ref():
    """The reference's own cmatrices.c compiled unmodified, as recorded under tests/golden/ (tests/helpers.py:
    reference_oracle): every call the tests make of it, answered by oracle/_ref/libcmatrices_ref.so."""
    from helpers import reference_oracle
    return reference_oracle("cmatrices")


@pytest.fixture(scope="session")
def checker(oracle_port):
    """The CPU checker the GPU parity tests compare against: the reference's OWN cmatrices.c (oracle/_ref, built in the
    dev container and shipped to the GPU box with the repo snapshot) when present, else our C restatement (which
    tests/test_oracle.py pins bit-for-bit to the reference)."""
    from oracle import binding
    return binding.ref() if binding.have_ref() else oracle_port

#!/usr/bin/env python
"""Records tests/golden/reference_cmatrices_calls.npz and reference_module_calls.npz: what the reference's own compiled
code -- cmatrices.c (oracle/_ref/libcmatrices_ref.so, through oracle.binding) and its CPython module _cmatrices
(oracle/_ref/_cmatrices.so) -- answers to every call the CPU tests make of it (tests/helpers.py: reference_oracle).

Run where the reference checkout exists (oracle/Makefile compiles it from $REFERENCE): it runs the CPU tests that use
those oracles with PRAD_RECORD_REFERENCE=1, so that the live code answers them and the recordings are rewritten.
The GPU tier of tests/test_reference_wrapper.py makes the same calls as its CPU tier.

Nothing here is reference SOURCE; the recordings are its outputs."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

if __name__ == "__main__":
    env = dict(os.environ, PRAD_RECORD_REFERENCE="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-m", "not gpu",
           os.path.join("tests", "test_oracle.py"), os.path.join("tests", "test_reference_wrapper.py")]
    sys.exit(subprocess.run(cmd, cwd=ROOT, env=env).returncode)

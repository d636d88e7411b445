"""The staging of libfdcn's host-array entry points under sanitizers, on the CPU.

`make host_call` (Makefile) builds tools/sanitize/host_call_driver.cpp with
AddressSanitizer (leak check on) + UndefinedBehaviorSanitizer (first report
aborts) and runs it: csrc/fdcn_host_call.h over a malloc / memcpy backend
that fails the n-th of its calls.  Those failure paths -- a refused
allocation, a failed copy, a launch that returns an error -- cannot be
provoked on a GPU, so this is the test of "the block is freed exactly once,
the stream is synchronised before return, the first message is the caller's",
and of the scoped workspace of the `_dev` entry points."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "build", "asan", "host_call_driver")

pytestmark = pytest.mark.skipif(
    not os.path.exists(os.path.join(ROOT, "Makefile")) or shutil.which("make") is None
    or shutil.which(os.environ.get("CXX", "g++")) is None,
    reason="needs the Makefile, make and a C++ compiler")


@pytest.fixture(scope="module")
def run():
    return subprocess.run(["make", "-s", "host_call"], cwd=ROOT, capture_output=True, text=True,
                          timeout=600)


def test_make_host_call_driver_clean(run):
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert "host_call_driver: ok" in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr
    assert "runtime error" not in run.stderr  # UBSan


def test_host_call_driver_is_instrumented(run):
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    p = subprocess.run(["nm", DRIVER], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "__asan_report" in p.stdout and "__ubsan_handle" in p.stdout

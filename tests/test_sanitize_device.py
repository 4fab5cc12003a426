"""Sanitizer job for the device-callback objective (LBFGS_OBJ_DEVICE) and the device-buffer entry
points, CPU only.

tests/sanitize_device/_build/san_devobj: lbfgs_driver.c, the unmodified host test double of the
device layer (tests/sanitize/host_device_double.c) and a stand-alone main, built with
-fsanitize=address,undefined -fno-sanitize-recover=all. Under the double "device" memory is host
memory: the callback is plain code on the pointers it is given, and the caller's x0 / x buffers are
heap blocks of exactly n doubles, so one element read or written past either end is an ASan report.
All four searches at n in {1, 3, 513} with eager_grad off and on, a callback failing at its k-th
call, every refusal, and the device-buffer forms for the other objectives, every trajectory bit
for bit the oracle's. The link itself shows that the driver calls no lbk_* function the double does
not have. The binary runs on its own (no preloaded runtime).
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = os.path.join(HERE, "sanitize_device")


def _gcc_lib(name):
    try:
        p = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True, timeout=30).stdout.strip()
    except (OSError, subprocess.SubprocessError):
        return None
    return p if p and os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def built():
    if shutil.which("gcc") is None or shutil.which("make") is None or _gcc_lib("libasan.so") is None:
        pytest.skip("no gcc / make / ASan runtime here")
    p = subprocess.run(["make", "-C", SAN, "-j4"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return SAN


def test_device_objective_under_asan_ubsan(built):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(built, "_build", "san_devobj")], capture_output=True, text=True, timeout=600,
                       env=env)
    tail = p.stdout[-1500:] + p.stderr[-3000:]
    assert p.returncode == 0, tail
    assert "device-objective sanitizer job: all checks passed" in p.stdout, tail
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, tail

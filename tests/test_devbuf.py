"""The growable device buffer (grom_amd/csrc/devbuf.h) on the host (CPU only).

tools/devbuf_check.cpp includes devbuf.h over stand-ins for the device
allocator (malloc underneath, every call recorded) and checks the sizes each
module's buffers ask for -- the formulas written out, per module -- regrowth,
the phase arena (a piece of it, the overflow when it is full, the three cases
of a new phase), moves, and that every block is freed exactly once.  Built
with AddressSanitizer + UBSan (the Makefile's sanitize rules) and run as a
plain executable; any sanitizer report fails the test.
"""
import os
import shutil
import subprocess

import pytest

from _util import REPO


def test_devbuf_under_sanitizer():
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = os.path.join("build", "san-asan", "devbuf_check")
    r = subprocess.run(["make", "-s", exe, "SAN=asan"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ)
    env.setdefault("ASAN_OPTIONS", "abort_on_error=0:detect_leaks=1")
    r = subprocess.run([os.path.join(REPO, exe)], cwd=REPO, env=env, capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]
    assert r.returncode == 0, out[-6000:]
    assert "devbuf_check: ok" in out, out[-6000:]

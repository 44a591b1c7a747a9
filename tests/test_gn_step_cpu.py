"""The Gauss-Newton step that the single and the batched alignment loops share, without a device:
gn_step called directly on a well-conditioned and on a singular system and held field by field
against what align_loop and refine_loop make of the same systems (tests/cpp/test_gn_step.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gn_step_under_the_sanitizers():
    """Stand-alone, with ASan and UBSan linked into the program."""
    path = os.path.join(ROOT, "tests", "cpp", "test_gn_step")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f gn_step.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "gn step ok" in r.stdout, r.stdout + r.stderr[-3000:]

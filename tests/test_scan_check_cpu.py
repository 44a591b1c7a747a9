"""The scan-and-pose checks the dense map's calls share (form_amd/csrc/probe_host.hpp,
scan_check), CPU only: fmx_dense_integrate's and fmx_carve_rays' texts for too many points, the
order of the complaints, and the probes' text through probe_check (tests/cpp/test_scan_check.cpp,
built by __graft_entry__.build())."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_check_under_the_sanitizers():
    """tests/cpp/test_scan_check (tests/cpp/scan_check.mk), with ASan and UBSan linked into the
    stand-alone program."""
    path = os.path.join(ROOT, "tests", "cpp", "test_scan_check")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f scan_check.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "scan check ok" in r.stdout, r.stdout + r.stderr[-3000:]

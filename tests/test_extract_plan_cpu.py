"""The extraction's host-side kernel choice (form_amd/csrc/extract_plan.hpp), CPU only:
tests/cpp/test_extract_plan.cpp (built by __graft_entry__.build(), tests/cpp/extract_plan.mk) pins the plans of the
project's geometries and of the case table and sweeps every accepted shape for the sort
capacity and the LDS grants; here it runs, and the Python case table
(tests/extract_cases.py) is compared with the same function row by row."""
import os
import subprocess

import pytest

import extract_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "test_extract_plan")


def _need_bin():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} missing: run __graft_entry__.build() (make -C tests/cpp -f extract_plan.mk)")


def test_extract_plan_pins_and_sweep():
    _need_bin()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "extract plan ok" in r.stdout, r.stdout + r.stderr[-3000:]


@pytest.mark.parametrize("case", extract_cases.CASES, ids=lambda c: c.id)
def test_case_table_names_its_plan(case):
    _need_bin()
    args = [case.rows, case.cols, case.k, case.S, case.P]
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    par, kc5, fused, lds_rows, lds_normals = (int(x) for x in r.stdout.split())
    assert (bool(par), bool(fused)) == (case.sector_parallel, case.fused)
    assert bool(kc5) == (case.k == 5)
    assert lds_rows == 32 * case.cols


def test_case_table_covers_all_eight_combinations():
    """(row kernel, KC, normals): every combination extract.hip can launch is in the table."""
    seen = {(c.sector_parallel, c.k == 5, c.fused) for c in extract_cases.CASES}
    assert len(seen) == 8

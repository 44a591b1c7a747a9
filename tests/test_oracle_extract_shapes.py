"""CPU oracle extraction vs the independent numpy restatement (tests/np_ref.py) over the
whole case table (tests/extract_cases.py): the yardstick of
tests/test_gpu_extract_shapes.py, checked shape by shape.

The assertions are those of test_oracle_extract.py::test_extract_matches_numpy: masks,
curvature and every selected index bit-exact; normals against numpy eigh in float64
(|dot| >= 1 - 1e-5, skipping near-degenerate covariances where the smallest eigenvector
is ill-defined — parity hazard 7).
"""
import numpy as np
import pytest

import extract_cases
import np_ref


@pytest.mark.parametrize("case", extract_cases.CASES, ids=lambda c: c.id)
def test_extract_matches_numpy_over_the_case_table(oracle, case):
    """A case that selects nothing or finds no normal (group F's first, one scan line)
    has no normals to compare; every other case must have compared most of them."""
    s = extract_cases.scan(case)
    p = extract_cases.params(case)
    ex = oracle.extract(s, p)
    sel, pts, planar, curv = np_ref.select(s, p)
    _, pointv = np_ref.masks(s, p)
    assert np.array_equal(ex["planar_mask"], planar)
    assert np.array_equal(ex["point_mask"], pointv)
    assert np.array_equal(ex["curvature"], curv)
    assert np.array_equal(ex["sel"].astype(np.int64), sel)
    assert np.array_equal(ex["point_idx"].astype(np.int64), pts)
    checked = nok = 0
    for i, idx in enumerate(ex["sel"]):
        ok, n, w = np_ref.normal(s, p, int(idx), planar)
        assert ok == bool(ex["normal_ok"][i])
        nok += ok
        if not ok or w[1] < w[0] * (1 + 1e-3) + 1e-12:
            continue
        assert abs(float(np.dot(n, ex["normals"][i]))) >= 1 - 1e-5
        checked += 1
    assert checked > 0.8 * nok or nok == 0
    extract_cases.check_preconditions(case, ex)

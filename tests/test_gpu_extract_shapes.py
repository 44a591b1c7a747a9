"""extract.hip off its default shapes, against the CPU oracle (tests/extract_cases.py).

The bars are those of test_gpu_parity.py::test_extract_matches_oracle: planar mask,
selected planar and point indices and the copied coordinates bit-exact, the found-normal
set equal to the oracle's, |n_gpu . n_oracle| >= 1 - 1e-6 on every found normal.  Each
case runs through the device pointer and the host pointer; the profiler's launch counts
tie the case to the kernels the table names for it (split normals launch under "closest",
fused ones never do); a sector-parallel case runs twice and must repeat itself bit for bit
(its candidate keys reach LDS in atomic order).
"""
import numpy as np
import pytest

import extract_cases

pytestmark = pytest.mark.gpu

_REF: dict = {}


def _ref(oracle, case):
    """The oracle's extraction of the case, computed once and left unchanged."""
    if case.id not in _REF:
        ex = oracle.extract(extract_cases.scan(case), extract_cases.params(case))
        for v in ex.values():
            v.setflags(write=False)
        _REF[case.id] = ex
    return _REF[case.id]


def _ctx(fmx, p):
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _run(ctx, scan, idx=0):
    counts = ctx.extract(scan, idx)
    got = ctx.extract_download(with_mask=True)
    got["counts"] = counts
    return got


def _check(got, ref, s):
    ok = ref["normal_ok"]
    assert np.array_equal(got["planar_mask"], ref["planar_mask"])
    assert got["counts"] == (int(ok.sum()), len(ref["point_idx"]), len(ref["sel"]))
    # the found-normal set is the oracle's: same selected indices survive, in order
    assert np.array_equal(got["planar_index"], ref["sel"][ok])
    assert np.array_equal(got["point_index"], ref["point_idx"])
    assert np.array_equal(got["planar"][:, :3], s[ref["sel"][ok], :3])
    assert np.array_equal(got["point"], s[ref["point_idx"], :3])
    if ok.any():
        dots = np.abs(np.sum(got["planar"][:, 3:].astype(np.float64) * ref["normals"][ok], 1))
        print(f"min |n_gpu . n_oracle| = {dots.min():.9f} over {len(dots)} normals")
        assert dots.min() >= 1 - 1e-6


def _same(a, b):
    for key in ("planar_mask", "planar_index", "point_index", "planar", "point"):
        assert np.array_equal(a[key], b[key]), key
    assert a["counts"] == b["counts"]


@pytest.mark.parametrize("case", extract_cases.CASES, ids=lambda c: c.id)
def test_extract_shape_matches_oracle(fmx_mod, oracle, case):
    import torch
    s = extract_cases.scan(case)
    p = extract_cases.params(case)
    ref = _ref(oracle, case)
    # the case is worth running: group D's last sector is over the sort capacity (or
    # exactly at it), a one-line scan still has selections to get right, ...
    extract_cases.check_preconditions(case, ref)

    ctx = _ctx(fmx_mod, p)
    try:
        dev = torch.from_numpy(s.copy()).to("cuda:0")
        ctx.profile(True)
        ctx.profile_reset()
        got = _run(ctx, dev)
        prof = ctx.profile_read()
        ctx.profile(False)
        _check(got, ref, s)
        # what ran is what the table says: one row launch; split normals under "closest"
        assert prof["extract_rows"]["launches"] == 1 and prof["fit"]["launches"] == 1
        assert (prof["closest"]["launches"] == 0) == case.fused, prof["closest"]
        assert prof["unpack"]["launches"] == 0
        # host pointer: the scan is staged (packed x, y, z) and unpacked on the device
        host = _run(ctx, s, 1)
        _check(host, ref, s)
        _same(host, got)
        if case.sector_parallel:
            again = _run(ctx, dev, 2)
            _same(again, got)
    finally:
        ctx.close()


def test_context_reused_on_a_sparser_scan_and_narrow_after_wide(fmx_mod, oracle):
    """Stale state.  A context's geometry is fixed when it is created, so a change of width
    is a new context: a wide split-path case, then a narrow fused one in the same process
    (whose scratch comes back from the allocator with the wide case's contents), must
    still match.  Within one context, a dense scan followed by one with most of its
    points gone must not see the dense scan's slots, counts or normals."""
    import torch
    wide, narrow = extract_cases.BY_ID["B-2560-k5"], extract_cases.BY_ID["A-200-S16"]
    for case in (wide, narrow):
        ctx = _ctx(fmx_mod, extract_cases.params(case))
        try:
            s = extract_cases.scan(case)
            _check(_run(ctx, torch.from_numpy(s.copy()).to("cuda:0")), _ref(oracle, case), s)
        finally:
            ctx.close()
    for case in (extract_cases.BY_ID["A-1800"], wide):  # fused and split normals
        p = extract_cases.params(case)
        dense = extract_cases.scan(case)
        sparse = dense.copy().reshape(case.rows, case.cols, 4)
        sparse[:, case.cols // 3:] = 0   # two thirds of every line dropped
        sparse[1] = 0                    # and one line entirely
        sparse = sparse.reshape(-1, 4)
        ref = oracle.extract(sparse, p)
        assert 0 < len(ref["sel"]) < len(_ref(oracle, case)["sel"]) // 2
        ctx = _ctx(fmx_mod, p)
        try:
            _check(_run(ctx, dense), _ref(oracle, case), dense)
            _check(_run(ctx, sparse, 1), ref, sparse)
            _check(_run(ctx, torch.from_numpy(sparse).to("cuda:0"), 2), ref, sparse)
        finally:
            ctx.close()

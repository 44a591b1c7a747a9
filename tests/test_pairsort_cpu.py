"""The pair sort's host side, CPU only: the numpy reference (tests/pairsort_ref.py) against
a naive per-query loop, and fmx_pair_sort_plan (form_amd/csrc/pair_sort_plan.hpp, host only:
no device is needed) pinned for every row of the case table (tests/pairsort_cases.py) and on
both sides of every dispatch boundary."""
import numpy as np
import pytest

import pairsort_cases as PC
import pairsort_ref as PR

SCAN_TILE = 4096  # words per block of the device-wide scan


def _naive(pair, pi, ni, q_pl, q_pt, K):
    """Row lists per (type, pair) filled by one pass over the queries in order."""
    npl = len(q_pl)
    rows = {(t, k): [] for t in (0, 1) for k in range(K)}
    for q in range(len(pair)):
        if pair[q] < 0:
            continue
        if q < npl:
            rows[0, pair[q]].append((pi[q], ni[q], q_pl[q, :3].astype(np.float64)))
        else:
            rows[1, pair[q]].append((pi[q], q_pt[q - npl].astype(np.float64)))
    out = dict(counts_plane=np.array([len(rows[0, k]) for k in range(K)], np.uint32),
               counts_point=np.array([len(rows[1, k]) for k in range(K)], np.uint32))
    for t, name, fields in ((0, "plane", ("pi", "ni", "pj")), (1, "point", ("pi", "pj"))):
        flat = [r for k in range(K) for r in rows[t, k]]
        for f, fname in enumerate(fields):
            out[f"{name}_{fname}"] = np.array([r[f] for r in flat], np.float64).reshape(-1, 3)
        base, run = [], 0
        for k in range(K):
            base.append(run)
            run += len(rows[t, k])
        out["base_" + name] = np.array(base, np.uint32)
    chunks, cr = [], []
    for k in range(K):
        cr.append(len(chunks))
        for t, name in ((0, "plane"), (1, "point")):
            b, n = int(out["base_" + name][k]), int(out["counts_" + name][k])
            r = 0
            while r < n:
                chunks.append((t, k, b + r, b + min(n, r + 256)))
                r += 256
    cr.append(len(chunks))
    out.update(chunk_range=np.array(cr, np.uint32), n_chunks=len(chunks),
               chunks=np.array(chunks, np.uint32).reshape(-1, 4))
    return out


def _random_match(rng, K, npl, npt):
    pair = rng.integers(-1, K, npl + npt).astype(np.int32)
    return (pair, rng.normal(size=(npl + npt, 3)), rng.normal(size=(npl, 3)),
            rng.normal(size=(npl, 6)).astype(np.float32), rng.normal(size=(npt, 3)).astype(np.float32))


@pytest.mark.parametrize("K,npl,npt", [(1, 7, 3), (3, 0, 40), (4, 900, 0), (6, 1300, 600), (9, 0, 0)])
def test_reference_equals_naive_loop(K, npl, npt):
    rng = np.random.default_rng(K * 1000 + npl)
    pair, pi, ni, q_pl, q_pt = _random_match(rng, K, npl, npt)
    if npl >= 900:  # one pair across chunk edges: 256 and 257 rows
        pair[:npl] = np.where(pair[:npl] == 0, 1, pair[:npl])
        pair[rng.permutation(npl)[:257]] = 0
    PR.assert_same(PR.pair_sort_ref(pair, pi, ni, q_pl, q_pt, K), _naive(pair, pi, ni, q_pl, q_pt, K))


def test_reference_is_stable_and_notices_a_swap():
    """Two rows of one pair exchanged (what a non-stable sort does) is a difference."""
    rng = np.random.default_rng(5)
    pair, pi, ni, q_pl, q_pt = _random_match(rng, 3, 200, 50)
    ref = PR.pair_sort_ref(pair, pi, ni, q_pl, q_pt, 3)
    bad = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in ref.items()}
    b = int(ref["base_plane"][1])
    assert ref["counts_plane"][1] >= 2
    bad["plane_pj"][[b, b + 1]] = bad["plane_pj"][[b + 1, b]]
    with pytest.raises(AssertionError):
        PR.assert_same(bad, ref)


def _plan(npl, npt, K, sorted=True):
    from form_amd import fmx
    return fmx.pair_sort_plan(npl, npt, K, sorted)


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.id)
def test_plan_of_every_case(case):
    p = _plan(case.npl, case.npt, case.K)
    qpb = 256 // case.group
    nb_pl, nb_pt = -(-case.npl // qpb), -(-case.npt // qpb)
    assert (p["group"], p["form"], p["scan_launches"]) == (case.group, case.form, case.scan_launches)
    assert (p["nb_pl"], p["nb_pt"]) == (nb_pl, nb_pt)
    assert (p["ntl_pl"], p["ntl_pt"]) == (-(-case.npl // 1024), -(-case.npt // 1024))
    assert p["hist_words"] == (case.K * (nb_pl + nb_pt) if case.form == "per-block" else 0)


@pytest.mark.parametrize("shape,want", PC.BOUNDARIES, ids=["-".join(map(str, s)) for s, _ in PC.BOUNDARIES])
def test_plan_boundaries(shape, want):
    p = _plan(*shape)
    assert (p["group"], p["form"], p["hist_words"], p["scan_launches"]) == want


def test_plan_pins():
    """The boundary rows come in pairs that differ by the least step across each threshold."""
    B = dict(PC.BOUNDARIES)
    assert B[110000, 21071, 40][0] == 8 and B[110000, 21072, 40][0] == 1             # 131071 | 131072 queries
    assert B[110000, 21072, 256][1] == "tail-scanned" and B[110000, 21072, 257][1] == "per-block"  # K 256 | 257
    assert _plan(6144 * 1024, 0, 1)["ntl_pl"] == 6144 and _plan(6144 * 1024 + 1, 0, 1)["ntl_pl"] == 6145
    assert B[32 * 32, 0, 512][2:] == (16384, 1) and B[29 * 32, 0, 565][2:] == (16385, 3)
    tiles = [-(-B[s][2] // SCAN_TILE) for s in ((4096 * 32, 0, 1024), (5 * 32, 0, 838861))]
    assert tiles == [1024, 1025]  # one pass of k_scan_blocks' loop | two
    # not sorted: no form, nothing scanned; no queries: nothing to scan
    assert _plan(2500, 700, 300, sorted=False)["form"] == "none"
    assert _plan(2500, 700, 300, sorted=False)["hist_words"] == 0
    assert _plan(0, 0, 300)["scan_launches"] == 0
    from form_amd import fmx
    assert fmx.lib().fmx_pair_sort_plan(1, 1, 1, 1, None) == 1  # FMX_E_INVAL


def test_table_reaches_every_form():
    forms = {(c.group, c.form) for c in PC.CASES}
    assert forms == {(8, "scatter-scanned"), (8, "tail-scanned"), (8, "per-block"), (1, "scatter-scanned"),
                     (1, "tail-scanned")}
    # the three scan forms of the per-block sort: one launch, three, three with > 1024 scan tiles
    scans = set()
    for c in PC.CASES:
        if c.form == "per-block":
            p = _plan(c.npl, c.npt, c.K)
            scans.add((p["scan_launches"], -(-p["hist_words"] // SCAN_TILE) > 1024))
    assert scans == {(1, False), (3, False), (3, True)}
    # both sides of each boundary are in the table itself, as far as a test-sized case reaches them
    ids = PC.BY_ID
    assert ids["E"].npl + ids["E"].npt == 131071 and ids["E'"].npl + ids["E'"].npt == 131072
    assert ids["B"].K * 24 == 6144 and (ids["B"].form, ids["C"].form) == ("scatter-scanned", "tail-scanned")
    assert (ids["F256"].K, ids["D"].K) == (256, 257)
    assert _plan(ids["D"].npl, ids["D"].npt, ids["D"].K)["hist_words"] <= 16384
    assert _plan(ids["D2"].npl, ids["D2"].npt, ids["D2"].K)["hist_words"] > 16384
    assert _plan(ids["D3"].npl, ids["D3"].npt, ids["D3"].K)["hist_words"] == 4195328 > 4194304


@pytest.mark.parametrize("cid", ["A", "C", "D2", "F64"])
def test_design_carries_the_count_patterns(cid):
    case = PC.BY_ID[cid]
    pl, pt = PC.case_design(case)
    R = PC.roles(case.K)
    cpl, cpt = PC.design_counts(case.K, pl, pt)
    for k in R["empty"]:
        assert cpl[k] == 0 and cpt[k] == 0
    for k, rows in zip(R["edge"], R["edge_rows"]):
        assert (cpl[k], cpt[k]) == (rows, 0)
    assert cpl[R["point_only"]] == 0 and cpt[R["point_only"]] > 0
    waves = pl[:len(pl) // 64 * 64].reshape(-1, 64)
    assert np.any(np.all(waves == R["wave"], axis=1))
    a, b = R["alt"]
    assert np.any(np.all(waves[:, 0::2] == a, axis=1) & np.all(waves[:, 1::2] == b, axis=1))
    s = 64 * ((len(pt) - 1) // 64)
    assert np.all(pt[:s] != R["last"]) and pt[s] == R["last"]
    assert (pl < 0).sum() > len(pl) // 20 and (pt < 0).sum() > len(pt) // 20  # unmatched, interleaved

"""The one-lane-per-query build of the match (fmx::gl, 131072 queries and more) and its
fused match + linearization at the search edges: the scenes of tests/match_edge_cases.py
(off-identity poses on four pairs, the same 1e5 m from the origin, exact ties in reference
shift order and queries on cell boundaries, dense and unsorted cells), cold, warm and
fused, on plain and subdivided maps, with the bounded and the unbounded search.

Bar of the match: bit-exact to the oracle VoxelMap over all queries (the contract of
tests/test_gpu_map.py::_check).  Bar of the systems: the project's 1e-10 of the largest
entry (tests/test_gpu_window.py), against the oracle's linearization of the oracle's own
match.  tests/test_match_edges_cpu.py shows on the CPU that the scenes realize their
design."""
import numpy as np
import pytest

import match_edge_cases as MC
from form_amd import synth
from scenario import perturb

pytestmark = pytest.mark.gpu

REL = 1e-10
SIGMA = 0.1


def _ctx(fmx, sc, subdiv):
    p = synth.default_params(synth.GEOMETRIES["tiny"])
    ctx = fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p), voxel_subdivision=subdiv))
    for k, (pl, pt) in enumerate(sc["scans"]):
        ctx.keypoints_add(k, pl, pt)
    ctx.map_build(list(range(len(sc["scans"]))), sc["poses"], sc["w"])
    return ctx


def _set_queries(fmx, ctx, sc):
    K = len(sc["scans"])
    assert fmx.pair_sort_plan(len(sc["q_pl"]), len(sc["q_pt"]), K)["group"] == 1  # the one-lane build
    ctx.set_queries(sc["q_pl"], sc["q_pt"], K)


def _first(sc, t, bad):
    """The first differing queries of a type and their edge blocks."""
    idx = np.nonzero(bad)[0][:4]
    return [(int(i), MC.describe(sc, **{"i_" + t: i})) for i in idx]


def _compare(sc, got, counts, refs, max_dist, K):
    """The bit-exact contract over all queries; counts: (cpl, cpt) or None."""
    npl = len(sc["q_pl"])
    for t, ref in zip(("pl", "pt"), refs):
        sl = slice(0, npl) if t == "pl" else slice(npl, None)
        acc = ref["found"] & (ref["d2"] < max_dist * max_dist)
        pair, d2, pi = got["pair"][sl], got["d2"][sl], got["pi"][sl]
        bad = (pair >= 0) != acc
        assert not bad.any(), ("accepted set", t, int(bad.sum()), _first(sc, t, bad))
        bad = acc & (pair.astype(np.int64) != np.where(acc, ref["scan"].astype(np.int64), -1))
        assert not bad.any(), ("pair", t, int(bad.sum()), _first(sc, t, bad), pair[bad][:4], ref["scan"][bad][:4])
        bad = acc & (d2 != ref["d2"])
        assert not bad.any(), ("d2", t, int(bad.sum()), _first(sc, t, bad), d2[bad][:4], ref["d2"][bad][:4])
        bad = acc & (pi != ref["pi"]).any(1)
        assert not bad.any(), ("pi", t, int(bad.sum()), _first(sc, t, bad), pi[bad][:4], ref["pi"][bad][:4])
        if t == "pl":
            bad = acc & (got["ni"] != ref["ni"]).any(1)
            assert not bad.any(), ("ni", int(bad.sum()), _first(sc, t, bad))
        bad = (d2 > 0.01) != (~ref["found"] | (ref["d2"] > 0.01))
        assert not bad.any(), ("insert decision", t, int(bad.sum()), _first(sc, t, bad))
        if max_dist > sc["w"]:  # the unbounded search: every neighbour the reference finds, accepted or not
            bad = ref["found"] & (d2 != ref["d2"])
            assert not bad.any(), ("found d2", t, int(bad.sum()), _first(sc, t, bad), d2[bad][:4], ref["d2"][bad][:4])
        if counts is not None:
            want = np.bincount(ref["scan"][acc].astype(np.int64), minlength=K)
            assert np.array_equal(counts[0 if t == "pl" else 1], want), ("counts", t, counts, want)


def _match_check(ctx, oracle, name, Tj, max_dist):
    sc = MC.scene(name)
    counts = ctx.match(Tj, max_dist)
    got = ctx.match_download()
    _compare(sc, got, counts, MC.oracle_match(oracle, name, Tj), max_dist, len(sc["scans"]))
    return got


# ------------------------------------------------------------------------- a. cold search
GRID = [("plain", 1, 1.0), ("plain", 2, 1.0), ("plain", 1, 1.25), ("plain_far", 1, 1.0),
        ("ties", 1, 1.0), ("ties", 1, 1.3), ("ties", 2, 1.0),
        ("dense", 1, 1.0), ("dense", 2, 1.0), ("dense", 1, 1.25)]


@pytest.mark.parametrize("name,subdiv,rel_dist", GRID)
def test_cold_search_matches_oracle(fmx_mod, oracle, name, subdiv, rel_dist):
    """One cold match per query pose of the scene (a new query set each: no warm state);
    max_dist = rel_dist * w, above w the unbounded search.  `ties`: the designed winners by
    name, and the tie block alone (a small set: the eight-lane build) agrees with the oracle
    and, query for query, with what the one-lane build returned for it."""
    sc = MC.scene(name)
    max_dist = rel_dist * sc["w"]
    K = len(sc["scans"])
    ctx = _ctx(fmx_mod, sc, subdiv)
    for i_pose, Tj in enumerate(sc["Tj"]):
        _set_queries(fmx_mod, ctx, sc)
        got = _match_check(ctx, oracle, name, Tj, max_dist)
        if name != "ties":
            continue
        npl = len(sc["q_pl"])
        want = MC.tie_winners(sc, i_pose, max_dist)
        a_pl, a_pt, ipl, ipt = MC.tie_block_alone(sc)
        assert list(got["pair"][ipl]) == want, (i_pose, dict(zip(2 * sc["tie_names"], got["pair"][ipl])))
        assert list(got["pair"][npl + ipt]) == want, (i_pose, dict(zip(2 * sc["tie_names"], got["pair"][npl + ipt])))
        # the block alone, on the eight-lane build
        assert fmx_mod.pair_sort_plan(len(a_pl), len(a_pt), K)["group"] == 8
        ctx.set_queries(a_pl, a_pt, K)
        cpl, cpt = ctx.match(Tj, max_dist)
        alone = ctx.match_download()
        rpl, rpt = MC.oracle_match(oracle, name, Tj)
        small = dict(sc, q_pl=a_pl, q_pt=a_pt, blocks={})
        _compare(small, alone, (cpl, cpt), ({k: v[ipl] for k, v in rpl.items()}, {k: v[ipt] for k, v in rpt.items()}),
                 max_dist, K)
        big = np.concatenate([ipl, npl + ipt])
        assert np.array_equal(alone["pair"], got["pair"][big])
        acc = alone["pair"] >= 0 if max_dist <= sc["w"] else np.ones(len(big), bool)
        assert np.array_equal(alone["d2"][acc], got["d2"][big][acc])
        assert np.array_equal(alone["pi"][acc], got["pi"][big][acc])
        assert np.array_equal(alone["ni"][acc[:len(ipl)]], got["ni"][ipl][acc[:len(ipl)]])
    ctx.close()


# ----------------------------------------------------------------------- b. warm rematch
@pytest.mark.parametrize("name", ["plain", "dense"])
def test_warm_rematch_matches_oracle(fmx_mod, oracle, name):
    """One map and one query set matched at a start pose, a sub-millimetre step, a 5 cm
    step that moves many queries across cell faces, and the first pose again: every match
    after the first starts warm (bounded by the previous record, the own cell from the
    per-query cache) and is bit-exact to the oracle.  A warm match at an unchanged pose
    probes no more bricks than a cold one at that pose."""
    sc = MC.scene(name)
    w = sc["w"]
    T0 = sc["Tj"][0]
    rng = np.random.default_rng(29)
    T1 = perturb(T0, rng, 1e-5, 2e-4)
    T2 = perturb(T1, rng, 0.002, 0.05)
    moved = np.floor((sc["q_pl"][:, :3].astype(np.float64) @ T2[:, :3].T + T2[:, 3]) / w) != \
        np.floor((sc["q_pl"][:, :3].astype(np.float64) @ T1[:, :3].T + T1[:, 3]) / w)
    assert moved.any(1).sum() > 5000  # the 5 cm step crosses cell faces
    ctx = _ctx(fmx_mod, sc, 1)
    ctx.profile(True)
    _set_queries(fmx_mod, ctx, sc)
    nq = len(sc["q_pl"]) + len(sc["q_pt"])
    for i, T in enumerate([T0, T1, T2, T0, T0]):
        _match_check(ctx, oracle, name, T, w)
        cc = ctx.match_cert()
        assert (cc["warm"] == 0) if i == 0 else (0.9 * nq < cc["warm"] <= nq), (i, cc)
    warm = ctx.match_work()  # at T0, after a match at T0
    _set_queries(fmx_mod, ctx, sc)  # same features, new query set: a cold match
    _match_check(ctx, oracle, name, T0, w)
    assert ctx.match_cert()["warm"] == 0
    cold = ctx.match_work()
    ctx.profile(False)
    print(f"{name}: probes per query warm {warm['probes'] / nq:.3f}, cold {cold['probes'] / nq:.3f}; "
          f"candidates warm {warm['candidates'] / nq:.2f}, cold {cold['candidates'] / nq:.2f}")
    assert warm["queries"] == cold["queries"] == nq
    assert warm["probes"] <= cold["probes"], (warm, cold)
    ctx.close()


# --------------------------------------------------------- c. fused match + linearization
def _oracle_systems(oracle, sc, refs, Tj, max_dist):
    """Per-pair single-pose systems (K, 28) and errors (K,) of the oracle's own match: rows
    pair-major, the fp32 queries widened to fp64."""
    K = len(sc["scans"])
    rows = []
    for ref, Q in zip(refs, (sc["q_pl"], sc["q_pt"])):
        acc = ref["found"] & (ref["d2"] < max_dist * max_dist)
        pair = ref["scan"][acc].astype(np.int64)
        order = np.argsort(pair, kind="stable")
        rows.append((np.bincount(pair, minlength=K), ref["pi"][acc][order], ref["ni"][acc][order],
                     Q[acc, :3].astype(np.float64)[order]))
    (n_pl, ppi, pni, ppj), (n_pt, tpi, _, tpj) = rows
    return oracle.linearize(n_pl.astype(np.uint32), ppi, pni, ppj, n_pt.astype(np.uint32), tpi, tpj, sc["poses"],
                            np.tile(Tj, (K, 1, 1)), SIGMA, True)


def _close(S, e, Sr, er):
    return np.all(np.abs(S - Sr) <= REL * np.abs(Sr).max()) and abs(e - er) <= REL * er


@pytest.mark.parametrize("name,subdiv", [("plain", 1), ("plain", 2), ("dense", 1)])
def test_fused_match_linearize_matches_oracle(fmx_mod, oracle, name, subdiv):
    """A deferred match consumed by fmx_linearize_matched at the same pose: one
    match_linearize launch, no match launch, and the summed system of K pairs at
    off-identity poses (plain: k_match<false, true>, dense: k_match<true, true>) equals
    the oracle's linearization of the oracle's match.  The download then settles the
    deferred match (bit-exact), the stored-results path and the window kernel's per-pair
    systems meet the same bar, a pose that accepts nothing gives exact zeros, and the call
    after it is right again (the reduction tickets were reset)."""
    sc = MC.scene(name)
    w, K, Tj = sc["w"], len(sc["scans"]), sc["Tj"][0]
    refs = MC.oracle_match(oracle, name, Tj)
    Gr, errr = _oracle_systems(oracle, sc, refs, Tj, w)
    Sr, er = Gr.sum(0), errr.sum()
    ctx = _ctx(fmx_mod, sc, subdiv)
    _set_queries(fmx_mod, ctx, sc)
    ctx.profile(True)
    ctx.profile_reset()
    assert ctx.match(Tj, w, counts=False) is None  # deferred
    S, e = ctx.linearize_matched(Tj, SIGMA)
    prof = ctx.profile_read()
    assert prof["match_linearize"]["launches"] == 1 and prof["match"]["launches"] == 0, prof
    print(f"{name}/{subdiv}: fused max |S - Sr| / max |Sr| = {np.abs(S - Sr).max() / np.abs(Sr).max():.3e}, "
          f"|e - er| / er = {abs(e - er) / er:.3e}")
    assert _close(S, e, Sr, er), (S - Sr, np.abs(Sr).max(), e, er)
    got = ctx.match_download()  # settles the deferred match
    assert ctx.profile_read()["match"]["launches"] == 1
    _compare(sc, got, None, refs, w, K)
    S2, e2 = ctx.linearize_matched(Tj, SIGMA)  # the stored results: k_linearize_total
    assert ctx.profile_read()["match_linearize"]["launches"] == 1
    assert _close(S2, e2, Sr, er), (S2 - Sr, e2, er)
    G, err = ctx.linearize(sc["poses"], np.tile(Tj, (K, 1, 1)), SIGMA, True)  # the window kernel, per pair
    for k in range(K):
        assert _close(G[k], err[k], Gr[k], errr[k]), (k, G[k] - Gr[k], err[k], errr[k])
    # nothing accepted: exact zeros; then the real pose again
    Taway = MC.translated(Tj, (500.0, 0.0, 0.0))
    ctx.match(Taway, w, counts=False)
    S0, e0 = ctx.linearize_matched(Taway, SIGMA)
    assert not S0.any() and e0 == 0.0, (S0, e0)
    ctx.match(Tj, w, counts=False)
    S3, e3 = ctx.linearize_matched(Tj, SIGMA)
    assert ctx.profile_read()["match_linearize"]["launches"] == 3
    ctx.profile(False)
    assert _close(S3, e3, Sr, er), (S3 - Sr, e3, er)
    ctx.close()

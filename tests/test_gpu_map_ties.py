"""Exact ties in full cells: the lattice scenes of tests/map_lattice_cases.py on the device.
Thousands of queries exactly equidistant from 2, 4 or 8 records, in cells the lane group
walks (64 records), sorted dense cells (512), an unsorted dense cell (> 8192), on the
seam between dense and plain cells and on subdivided maps (ring 2), with the tied records
in different sub-cells, cells, bricks and scans: the argmin key (d^2, reference shift rank,
build order) of fold / group_min / srank decides every one of them.

Bar: bit equality with the oracle's VoxelMap over all queries (the contract of
tests/test_gpu_mapbuild.py::_check: accepted set, pair, d2, pi, ni, per-pair counts), cold
and warm, on the eight-lane build of the match and, interleaved into filler queries over
empty space, on the one-lane build.  tests/test_map_lattice_cpu.py shows on the CPU that
the scenes realize their design and that the oracle's winners are the reference rule's."""
import numpy as np
import pytest

import map_lattice_cases as ML

pytestmark = pytest.mark.gpu


def _ctx(fmx, sc):
    ctx = fmx.Context(fmx.EstimatorParams(voxel_subdivision=sc["subdiv"]))
    for k, (pl, pt) in enumerate(sc["scans"]):
        ctx.keypoints_add(k, pl, pt)
    ctx.map_build(list(range(ML.K)), sc["poses"], sc["w"])
    return ctx


def _first(sc, t, at, bad):
    """The first differing tie queries of a type: class, multiplicity, block."""
    where = np.nonzero(bad)[0][:4]
    return [ML.describe(sc, t, int(np.nonzero(at == i)[0][0])) if i in at else ("filler", int(i)) for i in where]


def _compare(sc, got, counts, refs, at_pl, at_pt, n_pl, n_pt):
    """The bit-exact contract; the tie queries are rows at_pl / at_pt of the query arrays,
    every other row is filler that finds nothing."""
    w = sc["w"]
    for t, ref, at, sl in (("pl", refs[0], at_pl, slice(0, n_pl)), ("pt", refs[1], at_pt, slice(n_pl, None))):
        n = n_pl if t == "pl" else n_pt
        acc = np.zeros(n, bool)
        acc[at] = ref["found"] & (ref["d2"] < w * w)
        want = {k: np.zeros((n,) + ref[k].shape[1:], ref[k].dtype) for k in ("scan", "d2", "pi", "ni")}
        for k in want:
            want[k][at] = ref[k]
        pair, d2, pi = got["pair"][sl], got["d2"][sl], got["pi"][sl]
        bad = (pair >= 0) != acc
        assert not bad.any(), ("accepted set", int(bad.sum()), _first(sc, t, at, bad))
        bad = acc & (pair.astype(np.int64) != want["scan"].astype(np.int64))
        assert not bad.any(), ("pair", int(bad.sum()), _first(sc, t, at, bad), pair[bad][:4], want["scan"][bad][:4])
        bad = acc & (d2 != want["d2"])
        assert not bad.any(), ("d2", int(bad.sum()), _first(sc, t, at, bad), d2[bad][:4], want["d2"][bad][:4])
        bad = acc & (pi != want["pi"]).any(1)
        assert not bad.any(), ("pi", int(bad.sum()), _first(sc, t, at, bad), pi[bad][:4], want["pi"][bad][:4])
        if t == "pl":
            bad = acc & (got["ni"] != want["ni"]).any(1)
            assert not bad.any(), ("ni", int(bad.sum()), _first(sc, t, at, bad))
        cnt = np.bincount(want["scan"][acc].astype(np.int64), minlength=ML.K)
        assert np.array_equal(counts[0 if t == "pl" else 1], cnt), ("counts", sc["name"], t, counts, cnt)


def _cold_and_warm(ctx, sc, oracle, q_pl, q_pt, at_pl, at_pt):
    refs = ML.oracle_match(oracle, sc["name"])
    ctx.set_queries(q_pl, q_pt, ML.K)
    out = []
    for i in range(2):  # the second match starts warm: bounded by the previous nearest record
        counts = ctx.match(sc["Tj"], sc["w"])
        got = ctx.match_download()
        cc = ctx.match_cert()
        # warm: the queries whose previous record lies within max_dist (d2 <= w^2; accepted: d2 < w^2)
        lo, hi = (sum(int((r["found"] & op(r["d2"], sc["w"] ** 2)).sum()) for r in refs) for op in (np.less, np.less_equal))
        assert (cc["warm"] == 0) if i == 0 else (20000 < lo <= cc["warm"] <= hi), (i, cc, lo, hi)
        _compare(sc, got, counts, refs, at_pl, at_pt, len(q_pl), len(q_pt))
        out.append((got, counts))
    (cold, c_cold), (warm, c_warm) = out
    for k in ("pair", "d2", "pi", "ni"):
        assert cold[k].tobytes() == warm[k].tobytes(), (sc["name"], sc["cls"], k)
    assert np.array_equal(c_cold[0], c_warm[0]) and np.array_equal(c_cold[1], c_warm[1])
    return cold


@pytest.mark.parametrize("name", ML.SCENES)
def test_ties_eight_lane_build(fmx_mod, oracle, name):
    sc = ML.scene(name)
    assert fmx_mod.pair_sort_plan(ML.N_TIE, ML.N_TIE, ML.K)["group"] == 8
    ctx = _ctx(fmx_mod, sc)
    at = np.arange(ML.N_TIE)
    _cold_and_warm(ctx, sc, oracle, sc["q_pl"], sc["q_pt"], at, at)
    ctx.close()


@pytest.mark.parametrize("name", ML.SCENES)
def test_ties_one_lane_build(fmx_mod, oracle, name):
    sc = ML.scene(name)
    q_pl, q_pt, at_pl, at_pt = ML.with_filler(sc)
    assert len(q_pl) % 256 != 0 and len(q_pt) % 256 != 0
    assert fmx_mod.pair_sort_plan(len(q_pl), len(q_pt), ML.K)["group"] == 1
    ctx = _ctx(fmx_mod, sc)
    _cold_and_warm(ctx, sc, oracle, q_pl, q_pt, at_pl, at_pt)
    ctx.close()

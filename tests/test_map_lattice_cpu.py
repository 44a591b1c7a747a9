"""The lattice scenes of tests/map_lattice_cases.py realize their design, on the CPU oracle
and in numpy alone: the conditions that keep tests/test_gpu_map_ties.py and
tests/test_gpu_map_complete.py from being vacuous (the cells have the record counts that
send the search down the path the scene is named for, the queries are exactly tied 2, 4
and 8 ways, the oracle resolves every tie by the reference's rule, ties cross sub-cells,
bricks and the dense / plain seam, and the records are h apart)."""
import numpy as np
import pytest

import map_lattice_cases as ML

TYPES = (("pl", 0), ("pt", 1))


def _cells_of(sc, t):
    """Per record: internal cell (n, 3), sub-cell (n,), records in its cell (n,)."""
    cw = sc["w"] / sc["subdiv"]
    wp = ML.world(sc, t)
    cell = np.floor(wp / cw).astype(np.int64)
    sub = np.clip(np.floor((wp - cell * cw) / (cw / 4)).astype(np.int64), 0, 3)
    cells, inv, cnt = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
    return cell, sub[:, 0] + 4 * sub[:, 1] + 16 * sub[:, 2], cnt[inv.reshape(-1)]


@pytest.mark.parametrize("name", ML.SCENES)
def test_scene_realizes_its_class(name):
    sc = ML.scene(name)
    assert sc["w"] == ML.W and len(sc["scans"]) == ML.K == len(sc["poses"])
    assert sc["q_pl"].dtype == np.float32 and sc["q_pt"].dtype == np.float32
    assert len(sc["q_pl"]) == len(sc["q_pt"]) == ML.N_TIE
    for k, (pl, pt) in enumerate(sc["scans"]):
        assert pl.dtype == np.float32 and pt.dtype == np.float32 and len(pl) > 0 and len(pt) > 0
        assert np.array_equal(sc["poses"][k][:, :3], np.eye(3)) and np.array_equal(sc["poses"][k][:, 3], ML.T[k])
    lo, hi = sc["rpc"]
    for t, _ in TYPES:
        r = sc["rec"][t]
        assert len(r["iw"]) <= 64 ** 3
        # the scans are the records in build order
        assert np.array_equal(np.vstack([s[t == "pt"][:, :3] for s in sc["scans"]]), r["local"])
        assert np.array_equal(ML.world(sc, t), r["iw"] * ML.UNIT)
        cells, cnt = ML.cell_counts(sc, t)
        vox = cells // sc["subdiv"]
        assert vox.min() == -2 and vox.max() == 1 or t == "pt" and vox.min() >= -2 and vox.max() <= 1  # <= 4 voxels per axis
        assert cells.min() < 0 < cells.max()  # negative and positive cell indices
        print(f"{name} {t}: {len(r['iw'])} records, {len(cells)} cells of {cnt.min()}..{cnt.max()}")
        if name == "unsorted":
            assert (cnt > ML.UNSORTED_MIN).sum() == 1 and lo <= cnt.max() <= hi
            assert np.sort(cnt)[-2] <= ML.DENSE_MIN  # plain cells around it
        else:
            assert lo <= cnt.min() and cnt.max() <= hi
        if name in ("walk", "sub_walk"):
            assert cnt.max() <= ML.DENSE_MIN  # no dense cell: the DENSE = false kernel
        if name in ("sorted", "sub_sorted", "mixed"):
            assert ML.DENSE_MIN < cnt.max() <= ML.UNSORTED_MIN
        if name == "mixed":
            assert (cnt > ML.DENSE_MIN).any() and (cnt <= ML.DENSE_MIN).any()
            assert (cnt[cells[:, 0] < 0] == 512).all() and (cnt[cells[:, 0] >= 0] == 64).all()


@pytest.mark.parametrize("name", ML.SCENES)
def test_records_are_h_apart(name):
    """Completeness is decidable: distinct records differ by a whole number of h on every
    axis (so by at least h), and neighbours at exactly h exist."""
    sc = ML.scene(name)
    hu = int(round(sc["h"] / ML.UNIT))
    for t, _ in TYPES:
        iw = np.rint(ML.world(sc, t) / ML.UNIT).astype(np.int64)
        assert np.array_equal(iw * ML.UNIT, ML.world(sc, t))
        assert (iw % hu == 0).all() and len(np.unique(iw, axis=0)) == len(iw)
        keys = np.sort(ML._key(iw))
        nb = ML._key(iw + np.array([hu, 0, 0]))
        assert (keys[np.clip(np.searchsorted(keys, nb), 0, len(keys) - 1)] == nb).any()


@pytest.mark.parametrize("name", ML.SCENES)
def test_ties_exist_and_the_oracle_follows_the_reference_rule(oracle, name):
    sc = ML.scene(name)
    refs = ML.oracle_match(oracle, name)
    for t, kind in TYPES:
        a, ref, r = ML.tie_analysis(sc, t), refs[kind], sc["rec"][t]
        # every record at the minimum lies in one of the reference's 27 voxels
        assert a["visible"][a["tied"]].all()
        assert ref["found"].all()
        bad = ref["d2"] != a["dmin"]
        assert not bad.any(), (name, t, int(bad.sum()), np.nonzero(bad)[0][:4])
        mult = np.bincount(a["mult"], minlength=9)
        print(f"{name} {t}: queries of multiplicity 1 / 2 / 4 / 8: {mult[1]} / {mult[2]} / {mult[4]} / {mult[8]}"
              f" (others {mult.sum() - mult[[1, 2, 4, 8]].sum()})")
        assert mult[2] >= 500 and mult[4] >= 500 and mult[8] >= 500, mult
        # a sample in plain Python: the minimum and its multiplicity over ALL records
        wp = ML.world(sc, t)
        Q = sc["q_pl" if t == "pl" else "q_pt"][:, :3].astype(np.float64)
        for i in np.random.default_rng(7).choice(ML.N_TIE, 40, replace=False):
            d = wp - Q[i]
            d2 = (d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]) + d[:, 1] * d[:, 1]
            assert d2.min() == a["dmin"][i] and (d2 == d2.min()).sum() == a["mult"][i], (name, t, i)
            assert set(np.nonzero(d2 == d2.min())[0]) == set(a["cand"][i][a["tied"][i]])
        # the rule: first of the 27 shifts among the tied records, then build order
        w = a["winner"]
        bad = ref["scan"].astype(np.int64) != r["scan"][w]
        assert not bad.any(), (name, t, int(bad.sum()), [ML.describe(sc, t, i) for i in np.nonzero(bad)[0][:4]])
        assert np.array_equal(ref["pi"], r["local"][w].astype(np.float64))
        if t == "pl":
            assert np.array_equal(ref["ni"], r["nrm"][w].astype(np.float64))
        # the rule decides: on many tie queries the first tied record in build order loses,
        # and the tied records belong to different scans
        first = np.where(a["tied"], np.maximum(a["cand"], 0), 1 << 40).min(1)
        assert (first != w).sum() >= 200
        sc_of = np.where(a["tied"], r["scan"][np.maximum(a["cand"], 0)], -1)
        assert ((sc_of.max(1) != np.where(a["tied"], sc_of, 99).min(1)) & (a["mult"] > 1)).sum() >= 5000


@pytest.mark.parametrize("name", ML.DENSE_SCENES)
def test_ties_cross_sub_cells_bricks_and_the_seam(name):
    sc = ML.scene(name)
    for t, _ in TYPES:
        a = ML.tie_analysis(sc, t)
        cell, sub, n_in = _cells_of(sc, t)
        assert a["mult"].max() <= 8
        first8 = np.argsort(~a["tied"], axis=1, kind="stable")[:, :8]  # the tied candidates of each query
        c = np.maximum(np.take_along_axis(a["cand"], first8, 1), 0)
        tied = np.take_along_axis(a["tied"], first8, 1)
        ckey, bkey = ML._key(cell[c]), ML._key(cell[c] >> 1)
        dense = tied & (n_in[c] > ML.DENSE_MIN)
        plain = tied & (n_in[c] <= ML.DENSE_MIN)
        # two tied records in one dense cell, in different sub-cells of it
        pair = dense[:, :, None] & dense[:, None, :] & (ckey[:, :, None] == ckey[:, None, :])
        n_sub = int((pair & (sub[c][:, :, None] != sub[c][:, None, :])).any((1, 2)).sum())
        n_brick = int((np.where(tied, bkey, bkey[:, [0]]) != bkey[:, [0]]).any(1).sum())
        n_seam = int((dense.any(1) & plain.any(1)).sum())
        print(f"{name} {t}: tie queries across sub-cells of one dense cell {n_sub}, across bricks {n_brick}, "
              f"dense vs plain {n_seam}")
        assert n_sub >= 200 and n_brick >= 200
        if name == "mixed":
            assert n_seam >= 50
            assert (a["mult"][sc["blocks"]["seam"][t]] == 2).all()
            assert (dense.any(1) & plain.any(1))[sc["blocks"]["seam"][t]].all()


def test_filler_reaches_the_one_lane_build():
    sc = ML.scene("walk")
    q_pl, q_pt, at_pl, at_pt = ML.with_filler(sc)
    assert len(q_pl) + len(q_pt) >= 131072 and len(q_pl) % 256 != 0 and len(q_pt) % 256 != 0
    assert np.array_equal(q_pl[at_pl], sc["q_pl"]) and np.array_equal(q_pt[at_pt], sc["q_pt"])
    assert np.diff(at_pl).min() > 1 and np.diff(at_pt).min() > 1
    # the filler lies more than two voxels from every record and every tie query
    rest = np.ones(len(q_pl), bool)
    rest[at_pl] = False
    assert q_pl[rest, 0].min() > 50 and max(np.abs(ML.world(sc, "pl")).max(), np.abs(sc["q_pl"][:, :3]).max()) < 4

"""The scenes of tests/match_edge_cases.py realize their design, on the CPU oracle alone:
the conditions that keep tests/test_gpu_match_onelane.py from being vacuous (enough
queries for the one-lane build, partial blocks and a partial reduction group, most
queries accepted on every pair, exact ties whose oracle winner is the designed one,
dense cells with queries inside them)."""
import numpy as np
import pytest

import match_edge_cases as MC


def oracle_match(oracle, name):
    """[(planar ref, point ref)] per query pose of the scene."""
    return [MC.oracle_match(oracle, name, Tj) for Tj in MC.scene(name)["Tj"]]


@pytest.mark.parametrize("name", MC.SCENES)
def test_scene_reaches_the_one_lane_build_with_partial_blocks(name):
    sc = MC.scene(name)
    n_pl, n_pt = len(sc["q_pl"]), len(sc["q_pt"])
    assert sc["q_pl"].dtype == np.float32 and sc["q_pt"].dtype == np.float32
    assert n_pl + n_pt >= 128 * 1024 == MC.LARGE_MIN
    assert n_pl % MC.BLOCK != 0 and n_pt % MC.BLOCK != 0
    assert (-(-n_pl // MC.BLOCK) + -(-n_pt // MC.BLOCK)) % MC.FZ_GROUP != 0
    assert len(sc["poses"]) == len(sc["scans"]) <= 256
    # the index map partitions the queries, and the edge blocks are interleaved, not appended
    for t, n in (("pl", n_pl), ("pt", n_pt)):
        allidx = np.concatenate([b[t] for b in sc["blocks"].values()])
        assert np.array_equal(np.sort(allidx), np.arange(n))
        for k, b in sc["blocks"].items():
            if k != "filler" and len(b[t]) > 1:
                assert np.diff(b[t]).min() > 1 and b[t].max() < n - MC.BLOCK


@pytest.mark.parametrize("name", ["plain", "plain_far"])
def test_plain_scenes_accept_most_queries_on_every_pair(oracle, name):
    sc = MC.scene(name)
    assert len(sc["scans"]) == 4
    (rpl, rpt), = oracle_match(oracle, name)
    md2 = sc["w"] * sc["w"]
    out = []
    for ref, floor in ((rpl, 100000), (rpt, 10000)):
        acc = ref["found"] & (ref["d2"] < md2)
        per_pair = np.bincount(ref["scan"][acc].astype(np.int64), minlength=4)
        out.append((int(acc.sum()), per_pair.tolist()))
        assert acc.sum() >= floor, out
        assert per_pair.min() >= 1000, out
    print(f"{name}: accepted planar {out[0][0]} {out[0][1]}, point {out[1][0]} {out[1][1]}")
    # far from identity poses; far away, large negative world cells inside the key range
    assert all(np.abs(T[:, :3] - np.eye(3)).max() > 0.05 for T in list(sc["poses"]) + sc["Tj"])
    cells, cnt = MC.world_cell_counts(sc)
    assert cnt.max() < MC.DENSE_MIN  # no dense cell
    if name == "plain_far":
        assert np.abs(sc["q_pl"][:, :3]).max() < 64  # local coordinates stay small
        assert np.abs(cells).max() > 100000 and 2 * np.abs(cells).max() + 2 < 2 ** 19 - 2  # (also at half width)
    # the two scenes differ in nothing but the translation
    a, b = MC.scene("plain"), MC.scene("plain_far")
    assert np.array_equal(a["q_pl"], b["q_pl"]) and np.array_equal(a["poses"][:, :, :3], b["poses"][:, :, :3])
    assert np.array_equal(b["poses"][:, :, 3] - a["poses"][:, :, 3], np.tile(MC.FAR, (4, 1)))


def _d2(rec, q):
    """The reference's (dx*dx + dz*dz) + dy*dy in fp64."""
    d = np.asarray(rec, np.float64) - np.asarray(q, np.float64)
    return (d[0] * d[0] + d[2] * d[2]) + d[1] * d[1]


def test_ties_are_exact_and_the_oracle_takes_the_designed_record(oracle):
    sc = MC.scene("ties")
    cases = MC.tie_cases()
    n = len(cases)
    assert [c[0] for c in cases] == sc["tie_names"] and len(set(sc["tie_names"])) == n
    for i_pose, (Tj, block) in enumerate(zip(sc["Tj"], ("ties_origin", "ties_far"))):
        assert np.array_equal(Tj[:, :3], np.eye(3))
        b = sc["blocks"][block]
        for t, Q in (("pl", sc["q_pl"]), ("pt", sc["q_pt"])):
            kind = 0 if t == "pl" else 1
            ref = oracle_match(oracle, "ties")[i_pose][kind]
            for r, (name, s0, s1, _, win, d2) in enumerate(cases):
                # world coordinates in fp64 from the fp32 local ones, as the map computes them
                qw = Q[b[t][r], :3].astype(np.float64) + Tj[:, 3]
                recs = []
                for k in (0, 1):
                    kk = k + 2 * i_pose
                    F = sc["scans"][kk][kind]
                    off = sum(len(c[1 + k]) for c in cases[:r])
                    for j in range(len(cases[r][1 + k])):
                        recs.append((k, F[off + j, :3].astype(np.float64) + sc["poses"][kk][:, 3]))
                d = [_d2(p, qw) for _, p in recs]
                assert all(x == d2 for x in d), (name, block, t, d, d2)  # tied exactly, at the designed distance
                if name != "at_max_dist":
                    assert len(recs) == 2 and recs[0][0] != recs[1][0]
                i = b[t][r]
                assert ref["found"][i] and ref["d2"][i] == d2, (name, block, t)
                assert ref["scan"][i] == win + 2 * i_pose, (name, block, t, int(ref["scan"][i]))
            # the other copy's queries find nothing at this pose
            other = sc["blocks"]["ties_far" if i_pose == 0 else "ties_origin"][t]
            assert not ref["found"][other].any()
            # designed pairs at both radii of the device tests
            for md in (1.0, 1.3):
                want = np.array(MC.tie_winners(sc, i_pose, md))
                idx = np.concatenate([sc["blocks"]["ties_origin"][t], sc["blocks"]["ties_far"][t]])
                acc = ref["found"][idx] & (ref["d2"][idx] < md * md)
                got = np.where(acc, ref["scan"][idx].astype(np.int64), -1)
                assert np.array_equal(got, want), (block, t, md, got, want)
    # the example of the design: off centre, the nearer -x record loses to +x (scan 1; far: scan 3)
    r = sc["tie_names"].index("off_face")
    for i_pose, block in enumerate(("ties_origin", "ties_far")):
        ref = oracle_match(oracle, "ties")[i_pose][0]
        assert ref["scan"][sc["blocks"][block]["pl"][r]] == 1 + 2 * i_pose
    # found but not accepted at max_dist 1: d2 == max_d2 exactly
    assert MC.tie_winners(sc, 0, 1.0)[sc["tie_names"].index("at_max_dist")] == -1
    assert MC.tie_winners(sc, 0, 1.3)[sc["tie_names"].index("at_max_dist")] == 0
    # the filler is matched at both poses
    for i_pose in (0, 1):
        ref = oracle_match(oracle, "ties")[i_pose][0]
        f = sc["blocks"]["filler"]["pl"]
        assert (ref["found"][f] & (ref["d2"][f] < 1.0)).sum() > 100000


def test_dense_scene_has_dense_cells_and_queries_in_them(oracle):
    sc = MC.scene("dense")
    w = sc["w"]
    cells, cnt = MC.world_cell_counts(sc)
    assert (cnt >= MC.DENSE_MIN).sum() >= 20
    assert (cnt > MC.UNSORTED_MIN).sum() == 1
    dense = {tuple(c) for c in cells[cnt >= MC.DENSE_MIN]}
    Tj = sc["Tj"][0]
    qw = sc["q_pl"][:, :3].astype(np.float64) @ Tj[:, :3].T + Tj[:, 3]
    own = np.array([tuple(c) in dense for c in np.floor(qw[sc["blocks"]["dense"]["pl"]] / w).astype(np.int64)])
    assert own.sum() >= 2000
    assert len(sc["blocks"]["dense"]["pl"]) + len(sc["blocks"]["dense"]["pt"]) <= 8000
    # the filler lies in sparse cells only
    fq = np.floor(qw[sc["blocks"]["filler"]["pl"]] / w).astype(np.int64)
    assert not any(tuple(c) in dense for c in np.unique(fq, axis=0))
    (rpl, rpt), = oracle_match(oracle, "dense")
    acc_pl = rpl["found"] & (rpl["d2"] < w * w)
    acc_pt = rpt["found"] & (rpt["d2"] < w * w)
    print(f"dense: {(cnt >= MC.DENSE_MIN).sum()} dense cells, largest {cnt.max()}, {own.sum()} queries in dense own "
          f"cells; accepted planar {acc_pl.sum()} {np.bincount(rpl['scan'][acc_pl].astype(np.int64)).tolist()}, "
          f"point {acc_pt.sum()} {np.bincount(rpt['scan'][acc_pt].astype(np.int64)).tolist()}")
    assert acc_pl.sum() > 100000 and acc_pt.sum() > 10000
    # the edge block is the dense fixture (same seed and draws as tests/test_gpu_map.py's), unchanged by the filler
    scans, poses, qpl, qpt = MC.dense_fixture()
    assert np.array_equal(sc["q_pl"][sc["blocks"]["dense"]["pl"]], qpl)
    assert np.array_equal(sc["q_pt"][sc["blocks"]["dense"]["pt"]], qpt)
    assert all(np.array_equal(sc["scans"][k][0][:len(scans[k][0])], scans[k][0]) for k in range(6))

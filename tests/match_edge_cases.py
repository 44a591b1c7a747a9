"""Scenes that send the search edge cases of tests/test_gpu_map.py through the one-lane
build of the match (fmx::gl: 131072 queries and more, form_amd/csrc/pair_sort_plan.hpp) and
its fused linearization.  numpy only, fixed seeds; tests/test_match_edges_cpu.py checks on
the CPU oracle that every scene realizes its design, tests/test_gpu_match_onelane.py runs
them on the device.

A scene is a dict:
  scans   [(planar (n, 6) float32, point (n, 3) float32)] per map scan, in the scan's frame
  poses   (K, 3, 4) float64, scan k is scan id k
  w       voxel width
  q_pl, q_pt   the queries, (N_QPL, 6) and (N_QPT, 3) float32
  Tj      list of query poses (3, 4) float64
  blocks  {name: {"pl": indices into q_pl, "pt": indices into q_pt}}: which queries belong
          to which edge block ("filler" is the rest)
`ties` adds tie_names and, per query pose, the designed pair of every tie query
(tie_winners()).

Most queries are filler in a sparse random cloud.  The edge blocks are small and interleaved
into the query arrays at a fixed stride, so that they share waves (and blocks) with lanes
doing other work.  N_QPL + N_QPT >= 131072; neither count is a multiple of the 256 queries
of a match block, so both types end in a partial block, and the 469 + 67 = 536 blocks are no
multiple of the 64 blocks of a first-level reduction group of the fused kernel.
"""
import numpy as np

from scenario import perturb

N_QPL, N_QPT = 120001, 17003
LARGE_MIN = 128 * 1024  # kMatchLargeMin
BLOCK, FZ_GROUP = 256, 64  # queries per one-lane match block, blocks per reduction group
DENSE_MIN = 128  # FMX_DENSE_MIN: records from which a cell is dense
UNSORTED_MIN = 8192  # a dense cell above this is left unsorted
FAR = np.array([-81920.0, 40960.0, -1638.4])  # cells ~ -1e5 (0.8 m): well inside |c| < 2^19 - 2
FAR_Z = 0.375  # see _tie_scene
TIE_STRIDE = 997
W = 0.8

I34 = np.hstack([np.eye(3), np.zeros((3, 1))])

SCENES = ("plain", "plain_far", "ties", "dense")


def planar(xyz, rng=None):
    """(n, 6) float32 planar features: normal +z, or random unit normals."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if rng is None:
        n = np.tile(np.array([0, 0, 1], np.float32), (len(xyz), 1))
    else:
        n = rng.normal(size=(len(xyz), 3))
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(np.hstack([xyz, n]).astype(np.float32))


def to_local(T, world):
    """T^-1 applied to world points (fp64)."""
    return (np.asarray(world, np.float64) - T[:, 3]) @ T[:, :3]


def translated(T, t):
    out = np.array(T, np.float64)
    out[:, 3] += t
    return out


def interleave(filler, edge, stride, start=5):
    """edge[i] at index start + i * stride of the result, filler in order around it.
    Returns (array, indices of the edge rows)."""
    n = len(filler) + len(edge)
    at = start + stride * np.arange(len(edge))
    assert len(edge) == 0 or at[-1] < n
    out = np.empty((n,) + filler.shape[1:], filler.dtype)
    mask = np.zeros(n, bool)
    mask[at] = True
    out[at] = edge
    out[~mask] = filler
    return out, at


def _uniform(rng, box, n):
    lo, hi = np.asarray(box, np.float64).T
    return rng.uniform(lo, hi, (n, 3))


def _blocks(n_pl, n_pt, named):
    """named: {name: (planar indices, point indices)}; adds "filler"."""
    rest_pl, rest_pt = np.ones(n_pl, bool), np.ones(n_pt, bool)
    out = {}
    for k, (a, b) in named.items():
        rest_pl[a] = False
        rest_pt[b] = False
        out[k] = {"pl": np.asarray(a, np.int64), "pt": np.asarray(b, np.int64)}
    out["filler"] = {"pl": np.nonzero(rest_pl)[0], "pt": np.nonzero(rest_pt)[0]}
    return out


# ------------------------------------------------------------------------------- plain
PLAIN_BOX = [(-16, 16), (-16, 16), (-5, 5)]  # 20000 cells of 0.8 m
PLAIN_NPL, PLAIN_NPT = 40000, 14000  # ~2 planar and 0.7 point records per cell


def _plain_scene(far):
    rng = np.random.default_rng(101)
    K = 4
    poses = np.stack([perturb(I34, rng, 0.3, 1.0) for _ in range(K)])
    wpl, wpt = _uniform(rng, PLAIN_BOX, PLAIN_NPL), _uniform(rng, PLAIN_BOX, PLAIN_NPT)
    of_pl, of_pt = rng.integers(0, K, PLAIN_NPL), rng.integers(0, K, PLAIN_NPT)
    scans = []
    for k in range(K):
        scans.append((planar(to_local(poses[k], wpl[of_pl == k]), rng),
                      np.ascontiguousarray(to_local(poses[k], wpt[of_pt == k]), np.float32)))
    Tj = perturb(I34, rng, 0.2, 0.5)
    q_pl = planar(to_local(Tj, _uniform(rng, PLAIN_BOX, N_QPL)), rng)
    q_pt = np.ascontiguousarray(to_local(Tj, _uniform(rng, PLAIN_BOX, N_QPT)), np.float32)
    if far:  # the same local coordinates, every pose carried far away
        poses = np.stack([translated(T, FAR) for T in poses])
        Tj = translated(Tj, FAR)
    return dict(scans=scans, poses=poses, w=W, q_pl=q_pl, q_pt=q_pt, Tj=[Tj], blocks=_blocks(N_QPL, N_QPT, {}))


# -------------------------------------------------------------------------------- ties
def tie_cases():
    """(name, scan 0 records, scan 1 records, query, winner, d2) per region, w = 1: the
    nearest record's scan and squared distance.  Every coordinate is exact in fp32 and
    every distance exact in fp64.  Build order puts scan 0 first; rank is the position
    of the record's cell in the reference's fixed order of 27 shifts."""
    c = (0.5, 0.5, 0.5)
    return [
        # --- the six regions of tests/test_gpu_map.py::_tie_cases
        # faces +x (rank 1) vs -x (rank 2): the reference takes +x, which is in scan 1
        ("face_x", [(-0.25, 0.5, 0.5)], [(1.25, 0.5, 0.5)], c, 1, 0.5625),
        # own voxel (rank 0, scan 1) vs the +z face (rank 5, scan 0)
        ("own_vs_face_z", [(0.5, 0.5, 1.125)], [(0.5, 0.5, 0.625)], (0.5, 0.5, 0.875), 1, 0.0625),
        # edges (1, 1, 0) (rank 7, scan 1) vs (-1, -1, 0) (rank 10, scan 0)
        ("edge_xy", [(-0.25, -0.25, 0.5)], [(1.25, 1.25, 0.5)], c, 1, 1.125),
        # corners (1, 1, 1) (rank 19, scan 1) vs (-1, -1, -1) (rank 26, scan 0)
        ("corner", [(-0.25, -0.25, -0.25)], [(1.25, 1.25, 1.25)], c, 1, 1.6875),
        # one voxel, two scans: insertion order (scan 0 first)
        ("same_voxel", [(0.75, 0.5, 0.5)], [(0.25, 0.5, 0.5)], c, 0, 0.0625),
        # the face -y (rank 4, scan 1) vs the edge (1, 1, 0) (rank 7, scan 0), both at 1.25
        ("face_vs_edge", [(1.25, 1.5, 0.5)], [(0.5, -0.75, 0.5)], c, 1, 1.5625),
        # --- off centre: the nearer cell holds the record of the later shift
        # -x (rank 2, 0.25 away) vs +x (rank 1, 0.75 away), records both at 0.75; the +x
        # record lies exactly on the face it shares with the query's cell
        ("off_face", [(-0.5, 0.5, 0.5)], [(1.0, 0.5, 0.5)], (0.25, 0.5, 0.5), 1, 0.5625),
        # (-1, -1, 0) (rank 10, nearer) vs (1, 1, 0) (rank 7)
        ("off_edge", [(-0.25, -0.25, 0.5)], [(1.0, 1.0, 0.5)], (0.375, 0.375, 0.5), 1, 0.78125),
        # (-1, -1, -1) (rank 26, nearer) vs (1, 1, 1) (rank 19)
        ("off_corner", [(-0.125, -0.125, -0.0625)], [(1.0, 1.0, 1.0625)], (0.4375, 0.4375, 0.5), 1, 0.94921875),
        # --- queries exactly on cell boundaries (floor puts them in the upper cell)
        # on the face x = 2: own cell [2, 3) (rank 0, scan 1) vs -x (rank 2, scan 0)
        ("on_face", [(1.5, 0.5, 0.5)], [(2.5, 0.5, 0.5)], (2.0, 0.5, 0.5), 1, 0.25),
        # on the face x = -3: own cell [-3, -2) (scan 0) vs -x (scan 1)
        ("on_face_neg", [(-2.5, 0.5, 0.5)], [(-3.5, 0.5, 0.5)], (-3.0, 0.5, 0.5), 0, 0.25),
        # on the edge x = 2, y = -1 (cell (2, -1, 0)): -x (rank 2, scan 1) vs -y (rank 4, scan 0)
        ("on_edge", [(2.5, -1.5, 0.5)], [(1.5, -0.5, 0.5)], (2.0, -1.0, 0.5), 1, 0.5),
        # on the corner (-2, 3, 1): own cell (scan 1) vs (-1, -1, -1) (rank 26, scan 0); carried
        # far the query lies inside its cell in z, scan 1's record is then in +z (rank 5) and
        # scan 0's in (-1, -1, 0) (rank 10)
        ("on_corner", [(-2.5, 2.5, 0.5)], [(-1.5, 3.5, 1.5)], (-2.0, 3.0, 1.0), 1, 0.75),
        # a record on the lower face of the query's own cell (own cell, scan 0) and one on
        # the upper face (the +x cell, scan 1)
        ("rec_on_faces", [(0.0, 0.5, 0.5)], [(1.0, 0.5, 0.5)], c, 0, 0.25),
        # the only record at exactly max_dist = 1: found, not accepted (best < max_d2 is strict)
        ("at_max_dist", [(1.5, 0.5, 0.5)], [], c, 0, 1.0),
    ]


TIE_PITCH = 8.0  # regions lie this far apart along x: no region sees another
TIE_FAR_OFF = np.array([0.0, 8.0, FAR_Z])
TIES_BOX = [(0, 32), (16, 48), (-5, 5)]  # the filler cloud, clear of the tie regions


def tie_winners(scene, i_pose, max_dist):
    """The designed pair of every tie query (order of scene["blocks"]["ties_origin"], then
    "ties_far") in a match at scene["Tj"][i_pose]: -1 where the nearest record is not
    nearer than max_dist, and for the copy that this pose leaves without records."""
    live = [(-1 if d2 >= max_dist * max_dist else win) for (_, _, _, _, win, d2) in tie_cases()]
    dead = [-1] * len(live)
    return (live + dead) if i_pose == 0 else (dead + [(-1 if p < 0 else p + 2) for p in live])


def _tie_scene():
    """The tie block twice in one map of four scans.  Scans 0 and 1 (identity poses) hold
    it at the origin, queried at Tj[0] = identity.  Scans 2 and 3, posed at the far
    translation with identity rotation, hold it again (scan 2 as scan 0, scan 3 as scan 1),
    queried at Tj[1] = the far translation by a second copy of the tie queries.  That copy
    (records and queries) lies 8 m along y, and FAR_Z = 0.375 up: the far translation's
    z = -1638.4 is no whole number of cells, so the cell faces of the far copy lie at design
    z = 0.025 (mod 1) instead of 0, which no record or query of the block lies between:
    every record keeps its shift, except where a case sits on a z boundary (on_corner).
    At each pose the other copy's queries find no record at all."""
    rng = np.random.default_rng(103)
    cases = tie_cases()
    s = [[], [], [], []]
    q = [[], []]
    for r, (_, a, b, qq, _, _) in enumerate(cases):
        off = np.array([TIE_PITCH * r, 0.0, 0.0])
        s[0] += [np.add(p, off) for p in a]
        s[1] += [np.add(p, off) for p in b]
        s[2] += [np.add(p, off + TIE_FAR_OFF) for p in a]
        s[3] += [np.add(p, off + TIE_FAR_OFF) for p in b]
        q[0].append(np.add(qq, off))
        q[1].append(np.add(qq, off + TIE_FAR_OFF))
    scans = []
    n_fpl, n_fpt = PLAIN_NPL // 4, PLAIN_NPT // 4
    for k in range(4):
        fill_pl, fill_pt = _uniform(rng, TIES_BOX, n_fpl), _uniform(rng, TIES_BOX, n_fpt)
        scans.append((np.vstack([planar(s[k]), planar(fill_pl, rng)]),
                      np.ascontiguousarray(np.vstack([np.asarray(s[k]).reshape(-1, 3), fill_pt]), np.float32)))
    poses = np.stack([I34, I34, translated(I34, FAR), translated(I34, FAR)])
    tq = np.vstack(q[0] + q[1])
    n_t = len(tq)
    q_pl, at_pl = interleave(planar(_uniform(rng, TIES_BOX, N_QPL - n_t), rng), planar(tq), TIE_STRIDE)
    q_pt, at_pt = interleave(np.ascontiguousarray(_uniform(rng, TIES_BOX, N_QPT - n_t), np.float32),
                             np.asarray(tq, np.float32), 2 * 251)
    h = n_t // 2
    blocks = _blocks(N_QPL, N_QPT, {"ties_origin": (at_pl[:h], at_pt[:h]), "ties_far": (at_pl[h:], at_pt[h:])})
    return dict(scans=scans, poses=poses, w=1.0, q_pl=q_pl, q_pt=q_pt, Tj=[I34.copy(), translated(I34, FAR)],
                blocks=blocks, tie_names=[c[0] for c in cases])


def tie_block_alone(scene):
    """The tie queries of both copies alone (a small set: the eight-lane build) and their
    indices in the scene's query arrays."""
    ipl = np.concatenate([scene["blocks"]["ties_origin"]["pl"], scene["blocks"]["ties_far"]["pl"]])
    ipt = np.concatenate([scene["blocks"]["ties_origin"]["pt"], scene["blocks"]["ties_far"]["pt"]])
    return scene["q_pl"][ipl], scene["q_pt"][ipt], ipl, ipt


# ------------------------------------------------------------------------------- dense
def dense_fixture():
    """The fixture of tests/test_gpu_map.py::test_dense_cells_match_oracle (same seed, same
    draws in the same order: the same arrays, which that test runs on the eight-lane build):
    clusters of ~1900 records per 0.8 m cell around the origin (sorted into sub-cells),
    a thin strip of dense cells, one cell with 9000 records of scan 2 (> 8192: left
    unsorted), and queries in and around them.  Returns scans, poses, qpl, qpt."""
    rng = np.random.default_rng(11)
    scans, poses = [], []
    for k in range(6):
        c = rng.uniform(-0.8, 0.8, (2500, 3))
        flat = np.c_[rng.uniform(2, 6, 1500), rng.uniform(-1, 1, 1500), rng.normal(0, 0.01, 1500) - 1.5]
        pl = np.vstack([c, flat])
        if k == 2:
            pl = np.vstack([pl, np.c_[rng.uniform(3.25, 3.95, 9000), rng.uniform(4.05, 4.75, (9000, 2))]])
        pt = rng.uniform(-0.8, 0.8, (600, 3))
        T = I34.copy()
        T[:, 3] = rng.normal(0, 0.01, 3)
        poses.append(T)
        scans.append((planar(pl, rng), np.asarray(pt, np.float32)))
    qpl = planar(np.vstack([rng.uniform(-1.2, 1.2, (3000, 3)),
                            np.c_[rng.uniform(2, 6, 1000), rng.uniform(-1, 1, 1000), np.full(1000, -1.45)],
                            np.c_[rng.uniform(3.1, 4.1, 1000), rng.uniform(3.9, 4.9, (1000, 2))]]), rng)
    qpt = np.asarray(rng.uniform(-1.2, 1.2, (1500, 3)), np.float32)
    return scans, poses, qpl, qpt


DENSE_TJ = (0.003, -0.002, 0.001)
DENSE_BOX = [(10, 42), (-16, 16), (-5, 5)]  # the filler cloud, clear of the dense cells


def _dense_scene():
    scans, poses, eq_pl, eq_pt = dense_fixture()
    rng = np.random.default_rng(107)
    K = len(scans)
    wpl, wpt = _uniform(rng, DENSE_BOX, PLAIN_NPL), _uniform(rng, DENSE_BOX, PLAIN_NPT)
    of_pl, of_pt = rng.integers(0, K, PLAIN_NPL), rng.integers(0, K, PLAIN_NPT)
    for k in range(K):
        pl, pt = scans[k]
        scans[k] = (np.vstack([pl, planar(to_local(poses[k], wpl[of_pl == k]), rng)]),
                    np.ascontiguousarray(np.vstack([pt, to_local(poses[k], wpt[of_pt == k])]), np.float32))
    Tj = translated(I34, DENSE_TJ)
    q_pl, at_pl = interleave(planar(to_local(Tj, _uniform(rng, DENSE_BOX, N_QPL - len(eq_pl))), rng), eq_pl, 23)
    q_pt, at_pt = interleave(np.ascontiguousarray(to_local(Tj, _uniform(rng, DENSE_BOX, N_QPT - len(eq_pt))),
                                                  np.float32), eq_pt, 11)
    return dict(scans=scans, poses=np.stack(poses), w=W, q_pl=q_pl, q_pt=q_pt, Tj=[Tj],
                blocks=_blocks(N_QPL, N_QPT, {"dense": (at_pl, at_pt)}))


_BUILT = {}


def scene(name):
    """Built once and shared: never modify what this returns."""
    if name not in _BUILT:
        _BUILT[name] = {"plain": lambda: _plain_scene(False), "plain_far": lambda: _plain_scene(True),
                        "ties": _tie_scene, "dense": _dense_scene}[name]()
    return _BUILT[name]


_OMAPS, _OREF = {}, {}


def oracle_match(oracle, name, Tj):
    """(planar ref, point ref): the oracle VoxelMap's match of the scene's queries at Tj.
    The maps and every pose's result are computed once and shared: never modify them."""
    sc = scene(name)
    if name not in _OMAPS:
        omaps = [oracle.VoxelMap(sc["w"], 0), oracle.VoxelMap(sc["w"], 1)]
        for k, (pl, pt) in enumerate(sc["scans"]):
            omaps[0].add_scan(k, sc["poses"][k], pl)
            omaps[1].add_scan(k, sc["poses"][k], pt)
        _OMAPS[name] = omaps
    key = (name, np.ascontiguousarray(Tj, np.float64).tobytes())
    if key not in _OREF:
        _OREF[key] = (_OMAPS[name][0].match(sc["q_pl"], Tj), _OMAPS[name][1].match(sc["q_pt"], Tj))
    return _OREF[key]


def world_cell_counts(sc, kind=0):
    """(cells (m, 3) int64, records per cell) of the scene's map in fp64."""
    wp = np.vstack([f[kind][:, :3].astype(np.float64) @ sc["poses"][k][:, :3].T + sc["poses"][k][:, 3]
                    for k, f in enumerate(sc["scans"])])
    return np.unique(np.floor(wp / sc["w"]).astype(np.int64), axis=0, return_counts=True)


def describe(sc, i_pl=None, i_pt=None):
    """Which edge block a failing query index belongs to (for assertion messages)."""
    out = []
    for name, b in sc["blocks"].items():
        if i_pl is not None and i_pl in b["pl"]:
            out.append((name, "pl", int(np.nonzero(b["pl"] == i_pl)[0][0])))
        if i_pt is not None and i_pt in b["pt"]:
            out.append((name, "pt", int(np.nonzero(b["pt"] == i_pt)[0][0])))
    return out

"""Record conservation of the voxel map build (voxelmap.hip: k_map_insert / count / alloc /
scatter / dense), proved from outside: every record of a built map is queried with itself.
Scan k's own features, matched at scan k's build pose, must each come back as a match of
pair k at distance 0 that carries the record's own position and normal.  A record that the
build dropped, overwrote or stored with another record's normal shows as a distance of at
least the record separation, or as the wrong position or normal; a match test over sampled
queries near surviving records cannot see one.

Run on the lattice scenes of tests/map_lattice_cases.py (every path of the search) and on
build shapes at the build's own thresholds: record counts around the wave, block and
allocation-block sizes, absent / one-type / empty scans in the build list, a build of no
records, cells of exactly 128 / 129 / 8192 / 8193 records, a brick with plain, dense and
empty cells, a planar section whose header slots reach the point section exactly, and the
smallest build that takes the interleaved record layout.  The small shapes are also
compared with the oracle's VoxelMap on a few hundred perturbed queries."""
import numpy as np
import pytest

import map_lattice_cases as ML
from match_edge_cases import I34, planar, to_local
from scenario import perturb

pytestmark = pytest.mark.gpu

W = 0.8
EPS = 2.0 ** -52
DENSE_MIN, HDR = 128, 8  # records above which a cell is dense; header slots of a dense cell
CHUNK = 1 << 20


def _world(T, local):
    return np.asarray(local, np.float64) @ T[:, :3].T + T[:, 3]


def check_complete(ctx, scans, poses, w, exact=False, label=""):
    """Every record of the map built from `scans` (one (planar, point) per build-list entry,
    None for a scan that is not in the pool) at `poses` queried with itself.  d2 is bounded by
    the rounding of d_xform's three products and sums, which the build and the match both
    evaluate: (16 * 2^-52 * c)^2 with c the largest |world coordinate| plus |t|; exact: 0.
    Returns the number of records queried."""
    K = len(scans)
    total = 0
    for k, feats in enumerate(scans):
        if feats is None:
            continue
        pl, pt = feats
        n_rec = (len(pl), len(pt))
        if n_rec == (0, 0):
            continue
        T = np.asarray(poses[k], np.float64)
        c = max([np.abs(_world(T, f[:, :3])).max() for f in (pl, pt) if len(f)]) + np.abs(T[:, 3]).max()
        bound = 0.0 if exact else (16 * EPS * c) ** 2
        for o in range(0, max(n_rec), CHUNK):
            qpl, qpt = pl[o:o + CHUNK], pt[o:o + CHUNK]
            ctx.set_queries(qpl, qpt, 1 << 20)
            cpl, cpt = ctx.match(T, w)
            got = ctx.match_download()
            for t, q, cnt, sl in (("planar", qpl, cpl, slice(0, len(qpl))), ("point", qpt, cpt, slice(len(qpl), None))):
                where = (label, "scan", k, t, "from", o)
                pair, d2, pi = got["pair"][sl], got["d2"][sl], got["pi"][sl]
                bad = pair != k
                assert not bad.any(), (where, "pair", int(bad.sum()), np.nonzero(bad)[0][:4] + o, pair[bad][:4], d2[bad][:4])
                bad = ~(d2 <= bound)
                assert not bad.any(), (where, "d2", int(bad.sum()), np.nonzero(bad)[0][:4] + o, d2[bad][:4], bound)
                bad = ~(np.abs(pi - q[:, :3].astype(np.float64)) <= 1e-9).all(1)
                assert not bad.any(), (where, "pi", int(bad.sum()), np.nonzero(bad)[0][:4] + o)
                if t == "planar":
                    bad = ~(np.abs(got["ni"] - q[:, 3:].astype(np.float64)) <= 1e-9).all(1)
                    assert not bad.any(), (where, "ni", int(bad.sum()), np.nonzero(bad)[0][:4] + o)
                want = np.zeros(K, np.int64)
                want[k] = len(q)
                assert np.array_equal(cnt, want), (where, "counts", cnt, want)
            total += len(qpl) + len(qpt)
    return total


def _oracle_check(ctx, oracle, scans, poses, w, seed, n_q=300):
    """The bit-exact match contract (tests/test_gpu_mapbuild.py::_check) on up to n_q
    perturbed records per type, queried at a perturbed pose."""
    rng = np.random.default_rng(seed)
    K = len(scans)
    omaps = [oracle.VoxelMap(w, 0), oracle.VoxelMap(w, 1)]
    wp = [[], []]
    for k, feats in enumerate(scans):
        if feats is None:
            continue
        for t in (0, 1):
            omaps[t].add_scan(k, poses[k], feats[t])
            wp[t].append(_world(poses[k], feats[t][:, :3]))
    Tj = perturb(I34, rng, 0.01, 0.05)
    Q = []
    for t in (0, 1):
        pts = np.vstack(wp[t] + [np.zeros((0, 3))])
        pts = pts[rng.choice(len(pts), min(n_q, len(pts)), replace=False)] + rng.normal(0, 0.05, (min(n_q, len(pts)), 3))
        loc = to_local(Tj, pts)
        Q.append(planar(loc, rng) if t == 0 else np.ascontiguousarray(loc, np.float32))
    ctx.set_queries(Q[0], Q[1], 1 << 20)
    cpl, cpt = ctx.match(Tj, w)
    got = ctx.match_download()
    npl = len(Q[0])
    for t in (0, 1):
        ref = omaps[t].match(Q[t], Tj)
        sl = slice(0, npl) if t == 0 else slice(npl, None)
        acc = ref["found"] & (ref["d2"] < w * w)
        pair = got["pair"][sl]
        assert np.array_equal(pair >= 0, acc)
        assert np.array_equal(pair[acc].astype(np.uint64), ref["scan"][acc])
        assert np.array_equal(got["d2"][sl][acc], ref["d2"][acc])
        assert np.array_equal(got["pi"][sl][acc], ref["pi"][acc])
        if t == 0:
            assert np.array_equal(got["ni"][acc], ref["ni"][acc])
        assert np.array_equal(cpl if t == 0 else cpt, np.bincount(ref["scan"][acc].astype(np.int64), minlength=K))
    return int(acc.sum())


def _ctx(fmx, subdiv=1, capacity=None):
    kw = {} if capacity is None else dict(keypoint_pool_capacity=capacity)
    return fmx.Context(fmx.EstimatorParams(voxel_subdivision=subdiv, **kw))


def _build(ctx, ids, scans, poses, w, add=True):
    if add:
        for i, feats in zip(ids, scans):
            if feats is not None:
                ctx.keypoints_add(i, feats[0], feats[1])
    ctx.map_build(list(ids), np.stack(poses), w)


def _in_cell(rng, cell, n, w=W, margin=0.01):
    """n points inside the cell, `margin` clear of its faces."""
    return (np.asarray(cell, np.float64) + rng.uniform(margin / w, 1 - margin / w, (n, 3))) * w


def _cells(xyz, w=W):
    return np.floor(np.asarray(xyz, np.float64) / w).astype(np.int64)


def _sparse(rng, n, avoid, box=3.0, w=W):
    """~n points in (-box, box)^3 outside the cells of `avoid` ((m, 3) cell indices)."""
    p = rng.uniform(-box, box, (n, 3)).astype(np.float32)
    c = _cells(p, w)
    keep = ~(c[:, None, :] == np.asarray(avoid)[None]).all(2).any(1)
    return p[keep]


def _feats(rng, xyz_pl, xyz_pt):
    return (planar(np.asarray(xyz_pl, np.float32).reshape(-1, 3), rng),
            np.ascontiguousarray(np.asarray(xyz_pt, np.float32).reshape(-1, 3)))


def _count_in(xyz, cell, w=W):
    return int((_cells(xyz, w) == np.asarray(cell)).all(1).sum())


# --------------------------------------------------------------------- the lattice scenes
@pytest.mark.parametrize("name", ML.SCENES)
def test_lattice_scene_is_complete(fmx_mod, name):
    sc = ML.scene(name)
    ctx = _ctx(fmx_mod, sc["subdiv"])
    _build(ctx, range(ML.K), sc["scans"], sc["poses"], sc["w"])
    n = check_complete(ctx, sc["scans"], sc["poses"], sc["w"], exact=True, label=(name, sc["cls"]))
    assert n == len(sc["rec"]["pl"]["iw"]) + len(sc["rec"]["pt"]["iw"])
    ctx.close()


# ------------------------------------------------------------- 1. record-count boundaries
COUNTS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)  # wave, insert / count block, allocation block of 1024 * 4


@pytest.mark.parametrize("mode", ["planar", "point", "split"])
def test_record_count_boundaries(fmx_mod, oracle, mode):
    """One scan of N records at an off-identity pose, rebuilt on one context for every N.
    split: 10 planar records, then the point records, the first of which lie in the planar
    records' bricks: the wave that holds both types holds them in one brick, told apart
    only by the type bit of the grouping key."""
    rng = np.random.default_rng(71)
    ctx = _ctx(fmx_mod)
    T = perturb(I34, rng, 0.2, 0.7)
    for i, N in enumerate(COUNTS):
        n_pl = {"planar": N, "point": 0, "split": min(10, N)}[mode]
        wpl = rng.uniform(-6, 6, (n_pl, 3))
        wpt = rng.uniform(-6, 6, (N - n_pl, 3))
        if mode == "split" and N > n_pl:
            m = min(n_pl, N - n_pl)
            centre = (np.floor(wpl[:m] / (2 * W)) + 0.5) * (2 * W)  # towards the brick's centre: the same brick
            wpt[:m] = wpl[:m] + 0.25 * (centre - wpl[:m])
        feats = _feats(rng, to_local(T, wpl), to_local(T, wpt))
        if mode == "split" and N > n_pl:
            bpl, bpt = _cells(_world(T, feats[0][:m, :3])) >> 1, _cells(_world(T, feats[1][:m])) >> 1
            assert np.array_equal(bpl, bpt)  # (fp32 rounding did not move them out)
        _build(ctx, [i], [feats], [T], W)
        assert check_complete(ctx, [feats], [T], W, label=(mode, N)) == N
        _oracle_check(ctx, oracle, [feats], [T], W, seed=N)
    ctx.close()


# ---------------------------------------------------------- 2. empty and partial segments
def test_absent_one_type_and_empty_scans(fmx_mod, oracle):
    """A build list of six scan ids: the first and the last were never added, one scan is
    planar only, one point only, one was added with no features, one has both."""
    rng = np.random.default_rng(73)
    poses = [perturb(I34, rng, 0.2, 0.7) for _ in range(6)]
    none_pl, none_pt = np.zeros((0, 6), np.float32), np.zeros((0, 3), np.float32)
    scans = [None,
             (planar(rng.uniform(-4, 4, (700, 3)), rng), none_pt),
             (none_pl, rng.uniform(-4, 4, (333, 3)).astype(np.float32)),
             (none_pl, none_pt),
             _feats(rng, rng.uniform(-4, 4, (513, 3)), rng.uniform(-4, 4, (129, 3))),
             None]
    ctx = _ctx(fmx_mod)
    _build(ctx, range(10, 16), scans, poses, W)
    assert check_complete(ctx, scans, poses, W) == 700 + 333 + 513 + 129
    assert _oracle_check(ctx, oracle, scans, poses, W, seed=1) > 50
    ctx.close()


# ------------------------------------------------------------------- 3. all-absent list
def test_build_of_no_records_then_rebuild(fmx_mod, oracle):
    """A map with a dense cell, then a build whose list holds only absent scans (no
    records: no match at all), then the first map again on the same context."""
    rng = np.random.default_rng(79)
    T = perturb(I34, rng, 0.2, 0.7)
    wpl = np.vstack([_in_cell(rng, (1, 0, -1), 300), rng.uniform(-4, 4, (1500, 3))])
    feats = _feats(rng, to_local(T, wpl), to_local(T, rng.uniform(-4, 4, (400, 3))))
    ctx = _ctx(fmx_mod)
    _build(ctx, [0], [feats], [T], W)
    assert check_complete(ctx, [feats], [T], W) == 2200
    ctx.map_build([7, 8], np.stack([T, I34]), W)
    ctx.set_queries(feats[0], feats[1], 1 << 20)
    cpl, cpt = ctx.match(T, W)
    got = ctx.match_download()
    assert (got["pair"] == -1).all()
    assert not cpl.any() and not cpt.any() and len(cpl) == len(cpt) == 2
    _build(ctx, [0], [feats], [T], W, add=False)
    assert check_complete(ctx, [feats], [T], W) == 2200
    _oracle_check(ctx, oracle, [feats], [T], W, seed=2)
    ctx.close()


# ------------------------------------------------------------ 4. cell-count thresholds
@pytest.mark.parametrize("n_big", [128, 129, 8192, 8193])
def test_cell_count_thresholds(fmx_mod, oracle, n_big):
    """One cell of exactly n_big records of each type (129: the first dense count, 8193: the
    first left unsorted), sparse cells around it."""
    rng = np.random.default_rng(n_big)
    cell = (0, 0, 0)
    feats = _feats(rng, np.vstack([_in_cell(rng, cell, n_big), _sparse(rng, 2000, [cell])]),
                   np.vstack([_in_cell(rng, cell, n_big), _sparse(rng, 1000, [cell])]))
    assert _count_in(feats[0][:, :3], cell) == n_big == _count_in(feats[1], cell)  # identity pose: world = local
    ctx = _ctx(fmx_mod)
    _build(ctx, [0], [feats], [I34], W)
    assert check_complete(ctx, [feats], [I34], W, label=n_big) == len(feats[0]) + len(feats[1])
    _oracle_check(ctx, oracle, [feats], [I34], W, seed=3)
    ctx.close()


# ------------------------------------------------------------------------ 5. mixed brick
BRICK_COUNTS = (129, 1, 0, 200, 128, 130, 0, 300)  # cell x | y << 1 | z << 2 of brick (0, 0, 0)


def test_brick_of_plain_dense_and_empty_cells(fmx_mod, oracle):
    rng = np.random.default_rng(83)
    cells = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]
    scans = []
    for k in range(2):  # two scans with the same counts: every cell twice as full, split over the scans at random
        xyz = [np.vstack([_in_cell(rng, cells[c], n) for c, n in enumerate(BRICK_COUNTS)] + [_sparse(rng, 800, cells)])
               for _ in range(2)]
        scans.append(_feats(rng, xyz[0][rng.permutation(len(xyz[0]))], xyz[1]))
    # one scan alone: the counts as stated; both scans: 258 2 0 400 256 260 0 600
    for use in ([0], [0, 1]):
        feats = [scans[k] for k in use]
        for t in (0, 1):
            allp = np.vstack([f[t][:, :3] for f in feats])
            assert [_count_in(allp, c) for c in cells] == [len(use) * n for n in BRICK_COUNTS]
        ctx = _ctx(fmx_mod)
        _build(ctx, use, feats, [I34] * len(use), W)
        assert check_complete(ctx, feats, [I34] * len(use), W, label=use) == sum(len(f[0]) + len(f[1]) for f in feats)
        _oracle_check(ctx, oracle, feats, [I34] * len(use), W, seed=4)
        ctx.close()


# ----------------------------------------------------------------- 6. full header region
def test_planar_headers_fill_their_section_exactly(fmx_mod, oracle):
    """50 planar cells of exactly 129 records and one of 128: 6578 planar records reserve
    6578 // 129 = 50 dense headers, and the build uses all 50, so the last planar slot is the
    one before the first point slot.  The point records, with a dense cell of their own, follow."""
    rng = np.random.default_rng(89)
    cells = [(2 * i - 7, 2 * j - 5, 3 * l - 2) for i in range(6) for j in range(5) for l in range(2)][:51]
    counts = [129] * 50 + [128]
    wpl = np.vstack([_in_cell(rng, c, n) for c, n in zip(cells, counts)])
    wpl = wpl[rng.permutation(len(wpl))]
    wpt = np.vstack([_in_cell(rng, cells[3], 200), _sparse(rng, 500, [cells[3]], box=6.0)])
    feats = _feats(rng, wpl, wpt)
    n0 = len(feats[0])
    assert n0 == 6578 and n0 // (DENSE_MIN + 1) == 50
    assert [_count_in(feats[0][:, :3], c) for c in cells] == counts
    assert _count_in(feats[1], cells[3]) == 200
    ctx = _ctx(fmx_mod)
    _build(ctx, [0], [feats], [I34], W)
    assert check_complete(ctx, [feats], [I34], W) == n0 + len(feats[1])
    _oracle_check(ctx, oracle, [feats], [I34], W, seed=5)
    ctx.close()


# --------------------------------------------------------------------- 7. interleaved layout
INTERLEAVE_MIN = 4 << 20  # kInterleaveMin: builds of this many records interleave positions and normals


def test_interleaved_layout_is_complete(fmx_mod):
    """The smallest lattice build at or above kInterleaveMin: 162^3 planar records at pitch
    0.25 m, jittered by +-0.1 (separation >= 0.05), and 10000 point records, in two scans at
    different off-identity poses; every record queried, in chunks of 2^20, after the build
    and after a rebuild on the same context."""
    rng = np.random.default_rng(97)
    side, pitch = 162, 0.25
    g = (np.arange(side) - side // 2) * pitch
    wpl = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    wpl = wpl + rng.uniform(-0.1, 0.1, wpl.shape)
    wpt = rng.uniform(-20, 20, (10000, 3))
    poses = [perturb(I34, rng, 0.3, 1.0), perturb(I34, rng, 0.3, 1.0)]
    of_pl, of_pt = rng.integers(0, 2, len(wpl)), rng.integers(0, 2, len(wpt))
    scans = []
    for k in range(2):
        loc = to_local(poses[k], wpl[of_pl == k]).astype(np.float32)
        nrm = rng.normal(size=loc.shape)
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        scans.append((np.ascontiguousarray(np.hstack([loc, nrm])),
                      np.ascontiguousarray(to_local(poses[k], wpt[of_pt == k]), np.float32)))
    n = len(wpl) + len(wpt)
    assert n >= INTERLEAVE_MIN and (side - 1) ** 3 + len(wpt) < INTERLEAVE_MIN  # the smallest such lattice
    ctx = _ctx(fmx_mod, capacity=n + 1024)
    _build(ctx, [0, 1], scans, poses, W)
    assert check_complete(ctx, scans, poses, W, label="build") == n
    _build(ctx, [0, 1], scans, poses, W, add=False)
    assert check_complete(ctx, scans, poses, W, label="rebuild") == n
    ctx.close()

"""Lattice maps for the voxel map's tie order and record conservation.  numpy only, fixed
seeds; tests/test_map_lattice_cpu.py checks on the CPU oracle that every scene realizes
its design, tests/test_gpu_map_ties.py and tests/test_gpu_map_complete.py run them on
the device.

Every record sits on a lattice h * Z^3 inside a box of whole cells around the origin, every
query on a lattice point plus (h / 2) * (a, b, c) with a, b, c in {0, 1}: a query with one,
two or three half-steps is exactly equidistant from 2, 4 or 8 records.  Every coordinate is
a whole number of UNIT = 1 / 128 m, so fp32 holds it exactly, every distance is exact in
fp64 and every tie is exact: no tolerance is involved.  The records are shuffled and dealt
at random to K = 3 scans, so build order disagrees with spatial and sub-cell order; the
scans' poses are translations by binary fractions (local = world - t, exactly).

A scene is a dict:
  name, w, subdiv, h  voxel width (0.5), voxel_subdivision of the context, finest pitch
  cls      the search path the scene is meant to take (for assertion messages)
  rpc      (lo, hi): records per internal cell (w / subdiv) of the cells meant by cls
  scans    [(planar (n, 6) float32, point (n, 3) float32)] per scan, in the scan's frame
  poses    (K, 3, 4) float64, scan k is scan id k
  rec      per type: dict(iw (n, 3) int64 world coordinates in UNITs, scan (n,), local
           (n, 3) float32, nrm (n, 3) float32 (planar)) in build order: scan, then order
           in the scan
  comps    per type: [(origin (3,), count (3,), pitch)] in UNITs: the product lattices
           whose union (minus coincident points) is the record set
  q_pl, q_pt, Tj   the tie queries (N_TIE per type) and their pose (identity)
  blocks   {name: {"pl": indices, "pt": indices}} of the aimed query blocks
"""
import numpy as np

from match_edge_cases import I34, interleave, planar

UNIT = 1.0 / 128
W = 0.5
WU = 64  # W in UNITs
K = 3
T = np.array([(0.0, 0.0, 0.0), (1.5, -2.0, 0.25), (-0.75, 0.5, 3.0)])
N_TIE = 20000
SHELL = 4  # queries up to this many lattice steps outside the box
DENSE_MIN, UNSORTED_MIN = 128, 8192
# the one-lane run: the tie queries interleaved into filler over empty space
N_QPL, N_QPT = 100001, 40007
FILL_BOX = [(100, 132), (-16, 16), (-5, 5)]

SCENES = ("walk", "sorted", "unsorted", "mixed", "sub_walk", "sub_sorted")
DENSE_SCENES = ("sorted", "unsorted", "mixed", "sub_sorted")

# the reference's fixed order of the 27 voxel shifts
SHIFTS = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
                   (1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (1, 0, 1), (1, 0, -1), (-1, 0, 1),
                   (-1, 0, -1), (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1), (1, 1, 1), (1, 1, -1),
                   (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1)])
SHIFT_RANK = np.full((3, 3, 3), -1)
SHIFT_RANK[SHIFTS[:, 0] + 1, SHIFTS[:, 1] + 1, SHIFTS[:, 2] + 1] = np.arange(27)


def _box(cells):
    """A box of `cells` whole voxels per axis around the origin: (origin, extent) in UNITs."""
    return -(cells // 2) * WU, cells * WU


def _comp(lo, ext, pitch):
    lo, ext = np.broadcast_to(lo, 3), np.broadcast_to(ext, 3)
    return (np.array(lo, np.int64), np.array(ext, np.int64) // pitch, int(pitch))


def _points(comp):
    o, n, p = comp
    g = np.stack(np.meshgrid(*[o[a] + p * np.arange(n[a]) for a in range(3)], indexing="ij"), -1)
    return g.reshape(-1, 3)


def _deal(rng, iw, with_nrm):
    """Shuffle the records and deal them at random to the K scans; build order."""
    iw = iw[rng.permutation(len(iw))]
    scan = np.sort(rng.integers(0, K, len(iw)))  # (the shuffle made the deal random)
    world = iw * UNIT
    local = (world - T[scan]).astype(np.float32)
    assert np.array_equal(local.astype(np.float64) + T[scan], world)  # local = world - t exactly
    out = dict(iw=iw, scan=scan, local=local)
    if with_nrm:
        out["nrm"] = planar(local, rng)[:, 3:]
    return out


def _queries(rng, comp, n):
    """n queries on the component's lattice, SHELL steps past it, with random half-steps."""
    o, cnt, p = comp
    idx = np.stack([rng.integers(-SHELL, cnt[a] + SHELL, n) for a in range(3)], 1)
    return o + p * idx + (p // 2) * rng.integers(0, 2, (n, 3))


def _scene(name, seed, subdiv, h_units, cls, rpc, comps_pl, comps_pt, q_of):
    rng = np.random.default_rng(seed)
    rec = {}
    for t, comps in (("pl", comps_pl), ("pt", comps_pt)):
        iw = np.unique(np.vstack([_points(c) for c in comps]), axis=0)  # a point of two lattices is one record
        rec[t] = _deal(rng, iw, t == "pl")
    scans = []
    for k in range(K):
        a, b = rec["pl"]["scan"] == k, rec["pt"]["scan"] == k
        scans.append((np.ascontiguousarray(np.hstack([rec["pl"]["local"][a], rec["pl"]["nrm"][a]])),
                      np.ascontiguousarray(rec["pt"]["local"][b])))
    poses = np.stack([np.hstack([np.eye(3), T[k][:, None]]) for k in range(K)])
    q, blocks = {}, {}
    for t in ("pl", "pt"):
        parts, at = [], 0
        for bname, comp, n in q_of(t):
            parts.append(_queries(rng, comp, n))
            blocks.setdefault(bname, {})[t] = np.arange(at, at + n)
            at += n
        assert at == N_TIE
        q[t] = (np.vstack(parts) * UNIT).astype(np.float32)
    return dict(name=name, w=W, subdiv=subdiv, h=h_units * UNIT, cls=cls, rpc=rpc, scans=scans, poses=poses,
                rec=rec, comps={"pl": comps_pl, "pt": comps_pt}, q_pl=planar(q["pl"], rng),
                q_pt=np.ascontiguousarray(q["pt"]), Tj=I34.copy(), blocks=blocks)


def _uniform_scene(name, seed, subdiv, h_units, cls, rpc, cells_pt=4):
    lo, ext = _box(4)
    cpl = [_comp(lo, ext, h_units)]
    cpt = [_comp(*_box(cells_pt), h_units)]
    return _scene(name, seed, subdiv, h_units, cls, rpc, cpl, cpt,
                  lambda t: [("lattice", (cpl if t == "pl" else cpt)[0], N_TIE)])


FINE_N, FINE_PITCH, N_FINE_Q = 21, 2, 2000  # the unsorted cell: 21^3 records at 1 / 64 m from the origin


def _unsorted_scene():
    lo, ext = _box(4)
    coarse, fine = _comp(lo, ext, 16), _comp(0, FINE_N * FINE_PITCH, FINE_PITCH)
    return _scene("unsorted", 43, 1, FINE_PITCH, "unsorted dense cell next to plain cells", (UNSORTED_MIN + 1, 10 ** 9),
                  [coarse, fine], [coarse, fine],
                  lambda t: [("lattice", coarse, N_TIE - N_FINE_Q), ("fine", fine, N_FINE_Q)])


N_SEAM_Q = 600


def _mixed_scene():
    lo, ext = _box(4)
    fine = _comp((lo, lo, lo), (ext // 2, ext, ext), 8)  # x < 0: 512 records per cell
    coarse = _comp((0, lo, lo), (ext // 2, ext, ext), 16)  # x >= 0: 64 per cell
    # the seam block: half a fine step below x = 0, y and z on the coarse lattice: one record
    # of a dense cell (x = -1 / 16) and one of a plain cell (x = 0) at exactly h / 2
    seam = (np.array([-8, lo, lo], np.int64), np.array([1, ext // 16, ext // 16], np.int64), 16)

    def q_of(t):
        n = (N_TIE - N_SEAM_Q) // 2
        return [("fine", fine, n), ("coarse", coarse, N_TIE - N_SEAM_Q - n), ("seam", seam, N_SEAM_Q)]
    sc = _scene("mixed", 47, 1, 8, "dense cells beside plain cells", (64, 512), [fine, coarse], [fine, coarse], q_of)
    rng = np.random.default_rng(48)
    for t, Q in (("pl", sc["q_pl"]), ("pt", sc["q_pt"])):  # the seam block: x = -1 / 32, y and z inside the box, no half-steps
        i = sc["blocks"]["seam"][t]
        Q[i, 0] = -4 * UNIT
        Q[i, 1:3] = (lo + 16 * rng.integers(0, ext // 16, (len(i), 2))) * UNIT
    return sc


_MAKE = {
    "walk": lambda: _uniform_scene("walk", 31, 1, 16, "group walk, no dense cell", (64, 64)),
    "sorted": lambda: _uniform_scene("sorted", 37, 1, 8, "sorted dense cells", (512, 512)),
    "unsorted": _unsorted_scene,
    "mixed": _mixed_scene,
    "sub_walk": lambda: _uniform_scene("sub_walk", 53, 2, 8, "ring 2, group walk", (64, 64)),
    "sub_sorted": lambda: _uniform_scene("sub_sorted", 59, 2, 4, "ring 2, sorted dense cells", (512, 512), cells_pt=2),
}
_BUILT, _TIES, _OREF = {}, {}, {}


def scene(name):
    """Built once and shared: never modify what this returns."""
    if name not in _BUILT:
        _BUILT[name] = _MAKE[name]()
    return _BUILT[name]


def world(sc, t):
    """fp64 world positions of the records as the map computes them: local + t."""
    r = sc["rec"][t]
    return r["local"].astype(np.float64) + T[r["scan"]]


def cell_counts(sc, t):
    """(internal cells (m, 3) int64, records per cell) in fp64."""
    cw = sc["w"] / sc["subdiv"]
    return np.unique(np.floor(world(sc, t) / cw).astype(np.int64), axis=0, return_counts=True)


def _key(iw):
    iw = np.asarray(iw, np.int64) + (1 << 19)
    return (iw[..., 0] << 40) | (iw[..., 1] << 20) | iw[..., 2]


WIN = np.arange(-2, 3)


def tie_analysis(sc, t):
    """The nearest records of every tie query by brute force over a window that provably
    holds them, and the reference's tie rule restated.

    Per product lattice, the window is the 5^3 lattice points around the one nearest the
    query (clamped into the lattice's box).  A lattice point outside the window on some axis
    is more than h farther on that axis than the point with that axis moved to the
    window's centre, which is also a record (of this lattice or, in `unsorted`, of the fine
    one that replaced it): no record outside the windows is at the minimum.

    Returns dict(dmin (N,) fp64, mult (N,), cand (N, C) record indices (-1: none), tied
    (N, C) bool, winner (N,) record index, rank (N, C) shift rank of each candidate): d2 in
    the reference's order (dx^2 + dz^2) + dy^2 from the fp64 world coordinates; winner = the
    tied record of the first of the 27 shifts, inside a voxel the first in build order."""
    key = (sc["name"], t)
    if key in _TIES:
        return _TIES[key]
    r = sc["rec"][t]
    Q = sc["q_pl" if t == "pl" else "q_pt"][:, :3].astype(np.float64)
    qi = np.rint(Q / UNIT).astype(np.int64)
    assert np.array_equal(qi * UNIT, Q)
    rkeys = _key(r["iw"])
    order = np.argsort(rkeys)
    skeys = rkeys[order]
    cands = []
    for o, cnt, p in sc["comps"][t]:
        c = np.clip(np.floor_divide(2 * (qi - o) + p, 2 * p), 0, cnt - 1)  # nearest lattice index, clamped
        idx = c[:, None, None, None, :] + np.stack(np.meshgrid(WIN, WIN, WIN, indexing="ij"), -1)[None]
        ok = ((idx >= 0) & (idx < cnt)).all(-1).reshape(len(qi), -1)
        k = _key(o + p * idx).reshape(len(qi), -1)
        pos = np.clip(np.searchsorted(skeys, k), 0, len(skeys) - 1)
        hit = ok & (skeys[pos] == k)
        cands.append(np.where(hit, order[pos], -1))
    cand = np.sort(np.hstack(cands), axis=1)
    cand[:, 1:][cand[:, 1:] == cand[:, :-1]] = -1  # a record reached through two lattices counts once
    wp = world(sc, t)
    d = wp[cand] - Q[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 2] * d[..., 2]) + d[..., 1] * d[..., 1]
    d2[cand < 0] = np.inf
    dmin = d2.min(1)
    tied = d2 == dmin[:, None]
    shift = np.floor(wp[cand] / sc["w"]).astype(np.int64) - np.floor(Q / sc["w"]).astype(np.int64)[:, None, :]
    vis = (np.abs(shift) <= 1).all(-1)
    s = np.clip(shift, -1, 1) + 1
    rank = np.where(vis, SHIFT_RANK[s[..., 0], s[..., 1], s[..., 2]], 99)
    order_key = np.where(tied, rank.astype(np.int64) << 32 | np.maximum(cand, 0), np.int64(1) << 62)
    winner = cand[np.arange(len(cand)), order_key.argmin(1)]
    out = dict(dmin=dmin, mult=tied.sum(1), cand=cand, tied=tied, winner=winner, rank=rank, visible=vis)
    _TIES[key] = out
    return out


def oracle_match(oracle, name):
    """(planar ref, point ref) of the scene's tie queries on the oracle's VoxelMap (width w,
    whatever the scene's subdivision).  Computed once and shared: never modify it."""
    if name not in _OREF:
        sc = scene(name)
        omaps = [oracle.VoxelMap(sc["w"], 0), oracle.VoxelMap(sc["w"], 1)]
        for k, (pl, pt) in enumerate(sc["scans"]):
            omaps[0].add_scan(k, sc["poses"][k], pl)
            omaps[1].add_scan(k, sc["poses"][k], pt)
        _OREF[name] = (omaps[0].match(sc["q_pl"], sc["Tj"]), omaps[1].match(sc["q_pt"], sc["Tj"]))
    return _OREF[name]


def with_filler(sc):
    """(q_pl, q_pt, at_pl, at_pt): the tie queries interleaved into filler queries over empty
    space, N_QPL + N_QPT >= 131072 queries (the one-lane build of the match), neither count
    a multiple of the 256 queries of a match block."""
    rng = np.random.default_rng(61)
    lo, hi = np.asarray(FILL_BOX, np.float64).T
    f_pl = planar(rng.uniform(lo, hi, (N_QPL - N_TIE, 3)), rng)
    f_pt = np.ascontiguousarray(rng.uniform(lo, hi, (N_QPT - N_TIE, 3)), np.float32)
    q_pl, at_pl = interleave(f_pl, sc["q_pl"], 4)
    q_pt, at_pt = interleave(f_pt, sc["q_pt"], 2)
    return q_pl, q_pt, at_pl, at_pt


def describe(sc, t, i):
    """Class, tie multiplicity and block of tie query i of a type (for assertion messages)."""
    blk = [b for b, v in sc["blocks"].items() if i in v[t]]
    return dict(scene=sc["name"], cls=sc["cls"], type=t, query=int(i), mult=int(tie_analysis(sc, t)["mult"][i]), block=blk)

"""Case table and scene builder of the pair-sort tests (tests/test_pairsort_cpu.py,
tests/test_gpu_pairsort.py).

A case is a match of npl planar + npt point queries against K scans.  design() fixes every
query's pair (or -1: unmatched) so that the per-pair counts carry the patterns the sort can
get wrong; build_scene() then places scan k's records in a cluster of its own, several
voxel widths from every other cluster, and every query a few centimetres from a record of
its designed scan (or far from everything), so the match realizes the design exactly."""
from dataclasses import dataclass

import numpy as np

VOXEL = 0.8
MAX_DIST = 0.8
MIN_DIST_MAP = 0.1


@dataclass(frozen=True)
class Case:
    id: str
    K: int
    npl: int
    npt: int
    group: int          # lanes per query: 8 (g8 build) or 1 (gl build)
    form: str           # "per-block", "tail-scanned", "scatter-scanned"
    scan_launches: int  # per-block: 1 (k_scan_single) or 3, else 0
    reach: bool = True  # False: every query out of reach of every record


CASES = [
    Case("A", 5, 2500, 700, 8, "scatter-scanned", 0),
    Case("A1", 1, 70, 0, 8, "scatter-scanned", 0),
    Case("A2-nopl", 5, 0, 700, 8, "scatter-scanned", 0),
    Case("A2-nopt", 5, 2500, 0, 8, "scatter-scanned", 0),
    Case("A3", 5, 2500, 700, 8, "scatter-scanned", 0, reach=False),
    Case("B", 256, 20480, 4096, 8, "scatter-scanned", 0),  # table = 256 * 24 = 6144 words
    Case("C", 256, 20481, 4096, 8, "tail-scanned", 0),     # 25 tiles: 6400 words
    Case("D", 257, 300, 100, 8, "per-block", 1),           # 257 * 14 = 3598 words
    Case("D2", 300, 2500, 700, 8, "per-block", 3),         # 300 * 101 = 30300 words
    Case("D3", 1024, 110000, 21072, 8, "per-block", 3),    # 1024 * 4097 words: 1025 scan tiles
    Case("E", 40, 110000, 21071, 8, "scatter-scanned", 0),   # 131071 queries
    Case("E'", 40, 110000, 21072, 1, "scatter-scanned", 0),  # 131072 queries
    Case("F64", 64, 110000, 21072, 1, "tail-scanned", 0),
    Case("F256", 256, 110000, 21072, 1, "tail-scanned", 0),
]
BY_ID = {c.id: c for c in CASES}

# (n_qpl, n_qpt, K) on either side of every dispatch boundary, with the expected
# (group, form, hist_words, scan_launches)
BOUNDARIES = [
    ((110000, 21071, 40), (8, "scatter-scanned", 0, 0)),   # nq = 131071
    ((110000, 21072, 40), (1, "scatter-scanned", 0, 0)),   # nq = 131072
    ((110000, 21072, 256), (1, "tail-scanned", 0, 0)),     # K = 256: still tiled, large build
    ((110000, 21072, 257), (8, "per-block", 257 * 4097, 3)),  # K = 257: per-block, g8 whatever nq
    ((20480, 4096, 256), (8, "scatter-scanned", 0, 0)),    # table 6144 words
    ((20481, 4096, 256), (8, "tail-scanned", 0, 0)),       # 6400 words (the next reachable size)
    ((6144 * 1024, 0, 1), (1, "scatter-scanned", 0, 0)),   # K = 1: 6144 tiles
    ((6144 * 1024 + 1, 0, 1), (1, "tail-scanned", 0, 0)),  # 6145 tiles = 6145 words
    ((32 * 32, 0, 512), (8, "per-block", 16384, 1)),       # 512 pairs x 32 blocks: one scan launch
    ((29 * 32, 0, 565), (8, "per-block", 16385, 3)),       # 16385 = 565 pairs x 29 blocks: three
    ((4096 * 32, 0, 1024), (8, "per-block", 4194304, 3)),  # 1024 scan tiles: one k_scan_blocks pass
    ((5 * 32, 0, 838861), (8, "per-block", 4194305, 3)),   # 4194305 = 838861 pairs x 5 blocks: 1025 tiles
]


def roles(K):
    """Which pairs play which part in design()."""
    if K >= 16:
        empty = {0, K // 2, K - 1}
        ids = [k for k in range(K) if k not in empty]
        return dict(empty=sorted(empty), edge=ids[0:4], edge_rows=(255, 256, 257, 512), point_only=ids[4],
                    wave=ids[5], alt=(ids[6], ids[7]), last=ids[8], filler=ids[9:])
    if K >= 5:  # no room for every part: one chunk-edge pair; the point-only pair is also the last-wave pair
        return dict(empty=[0], edge=[1], edge_rows=(257,), point_only=2, wave=3, alt=(3, 4), last=2, filler=[3, 4])
    return dict(empty=[], edge=[], edge_rows=(), point_only=None, wave=0, alt=(0, 0), last=0, filler=list(range(K)))


def design(case, seed=0):
    """Designed pair of every planar and every point query (-1: stays unmatched):
    chunk-edge pairs with exactly 255 / 256 / 257 / 512 plane rows and no point rows, a pair
    with point rows only, empty pairs at the first, a middle and the last index, a whole wave
    on one pair, two pairs alternating lane by lane, a pair matched only in each type's last
    (partial) wave, and unmatched queries interleaved throughout."""
    K = case.K
    if not case.reach:
        return np.full(case.npl, -1, np.int32), np.full(case.npt, -1, np.int32)
    R = roles(K)
    rng = np.random.default_rng([seed, K])
    out = []
    for t, n in enumerate((case.npl, case.npt)):
        u = rng.random((n, 2))
        fill = np.asarray(R["filler"], np.int32)
        arr = np.full(n, -1, np.int32)
        if len(fill):
            arr = np.where(u[:, 0] < 0.8, fill[(u[:, 1] * len(fill)).astype(np.int64) % len(fill)], -1).astype(np.int32)
        free = np.ones(n, bool)
        if n >= 256:
            w0 = (n // 64) // 3
            arr[64 * w0:64 * w0 + 64] = R["wave"]
            arr[64 * w0 + 64:64 * w0 + 128] = np.where(np.arange(64) % 2 == 0, R["alt"][0], R["alt"][1])
            free[64 * w0:64 * w0 + 128] = False
        if n > 0:
            s = 64 * ((n - 1) // 64)  # the last wave of the last tile
            if t == 1 or R["last"] != R["point_only"]:
                arr[s:] = R["last"]
                arr[s + 1::3] = -1  # (unmatched queries in it too; at least the first lane matches)
                free[s:] = False
        idx = rng.permutation(np.flatnonzero(free))
        if t == 0 and len(idx) >= sum(R["edge_rows"]) + 64:
            o = 0
            for k, rows in zip(R["edge"], R["edge_rows"]):
                arr[idx[o:o + rows]] = k
                o += rows
        elif t == 1 and R["point_only"] is not None and R["point_only"] != R["last"]:
            arr[idx[:max(len(idx) // 10, 1)]] = R["point_only"]
        out.append(arr)
    return out[0], out[1]


def design_counts(K, pair_pl, pair_pt):
    return (np.bincount(pair_pl[pair_pl >= 0], minlength=K).astype(np.uint32),
            np.bincount(pair_pt[pair_pt >= 0], minlength=K).astype(np.uint32))


def _rot(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _pose(rng, rot, trans):
    v = rng.normal(size=3)
    return np.hstack([_rot(v, rot * rng.uniform(0.5, 1.0)), rng.uniform(-trans, trans, (3, 1))])


def _xf(T, p):
    return p @ T[:, :3].T + T[:, 3]


def _inv(T):
    R = T[:, :3].T
    return np.hstack([R, -(R @ T[:, 3])[:, None]])


# records of one scan and type: four, 1 m apart, all inside the scan's own cluster
REC_OFF = np.array([[0.5, 0.5, 0.0], [-0.5, 0.5, 0.0], [0.5, -0.5, 0.0], [-0.5, -0.5, 0.0]])
SPACING = 5 * VOXEL  # between cluster centres


def build_scene(K, pair_pl, pair_pt, seed=0):
    """Scan k's records (both types) around centre k of a grid with SPACING; each query
    3 cm (one in ten: 30 cm, so it is matched and inserted) from a record of its designed
    scan, an unmatched one 40 m above the grid.  Everything is moved by one common
    non-identity pose W; the map scans and the query scan have poses of their own."""
    rng = np.random.default_rng([seed, K, 7])
    side = int(np.ceil(np.sqrt(K)))
    k = np.arange(K)
    centres = np.stack([SPACING * (k % side), SPACING * (k // side), np.zeros(K)], 1)
    W = _pose(rng, 0.6, 30.0)
    poses = np.stack([_pose(rng, 0.05, 1.0) for _ in range(K)])
    Tj = _pose(rng, 0.03, 0.5)
    scans = []
    for s in range(K):
        Ti = _inv(poses[s])
        wp = _xf(W, centres[s] + REC_OFF)
        wn = rng.normal(size=(4, 3))
        wn /= np.linalg.norm(wn, axis=1, keepdims=True)
        pl = np.hstack([_xf(Ti, wp), wn @ Ti[:, :3].T]).astype(np.float32)
        scans.append((pl, _xf(Ti, wp).astype(np.float32)))
    Tji = _inv(Tj)
    q = []
    for t, pr in enumerate((pair_pl, pair_pt)):
        n = len(pr)
        u = np.random.default_rng([seed, K, 11 + t]).random((n, 6))  # (row-major: a prefix of a longer draw)
        hit = pr >= 0
        c = centres[np.where(hit, pr, (u[:, 0] * K).astype(np.int64) % K)]
        d = u[:, 1:4] - 0.5 + 1e-3
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        off = REC_OFF[(u[:, 4] * 4).astype(np.int64) % 4] + d * np.where(u[:, 5] < 0.1, 0.3, 0.03)[:, None]
        off = np.where(hit[:, None], off, np.array([0.0, 0.0, 40.0]) + d)
        q.append(_xf(Tji, _xf(W, c + off)).astype(np.float32))
    q_pl = np.hstack([q[0], np.tile(np.float32([0, 0, 1]), (len(q[0]), 1))]).astype(np.float32)
    return dict(K=K, scans=scans, poses=poses, Tj=Tj, q_pl=q_pl, q_pt=q[1], pair_pl=pair_pl, pair_pt=pair_pt)


def case_design(case, seed=0):
    """design(), except that E' is E with one more point query (of a filler pair) at the
    end: its rows but that query's must equal E's although another build sorts them."""
    if case.id == "E'":
        pl, pt = design(BY_ID["E"], seed)
        return pl, np.append(pt, np.int32(roles(case.K)["filler"][0]))
    return design(case, seed)


def case_scene(case, seed=0):
    pl, pt = case_design(case, seed)
    assert (len(pl), len(pt)) == (case.npl, case.npt)
    return build_scene(case.K, pl, pt, seed)

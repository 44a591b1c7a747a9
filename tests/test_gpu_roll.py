"""Rolling the dense voxel map on the device (fmx_roll_*; DESIGN.md §Dense map, Rolling)
against the numpy restatement (tests/roll_ref.py).  Every comparison with the restatement is
equality on key-sorted arrays, doubles compared as bits: which voxels a roll evicts, and what
the map holds afterwards, is defined exactly and does not depend on thread order."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

import dense_ref as R
import roll_ref as RR
from form_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = {"odd": (5, 200), "tiny": (16, 256)}
OOM, STATE, SIZE, INVAL = 3, 5, 2, 1
FULL = (1 << 21,) * 3  # a box that holds every voxel


def _geo(name):
    r, c = SHAPES[name]
    return synth.ScanGeometry(r, c, 15.0, 0.01, 0.02)


def _ctx(fmx, geo=None, window=None, **over):
    p = synth.default_params(geo or _geo("tiny"))
    kw = dict(over)
    if window:
        kw.update(max_num_recent_scans=window[0], max_num_keyscans=window[1])
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p), **kw))


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _pose(Rm, t):
    T = np.zeros((3, 4))
    T[:, :3] = Rm
    T[:, 3] = t
    return T


# test_gpu_dense.py's poses, scan ids and scans, restated
POSES = [_pose(_rot("z", 0.3), (-12.5, -3.25, -0.75)), _pose(_rot("x", 0.4) @ _rot("y", -0.7), (2.0, 1.0, 0.5)),
         _pose(_rot("y", 1.1) @ _rot("z", -2.0), (-0.3, 14.0, -2.0))]
SCAN_IDS = [(1 << 32) + 7, (1 << 40) + 1, (1 << 33)]
I34 = np.eye(3, 4)


@functools.lru_cache(maxsize=None)
def _points(name, k):
    if name == "list":
        g = np.random.default_rng(100 + k)
        p = np.zeros((777, 4), np.float32)
        p[:, :3] = g.normal(0, 1, (777, 3)) * g.choice([0.3, 3.0, 30.0, 80.0], (777, 1))
        p[g.choice(777, 20, replace=False), :3] = 0
        p[5, 0], p[6, 1], p[7, 2] = np.nan, np.inf, -np.inf
    else:
        p = synth.raycast(synth.World(), synth.trajectory_pose(k), _geo(name), 4242 + k).numpy()
    p.setflags(write=False)
    return p


def _arg(p, on_device):
    return torch.from_numpy(np.array(p)).to("cuda:0") if on_device else np.array(p)


def _check(ctx, ref, min_hits=1):
    got = R.sort_download(ctx.dense_download(min_hits), ref.w)
    want = ref.sorted(min_hits)
    assert R.same(got, want) is None, R.same(got, want)
    assert ctx.dense_stats()["voxels"] == ref.voxels and ctx.dense_stats()["integrations"] == len(ref.seq_scan)
    return want


def _evict(ctx, ref, centre, half):
    """A roll on both; the evicted sets agree.  Returns the reference's."""
    assert ctx.roll_count(centre, half) == ref.count(centre, half)
    got = R.sort_download(ctx.roll_evict(centre, half), ref.w)
    want = ref.evict(centre, half)
    assert R.same(got, want) is None, R.same(got, want)
    return want


def _status(fmx, fn):
    with pytest.raises(fmx.FmxError) as e:
        fn()
    return e.value.status


def _centres(voxels):
    """Points at the centres of voxels of width 1 (exact in fp32 below 2^23); a list of cx
    stands for (cx, 0, 0)."""
    v = np.array([(c, 0, 0) if np.isscalar(c) else c for c in voxels], np.float64).reshape(-1, 3)
    p = np.zeros((len(v), 4), np.float32)
    p[:, :3] = v + 0.5
    assert np.array_equal(p[:, :3].astype(np.float64), v + 0.5)
    return p


# ------------------------------------------------------------------ 1. stand-alone
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["odd", "tiny", "list"])
def test_evict_matches_restatement(fmx_mod, name, on_device):
    ctx = _ctx(fmx_mod, _geo(name) if name != "list" else None)
    ctx.dense_configure(True, 0.5, 1 << 14)
    ref = RR.RollRef(0.5, 1 << 14)
    for k in range(2):
        p = _points(name, k)
        assert ctx.dense_integrate(_arg(p, on_device), POSES[k], SCAN_IDS[k]) == ref.integrate(p, POSES[k], SCAN_IDS[k])
        _check(ctx, ref)
    ev = _evict(ctx, ref, POSES[1][:, 3], (40, 40, 12))
    kept = _check(ctx, ref)
    print(name, "kept / evicted", len(kept["key"]), len(ev["key"]))
    assert len(kept["key"]) > 0 and len(ev["key"]) > 0
    assert ctx.dense_stats() == dict(voxels=ref.voxels, max_voxels=1 << 14, integrations=2, slots=1 << 15)
    assert ctx.roll_stats() == dict(rolls=0, evicted=0, spilled=0, last_kept=0, last_evicted=0, last_scan=0)
    p = _points(name, 2)
    assert ctx.dense_integrate(_arg(p, on_device), POSES[2], SCAN_IDS[2]) == ref.integrate(p, POSES[2], SCAN_IDS[2])
    _check(ctx, ref)
    p = _points(name, 0)  # scan 0 again under a new scan_idx: its evicted voxels open anew
    got = ctx.dense_integrate(_arg(p, on_device), POSES[0], 99)
    assert got == ref.integrate(p, POSES[0], 99)
    m = _check(ctx, ref)
    reopened = (m["scan"] == 99) & np.isin(m["key"], ev["key"])
    assert got["added"] == int((m["scan"] == 99).sum()) and int(reopened.sum()) > 0


# ------------------------------------------------------------------ 2. probe chains across the wrap
@functools.lru_cache(maxsize=None)
def _colliders():
    """Four voxels (cx, 0, 0) homing to slot 2047 of 2048 and four to slot 0, by brute force."""
    last, zero = [], []
    for cx in range(1, 200000):
        h = R.home_slot(R.pack_key(cx, 0, 0), 2048)
        if h == 2047 and len(last) < 4:
            last.append(cx)
        elif h == 0 and len(zero) < 4:
            zero.append(cx)
        if len(last) == 4 and len(zero) == 4:
            return last, zero
    raise AssertionError("no colliding voxels found")


def _x_box(lo, hi):
    """Centre and half-extents of the box that holds the voxels (cx, 0, 0) with cx in [lo', hi],
    lo' = lo or lo - 1."""
    cc = (lo + hi) // 2
    return (cc + 0.5, 0.5, 0.5), (hi - cc, 0, 0)


def test_probe_chains_survive_the_rebuild(fmx_mod):
    last, zero = _colliders()
    # a box is an interval of cx: of the eight sorted by cx, some four neighbours are two of each
    # chain (the count of `last` among four neighbours goes from a to 4 - a in steps of one)
    both = sorted(last + zero)
    keep = next(both[i:i + 4] for i in range(5) if len(set(both[i:i + 4]) & set(last)) == 2)
    centre, half = _x_box(keep[0], keep[-1])
    # one voxel per integration, so the order along each probe chain is the order given here:
    # evicted, kept, evicted, kept from slot 2047 across the wrap, then the same behind them from slot 0
    order = []
    for chain in (last, zero):
        k, e = [c for c in chain if c in keep], [c for c in chain if c not in keep]
        order += [e[0], k[0], e[1], k[1]]
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 1024, min_norm_squared=0.1, max_norm_squared=1e12)
    ref = RR.RollRef(1.0, 1024, 0.1, 1e12)
    assert ctx.dense_stats()["slots"] == 2048
    for i, cx in enumerate(order):
        assert ctx.dense_integrate(_centres([cx]), I34, i) == ref.integrate(_centres([cx]), I34, i)
    ev = _evict(ctx, ref, centre, half)
    assert sorted(int(k) for k in ev["key"]) == sorted(R.pack_key(c, 0, 0) for c in order[0::2])
    assert sorted(int(k) for k in _check(ctx, ref)["key"]) == sorted(R.pack_key(c, 0, 0) for c in keep)
    # a hole in a chain would let a kept voxel behind it be inserted a second time
    again = _centres(order)
    got = ctx.dense_integrate(again, I34, 50)
    assert got == ref.integrate(again, I34, 50) == dict(added=4, merged=4, gated=0, out_of_range=0, invalid=0)
    m = _check(ctx, ref)
    keys = R.key_of_points(ctx.dense_download()["points"], 1.0)
    assert len(np.unique(keys)) == len(keys) == 8
    assert sorted(m["hits"].tolist()) == [1, 1, 1, 1, 2, 2, 2, 2]


# ------------------------------------------------------------------ 3. box edges
FAR = (1 << 20) - 2  # the largest voxel coordinate


def _edges(fmx, centre, half):
    """Voxels at cc, cc +- half and cc +- (half + 1) on each axis separately (those the key range
    holds); returns the kept and the evicted voxel coordinates after the roll about centre."""
    cc = [math.floor(centre[k]) for k in range(3)]  # voxel width 1
    assert RR.centre_voxel(centre, 1.0) == cc
    vox = {tuple(cc)}
    for ax in range(3):
        for d in (-half[ax] - 1, -half[ax], half[ax], half[ax] + 1):
            v = list(cc)
            v[ax] += d
            if abs(v[ax]) <= FAR:
                vox.add(tuple(v))
    vox = sorted(vox)
    ctx = _ctx(fmx)
    ctx.dense_configure(True, 1.0, 1024, min_norm_squared=0.1, max_norm_squared=1e15)
    ref = RR.RollRef(1.0, 1024, 0.1, 1e15)
    got = ctx.dense_integrate(_centres(vox), I34, 3)
    assert got == ref.integrate(_centres(vox), I34, 3) and got["added"] == len(vox)
    ev = _evict(ctx, ref, centre, half)
    kept = _check(ctx, ref)
    want_kept = [v for v in vox if all(abs(v[k] - cc[k]) <= half[k] for k in range(3))]
    assert sorted(int(k) for k in kept["key"]) == sorted(R.pack_key(*v) for v in want_kept)
    assert len(ev["key"]) == len(vox) - len(want_kept)
    return want_kept, [v for v in vox if v not in want_kept]


def test_box_edges(fmx_mod):
    kept, ev = _edges(fmx_mod, (-7.5, -3.5, -9.5), (3, 2, 1))  # negative coordinates
    assert len(kept) == 7 and len(ev) == 6 and (-11, -4, -10) in kept and (-12, -4, -10) in ev
    kept, ev = _edges(fmx_mod, (5.5, -2.5, 0.5), (0, 0, 0))  # half = 0: the centre voxel alone
    assert kept == [(5, -3, 0)] and len(ev) == 6
    kept, ev = _edges(fmx_mod, (3.0, -2.0, 0.0), (2, 2, 2))  # on a voxel face: that voxel's
    assert (5, -2, 0) in kept and (6, -2, 0) in ev and (3, -4, 0) in kept and (3, -5, 0) in ev
    below = (np.nextafter(3.0, 0.0), np.nextafter(-2.0, -3.0), np.nextafter(0.0, -1.0))  # one ulp below: the one before
    kept, ev = _edges(fmx_mod, below, (2, 2, 2))
    assert (4, -3, -1) in kept and (5, -3, -1) in ev and (0, -3, -1) in kept and (-1, -3, -1) in ev
    # the ends of the key range
    kept, ev = _edges(fmx_mod, (FAR - 2 + 0.5, -(FAR - 2) + 0.5, 7.5), (2, 2, 2))
    assert (FAR, -(FAR - 2), 7) in kept and (FAR - 2, -FAR, 7) in kept
    kept, ev = _edges(fmx_mod, (FAR - 3 + 0.5, -(FAR - 3) + 0.5, 7.5), (2, 2, 2))
    assert (FAR, -(FAR - 3), 7) in ev and (FAR - 3, -FAR, 7) in ev
    # centres and half-extents that are refused
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 1024)
    for centre in ((FAR + 1.5, 0, 0), (0, -(FAR + 1) + 0.5, 0), (0, 0, 1e300), (np.nan, 0, 0), (0, np.inf, 0),
                   (0, 0, -np.inf)):
        assert _status(fmx_mod, lambda: ctx.roll_count(centre, (1, 1, 1))) == INVAL, centre
        assert _status(fmx_mod, lambda: ctx.roll_evict(centre, (1, 1, 1), discard=True)) == INVAL, centre
    assert ctx.roll_count((FAR + 0.5, -FAR + 0.5, 0), FULL) == (0, 0)
    assert _status(fmx_mod, lambda: ctx.roll_count((0, 0, 0), (1, (1 << 21) + 1, 1))) == INVAL
    assert _status(fmx_mod, lambda: ctx.roll_evict((0, 0, 0), (1, 1, (1 << 21) + 1))) == INVAL


# ------------------------------------------------------------------ 4 / 9. degenerate rolls, profiling
NOWHERE = (5000.25, 5000.25, 5000.25)


def test_degenerate_rolls_and_the_profile(fmx_mod):
    ctx = _ctx(fmx_mod, _geo("odd"))
    ctx.dense_configure(True, 0.5, 4096)
    ref = RR.RollRef(0.5, 4096)
    S = 8192
    ctx.profile(True)
    assert list(ctx.profile_read())[-3:] == ["deskew", "organize", "dense"]  # no id added
    # an empty map
    ctx.profile_reset()
    assert len(ctx.roll_evict((0, 0, 0), (1, 1, 1), discard=True)["hits"]) == 0
    assert ctx.roll_count((0, 0, 0), (1, 1, 1)) == (0, 0) and ctx.dense_stats()["voxels"] == 0
    d = ctx.profile_read()["dense"]
    assert d["launches"] == 2 and d["bytes"] == 2 * S * 8
    for k in range(2):
        ctx.dense_integrate(_points("odd", k), POSES[k], k)
        ref.integrate(_points("odd", k), POSES[k], k)
    before = _check(ctx, ref)
    # nothing outside: the count alone
    ctx.profile_reset()
    ctx.roll_evict(POSES[1][:, 3], FULL, discard=True)
    d = ctx.profile_read()["dense"]
    assert d["launches"] == 1 and d["bytes"] == S * 8
    assert R.same(_check(ctx, ref), before) is None
    # some of each: count, split, reinsert
    kept, ev = ref.count(POSES[1][:, 3], (40, 40, 12))
    assert kept > 0 and ev > 0
    ctx.profile_reset()
    ctx.roll_evict(POSES[1][:, 3], (40, 40, 12), discard=True)
    d = ctx.profile_read()["dense"]
    assert d["launches"] == 3 and d["bytes"] == S * 8 + (S * 16 + ev * 92 + kept * 100) + kept * 88
    ref.evict(POSES[1][:, 3], (40, 40, 12))
    _check(ctx, ref)
    # everything outside: count and split
    ctx.profile_reset()
    ctx.roll_evict(NOWHERE, (0, 0, 0), discard=True)
    d = ctx.profile_read()["dense"]
    assert d["launches"] == 2 and d["bytes"] == S * 8 + S * 16 + kept * 92
    assert len(ref.evict(NOWHERE, (0, 0, 0))["key"]) == kept and ref.voxels == 0
    assert ctx.dense_stats()["voxels"] == 0 and len(ctx.dense_download()["hits"]) == 0
    p = _points("odd", 2)
    assert ctx.dense_integrate(p, POSES[2], 7) == ref.integrate(p, POSES[2], 7)
    _check(ctx, ref)


# ------------------------------------------------------------------ 5. load 1/2
def test_full_table_rolls_and_fills_again(fmx_mod):
    last, zero = _colliders()
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 1024, min_norm_squared=0.1, max_norm_squared=1e12)
    ref = RR.RollRef(1.0, 1024, 0.1, 1e12)
    first = _centres(last + zero + zero[::-1] + last[::-1])
    assert ctx.dense_integrate(first, I34, 0) == ref.integrate(first, I34, 0)
    rest = list(range(300000, 301016))
    for k, (a, b) in enumerate(((0, 500), (500, 900), (900, 1016))):
        chunk = _centres(rest[a:b])
        assert ctx.dense_integrate(_arg(chunk, k % 2 == 0), I34, k + 1) == ref.integrate(chunk, I34, k + 1)
    assert ctx.dense_stats()["voxels"] == ref.voxels == 1024
    assert _status(fmx_mod, lambda: ctx.dense_integrate(_centres([5]), I34, 9)) == OOM
    lo = min(last + zero)
    ev = _evict(ctx, ref, *_x_box(lo, rest[-2]))  # all but the last of `rest`
    assert ev["key"].tolist() == [R.pack_key(rest[-1], 0, 0)]
    assert len(_check(ctx, ref)["key"]) == 1023  # the 1023 survive, bit for bit
    K = 37
    ev = _evict(ctx, ref, *_x_box(lo, rest[-2 - K]))
    assert len(ev["key"]) == K and ref.voxels == 1023 - K
    _check(ctx, ref)
    fresh = list(range(400000, 400000 + K + 2))
    assert ref.integrate(_centres(fresh), I34, 10) is None  # K + 2 points: one too many
    assert _status(fmx_mod, lambda: ctx.dense_integrate(_centres(fresh), I34, 10)) == OOM
    got = ctx.dense_integrate(_centres(fresh[:K]), I34, 11)
    assert got == ref.integrate(_centres(fresh[:K]), I34, 11) and got["added"] == K
    assert ctx.dense_stats()["voxels"] == 1023
    _check(ctx, ref)


# ------------------------------------------------------------------ 6. buffers and errors
def test_buffers_errors_and_clear(fmx_mod):
    fmx = fmx_mod
    L = fmx.lib()
    ctx, other = _ctx(fmx, _geo("odd")), _ctx(fmx, _geo("odd"))
    centre, half = POSES[1][:, 3].copy(), (40, 40, 12)
    calls = (lambda: ctx.roll_configure(True, half, 1.0), lambda: ctx.roll_count(centre, half),
             lambda: ctx.roll_evict(centre, half), lambda: ctx.roll_evict(centre, half, discard=True), ctx.roll_drain)
    for fn in calls:  # before fmx_dense_configure
        assert _status(fmx, fn) == STATE
    assert ctx.roll_stats() == dict(rolls=0, evicted=0, spilled=0, last_kept=0, last_evicted=0, last_scan=0)
    ctx.dense_configure(False, 0.5, 4096)  # configured, not enabled
    for fn in calls:
        assert _status(fmx, fn) == STATE
    ctx.dense_configure(True, 0.5, 4096)
    other.dense_configure(True, 0.5, 4096)
    for kw in (dict(step=-1.0), dict(step=np.nan), dict(step=np.inf), dict(half=(1, 1, (1 << 21) + 1))):
        args = dict(half=half, step=1.0)
        args.update(kw)
        assert _status(fmx, lambda: ctx.roll_configure(True, **args)) == INVAL, kw
    ctx.roll_configure(True, FULL, 0.0)
    ctx.roll_configure(False, half, 1.0)
    h3 = np.array(half, np.uint32)
    out2 = np.zeros(2, np.uint64)
    assert L.fmx_roll_count(ctx.h, None, fmx._p(h3), fmx._p(out2)) == INVAL
    assert L.fmx_roll_evict(ctx.h, None, fmx._p(h3), None, None, None, None, None) == INVAL
    assert L.fmx_roll_configure(ctx.h, None) == INVAL

    def start(c):
        ref = RR.RollRef(0.5, 4096)
        for k in range(2):
            q = _points("odd", k)
            assert c.dense_integrate(_arg(q, k == 1), POSES[k], SCAN_IDS[k]) == ref.integrate(q, POSES[k], SCAN_IDS[k])
        return ref

    def sequence(c):
        ref = start(c)
        ev = _evict(c, ref, centre, half)
        q = _points("odd", 2)
        assert c.dense_integrate(q, POSES[2], SCAN_IDS[2]) == ref.integrate(q, POSES[2], SCAN_IDS[2])
        return ev, _check(c, ref)

    ref = start(ctx)
    before, stats = _check(ctx, ref), ctx.dense_stats()
    m = ref.count(centre, half)[1]
    # a short buffer: FMX_E_SIZE, nothing written, nothing evicted
    pts, sc = np.full((m, 3), 7.0), np.full(m, 7, np.uint64)
    ix, hi = np.full(m, 7, np.uint32), np.full(m, 7, np.uint32)
    cap = C.c_uint32(m - 1)
    st = L.fmx_roll_evict(ctx.h, fmx._p(centre), fmx._p(h3), fmx._p(pts), fmx._p(sc), fmx._p(ix), fmx._p(hi), C.byref(cap))
    assert st == SIZE and cap.value == m - 1
    assert (pts == 7.0).all() and (sc == 7).all() and (ix == 7).all() and (hi == 7).all()
    assert R.same(_check(ctx, ref), before) is None and ctx.dense_stats() == stats
    assert ctx.roll_stats()["rolls"] == 0
    # only two of the four outputs
    cap = C.c_uint32(m)
    assert L.fmx_roll_evict(ctx.h, fmx._p(centre), fmx._p(h3), None, None, fmx._p(ix), fmx._p(hi), C.byref(cap)) == 0
    ev = ref.evict(centre, half)
    assert cap.value == m == len(ev["key"]) and (pts == 7.0).all() and (sc == 7).all()
    assert sorted(zip(ix.tolist(), hi.tolist())) == sorted(zip(ev["index"].tolist(), ev["hits"].tolist()))
    _check(ctx, ref)
    # discarded: no buffer, with and without a count
    h2 = np.array((20, 20, 6), np.uint32)
    m2 = ref.count(centre, h2)[1]
    assert m2 > 0
    assert L.fmx_roll_evict(ctx.h, fmx._p(centre), fmx._p(h2), None, None, None, None, None) == 0
    ref.evict(centre, h2)
    _check(ctx, ref)
    h1 = np.array((8, 8, 3), np.uint32)
    m1 = ref.count(centre, h1)[1]
    cap = C.c_uint32(0)
    assert L.fmx_roll_evict(ctx.h, fmx._p(centre), fmx._p(h1), None, None, None, None, C.byref(cap)) == 0
    assert cap.value == m1 > 0
    ref.evict(centre, h1)
    _check(ctx, ref)
    assert ctx.roll_stats()["rolls"] == 0  # stand-alone evictions are not the register path's
    # a clear after rolls, then a whole sequence: as on a fresh context
    ctx.dense_clear()
    assert ctx.dense_stats() == dict(voxels=0, max_voxels=4096, integrations=0, slots=8192)
    a, b = sequence(ctx), sequence(other)
    assert R.same(a[0], b[0]) is None and R.same(a[1], b[1]) is None and len(a[0]["key"]) > 0


# ------------------------------------------------------------------ 7 / 8. the register path
XI0 = np.array([0.0, 0.0, 0.01, 0.15, 0.0, 0.0])
W_REG, CAP_REG, N_REG = 0.25, 1 << 16, 9
HALF_REG, STEP_REG = (40, 40, 40), 0.25
NO_ROLL = dict(rolls=0, evicted=0, spilled=0, last_kept=0, last_evicted=0, last_scan=0)


@functools.lru_cache(maxsize=None)
def _stream(n):
    world = synth.World()
    out = []
    for k in range(n):
        s = synth.make_scan_skewed("tiny", k, world=world)[0].numpy()
        s.setflags(write=False)
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def _run(roll, deskew, feed, spill=True, step=STEP_REG, cap=CAP_REG):
    """One N_REG-scan stream with the dense map on (every 1) and rolling on or off.  Returns the
    poses, twists, per-scan dense_last, per-scan roll_stats, the key-sorted download, the
    dense_stats and the drained spill sorted by (scan, index)."""
    from form_amd import fmx
    geo = synth.GEOMETRIES["tiny"]
    scans = _stream(N_REG)
    ctx = _ctx(fmx, geo, window=(4, 3))
    if deskew:
        ctx.deskew_configure(True, initial_twist=XI0)
    ctx.dense_configure(True, W_REG, cap)
    if roll:
        ctx.roll_configure(True, HALF_REG, step, spill)
    on_device = feed in ("device", "announced")
    held = [_arg(s, on_device) for s in scans]
    poses, twists, lasts, rolls = [], [], [], []
    for k in range(N_REG):
        if feed.startswith("announced") and k + 1 < N_REG:
            ctx.next_scan(held[k + 1])
        ctx.register_scan(held[k])
        poses.append(ctx.current_pose().copy())
        twists.append(ctx.deskew_last()[0].copy())
        lasts.append(ctx.dense_last())
        rolls.append(ctx.roll_stats())
    down = R.sort_download(ctx.dense_download(), W_REG)
    stats = ctx.dense_stats()
    spilled = RR.sort_by_owner(ctx.roll_drain())
    assert ctx.roll_stats()["spilled"] == 0 and len(ctx.roll_drain()["hits"]) == 0  # a drain empties it
    ctx.close()
    return poses, twists, lasts, rolls, down, stats, spilled


def _drive(fmx, run, deskew, spill=True, step=STEP_REG, cap=CAP_REG):
    """The restatement over the scans the extractor saw at the poses the device ended with;
    asserts every registration's counts and roll statistics.  Returns it and the number of
    evicted voxels that a later scan opened again."""
    scans = _stream(N_REG)
    poses, twists, lasts, rolls = run[:4]
    other = _ctx(fmx, synth.GEOMETRIES["tiny"])
    ref = RR.RollRef(W_REG, cap)
    ref.roll_configure(True, HALF_REG, step, spill)
    gone, reopened = set(), 0
    for k in range(N_REG):
        seen = other.deskew(np.array(scans[k]), twists[k]) if deskew else scans[k]
        had = set(ref.vox)
        ref.before_scan(k, len(seen), poses[k - 1] if k else None)
        kept = set(ref.vox)
        gone |= had - kept
        counts = ref.integrate(seen, poses[k], k)  # every = 1: each scan is due
        integrated = 1 if counts is not None else -1
        reopened += len((set(ref.vox) - kept) & gone)
        want = counts if counts is not None else dict(added=0, merged=0, gated=0, out_of_range=0, invalid=0)
        assert lasts[k] == (want, integrated), k
        assert rolls[k] == ref.stats(), k
    return ref, reopened


REG_CASES = [(False, "device"), (False, "host"), (False, "announced"), (False, "announced-host"), (True, "device"),
             (True, "announced")]


@pytest.mark.parametrize("deskew,feed", REG_CASES)
def test_register_path_rolls_as_restated(fmx_mod, deskew, feed):
    run = _run(True, deskew, feed)
    ref, reopened = _drive(fmx_mod, run, deskew)
    print("rolls (scan, kept, evicted)", ref.rolls, "re-opened", reopened)
    assert len(ref.rolls) >= 2 and all(k > 0 and e > 0 for _, k, e in ref.rolls) and reopened > 0
    assert R.same(run[4], ref.sorted()) is None
    assert run[5]["voxels"] == ref.voxels and run[5]["integrations"] == N_REG
    assert RR.same_owner_sorted(run[6], ref.drain()) is None
    assert len(run[6]["hits"]) == sum(e for _, _, e in ref.rolls)


def test_register_path_feeds_agree_and_estimation_is_untouched(fmx_mod):
    for deskew, feeds in ((True, ("device", "announced")), (False, ("device", "host", "announced", "announced-host"))):
        runs = [_run(True, deskew, f) for f in feeds]
        for r in runs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(runs[0][0], r[0]))
            assert runs[0][2] == r[2] and runs[0][3] == r[3]
            assert R.same(runs[0][4], r[4]) is None and RR.same_owner_sorted(runs[0][6], r[6]) is None
        off = _run(False, deskew, feeds[-1])
        assert all(s == NO_ROLL for s in off[3]) and len(off[6]["hits"]) == 0
        for k in range(N_REG):  # poses and twists with rolling on: the rolling-off run's, bit for bit
            assert np.array_equal(runs[-1][0][k].view(np.uint64), off[0][k].view(np.uint64)), k
            assert np.array_equal(runs[-1][1][k], off[1][k]), k
        assert len(off[4]["key"]) > len(runs[-1][4]["key"])


def test_register_path_without_spill(fmx_mod):
    kept, gone = _run(True, False, "device"), _run(True, False, "device", spill=False)
    assert R.same(kept[4], gone[4]) is None and kept[2] == gone[2]
    assert len(gone[6]["hits"]) == 0 and all(s["spilled"] == 0 for s in gone[3])
    assert [dict(s, spilled=0) for s in kept[3]] == gone[3]
    ref, _ = _drive(fmx_mod, gone, False, spill=False)
    assert R.same(gone[4], ref.sorted()) is None and len(ref.drain()["hits"]) == 0


def test_capacity_trigger_rolls_instead_of_refusing(fmx_mod):
    scans = _stream(N_REG)
    n = len(scans[0])
    poses = _run(False, False, "device")[0]
    big = RR.RollRef(W_REG, CAP_REG)
    v = []
    for k in range(2):
        big.integrate(scans[k], poses[k], k)
        v.append(big.voxels)
    cap = v[1] + n - 1  # scan 1 fits (v[0] + n <= cap), scan 2 would not
    assert v[0] < v[1]
    off = _run(False, False, "device", cap=cap)
    assert [l[1] for l in off[2][:3]] == [1, 1, -1]
    run = _run(True, False, "device", step=1e9, cap=cap)
    assert [l[1] for l in run[2][:3]] == [1, 1, 1]
    assert run[3][1] == NO_ROLL and run[3][2]["rolls"] == 1 and run[3][2]["last_scan"] == 2
    assert run[3][2]["last_kept"] > 0 and run[3][2]["last_evicted"] > 0
    ref, _ = _drive(fmx_mod, run, False, step=1e9, cap=cap)
    assert R.same(run[4], ref.sorted()) is None and RR.same_owner_sorted(run[6], ref.drain()) is None
    for k in range(N_REG):
        assert np.array_equal(run[0][k].view(np.uint64), poses[k].view(np.uint64)), k


# ------------------------------------------------------------------ 10. FORM
def test_form_dense_roll_round_trip(fmx_mod):
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    scans = _stream(5)
    f = fmx_mod.FORM()
    f.set_lidar_params(lidar)
    assert len(f.dense_evicted()["hits"]) == 0
    f.set_dense_map(True, voxel_width=0.5, max_voxels=1 << 15)
    f.set_dense_roll(True, 9.9, 0.1)  # ceil(9.9 / 0.5) = 20 voxels
    f.initialize()
    ref = RR.RollRef(0.5, 1 << 15)
    ref.roll_configure(True, (20, 20, 20), 0.1)
    prev = None
    for k in range(5):
        f.add_lidar(scans[k][:, :3])
        ref.register(k, scans[k], f.pose()[:3], prev)
        prev = f.pose()[:3].copy()
    assert len(ref.rolls) >= 1 and ref.stats()["evicted"] > 0
    assert f._est.roll_stats() == ref.stats()
    d = f.dense_map()
    assert R.same(R.sort_download(d, 0.5), ref.sorted()) is None
    e = f.dense_evicted()
    assert sorted(e) == ["hits", "index", "points", "scan"]
    assert e["points"].dtype == np.float64 and e["scan"].dtype == np.uint64
    assert e["index"].dtype == np.uint32 and e["hits"].dtype == np.uint32
    assert RR.same_owner_sorted(RR.sort_by_owner(e), ref.drain()) is None
    assert len(f.dense_evicted()["hits"]) == 0

"""The dense voxel map on the device (fmx_dense_*; DESIGN.md §Dense map) against the numpy
restatement (tests/dense_ref.py).  Every comparison with the restatement is equality on the
key-sorted arrays, doubles compared as bits: the map's content is defined exactly and does
not depend on the order the device's threads run in."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

import dense_ref as R
from form_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = {"odd": (5, 200), "tiny": (16, 256)}
OOM, STATE, SIZE, INVAL = 3, 5, 2, 1


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


# a negative translation; a rotation about an axis that is not z; both
POSES = [_pose(_rot("z", 0.3), (-12.5, -3.25, -0.75)), _pose(_rot("x", 0.4) @ _rot("y", -0.7), (2.0, 1.0, 0.5)),
         _pose(_rot("y", 1.1) @ _rot("z", -2.0), (-0.3, 14.0, -2.0))]
SCAN_IDS = [(1 << 32) + 7, (1 << 40) + 1, (1 << 33)]


@functools.lru_cache(maxsize=None)
def _points(name, k):
    """Scan k of a shape: a raycast 5 x 200 or 16 x 256 scan (with dropouts), or a plain list
    of 777 points with some invalid ones and some beyond the gate."""
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
    return want


def _status(fmx, fn):
    with pytest.raises(fmx.FmxError) as e:
        fn()
    return e.value.status


# ------------------------------------------------------------------ 1. stand-alone
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["odd", "tiny", "list"])
def test_integrate_matches_restatement(fmx_mod, name, on_device):
    ctx = _ctx(fmx_mod, _geo(name) if name != "list" else None)
    ctx.dense_configure(True, 0.5, 1 << 14)
    ref = R.DenseRef(0.5, 1 << 14)
    assert ctx.dense_stats() == dict(voxels=0, max_voxels=1 << 14, integrations=0, slots=1 << 15)
    for k in range(3):
        p = _points(name, k)
        got = ctx.dense_integrate(_arg(p, on_device), POSES[k], SCAN_IDS[k])
        want = ref.integrate(p, POSES[k], SCAN_IDS[k])
        assert got == want and sum(got.values()) == len(p), k
        assert ctx.dense_stats() == dict(voxels=ref.voxels, max_voxels=1 << 14, integrations=k + 1, slots=1 << 15)
        _check(ctx, ref)
    all_ = _check(ctx, ref, 1)
    some = _check(ctx, ref, 2)
    assert 0 < len(some["key"]) < len(all_["key"]) and len(set(all_["scan"].tolist())) == 3
    assert len(_check(ctx, ref, 1 << 30)["key"]) == 0
    assert R.same(R.sort_download(ctx.dense_download(0), 0.5), all_) is None  # 0 is taken as 1


# ------------------------------------------------------------------ 2. contention and spread
def test_one_voxel_and_one_voxel_per_point(fmx_mod):
    T = _pose(_rot("x", 0.2), (1000.0, 1000.0, 1000.0))  # every world coordinate in (0, 4096)
    a, b = _points("odd", 0), _points("odd", 1)
    ctx = _ctx(fmx_mod, _geo("odd"))
    ctx.dense_configure(True, 4096.0, 4096)
    ref = R.DenseRef(4096.0, 4096)
    for k, p in enumerate((a, b)):
        assert ctx.dense_integrate(_arg(p, k == 1), T, 50 + k) == ref.integrate(p, T, 50 + k)
    d = ctx.dense_download()
    valid = [int((R.classify(p, T, 4096.0, 1.0, 1e4)[0] == 0).sum()) for p in (a, b)]
    first = int(np.flatnonzero(R.classify(a, T, 4096.0, 1.0, 1e4)[0] == 0)[0])
    assert min(valid) > 500
    assert d["hits"].tolist() == [valid[0] + valid[1]] and d["scan"].tolist() == [50] and d["index"].tolist() == [first]
    _check(ctx, ref)
    # 1 mm voxels: every valid point its own
    ctx = _ctx(fmx_mod, _geo("odd"))
    ctx.dense_configure(True, 1e-3, 4096)
    ref = R.DenseRef(1e-3, 4096)
    got = ctx.dense_integrate(a, POSES[0], 1)
    assert got == ref.integrate(a, POSES[0], 1) and got["added"] == valid[0] and got["merged"] == 0
    assert (_check(ctx, ref)["hits"] == 1).all()


# ------------------------------------------------------------------ 3. boundaries
def test_boundaries(fmx_mod):
    I = np.eye(3, 4)
    f32 = np.float32
    rows = []
    for k in range(-8, 9):  # coordinates exactly k * 0.25 on both sides of 0, in x and in z
        rows.append((k * 0.25, 3.0, 0.0))
        rows.append((3.0, 0.0, k * 0.25))
    two, hundred = f32(2.0), f32(100.0)
    gate = [(np.nextafter(two, f32(0)), 0, 0), (two, 0, 0), (np.nextafter(two, f32(3)), 0, 0),  # r2 around min2 = 4
            (0, np.nextafter(hundred, f32(0)), 0), (0, hundred, 0), (0, np.nextafter(hundred, f32(200)), 0)]  # max2 = 1e4
    bad = [(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (0, 0, 0), (-0.0, 0.0, -0.0)]
    p = np.zeros((len(rows) + len(gate) + len(bad), 4), np.float32)
    p[:, :3] = np.array(rows + gate + bad, np.float32)
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 0.25, 1024, min_norm_squared=4.0, max_norm_squared=1e4)
    ref = R.DenseRef(0.25, 1024, 4.0, 1e4)
    got = ctx.dense_integrate(p, I, 0)
    assert got == ref.integrate(p, I, 0)
    assert got == dict(added=len(rows) + 2, merged=0, gated=4, out_of_range=0, invalid=5)
    m = _check(ctx, ref)
    # floor, not truncation: the x coordinates -0.25 and 0.25 are three different voxels with 0's
    cx = sorted(int(k) >> 42 for k, q in zip(m["key"], m["points"]) if q[1] == 3.0)
    assert cx == [R.BIAS + k for k in range(-8, 9)]
    # far points and the edge of the key range, voxel width 1
    L = float((1 << 20) - 2)
    far = np.zeros((8, 4), np.float32)
    far[:, :3] = [(1e7, 0, 0), (0, -1e7, 0), (L, 5, 5), (-L, 5, 5), (5, 5, L), (L + 1, 5, 5), (5, -L - 0.5, 5),
                  (5, 5, -L)]
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 1024, min_norm_squared=1.0, max_norm_squared=1e15)
    ref = R.DenseRef(1.0, 1024, 1.0, 1e15)
    got = ctx.dense_integrate(far, I, 3)
    assert got == ref.integrate(far, I, 3)
    assert got == dict(added=4, merged=0, gated=0, out_of_range=4, invalid=0)
    _check(ctx, ref)


# ------------------------------------------------------------------ 4. probing
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


def _centres(cxs):
    p = np.zeros((len(cxs), 4), np.float32)
    p[:, 0] = np.array(cxs, np.float64) + 0.5  # exact in fp32 (< 2^23)
    p[:, 1] = p[:, 2] = 0.5
    return p


def test_probing_collisions_wrap_and_full_table(fmx_mod):
    last, zero = _colliders()
    I = np.eye(3, 4)
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 1024, min_norm_squared=0.1, max_norm_squared=1e12)
    ref = R.DenseRef(1.0, 1024, 0.1, 1e12)
    assert ctx.dense_stats()["slots"] == 2048
    # the four of slot 2047 probe past the end of the table into the slots the four of slot 0 want; each twice
    first = _centres(last + zero + zero[::-1] + last[::-1])
    got = ctx.dense_integrate(first, I, 0)
    assert got == ref.integrate(first, I, 0) == dict(added=8, merged=8, gated=0, out_of_range=0, invalid=0)
    assert (_check(ctx, ref)["hits"] == 2).all()
    used = set(last + zero)
    rest = [cx for cx in range(300000, 302000) if cx not in used][:1016]
    for k, (a, b) in enumerate(((0, 500), (500, 900), (900, 1016))):
        chunk = _centres(rest[a:b])
        assert ctx.dense_integrate(_arg(chunk, k % 2 == 0), I, k + 1) == ref.integrate(chunk, I, k + 1)
    assert ctx.dense_stats()["voxels"] == ref.voxels == 1024
    _check(ctx, ref)
    # full by the rule: one more point is refused, a second look at old voxels too
    assert _status(fmx_mod, lambda: ctx.dense_integrate(_centres([5]), I, 9)) == OOM
    _check(ctx, ref)


# ------------------------------------------------------------------ 5. capacity
def test_capacity_refusal_is_the_rule_not_a_full_table(fmx_mod):
    a, b = _points("odd", 0), _points("odd", 1)
    big = R.DenseRef(2.0, 1 << 14)
    big.integrate(a, POSES[0], 0)
    v1 = big.voxels
    big.integrate(b, POSES[0], 1)
    assert v1 + len(b) > 1200 >= big.voxels  # refused by the rule although it would have fit
    ctx = _ctx(fmx_mod, _geo("odd"))
    ctx.dense_configure(True, 2.0, 1200)
    ref = R.DenseRef(2.0, 1200)
    assert ctx.dense_integrate(a, POSES[0], 0) == ref.integrate(a, POSES[0], 0)
    before = _check(ctx, ref)
    stats = ctx.dense_stats()
    assert ref.integrate(b, POSES[0], 1) is None
    assert _status(fmx_mod, lambda: ctx.dense_integrate(b, POSES[0], 1)) == OOM
    assert ctx.dense_stats() == stats
    assert R.same(_check(ctx, ref), before) is None
    # a smaller integration still goes in
    assert ctx.dense_integrate(b[:150], POSES[0], 2) == ref.integrate(b[:150], POSES[0], 2)
    _check(ctx, ref)


def test_capacity_refusal_never_fails_a_registration(fmx_mod):
    scans = _stream(2)
    n = len(scans[0])
    cap = n + 200
    ctx, off = _ctx(fmx_mod), _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, cap)
    big = R.DenseRef(1.0, 1 << 16)
    for k in range(2):
        assert ctx.register_scan(_arg(scans[k], True)) == off.register_scan(_arg(scans[k], True))
        assert np.array_equal(ctx.current_pose(), off.current_pose())
        big.integrate(scans[k], ctx.current_pose(), k)
        counts, integrated = ctx.dense_last()
        if k == 0:
            assert integrated == 1 and sum(counts.values()) == n and counts["added"] > 200
        else:
            assert integrated == -1 and sum(counts.values()) == 0
    assert big.voxels <= cap  # the refused scan would have fit physically
    assert ctx.dense_stats()["integrations"] == 1
    assert set(ctx.dense_download()["scan"].tolist()) == {0}


# ------------------------------------------------------------------ 6. clear, reuse, errors
def test_clear_reuse_and_error_paths(fmx_mod):
    fmx = fmx_mod
    ctx, other = _ctx(fmx, _geo("odd")), _ctx(fmx, _geo("odd"))
    p = _points("odd", 0)
    assert _status(fmx, lambda: ctx.dense_integrate(p, POSES[0], 0)) == STATE  # before configuration
    assert _status(fmx, ctx.dense_download) == STATE
    assert _status(fmx, ctx.dense_clear) == STATE
    assert ctx.dense_stats() == dict(voxels=0, max_voxels=0, integrations=0, slots=0)
    assert ctx.dense_last() == (dict(added=0, merged=0, gated=0, out_of_range=0, invalid=0), 0)
    for kw in (dict(voxel_width=0.0), dict(voxel_width=-1.0), dict(voxel_width=np.nan), dict(voxel_width=np.inf),
               dict(max_voxels=0), dict(max_voxels=(1 << 29) + 1), dict(min_norm_squared=-1.0, max_norm_squared=4.0),
               dict(min_norm_squared=4.0, max_norm_squared=4.0), dict(min_norm_squared=np.nan, max_norm_squared=4.0)):
        args = dict(voxel_width=0.5, max_voxels=4096)
        args.update(kw)
        assert _status(fmx, lambda: ctx.dense_configure(True, **args)) == INVAL, kw
    ctx.dense_configure(False, 0.5, 4096)  # configured, not enabled
    assert _status(fmx, lambda: ctx.dense_integrate(p, POSES[0], 0)) == STATE
    ctx.dense_configure(True, 0.5, 4096, every=0)
    other.dense_configure(True, 0.5, 4096)
    bad = POSES[0].copy()
    bad[1, 3] = np.inf
    assert _status(fmx, lambda: ctx.dense_integrate(p, bad, 0)) == INVAL
    assert ctx.dense_integrate(np.zeros((0, 4), np.float32), POSES[0], 5) == dict(added=0, merged=0, gated=0,
                                                                                 out_of_range=0, invalid=0)
    assert ctx.dense_stats()["integrations"] == 1
    ctx.dense_clear()
    assert ctx.dense_stats()["integrations"] == 0

    def sequence(c):
        ref = R.DenseRef(0.5, 4096)
        for k in range(2):
            q = _points("odd", k)
            assert c.dense_integrate(_arg(q, k == 1), POSES[k], SCAN_IDS[k]) == ref.integrate(q, POSES[k], SCAN_IDS[k])
        return _check(c, ref)

    first = sequence(ctx)
    ctx.dense_clear()
    assert ctx.dense_stats() == dict(voxels=0, max_voxels=4096, integrations=0, slots=8192)
    assert len(ctx.dense_download()["hits"]) == 0
    assert R.same(sequence(ctx), first) is None  # after a clear: the same map, seq from 0 again
    assert R.same(sequence(other), first) is None  # a fresh context: identical
    assert _status(fmx, lambda: ctx.dense_configure(True, 0.5, 4096)) == STATE  # after an integration
    # a short buffer: FMX_E_SIZE, nothing written
    m = len(first["key"])
    L = fmx.lib()
    pts, sc = np.full((m, 3), 7.0), np.full(m, 7, np.uint64)
    ix, hi = np.full(m, 7, np.uint32), np.full(m, 7, np.uint32)
    cap = C.c_uint32(m - 1)
    st = L.fmx_dense_download(ctx.h, C.c_uint32(1), fmx._p(pts), fmx._p(sc), fmx._p(ix), fmx._p(hi), C.byref(cap))
    assert st == SIZE
    assert (pts == 7.0).all() and (sc == 7).all() and (ix == 7).all() and (hi == 7).all()
    cap = C.c_uint32(m)  # only two of the four outputs
    assert L.fmx_dense_download(ctx.h, C.c_uint32(1), None, None, fmx._p(ix), fmx._p(hi), C.byref(cap)) == 0
    assert cap.value == m and sorted(hi.tolist()) == sorted(first["hits"].tolist()) and (pts == 7.0).all()


# ------------------------------------------------------------------ 7 / 8. the register path
XI0 = np.array([0.0, 0.0, 0.01, 0.15, 0.0, 0.0])
W_REG, CAP_REG, N_REG = 0.25, 1 << 16, 9


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
def _run(dense, every, deskew, feed):
    """One N_REG-scan stream.  feed: "device" / "host" scans one at a time, "announced" /
    "announced-host" through next_scan, "cloud" through register_cloud.  Returns the poses,
    twists, per-scan dense_last and the key-sorted download (None with the map off)."""
    from form_amd import fmx
    geo = synth.GEOMETRIES["tiny"]
    scans = _stream(N_REG)
    ctx = _ctx(fmx, geo, window=(4, 3))
    if deskew:
        ctx.deskew_configure(True, initial_twist=XI0)
    if feed == "cloud":
        ctx.organize_configure(True)
    if dense:
        ctx.dense_configure(True, W_REG, CAP_REG, every=every)
    on_device = feed in ("device", "announced")
    held = [_arg(s, on_device) for s in scans]
    poses, twists, lasts = [], [], []
    for k in range(N_REG):
        if feed == "cloud":
            ctx.register_cloud(*synth.to_cloud(scans[k], geo, 100 + k)[:2])
        else:
            if feed.startswith("announced") and k + 1 < N_REG:
                ctx.next_scan(held[k + 1])
            ctx.register_scan(held[k])
            if feed.startswith("announced"):
                assert ctx.last_stats()["pipelined"] == (1 if k > 0 else 0)
        poses.append(ctx.current_pose().copy())
        twists.append(ctx.deskew_last()[0].copy())
        lasts.append(ctx.dense_last())
    down = R.sort_download(ctx.dense_download(), W_REG) if dense else None
    stats = ctx.dense_stats() if dense else None
    ctx.close()
    return poses, twists, lasts, down, stats


CASES = [(1, False, "device"), (3, False, "device"), (1, False, "host"), (1, False, "announced"),
         (1, False, "announced-host"), (1, True, "device"), (3, True, "announced"), (1, True, "announced"),
         (1, False, "cloud"), (3, False, "cloud")]


@pytest.mark.parametrize("every,deskew,feed", CASES)
def test_register_path_equals_standalone_integrations(fmx_mod, every, deskew, feed):
    scans = _stream(N_REG)
    poses, twists, lasts, down, stats = _run(True, every, deskew, feed)
    other = _ctx(fmx_mod, synth.GEOMETRIES["tiny"])
    other.dense_configure(True, W_REG, CAP_REG)
    ref = R.DenseRef(W_REG, CAP_REG)
    for k in range(N_REG):
        counts, integrated = lasts[k]
        if k % every:
            assert integrated == 0 and sum(counts.values()) == 0, k
            continue
        # the scan the extractor saw: the deskewed one with deskewing on (redone stand-alone)
        seen = other.deskew(np.array(scans[k]), twists[k]) if deskew else scans[k]
        assert integrated == 1, k
        assert other.dense_integrate(seen, poses[k], k) == counts, k
        assert ref.integrate(seen, poses[k], k) == counts, k
    assert stats["integrations"] == len(range(0, N_REG, every)) and stats["voxels"] == ref.voxels
    assert R.same(down, R.sort_download(other.dense_download(), W_REG)) is None
    assert R.same(down, ref.sorted()) is None
    assert len(set(down["scan"].tolist())) > 1 and poses[-1][:, 3].any()


def test_register_path_pipelined_equals_sequential(fmx_mod):
    for deskew, feeds in ((True, ("device", "announced")), (False, ("device", "host", "announced", "announced-host"))):
        runs = [_run(True, 1, deskew, f) for f in feeds]
        for r in runs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(runs[0][0], r[0]))
            assert runs[0][2] == r[2]
            assert R.same(runs[0][3], r[3]) is None


@pytest.mark.parametrize("every,deskew,feed", [(1, False, "device"), (3, True, "announced"), (1, False, "announced-host"),
                                               (1, False, "cloud")])
def test_estimation_is_untouched(fmx_mod, every, deskew, feed):
    on, off = _run(True, every, deskew, feed), _run(False, 1, deskew, feed)
    assert len(on[0]) == N_REG
    for k in range(N_REG):
        assert np.array_equal(on[0][k].view(np.uint64), off[0][k].view(np.uint64)), k
        assert np.array_equal(on[1][k], off[1][k]), k
    assert all(l == (dict(added=0, merged=0, gated=0, out_of_range=0, invalid=0), 0) for l in off[2])


# ------------------------------------------------------------------ 9. profiling
def test_profile_counts_the_launches(fmx_mod):
    plain = _ctx(fmx_mod, _geo("odd"))
    plain.profile(True)
    assert list(plain.profile_read())[-2:] == ["deskew", "organize"]  # never configured: reads as before
    ctx = _ctx(fmx_mod, _geo("odd"))
    ctx.dense_configure(True, 0.5, 4096)
    ctx.profile(True)
    assert list(ctx.profile_read())[-3:] == ["deskew", "organize", "dense"]  # appended: earlier ids keep their index
    total = 0
    for k in range(3):
        p = _points("odd", k)[:1000 - 100 * k]
        ctx.dense_integrate(p, POSES[k], k)
        total += len(p)
    d = ctx.profile_read()["dense"]
    assert d["launches"] == 6 and d["bytes"] == total * (40 + 12)  # claim + fill per integration
    ctx.dense_integrate(np.zeros((0, 4), np.float32), POSES[0], 9)  # nothing to launch
    assert ctx.profile_read()["dense"]["launches"] == 6
    ctx.profile_reset()
    m = len(ctx.dense_download()["hits"])  # the sizing call counts, the filling call counts and appends
    d = ctx.profile_read()["dense"]
    assert d["launches"] == 3 and d["bytes"] == 2 * 8192 * 4 + 8192 * 8 + m * 68
    ctx.profile_reset()
    assert len(ctx.dense_download(1 << 30)["hits"]) == 0  # nothing qualifies: the count alone
    assert ctx.profile_read()["dense"]["launches"] == 1


# ------------------------------------------------------------------ 10. FORM
def test_form_dense_map_round_trip(fmx_mod):
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    scans = _stream(5)
    f = fmx_mod.FORM()
    f.set_lidar_params(lidar)
    assert len(f.dense_map()["hits"]) == 0
    f.set_dense_map(True, voxel_width=0.5, max_voxels=1 << 15, every=2)
    f.initialize()
    ref = R.DenseRef(0.5, 1 << 15)
    for k in range(5):
        f.add_lidar(scans[k][:, :3])
        if k % 2 == 0:
            ref.integrate(scans[k], f.pose()[:3], k)
    d = f.dense_map()
    assert sorted(d) == ["hits", "index", "points", "scan"]
    assert d["points"].dtype == np.float64 and d["scan"].dtype == np.uint64
    assert d["index"].dtype == np.uint32 and d["hits"].dtype == np.uint32
    assert R.same(R.sort_download(d, 0.5), ref.sorted()) is None
    assert R.same(R.sort_download(f.dense_map(3), 0.5), ref.sorted(3)) is None
    assert set(d["scan"].tolist()) == {0, 2, 4}

"""Probing the dense voxel map on the device (fmx_probe_points, fmx_probe_rays; DESIGN.md
§Dense map, Probing) against the restatement (tests/probe_ref.py).  Every comparison is
equality, doubles compared as bits: the restatement decides every point and every ray."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import carve_ref as CR
import dense_ref as R
import probe_ref as PR
import roll_ref as RR
from form_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = {"odd": (5, 200), "tiny": (16, 256)}
INVAL, STATE, RANGE = 1, 5, 6
AHEAD = 4  # FMX_PROBE_AHEAD's default
I34 = np.eye(3, 4)
HALF = (0.5, 0.5, 0.5)
BOTH = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
RAY_FIELDS = ("state", "step", "t", "points", "scan", "index", "hits", "misses")


def _geo(name):
    r, c = SHAPES[name]
    return synth.ScanGeometry(r, c, 15.0, 0.01, 0.02)


def _ctx(fmx, geo=None):
    p = synth.default_params(geo or _geo("tiny"))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _pair(fmx, w, cap, gate=CR.SPECIAL_GATE, geo=None, carve=None):
    """A context with the dense map on (and carving, with carve = its parameters), and its restatement."""
    ctx = _ctx(fmx, geo)
    ctx.dense_configure(True, w, cap, min_norm_squared=gate[0], max_norm_squared=gate[1])
    ref = PR.ProbeRef(w, cap, gate[0], gate[1])
    if carve is not None:
        ctx.carve_configure(**carve)
        ref.carve_configure(**carve)
    assert 128 <= ctx.dense_stats()["slots"] <= 8192 or cap > 4096
    return ctx, ref


def _arg(p, on_device):
    return torch.from_numpy(np.array(p)).to("cuda:0") if on_device else np.array(p)


def _integrate(ctx, ref, p, T=I34, idx=0, on_device=False):
    assert ctx.dense_integrate(_arg(p, on_device), T, idx) == ref.integrate(p, T, idx)


def _voxels(ctx, ref, voxels, idx=0, on_device=False):
    """One point at the centre of each voxel (width 1.0), on both."""
    if voxels:
        _integrate(ctx, ref, CR.voxel_centres(list(voxels), 1.0), I34, idx, on_device)


def _reset(ctx, ref):
    ctx.dense_clear()
    ref.clear()


def _points(ctx, ref, p, T, on_device=False, **kw):
    got, want = ctx.probe_points(_arg(p, on_device), T, **kw), ref.probe_points(p, T, **kw)
    assert PR.same(got, want) is None, (PR.same(got, want), kw)
    assert sum(got["counts"].values()) == len(p)
    return got


def _rays(ctx, ref, p, T, on_device=False, **kw):
    got, want = ctx.probe_rays(_arg(p, on_device), T, **kw), ref.probe_rays(p, T, **kw)
    assert PR.same(got, want) is None, (PR.same(got, want), kw)
    c = got["counts"]
    assert c["hit"] + c["clear"] + c["out_of_range"] + c["invalid"] == len(p)
    return got


def _status(fmx, fn):
    with pytest.raises(fmx.FmxError) as e:
        fn()
    return e.value.status


def _snapshot(ctx, w):
    return (CR.sort_download(ctx.dense_download(misses=True), w), ctx.dense_stats(), ctx.dense_last(), ctx.carve_last())


def _same_snapshot(a, b):
    return CR.same(a[0], b[0]) is None and a[1:] == b[1:]


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _pose(Rm, t):
    T = np.zeros((3, 4))
    T[:, :3] = Rm
    T[:, 3] = t
    return T


# (tests/test_gpu_carve.py's poses, and a fourth for the scan that is probed)
POSES = [_pose(_rot("z", 0.3), (-12.5, -3.25, -0.75)), _pose(_rot("x", 0.4) @ _rot("y", -0.7), (2.0, 1.0, 0.5)),
         _pose(_rot("y", 1.1) @ _rot("z", -2.0), (-0.3, 14.0, -2.0)), _pose(_rot("z", -0.8) @ _rot("x", 0.2), (1.5, 4.0, -0.25))]


@functools.lru_cache(maxsize=None)
def _scan(name, k):
    p = synth.raycast(synth.World(), synth.trajectory_pose(k), _geo(name), 4242 + k).numpy()
    p.setflags(write=False)
    return p


# ------------------------------------------------------------------ 1. special rays
def _special(name):
    o, p = next((o, p) for n, o, p in CR.SPECIAL if n == name)
    return o, p, PR.walk_tau(o, CR.special_end(o, p), 1.0)


@BOTH
def test_special_rays_one_voxel_at_a_time(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod, 1.0, 2048)
    for name, o, p in CR.SPECIAL:
        path, tin = PR.walk_tau(o, CR.special_end(o, p), 1.0)
        S, T, pt = len(path) - 1, CR.special_pose(o), CR.special_point(p)
        on_path = set(path)
        shell = {u for v in path for u in ((v[0], v[1] + 1, v[2]), (v[0], v[1], v[2] - 1))} - on_path
        _voxels(ctx, ref, sorted(shell))
        got = _rays(ctx, ref, pt, T, on_device)  # beside the path: never hit
        assert got["counts"] == dict(hit=0, clear=1, out_of_range=0, invalid=0, steps=S + 1), name
        assert got["step"][0] == PR.NO_STEP and got["t"][0] == PR.INF and got["state"][0] == PR.ABSENT
        _reset(ctx, ref)
        for s in range(S + 1):  # only v_s present, the end voxel (s = S) included
            _voxels(ctx, ref, [path[s]], idx=s)
            got = _rays(ctx, ref, pt, T, on_device)
            assert got["state"][0] == PR.SOLID and got["step"][0] == s, (name, s)
            assert np.float64(got["t"][0]).view(np.uint64) == np.float64(tin[s]).view(np.uint64), (name, s)
            assert got["counts"]["steps"] == s + 1 and got["scan"][0] == s and got["hits"][0] == 1
            assert R.pack_key(*path[s]) == int(R.key_of_points(got["points"], 1.0)[0])
            _reset(ctx, ref)
        _voxels(ctx, ref, sorted(on_path))  # the whole path: the first examined voxel ends the ray
        for skip in sorted({0, 1, S, S + 1}):
            got = _rays(ctx, ref, pt, T, on_device, skip=skip)
            if skip <= S:
                assert got["step"][0] == skip and got["counts"]["steps"] == 1 and got["t"][0] == tin[skip], (name, skip)
            else:
                assert got["counts"] == dict(hit=0, clear=1, out_of_range=0, invalid=0, steps=0), (name, skip)
        _reset(ctx, ref)
    assert _special("same-voxel")[2][0] == [(0, 0, 0)] and len(_special("tie")[2][0]) == 10
    assert len(_special("face")[2][0]) == 7 and _special("straddle")[2][0][0] == (-2, -1, 0)


# ------------------------------------------------------------------ 2. look-ahead edges
AXIS_RAYS = [((1, 0, 0), 3), ((-1, 0, 0), 4), ((0, 1, 0), 5), ((0, -1, 0), 7), ((0, 0, 1), 8), ((0, 0, -1), 9)]


@BOTH
def test_look_ahead_edges(fmx_mod, on_device):
    """Six axis rays from one origin, S = 3, 4, 5, 7, 8, 9, in one launch: the only solid voxel
    at AHEAD - 1, AHEAD, S - 1 or S (where the path is that long), then a second one right
    behind it, which is loaded ahead with the first and must not show anywhere."""
    ctx, ref = _pair(fmx_mod, 1.0, 2048)
    pts = np.zeros((6, 4), np.float32)
    for j, (d, S) in enumerate(AXIS_RAYS):
        pts[j, :3] = np.array(d) * S
    T = CR.special_pose(HALF)
    for kind in ("ahead-1", "ahead", "S-1", "S"):
        for behind in (False, True):
            at, vox = [], []
            for d, S in AXIS_RAYS:
                s = min({"ahead-1": AHEAD - 1, "ahead": AHEAD, "S-1": S - 1, "S": S}[kind], S)
                at.append(s)
                vox.append(tuple(s * c for c in d))
                if behind:
                    vox += [tuple(u * c for c in d) for u in range(s + 1, S + 1)]
            _voxels(ctx, ref, vox)
            got = _rays(ctx, ref, pts, T, on_device)
            assert got["step"].tolist() == at and (got["state"] == PR.SOLID).all(), (kind, behind)
            assert got["counts"] == dict(hit=6, clear=0, out_of_range=0, invalid=0, steps=sum(at) + 6), (kind, behind)
            _reset(ctx, ref)


# ------------------------------------------------------------------ 3. probe chains
def _lookup_voxels():
    """64 voxels (cx, 0, 0), 1 <= cx < 400, for a table of 128 slots: at least three of them
    home to one slot, so that chains run past the home slot; returns them, the occupied
    slots (linear probing: the set does not depend on the insertion order), each voxel's
    probe distance and the absent cx whose home slot is occupied (tests/test_gpu_carve.py's
    construction)."""
    home = {cx: R.home_slot(R.pack_key(cx, 0, 0), 128) for cx in range(1, 400)}
    by = {}
    for cx, h in home.items():
        by.setdefault(h, []).append(cx)
    crowd = max(by.values(), key=len)[:4]
    rest = [cx for cx in range(1, 400, 3) if cx not in crowd][:64 - len(crowd)]
    chosen = sorted(crowd + rest)
    occ, dist = set(), {}
    for cx in chosen:
        h, dist[cx] = home[cx], 0
        while h in occ:
            h, dist[cx] = (h + 1) & 127, dist[cx] + 1
        occ.add(h)
    absent = [cx for cx in range(1, 400) if cx not in chosen and home[cx] in occ]
    return chosen, occ, dist, absent


@BOTH
def test_lookup_follows_probe_chains_and_stops_at_an_empty_slot(fmx_mod, on_device):
    chosen, occ, dist, absent = _lookup_voxels()
    assert len(chosen) == 64 and len(occ) == 64 and max(dist.values()) >= 3 and len(absent) > 50
    ctx, ref = _pair(fmx_mod, 1.0, 64, (0.1, 1e12))
    assert ctx.dense_stats()["slots"] == 128
    # (four keys with one home slot: whatever order the lanes insert them in, one sits three slots on)
    _voxels(ctx, ref, [(cx, 0, 0) for cx in chosen])
    assert ctx.dense_stats()["voxels"] == 64
    got = _points(ctx, ref, CR.voxel_centres([(cx, 0, 0) for cx in chosen], 1.0), I34, on_device)
    assert (got["state"] == PR.SOLID).all() and got["index"].tolist() == list(range(64))
    got = _points(ctx, ref, CR.voxel_centres([(cx, 0, 0) for cx in absent], 1.0), I34, on_device)
    assert (got["state"] == PR.ABSENT).all() and not got["hits"].any()
    # along the row: the first present voxel, and from behind it the next one
    T, shot = CR.special_pose(HALF), np.array([[399.0, 0, 0, 0]], np.float32)
    got = _rays(ctx, ref, shot, T, on_device)
    assert got["step"][0] == chosen[0] and got["counts"]["steps"] == chosen[0] + 1
    got = _rays(ctx, ref, shot, T, on_device, skip=chosen[0] + 1)
    assert got["step"][0] == chosen[1] and got["counts"]["steps"] == chosen[1] - chosen[0]
    got = _rays(ctx, ref, shot, T, on_device, skip=chosen[-1] + 1)  # nothing behind the last one
    assert got["counts"] == dict(hit=0, clear=1, out_of_range=0, invalid=0, steps=399 - chosen[-1])
    # beside the row: absent voxels only, some of them with an occupied home slot
    got = _rays(ctx, ref, shot, CR.special_pose((0.5, 1.5, 0.5)), on_device)
    assert got["counts"] == dict(hit=0, clear=1, out_of_range=0, invalid=0, steps=400)


# ------------------------------------------------------------------ 4. filter
@BOTH
def test_filter_by_hits_and_by_misses(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod, 1.0, 2048)
    T, shot = CR.special_pose(HALF), np.array([[7.0, 0, 0, 0]], np.float32)
    A, B = (3, 0, 0), (5, 0, 0)
    _voxels(ctx, ref, [B, B, A])  # A: one hit, B: two
    ctx.carve_configure(margin=0)  # from here on: the stand-alone carve below is the only one
    ref.carve_configure(margin=0)
    assert _rays(ctx, ref, shot, T, on_device)["step"][0] == 3
    got = _rays(ctx, ref, shot, T, on_device, min_hits=2)  # A is transparent
    assert got["step"][0] == 5 and got["hits"][0] == 2 and got["counts"]["steps"] == 6
    assert _rays(ctx, ref, shot, T, on_device, min_hits=3)["counts"]["clear"] == 1
    centres = CR.voxel_centres([A, B, (4, 0, 0)], 1.0)
    assert _points(ctx, ref, centres, I34, on_device, min_hits=2)["state"].tolist() == [1, 2, 0]
    # two rays through A (they end in the voxel behind it): A has 2 misses on 1 hit
    through = np.array([[4.0, 0, 0, 0], [4.25, 0, 0, 0]], np.float32)
    assert ctx.carve_rays(_arg(through, on_device), T) == ref.carve_rays(through, T)
    assert ref.misses == {R.pack_key(*A): 2}
    for ratio, step in ((1.0, 5), (1.99, 5), (2.0, 3), (None, 3)):
        got = _rays(ctx, ref, shot, T, on_device, max_miss_ratio=ratio)
        assert got["step"][0] == step and got["misses"][0] == (2 if step == 3 else 0), ratio
        st = _points(ctx, ref, centres, I34, on_device, max_miss_ratio=ratio)
        assert st["state"].tolist() == [2 if step == 3 else 1, 2, 0] and st["misses"].tolist() == [2, 0, 0], ratio
    # a map that never enabled carving: misses read 0 and every ratio admits
    plain, pref = _pair(fmx_mod, 1.0, 2048)
    _voxels(plain, pref, [B, B, A])
    for ratio in (0.0, 1.0, None):
        assert _rays(plain, pref, shot, T, on_device, max_miss_ratio=ratio)["step"][0] == 3
        assert _points(plain, pref, centres, I34, on_device, max_miss_ratio=ratio)["state"].tolist() == [2, 2, 0]


# ------------------------------------------------------------------ 5. classes and shapes
def _mixed():
    """1 + 64 * 5 + 3 points from the origin (0.5, 0.5, 0.5) at width 1.0: short rays, NaN / inf
    / zero points, an end voxel out of range, one 600-step ray, duplicates; and the voxels of
    the map they are cast through."""
    g = np.random.default_rng(3)
    n = 1 + 64 * 5 + 3
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = g.integers(-3, 4, (n, 3)) + g.choice([0.0, 0.25, -0.5], (n, 3))
    pts[:, 3] = g.normal(0, 1, n)  # w is never read
    pts[5, 0], pts[70, 1], pts[200, 2] = np.nan, np.inf, -np.inf
    pts[6, :3] = pts[130, :3] = 0.0
    pts[7, :3] = (2e6, 1.0, 1.0)      # end voxel out of range
    pts[8, :3] = (1.0, -1048576.0, 1.0)
    pts[150, :3] = (300.0, 200.0, 100.0)  # S = 600
    pts[151] = pts[150]
    pts[320:323] = pts[10:13]           # duplicates
    T = CR.special_pose(HALF)
    long_path = CR.walk(HALF, R.classify(pts[150:151], T, 1.0, *CR.SPECIAL_GATE)[1][0], 1.0)
    assert len(long_path) == 601
    near = {(int(v[0]), int(v[1]), int(v[2])) for v in g.integers(-3, 4, (60, 3)).tolist()} - set(long_path)
    return pts, T, sorted(near), long_path[590:601:5] + [long_path[600]]


def _raw_rays(fmx, ctx, pts, T, fields, fill=7, skip=0):
    """fmx_probe_rays with only `fields` of the outputs given, the others NULL; every given
    array prefilled.  Returns (status, outputs, counts)."""
    n = len(pts)
    A, vox = ctx._voxel_arrays(n, True)
    out = dict(vox, state=np.zeros(n, np.uint8), step=np.zeros(n, np.uint32), t=np.zeros(n))
    for v in out.values():
        v.fill(fill)
    for f, slot in (("points", "xyz"), ("scan", "scan"), ("index", "index"), ("hits", "hits"), ("misses", "misses")):
        if f not in fields:
            setattr(A, slot, None)
    ptr = lambda f: fmx._p(out[f]) if f in fields else None  # noqa: E731
    cnt = fmx._ProbeRayCounts()
    pose = np.ascontiguousarray(T, np.float64).reshape(12)
    p = np.ascontiguousarray(pts, np.float32)
    st = fmx.lib().fmx_probe_rays(ctx.h, fmx._p(p), C.c_size_t(n), C.c_int(0), fmx._p(pose), C.c_uint32(1), C.c_uint32(0),
                                  C.c_uint32(0), C.c_uint32(skip), ptr("state"), ptr("step"), ptr("t"),
                                  C.byref(A) if set(fields) & set(PR.VOXEL_FIELDS) else None, C.byref(cnt))
    return st, out, cnt.as_dict()


@BOTH
def test_classes_and_shapes_in_one_launch(fmx_mod, on_device):
    pts, T, near, far = _mixed()
    assert len(pts) == 324
    ctx, ref = _pair(fmx_mod, 1.0, 2048)
    _voxels(ctx, ref, near + far, idx=9)
    got = _rays(ctx, ref, pts, T, on_device)
    c = got["counts"]
    assert c["invalid"] == 5 and c["out_of_range"] == 2 and c["hit"] > 100 and c["clear"] > 20
    assert got["step"][150] == got["step"][151] == 590 and c["steps"] > 2 * 591
    assert got["state"][[5, 6, 7, 8]].tolist() == [4, 4, 3, 3] and (got["step"][[5, 6, 7, 8]] == PR.NO_STEP).all()
    assert all(np.array_equal(got[f][320:323], got[f][10:13]) for f in RAY_FIELDS)
    look = _points(ctx, ref, pts, T, on_device)
    assert look["counts"]["invalid"] == 5 and look["counts"]["out_of_range"] == 2 and look["state"][150] == PR.SOLID
    # one point, no point
    one = _rays(ctx, ref, pts[150:151], T, on_device)
    assert one["step"][0] == 590 and one["counts"]["steps"] == 591
    _points(ctx, ref, pts[150:151], T, on_device)
    none = np.zeros((0, 4), np.float32)
    assert _rays(ctx, ref, none, T, on_device)["counts"] == dict(hit=0, clear=0, out_of_range=0, invalid=0, steps=0)
    assert _points(ctx, ref, none, T, on_device)["counts"] == dict(absent=0, filtered=0, solid=0, out_of_range=0, invalid=0)


def test_null_outputs_are_skipped(fmx_mod):
    pts, T, near, far = _mixed()
    ctx, ref = _pair(fmx_mod, 1.0, 2048)
    _voxels(ctx, ref, near + far, idx=9)
    want = ref.probe_rays(pts, T)
    for fields in (RAY_FIELDS, ("state",), ("t",), ("step", "hits"), ("scan",), ("index", "points"), ("misses",), ()):
        st, out, counts = _raw_rays(fmx_mod, ctx, pts, T, fields)
        assert st == 0 and counts == want["counts"], fields
        assert PR.same(out, want, fields) is None, (fields, PR.same(out, want, fields))
        assert all((out[f] == 7).all() for f in RAY_FIELDS if f not in fields), fields
    # the lookup: only the state; only one voxel field; nothing but the counts
    L, p, pose = fmx_mod.lib(), np.ascontiguousarray(pts), np.ascontiguousarray(T).reshape(12)
    look = ref.probe_points(pts, T)
    for fields in (("state",), ("hits",), ("scan", "index"), ()):
        A, vox = ctx._voxel_arrays(len(pts), True)
        out = dict(vox, state=np.zeros(len(pts), np.uint8))
        for v in out.values():
            v.fill(7)
        for f, slot in (("points", "xyz"), ("scan", "scan"), ("index", "index"), ("hits", "hits"), ("misses", "misses")):
            if f not in fields:
                setattr(A, slot, None)
        cnt = fmx_mod._ProbePointCounts()
        assert L.fmx_probe_points(ctx.h, fmx_mod._p(p), C.c_size_t(len(p)), C.c_int(0), fmx_mod._p(pose), 1, 0, 0,
                                  fmx_mod._p(out["state"]) if "state" in fields else None,
                                  C.byref(A) if set(fields) & set(PR.VOXEL_FIELDS) else None, C.byref(cnt)) == 0
        assert cnt.as_dict() == look["counts"] and PR.same(out, look, fields) is None, fields
        assert all((out[f] == 7).all() for f in out if f not in fields), fields
    assert fmx_mod.lib().fmx_probe_rays(ctx.h, None, C.c_size_t(0), C.c_int(0), fmx_mod._p(pose), 1, 0, 0, 0, None, None, None,
                                        None, None) == 0


# ------------------------------------------------------------------ 6. read-only and repeatable
STREAM_CFG = {"odd": (0.5, dict(margin=1)), "tiny": (1.0, dict(margin=2, ray_stride=3, max_norm_squared=900.0))}
STREAM_ASK = (dict(), dict(max_miss_ratio=0.25), dict(min_hits=2))
STREAM_CAST = (dict(skip=1), dict(max_miss_ratio=0.25, skip=1), dict(min_hits=2, skip=3))


@functools.lru_cache(maxsize=None)
def _stream_ref(name):
    """The restatement after three scans integrated with carving, and its answers about the
    fourth at its pose (computed once, left unchanged)."""
    w, cfg = STREAM_CFG[name]
    ref = PR.ProbeRef(w, 1 << 14)
    ref.carve_configure(**cfg)
    for k in range(3):
        ref.integrate(_scan(name, k), POSES[k], k)
    p = _scan(name, 3)
    return ([ref.probe_points(p, POSES[3], **kw) for kw in STREAM_ASK], [ref.probe_rays(p, POSES[3], **kw) for kw in STREAM_CAST],
            ref.sorted())


@BOTH
@pytest.mark.parametrize("name", ["odd", "tiny"])
def test_streams_equal_the_restatement_repeat_and_change_nothing(fmx_mod, name, on_device):
    w, cfg = STREAM_CFG[name]
    ctx = _ctx(fmx_mod, _geo(name))
    ctx.dense_configure(True, w, 1 << 14, min_norm_squared=1.0, max_norm_squared=1e4)
    ctx.carve_configure(**cfg)
    for k in range(3):
        ctx.dense_integrate(_arg(_scan(name, k), on_device), POSES[k], k)
    want_points, want_rays, want_map = _stream_ref(name)
    before = _snapshot(ctx, w)
    assert CR.same(before[0], want_map) is None and before[0]["misses"].sum() > 0
    p = _arg(_scan(name, 3), on_device)
    for kw, want in zip(STREAM_ASK, want_points):
        got, again = ctx.probe_points(p, POSES[3], **kw), ctx.probe_points(p, POSES[3], **kw)
        assert PR.same(got, want) is None, (kw, PR.same(got, want))
        assert PR.same(got, again) is None
    for kw, want in zip(STREAM_CAST, want_rays):
        got, again = ctx.probe_rays(p, POSES[3], **kw), ctx.probe_rays(p, POSES[3], **kw)
        assert PR.same(got, want) is None, (kw, PR.same(got, want))
        assert PR.same(got, again) is None
    assert _same_snapshot(before, _snapshot(ctx, w))
    c = want_rays[0]["counts"]
    assert c["hit"] > 0 and c["clear"] > 0 and want_points[0]["counts"]["solid"] > 0 and want_points[0]["counts"]["absent"] > 0
    assert want_rays[1]["counts"]["steps"] >= c["steps"]  # a filter only lets rays go further


# ------------------------------------------------------------------ 7. after a roll
@BOTH
def test_after_a_roll(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod, 0.5, 1 << 12, (1.0, 1e4), geo=_geo("odd"))
    for k in range(2):
        _integrate(ctx, ref, _scan("odd", k), POSES[k], k, on_device)
    before = ref.sorted()
    centre, half = POSES[1][:, 3], (24, 24, 24)
    ev = ctx.roll_evict(centre, half)
    want_ev = ref.evict(centre, half)
    assert len(ev["hits"]) == len(want_ev["hits"]) > 0 and 0 < ref.voxels < len(before["key"])
    # one point in every voxel the map held: the stored representatives, seen from the identity
    q = np.zeros((len(before["key"]), 4), np.float32)
    q[:, :3] = (RR.unpack_keys(before["key"]).astype(np.float64) + 0.5) * 0.5
    got = _points(ctx, ref, q, I34, on_device)
    gone = np.isin(before["key"], want_ev["key"])
    assert (got["state"][gone] == PR.ABSENT).all() and (got["state"][~gone] == PR.SOLID).all()
    kept = {f: before[f][~gone] for f in ("points", "scan", "index", "hits")}
    for f in kept:  # bit for bit what the map held before the table was rebuilt
        assert np.array_equal(np.ascontiguousarray(got[f][~gone]).view(np.uint8), np.ascontiguousarray(kept[f]).view(np.uint8)), f
    # rays from the centre to every one of them: a kept voxel's ends in a solid voxel, an evicted
    # one's in a kept voxel on its way or nowhere (the centres are a quarter voxel from any face,
    # far more than the fp32 rounding of the sensor-frame point)
    to = q.copy()
    to[:, :3] = (q[:, :3].astype(np.float64) - centre).astype(np.float32)
    cast = _rays(ctx, ref, to, _pose(np.eye(3), centre), on_device)
    hit = cast["state"] == PR.SOLID
    assert hit[~gone].all() and ((cast["state"] == PR.ABSENT) | hit).all()
    assert not np.isin(R.key_of_points(cast["points"][hit], 0.5), want_ev["key"]).any()


# ------------------------------------------------------------------ 8. the scenario on the device
@BOTH
def test_dynamic_object_scenario(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod, CR.SCN_W, CR.SCN_CAP, (1.0, 1e4), carve=dict(margin=1))
    for k in range(CR.SCN_SCANS):
        _integrate(ctx, ref, CR.scenario_scan(k), I34, k, on_device)
    rays = CR.scenario_scan(CR.SCN_SCANS - 1)
    PR.check_scenario(lambda ratio: _rays(ctx, ref, rays, I34, on_device, max_miss_ratio=ratio))
    box = _points(ctx, ref, CR.scenario_scan(0)[PR.scenario_middle()], I34, on_device, max_miss_ratio=0.5)
    assert (box["state"] == PR.FILTERED).all() and (box["misses"] >= 3).all()
    assert (_points(ctx, ref, rays, I34, on_device, max_miss_ratio=0.5)["state"] == PR.SOLID).all()


# ------------------------------------------------------------------ 9. off means off
def test_never_probing_reads_as_before_and_a_probe_is_one_launch(fmx_mod):
    ctx = _ctx(fmx_mod, _geo("odd"))
    ctx.dense_configure(True, 0.5, 1 << 12)
    ctx.profile(True)
    for k in range(2):
        ctx.dense_integrate(_scan("odd", k), POSES[k], k)
    prof = ctx.profile_read()
    assert list(prof)[-1] == "dense" and "carve" not in prof
    assert prof["dense"]["launches"] == 4  # claim + fill, twice: as before
    ctx.dense_download()
    base = ctx.profile_read()["dense"]["launches"]
    ctx.probe_points(_scan("odd", 2), POSES[2])
    assert ctx.profile_read()["dense"]["launches"] == base + 1
    ctx.probe_rays(_scan("odd", 2), POSES[2], skip=1)
    prof = ctx.profile_read()
    assert prof["dense"]["launches"] == base + 2 and list(prof)[-1] == "dense" and "carve" not in prof
    ctx.probe_rays(np.zeros((0, 4), np.float32), POSES[2])  # no points: nothing launched
    assert ctx.profile_read()["dense"]["launches"] == base + 2


# ------------------------------------------------------------------ 10. status codes, FORM
def test_status_codes(fmx_mod):
    fmx, L = fmx_mod, fmx_mod.lib()
    ctx = _ctx(fmx, _geo("odd"))
    p0 = _scan("odd", 0)
    assert _status(fmx, lambda: ctx.probe_points(p0, POSES[0])) == STATE  # before fmx_dense_configure
    assert _status(fmx, lambda: ctx.probe_rays(p0, POSES[0])) == STATE
    ctx.dense_configure(True, 1.0, 2048)
    ctx.dense_integrate(p0, POSES[0], 0)
    for k, bad in ((3, np.inf), (0, np.nan), (11, -np.inf)):
        T = POSES[0].copy()
        T.reshape(12)[k] = bad
        assert _status(fmx, lambda: ctx.probe_points(p0, T)) == INVAL
        assert _status(fmx, lambda: ctx.probe_rays(p0, T)) == INVAL
    pose = np.ascontiguousarray(POSES[0]).reshape(12)
    pc, rc = fmx._ProbePointCounts(), fmx._ProbeRayCounts()
    assert L.fmx_probe_points(ctx.h, None, C.c_size_t(5), C.c_int(0), fmx._p(pose), 1, 0, 0, None, None, C.byref(pc)) == INVAL
    assert L.fmx_probe_rays(ctx.h, None, C.c_size_t(5), C.c_int(0), fmx._p(pose), 1, 0, 0, 0, None, None, None, None,
                            C.byref(rc)) == INVAL
    assert L.fmx_probe_points(ctx.h, fmx._p(p0), C.c_size_t(5), C.c_int(0), None, 1, 0, 0, None, None, C.byref(pc)) == INVAL
    assert L.fmx_probe_points(ctx.h, None, C.c_size_t(0), C.c_int(0), fmx._p(pose), 1, 0, 0, None, None, C.byref(pc)) == 0
    assert pc.as_dict() == dict(absent=0, filtered=0, solid=0, out_of_range=0, invalid=0)
    # the origin's voxel out of range: FMX_E_RANGE for the cast and nothing written; the lookup does not care
    far = CR.special_pose((float(1 << 20), 0.5, 0.5))
    near = CR.special_pose((float((1 << 20) - 2) + 0.5, 0.5, 0.5))
    shot = np.array([[-5.0, 0, 0, 0], [-6.0, 0, 0, 0]], np.float32)
    st, out, counts = _raw_rays(fmx, ctx, shot, far, RAY_FIELDS, fill=9)
    assert st == RANGE and all((v == 9).all() for v in out.values())
    assert _status(fmx, lambda: ctx.probe_rays(shot, far)) == RANGE
    st, out, counts = _raw_rays(fmx, ctx, shot, near, RAY_FIELDS, fill=9)
    assert st == 0 and counts == dict(hit=0, clear=2, out_of_range=0, invalid=0, steps=6 + 7)
    assert ctx.probe_points(shot, far)["counts"]["absent"] == 2
    assert ctx.probe_points(np.array([[5.0, 0, 0, 0]], np.float32), far)["counts"]["out_of_range"] == 1


@functools.lru_cache(maxsize=None)
def _reg_stream():
    world = synth.World()
    out = []
    for k in range(4):
        s = synth.make_scan_skewed("tiny", k, world=world)[0].numpy()
        s.setflags(write=False)
        out.append(s)
    return out


def test_form_dense_lookup_and_cast_round_trip(fmx_mod):
    import types
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    scans = _reg_stream()
    f = fmx_mod.FORM()
    f.set_lidar_params(lidar)
    with pytest.raises(RuntimeError):
        f.dense_lookup(scans[0])  # the dense map is off
    f.set_dense_carve(True, max_range_m=20.0, margin=1, ray_stride=4)
    f.set_dense_map(True, voxel_width=0.5, max_voxels=1 << 15)
    f.initialize()
    ref = PR.ProbeRef(0.5, 1 << 15)
    ref.carve_configure(True, 400.0, 1, 4, 1)
    for k in range(3):
        f.add_lidar(scans[k][:, :3])
        ref.integrate(scans[k], f.pose()[:3], k)
    q = scans[3][::7]
    T = f.pose()[:3]
    for kw in (dict(), dict(min_hits=2, max_miss_ratio=0.25)):
        assert PR.same(f.dense_lookup(q, **kw), ref.probe_points(q, T, **kw)) is None, kw
        assert PR.same(f.dense_cast(q[:, :3], skip=1, **kw), ref.probe_rays(q, T, skip=1, **kw)) is None, kw
    other = POSES[1]
    got, want = f.dense_cast(q, pose=other), ref.probe_rays(q, other)
    assert PR.same(got, want) is None and want["counts"]["hit"] > 0
    assert PR.same(f.dense_lookup(q, pose=_pose44(other)), ref.probe_points(q, other)) is None


def _pose44(T):
    out = np.eye(4)
    out[:3] = T
    return out

"""The nearest solid voxel of the dense map on the device (fmx_nearest_voxels; DESIGN.md §Dense
map, Nearest) against the restatement (tests/nearest_ref.py), a brute-force loop over the whole
cube.  Every comparison is equality, doubles compared as bits; `lookups`, which depends on what
the kernel may skip, is held between the restatement's two bounds in every case."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

import carve_ref as CR
import dense_ref as R
import nearest_ref as NR
import probe_ref as PR
import upload_ref as UR
from form_amd import synth

pytestmark = pytest.mark.gpu

INVAL, STATE = 1, 5
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
BOTH = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
FIELDS = ("state", "dist2", "points", "scan", "index", "hits", "misses")


class Ref(NR.NearestRef, UR.UploadRef):
    """The restatement with upload() as well (both only add methods to ProbeRef)."""


def _pts(rows):
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return p


def _ctx(fmx, geo=None):
    p = synth.default_params(geo or synth.ScanGeometry(16, 256, 15.0, 0.01, 0.02))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _pair(fmx, w=1.0, cap=2048, gate=GATE, carve=None):
    """tests/test_gpu_probe.py's: a context with the dense map on (and carving, with carve = its
    parameters), and its restatement."""
    ctx = _ctx(fmx)
    ctx.dense_configure(True, w, cap, min_norm_squared=gate[0], max_norm_squared=gate[1])
    ref = Ref(w, cap, gate[0], gate[1])
    if carve is not None:
        ctx.carve_configure(**carve)
        ref.carve_configure(**carve)
    assert 128 <= ctx.dense_stats()["slots"] <= 8192
    return ctx, ref


def _arg(p, on_device):
    return torch.from_numpy(np.array(p)).to("cuda:0") if on_device else np.array(p)


def _integrate(ctx, ref, p, T=I34, idx=0):
    assert ctx.dense_integrate(np.array(p), T, idx) == ref.integrate(p, T, idx)


def _reps(ctx, ref, rows, first=0):
    """One integration per representative (fp32 points at the identity pose: stored exactly)."""
    for k, r in enumerate(rows):
        _integrate(ctx, ref, _pts([r]), I34, first + k)


def _near(ctx, ref, p, T, on_device=False, max_dist2=None, **kw):
    """The device's answer, equal to the restatement's; max_dist2: the squared limit as given,
    through the C entry point's own argument (the wrapper squares a distance)."""
    if max_dist2 is None:
        got = ctx.nearest_voxels(_arg(p, on_device), T, **kw)
        want = ref.nearest_voxels(p, T, **kw)
    else:
        got = _raw(ctx, p, T, FIELDS, max_dist2=max_dist2, **kw)
        want = ref.nearest_voxels(p, T, max_dist2=max_dist2, **kw)
    assert NR.same(got, want) is None, (NR.same(got, want), kw)
    c, (lo, hi) = got["counts"], want["lookups_bounds"]
    assert c["found"] + c["none"] + c["out_of_range"] + c["invalid"] == len(p)
    assert lo <= c["lookups"] <= hi, (lo, c["lookups"], hi)
    return got


_FMX = {}


def _raw(ctx, pts, T, fields, reach=1, max_dist2=math.inf, min_hits=1, fill=7, n=None, null_points=False, null_pose=False,
         status=False):
    """fmx_nearest_voxels itself, with only `fields` of the outputs given and every given array
    prefilled.  Returns the result dict, or the status with status=True."""
    fmx = _FMX["mod"]
    m = len(pts) if n is None else n
    A, vox = ctx._voxel_arrays(len(pts), True)
    out = dict(vox, state=np.zeros(len(pts), np.uint8), dist2=np.zeros(len(pts)))
    for v in out.values():
        v.fill(fill)
    for f, slot in (("points", "xyz"), ("scan", "scan"), ("index", "index"), ("hits", "hits"), ("misses", "misses")):
        if f not in fields:
            setattr(A, slot, None)
    ptr = lambda f: fmx._p(out[f]) if f in fields else None  # noqa: E731
    cnt = fmx._NearestCounts()
    pose = np.ascontiguousarray(T, np.float64).reshape(12)
    p = np.ascontiguousarray(pts, np.float32)
    st = fmx.lib().fmx_nearest_voxels(ctx.h, None if null_points or not len(p) else fmx._p(p), C.c_size_t(m), C.c_int(0),
                                      None if null_pose else fmx._p(pose), C.c_uint32(min_hits), C.c_uint32(0), C.c_uint32(0),
                                      C.c_uint32(reach), C.c_double(max_dist2), ptr("state"), ptr("dist2"),
                                      C.byref(A) if set(fields) & set(PR.VOXEL_FIELDS) else None, C.byref(cnt))
    if status:
        return st, out
    assert st == 0
    return dict(out, counts=cnt.as_dict())


@pytest.fixture(autouse=True)
def _module(fmx_mod):
    _FMX["mod"] = fmx_mod


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


# ------------------------------------------------------------------ 1. shapes and reaches
@functools.lru_cache(maxsize=None)
def _few_dozen():
    """40 representatives in a 5^3 region and 257 queries around it, some invalid."""
    g = np.random.default_rng(23)
    reps = _pts(g.uniform(-2.5, 2.5, (40, 3)))
    q = _pts(g.uniform(-4.0, 4.0, (257, 3)))
    q[:, 3] = g.normal(0, 1, 257)  # w is never read
    q[3, 0], q[64, 2] = np.nan, np.inf
    q[100, :3] = 0.0
    reps.setflags(write=False)
    q.setflags(write=False)
    return reps, q


@BOTH
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_group_wave_and_block_edges(fmx_mod, n, on_device):
    reps, q = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    for reach in (1, 2):
        got = _near(ctx, ref, q[:n], I34, on_device, reach=reach)
        if n >= 63:
            assert got["counts"]["found"] > n // 4
    if n == 0:
        assert got["counts"] == dict(found=0, none=0, out_of_range=0, invalid=0, lookups=0)
    if n == 257:
        assert got["counts"]["invalid"] == 3 and got["counts"]["none"] > 0
        near = _near(ctx, ref, q, I34, on_device, reach=2, max_dist=1.25)
        assert 0 < near["counts"]["found"] < got["counts"]["found"]


@BOTH
def test_reach_0_is_the_lookup_and_reach_8_the_whole_cube(fmx_mod, on_device):
    reps, q = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    _integrate(ctx, ref, reps[:20], I34, 1)  # two hits in half of them
    for min_hits in (1, 2):
        got = _near(ctx, ref, q, I34, on_device, reach=0, min_hits=min_hits)
        look = ctx.probe_points(_arg(q, on_device), I34, min_hits=min_hits)
        solid = look["state"] == PR.SOLID
        assert np.array_equal(got["state"] == PR.SOLID, solid) and solid.any()
        assert got["counts"]["lookups"] == got["counts"]["found"] + got["counts"]["none"]
        for f in PR.VOXEL_FIELDS:  # the lookup's solid answers, field for field; zeros elsewhere
            assert np.array_equal(got[f][solid], look[f][solid]) and not got[f][~solid].any(), f
    far = _pts([(-9.5, 0.5, 0.5), (0.5, 9.25, 0.5), (7.5, 7.5, -7.5), (0.5, 0.5, 0.5), (10.5, 0.5, 0.5), (-6.5, -7.5, 8.5),
                (3.5, -9.5, 1.5), (-11.5, -11.5, -11.5)])
    got = _near(ctx, ref, far, I34, on_device, reach=8)
    assert got["counts"]["found"] >= 5 and got["state"][7] == PR.ABSENT  # more than 8 cells away on every axis
    assert got["counts"]["lookups"] <= 8 * 4913


def test_more_points_than_one_pass_of_the_grid(fmx_mod):
    """The grid is capped at 2048 blocks of 256 lanes and strides beyond: 140 001 points are more
    than one pass at the default 4 lanes per point (and at 8, 16, ...), the last one partial; 4096
    are a single pass up to 64 lanes.  Reach 0 against the restatement; reach 2
    against the device's own answers on pieces of a single pass each, which the other tests
    hold against the restatement."""
    reps, _ = _few_dozen()
    g = np.random.default_rng(77)
    n = 2 * 2048 * 256 // 8 + 8929
    q = _pts(g.uniform(-4.0, 4.0, (n, 3)))
    q[[5, 70000, n - 1], 0] = np.nan
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    assert n == 140001 and _near(ctx, ref, q, I34, reach=0)["counts"]["invalid"] == 3
    got = ctx.nearest_voxels(q, I34, reach=2, max_dist=1.5)
    parts = [ctx.nearest_voxels(q[a:a + 4096], I34, reach=2, max_dist=1.5) for a in range(0, n, 4096)]
    for f in FIELDS:
        assert np.array_equal(got[f], np.concatenate([p[f] for p in parts])), f
    assert got["counts"] == {k: sum(p["counts"][k] for p in parts) for k in got["counts"]}
    assert got["counts"]["found"] > n // 4 and got["counts"]["none"] > 0 and got["counts"]["invalid"] == 3


# ------------------------------------------------------------------ 2. shells
@BOTH
def test_a_nearer_voxel_in_a_farther_shell(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod)
    _reps(ctx, ref, [(0.999, 1.7, 0.5), (2.0, 0.5, 0.5)])
    q = _pts([(0.999, 0.5, 0.5)])
    one, two = _near(ctx, ref, q, I34, on_device, reach=1), _near(ctx, ref, q, I34, on_device, reach=2)
    assert one["scan"][0] == 0 and two["scan"][0] == 1 and 1.0 < two["dist2"][0] < 1.0041 < one["dist2"][0]
    # the mirror: the best well inside shell 1, a decoy in shell 3; a stop after shell 1 is allowed
    ctx, ref = _pair(fmx_mod)
    _reps(ctx, ref, [(1.25, 0.5, 0.5), (3.5, 0.5, 0.5)])
    for reach in (1, 3, 8):
        got = _near(ctx, ref, _pts([(0.5, 0.5, 0.5)]), I34, on_device, reach=reach)
        assert got["scan"][0] == 0 and got["dist2"][0] == 0.5625, reach


@BOTH
def test_ties_go_to_the_smaller_key(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod)
    _reps(ctx, ref, [(1.0, 1.75, 1.75), (0.5, 1.25, 2.25)])
    q = _pts([(0.25, 0.25, 0.25)])
    got = _near(ctx, ref, q, I34, on_device, reach=2)
    assert got["dist2"][0] == 81 / 16 and got["scan"][0] == 1  # cell (0, 1, 2): shell 2, the smaller key
    assert R.pack_key(0, 1, 2) == int(R.key_of_points(got["points"], 1.0)[0]) < R.pack_key(1, 1, 1)
    assert _near(ctx, ref, q, I34, on_device, reach=1)["scan"][0] == 0
    # inside one shell: two mirror images about the query
    ctx, ref = _pair(fmx_mod)
    _reps(ctx, ref, [(1.75, 0.5, 0.5), (-0.75, 0.5, 0.5)])
    got = _near(ctx, ref, _pts([(0.5, 0.5, 0.5)]), I34, on_device, reach=1)
    assert got["dist2"][0] == 1.5625 and got["scan"][0] == 1


# ------------------------------------------------------------------ 3. filter
@BOTH
def test_filter_by_hits_and_by_misses(fmx_mod, on_device):
    A, B = (1.5, 0.5, 0.5), (0.5, 2.5, 0.5)  # A nearer with one hit, B farther with two
    q = _pts([(0.5, 0.5, 0.5)])
    ctx, ref = _pair(fmx_mod)
    _reps(ctx, ref, [B, B, A])
    ctx.carve_configure(margin=0)  # from here on: the stand-alone carve below is the only one
    ref.carve_configure(margin=0)
    assert _near(ctx, ref, q, I34, on_device, reach=2)["dist2"][0] == 1.0
    got = _near(ctx, ref, q, I34, on_device, reach=2, min_hits=2)
    assert got["dist2"][0] == 4.0 and got["hits"][0] == 2
    assert _near(ctx, ref, q, I34, on_device, reach=2, min_hits=3)["state"][0] == PR.ABSENT
    # two rays through A's voxel (1, 0, 0), ending behind it: A has 2 misses on 1 hit
    T, through = CR.special_pose((0.5, 0.5, 0.5)), _pts([(2.0, 0, 0), (2.25, 0, 0)])
    assert ctx.carve_rays(_arg(through, on_device), T) == ref.carve_rays(through, T)
    assert ref.misses == {R.pack_key(1, 0, 0): 2}
    for ratio, d2 in ((1.0, 4.0), (1.99, 4.0), (2.0, 1.0), (None, 1.0)):
        got = _near(ctx, ref, q, I34, on_device, reach=2, max_miss_ratio=ratio)
        assert got["dist2"][0] == d2 and got["misses"][0] == (2 if d2 == 1.0 else 0), ratio
    # a map that never enabled carving: misses read 0 and every ratio admits
    plain, pref = _pair(fmx_mod)
    _reps(plain, pref, [B, B, A])
    for ratio in (0.0, 1.0, None):
        assert _near(plain, pref, q, I34, on_device, reach=2, max_miss_ratio=ratio)["dist2"][0] == 1.0


# ------------------------------------------------------------------ 4. the limit
def test_max_dist2_below_at_and_above_the_winner(fmx_mod):
    ctx, ref = _pair(fmx_mod)
    _reps(ctx, ref, [(1.3, 0.6, 0.2), (0.5, 2.5, 0.5)])
    q = _pts([(0.4, 0.5, 0.5)])
    d2 = float(_near(ctx, ref, q, I34, reach=2)["dist2"][0])
    assert 0.9 < d2 < 1.0
    below = _near(ctx, ref, q, I34, reach=2, max_dist2=float(np.nextafter(d2, 0.0)))
    assert below["state"][0] == PR.ABSENT and below["dist2"][0] == NR.INF and not below["points"].any()
    for md2 in (d2, float(np.nextafter(d2, 2.0)), math.inf):  # "at" is admitted
        got = _near(ctx, ref, q, I34, reach=2, max_dist2=md2)
        assert got["state"][0] == PR.SOLID and got["dist2"][0] == d2 and got["scan"][0] == 0
    co = _pts([(1.3, 0.6, 0.2), (1.3, 0.6, 0.25)])  # coincident; the same voxel but not coincident
    got = _near(ctx, ref, co, I34, reach=1, max_dist2=0.0)
    assert got["state"].tolist() == [PR.SOLID, PR.ABSENT] and got["dist2"][0] == 0.0
    # the wrapper squares a distance, None is no limit
    assert _near(ctx, ref, q, I34, reach=2, max_dist=math.sqrt(d2) * 1.01)["state"][0] == PR.SOLID
    assert _near(ctx, ref, q, I34, reach=2, max_dist=0.5)["state"][0] == PR.ABSENT


# ------------------------------------------------------------------ 5. pose, domain edge, classes
@BOTH
def test_rotated_pose_and_narrow_voxels(fmx_mod, on_device):
    g = np.random.default_rng(5)
    T = _pose(_rot("z", 0.3) @ _rot("x", -0.4), (-12.5, 3.25, 0.75))
    ctx, ref = _pair(fmx_mod, 0.2)
    cloud = _pts(g.uniform(-1.0, 1.0, (200, 3)))
    _integrate(ctx, ref, cloud, T, 4)
    q = _pts(g.uniform(-1.2, 1.2, (150, 3)))
    other = _pose(_rot("y", 0.05) @ _rot("z", 0.31) @ _rot("x", -0.4), (-12.45, 3.2, 0.8))
    for pose in (T, other):
        for kw in (dict(reach=1), dict(reach=2, max_dist=0.3), dict(reach=3)):
            got = _near(ctx, ref, q, pose, on_device, **kw)
            assert got["counts"]["found"] > 30, kw
    same_place = _near(ctx, ref, cloud, T, on_device, reach=1)
    assert (same_place["state"] == PR.SOLID).all() and same_place["dist2"].max() < 3 * 0.2 ** 2


@BOTH
def test_domain_edge_and_point_classes(fmx_mod, on_device):
    e = float((1 << 20) - 2)
    ctx, ref = _pair(fmx_mod, gate=(1e-12, 1e13))  # (the integration's range gate: e^2 is 1.1e12)
    _reps(ctx, ref, [(e + 0.25, 0.5, 0.5), (e - 1.5, 1.5, 0.5), (e + 0.5, -e + 0.5, e + 0.75)])
    assert ref.voxels == 3
    q = _pts([(e + 0.75, 0.5, 0.5), (e + 0.5, 2.5, 0.5), (e + 0.5, -e + 0.25, e + 0.5), (e + 1.0, 0.5, 0.5),
              (np.nan, 1, 1), (1, np.inf, 1), (0, 0, 0), (0.5, 0.5, -e - 1.5), (5.5, 5.5, 5.5)])
    q[6, 3] = 5.0
    for reach in (1, 2, 8):
        got = _near(ctx, ref, q, I34, on_device, reach=reach)
        assert got["state"][[3, 4, 5, 6, 7]].tolist() == [3, 4, 4, 4, 3] and got["state"][8] == PR.ABSENT
        assert got["counts"]["out_of_range"] == 2 and got["counts"]["invalid"] == 3
        assert got["state"][0] == got["state"][2] == PR.SOLID and got["dist2"][0] == 0.25
    # part of the cube cannot be stored: fewer lookups than 4 whole cubes
    want = ref.nearest_voxels(q, I34, 2)
    assert want["lookups_bounds"] == (4, 3 * 5 * 5 + 3 * 5 * 5 + 3 * 3 * 3 + 125)
    assert got["state"][1] == PR.SOLID and got["dist2"][1] == 4.0625  # (reach 8; none within reach 1)
    assert _near(ctx, ref, q, I34, on_device, reach=1)["state"][1] == PR.ABSENT


# ------------------------------------------------------------------ 6. after an eviction and an upload
@BOTH
def test_after_an_eviction_and_an_upload(fmx_mod, on_device):
    g = np.random.default_rng(9)
    ctx, ref = _pair(fmx_mod, carve=dict(margin=1))
    _integrate(ctx, ref, _pts(g.uniform(-5.0, 5.0, (150, 3))), I34, 3)
    ev = ctx.roll_evict((0.5, 0.5, 0.5), (2, 2, 2), misses=True)
    want_ev = ref.evict((0.5, 0.5, 0.5), (2, 2, 2))
    assert len(ev["hits"]) == len(want_ev["hits"]) > 20 and ref.voxels > 0
    q = _pts(g.uniform(-5.0, 5.0, (100, 3)))
    left = _near(ctx, ref, q, I34, on_device, reach=2)
    assert 0 < left["counts"]["found"] and left["counts"]["none"] > 0
    up = dict(points=np.array([[7.25, 0.5, 0.5], [0.5, 0.25, 0.5], [0.5, 0.75, 0.5]]), scan=np.array([1 << 40, 77, 5], np.uint64),
              index=np.array([0xFFFFFFFF, 123456, 9], np.uint32), hits=np.array([3, 2, 4], np.uint32),
              misses=np.array([1, 0, 2], np.uint32))
    up["points"][1:, 0], up["points"][1:, 1] = 7.5, (3.25, 3.75)  # two entries of the absent voxel (7, 3, 0)
    assert ctx.dense_upload(**up) == ref.upload(**up) == dict(added=2, merged=1, out_of_range=0, invalid=0)
    got = _near(ctx, ref, _pts([(7.5, 0.5, 0.5), (7.5, 3.5, 0.5)]), I34, on_device, reach=1)
    assert got["scan"].tolist() == [1 << 40, 77] and got["index"].tolist() == [0xFFFFFFFF, 123456]
    assert got["hits"].tolist() == [3, 6] and got["misses"].tolist() == [1, 2] and got["dist2"].tolist() == [0.0625, 0.0625]
    again = _near(ctx, ref, q, I34, on_device, reach=2)
    assert again["counts"]["found"] >= left["counts"]["found"]


# ------------------------------------------------------------------ 7. a random map; read only
@functools.lru_cache(maxsize=None)
def _random_map():
    g = np.random.default_rng(41)
    cloud = _pts(g.uniform(-6.0, 6.0, (320, 3)))
    q = _pts(g.uniform(-7.0, 7.0, (257, 3)))
    ref = Ref(1.0, 2048, *GATE)
    ref.integrate(cloud[:200], I34, 0)
    ref.integrate(cloud, I34, 1)
    asks = (dict(reach=2), dict(reach=2, max_dist=1.1), dict(reach=2, min_hits=2), dict(reach=1, max_dist=0.4))
    return cloud, q, ref, asks, [ref.nearest_voxels(q, I34, **kw) for kw in asks]


@BOTH
def test_random_map_repeats_and_changes_nothing(fmx_mod, on_device):
    cloud, q, ref, asks, wants = _random_map()
    assert 250 <= ref.voxels <= 320
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ctx.carve_configure(margin=1)
    ctx.carve_configure(False)
    ctx.dense_integrate(np.array(cloud[:200]), I34, 0)
    ctx.dense_integrate(np.array(cloud), I34, 1)
    before = _snapshot(ctx, 1.0)
    p = _arg(q, on_device)
    for kw, want in zip(asks, wants):
        got, again = ctx.nearest_voxels(p, I34, **kw), ctx.nearest_voxels(p, I34, **kw)
        assert NR.same(got, want) is None, (kw, NR.same(got, want))
        assert NR.same(got, again) is None
        assert want["lookups_bounds"][0] <= got["counts"]["lookups"] <= want["lookups_bounds"][1]
    assert _same_snapshot(before, _snapshot(ctx, 1.0))
    assert wants[0]["counts"]["found"] > wants[1]["counts"]["found"] > wants[3]["counts"]["found"] > 0
    assert wants[0]["counts"]["found"] > wants[2]["counts"]["found"] > 0


def test_null_outputs_are_skipped_and_one_launch(fmx_mod):
    cloud, q, ref, asks, wants = _random_map()
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ctx.profile(True)
    ctx.dense_integrate(np.array(cloud[:200]), I34, 0)
    ctx.dense_integrate(np.array(cloud), I34, 1)
    base = ctx.profile_read()["dense"]["launches"]
    for k, fields in enumerate((FIELDS, ("state",), ("dist2",), ("scan",), ("index", "points"), ("hits", "misses"), ())):
        got = _raw(ctx, q, I34, fields, reach=2)
        assert NR.same(dict(got, lookups_bounds=None), wants[0], fields) is None, fields
        assert all((got[f] == 7).all() for f in FIELDS if f not in fields), fields
        prof = ctx.profile_read()
        assert prof["dense"]["launches"] == base + k + 1 and list(prof)[-1] == "dense"
    _raw(ctx, q[:0], I34, (), reach=2)  # no points: nothing launched
    assert ctx.profile_read()["dense"]["launches"] == base + 7


# ------------------------------------------------------------------ 8. status codes
def test_status_codes(fmx_mod):
    fmx = fmx_mod
    cloud, q, _, _, _ = _random_map()
    ctx = _ctx(fmx)
    assert _status(fmx, lambda: ctx.nearest_voxels(q, I34)) == STATE  # before fmx_dense_configure
    ctx.dense_configure(True, 1.0, 2048)
    ctx.dense_integrate(np.array(cloud), I34, 0)
    assert _status(fmx, lambda: ctx.nearest_voxels(q, I34, reach=9)) == INVAL
    assert ctx.nearest_voxels(q, I34, reach=8)["counts"]["found"] > 0
    for bad in (math.nan, -1.0, -math.inf):
        st, out = _raw(ctx, q, I34, FIELDS, max_dist2=bad, status=True, fill=9)
        assert st == INVAL and all((v == 9).all() for v in out.values()), bad
    st, out = _raw(ctx, q, I34, FIELDS, reach=9, status=True, fill=9)
    assert st == INVAL and all((v == 9).all() for v in out.values())
    assert _raw(ctx, q, I34, FIELDS, null_pose=True, status=True)[0] == INVAL
    assert _raw(ctx, q, I34, FIELDS, null_points=True, status=True)[0] == INVAL
    assert _raw(ctx, q[:0], I34, FIELDS, null_points=True, status=True)[0] == 0
    for k, bad in ((3, np.inf), (0, np.nan)):
        T = I34.copy()
        T.reshape(12)[k] = bad
        assert _status(fmx, lambda: ctx.nearest_voxels(q, T)) == INVAL
    off = _ctx(fmx)
    off.dense_configure(True, 1.0, 2048)
    off.dense_configure(False, 1.0, 2048)
    assert _status(fmx, lambda: off.nearest_voxels(q, I34)) == STATE  # the map is off


# ------------------------------------------------------------------ 9. the FORM wrappers
def test_form_dense_nearest_and_fitness(fmx_mod):
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    world = synth.World()
    scans = [synth.make_scan_skewed("tiny", k, world=world)[0].numpy() for k in range(3)]
    f = fmx_mod.FORM()
    f.set_lidar_params(lidar)
    with pytest.raises(RuntimeError):
        f.dense_nearest(scans[0], 0.5)  # the dense map is off
    w = 0.5
    f.set_dense_map(True, voxel_width=w, max_voxels=1 << 15)
    f.initialize()
    ref = Ref(w, 1 << 15)
    for k in range(3):
        f.add_lidar(scans[k][:, :3])
        ref.integrate(scans[k], f.pose()[:3], k)
    q, T = scans[2][::5], f.pose()[:3]
    diag = math.sqrt(3.0) * w
    got = f.dense_nearest(q[:, :3], diag)
    want = ref.nearest_voxels(q, T, math.floor(diag / w) + 1, diag)
    assert NR.same(got, want) is None, NR.same(got, want)
    fit = f.dense_fitness(q, diag)
    took = R.classify(q, T, w, ref.min2, ref.max2)[0] == 0  # the points the last integration took
    assert took.sum() > 100 and (got["state"][took] == PR.SOLID).all() and got["dist2"][took].max() <= diag * diag
    assert f.dense_fitness(q[took], diag)["fitness"] == 1.0
    assert fit == NR.fitness(want) and fit["n_found"] == want["counts"]["found"] and 0.0 < fit["rmse"] < diag
    other = _pose(_rot("z", 0.02), T[:, 3] + (0.3, -0.2, 0.1))
    assert NR.same(f.dense_nearest(q, 0.4, pose=other, min_hits=2), ref.nearest_voxels(q, other, 1, 0.4, 2)) is None
    assert f.dense_fitness(q, 0.4, pose=other)["fitness"] < 1.0
    with pytest.raises(ValueError):
        f.dense_nearest(q, 8 * w)  # reach 9
    assert f.dense_nearest(q, 8 * w - 1e-9)["counts"]["found"] > 0

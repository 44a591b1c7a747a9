"""Point-to-plane alignment against the dense map's normals on the device (fmx_plane_system,
fmx_plane_align; DESIGN.md §Dense map, Plane alignment) against the restatement
(tests/plane_ref.py over tests/nearest_ref.py's search, fed with the device's downloaded
normals) and against fmx_corr_set + fmx_linearize.  The class counts are compared with equality,
the 28 + 1 sums within tests/test_gpu_align.py's tolerance (1e-10 relative to the system's largest
entry; the error 1e-10 relative), poses within 1e-6."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

import align_ref as AR
import carve_ref as CR
import nearest_ref as NR
import normals_ref as MR
import plane_ref as PL
import probe_ref as PR
from form_amd import synth

pytestmark = pytest.mark.gpu

INVAL, STATE = 1, 5
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
INF = math.inf
BOTH = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
FIX = dict(reach=1, min_support=5, max_flatness=0.05)
GRID_CAP_LANES = 2048 * 256  # the grid's cap in lanes: a grid stride beyond (one lane per point)

_FMX = {}


@pytest.fixture(autouse=True)
def _module(fmx_mod):
    _FMX["mod"] = fmx_mod


def _pts(rows):
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return p


def _ctx(fmx):
    p = synth.default_params(synth.ScanGeometry(16, 256, 15.0, 0.01, 0.02))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _arg(p, on_device):
    return torch.from_numpy(np.array(p)).to("cuda:0") if on_device else np.array(p)


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


TILT = np.zeros((3, 4))
TILT[:, :3] = _rot("z", 0.02) @ _rot("x", -0.015)
TILT[:, 3] = (0.05, -0.04, 0.03)


@functools.lru_cache(maxsize=None)
def _world():
    """The fixture's map restated (computed once, left unchanged) and 257 queries in the frame of
    TILT: fixture points moved by up to 0.4, some far from the map, three invalid."""
    ref = NR.NearestRef(1.0, 2048, *GATE)
    fix = MR.fixture()
    ref.integrate(fix, I34, 0)
    g = np.random.default_rng(59)
    w = fix[g.choice(448, 257, replace=False), :3].astype(np.float64) + g.uniform(-0.4, 0.4, (257, 3))
    w[::16] += 30.0  # nothing within reach
    q = _pts((w - TILT[:, 3]) @ TILT[:, :3])
    q[:, 3] = g.normal(0, 1, 257)  # w is never read
    q[3, 0], q[64, 2] = np.nan, np.inf
    q[100, :3] = 0.0
    fix.setflags(write=False)
    q.setflags(write=False)
    return ref, fix, q


def _map(fmx, build=FIX):
    """A context holding the fixture with a current snapshot, and {(scan, index): normal} of it."""
    ref, fix, _ = _world()
    ctx = _ctx(fmx)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ctx.dense_integrate(np.array(fix), I34, 0)
    if build is None:
        return ctx, None
    ctx.normals_build(**build)
    d = ctx.normals_download(oriented_only=False)
    return ctx, PL.by_owner(d["scan"], d["index"], d["normals"])


def _raw_system(ctx, p, T, on_device=False, reach=1, max_dist2=INF, sigma=1.0, min_hits=1, stride=1, status=False, null=(),
                n=None, fill=0.0):
    """fmx_plane_system itself (the wrapper squares a distance: max_dist2 goes in as given)."""
    fmx = _FMX["mod"]
    prm = fmx._AlignParams(min_hits, 0, 0, reach, max_dist2, sigma, stride)
    on_dev, ptr, m, keep = fmx._scan_ptr(_arg(p, on_device))
    if on_dev:
        fmx._ready(keep)
    pose = np.ascontiguousarray(T, np.float64).reshape(12)
    out, cnt = np.full(29, fill), fmx._PlaneCounts()
    st = fmx.lib().fmx_plane_system(ctx.h, None if "points" in null or not m else ptr, C.c_size_t(m if n is None else n),
                                    C.c_int(on_dev), None if "pose" in null else fmx._p(pose),
                                    None if "params" in null else C.byref(prm), None if "out" in null else fmx._p(out),
                                    None if "counts" in null else C.byref(cnt))
    del keep
    if status:
        return st, out
    assert st == 0, st
    return out, cnt.as_dict()


def _raw_align(ctx, p, T, on_device=False, reach=1, max_dist2=INF, sigma=1.0, stride=1, max_iters=30, threshold=1e-6,
               null=(), fill=7.0):
    """fmx_plane_align itself with a prefilled pose_out: (status, pose_out, result)."""
    fmx = _FMX["mod"]
    prm = fmx._AlignParams(1, 0, 0, reach, max_dist2, sigma, stride)
    on_dev, ptr, m, keep = fmx._scan_ptr(_arg(p, on_device))
    if on_dev:
        fmx._ready(keep)
    pose = np.ascontiguousarray(T, np.float64).reshape(12)
    out, res = np.full(12, fill), fmx._PlaneResult()
    st = fmx.lib().fmx_plane_align(ctx.h, None if "points" in null or not m else ptr, C.c_size_t(m), C.c_int(on_dev),
                                   None if "pose" in null else fmx._p(pose), None if "params" in null else C.byref(prm),
                                   C.c_uint32(max_iters), C.c_double(threshold), None if "pose_out" in null else fmx._p(out),
                                   None if "result" in null else C.byref(res))
    del keep
    return st, out, res


def _close(got, want):
    """tests/test_gpu_align.py's measure: the 28 entries relative to the largest, the error relative."""
    scale = np.abs(want[:28]).max() + 1e-300
    return bool(np.all(np.abs(got[:28] - want[:28]) <= 1e-10 * scale) and np.allclose(got[28], want[28], rtol=1e-10, atol=0))


def _sys(ctx, normal_at, p, T, on_device=False, **kw):
    """The device's system and counts, held against the restatement's (its own search, the
    device's normals) and, found + unoriented, against the device's own nearest_voxels."""
    ref = _world()[0]
    sigma, stride = kw.get("sigma", 1.0), kw.get("stride", 1)
    search = {k: v for k, v in kw.items() if k in ("reach", "min_hits")}
    got, cnt = _raw_system(ctx, p, T, on_device, **kw)
    want, wcnt, (lo, hi) = PL.system_from(ref.nearest_voxels, normal_at, p, T, sigma, stride, max_dist2=kw.get("max_dist2", INF),
                                          **search)
    look = cnt.pop("lookups")
    assert cnt == wcnt and sum(cnt.values()) == len(p), (cnt, wcnt, kw)
    assert lo <= look <= hi, (lo, look, hi, kw)
    assert _close(got, want), (kw, np.abs(got - want).max(), got, want)
    flipped = PL.system_from(ref.nearest_voxels, {k: -v for k, v in normal_at.items()}, p, T, sigma, stride,
                             max_dist2=kw.get("max_dist2", INF), **search)[0]
    assert _close(got, flipped)  # the sign of the normals plays no part
    if not cnt["found"]:
        assert not got.any()
    return got, cnt


# ------------------------------------------------------------------ 1. shapes
@BOTH
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges_reaches_limits_and_strides(fmx_mod, n, on_device):
    _, _, q = _world()
    ctx, normal_at = _map(fmx_mod)
    found = unoriented = 0
    for reach in (1, 2):
        for stride in (1, 3, n + 5):
            _, cnt = _sys(ctx, normal_at, q[:n], TILT, on_device, reach=reach, stride=stride, sigma=0.1)
            assert cnt["skipped"] == n - len(range(0, n, stride))
            found += cnt["found"]
            unoriented += cnt["unoriented"]
    assert found > (n // 4 if n >= 63 else -1) and unoriented > (n // 16 if n >= 63 else -1)
    for md2 in (0.0, 2.25, INF):
        _sys(ctx, normal_at, q[:n], TILT, on_device, reach=2, max_dist2=md2, sigma=0.5)
    _, zero = _sys(ctx, normal_at, q[:n], TILT, on_device, reach=2, stride=0)  # stride 0 reads 1
    assert zero["skipped"] == 0


@BOTH
def test_unoriented_winners_add_nothing(fmx_mod, on_device):
    """The points whose winner has no normal are counted apart, and the system is the one of the
    other points alone."""
    _, _, q = _world()
    ctx, normal_at = _map(fmx_mod)
    S, cnt = _sys(ctx, normal_at, q, TILT, on_device, reach=1, sigma=0.1)
    assert cnt["unoriented"] > 20 and cnt["found"] > 100
    near = ctx.nearest_voxels(_arg(q, on_device), TILT, reach=1)
    looked = _raw_system(ctx, q, TILT, on_device, reach=1, sigma=0.1)[1]["lookups"]  # (_sys took it out of cnt)
    assert near["counts"]["found"] == cnt["found"] + cnt["unoriented"] and near["counts"]["lookups"] == looked
    has = PL.normals_of(near, normal_at).any(axis=1)
    only, ocnt = _raw_system(ctx, q[has], TILT, on_device, reach=1, sigma=0.1)
    assert ocnt["unoriented"] == 0 and ocnt["found"] == cnt["found"] and _close(only, S)
    rest, rcnt = _raw_system(ctx, q[~has], TILT, on_device, reach=1, sigma=0.1)
    assert not rest.any() and rcnt["found"] == 0 and rcnt["unoriented"] == cnt["unoriented"]


# ------------------------------------------------------------------ 2. nothing found
@BOTH
def test_clouds_without_a_found_point_give_the_zero_system(fmx_mod, on_device):
    ctx, normal_at = _map(fmx_mod)
    n = 70
    invalid = _pts([(np.nan, 1, 1), (1, np.inf, 1), (0, 0, 0)] * 24)[:n]
    far = _pts([(3e6 + k, 0.5, -3e6) for k in range(n)])
    lonely = _pts([(60.5 + k, 50.5, 40.5) for k in range(n)])
    sparse = _pts([(20.5 + 3 * (k % 6), 20.5, 20.5) for k in range(n)])  # the isolated voxels: found, never oriented
    for cloud, cls in ((invalid, "invalid"), (far, "out_of_range"), (lonely, "none"), (sparse, "unoriented")):
        for stride in (1, 3):
            S, cnt = _sys(ctx, normal_at, cloud, I34, on_device, reach=2, stride=stride)
            kept = len(range(0, n, stride))
            assert not S.any() and cnt == dict(dict.fromkeys(PL.CLASSES, 0), **{cls: kept}, skipped=n - kept), (cls, cnt)
    S, cnt = _raw_system(ctx, lonely[:0], I34, on_device, fill=3.0)  # no points: zeros, nothing launched
    assert not S.any() and not any(cnt.values())


# ------------------------------------------------------------------ 3. against fmx_linearize
@BOTH
def test_system_equals_the_plane_factor_of_fmx_linearize(fmx_mod, on_device):
    _, _, q = _world()
    ctx, normal_at = _map(fmx_mod)
    lin = _ctx(fmx_mod)
    for kw in (dict(reach=2, sigma=0.1), dict(reach=1, sigma=0.7, stride=2)):
        sub = np.ascontiguousarray(q[::kw.get("stride", 1)])
        S, cnt = _sys(ctx, normal_at, q, TILT, on_device, **kw)
        near = ctx.nearest_voxels(_arg(sub, on_device), TILT, reach=kw["reach"])
        nrm = PL.normals_of(near, normal_at)
        use = (near["state"] == PR.SOLID) & nrm.any(axis=1)
        assert use.sum() == cnt["found"] > 40
        none = np.zeros((0, 3))
        lin.corr_set([int(use.sum())], near["points"][use], nrm[use], sub[use, :3].astype(np.float64), [0], none, none)
        G, err = lin.linearize(I34, TILT, kw["sigma"], True)
        assert G.shape == (1, 28) and _close(S, np.concatenate([G[0], err])), (kw, np.abs(S[:28] - G[0]).max())


# ------------------------------------------------------------------ 4. bit for bit
def test_same_bits_twice_and_from_either_pointer(fmx_mod):
    _, fix, q = _world()
    ctx, _ = _map(fmx_mod)
    g = np.random.default_rng(61)
    big = _pts(g.uniform(-1.0, 14.0, (5000, 3)))
    for p, kw in ((q, dict(reach=2, sigma=0.1)), (big, dict(reach=1, sigma=0.1, stride=3)), (big, dict(reach=2, max_dist2=1.0))):
        runs = [_raw_system(ctx, p, TILT, dev, **kw) for dev in (False, True, False, True)]
        for S, cnt in runs[1:]:
            assert S.tobytes() == runs[0][0].tobytes() and cnt == runs[0][1], kw
        assert runs[0][1]["found"] > 50


# ------------------------------------------------------------------ 5. past the grid's cap
def test_more_points_than_one_pass_of_the_grid(fmx_mod):
    """One pass of the capped grid holds at most 2048 * 256 points: 65 past that, most of them far
    from the map so that they end at shell 1, strided once.  The reference is built vectorised
    from the device's own nearest_voxels answers (tests/test_gpu_nearest.py holds those against
    the restatement) and the downloaded normals."""
    ctx, normal_at = _map(fmx_mod)
    g = np.random.default_rng(67)
    n = GRID_CAP_LANES + 65
    q = _pts(g.uniform(40.0, 80.0, (n, 3)))
    close = g.choice(n, 6000, replace=False)
    q[close, :3] = g.uniform(-1.0, 14.0, (6000, 3)).astype(np.float32)
    q[n - 1, :3] = (0.55, 6.4, 6.3)  # the last point counts: on the x patch
    q[[5, 300000], 0] = np.nan
    d = torch.from_numpy(q).to("cuda:0")
    for stride in (1, 7):
        S, cnt = ctx.plane_system(d, TILT, reach=1, sigma=0.1, stride=stride)
        sub = q[::stride]
        near = ctx.nearest_voxels(sub, TILT, reach=1)
        nrm = PL.normals_of(near, normal_at)
        want = PL.system(sub, TILT, near["state"], near["points"], nrm, 0.1)
        wcnt = PL.counts_of(near["state"], nrm, n, stride)
        assert {k: cnt[k] for k in wcnt} == wcnt and cnt["lookups"] == near["counts"]["lookups"]
        assert cnt["found"] > 200 // stride and cnt["none"] > n // stride - 7000
        assert _close(S, want), (stride, np.abs(S - want).max())
    assert ctx.plane_system(q, TILT, reach=1, sigma=0.1, stride=7)[0].tobytes() == S.tobytes()


# ------------------------------------------------------------------ 6. read only
def _snapshot(ctx, w):
    return (CR.sort_download(ctx.dense_download(misses=True), w), ctx.dense_stats(), ctx.dense_last(), ctx.carve_last())


@BOTH
def test_the_calls_change_nothing(fmx_mod, on_device):
    _, fix, q = _world()
    ctx, _ = _map(fmx_mod, build=None)
    ctx.carve_configure(margin=1)
    ctx.dense_integrate(np.array(fix[:200]), TILT, 1)
    before = _snapshot(ctx, 1.0)
    ctx.normals_build(**FIX)
    ctx.normals_download(False)
    _raw_system(ctx, q, TILT, on_device, reach=2, sigma=0.1)
    _raw_system(ctx, q, TILT, on_device, reach=1, stride=3, min_hits=2)
    got = ctx.dense_align(_arg(q, on_device), TILT, reach=2, sigma=0.1, max_iters=3, plane=True)
    assert got["iters"] >= 1 and ctx.normals_stats()["current"]
    after = _snapshot(ctx, 1.0)
    assert CR.same(before[0], after[0]) is None and before[1:] == after[1:]


# ------------------------------------------------------------------ 7. the loop
@functools.lru_cache(maxsize=None)
def _zero_residual():
    p, T0 = PL.zero_residual_cloud()
    ref = NR.NearestRef(1.0, 2048, *GATE)
    assert ref.integrate(p, I34, 0)["merged"] == 0
    built = MR.build(ref, **PL.ZERO_BUILD)
    normal_at = PL.by_owner_of(ref, built)
    want = AR.align(lambda T: PL.system_from(ref.nearest_voxels, normal_at, p, T, sigma=0.1, reach=1)[:2], T0, 30,
                    PL.ZERO_THRESHOLD)
    p.setflags(write=False)
    return p, T0, ref, normal_at, built, want


def _zero_map(fmx):
    p, _, _, _, built, _ = _zero_residual()
    ctx = _ctx(fmx)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    assert ctx.dense_integrate(np.array(p), I34, 0)["merged"] == 0
    cnt = ctx.normals_build(**PL.ZERO_BUILD)
    assert {k: cnt[k] for k in MR.CLASSES} == MR.counts_of(built)
    return ctx


@BOTH
def test_plane_align_recovers_the_pose_of_the_zero_residual_problem(fmx_mod, on_device):
    p, T0, ref, normal_at, built, want = _zero_residual()
    ctx = _zero_map(fmx_mod)
    d = ctx.normals_download(True)
    assert sorted(set(map(tuple, np.abs(d["normals"]).tolist()))) == [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)]
    assert not d["flatness"].any()  # an exact axis plane: the Jacobi returns the axis exactly
    kw = dict(reach=1, sigma=0.1, plane=True)
    got = ctx.dense_align(_arg(p, on_device), T0, max_iters=30, threshold=PL.ZERO_THRESHOLD, **kw)
    assert got["iters"] == want["iters"] and got["converged"] and want["converged"]
    assert np.abs(got["pose"] - want["pose"]).max() < 1e-6 and np.abs(got["pose"] - I34).max() < 1e-6
    assert got["last_step"] < PL.ZERO_THRESHOLD and got["counts"] == dict(want["counts"], lookups=got["counts"]["lookups"])
    assert got["counts"]["found"] == MR.counts_of(built)["oriented"] and got["error"] < 1e-6
    # max_iters = 0: the initial pose; 1: one restated step; neither converged
    zero = ctx.dense_align(_arg(p, on_device), T0, max_iters=0, **kw)
    assert np.array_equal(zero["pose"], T0) and zero["iters"] == 0 and not zero["converged"] and zero["last_step"] == 0.0
    assert zero["error"] == 0.0 and not any(zero["counts"].values())
    one = ctx.dense_align(_arg(p, on_device), T0, max_iters=1, threshold=PL.ZERO_THRESHOLD, **kw)
    S0 = PL.system_from(ref.nearest_voxels, normal_at, p, T0, sigma=0.1, reach=1)[0]
    step = AR.gn_step(S0, T0)
    assert one["iters"] == 1 and not one["converged"] and np.abs(one["pose"] - step[0]).max() < 1e-6
    assert abs(one["last_step"] - step[1]) < 1e-6 and np.allclose(one["error"], S0[28], rtol=1e-10, atol=0)
    # converged and last_step agree with the threshold on either side of it
    loose = ctx.dense_align(_arg(p, on_device), T0, max_iters=30, threshold=1.0, **kw)
    assert loose["iters"] == 1 and loose["converged"] and loose["last_step"] == one["last_step"] < 1.0
    never = ctx.dense_align(_arg(p, on_device), T0, max_iters=4, threshold=0.0, **kw)
    assert never["iters"] == 4 and not never["converged"] and never["last_step"] >= 0.0
    # the stride: every other point still fixes the pose
    half = ctx.dense_align(_arg(p, on_device), T0, stride=2, threshold=PL.ZERO_THRESHOLD, **kw)
    assert half["converged"] and half["counts"]["skipped"] == 73 and np.abs(half["pose"] - I34).max() < 1e-6


def test_a_singular_system_leaves_pose_out_alone(fmx_mod):
    p, T0, _, _, _, _ = _zero_residual()
    ctx = _zero_map(fmx_mod)
    one_patch = p[:49]  # the plane x = 0.5 only: at the identity m = n = e_x, H[0][0] = 0 exactly
    lonely = _pts([(40.5 + k, 30.5, 20.5) for k in range(70)])
    for on_device in (False, True):
        st, out, res = _raw_align(ctx, one_patch, I34, on_device)
        assert st == STATE and (out == 7.0).all() and res.iters == 0
        st, out, res = _raw_align(ctx, lonely, T0, on_device)  # nothing found: the zero system
        assert st == STATE and (out == 7.0).all()
        st, out, res = _raw_align(ctx, lonely[:0], T0, on_device)  # no points
        assert st == STATE and (out == 7.0).all()
    S, cnt = _raw_system(ctx, one_patch, I34)
    assert cnt["found"] > 20 and S[0] == 0.0 and S[AR.pack_index(3, 3)] > 0.0
    st, out, res = _raw_align(ctx, lonely, T0, max_iters=0)
    assert st == 0 and np.array_equal(out.reshape(3, 4), T0) and res.iters == 0
    st, out, _ = _raw_align(ctx, p, T0, null=("result",), sigma=0.1, threshold=PL.ZERO_THRESHOLD)  # a NULL result is allowed
    assert st == 0 and np.abs(out.reshape(3, 4) - I34).max() < 1e-6


# ------------------------------------------------------------------ 8. status codes, staleness
def test_status_codes(fmx_mod):
    fmx = fmx_mod
    _, fix, q = _world()
    ctx = _ctx(fmx)
    assert _raw_system(ctx, q, I34, status=True)[0] == STATE  # before fmx_dense_configure
    assert _raw_align(ctx, q, I34)[0] == STATE
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ctx.dense_integrate(np.array(fix), I34, 0)
    st, out = _raw_system(ctx, q, I34, status=True, fill=9.0)  # never built
    assert st == STATE and (out == 9.0).all()
    st, out, _ = _raw_align(ctx, q, I34)
    assert st == STATE and (out == 7.0).all()
    ctx.normals_build(**FIX)
    assert _raw_system(ctx, q, I34, status=True, reach=8)[0] == 0
    bad_params = [dict(reach=9)] + [dict(max_dist2=v) for v in (math.nan, -1.0, -INF)] + \
                 [dict(sigma=v) for v in (math.nan, 0.0, -0.5, INF, -INF)]
    for bad in bad_params:
        st, out = _raw_system(ctx, q, I34, status=True, fill=9.0, **bad)
        assert st == INVAL and (out == 9.0).all(), bad
        st, out, _ = _raw_align(ctx, q, I34, **bad)
        assert st == INVAL and (out == 7.0).all(), bad
    for null in ("params", "out", "pose", "points"):
        st, out = _raw_system(ctx, q, I34, status=True, fill=9.0, null=(null,))
        assert st == INVAL and (out == 9.0).all(), null
    assert _raw_system(ctx, q, I34, null=("counts",))[0].any()  # NULL counts are allowed
    assert _raw_system(ctx, q[:0], I34, status=True, null=("points",))[0] == 0
    for null in ("params", "pose_out", "pose", "points"):
        st, out, _ = _raw_align(ctx, q, I34, null=(null,))
        assert st == INVAL and (out == 7.0).all(), null
    for bad in (math.nan, -1e-300, -INF):
        st, out, _ = _raw_align(ctx, q, I34, threshold=bad)
        assert st == INVAL and (out == 7.0).all(), bad
    for k, bad in ((3, np.inf), (0, np.nan)):
        T = I34.copy()
        T.reshape(12)[k] = bad
        assert _raw_system(ctx, q, T, status=True)[0] == INVAL and _raw_align(ctx, q, T)[0] == INVAL
    assert _raw_system(ctx, q, I34, status=True, n=1 << 32)[0] == INVAL
    with pytest.raises(fmx.FmxError) as e:
        ctx.dense_align(q, I34, reach=9, plane=True)
    assert e.value.status == INVAL

    # stale after each call that changes the table, current again after a rebuild
    def stale():
        st, out = _raw_system(ctx, q, I34, status=True, fill=9.0)
        assert st == STATE and (out == 9.0).all()
        st, out, _ = _raw_align(ctx, q, I34)
        assert st == STATE and (out == 7.0).all()
        ctx.normals_build(**FIX)
        assert _raw_system(ctx, q, I34, status=True)[0] == 0 and _raw_align(ctx, q, I34, max_iters=0)[0] == 0

    ctx.carve_configure(margin=0)
    assert _raw_system(ctx, q, I34, status=True)[0] == 0  # enabling the carve changes no voxel
    ctx.dense_integrate(_pts([(40.5, 40.5, 40.5)]), I34, 1)
    stale()
    held = ctx.roll_evict((6.0, 6.0, 6.0), (8, 8, 8))
    assert len(held["hits"]) == 17
    stale()
    ctx.dense_upload(held["points"], held["scan"], held["index"], held["hits"])
    stale()
    assert ctx.carve_rays(_pts([(0.0, 6.0, 0.0)]), CR.special_pose((0.5, -1.5, 1.5)))["misses"] >= 1
    stale()
    ctx.dense_clear()
    stale()
    off = _ctx(fmx)
    off.dense_configure(True, 1.0, 2048)
    off.normals_build(**FIX)
    off.dense_configure(False, 1.0, 2048)
    assert _raw_system(off, q, I34, status=True)[0] == STATE and _raw_align(off, q, I34)[0] == STATE  # the map is off


def test_one_launch_per_system_under_the_dense_profile_id(fmx_mod):
    _, fix, q = _world()
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ctx.profile(True)
    ctx.dense_integrate(np.array(fix), I34, 0)
    ctx.normals_build(**FIX)
    base = ctx.profile_read()["dense"]["launches"]
    ctx.plane_system(q, TILT, reach=2)
    assert ctx.profile_read()["dense"]["launches"] == base + 1
    got = ctx.dense_align(q, TILT, reach=2, sigma=0.1, max_iters=3, threshold=0.0, plane=True)
    assert got["iters"] == 3 and ctx.profile_read()["dense"]["launches"] == base + 4
    _raw_system(ctx, q[:0], I34)  # no points: nothing launched
    assert ctx.profile_read()["dense"]["launches"] == base + 4


# ------------------------------------------------------------------ 9. FORM.dense_localize(plane=True)
def test_form_dense_localize_plane_after_save_and_load(fmx_mod, tmp_path):
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    world = synth.World()
    scans = [synth.make_scan_skewed("tiny", k, world=world)[0].numpy() for k in range(3)]
    w = 0.5

    def form():
        f = fmx_mod.FORM()
        f.set_lidar_params(lidar)
        f.set_dense_map(True, voxel_width=w, max_voxels=1 << 15)
        f.initialize()
        return f

    f = form()
    poses = []
    for k in range(3):
        f.add_lidar(scans[k][:, :3])
        poses.append(np.array(f.pose()[:3]))
    path = tmp_path / "map.npz"
    f.dense_save(path)
    g = form()
    assert g.dense_load(path)["added"] == len(f.dense_map()["hits"]) > 500
    scan, truth = scans[1], poses[1]
    guess = AR.compose(truth, AR.expmap((0.01, -0.008, 0.012, 0.05, -0.04, 0.03)))
    radius, sigma = 0.6, 0.1
    kw = dict(pose_guess=guess, sigma=sigma, max_iters=30, threshold=1e-6)
    point = g.dense_localize(scan, radius, **kw)  # plane=False: today's path, no snapshot
    assert not g._est.normals_stats()["built"] and "n_unoriented" not in point
    reach = math.floor(radius / w) + 1
    direct = g._est.dense_align(scan, guess, reach, radius, sigma, max_iters=30, threshold=1e-6)
    assert np.array_equal(point["pose"], direct["pose"]) and point["iters"] == direct["iters"]
    got = g.dense_localize(scan, radius, plane=True, **kw)  # builds the snapshot itself
    st = g._est.normals_stats()
    assert st["current"] and st["oriented"] > 100
    direct = g._est.dense_align(scan, guess, reach, radius, sigma, max_iters=30, threshold=1e-6, plane=True)
    assert np.array_equal(got["pose"], direct["pose"]) and got["iters"] == direct["iters"] >= 2
    assert got["converged"] == direct["converged"]
    # nearer to where the scan was integrated than the guess was
    assert np.abs(got["pose"] - truth).max() < np.abs(guess - truth).max()
    # n_found and the point-to-plane RMSE are those of one more plane_system at the returned pose
    S, cnt = g._est.plane_system(scan, got["pose"], reach, radius, sigma)
    assert got["n_found"] == cnt["found"] > 200 and got["n_unoriented"] == cnt["unoriented"]
    assert got["n_valid"] == cnt["found"] + cnt["unoriented"] + cnt["none"] == point["n_valid"]
    assert got["fitness"] == cnt["found"] / got["n_valid"]
    assert got["rmse"] == math.sqrt(2.0 * float(S[28]) * sigma * sigma / cnt["found"]) > 0.0
    assert got["rmse"] < point["rmse"]  # the distance to the plane, not to the representative
    # the estimator is not fed: a fresh FORM has no pose to report beyond its initial one
    assert np.array_equal(np.array(g.pose()), np.array(form().pose()))

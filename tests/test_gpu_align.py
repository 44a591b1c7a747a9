"""Aligning a scan to the dense map on the device (fmx_align_system, fmx_align_dense; DESIGN.md
§Dense map, Aligning) against the restatement (tests/align_ref.py over tests/nearest_ref.py).
The class counts are compared with equality, the 28 + 1 sums within the project's tolerance for
normal equations (1e-10 relative to the system's largest entry, tests/test_gpu_parity.py's
measure for G; the error 1e-10 relative), poses within 1e-6."""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

import align_ref as AR
import carve_ref as CR
import dense_ref as R
import nearest_ref as NR
import probe_ref as PR
from form_amd import synth

pytestmark = pytest.mark.gpu

INVAL, STATE = 1, 5
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
INF = math.inf
BOTH = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
CLASSES = ("found", "none", "out_of_range", "invalid")
GRID_CAP_LANES = 2048 * 256  # the grid's cap in lanes: a grid stride beyond, whatever the lanes per point


def _pts(rows):
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return p


def _ctx(fmx):
    p = synth.default_params(synth.ScanGeometry(16, 256, 15.0, 0.01, 0.02))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _pair(fmx, w=1.0, cap=2048, carve=None):
    ctx = _ctx(fmx)
    ctx.dense_configure(True, w, cap, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ref = NR.NearestRef(w, cap, *GATE)
    if carve is not None:
        ctx.carve_configure(**carve)
        ref.carve_configure(**carve)
    return ctx, ref


def _integrate(ctx, ref, p, T=I34, idx=0):
    got = ctx.dense_integrate(np.array(p), T, idx)
    assert got == ref.integrate(p, T, idx)
    return got


def _arg(p, on_device):
    return torch.from_numpy(np.array(p)).to("cuda:0") if on_device else np.array(p)


_FMX = {}


@pytest.fixture(autouse=True)
def _module(fmx_mod):
    _FMX["mod"] = fmx_mod


def _raw_system(ctx, p, T, on_device=False, reach=1, max_dist2=INF, sigma=1.0, min_hits=1, max_miss_ratio=None, stride=1,
                status=False, null=(), n=None, fill=0.0):
    """fmx_align_system itself (the wrapper squares a distance: max_dist2 goes in as given)."""
    fmx = _FMX["mod"]
    num, den = fmx.miss_fraction(max_miss_ratio)
    prm = fmx._AlignParams(min_hits, num, den, reach, max_dist2, sigma, stride)
    on_dev, ptr, m, keep = fmx._scan_ptr(_arg(p, on_device))
    if on_dev:
        fmx._ready(keep)
    pose = np.ascontiguousarray(T, np.float64).reshape(12)
    out, cnt = np.full(29, fill), fmx._AlignCounts()
    st = fmx.lib().fmx_align_system(ctx.h, None if "points" in null or not m else ptr, C.c_size_t(m if n is None else n),
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
    """fmx_align_dense itself with a prefilled pose_out: (status, pose_out, result)."""
    fmx = _FMX["mod"]
    prm = fmx._AlignParams(1, 0, 0, reach, max_dist2, sigma, stride)
    on_dev, ptr, m, keep = fmx._scan_ptr(_arg(p, on_device))
    if on_dev:
        fmx._ready(keep)
    pose = np.ascontiguousarray(T, np.float64).reshape(12)
    out, res = np.full(12, fill), fmx._AlignResult()
    st = fmx.lib().fmx_align_dense(ctx.h, None if "points" in null or not m else ptr, C.c_size_t(m), C.c_int(on_dev),
                                   None if "pose" in null else fmx._p(pose), None if "params" in null else C.byref(prm),
                                   C.c_uint32(max_iters), C.c_double(threshold), None if "pose_out" in null else fmx._p(out),
                                   None if "result" in null else C.byref(res))
    del keep
    return st, out, res


def _close(got, want):
    """tests/test_gpu_parity.py's measure for G on the 28 entries, its measure for the error."""
    scale = np.abs(want[:28]).max() + 1e-300
    return bool(np.all(np.abs(got[:28] - want[:28]) <= 1e-10 * scale) and np.allclose(got[28], want[28], rtol=1e-10, atol=0))


def _sys(ctx, ref, p, T, on_device=False, **kw):
    """The device's system and counts, held against the restatement's and against the device's
    own nearest_voxels on the kept points."""
    sigma, stride = kw.get("sigma", 1.0), kw.get("stride", 1)
    search = {k: v for k, v in kw.items() if k in ("reach", "min_hits", "max_miss_ratio")}
    got, cnt = _raw_system(ctx, p, T, on_device, **kw)
    want, wcnt, (lo, hi) = AR.system_from(ref.nearest_voxels, p, T, sigma, stride, max_dist2=kw.get("max_dist2", INF), **search)
    look = cnt.pop("lookups")
    assert cnt == wcnt and sum(cnt.values()) == len(p), (cnt, wcnt, kw)
    assert lo <= look <= hi, (lo, look, hi, kw)
    sub = np.ascontiguousarray(p)[AR.kept(len(p), stride)]
    md = math.sqrt(kw.get("max_dist2", INF))
    assert md * md == kw.get("max_dist2", INF)  # (the wrapper squares a distance: the tests' limits are exact squares)
    near = ctx.nearest_voxels(_arg(sub, on_device), T, max_dist=md, **search)
    assert {k: near["counts"][k] for k in CLASSES} == {k: cnt[k] for k in CLASSES} and near["counts"]["lookups"] == look, kw
    assert _close(got, want), (kw, np.abs(got - want).max(), got, want)
    if not cnt["found"]:
        assert not got.any()
    return got, cnt


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _pose(Rm, t):
    T = np.zeros((3, 4))
    T[:, :3] = Rm
    T[:, 3] = t
    return T


TILT = _pose(_rot("z", 0.2) @ _rot("x", -0.1), (0.3, -0.2, 0.1))


# ------------------------------------------------------------------ 1. shapes
@functools.lru_cache(maxsize=None)
def _few_dozen():
    """40 representatives in a 5^3 region and 257 queries around it (in the frame of TILT), some
    invalid, four of them on a representative."""
    g = np.random.default_rng(29)
    reps = _pts(g.uniform(-2.5, 2.5, (40, 3)))
    q = _pts(g.uniform(-4.0, 4.0, (257, 3)))
    q[:, 3] = g.normal(0, 1, 257)  # w is never read
    q[3, 0], q[64, 2] = np.nan, np.inf
    q[100, :3] = 0.0
    reps.setflags(write=False)
    q.setflags(write=False)
    return reps, q


@BOTH
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges_reaches_limits_and_strides(fmx_mod, n, on_device):
    reps, q = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    found = 0
    for reach in (0, 1, 2):
        for stride in (1, 3, n + 5):
            _, cnt = _sys(ctx, ref, q[:n], TILT, on_device, reach=reach, stride=stride, sigma=0.1)
            assert cnt["skipped"] == n - len(range(0, n, stride))
            found += cnt["found"]
    assert found > (n // 4 if n >= 63 else -1)
    for md2 in (0.0, 2.25, INF):
        _sys(ctx, ref, q[:n], TILT, on_device, reach=2, max_dist2=md2, sigma=0.5)
    _, zero = _sys(ctx, ref, q[:n], TILT, on_device, reach=2, stride=0)  # stride 0 reads 1
    assert zero["skipped"] == 0


@BOTH
def test_coincident_points_at_max_dist2_zero(fmx_mod, on_device):
    reps, q = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    both = np.concatenate([reps[:9], q[:60]])  # at the identity the first nine lie on their representatives
    S, cnt = _sys(ctx, ref, both, I34, on_device, reach=1, max_dist2=0.0, sigma=0.1)
    assert cnt["found"] == 9 and S[28] == 0.0 and S[0] > 0.0 and not S[[6, 12, 17, 21, 24, 26, 27]].any()


# ------------------------------------------------------------------ 2. the filter
@BOTH
def test_filter_by_hits_and_by_misses(fmx_mod, on_device):
    A, B = (1.5, 0.5, 0.5), (0.5, 2.5, 0.5)  # A nearer with one hit, B farther with two
    q = _pts([(0.5, 0.5, 0.5), (0.75, 0.25, 0.5), (1.25, 1.5, 0.25)])
    ctx, ref = _pair(fmx_mod)
    for k, r in enumerate((B, B, A)):
        _integrate(ctx, ref, _pts([r]), I34, k)
    ctx.carve_configure(margin=0)
    ref.carve_configure(margin=0)
    one, _ = _sys(ctx, ref, q, I34, on_device, reach=2)
    two, c2 = _sys(ctx, ref, q, I34, on_device, reach=2, min_hits=2)
    assert c2["found"] == 3 and not np.array_equal(one, two)
    assert _sys(ctx, ref, q, I34, on_device, reach=2, min_hits=3)[1]["none"] == 3
    T, through = CR.special_pose((0.5, 0.5, 0.5)), _pts([(2.0, 0, 0), (2.25, 0, 0)])
    assert ctx.carve_rays(_arg(through, on_device), T) == ref.carve_rays(through, T)
    assert ref.misses == {R.pack_key(1, 0, 0): 2}  # A: 2 misses on 1 hit
    for ratio, same_as in ((1.0, two), (1.99, two), (2.0, one), (None, one)):
        got, _ = _sys(ctx, ref, q, I34, on_device, reach=2, max_miss_ratio=ratio)
        assert np.array_equal(got, same_as), ratio


# ------------------------------------------------------------------ 3. nothing found
@BOTH
def test_clouds_without_a_found_point_give_the_zero_system(fmx_mod, on_device):
    reps, _ = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    n = 70
    invalid = _pts([(np.nan, 1, 1), (1, np.inf, 1), (0, 0, 0)] * 24)[:n]
    far = _pts([(3e6 + k, 0.5, -3e6) for k in range(n)])
    lonely = _pts([(40.5 + k, 30.5, 20.5) for k in range(n)])
    for cloud, cls in ((invalid, "invalid"), (far, "out_of_range"), (lonely, "none")):
        for stride in (1, 3):
            S, cnt = _sys(ctx, ref, cloud, TILT if cls != "out_of_range" else I34, on_device, reach=2, stride=stride)
            kept = len(range(0, n, stride))
            assert not S.any() and cnt == dict(dict.fromkeys(CLASSES, 0), **{cls: kept}, skipped=n - kept), (cls, cnt)
    S, cnt = _raw_system(ctx, lonely[:0], I34, on_device, fill=3.0)  # no points: zeros, nothing launched
    assert not S.any() and not any(cnt.values())


# ------------------------------------------------------------------ 4. against fmx_linearize
@BOTH
def test_system_equals_the_point_factor_of_fmx_linearize(fmx_mod, on_device):
    reps, q = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    lin = _ctx(fmx_mod)
    for kw in (dict(reach=2, sigma=0.1), dict(reach=1, sigma=0.7, stride=2)):
        sub = np.ascontiguousarray(q[::kw.get("stride", 1)])
        S, cnt = _sys(ctx, ref, q, TILT, on_device, **kw)
        near = ctx.nearest_voxels(_arg(sub, on_device), TILT, reach=kw["reach"])
        found = near["state"] == PR.SOLID
        assert found.sum() == cnt["found"] > 20
        none = np.zeros((0, 3))
        lin.corr_set([0], none, none, none, [int(found.sum())], near["points"][found], sub[found, :3].astype(np.float64))
        G, err = lin.linearize(I34, TILT, kw["sigma"], True)
        assert G.shape == (1, 28) and _close(S, np.concatenate([G[0], err])), (kw, np.abs(S[:28] - G[0]).max())


# ------------------------------------------------------------------ 5. bit for bit
def test_same_bits_twice_and_from_either_pointer(fmx_mod):
    reps, q = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    g = np.random.default_rng(31)
    big = _pts(g.uniform(-3.0, 3.0, (5000, 3)))
    for p, kw in ((q, dict(reach=2, sigma=0.1)), (big, dict(reach=1, sigma=0.1, stride=3)), (big, dict(reach=2, max_dist2=1.0))):
        runs = [_raw_system(ctx, p, TILT, dev, **kw) for dev in (False, True, False, True)]
        for S, cnt in runs[1:]:
            assert S.tobytes() == runs[0][0].tobytes() and cnt == runs[0][1], kw
        assert runs[0][1]["found"] > 50


# ------------------------------------------------------------------ 6. past the grid's cap
def test_more_points_than_one_pass_of_the_grid(fmx_mod):
    """One pass of the capped grid holds at most 2048 * 256 points (one lane per point): 65 past
    that, most of them far from the map so that they end at shell 1.  The reference is built
    vectorised from the device's own nearest_voxels answers, which tests/test_gpu_nearest.py
    holds against the restatement."""
    reps, _ = _few_dozen()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    g = np.random.default_rng(37)
    n = GRID_CAP_LANES + 65
    q = _pts(g.uniform(20.0, 60.0, (n, 3)))
    close = g.choice(n, 6000, replace=False)
    q[close, :3] = g.uniform(-3.0, 3.0, (6000, 3)).astype(np.float32)
    q[n - 1, :3] = (0.25, 0.5, -0.25)  # the last point counts
    q[[5, 300000], 0] = np.nan
    d = torch.from_numpy(q).to("cuda:0")
    for stride in (1, 7):
        S, cnt = ctx.align_system(d, TILT, reach=1, sigma=0.1, stride=stride)
        sub = q[::stride]
        near = ctx.nearest_voxels(sub, TILT, reach=1)
        want = AR.system(sub, TILT, near["state"], near["points"], 0.1)
        assert {k: cnt[k] for k in CLASSES} == {k: near["counts"][k] for k in CLASSES} and cnt["skipped"] == n - len(sub)
        assert cnt["found"] > 300 // stride and cnt["none"] > n // stride - 7000 and cnt["lookups"] == near["counts"]["lookups"]
        assert _close(S, want), (stride, np.abs(S - want).max())
        again, _ = ctx.align_system(q, TILT, reach=1, sigma=0.1, stride=stride)
        assert again.tobytes() == S.tobytes()


# ------------------------------------------------------------------ 7. read only
def _snapshot(ctx, w):
    return (CR.sort_download(ctx.dense_download(misses=True), w), ctx.dense_stats(), ctx.dense_last(), ctx.carve_last())


@BOTH
def test_the_calls_change_nothing(fmx_mod, on_device):
    reps, q = _few_dozen()
    ctx, ref = _pair(fmx_mod, carve=dict(margin=1))
    _integrate(ctx, ref, reps)
    _integrate(ctx, ref, reps[:20], TILT, 1)
    before = _snapshot(ctx, 1.0)
    _sys(ctx, ref, q, TILT, on_device, reach=2, sigma=0.1)
    _sys(ctx, ref, q, TILT, on_device, reach=1, stride=3, min_hits=2)
    got = ctx.dense_align(_arg(q, on_device), TILT, reach=2, sigma=0.1, max_iters=3)
    assert got["iters"] >= 1
    after = _snapshot(ctx, 1.0)
    assert CR.same(before[0], after[0]) is None and before[1:] == after[1:]


# ------------------------------------------------------------------ 8. the loop
@functools.lru_cache(maxsize=None)
def _zero_residual():
    p, T0 = AR.zero_residual_cloud()
    ref = NR.NearestRef(AR.ZERO_W, 2048, *GATE)
    assert ref.integrate(p, I34, 0)["merged"] == 0
    want = AR.align(lambda T: AR.system_from(ref.nearest_voxels, p, T, sigma=0.1, reach=1)[:2], T0, 30, AR.ZERO_THRESHOLD)
    p.setflags(write=False)
    return p, T0, ref, want


@BOTH
def test_dense_align_recovers_the_pose_of_the_zero_residual_problem(fmx_mod, on_device):
    p, T0, ref, want = _zero_residual()
    ctx, dref = _pair(fmx_mod, AR.ZERO_W)
    assert _integrate(ctx, dref, p)["merged"] == 0
    got = ctx.dense_align(_arg(p, on_device), T0, reach=1, sigma=0.1, max_iters=30, threshold=AR.ZERO_THRESHOLD)
    assert got["iters"] == want["iters"] == 3 and got["converged"] and want["converged"]
    assert np.abs(got["pose"] - want["pose"]).max() < 1e-6 and np.abs(got["pose"] - I34).max() < 1e-6
    assert got["last_step"] < AR.ZERO_THRESHOLD and got["counts"] == dict(want["counts"], lookups=got["counts"]["lookups"])
    assert got["counts"]["found"] == 48 and got["error"] < 1e-6
    # max_iters = 0: the initial pose; 1: one restated step; neither converged
    zero = ctx.dense_align(_arg(p, on_device), T0, reach=1, sigma=0.1, max_iters=0)
    assert np.array_equal(zero["pose"], T0) and zero["iters"] == 0 and not zero["converged"] and zero["last_step"] == 0.0
    assert zero["error"] == 0.0 and not any(zero["counts"].values())
    one = ctx.dense_align(_arg(p, on_device), T0, reach=1, sigma=0.1, max_iters=1, threshold=AR.ZERO_THRESHOLD)
    S0 = AR.system_from(ref.nearest_voxels, p, T0, sigma=0.1, reach=1)[0]
    step = AR.gn_step(S0, T0)
    assert one["iters"] == 1 and not one["converged"] and np.abs(one["pose"] - step[0]).max() < 1e-6
    assert abs(one["last_step"] - step[1]) < 1e-6 and np.allclose(one["error"], S0[28], rtol=1e-10, atol=0)
    # converged and last_step agree with the threshold on either side of it
    loose = ctx.dense_align(_arg(p, on_device), T0, reach=1, sigma=0.1, max_iters=30, threshold=1.0)
    assert loose["iters"] == 1 and loose["converged"] and loose["last_step"] == one["last_step"] < 1.0
    never = ctx.dense_align(_arg(p, on_device), T0, reach=1, sigma=0.1, max_iters=4, threshold=0.0)
    assert never["iters"] == 4 and not never["converged"] and never["last_step"] >= 0.0
    # the stride: every other point still fixes the pose
    half = ctx.dense_align(_arg(p, on_device), T0, reach=1, sigma=0.1, stride=2, threshold=AR.ZERO_THRESHOLD)
    assert half["converged"] and half["counts"]["skipped"] == 24 and np.abs(half["pose"] - I34).max() < 1e-6


def test_a_singular_system_leaves_pose_out_alone(fmx_mod):
    p, T0, _, _ = _zero_residual()
    ctx, ref = _pair(fmx_mod, AR.ZERO_W)
    _integrate(ctx, ref, p)
    lonely = _pts([(40.5 + k, 30.5, 20.5) for k in range(70)])
    for on_device in (False, True):
        st, out, res = _raw_align(ctx, lonely, T0, on_device)  # nothing found: the zero system
        assert st == STATE and (out == 7.0).all() and res.iters == 0
        st, out, res = _raw_align(ctx, _pts([(1.0, 0.0, 0.0)]), I34, on_device, max_dist2=4.0)  # one pair: H[0][0] = 0
        assert st == STATE and (out == 7.0).all()
        st, out, res = _raw_align(ctx, lonely[:0], T0, on_device)  # no points
        assert st == STATE and (out == 7.0).all()
    st, out, res = _raw_align(ctx, lonely, T0, max_iters=0)
    assert st == 0 and np.array_equal(out.reshape(3, 4), T0) and res.iters == 0
    st, out, _ = _raw_align(ctx, p, T0, null=("result",), threshold=AR.ZERO_THRESHOLD)  # a NULL result is allowed
    assert st == 0 and np.abs(out.reshape(3, 4) - I34).max() < 1e-6


# ------------------------------------------------------------------ 9. status codes
def test_status_codes(fmx_mod):
    fmx = fmx_mod
    reps, q = _few_dozen()
    ctx = _ctx(fmx)
    assert _raw_system(ctx, q, I34, status=True)[0] == STATE  # before fmx_dense_configure
    assert _raw_align(ctx, q, I34)[0] == STATE
    ctx.dense_configure(True, 1.0, 2048)
    ctx.dense_integrate(np.array(reps), I34, 0)
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
        ctx.dense_align(q, I34, reach=9)
    assert e.value.status == INVAL
    off = _ctx(fmx)
    off.dense_configure(True, 1.0, 2048)
    off.dense_configure(False, 1.0, 2048)
    assert _raw_system(off, q, I34, status=True)[0] == STATE and _raw_align(off, q, I34)[0] == STATE  # the map is off


def test_one_launch_per_system_under_the_dense_profile_id(fmx_mod):
    reps, q = _few_dozen()
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ctx.profile(True)
    ctx.dense_integrate(np.array(reps), I34, 0)
    base = ctx.profile_read()["dense"]["launches"]
    ctx.align_system(q, TILT, reach=2)
    assert ctx.profile_read()["dense"]["launches"] == base + 1
    got = ctx.dense_align(q, TILT, reach=2, sigma=0.1, max_iters=3, threshold=0.0)
    assert got["iters"] == 3 and ctx.profile_read()["dense"]["launches"] == base + 4
    _raw_system(ctx, q[:0], I34)  # no points: nothing launched
    assert ctx.profile_read()["dense"]["launches"] == base + 4


# ------------------------------------------------------------------ 10. FORM.dense_localize
def test_form_dense_localize_after_save_and_load(fmx_mod, tmp_path):
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
    got = g.dense_localize(scan, radius, pose_guess=guess, sigma=sigma, max_iters=30, threshold=1e-6)
    reach = math.floor(radius / w) + 1
    direct = g._est.dense_align(scan, guess, reach, radius, sigma, max_iters=30, threshold=1e-6)
    assert np.array_equal(got["pose"], direct["pose"]) and got["iters"] == direct["iters"] >= 2
    assert got["converged"] == direct["converged"]
    fit = g.dense_fitness(scan, radius, pose=got["pose"])
    assert got["n_valid"] == fit["n_valid"] > 500 and got["n_found"] == fit["n_found"] > 500
    assert got["fitness"] == fit["fitness"] and fit["rmse"] > 0.0
    assert abs(got["rmse"] - fit["rmse"]) <= 1e-10 * fit["rmse"], (got["rmse"], fit["rmse"])
    # nearer to where the scan was integrated than the guess was, and better than the guess
    assert np.abs(got["pose"] - truth).max() < np.abs(guess - truth).max()
    assert fit["rmse"] < g.dense_fitness(scan, radius, pose=guess)["rmse"]
    assert g.dense_localize(scan[:, :3], radius, pose_guess=guess, sigma=sigma, stride=4)["n_valid"] < got["n_valid"]
    with pytest.raises(ValueError):
        g.dense_localize(scan, 8 * w, pose_guess=guess)  # reach 9
    # the estimator is not fed: a fresh FORM has no pose to report beyond its initial one
    assert np.array_equal(np.array(g.pose()), np.array(form().pose()))

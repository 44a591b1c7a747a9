"""Scoring many candidate poses of a scan against the dense map on the device (fmx_score_poses;
DESIGN.md §Dense map, Scoring) against the restatement (tests/score_ref.py over
tests/nearest_ref.py) and against the calls that exist (fmx_align_system, fmx_nearest_voxels).
The class counts are compared with equality, sum_d2 within the project's tolerance for an
error term (1e-10 relative, tests/test_gpu_align.py's figure for out[28]) and with 0.0 exactly
where nothing is found, `lookups` within the restatement's bounds and with equality against
fmx_nearest_voxels (the search is reused unchanged); independence and repeatability compare the
32-byte records as bytes.  Tile, chunk and cap come from fmx_score_plan."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import carve_ref as CR
import dense_ref as R
import nearest_ref as NR
import score_cases as SC
import score_ref as SR
from form_amd import synth

pytestmark = pytest.mark.gpu

OK, INVAL, STATE = 0, 1, 5
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
INF = math.inf
CLASSES = SR.CLASSES
FILL = 0xA5  # every byte of a prefilled record


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


def _raw(ctx, p, poses, on_device=False, reach=1, max_dist2=INF, sigma=1.0, min_hits=1, max_miss_ratio=None, stride=1,
         status=False, null=(), n=None, n_poses=None):
    """fmx_score_poses itself (the wrapper squares a distance: max_dist2 goes in as given) over
    records prefilled with FILL: the records, or (status, records)."""
    fmx = _FMX["mod"]
    num, den = fmx.miss_fraction(max_miss_ratio)
    prm = fmx._AlignParams(min_hits, num, den, reach, max_dist2, sigma, stride)
    on_dev, ptr, m, keep = fmx._scan_ptr(_arg(p, on_device))
    if on_dev:
        fmx._ready(keep)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    rec = np.frombuffer(bytearray([FILL]) * (32 * max(len(P), 1)), fmx.SCORE_DTYPE).copy()
    st = fmx.lib().fmx_score_poses(ctx.h, None if "points" in null or not m else ptr, C.c_size_t(m if n is None else n),
                                   C.c_int(on_dev), None if "poses" in null else fmx._p(P if len(P) else np.zeros(12)),
                                   C.c_uint32(len(P) if n_poses is None else n_poses),
                                   None if "params" in null else C.byref(prm), None if "scores" in null else fmx._p(rec))
    del keep
    if status:
        return st, rec
    assert st == OK, (st, ctx._L.fmx_last_error(ctx.h))
    return rec[:len(P)]


def _untouched(rec):
    return rec.tobytes() == bytes([FILL]) * rec.nbytes


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


def _poses(K, seed=1, spread=0.6, about=(0.0, 0.0, 0.0)):
    """K distinct poses: TILT first, then moderate rotations and shifts of up to `spread`."""
    g = np.random.default_rng(seed)
    out = [TILT + _pose(np.zeros((3, 3)), about)]
    for _ in range(K - 1):
        a = g.uniform(-0.5, 0.5, 3)
        out.append(_pose(_rot("z", a[0]) @ _rot("y", a[1]) @ _rot("x", a[2]), np.array(about) + g.uniform(-spread, spread, 3)))
    return np.ascontiguousarray(out)


@functools.lru_cache(maxsize=None)
def _scene():
    """40 representatives in a 5^3 region and 1100 queries around it, some invalid."""
    g = np.random.default_rng(29)
    reps = _pts(g.uniform(-2.5, 2.5, (40, 3)))
    q = _pts(g.uniform(-3.5, 3.5, (1100, 3)))
    q[:, 3] = g.normal(0, 1, len(q))  # w is never read
    q[3, 0], q[64, 2], q[700, 1] = np.nan, np.inf, -np.inf
    q[100, :3] = 0.0
    reps.setflags(write=False)
    q.setflags(write=False)
    return reps, q


@functools.lru_cache(maxsize=None)
def _plan():
    return _FMX["mod"].score_plan(1, 1, 1)


def _same_as_restatement(got, want, kept):
    """The device's records against score_ref's: the first thing that differs, or None."""
    for c in CLASSES:
        if not np.array_equal(got[c], want[c]):
            return c
    if not np.array_equal(sum(got[c].astype(np.int64) for c in CLASSES), np.full(len(got), kept)):
        return "the classes do not sum to the kept points"
    if not np.allclose(got["sum_d2"], want["sum_d2"], rtol=1e-10, atol=0.0):
        return "sum_d2"
    if got["sum_d2"][got["found"] == 0].tobytes() != bytes(8 * int((got["found"] == 0).sum())):
        return "sum_d2 is not +0.0 where nothing is found"
    if not ((want["lookups_lo"] <= got["lookups"]) & (got["lookups"] <= want["lookups_hi"])).all():
        return "lookups"
    return None


def _check(ctx, ref, p, poses, on_device=False, **kw):
    stride = kw.get("stride", 1)
    search = {k: v for k, v in kw.items() if k in ("reach", "min_hits", "max_miss_ratio", "max_dist2")}
    got = _raw(ctx, p, poses, on_device, **kw)
    want = SR.score_poses(ref, p, poses, stride, **search)
    why = _same_as_restatement(got, want, len(range(0, len(p), max(stride, 1))))
    assert why is None, (why, kw, got, want)
    return got


def _check_existing(ctx, p, poses, got, sigma=0.5, **kw):
    """Each record against fmx_align_system at that pose with the same params (the four counts;
    sum_d2 = 2 sigma^2 out[28]) and fmx_nearest_voxels on the kept points (lookups)."""
    fmx = _FMX["mod"]
    stride = kw.get("stride", 1)
    md = math.sqrt(kw.get("max_dist2", INF))
    assert md * md == kw.get("max_dist2", INF)  # (the wrappers square a distance: the tests' limits are exact squares)
    search = dict(reach=kw.get("reach", 1), min_hits=kw.get("min_hits", 1), max_miss_ratio=kw.get("max_miss_ratio"))
    sub = np.ascontiguousarray(np.asarray(p)[::max(stride, 1)])
    for k, T in enumerate(np.asarray(poses).reshape(-1, 3, 4)):
        S, cnt = ctx.align_system(p, T, max_dist=md, sigma=sigma, stride=stride, **search)
        assert {c: int(got[c][k]) for c in CLASSES} == {c: cnt[c] for c in CLASSES}, (k, kw)
        assert math.isclose(float(got["sum_d2"][k]), 2.0 * sigma * sigma * float(S[28]), rel_tol=1e-10, abs_tol=0.0), (k, kw)
        near = ctx.nearest_voxels(sub, T, max_dist=md, **search)
        assert int(got["lookups"][k]) == near["counts"]["lookups"] == cnt["lookups"], (k, kw)
        assert math.isclose(float(got["sum_d2"][k]), math.fsum(near["dist2"][near["state"] == fmx.PROBE_SOLID]),
                            rel_tol=1e-10, abs_tol=0.0)


# ------------------------------------------------------------------ 1. shapes
KEPT = {"1": lambda t: 1, "63": lambda t: 63, "64": lambda t: 64, "65": lambda t: 65, "tile-1": lambda t: t - 1,
        "tile": lambda t: t, "tile+1": lambda t: t + 1, "3tile+5": lambda t: 3 * t + 5}


@pytest.mark.parametrize("kept", list(KEPT))
def test_wave_and_tile_edges_against_the_restatement_and_the_calls_that_exist(fmx_mod, kept):
    reps, q = _scene()
    m = KEPT[kept](_plan()["tile"])
    assert m <= len(q) and fmx_mod.score_plan(m, 1, 1)["tiles"] == (m + _plan()["tile"] - 1) // _plan()["tile"]
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    found = 0
    for K in (1, 2, 7):
        got = _check(ctx, ref, q[:m], _poses(K, seed=K), reach=1)
        found += int(got["found"].sum())
    assert found > (m if m >= 63 else -1)
    many = _poses(65, seed=65)
    got = _raw(ctx, q[:m], many, reach=2, max_dist2=2.25)
    _check_existing(ctx, q[:m], many, got, reach=2, max_dist2=2.25)
    _check(ctx, ref, q[:m], many[:2], reach=2, max_dist2=2.25)
    for k in (0, 1, 33, 64):  # each record is the K = 1 call's
        assert _raw(ctx, q[:m], many[k:k + 1], reach=2, max_dist2=2.25).tobytes() == got[k:k + 1].tobytes(), k


def test_more_items_than_the_grid_cap(fmx_mod):
    """cap + 50 poses of 64 points, one item each: the grid stride takes a second pass.  The
    restatement at reach 0 (one cell per point); at reach 1 the records at the seam equal the
    K = 1 calls'."""
    reps, q = _scene()
    cap = _plan()["cap"]
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    poses = _poses(cap + 50, seed=7, spread=1.5)
    assert fmx_mod.score_plan(64, 1, len(poses))["tiles"] * len(poses) > cap
    p = q[110:174]
    got = _check(ctx, ref, p, poses, reach=0)
    assert len(set(got["found"].tolist())) > 5  # the poses differ in what they find
    wide = _raw(ctx, p, poses, reach=1)
    for k in (0, cap - 1, cap, cap + 1, cap + 49):
        assert _raw(ctx, p, poses[k:k + 1], reach=1).tobytes() == wide[k:k + 1].tobytes(), k
    assert wide["found"].sum() > got["found"].sum()


def test_more_poses_than_a_chunk(fmx_mod):
    """chunk + 1 poses of 5 points at reach 0, repeats of 7 distinct poses, so the restatement
    computes 7: the second chunk's one pose is staged and scored like the first's."""
    reps, q = _scene()
    chunk = _plan()["chunk"]
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    seven = _poses(7, seed=11, spread=0.3)
    which = np.arange(chunk + 1) % 7
    which[-1] = 1  # (not what the cycle would put there)
    p = np.ascontiguousarray(reps[:5])  # on representatives at the identity: reach 0 finds some at the poses near it
    assert fmx_mod.score_plan(5, 1, chunk + 1)["chunks"] == 2
    got = _check(ctx, ref, p, seven[which], reach=0)
    first = _raw(ctx, p, seven, reach=0)
    assert got.tobytes() == first[which].tobytes() and first["found"].sum() > 0
    assert len({first[k:k + 1].tobytes() for k in range(7)}) > 1


@pytest.mark.parametrize("n", [100, 770])
def test_strides_that_do_not_divide_the_points(fmx_mod, n):
    reps, q = _scene()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    poses = _poses(3, seed=5)
    for stride in (3, 0, n + 5):
        got = _check(ctx, ref, q[:n], poses, reach=1, stride=stride)
        sub = _raw(ctx, np.ascontiguousarray(q[:n][::max(stride, 1)]), poses, reach=1)
        assert got.tobytes() == sub.tobytes()  # the kept points alone, in a call of their own
    _check_existing(ctx, q[:n], poses, _raw(ctx, q[:n], poses, reach=1, stride=3), reach=1, stride=3)


# ------------------------------------------------------------------ 2. classes and edges
def test_invalid_points_and_poses_that_put_points_out_of_range(fmx_mod):
    reps, q = _scene()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    p = np.concatenate([_pts([(np.nan, 1, 1), (1, np.inf, 1), (0, 0, 0), (1, 1, -np.inf)]), q[200:260], _pts([(2e6, 0.5, 0.5)])])
    # in range at the identity, out of range 3e6 m away; the last point is out of range at both
    # and comes back into range under the third pose
    poses = np.ascontiguousarray([I34, _pose(np.eye(3), (3e6, 0.0, -3e6)), _pose(np.eye(3), (-1.5e6, 0.0, 0.0)), TILT])
    got = _check(ctx, ref, p, poses, reach=2)
    assert got["invalid"].tolist() == [4] * 4 and got["out_of_range"].tolist() == [1, 61, 60, 1]
    assert got["found"][0] > 20 and got["found"][2] + got["none"][2] == 1 and got["sum_d2"][1] == 0.0
    only_invalid = _check(ctx, ref, p[:4], poses, reach=1)
    assert only_invalid["invalid"].tolist() == [4] * 4 and not only_invalid["lookups"].any()


def test_poses_far_from_the_identity_and_from_the_origin(fmx_mod):
    reps, q = _scene()
    ctx, ref = _pair(fmx_mod)
    far = _pose(_rot("y", 2.5) @ _rot("z", -1.9), (1e5 + 0.25, -1e5 - 0.5, 512.75))
    _integrate(ctx, ref, reps, far)
    poses = [far, far @ np.vstack([TILT, [0, 0, 0, 1.0]])]
    for k in range(3):
        step = _pose(_rot("x", 0.3 * (k + 1)) @ _rot("z", -0.2 * k), (0.2 * k, -0.1, 0.3))
        poses.append(far @ np.vstack([step, [0, 0, 0, 1.0]]))
    poses = np.ascontiguousarray(poses)
    p = np.concatenate([reps[:20], q[:200]])
    got = _check(ctx, ref, p, poses, reach=2)
    assert got["found"][0] > 100 and (got["found"][1:] > 40).all() and got["out_of_range"].sum() == 0
    _check_existing(ctx, p, poses, got, reach=2)


def test_max_dist2_equal_to_a_winners_d2_admits_it_and_just_below_does_not(fmx_mod):
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, _pts([(0.3, 0.6, 0.2), (5.5, 5.5, 5.5)]))
    p = _pts([(0.7, 0.1, 0.9), (5.25, 5.5, 5.75)])
    poses = np.ascontiguousarray([I34, TILT])
    near = [ctx.nearest_voxels(p, T, reach=1) for T in poses]
    d2 = float(near[0]["dist2"][0])
    assert near[0]["counts"]["found"] == 2 and d2 > near[0]["dist2"][1] > 0.0
    at = _check(ctx, ref, p, poses, reach=1, max_dist2=d2)
    below = _check(ctx, ref, p, poses, reach=1, max_dist2=float(np.nextafter(d2, 0.0)))
    assert at["found"][0] == 2 and below["found"][0] == 1 and below["none"][0] == 1
    assert at["sum_d2"][0] == d2 + float(near[0]["dist2"][1]) and below["sum_d2"][0] == float(near[0]["dist2"][1])
    zero = _check(ctx, ref, np.concatenate([_pts([(0.3, 0.6, 0.2)]), p]), poses, reach=1, max_dist2=0.0)
    assert zero["found"].tolist() == [1, 0] and zero["sum_d2"][0] == 0.0  # coincident points only: found, and a sum of 0


def test_filter_by_hits_and_by_misses(fmx_mod):
    A, B = (1.5, 0.5, 0.5), (0.5, 2.5, 0.5)  # A nearer with one hit, B farther with two
    q = _pts([(0.5, 0.5, 0.5), (0.75, 0.25, 0.5), (1.25, 1.5, 0.25)])
    ctx, ref = _pair(fmx_mod)
    for k, r in enumerate((B, B, A)):
        _integrate(ctx, ref, _pts([r]), I34, k)
    ctx.carve_configure(margin=0)
    ref.carve_configure(margin=0)
    poses = np.ascontiguousarray([I34, _pose(np.eye(3), (0.1, 0.0, 0.0))])
    one = _check(ctx, ref, q, poses, reach=2)
    two = _check(ctx, ref, q, poses, reach=2, min_hits=2)
    assert two["found"].tolist() == [3, 3] and (two["sum_d2"] > one["sum_d2"]).all()
    assert _check(ctx, ref, q, poses, reach=2, min_hits=3)["none"].tolist() == [3, 3]
    T, through = CR.special_pose((0.5, 0.5, 0.5)), _pts([(2.0, 0, 0), (2.25, 0, 0)])
    assert ctx.carve_rays(through, T) == ref.carve_rays(through, T)
    assert ref.misses == {R.pack_key(1, 0, 0): 2}  # A: 2 misses on 1 hit
    for ratio, same_as in ((1.0, two), (1.99, two), (2.0, one), (None, one)):
        got = _check(ctx, ref, q, poses, reach=2, max_miss_ratio=ratio)
        assert all(got[f].tobytes() == same_as[f].tobytes() for f in CLASSES + ("sum_d2",)), ratio  # (not the lookups)
    _check_existing(ctx, q, poses, two, reach=2, min_hits=2)


# ------------------------------------------------------------------ 3. independence and repeatability
def test_records_are_functions_of_their_own_pose_bit_for_bit(fmx_mod):
    reps, q = _scene()
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    tile = _plan()["tile"]
    p = q[:3 * tile + 5]
    poses = _poses(23, seed=3)
    kw = dict(reach=2, max_dist2=4.0, stride=1)
    base = _raw(ctx, p, poses, **kw)
    assert base["found"].min() > 100 and len({base[k:k + 1].tobytes() for k in range(23)}) == 23
    perm = np.random.default_rng(4).permutation(23)
    assert _raw(ctx, p, poses[perm], **kw).tobytes() == base[perm].tobytes()  # a permuted list: permuted records
    dup = np.array([5, 5, 0, 22, 5, 0])
    assert _raw(ctx, p, poses[dup], **kw).tobytes() == base[dup].tobytes()  # duplicates: identical records
    for k in range(23):
        assert _raw(ctx, p, poses[k:k + 1], **kw).tobytes() == base[k:k + 1].tobytes(), k  # the K = 1 call's
    assert _raw(ctx, p, poses, **kw).tobytes() == base.tobytes()  # twice
    assert _raw(ctx, p, poses, True, **kw).tobytes() == base.tobytes()  # from a device pointer
    strided = _raw(ctx, p, poses, False, reach=2, max_dist2=4.0, stride=3)
    assert _raw(ctx, p, poses, True, reach=2, max_dist2=4.0, stride=3).tobytes() == strided.tobytes() != base.tobytes()
    # the wrapper: the same records as arrays
    got = ctx.score_poses(_arg(p, True), poses, reach=2, max_dist=2.0)
    assert all(np.array_equal(got[f], base[f]) and got[f].dtype == base[f].dtype for f in fmx_mod.SCORE_FIELDS)
    assert sorted(got) == sorted(fmx_mod.SCORE_FIELDS)


# ------------------------------------------------------------------ 4. reads only
def test_the_call_changes_nothing(fmx_mod):
    reps, q = _scene()
    ctx, ref = _pair(fmx_mod, carve=dict(margin=0))
    _integrate(ctx, ref, reps)
    _integrate(ctx, ref, q[200:260], TILT, 1)
    through = _pts([(2.0, 0.5, 0.25), (2.25, -1.0, 0.5), (-3.0, 1.5, 2.0)])
    assert ctx.carve_rays(through, I34) == ref.carve_rays(through, I34)
    ctx.normals_build(reach=2, min_support=3, max_flatness=1.0)
    L = fmx_mod.lib()

    def pose_now():
        T = np.full(12, 3.0)
        return L.fmx_current_pose(ctx.h, fmx_mod._p(T)), T.tobytes()

    def table():
        d = ctx.dense_download(min_hits=1, misses=True)
        order = np.lexsort(d["points"].T)
        return {k: v[order].tobytes() for k, v in d.items()}

    def state():
        return (ctx.dense_stats(), table(), ctx.normals_stats(), pose_now(), ctx.dense_last(), ctx.carve_last())

    p, poses = q[:300], _poses(9, seed=8)
    point = ctx.align_system(p, TILT, reach=2, sigma=0.1)
    plane = ctx.plane_system(p, TILT, reach=2, sigma=0.1)
    before = state()
    assert before[2]["current"] and plane[1]["found"] > 20 and point[1]["found"] > 100
    for dev in (False, True):
        got = _raw(ctx, p, poses, dev, reach=2, stride=2)
        assert got["found"].min() > 20
        after = state()
        assert after == before and after[2]["current"]
    again_point, again_plane = ctx.align_system(p, TILT, reach=2, sigma=0.1), ctx.plane_system(p, TILT, reach=2, sigma=0.1)
    assert again_point[0].tobytes() == point[0].tobytes() and again_point[1] == point[1]
    assert again_plane[0].tobytes() == plane[0].tobytes() and again_plane[1] == plane[1]


# ------------------------------------------------------------------ 5. status codes
def test_status_codes_and_what_each_leaves_in_scores(fmx_mod):
    reps, q = _scene()
    p, poses = q[:70], _poses(4, seed=2)
    off = _ctx(fmx_mod)
    st, rec = _raw(off, p, poses, status=True)
    assert st == STATE and _untouched(rec)  # the dense map is not configured
    off.dense_configure(True, 1.0, 2048)
    off.dense_configure(False)
    assert _raw(off, p, poses, status=True)[0] == STATE  # ... nor enabled
    ctx, ref = _pair(fmx_mod)
    _integrate(ctx, ref, reps)
    refused = [dict(null=("params",)), dict(null=("poses",)), dict(null=("scores",)), dict(null=("points",)),
               dict(n_poses=fmx_mod.SCORE_MAX_POSES + 1), dict(n=1 << 32), dict(reach=fmx_mod.NEAREST_MAX_REACH + 1),
               dict(max_dist2=math.nan), dict(max_dist2=-1.0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=math.nan),
               dict(sigma=INF)]
    for kw in refused:
        st, rec = _raw(ctx, p, poses, status=True, **kw)
        assert st == INVAL and _untouched(rec), kw
    for k, e, bad in ((0, 0, math.nan), (2, 7, INF), (3, 11, -INF)):  # any entry of any pose
        B = poses.copy()
        B.reshape(-1, 12)[k, e] = bad
        st, rec = _raw(ctx, p, B, status=True)
        assert st == INVAL and _untouched(rec), (k, e)
    # no poses: nothing written, whatever else is there
    for kw in (dict(), dict(null=("poses", "scores")), dict(null=("points",), n=0)):
        st, rec = _raw(ctx, p, poses[:0], status=True, **kw)
        assert st == OK and _untouched(rec), kw
    # no points: all-zero records
    for dev in (False, True):
        st, rec = _raw(ctx, p[:0], poses, dev, status=True)
        assert st == OK and rec.tobytes() == bytes(rec.nbytes)
    st, rec = _raw(ctx, p, poses, status=True, null=("points",), n=0)
    assert st == OK and rec.tobytes() == bytes(rec.nbytes)
    ok = _check(ctx, ref, p[:24], poses[:2], reach=fmx_mod.NEAREST_MAX_REACH, max_dist2=0.25)  # the limits themselves pass
    assert ok["found"].sum() > 0
    with pytest.raises(fmx_mod.FmxError):
        ctx.score_poses(p, np.zeros((fmx_mod.SCORE_MAX_POSES + 1, 12)))


# ------------------------------------------------------------------ 6. FORM.dense_score and FORM.dense_relocalize
def test_relocalize_on_the_ranking_fixture(fmx_mod):
    world, scan, cands, truth = SC.ranking_fixture()
    f = fmx_mod.FORM()
    f.set_dense_map(True, voxel_width=SC.WIDTH, max_voxels=SC.CAPACITY, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    f.initialize()
    ref = NR.NearestRef(SC.WIDTH, SC.CAPACITY, *GATE)
    _integrate(f._est, ref, world)
    reach = math.floor(SC.RADIUS / SC.WIDTH) + 1
    want = SR.score_poses(ref, scan, cands, 1, reach=reach, max_dist=SC.RADIUS)
    pose_before = fmx_mod.lib().fmx_current_pose(f._est.h, fmx_mod._p(np.zeros(12)))
    got = f.dense_relocalize(scan, SC.RADIUS, cands, top=3, sigma=0.1, max_iters=10, threshold=1e-9)
    assert list(got["ranking"]) == SR.rank_scores(want) and got["ranking"][0] == truth == got["candidate"]
    s = got["scores"]
    assert all(np.array_equal(s[c], want[c]) for c in CLASSES) and np.allclose(s["sum_d2"], want["sum_d2"], rtol=1e-10, atol=0)
    assert (np.delete(s["found"], truth) < s["found"][truth]).all()
    # dense_fitness's figures per pose
    for k in (truth, int(got["ranking"][1])):
        fit = f.dense_fitness(scan, SC.RADIUS, pose=cands[k])
        assert (s["n_valid"][k], s["found"][k], s["fitness"][k]) == (fit["n_valid"], fit["n_found"], fit["fitness"])
        assert math.isclose(s["rmse"][k], fit["rmse"], rel_tol=1e-9, abs_tol=0.0)
    by_hand = f.dense_localize(scan, SC.RADIUS, cands[truth], sigma=0.1, max_iters=10, threshold=1e-9)
    assert sorted(set(got) - {"candidate", "ranking", "scores"}) == sorted(by_hand)
    for k, v in by_hand.items():
        assert (got[k].tobytes() == v.tobytes()) if isinstance(v, np.ndarray) else (got[k] == v), k
    assert got["n_found"] == len(scan) and np.abs(got["pose"] - cands[truth]).max() < 1e-5
    assert fmx_mod.lib().fmx_current_pose(f._est.h, fmx_mod._p(np.zeros(12))) == pose_before  # the estimator is as before
    # a stride of its own for the scoring, and the default one
    strided = f.dense_relocalize(scan, SC.RADIUS, cands, top=1, score_stride=2, sigma=0.1, max_iters=10, threshold=1e-9)
    assert strided["candidate"] == truth and strided["scores"]["found"][truth] == len(scan[::2])
    assert strided["pose"].tobytes() == got["pose"].tobytes()

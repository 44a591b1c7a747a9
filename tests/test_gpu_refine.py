"""Refining many candidate poses of a scan against the dense map on the device
(fmx_refine_systems, fmx_refine_poses; DESIGN.md §Dense map, Refining) against the restatement
(tests/refine_ref.py over tests/nearest_ref.py, tests/align_ref.py and tests/plane_ref.py) and
against the calls that exist (fmx_align_system, fmx_plane_system, fmx_align_dense,
fmx_plane_align).  The class counts and `lookups` are compared with equality, the 28 + 1 sums
with tests/test_gpu_align.py's measure (1e-10 relative to the system's largest entry; the error
1e-10 relative) and with +0.0 exactly where nothing is found; independence and repeatability
compare the 264-byte records as bytes.  Tile, chunk and cap come from fmx_refine_plan."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import align_ref as AR
import carve_ref as CR
import dense_ref as R
import nearest_ref as NR
import normals_ref as MR
import plane_ref as PL
import refine_ref as RR
import score_cases as SC
from form_amd import synth

pytestmark = pytest.mark.gpu

OK, INVAL, STATE = 0, 1, 5
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
INF = math.inf
CLASSES = RR.CLASSES
FILL = 0xA5  # every byte of a prefilled record
FIX = dict(reach=1, min_support=5, max_flatness=0.05)  # tests/test_gpu_plane.py's build: some winners stay unoriented
FORMS = pytest.mark.parametrize("form", ["point", "plane"])


def _pts(rows):
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return p


def _ctx(fmx):
    p = synth.default_params(synth.ScanGeometry(16, 256, 15.0, 0.01, 0.02))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _arg(p, on_device):
    return torch.from_numpy(np.array(p)).to("cuda:0") if on_device else np.array(p)


_FMX = {}


@pytest.fixture(autouse=True)
def _module(fmx_mod):
    _FMX["mod"] = fmx_mod


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _pose(Rm, t):
    T = np.zeros((3, 4))
    T[:, :3] = Rm
    T[:, 3] = t
    return T


def _mul(A, B):
    return A @ np.vstack([B, [0, 0, 0, 1.0]])


TILT = _pose(_rot("z", 0.2) @ _rot("x", -0.1), (0.3, -0.2, 0.1))
PLANE_TILT = _pose(_rot("z", 0.02) @ _rot("x", -0.015), (0.05, -0.04, 0.03))  # tests/test_gpu_plane.py's


def _poses(K, seed=1, spread=0.6, turn=0.5, first=TILT):
    """K distinct poses: `first`, then `first` moved by rotations of up to `turn` and shifts of up to `spread`."""
    g = np.random.default_rng(seed)
    out = [first.copy()]
    for _ in range(K - 1):
        a = g.uniform(-turn, turn, 3)
        out.append(_mul(first, _pose(_rot("z", a[0]) @ _rot("y", a[1]) @ _rot("x", a[2]), g.uniform(-spread, spread, 3))))
    return np.ascontiguousarray(out)


@functools.lru_cache(maxsize=None)
def _plan():
    return _FMX["mod"].refine_plan(1, 1, 1)


@functools.lru_cache(maxsize=None)
def _scene(form):
    """point: tests/test_gpu_score.py's scene, 40 representatives in a 5^3 region and queries
    around it.  plane: tests/test_gpu_plane.py's, the normals fixture and queries in the frame of
    its tilt, fixture points moved by up to 0.4, some far from the map.  3 tiles + 5 queries
    each, some invalid.  (the map's points, the queries, the restated map, the poses' centre)"""
    n = 3 * _plan()["tile"] + 5
    ref = NR.NearestRef(1.0, 2048, *GATE)
    if form == "point":
        g = np.random.default_rng(29)
        reps = _pts(g.uniform(-2.5, 2.5, (40, 3)))
        q = _pts(g.uniform(-3.5, 3.5, (n, 3)))
        first = TILT
    else:
        g = np.random.default_rng(59)
        reps = MR.fixture()
        w = reps[g.integers(0, len(reps), n), :3].astype(np.float64) + g.uniform(-0.4, 0.4, (n, 3))
        w[::16] += 30.0  # nothing within reach
        q = _pts((w - PLANE_TILT[:, 3]) @ PLANE_TILT[:, :3])
        first = PLANE_TILT
    ref.integrate(reps, I34, 0)
    q[:, 3] = g.normal(0, 1, len(q))  # w is never read
    q[3, 0], q[64, 2], q[700, 1] = np.nan, np.inf, -np.inf
    q[100, :3] = 0.0
    reps.setflags(write=False)
    q.setflags(write=False)
    return reps, q, ref, first


def _map(fmx, form, carve=None):
    """A context holding the scene (plane: with a current snapshot) and plane_ref's normal_at
    from the device's download (None in the point form)."""
    reps, _, _, _ = _scene(form)
    ctx = _ctx(fmx)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    if carve is not None:
        ctx.carve_configure(**carve)
    ctx.dense_integrate(np.array(reps), I34, 0)
    if form == "point":
        return ctx, None
    ctx.normals_build(**FIX)
    d = ctx.normals_download(oriented_only=False)
    return ctx, PL.by_owner(d["scan"], d["index"], d["normals"])


def _call_args(p, poses, on_device, reach, max_dist2, sigma, min_hits, max_miss_ratio, stride, null, n, n_poses):
    fmx = _FMX["mod"]
    num, den = fmx.miss_fraction(max_miss_ratio)
    prm = fmx._AlignParams(min_hits, num, den, reach, max_dist2, sigma, stride)
    on_dev, ptr, m, keep = fmx._scan_ptr(_arg(p, on_device))
    if on_dev:
        fmx._ready(keep)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    head = (None if "points" in null or not m else ptr, C.c_size_t(m if n is None else n), C.c_int(on_dev),
            None if "poses" in null else fmx._p(P if len(P) else np.zeros(12)), C.c_uint32(len(P) if n_poses is None else n_poses),
            None if "params" in null else C.byref(prm))
    return head, P, (keep, prm)


def _raw(ctx, p, poses, on_device=False, plane=False, reach=1, max_dist2=INF, sigma=1.0, min_hits=1, max_miss_ratio=None,
         stride=1, status=False, null=(), n=None, n_poses=None):
    """fmx_refine_systems itself (the wrapper squares a distance: max_dist2 goes in as given) over
    records prefilled with FILL: the records, or (status, records)."""
    fmx = _FMX["mod"]
    head, P, keep = _call_args(p, poses, on_device, reach, max_dist2, sigma, min_hits, max_miss_ratio, stride, null, n, n_poses)
    rec = np.frombuffer(bytearray([FILL]) * (264 * max(len(P), 1)), fmx.REFINE_SYSTEM_DTYPE).copy()
    st = fmx.lib().fmx_refine_systems(ctx.h, *head, C.c_int(int(plane)), None if "out" in null else fmx._p(rec))
    del keep
    if status:
        return st, rec
    assert st == OK, (st, ctx._L.fmx_last_error(ctx.h))
    return rec[:len(P)]


def _raw_loop(ctx, p, poses, on_device=False, plane=False, reach=1, max_dist2=INF, sigma=0.1, stride=1, max_iters=30,
              threshold=1e-6, null=(), n=None, n_poses=None):
    """fmx_refine_poses itself over outputs prefilled with FILL: (status, poses_out, results)."""
    fmx = _FMX["mod"]
    head, P, keep = _call_args(p, poses, on_device, reach, max_dist2, sigma, 1, None, stride, null, n, n_poses)
    K = max(len(P), 1)
    out = np.frombuffer(bytearray([FILL]) * (96 * K), np.float64).copy().reshape(K, 12)
    res = np.frombuffer(bytearray([FILL]) * (64 * K), fmx.REFINE_RESULT_DTYPE).copy()
    st = fmx.lib().fmx_refine_poses(ctx.h, *head, C.c_int(int(plane)), C.c_uint32(max_iters), C.c_double(threshold),
                                    None if "poses_out" in null else fmx._p(out), None if "results" in null else fmx._p(res))
    del keep
    cut = len(P) if st == OK and len(P) else K  # (refused, or no poses: the whole prefilled buffers)
    return st, out[:cut], res[:cut]


def _untouched(*arrays):
    return all(a.tobytes() == bytes([FILL]) * a.nbytes for a in arrays)


def _close(got, want):
    """tests/test_gpu_align.py's measure: the 28 entries relative to the largest, the error relative."""
    scale = np.abs(want[:28]).max() + 1e-300
    return bool(np.all(np.abs(got[:28] - want[:28]) <= 1e-10 * scale) and np.allclose(got[28], want[28], rtol=1e-10, atol=0))


def _same_as_restatement(got, want, kept):
    """The device's records against refine_ref's: the first thing that differs, or None."""
    for c in CLASSES:
        if not np.array_equal(got[c], want[c]):
            return c
    if not np.array_equal(sum(got[c].astype(np.int64) for c in CLASSES), np.full(len(got), kept)):
        return "the classes do not sum to the kept points"
    if got["reserved"].any():
        return "reserved"
    for k in range(len(got)):
        if not _close(got["system"][k], want["system"][k]):
            return f"system {k}: off by {np.abs(got['system'][k] - want['system'][k]).max()}"
        if got["found"][k] == 0 and got["system"][k].tobytes() != bytes(232):
            return f"system {k} is not +0.0 where nothing is found"
    if not ((want["lookups_lo"] <= got["lookups"]) & (got["lookups"] <= want["lookups_hi"])).all():
        return "lookups"
    return None


def _check(ctx, ref, p, poses, on_device=False, normal_at=None, **kw):
    stride = kw.get("stride", 1)
    search = {k: v for k, v in kw.items() if k in ("reach", "min_hits", "max_miss_ratio", "max_dist2")}
    got = _raw(ctx, p, poses, on_device, plane=normal_at is not None, **kw)
    want = RR.systems(ref, p, poses, kw.get("sigma", 1.0), stride, normal_at, **search)
    why = _same_as_restatement(got, want, len(range(0, len(p), max(stride, 1))))
    assert why is None, (why, kw, got, want)
    return got


def _check_existing(ctx, p, poses, got, plane=False, **kw):
    """Each record against fmx_align_system / fmx_plane_system at that pose with the same params:
    the system within the measure (the order of the sums is another), the counts and lookups equal."""
    md2 = kw.pop("max_dist2", INF)
    md = math.sqrt(md2)
    assert md * md == md2  # (the wrappers square a distance: the tests' limits are exact squares)
    call = ctx.plane_system if plane else ctx.align_system
    for k, T in enumerate(np.asarray(poses).reshape(-1, 3, 4)):
        S, cnt = call(p, T, max_dist=md, **kw)
        assert _close(got["system"][k], S), (k, kw, np.abs(got["system"][k] - S).max())
        assert {c: int(got[c][k]) for c in CLASSES} == {c: cnt.get(c, 0) for c in CLASSES}, (k, kw)
        assert int(got["lookups"][k]) == cnt["lookups"], (k, kw)


# ------------------------------------------------------------------ 1. shapes
KEPT = {"1": lambda t: 1, "63": lambda t: 63, "64": lambda t: 64, "65": lambda t: 65, "tile-1": lambda t: t - 1,
        "tile": lambda t: t, "tile+1": lambda t: t + 1, "3tile+5": lambda t: 3 * t + 5}


@FORMS
@pytest.mark.parametrize("kept", list(KEPT))
def test_wave_and_tile_edges_against_the_restatement_and_the_calls_that_exist(fmx_mod, form, kept):
    reps, q, ref, first = _scene(form)
    tile = _plan()["tile"]
    m = KEPT[kept](tile)
    assert m <= len(q) and fmx_mod.refine_plan(m, 1, 1)["tiles"] == (m + tile - 1) // tile
    ctx, normal_at = _map(fmx_mod, form)
    plane = form == "plane"
    seven = _poses(7, seed=7, spread=0.3 if plane else 0.6, turn=0.05 if plane else 0.5, first=first)
    found = unoriented = 0
    for K in (1, 2, 7):  # (prefixes of one list: the restatement computes seven systems)
        got = _check(ctx, ref, q[:m], seven[:K], normal_at=normal_at, reach=1, sigma=0.5)
        _check_existing(ctx, q[:m], seven[:K], got, plane, reach=1, sigma=0.5)
        found += int(got["found"].sum())
        unoriented += int(got["unoriented"].sum())
    assert found > (m if m >= 63 else -1)
    assert unoriented > (m // 16 if m >= 63 else -1) if plane else unoriented == 0
    wide = _raw(ctx, q[:m], seven, plane=plane, reach=2, max_dist2=2.25, sigma=0.1)
    _check_existing(ctx, q[:m], seven, wide, plane, reach=2, max_dist2=2.25, sigma=0.1)


# ------------------------------------------------------------------ 2. independence and repeatability
@FORMS
def test_records_are_functions_of_their_own_pose_byte_for_byte(fmx_mod, form):
    reps, q, ref, first = _scene(form)
    ctx, normal_at = _map(fmx_mod, form)
    plane = form == "plane"
    poses = _poses(65, seed=65, spread=0.3 if plane else 0.6, turn=0.05 if plane else 0.5, first=first)
    kw = dict(plane=plane, reach=2, max_dist2=4.0, sigma=0.1)
    base = _raw(ctx, q, poses, **kw)
    assert base["found"].min() > 100 and len({base[k:k + 1].tobytes() for k in range(65)}) == 65
    for k in (0, 1, 33, 64):  # each record is the one-pose call's
        assert _raw(ctx, q, poses[k:k + 1], **kw).tobytes() == base[k:k + 1].tobytes(), k
    perm = np.random.default_rng(4).permutation(65)
    assert _raw(ctx, q, poses[perm], **kw).tobytes() == base[perm].tobytes()  # a permuted list: permuted records
    dup = np.array([5, 5, 0, 64, 5, 0])
    assert _raw(ctx, q, poses[dup], **kw).tobytes() == base[dup].tobytes()  # duplicates: identical records
    assert _raw(ctx, q, poses, **kw).tobytes() == base.tobytes()  # twice
    assert _raw(ctx, q, poses, True, **kw).tobytes() == base.tobytes()  # from a device pointer
    strided = _raw(ctx, q, poses, False, stride=3, **kw)
    assert _raw(ctx, q, poses, True, stride=3, **kw).tobytes() == strided.tobytes() != base.tobytes()
    # the wrapper: the same records as arrays
    got = ctx.refine_systems(_arg(q, True), poses, reach=2, max_dist=2.0, sigma=0.1, plane=plane)
    assert sorted(got) == sorted(fmx_mod.REFINE_SYSTEM_FIELDS) and got["system"].shape == (65, 29)
    assert all(np.array_equal(got[f], base[f]) and got[f].dtype == base[f].dtype for f in fmx_mod.REFINE_SYSTEM_FIELDS)


# ------------------------------------------------------------------ 3. grid and chunk seams
def test_more_items_than_the_grid_cap(fmx_mod):
    """cap + 50 poses of 64 points, one item each: the grid stride takes a second pass.  The
    restatement at reach 0 (one cell per point); at reach 1 the records at the seam equal the
    one-pose calls'."""
    reps, q, ref, _ = _scene("point")
    cap = _plan()["cap"]
    ctx, _ = _map(fmx_mod, "point")
    poses = _poses(cap + 50, seed=7, spread=1.5)
    assert fmx_mod.refine_plan(64, 1, len(poses))["tiles"] * len(poses) > cap
    p = q[110:174]
    got = _check(ctx, ref, p, poses, reach=0)
    assert len(set(got["found"].tolist())) > 5  # the poses differ in what they find
    wide = _raw(ctx, p, poses, reach=1)
    for k in (0, cap - 1, cap, cap + 1, cap + 49):
        assert _raw(ctx, p, poses[k:k + 1], reach=1).tobytes() == wide[k:k + 1].tobytes(), k
    assert wide["found"].sum() > got["found"].sum()


@FORMS
def test_more_poses_than_a_chunk(fmx_mod, form):
    """chunk + 1 poses of 5 points, repeats of 7 distinct poses, so the restatement computes 7:
    the second chunk's one pose is staged and evaluated like the first's."""
    reps, q, ref, first = _scene(form)
    chunk = _plan()["chunk"]
    ctx, normal_at = _map(fmx_mod, form)
    plane = form == "plane"
    seven = _poses(7, seed=11, spread=0.3, turn=0.05 if plane else 0.5, first=I34 if not plane else first)
    which = np.arange(chunk + 1) % 7
    which[-1] = 1  # (not what the cycle would put there)
    p = np.ascontiguousarray(reps[:5]) if not plane else np.ascontiguousarray(q[5:10])
    reach = 0 if not plane else 1
    assert fmx_mod.refine_plan(5, 1, chunk + 1)["chunks"] == 2
    got = _check(ctx, ref, p, seven[which], normal_at=normal_at, reach=reach)
    firsts = _raw(ctx, p, seven, plane=plane, reach=reach)
    assert got.tobytes() == firsts[which].tobytes() and firsts["found"].sum() > 0
    assert len({firsts[k:k + 1].tobytes() for k in range(7)}) > 1


# ------------------------------------------------------------------ 4. strides
@FORMS
@pytest.mark.parametrize("n", [100, 770])
def test_strides_that_do_not_divide_the_points(fmx_mod, form, n):
    reps, q, ref, first = _scene(form)
    ctx, normal_at = _map(fmx_mod, form)
    plane = form == "plane"
    poses = _poses(3, seed=5, spread=0.3, turn=0.05 if plane else 0.5, first=first)
    for stride in (3, 0, n + 5):
        got = _check(ctx, ref, q[:n], poses, normal_at=normal_at, reach=1, stride=stride, sigma=0.1)
        sub = _raw(ctx, np.ascontiguousarray(q[:n][::max(stride, 1)]), poses, plane=plane, reach=1, sigma=0.1)
        assert got.tobytes() == sub.tobytes()  # the kept points alone, in a call of their own
    _check_existing(ctx, q[:n], poses, _raw(ctx, q[:n], poses, plane=plane, reach=1, stride=3), plane, reach=1, stride=3)


# ------------------------------------------------------------------ 5. classes and edges
def test_invalid_points_and_poses_that_put_points_out_of_range(fmx_mod):
    reps, q, ref, _ = _scene("point")
    ctx, _ = _map(fmx_mod, "point")
    p = np.concatenate([_pts([(np.nan, 1, 1), (1, np.inf, 1), (0, 0, 0), (1, 1, -np.inf)]), q[200:260], _pts([(2e6, 0.5, 0.5)])])
    # in range at the identity, out of range 3e6 m away; the last point is out of range at both
    # and comes back into range under the third pose; the last pose is far from every voxel
    poses = np.ascontiguousarray([I34, _pose(np.eye(3), (3e6, 0.0, -3e6)), _pose(np.eye(3), (-1.5e6, 0.0, 0.0)), TILT,
                                  _pose(_rot("y", 1.0), (500.0, -400.0, 300.0))])
    got = _check(ctx, ref, p, poses, reach=2)
    assert got["invalid"].tolist() == [4] * 5 and got["out_of_range"].tolist() == [1, 61, 60, 1, 1]
    assert got["found"][0] > 20 and got["found"][2] + got["none"][2] == 1
    for k in (1, 4):  # nothing found: S all +0.0, as bytes
        assert got["found"][k] == 0 and got["system"][k].tobytes() == bytes(232), k
    assert got["none"][4] == 60
    only_invalid = _check(ctx, ref, p[:4], poses, reach=1)
    assert only_invalid["invalid"].tolist() == [4] * 5 and not only_invalid["lookups"].any()
    assert only_invalid["system"].tobytes() == bytes(232 * 5)


@FORMS
def test_poses_far_from_the_identity_and_from_the_origin(fmx_mod, form):
    reps, q, _, first = _scene(form)
    plane = form == "plane"
    far = _pose(_rot("y", 2.5) @ _rot("z", -1.9), (1e5 + 0.25, -1e5 - 0.5, 512.75))
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ref = NR.NearestRef(1.0, 2048, *GATE)
    assert ctx.dense_integrate(np.array(reps), far, 0) == ref.integrate(reps, far, 0)
    normal_at = None
    if plane:
        cnt = ctx.normals_build(**FIX)
        assert cnt["oriented"] > 100
        d = ctx.normals_download(oriented_only=False)
        normal_at = PL.by_owner(d["scan"], d["index"], d["normals"])
    poses = [_mul(far, first)]
    for k in range(3):
        step = _pose(_rot("x", 0.03 * (k + 1)) @ _rot("z", -0.02 * k), (0.2 * k, -0.1, 0.3))
        poses.append(_mul(far, _mul(first, step)))
    poses = np.ascontiguousarray(poses)
    p = np.concatenate([reps[:20], q[:200]])
    got = _check(ctx, ref, p, poses, normal_at=normal_at, reach=2, sigma=0.1)
    assert (got["found"] > 40).all() and got["out_of_range"].sum() == 0
    _check_existing(ctx, p, poses, got, plane, reach=2, sigma=0.1)


def test_filter_by_hits_and_by_misses(fmx_mod):
    A, B = (1.5, 0.5, 0.5), (0.5, 2.5, 0.5)  # A nearer with one hit, B farther with two
    q = _pts([(0.5, 0.5, 0.5), (0.75, 0.25, 0.5), (1.25, 1.5, 0.25)])
    ctx = _ctx(fmx_mod)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ref = NR.NearestRef(1.0, 2048, *GATE)
    for k, r in enumerate((B, B, A)):
        assert ctx.dense_integrate(_pts([r]), I34, k) == ref.integrate(_pts([r]), I34, k)
    ctx.carve_configure(margin=0)
    ref.carve_configure(margin=0)
    poses = np.ascontiguousarray([I34, _pose(np.eye(3), (0.1, 0.0, 0.0))])
    one = _check(ctx, ref, q, poses, reach=2)
    two = _check(ctx, ref, q, poses, reach=2, min_hits=2)
    assert two["found"].tolist() == [3, 3] and (two["system"][:, 28] > one["system"][:, 28]).all()
    assert _check(ctx, ref, q, poses, reach=2, min_hits=3)["none"].tolist() == [3, 3]
    T, through = CR.special_pose((0.5, 0.5, 0.5)), _pts([(2.0, 0, 0), (2.25, 0, 0)])
    assert ctx.carve_rays(through, T) == ref.carve_rays(through, T)
    assert ref.misses == {R.pack_key(1, 0, 0): 2}  # A: 2 misses on 1 hit
    for ratio, same_as in ((1.0, two), (1.99, two), (2.0, one), (None, one)):
        got = _check(ctx, ref, q, poses, reach=2, max_miss_ratio=ratio)
        assert all(got[f].tobytes() == same_as[f].tobytes() for f in CLASSES + ("system",)), ratio  # (not the lookups)
    _check_existing(ctx, q, poses, two, reach=2, min_hits=2)


# ------------------------------------------------------------------ 6. reads only
def test_the_call_changes_nothing(fmx_mod):
    reps, q, _, _ = _scene("point")
    ctx, _ = _map(fmx_mod, "point", carve=dict(margin=0))
    ctx.dense_integrate(np.array(q[200:260]), TILT, 1)
    through = _pts([(2.0, 0.5, 0.25), (2.25, -1.0, 0.5), (-3.0, 1.5, 2.0)])
    ctx.carve_rays(through, I34)
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
        for form in (False, True):
            got = _raw(ctx, p, poses, dev, plane=form, reach=2, stride=2)
            assert got["found"].min() > 5
            st, out, res = _raw_loop(ctx, p, poses, dev, plane=form, reach=2, max_iters=3)
            assert st == OK and res["iters"].min() >= 1
            after = state()
            assert after == before and after[2]["current"]
    again_point, again_plane = ctx.align_system(p, TILT, reach=2, sigma=0.1), ctx.plane_system(p, TILT, reach=2, sigma=0.1)
    assert again_point[0].tobytes() == point[0].tobytes() and again_point[1] == point[1]
    assert again_plane[0].tobytes() == plane[0].tobytes() and again_plane[1] == plane[1]


# ------------------------------------------------------------------ 7. status codes
def test_status_codes_and_what_each_leaves_in_the_outputs(fmx_mod):
    reps, q, ref, _ = _scene("point")
    p, poses = q[:70], _poses(4, seed=2)

    def both(ctx, p, poses, **kw):
        """(statuses, untouched) of the two calls."""
        st, rec = _raw(ctx, p, poses, status=True, **kw)
        lkw = {k: v for k, v in kw.items() if k not in ("min_hits", "max_miss_ratio")}
        if "out" in lkw.get("null", ()):
            lkw["null"] = tuple("poses_out" if x == "out" else x for x in lkw["null"])
        st2, out, res = _raw_loop(ctx, p, poses, **lkw)
        return (st, st2), _untouched(rec, out, res)

    off = _ctx(fmx_mod)
    assert both(off, p, poses) == ((STATE, STATE), True)  # the dense map is not configured
    off.dense_configure(True, 1.0, 2048)
    off.dense_configure(False)
    assert both(off, p, poses) == ((STATE, STATE), True)  # ... nor enabled
    ctx, _ = _map(fmx_mod, "point")
    assert both(ctx, p, poses, plane=True) == ((STATE, STATE), True)  # no normal snapshot
    ctx.normals_build(**FIX)
    assert both(ctx, p, poses, plane=True)[0] == (OK, OK)
    ctx.dense_integrate(np.array(q[300:310]), I34, 1)
    assert both(ctx, p, poses, plane=True) == ((STATE, STATE), True)  # ... a stale one
    assert both(ctx, p, poses)[0] == (OK, OK)
    refused = [dict(null=("params",)), dict(null=("poses",)), dict(null=("out",)), dict(null=("points",)),
               dict(n_poses=fmx_mod.REFINE_MAX_POSES + 1), dict(n=1 << 32), dict(reach=fmx_mod.NEAREST_MAX_REACH + 1),
               dict(max_dist2=math.nan), dict(max_dist2=-1.0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=math.nan),
               dict(sigma=INF)]
    for kw in refused:
        assert both(ctx, p, poses, **kw) == ((INVAL, INVAL), True), kw
    for bad in (math.nan, -1.0):  # the loop's threshold
        st, out, res = _raw_loop(ctx, p, poses, threshold=bad)
        assert st == INVAL and _untouched(out, res), bad
    for k, e, bad in ((0, 0, math.nan), (2, 7, INF), (3, 11, -INF)):  # any entry of any pose
        B = poses.copy()
        B.reshape(-1, 12)[k, e] = bad
        assert both(ctx, p, B) == ((INVAL, INVAL), True), (k, e)
    # no poses: nothing written, whatever else is there
    for kw in (dict(), dict(null=("poses", "out")), dict(null=("points",), n=0)):
        assert both(ctx, p, poses[:0], **kw) == ((OK, OK), True), kw
    # no points: all-zero systems; in the loop every pose is singular at iteration 1
    for dev in (False, True):
        for kw in (dict(), dict(null=("points",), n=0)):
            st, rec = _raw(ctx, p[:0], poses, dev, status=True, **kw)
            assert st == OK and rec.tobytes() == bytes(rec.nbytes)
            st, out, res = _raw_loop(ctx, p[:0], poses, dev, **kw)
            assert st == OK and out.tobytes() == poses.tobytes() and (res["singular"] == 1).all() and (res["iters"] == 1).all()
            assert not res["converged"].any() and not res["found"].any() and not res["error"].any()
    st, out, res = _raw_loop(ctx, p, poses, null=("results",), max_iters=2)  # a NULL results is allowed
    assert st == OK and not _untouched(out) and _untouched(res)
    ok = _check(ctx, ref_with(ref, q[300:310]), p[:24], poses[:2], reach=fmx_mod.NEAREST_MAX_REACH, max_dist2=0.25)
    assert ok["found"].sum() > 0  # the limits themselves pass
    with pytest.raises(fmx_mod.FmxError):
        ctx.refine_systems(p, np.zeros((fmx_mod.REFINE_MAX_POSES + 1, 12)))
    with pytest.raises(fmx_mod.FmxError):
        ctx.refine_poses(p, np.zeros((fmx_mod.REFINE_MAX_POSES + 1, 12)))


def ref_with(ref, more):
    """The scene's restated map after one more integration (the cached one stays as it is)."""
    out = NR.NearestRef(1.0, 2048, *GATE)
    out.integrate(_scene("point")[0], I34, 0)
    out.integrate(more, I34, 1)
    return out


# ------------------------------------------------------------------ 8. the loop
@functools.lru_cache(maxsize=None)
def _zero(form):
    """The zero-residual fixture of tests/test_gpu_align.py / tests/test_gpu_plane.py, its restated
    map (and normals), the three starts Exp(s ZERO_XI) and the threshold."""
    if form == "point":
        p, _ = AR.zero_residual_cloud()
        ref, normal_at, xi, thr, build = NR.NearestRef(AR.ZERO_W, 2048, *GATE), None, AR.ZERO_XI, AR.ZERO_THRESHOLD, None
        assert ref.integrate(p, I34, 0)["merged"] == 0
    else:
        p, _ = PL.zero_residual_cloud()
        ref, xi, thr, build = NR.NearestRef(1.0, 2048, *GATE), PL.ZERO_XI, PL.ZERO_THRESHOLD, PL.ZERO_BUILD
        assert ref.integrate(p, I34, 0)["merged"] == 0
        normal_at = PL.by_owner_of(ref, MR.build(ref, **build))
    starts = np.ascontiguousarray([AR.expmap([s * x for x in xi]) for s in (1.0, 0.5, 0.0)])
    p.setflags(write=False)
    starts.setflags(write=False)
    return p, ref, normal_at, starts, thr, build


def _zero_map(fmx, form):
    p, _, _, _, _, build = _zero(form)
    ctx = _ctx(fmx)
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    assert ctx.dense_integrate(np.array(p), I34, 0)["merged"] == 0
    if build:
        ctx.normals_build(**build)
    return ctx


@FORMS
def test_the_loop_recovers_the_pose_of_the_zero_residual_problem_from_three_starts(fmx_mod, form):
    p, ref, normal_at, starts, thr, _ = _zero(form)
    ctx = _zero_map(fmx_mod, form)
    plane = form == "plane"
    kw = dict(plane=plane, reach=1, sigma=0.1, threshold=thr)
    st, out, res = _raw_loop(ctx, p, starts, **kw)
    assert st == OK
    for k in range(3):
        assert np.abs(out[k].reshape(3, 4) - I34).max() < 1e-6, k
        assert res["last_step"][k] < thr and res["converged"][k] == 1 and res["singular"][k] == 0, k
    assert res["iters"][2] == 1 and res["iters"][0] > 1 and not res["reserved"].any() and not res["reserved2"].any()
    assert (res["found"] + res["unoriented"] + res["none"] == len(p)).all() and (res["found"] > 40).all()
    for k in range(3):  # the batch's poses and results are the one-pose calls'
        st1, o1, r1 = _raw_loop(ctx, p, starts[k:k + 1], **kw)
        assert st1 == OK and o1.tobytes() == out[k:k + 1].tobytes() and r1.tobytes() == res[k:k + 1].tobytes(), k
    for dev in (True,):  # from a device pointer: the same bytes
        st2, o2, r2 = _raw_loop(ctx, p, starts, dev, **kw)
        assert st2 == OK and o2.tobytes() == out.tobytes() and r2.tobytes() == res.tobytes()
    # against the loop that exists, from the same start: the sums' order differs, the poses agree
    alone = ctx.dense_align(p, starts[0].reshape(3, 4), reach=1, sigma=0.1, max_iters=30, threshold=thr, plane=plane)
    assert alone["converged"] and np.abs(alone["pose"].reshape(12) - out[0]).max() < 1e-6
    # max_iters == 0: the input bytes, nothing evaluated
    st0, o0, r0 = _raw_loop(ctx, p, starts, max_iters=0, **kw)
    assert st0 == OK and o0.tobytes() == starts.tobytes() and r0.tobytes() == bytes(r0.nbytes)
    # the wrapper
    got = ctx.refine_poses(p, starts, reach=1, sigma=0.1, threshold=thr, plane=plane)
    assert got["pose"].shape == (3, 3, 4) and got["pose"].tobytes() == out.tobytes()
    assert got["converged"].all() and not got["singular"].any() and np.array_equal(got["iters"], res["iters"])


@FORMS
def test_a_singular_and_a_capped_pose_among_the_others(fmx_mod, form):
    """Five poses: the three starts interleaved with a pose that has nothing in reach (singular)
    and a copy of the first start, all under max_iters = 1 (capped: one restated step)."""
    p, ref, normal_at, starts, thr, _ = _zero(form)
    ctx = _zero_map(fmx_mod, form)
    plane = form == "plane"
    lost = starts[0].copy()
    lost[:, 3] += (300.0, -200.0, 100.0)
    five = np.ascontiguousarray([starts[0], lost, starts[1], starts[0], starts[2]])
    kw = dict(plane=plane, reach=1, sigma=0.1, threshold=thr)
    for max_iters in (1, 30):
        st, out, res = _raw_loop(ctx, p, five, max_iters=max_iters, **kw)
        assert st == OK
        for k in range(5):
            st1, o1, r1 = _raw_loop(ctx, p, five[k:k + 1], max_iters=max_iters, **kw)
            assert st1 == OK and o1.tobytes() == out[k:k + 1].tobytes() and r1.tobytes() == res[k:k + 1].tobytes(), (max_iters, k)
        assert res["singular"].tolist() == [0, 1, 0, 0, 0] and res["converged"][1] == 0 and res["iters"][1] == 1
        assert out[1].tobytes() == lost.tobytes() and res["found"][1] == 0 and res["none"][1] == len(p)
        assert res["error"][1] == 0.0 and res["last_step"][1] == 0.0
        assert out[0].tobytes() == out[3].tobytes() and res[0:1].tobytes() == res[3:4].tobytes()
        if max_iters == 30:
            assert res["converged"].tolist() == [1, 0, 1, 1, 1]
            continue
        # capped: one step of the restated system, to the 1e-6 of the one-iteration test that exists
        assert res["iters"].tolist() == [1] * 5 and res["converged"].tolist() == [0, 0, 0, 0, 1]
        S0, cnt, _ = RR.system_from(ref, p, starts[0], 0.1, 1, normal_at, reach=1)
        step = AR.gn_step(S0, starts[0])
        assert np.abs(out[0].reshape(3, 4) - step[0]).max() < 1e-6 and abs(res["last_step"][0] - step[1]) < 1e-6
        assert np.allclose(res["error"][0], S0[28], rtol=1e-10, atol=0)
        assert {c: int(res[c][0]) for c in CLASSES} == cnt
    # the existing loop refuses the singular pose; the batch reports it
    with pytest.raises(fmx_mod.FmxError):
        ctx.dense_align(p, lost, reach=1, sigma=0.1, plane=plane)


# ------------------------------------------------------------------ 9. FORM.dense_localize_many and dense_relocalize(batched=True)
def _form(fmx_mod):
    world, scan, cands, truth = SC.ranking_fixture()
    f = fmx_mod.FORM()
    f.set_dense_map(True, voxel_width=SC.WIDTH, max_voxels=SC.CAPACITY, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    f.initialize()
    f._est.dense_integrate(np.array(world), I34, 0)
    return f, scan, cands, truth


def test_localize_many_on_the_ranking_fixture(fmx_mod):
    f, scan, cands, truth = _form(fmx_mod)
    ranking = f.dense_relocalize(scan, SC.RADIUS, cands, top=1, sigma=0.1, max_iters=10, threshold=1e-9)["ranking"]
    first = cands[ranking[:3]]
    got = f.dense_localize_many(scan, SC.RADIUS, first, sigma=0.1, max_iters=10, threshold=1e-9)
    assert got["pose"].shape == (3, 3, 4) and got["converged"][0] and not got["singular"][0]
    checked = 0
    for k in range(3):
        if not got["converged"][k]:
            continue
        fit = f.dense_fitness(scan, SC.RADIUS, pose=got["pose"][k])
        assert (int(got["n_valid"][k]), int(got["n_found"][k]), float(got["fitness"][k])) == \
            (fit["n_valid"], fit["n_found"], fit["fitness"]), k
        assert math.isclose(float(got["rmse"][k]), fit["rmse"], rel_tol=1e-9, abs_tol=0.0), k
        checked += 1
    assert checked >= 1 and got["n_found"][0] == len(scan) and np.abs(got["pose"][0] - cands[truth]).max() < 1e-5
    # one guess alone: the same figures, byte for byte
    one = f.dense_localize_many(scan, SC.RADIUS, first[1:2], sigma=0.1, max_iters=10, threshold=1e-9)
    assert all(one[k].tobytes() == got[k][1:2].tobytes() for k in got), [k for k in got if one[k].tobytes() != got[k][1:2].tobytes()]
    # a guess with nothing in reach is reported, not raised
    lost = first[0].copy()
    lost[:, 3] += 1000.0
    mixed = f.dense_localize_many(scan, SC.RADIUS, [first[0], lost], sigma=0.1, max_iters=10, threshold=1e-9)
    assert mixed["singular"].tolist() == [False, True] and mixed["pose"][1].tobytes() == lost.tobytes()
    assert mixed["n_found"][1] == 0 and mixed["rmse"][1] == 0.0 and mixed["fitness"][1] == 0.0
    assert all(mixed[k][0:1].tobytes() == got[k][0:1].tobytes() for k in got)


def test_relocalize_batched_picks_what_the_sequential_path_picks(fmx_mod):
    f, scan, cands, truth = _form(fmx_mod)
    L = fmx_mod.lib()
    before = np.full(12, 3.0)
    st_before = L.fmx_current_pose(f._est.h, fmx_mod._p(before))
    kw = dict(top=3, sigma=0.1, max_iters=10, threshold=1e-9)
    seq = f.dense_relocalize(scan, SC.RADIUS, cands, **kw)
    bat = f.dense_relocalize(scan, SC.RADIUS, cands, batched=True, **kw)
    assert bat["candidate"] == seq["candidate"] == truth and list(bat["ranking"]) == list(seq["ranking"])
    assert sorted(bat["scores"]) == sorted(seq["scores"])
    assert all(bat["scores"][k].tobytes() == seq["scores"][k].tobytes() for k in seq["scores"])
    assert sorted(bat) == sorted(seq)
    assert np.abs(bat["pose"] - cands[truth]).max() < 1e-5 and np.abs(bat["pose"] - seq["pose"]).max() < 1e-6
    assert (bat["n_found"], bat["n_valid"], bat["converged"]) == (seq["n_found"], seq["n_valid"], seq["converged"])
    after = np.full(12, 3.0)
    assert L.fmx_current_pose(f._est.h, fmx_mod._p(after)) == st_before and after.tobytes() == before.tobytes()
    # every candidate singular: status 5
    far = cands.copy()
    far[:, :, 3] += 1e4
    with pytest.raises(fmx_mod.FmxError) as e:
        f.dense_relocalize(scan, SC.RADIUS, far, batched=True, **kw)
    assert e.value.status == 5

"""The dense map's surface normals on the device (fmx_normals_build, fmx_normals_stats,
fmx_normals_download; DESIGN.md §Dense map, Normals) against the restatement
(tests/normals_ref.py over tests/nearest_ref.py's map), matched by voxel key.  Support and the
four class counts are compared with equality, normals up to sign with |dot| >= 1 - 1e-6 against
numpy.linalg.eigh of the restated covariance, flatness within normals_ref.flatness_bound."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import carve_ref as CR
import dense_ref as R
import nearest_ref as NR
import normals_ref as MR
from form_amd import synth

pytestmark = pytest.mark.gpu

INVAL, SIZE, STATE = 1, 2, 5
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
INF = math.inf
EPS = float(np.finfo(np.float64).eps)
FIX = dict(reach=1, min_support=5, max_flatness=0.05)
LIM = (1 << 20) - 2  # the largest storable |coordinate|


def _ctx(fmx):
    p = synth.default_params(synth.ScanGeometry(16, 256, 15.0, 0.01, 0.02))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _pair(fmx, w=1.0, cap=2048, carve=None, gate=GATE):
    ctx = _ctx(fmx)
    ctx.dense_configure(True, w, cap, min_norm_squared=gate[0], max_norm_squared=gate[1])
    ref = NR.NearestRef(w, cap, *gate)
    if carve is not None:
        ctx.carve_configure(**carve)
        ref.carve_configure(**carve)
    return ctx, ref


def _integrate(ctx, ref, p, T=I34, idx=0):
    got = ctx.dense_integrate(np.array(p), T, idx)
    assert got == ref.integrate(p, T, idx)
    return got


def _pts(rows):
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return p


@functools.lru_cache(maxsize=None)
def _fixture():
    p = MR.fixture()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _fixture_ref(reach):
    """The restatement of the fixture's build at a reach, computed once and left unchanged."""
    ref = NR.NearestRef(1.0, 2048, *GATE)
    ref.integrate(_fixture(), I34, 0)
    return ref, MR.build(ref, **dict(FIX, reach=reach))


def _cube_cells(built, reach):
    """The storable cells of the cubes of the voxels that walk them: the build's `lookups`
    exactly (there is no early stop)."""
    total = 0
    for key, v in built.items():
        if v["cls"] == "filtered":
            continue
        n = 1
        for c in MR.cell_of(key):
            n *= min(c + reach, LIM) - max(c - reach, -LIM) + 1
        total += n
    return total


def _sorted(d, w=1.0):
    key = R.key_of_points(d["points"], w)
    o = np.argsort(key, kind="stable")
    return {k: np.asarray(v)[o] for k, v in dict(d, key=key).items()}


def _hold(ctx, built, counts, reach, w=1.0):
    """The device's counts and its full download against the restatement's records; returns the
    largest flatness deviation relative to its bound and the smallest |dot|."""
    want = MR.counts_of(built)
    look = counts.pop("lookups")
    assert counts == want, (counts, want)
    assert look == _cube_cells(built, reach)
    st = ctx.normals_stats()
    assert st == dict(built=True, current=True, voxels=len(built), oriented=want["oriented"])
    d = _sorted(ctx.normals_download(oriented_only=False, misses=True), w)
    solid = sorted(k for k, v in built.items() if v["cls"] != "filtered")
    assert d["key"].tolist() == solid
    worst, low = 0.0, 1.0
    for i, key in enumerate(solid):
        v = built[key]
        assert d["support"][i] == v["support"] and np.array_equal(d["points"][i], v["point"]), key
        n = d["normals"][i].astype(np.float64)
        if v["cls"] == "oriented":
            low = min(low, abs(float(n @ v["normal"])))
            assert abs(np.linalg.norm(n) - 1.0) < 1e-6 and n[np.argmax(np.abs(n))] > 0.0  # the sign rule
            assert float(n @ v["normal"]) > 0.0  # ... which the restatement applies too
        else:
            assert not n.any(), (key, v["cls"], n)
        l0, l1, l2 = v["lams"]
        if l1 > 64.0 * EPS * l2:
            dev = abs(float(d["flatness"][i]) - v["flatness"])
            worst = max(worst, dev / MR.flatness_bound(v["flatness"], v["lams"]))
        elif l2 == 0.0:  # one point: the covariance is exactly zero on both sides
            assert d["flatness"][i] == np.float32(INF)
        # (otherwise l1 is within the eigenvalues' backward error, 64 eps l2, of zero: a line of
        # points.  Its sign, and with it a flatness of 0 / l1 or +inf, is rounding on either side)
    assert low >= 1.0 - 1e-6, low
    assert worst <= 1.0, worst
    only = _sorted(ctx.normals_download(oriented_only=True), w)
    assert only["key"].tolist() == [k for k in solid if built[k]["cls"] == "oriented"]
    assert all(np.asarray(v).tobytes() == np.asarray(d[f])[d["normals"].any(axis=1)].tobytes() for f, v in only.items()
               if f != "misses")
    return worst, low


# ------------------------------------------------------------------ 1. the build
@pytest.mark.parametrize("reach", [1, 2])
def test_build_equals_the_restatement_on_the_fixture(fmx_mod, reach):
    """Largest deviations the device showed on the MI355X (the test prints them): the flatness
    0.239 of its bound at reach 1 and 0.235 at reach 2 (the fp32 storage rounding: the bound's
    2^-22 is four times that), 1 - the smallest |dot| 2.96e-8 and 2.97e-8 (the fp32 rounding of
    the stored normal)."""
    ref, built = _fixture_ref(reach)
    ctx, dref = _pair(fmx_mod)
    _integrate(ctx, dref, _fixture())
    kw = dict(FIX, reach=reach)
    cnt = ctx.normals_build(**kw)
    worst, low = _hold(ctx, built, dict(cnt), reach)
    print(f"normals reach {reach}: counts {cnt}, flatness deviation / bound {worst:.3g}, 1 - min|dot| {1.0 - low:.3g}")
    # two builds store the same bits
    first = _sorted(ctx.normals_download(oriented_only=False))
    assert ctx.normals_build(**kw) == cnt
    again = _sorted(ctx.normals_download(oriented_only=False))
    assert all(first[f].tobytes() == again[f].tobytes() for f in first)
    # min_support below 3 reads as 3
    assert ctx.normals_build(**dict(kw, min_support=0)) == ctx.normals_build(**dict(kw, min_support=3))


def test_max_dist2_excludes_cube_corners(fmx_mod):
    ref, whole = _fixture_ref(1)
    ctx, dref = _pair(fmx_mod)
    _integrate(ctx, dref, _fixture())
    for md in (1.25, 0.0):
        built = MR.build(ref, **FIX, max_dist=md)
        cnt = ctx.normals_build(**FIX, max_dist=md)
        _hold(ctx, built, dict(cnt), 1)
        fewer = sum(built[k]["support"] < whole[k]["support"] for k in built)
        assert fewer > 300 and all(built[k]["support"] <= whole[k]["support"] for k in built)
    assert cnt["sparse"] == 448  # max_dist2 = 0: every voxel admits itself alone


def test_filter_is_applied_to_voxel_and_neighbours(fmx_mod):
    """Part of a patch is integrated twice; with min_hits = 2 its once-hit neighbours neither get
    a normal nor count as support."""
    p = _fixture()
    ctx, ref = _pair(fmx_mod, carve=dict(margin=0))
    _integrate(ctx, ref, p)
    _integrate(ctx, ref, p[:100], I34, 1)
    built = MR.build(ref, **FIX, min_hits=2)
    cnt = ctx.normals_build(**FIX, min_hits=2)
    assert cnt["filtered"] == 348 and cnt["oriented"] > 20
    _hold(ctx, built, dict(cnt), 1)
    one = MR.build(ref, **FIX)
    assert any(0 < built[k]["support"] < one[k]["support"] for k in built)
    # ... and by misses: two rays through the first voxel of the patch
    key = int(R.key_of_points(p[:1, :3].astype(np.float64), 1.0)[0])
    c = MR.cell_of(key)
    T = CR.special_pose((c[0] + 0.5, c[1] + 0.5 - 3.0, c[2] + 0.5))
    through = _pts([(0.0, 6.0, 0.0), (0.0, 6.25, 0.0)])
    assert ctx.carve_rays(through, T) == ref.carve_rays(through, T)
    assert ref.misses.get(key, 0) >= 1
    assert not ctx.normals_stats()["current"]  # the carve ended the snapshot
    built = MR.build(ref, **FIX, max_miss_ratio=0.25)
    assert built[key]["cls"] == "filtered"
    cnt = ctx.normals_build(**FIX, max_miss_ratio=0.25)
    _hold(ctx, built, dict(cnt), 1)


def test_cells_past_the_coordinate_limit_are_skipped(fmx_mod):
    g = np.random.default_rng(53)
    rows = [(LIM - i + 0.5, LIM - j + 0.5, 0.5 + g.uniform(-0.1, 0.1)) for i in range(6) for j in range(6)]
    rows += [(-(LIM - i) + 0.5, 0.5, -(LIM - j) + 0.5) for i in range(4) for j in range(4)]
    p = _pts(rows)
    ctx, ref = _pair(fmx_mod, gate=(1e-12, 1e13))  # (the points are 1.5e6 from the origin)
    assert _integrate(ctx, ref, p) == dict(added=52, merged=0, gated=0, out_of_range=0, invalid=0)
    for reach in (1, 2):
        built = MR.build(ref, **dict(FIX, reach=reach))
        cnt = ctx.normals_build(**dict(FIX, reach=reach))
        assert cnt["lookups"] < 52 * (2 * reach + 1) ** 3
        _hold(ctx, built, dict(cnt), reach)
    assert cnt["oriented"] > 20


@pytest.mark.parametrize("cap", [1, 40, 1 << 19])
def test_table_sizes(fmx_mod, cap):
    """Two slots with one voxel; a small table; and more slots (2^20) than one pass of the build's
    capped grid (2048 blocks of 256 lanes) holding the fixture's few hundred voxels."""
    p = _fixture()[:cap] if cap < 448 else _fixture()
    ctx, ref = _pair(fmx_mod, cap=cap)
    _integrate(ctx, ref, p)
    assert ctx.dense_stats()["slots"] == R.slots_for(cap) and (cap < 1 << 19 or R.slots_for(cap) > 2048 * 256)
    built = MR.build(ref, **FIX)
    cnt = ctx.normals_build(**FIX)
    _hold(ctx, built, dict(cnt), 1)
    if cap == 1:
        assert cnt == dict(oriented=0, flat_rejected=0, sparse=1, filtered=0, lookups=27)
    if cap == 1 << 19:
        assert {k: cnt[k] for k in MR.CLASSES} == MR.counts_of(_fixture_ref(1)[1])


def test_an_empty_map_gives_zero_counts_and_launches_nothing(fmx_mod):
    ctx, _ = _pair(fmx_mod)
    ctx.profile(True)
    assert ctx.normals_stats() == dict(built=False, current=False, voxels=0, oriented=0)
    base = ctx.profile_read()["dense"]["launches"]
    assert ctx.normals_build(**FIX) == dict(oriented=0, flat_rejected=0, sparse=0, filtered=0, lookups=0)
    assert ctx.normals_stats() == dict(built=True, current=True, voxels=0, oriented=0)
    assert len(ctx.normals_download(False)["hits"]) == 0
    assert ctx.profile_read()["dense"]["launches"] == base
    ctx.dense_integrate(np.array(_fixture()), I34, 0)
    base = ctx.profile_read()["dense"]["launches"]
    ctx.normals_build(**FIX)
    assert ctx.profile_read()["dense"]["launches"] == base + 1  # one launch per build
    ctx.normals_download(True)
    assert ctx.profile_read()["dense"]["launches"] == base + 2  # ... and one per download (the sizing call: none)


# ------------------------------------------------------------------ 2. staleness
def _raw_download(fmx, ctx, cap, oriented_only=1):
    A, out = ctx._voxel_arrays(max(cap, 1), False)
    nrm = np.full((max(cap, 1), 3), 9.0, np.float32)
    n = C.c_uint32(cap)
    st = fmx.lib().fmx_normals_download(ctx.h, C.c_int(oriented_only), C.byref(A), fmx._p(nrm), None, None, C.byref(n))
    return st, n.value, nrm, out


def test_staleness(fmx_mod):
    fmx = fmx_mod
    ctx, ref = _pair(fmx, carve=dict(margin=0))
    _integrate(ctx, ref, _fixture())
    assert _raw_download(fmx, ctx, 448)[0] == STATE  # never built
    never = ctx.normals_stats()
    assert never == dict(built=False, current=False, voxels=0, oriented=0)

    def current():
        cnt = ctx.normals_build(**FIX)
        st = ctx.normals_stats()
        assert st["current"] and st["built"] and st["voxels"] == ctx.dense_stats()["voxels"] and st["oriented"] == cnt["oriented"]
        assert _raw_download(fmx, ctx, 2048)[:2] == (0, cnt["oriented"])
        return cnt

    def stale():
        st = ctx.normals_stats()
        assert st["built"] and not st["current"]
        code, n, nrm, _ = _raw_download(fmx, ctx, 2048)
        assert code == STATE and n == 2048 and (nrm == 9.0).all()
        with pytest.raises(fmx.FmxError) as e:
            ctx.normals_download()
        assert e.value.status == STATE

    first = current()
    ctx.dense_integrate(_pts([(40.5, 40.5, 40.5)]), I34, 1)  # an integration that adds a voxel
    stale()
    assert current()["sparse"] == first["sparse"] + 1
    held = ctx.roll_evict((6.0, 6.0, 6.0), (8, 8, 8))  # a roll that evicts the far voxels
    assert len(held["hits"]) == 17
    stale()
    assert current()["sparse"] == first["sparse"] - 16
    ctx.dense_upload(held["points"], held["scan"], held["index"], held["hits"])  # an upload
    stale()
    assert current()["sparse"] == first["sparse"] + 1
    T = CR.special_pose((0.5, -1.5, 1.5))
    got = ctx.carve_rays(_pts([(0.0, 6.0, 0.0)]), T)  # a ray along a patch: it counts a miss
    assert got["misses"] >= 1
    stale()
    current()
    ctx.dense_clear()
    stale()
    assert current() == dict(oriented=0, flat_rejected=0, sparse=0, filtered=0, lookups=0)
    # calls that only read leave it current
    ctx.dense_integrate(np.array(_fixture()), I34, 0)
    cnt = current()
    ctx.dense_download()
    ctx.nearest_voxels(_fixture(), I34)
    ctx.roll_evict((6.0, 6.0, 6.0), (1 << 20, 1 << 20, 1 << 20))  # evicts nothing
    assert ctx.normals_stats()["current"] and _raw_download(fmx, ctx, 2048)[:2] == (0, cnt["oriented"])


def test_status_codes_and_the_two_call_protocol(fmx_mod):
    fmx = fmx_mod
    ctx = _ctx(fmx)
    with pytest.raises(fmx.FmxError) as e:
        ctx.normals_build(**FIX)  # before fmx_dense_configure
    assert e.value.status == STATE
    assert ctx.normals_stats() == dict(built=False, current=False, voxels=0, oriented=0)  # FMX_OK on any context
    ctx.dense_configure(True, 1.0, 2048, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    ctx.dense_integrate(np.array(_fixture()), I34, 0)
    L = fmx.lib()

    def raw(reach=1, max_dist2=INF, min_support=5, max_flatness=0.05, null=False):
        prm, cnt = fmx._NormalsParams(1, 0, 0, reach, max_dist2, min_support, max_flatness), fmx._NormalsCounts()
        return L.fmx_normals_build(ctx.h, None if null else C.byref(prm), C.byref(cnt))

    bad = [dict(reach=0), dict(reach=9), dict(null=True)] + [dict(max_dist2=v) for v in (math.nan, -1.0, -INF)] + \
          [dict(max_flatness=v) for v in (math.nan, -0.1, 1.5, INF)]
    for kw in bad:
        assert raw(**kw) == INVAL, kw
    assert not ctx.normals_stats()["built"]
    assert raw(reach=8, max_flatness=1.0) == 0 and raw(max_flatness=0.0, max_dist2=0.0) == 0
    assert L.fmx_normals_build(ctx.h, C.byref(fmx._NormalsParams(1, 0, 0, 1, INF, 5, 0.05)), None) == 0  # NULL counts
    cnt = ctx.normals_build(**FIX)
    assert raw(reach=0) == INVAL and ctx.normals_stats()["current"]  # a refused build leaves the snapshot alone
    # the sizing call, a capacity that is too small (nothing written), an exact one
    n = C.c_uint32(0)
    assert L.fmx_normals_download(ctx.h, C.c_int(0), None, None, None, None, C.byref(n)) == 0 and n.value == 448
    assert L.fmx_normals_download(ctx.h, C.c_int(1), None, None, None, None, None) == INVAL
    code, m, nrm, out = _raw_download(fmx, ctx, cnt["oriented"] - 1)
    assert code == SIZE and m == cnt["oriented"] - 1 and (nrm == 9.0).all() and not out["hits"].any()
    code, m, nrm, out = _raw_download(fmx, ctx, cnt["oriented"])
    assert code == 0 and m == cnt["oriented"] and (np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-6).all()
    # fmx_dense_configure drops the arrays with the map
    off = _ctx(fmx)
    off.dense_configure(True, 1.0, 64)
    off.normals_build(**FIX)
    assert off.normals_stats()["built"]
    off.dense_configure(False, 1.0, 64)
    assert off.normals_stats() == dict(built=False, current=False, voxels=0, oriented=0)
    with pytest.raises(fmx.FmxError) as e:
        off.normals_download()
    assert e.value.status == STATE


# ------------------------------------------------------------------ 3. read only
def _snapshot(ctx, w):
    return (CR.sort_download(ctx.dense_download(misses=True), w), ctx.dense_stats(), ctx.dense_last(), ctx.carve_last())


def test_build_and_download_change_nothing(fmx_mod):
    ctx, ref = _pair(fmx_mod, carve=dict(margin=1))
    _integrate(ctx, ref, _fixture())
    _integrate(ctx, ref, _fixture()[:50], I34, 1)
    before = _snapshot(ctx, 1.0)
    ctx.normals_build(**FIX)
    ctx.normals_download(False, misses=True)
    ctx.normals_build(**dict(FIX, reach=2, min_hits=2))
    ctx.normals_download(True)
    after = _snapshot(ctx, 1.0)
    assert CR.same(before[0], after[0]) is None and before[1:] == after[1:]


# ------------------------------------------------------------------ 4. FORM.dense_normals
def test_form_dense_normals_faces_the_viewpoint(fmx_mod):
    import types
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    f = fmx_mod.FORM()
    f.set_lidar_params(lidar)
    f.set_dense_map(True, voxel_width=0.5, max_voxels=1 << 15)
    f.initialize()
    f.add_lidar(synth.make_scan_skewed("tiny", 0, world=synth.World())[0].numpy()[:, :3])
    plain = f.dense_normals()
    n = len(plain["hits"])
    assert n > 20 and plain["normals"].shape == (n, 3) and (plain["support"] >= 5).all()
    assert (plain["normals"][np.arange(n), np.argmax(np.abs(plain["normals"]), axis=1)] > 0).all()
    eye = np.array(f.pose()[:3, 3])
    seen = f.dense_normals(viewpoint=eye)
    a, b = _sorted(plain, 0.5), _sorted(seen, 0.5)
    assert np.array_equal(a["key"], b["key"]) and np.array_equal(np.abs(a["normals"]), np.abs(b["normals"]))
    assert (np.einsum("ij,ij->i", eye - b["points"], b["normals"].astype(np.float64)) >= 0.0).all()
    assert (a["normals"] != b["normals"]).any()
    wide = f.dense_normals(reach_m=1.0)
    assert f._est.normals_stats()["current"] and len(wide["hits"]) > 0
    with pytest.raises(ValueError):
        f.dense_normals(reach_m=4.5)  # reach 9

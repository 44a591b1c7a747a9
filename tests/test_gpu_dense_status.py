"""What the dense map's entry points answer to a call they refuse or have nothing to do for
(include/fmx/fmx.h, the fmx_dense_* ... fmx_align_* blocks): the status, the exact text of
fmx_last_error and which complaint wins when two apply; empty calls; the per-call tag buffers;
a host scan against the same scan on the device; the voxel lists of a map that never carved.
The per-feature suites check what the kernels compute; this one pins the argument handling and
the copy bookkeeping around them, on a 64-voxel map and clouds of four points.

The expected texts are literals.  Two things an empty call does are results, not writes to a
per-point array, and are pinned as such: an empty fmx_dense_integrate is still an integration
(it draws an owner number, so `integrations` rises by one and nothing else of fmx_dense_stats
moves), and an empty fmx_align_system returns the all-zero system in `out`."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from form_amd import synth

pytestmark = pytest.mark.gpu

OK, INVAL, SIZE, OOM, STATE, RANGE = 0, 1, 2, 3, 5, 6
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
FILL = 0xA5
NOT_ENABLED = "the dense map is not enabled (fmx_dense_configure)"
NO_CARVING = "carving has not been enabled on this map (fmx_carve_configure)"
SIX = ("dense_integrate", "carve_rays", "probe_points", "probe_rays", "nearest_voxels", "align_system")
# one point in each of four voxels (width 1.0), and a query cloud: three of them and an empty place
CLOUD = np.array([[0.5, 0.5, 0.5, 0], [2.5, 0.5, 0.5, 0], [0.5, 3.5, 0.5, 0], [5.5, 5.5, 1.5, 0]], np.float32)
QUERY = np.array([[0.5, 3.5, 0.5, 0], [9.5, 9.5, 9.5, 0], [0.5, 0.5, 0.5, 0], [2.5, 0.5, 0.5, 0]], np.float32)
FAR = (np.array([100.5, 100.5, 100.5]), np.zeros(3, np.uint32))  # a box that holds none of CLOUD


def _ctx(fmx):
    p = synth.default_params(synth.ScanGeometry(16, 256, 15.0, 0.01, 0.02))
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p)))


def _map(fmx, carve=False, cloud=True):
    ctx = _ctx(fmx)
    ctx.dense_configure(True, 1.0, 64, min_norm_squared=GATE[0], max_norm_squared=GATE[1])
    if carve:
        ctx.carve_configure(True)
    if cloud:
        assert ctx.dense_integrate(CLOUD, I34, 7)["added"] == 4
    return ctx


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bufs(fmx, room=4):
    """Caller arrays for `room` points, every byte a sentinel, and the fmx_voxel_arrays over them."""
    b = dict(state=np.full(room, FILL, np.uint8), step=np.full(room, FILL, np.uint32), t=np.full(room, float(FILL)),
             dist2=np.full(room, float(FILL)), points=np.full((room, 3), float(FILL)),
             scan=np.full(room, FILL, np.uint64), index=np.full(room, FILL, np.uint32),
             hits=np.full(room, FILL, np.uint32), misses=np.full(room, FILL, np.uint32))
    A = fmx._VoxelArrays()
    A.xyz, A.scan, A.index, A.hits, A.misses = (b[k].ctypes.data for k in ("points", "scan", "index", "hits", "misses"))
    return b, A


def _untouched(b):
    return all((v == FILL).all() for v in b.values())


def _call(fmx, ctx, name, pts, n, pose, b=None, A=None, out=None, prm=True, state=True):
    """One of SIX through the C entry point itself: pts and pose are arrays or None (NULL).
    Returns (status, fmx_last_error's text, the counts as a dict)."""
    L, h = ctx._L, ctx.h
    if b is None:
        b, A = _bufs(fmx)
    head = (h, _ptr(pts), C.c_size_t(n), C.c_int(0), _ptr(pose))
    flt = (C.c_uint32(1), C.c_uint32(0), C.c_uint32(0))
    st_p = _ptr(b["state"]) if state else None
    if name == "dense_integrate":
        cnt = fmx._DenseCounts()
        st = L.fmx_dense_integrate(*head, C.c_uint64(9), C.byref(cnt))
    elif name == "carve_rays":
        cnt = fmx._CarveCounts()
        st = L.fmx_carve_rays(*head, C.byref(cnt))
    elif name == "probe_points":
        cnt = fmx._ProbePointCounts()
        st = L.fmx_probe_points(*head, *flt, st_p, C.byref(A), C.byref(cnt))
    elif name == "probe_rays":
        cnt = fmx._ProbeRayCounts()
        st = L.fmx_probe_rays(*head, *flt, C.c_uint32(0), st_p, _ptr(b["step"]), _ptr(b["t"]), C.byref(A), C.byref(cnt))
    elif name == "nearest_voxels":
        cnt = fmx._NearestCounts()
        st = L.fmx_nearest_voxels(*head, *flt, C.c_uint32(1), C.c_double(math.inf), st_p, _ptr(b["dist2"]),
                                  C.byref(A), C.byref(cnt))
    else:
        assert name == "align_system"
        cnt = fmx._AlignCounts()
        p = fmx._AlignParams(1, 0, 0, 1, math.inf, 1.0, 1)
        st = L.fmx_align_system(*head, C.byref(p) if prm else None, _ptr(out), C.byref(cnt))
    return st, L.fmx_last_error(h).decode(), cnt.as_dict()


def _err(fmx, fn):
    with pytest.raises(fmx.FmxError) as e:
        fn()
    return e.value.status, str(e.value).split(": ", 1)[1]


def _pose_with(k, v):
    T = I34.copy()
    T.reshape(12)[k] = v
    return T


# ------------------------------------------------------------------ 1. the map is off
def test_disabled_map_one_text(fmx_mod):
    fmx = fmx_mod
    never = _ctx(fmx)
    off = _ctx(fmx)
    off.dense_configure(True, 1.0, 64)
    off.dense_configure(False, 1.0, 64)
    sys29 = np.zeros(29)
    for ctx in (never, off):
        for name in SIX:
            assert _call(fmx, ctx, name, CLOUD, 4, I34.copy(), out=sys29)[:2] == (STATE, NOT_ENABLED), name
            # the map comes first: before a null pose, null points, a null output, null params
            assert _call(fmx, ctx, name, None, 2, None, out=None, prm=False)[:2] == (STATE, NOT_ENABLED), name
        wrappers = dict(
            dense_download=lambda: ctx.dense_download(), carve_download=lambda: ctx.dense_download(misses=True),
            dense_clear=lambda: ctx.dense_clear(), roll_configure=lambda: ctx.roll_configure(True, (1, 1, 1), 1.0),
            roll_count=lambda: ctx.roll_count(*FAR), carve_evict=lambda: ctx.roll_evict(*FAR, discard=True),
            carve_drain=lambda: ctx.roll_drain(), carve_configure=lambda: ctx.carve_configure(True),
            align_dense=lambda: ctx.dense_align(CLOUD, I34), upload_voxels=lambda: ctx.dense_upload(CLOUD[:, :3]))
        for name, fn in wrappers.items():
            assert _err(fmx, fn) == (STATE, NOT_ENABLED), name
        # the entry points without the struct, and the null arguments the map check comes before
        L, h, n = ctx._L, ctx.h, C.c_uint32(0)
        assert L.fmx_dense_download(h, C.c_uint32(1), None, None, None, None, C.byref(n)) == STATE
        assert L.fmx_last_error(h).decode() == NOT_ENABLED
        assert L.fmx_roll_evict(h, _ptr(FAR[0]), _ptr(FAR[1]), None, None, None, None, C.byref(n)) == STATE
        assert L.fmx_last_error(h).decode() == NOT_ENABLED
        assert L.fmx_roll_drain(h, None, None, None, None, C.byref(n)) == STATE
        assert L.fmx_last_error(h).decode() == NOT_ENABLED
        for st in (L.fmx_carve_download(h, C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), None, None),
                   L.fmx_carve_evict(h, None, None, None, None), L.fmx_carve_drain(h, None, None),
                   L.fmx_roll_count(h, None, None, None), L.fmx_carve_configure(h, None),
                   L.fmx_align_dense(h, None, C.c_size_t(2), C.c_int(0), None, None, C.c_uint32(1), C.c_double(-1.0),
                                     None, None)):
            assert st == STATE and L.fmx_last_error(h).decode() == NOT_ENABLED
        assert ctx.dense_stats() == dict(voxels=0, max_voxels=0, integrations=0, slots=0)


def test_carve_rays_needs_carving(fmx_mod):
    ctx = _map(fmx_mod)
    assert _call(fmx_mod, ctx, "carve_rays", CLOUD, 4, I34.copy())[:2] == (STATE, NO_CARVING)
    assert _call(fmx_mod, ctx, "carve_rays", None, 2, None)[:2] == (STATE, NO_CARVING)  # before the arguments


# ------------------------------------------------------------------ 2. rejected inputs
def test_rejected_inputs_texts_and_precedence(fmx_mod):
    fmx = fmx_mod
    ctx = _map(fmx, carve=True)
    stats = ctx.dense_stats()
    sys29 = np.full(29, float(FILL))
    for name in SIX:
        b, A = _bufs(fmx)
        call = lambda pts, n, pose: _call(fmx, ctx, name, pts, n, pose, b, A, out=sys29)[:2]
        assert call(CLOUD, 4, None) == (INVAL, "null pose"), name
        for k, bad in ((0, math.nan), (3, math.nan), (11, math.inf)):
            assert call(CLOUD, 4, _pose_with(k, bad)) == (INVAL, "non-finite pose"), (name, k)
        assert call(None, 2, I34.copy()) == (INVAL, "null points"), name
        assert call(None, 2, None) == (INVAL, "null pose"), name  # two faults: the pose's text wins
        assert call(None, 2, _pose_with(5, math.nan)) == (INVAL, "non-finite pose"), name
        assert _untouched(b) and (sys29 == FILL).all(), name
    # the calls' own complaints, in their places
    big = np.zeros((61, 4), np.float32)
    assert _call(fmx, ctx, "dense_integrate", big, 61, I34.copy())[:2] == (
        OOM, "dense map: 4 voxels + 61 points exceed max_voxels 64")
    assert _call(fmx, ctx, "dense_integrate", None, 61, I34.copy())[:2] == (INVAL, "null points")
    away = _pose_with(3, 2.0e6)
    assert _call(fmx, ctx, "probe_rays", CLOUD, 4, away)[:2] == (RANGE, "probe: the voxel of the ray origin is out of range")
    assert _call(fmx, ctx, "probe_rays", None, 2, away)[:2] == (INVAL, "null points")
    assert _call(fmx, ctx, "align_system", None, 2, None, out=None)[:2] == (INVAL, "null output")
    assert _call(fmx, ctx, "align_system", None, 2, None, out=sys29, prm=False)[:2] == (INVAL, "null params")
    L, h = ctx._L, ctx.h
    prm = fmx._AlignParams(1, 0, 0, 1, math.inf, 1.0, 1)
    T = np.zeros(12)
    assert L.fmx_align_dense(h, None, C.c_size_t(2), C.c_int(0), None, C.byref(prm), C.c_uint32(1), C.c_double(1e-6),
                             None, None) == INVAL and L.fmx_last_error(h).decode() == "null pose_out"
    assert L.fmx_align_dense(h, None, C.c_size_t(2), C.c_int(0), None, C.byref(prm), C.c_uint32(1), C.c_double(1e-6),
                             _ptr(T), None) == INVAL and L.fmx_last_error(h).decode() == "null pose"
    assert L.fmx_align_dense(h, None, C.c_size_t(2), C.c_int(0), _ptr(I34.copy()), C.byref(prm), C.c_uint32(1),
                             C.c_double(1e-6), _ptr(T), None) == INVAL and L.fmx_last_error(h).decode() == "null points"
    assert ctx.dense_stats() == stats  # none of it changed the map
    assert ctx.probe_points(CLOUD, I34)["counts"]["solid"] == 4


# ------------------------------------------------------------------ 3. empty calls
def test_empty_calls(fmx_mod):
    fmx = fmx_mod
    ctx = _map(fmx, carve=True)
    for name in SIX:
        stats = ctx.dense_stats()
        b, A = _bufs(fmx)
        sys29 = np.full(29, float(FILL))
        st, text, cnt = _call(fmx, ctx, name, CLOUD, 0, I34.copy(), b, A, out=sys29)
        assert (st, text) == (OK, "") and all(v == 0 for v in cnt.values()), (name, st, text, cnt)
        assert _untouched(b), name
        if name == "align_system":
            assert (sys29 == 0.0).all()  # the system of no points: a result, like the counts
        if name == "dense_integrate":
            stats["integrations"] += 1  # an integration that counts nothing is still one
        assert ctx.dense_stats() == stats, name
        # no points to read: a null pointer is as good
        assert _call(fmx, ctx, name, None, 0, I34.copy(), b, A, out=sys29)[:2] == (OK, ""), name
        assert _untouched(b), name
    assert ctx.dense_stats()["voxels"] == 4


# ------------------------------------------------------------------ 4. the call's own tag and state buffers
@pytest.mark.parametrize("name", ["probe_points", "nearest_voxels"])
def test_tags_without_a_state_array(fmx_mod, name):
    fmx = fmx_mod
    ctx = _map(fmx)
    got = {}
    for with_state in (True, False):
        b, _ = _bufs(fmx)
        A = fmx._VoxelArrays()  # scan and index alone
        A.scan, A.index = b["scan"].ctypes.data, b["index"].ctypes.data
        st, text, cnt = _call(fmx, ctx, name, QUERY, 4, I34.copy(), b, A, state=with_state)
        assert (st, text) == (OK, ""), (st, text)
        assert with_state or (b["state"] == FILL).all()
        assert all((b[k] == FILL).all() for k in ("points", "hits", "misses", "step", "t"))
        got[with_state] = (b["scan"].copy(), b["index"].copy(), cnt)
    assert np.array_equal(got[True][0], got[False][0]) and np.array_equal(got[True][1], got[False][1])
    assert got[True][2] == got[False][2]
    # the voxels of CLOUD's points 2, none, 0, 1, all of integration 7
    assert got[False][0].tolist() == [7, 0, 7, 7] and got[False][1].tolist() == [2, 0, 0, 1]


# ------------------------------------------------------------------ 5. a host scan and the same scan on the device
def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "counts":
            assert a[k] == b[k], k
        else:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_host_source_equals_device_source(fmx_mod):
    ctx = _map(fmx_mod)
    dev = torch.from_numpy(QUERY.copy()).to("cuda:0")
    T = np.eye(3, 4)
    T[:, 3] = (0.25, -0.5, -2.5)  # a second pose: the rays start below the map
    for call in (ctx.probe_points, ctx.probe_rays, ctx.nearest_voxels):
        _same(call(QUERY.copy(), T), call(dev, T))
    points = ctx.probe_points(QUERY.copy(), I34), ctx.probe_points(dev, I34)
    _same(*points)
    assert points[0]["counts"] == dict(absent=1, filtered=0, solid=3, out_of_range=0, invalid=0)
    rays = ctx.probe_rays(QUERY.copy(), I34), ctx.probe_rays(dev, I34)
    _same(*rays)
    assert rays[0]["counts"]["hit"] >= 3 and rays[0]["counts"]["steps"] > 0
    near = ctx.nearest_voxels(QUERY.copy(), I34, reach=1), ctx.nearest_voxels(dev, I34, reach=1)
    _same(*near)
    assert near[0]["counts"]["found"] == 3 and near[0]["counts"]["none"] == 1


# ------------------------------------------------------------------ 6. the voxel lists of a map that never carved
def _list(fmx, fn, room, only=None, n_in=None):
    """fn(arrays, n) with caller arrays of `room` entries (only: that one array, the rest NULL)."""
    b, A = _bufs(fmx, room)
    if only is not None:
        A = fmx._VoxelArrays()
        setattr(A, only, b[only].ctypes.data)
    n = C.c_uint32(room if n_in is None else n_in)
    st = fn(C.byref(A), C.byref(n))
    return st, int(n.value), b


def _is_cloud(b, n):
    """The four voxels of CLOUD as integration 7 left them, in any order; misses zero."""
    o = np.argsort(b["index"][:4])
    assert n == 4 and b["index"][o].tolist() == [0, 1, 2, 3] and (b["scan"] == 7).all() and (b["hits"] == 1).all()
    assert np.array_equal(b["points"][o], CLOUD[:, :3].astype(np.float64))
    assert (b["misses"] == 0).all()
    assert all((b[k] == FILL).all() for k in ("state", "step", "t", "dist2"))


def test_voxel_lists_without_carving(fmx_mod):
    fmx = fmx_mod
    ctx = _map(fmx)
    L, h = ctx._L, ctx.h
    err = lambda: L.fmx_last_error(h).decode()
    down = lambda A, n: L.fmx_carve_download(h, C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), A, n)
    evict = lambda A, n: L.fmx_carve_evict(h, _ptr(FAR[0]), _ptr(FAR[1]), A, n)
    # download: sizing (all arrays null: no room needed), one short, scan alone, all five
    n = C.c_uint32(0)
    assert down(None, C.byref(n)) == OK and n.value == 4
    n = C.c_uint32(0)
    assert down(C.byref(fmx._VoxelArrays()), C.byref(n)) == OK and n.value == 4
    st, m, b = _list(fmx, down, 4, n_in=3)
    assert (st, err(), m) == (SIZE, "dense map download: room for 3 of 4 voxels", 3) and _untouched(b)
    st, m, b = _list(fmx, down, 4, only="scan")
    assert (st, m) == (OK, 4) and (b.pop("scan") == 7).all() and _untouched(b)
    st, m, b = _list(fmx, down, 4)
    assert st == OK
    _is_cloud(b, m)
    # evict, every voxel outside the box: one short (nothing leaves), scan alone, all five, discard
    st, m, b = _list(fmx, evict, 4, n_in=3)
    assert (st, err(), m) == (SIZE, "dense map roll: room for 3 of 4 evicted voxels", 3) and _untouched(b)
    assert ctx.dense_stats()["voxels"] == 4
    st, m, b = _list(fmx, evict, 4, only="scan")
    assert (st, m) == (OK, 4) and (b.pop("scan") == 7).all() and _untouched(b)
    assert ctx.dense_stats()["voxels"] == 0
    assert ctx.dense_integrate(CLOUD, I34, 7)["added"] == 4
    st, m, b = _list(fmx, evict, 4)
    assert st == OK
    _is_cloud(b, m)
    assert ctx.dense_integrate(CLOUD, I34, 7)["added"] == 4
    n = C.c_uint32(0)
    assert evict(None, C.byref(n)) == OK and n.value == 4 and ctx.dense_stats()["voxels"] == 0
    assert evict(None, None) == OK  # a discard needs no count either
    st, m, b = _list(fmx, evict, 4)  # nothing left to evict: nothing written
    assert (st, m) == (OK, 0) and _untouched(b)
    # the spill of a context that never rolled: the sizing call and a filling call of nothing
    drain = lambda A, n: L.fmx_carve_drain(h, A, n)
    n = C.c_uint32(9)
    assert drain(None, C.byref(n)) == OK and n.value == 0
    st, m, b = _list(fmx, drain, 4, only="scan")
    assert (st, m) == (OK, 0) and _untouched(b)
    assert drain(C.byref(fmx._VoxelArrays()), None) == INVAL and err() == "null count"

"""Carving the dense voxel map on the device (fmx_carve_*; DESIGN.md §Dense map, Carving)
against the restatement (tests/carve_ref.py).  Every comparison with the restatement is
equality on the key-sorted download, misses included, and on the launch's counts: the result
is a sum over a set of (ray, voxel) pairs that the definition fixes."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import carve_ref as CR
import dense_ref as R
from form_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = {"odd": (5, 200), "tiny": (16, 256)}
OOM, STATE, SIZE, INVAL = 3, 5, 2, 1
I34 = np.eye(3, 4)
BOTH = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])


def _geo(name):
    r, c = SHAPES[name]
    return synth.ScanGeometry(r, c, 15.0, 0.01, 0.02)


def _ctx(fmx, geo=None, window=None, **over):
    p = synth.default_params(geo or _geo("tiny"))
    kw = dict(over)
    if window:
        kw.update(max_num_recent_scans=window[0], max_num_keyscans=window[1])
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p), **kw))


def _pair(fmx, w, cap, gate=(1.0, 1e4), geo=None, **carve):
    """A context with the dense map and carving on, and its restatement."""
    ctx = _ctx(fmx, geo)
    ctx.dense_configure(True, w, cap, min_norm_squared=gate[0], max_norm_squared=gate[1])
    ref = CR.CarveRef(w, cap, gate[0], gate[1])
    _both(ctx, ref, **carve)
    return ctx, ref


def _both(ctx, ref, **carve):
    ctx.carve_configure(**carve)
    ref.carve_configure(**carve)


def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def _pose(Rm, t):
    T = np.zeros((3, 4))
    T[:, :3] = Rm
    T[:, 3] = t
    return T


# (tests/test_gpu_dense.py's poses)
POSES = [_pose(_rot("z", 0.3), (-12.5, -3.25, -0.75)), _pose(_rot("x", 0.4) @ _rot("y", -0.7), (2.0, 1.0, 0.5)),
         _pose(_rot("y", 1.1) @ _rot("z", -2.0), (-0.3, 14.0, -2.0))]


@functools.lru_cache(maxsize=None)
def _points(name, k):
    p = synth.raycast(synth.World(), synth.trajectory_pose(k), _geo(name), 4242 + k).numpy()
    p.setflags(write=False)
    return p


def _arg(p, on_device):
    return torch.from_numpy(np.array(p)).to("cuda:0") if on_device else np.array(p)


def _check(ctx, ref, min_hits=1, ratio=None):
    got = CR.sort_download(ctx.dense_download(min_hits, ratio), ref.w)
    want = ref.sorted(min_hits, ratio)
    assert CR.same(got, want) is None, CR.same(got, want)
    return want


def _integrate(ctx, ref, p, T, idx, on_device=False):
    """One integration on both; the dense counts and the carve's agree."""
    got = ctx.dense_integrate(_arg(p, on_device), T, idx)
    assert got == ref.integrate(p, T, idx)
    assert ctx.carve_last() == ref.carve_last, (ctx.carve_last(), ref.carve_last)
    return ref.carve_last[0]


def _status(fmx, fn):
    with pytest.raises(fmx.FmxError) as e:
        fn()
    return e.value.status


# ------------------------------------------------------------------ 1. special rays
def _group(o):
    names = [n for n, oo, _ in CR.SPECIAL if oo == o]
    pts = np.concatenate([CR.special_point(p) for _, oo, p in CR.SPECIAL if oo == o])
    return names, pts


def _special_map(fmx, rays, **carve):
    """A map holding every voxel on the rays' paths and a shell of voxels beside them."""
    ctx, ref = _pair(fmx, 1.0, 4096, CR.SPECIAL_GATE, **carve)
    vox = set()
    for _, o, p in rays:
        for v in CR.walk(o, CR.special_end(o, p), 1.0):
            vox.update({v, (v[0], v[1] + 1, v[2]), (v[0], v[1], v[2] - 1)})
    _integrate(ctx, ref, CR.voxel_centres(sorted(vox), 1.0), I34, 0)
    _check(ctx, ref)
    return ctx, ref


@BOTH
def test_special_rays_each_alone(fmx_mod, on_device):
    ctx, ref = _special_map(fmx_mod, CR.SPECIAL, margin=1)
    for name, o, p in CR.SPECIAL:
        S = len(CR.walk(o, CR.special_end(o, p), 1.0)) - 1
        got = ctx.carve_rays(_arg(CR.special_point(p), on_device), CR.special_pose(o))
        assert got == ref.carve_rays(CR.special_point(p), CR.special_pose(o)), name
        # every path voxel is in the map and nothing is exempt in this call
        assert got == dict(rays=1, steps=max(S - 1, 0), misses=max(S - 1, 0), exempt=0), name
        _check(ctx, ref)
    assert ctx.carve_last() == ref.carve_last  # the stand-alone call is not "the last integration"


@BOTH
def test_special_rays_in_one_launch_margins_gate_and_stride(fmx_mod, on_device):
    names, pts = _group(CR._H)
    assert len(names) == 9
    ctx, ref = _special_map(fmx_mod, CR.SPECIAL, margin=0)
    T = CR.special_pose(CR._H)
    total = {}
    # margin 0: up to the voxel before the return; margin >= every S (the longest is 9): nothing
    for cfg in (dict(margin=0), dict(margin=2), dict(margin=9), dict(margin=1 << 31), dict(margin=1, ray_stride=3),
                dict(margin=1, max_norm_squared=25.0),  # +-x have r2 = 25: just outside (strict)
                dict(margin=1, max_norm_squared=float(np.nextafter(25.0, 26.0)))):  # just inside
        _both(ctx, ref, **cfg)
        got = ctx.carve_rays(_arg(pts, on_device), T)
        assert got == ref.carve_rays(pts, T), cfg
        total[tuple(cfg.items())] = got
        _check(ctx, ref)
    t = list(total.values())
    assert t[0]["rays"] == 9 and t[0]["steps"] == 5 + 5 + 4 + 4 + 6 + 6 + 9 + 9 + 0 == t[0]["misses"]
    assert t[2] == dict(rays=9, steps=0, misses=0, exempt=0) == t[3]
    assert t[4]["rays"] == 3  # indices 0, 3, 6
    assert t[5]["rays"] == 3 and t[6]["rays"] == 5  # {+-y, same-voxel}, and +-x as well


@BOTH
def test_one_long_ray_among_short_ones(fmx_mod, on_device):
    w, o = 0.01, (0.005, 0.005, 0.005)
    ctx, ref = _pair(fmx_mod, w, 4096, (1e-6, 1e4), margin=1)
    T = CR.special_pose(o)
    pts = np.zeros((64, 4), np.float32)
    pts[:, 0] = 0.011 + 0.0001 * np.arange(64)  # S = 1 or 2
    pts[::5, 1] = 0.011
    pts[17, :3] = (20.0, 12.0, 8.0)
    long_path = CR.walk(o, R.classify(pts[17:18], T, w, 1e-6, 1e4)[1][0], w)
    assert len(long_path) == 4001
    _integrate(ctx, ref, CR.voxel_centres(long_path[::40] + long_path[1:3], w), I34, 0)
    got = ctx.carve_rays(_arg(pts, on_device), T)
    assert got == ref.carve_rays(pts, T)
    assert got["rays"] == 64 and 3999 < got["steps"] <= 3999 + 63 * 2 and got["misses"] >= 4000 // 40
    _check(ctx, ref)


@BOTH
def test_origin_out_of_range_casts_nothing(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod, 1.0, 4096, CR.SPECIAL_GATE, margin=0)
    far = CR.special_pose((float(1 << 20), 0.5, 0.5))  # a_x = 2^20: out of range
    near = CR.special_pose((float((1 << 20) - 2) + 0.5, 0.5, 0.5))  # a_x = 2^20 - 2: the last one in range
    pts = np.array([[-5.0, 0, 0, 0], [-6.0, 0, 0, 0], [-7.0, 0, 0, 0]], np.float32)  # their voxels are in range
    c = _integrate(ctx, ref, pts, far, 0, on_device)
    assert c == CR.no_counts() and ctx.carve_last()[1] == 1 and ctx.dense_stats()["voxels"] == 3
    before = _check(ctx, ref)
    assert ctx.carve_rays(_arg(pts, on_device), far) == ref.carve_rays(pts, far) == CR.no_counts()
    assert CR.same(_check(ctx, ref), before) is None and (before["misses"] == 0).all()
    # the same points from an origin in range do carve
    more = np.array([[-2.5, 0, 0, 0]], np.float32)
    got = ctx.carve_rays(_arg(more, on_device), far)
    assert got == ref.carve_rays(more, far) == CR.no_counts()
    shot = np.array([[-20.0, 0, 0, 0]], np.float32)
    got = ctx.carve_rays(_arg(shot, on_device), near)
    assert got == ref.carve_rays(shot, near) and got["rays"] == 1 and got["misses"] == 3
    _check(ctx, ref)


# ------------------------------------------------------------------ 2. lookup
def _lookup_voxels():
    """64 voxels (cx, 0, 0), 1 <= cx < 400, for a table of 128 slots: at least three of them
    home to one slot, so that chains run past the home slot; returns them, the occupied
    slots (linear probing: the set does not depend on the insertion order), the longest
    probe distance and an absent cx whose home slot is occupied."""
    home = {cx: R.home_slot(R.pack_key(cx, 0, 0), 128) for cx in range(1, 400)}
    by = {}
    for cx, h in home.items():
        by.setdefault(h, []).append(cx)
    crowd = max(by.values(), key=len)[:4]
    rest = [cx for cx in range(1, 400, 3) if cx not in crowd][:64 - len(crowd)]
    chosen = sorted(crowd + rest)
    occ, far = set(), 0
    for cx in chosen:
        h, dist = home[cx], 0
        while h in occ:
            h, dist = (h + 1) & 127, dist + 1
        occ.add(h)
        far = max(far, dist)
    absent = [cx for cx in range(1, 400) if cx not in chosen and home[cx] in occ]
    return chosen, occ, far, absent


@BOTH
def test_lookup_follows_probe_chains_and_stops_at_an_empty_slot(fmx_mod, on_device):
    chosen, occ, far, absent = _lookup_voxels()
    assert len(chosen) == 64 and len(occ) == 64 and far >= 3 and len(absent) > 50
    ctx, ref = _pair(fmx_mod, 1.0, 64, (0.1, 1e12), margin=0)
    assert ctx.dense_stats()["slots"] == 128
    centres = CR.voxel_centres([(cx, 0, 0) for cx in chosen], 1.0)
    _integrate(ctx, ref, centres[::-1], I34, 0)
    assert ctx.dense_stats()["voxels"] == 64
    # along the row: every present voxel once, every absent one (its home slot occupied or not) never
    T, shot = CR.special_pose((0.5, 0.5, 0.5)), np.array([[399.0, 0, 0, 0]], np.float32)
    got = ctx.carve_rays(_arg(shot, on_device), T)
    assert got == ref.carve_rays(shot, T) == dict(rays=1, steps=399, misses=64, exempt=0)
    want = _check(ctx, ref)
    assert (want["misses"] == 1).all()
    # beside the row: absent voxels only, some of them with an occupied home slot
    homes = [R.home_slot(R.pack_key(cx, 1, 0), 128) in occ for cx in range(0, 399)]
    assert any(homes) and not all(homes)
    T1 = CR.special_pose((0.5, 1.5, 0.5))
    assert ctx.carve_rays(_arg(shot, on_device), T1) == ref.carve_rays(shot, T1) == dict(rays=1, steps=399, misses=0,
                                                                                        exempt=0)
    assert CR.same(_check(ctx, ref), want) is None


# ------------------------------------------------------------------ 3. exemption
def _grazing_plane():
    """A floor 0.6 below the sensor, seen out to 20 m: the rays to its far end run through the
    voxels of its middle."""
    xs, ys = np.arange(2.0, 20.0, 0.25), np.arange(-1.0, 1.01, 0.25)
    p = np.zeros((len(xs) * len(ys), 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = np.repeat(xs, len(ys)), np.tile(ys, len(xs)), -0.6
    return p


@BOTH
def test_a_scan_does_not_carve_itself(fmx_mod, on_device):
    p = _grazing_plane()
    assert len(p) < 1000
    ctx, ref = _pair(fmx_mod, 0.5, 4096, margin=1)
    for k in range(2):  # the same scan twice: its voxels are marked again
        c = _integrate(ctx, ref, p, I34, k, on_device)
        assert c["misses"] == 0 and c["exempt"] > 0 and c["rays"] == len(p)
        assert (_check(ctx, ref)["misses"] == 0).all()
    got = ctx.carve_rays(_arg(p, on_device), I34)  # nothing is exempt here
    assert got == ref.carve_rays(p, I34) and got["exempt"] == 0 and got["misses"] == c["exempt"]
    assert _check(ctx, ref)["misses"].sum() == got["misses"] > 0


# ------------------------------------------------------------------ 4. a dynamic object
@BOTH
def test_dynamic_object_is_filtered_out(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod, CR.SCN_W, CR.SCN_CAP, margin=1)
    for k in range(CR.SCN_SCANS):
        _integrate(ctx, ref, CR.scenario_scan(k), I34, k, on_device)
    everything = _check(ctx, ref)
    kept = _check(ctx, ref, 1, 0.5)
    obj = set(CR.scenario_object_keys(ref))
    assert len(obj) == 4 and set(everything["key"].tolist()) - set(kept["key"].tolist()) == obj
    assert all(int(m) >= 3 for k, m in zip(everything["key"].tolist(), everything["misses"]) if k in obj)
    assert (kept["misses"] == 0).all()
    _check(ctx, ref, 2, 0.0)
    _check(ctx, ref, 1, 1000.0)


# ------------------------------------------------------------------ 5. streams
STREAM_CFG = {"odd": (0.5, dict(margin=1)), "tiny": (1.0, dict(margin=2, ray_stride=3, max_norm_squared=900.0))}


@functools.lru_cache(maxsize=None)
def _stream_ref(name):
    """The restatement's counts and key-sorted map after each of three scans (computed once)."""
    w, cfg = STREAM_CFG[name]
    ref = CR.CarveRef(w, 1 << 14)
    ref.carve_configure(**cfg)
    out = []
    for k in range(3):
        counts = ref.integrate(_points(name, k), POSES[k], k)
        out.append((counts, ref.carve_last, ref.sorted()))
    return out


def _stream_run(fmx, name, on_device):
    w, cfg = STREAM_CFG[name]
    ctx = _ctx(fmx, _geo(name))
    ctx.dense_configure(True, w, 1 << 14, min_norm_squared=1.0, max_norm_squared=1e4)
    ctx.carve_configure(**cfg)
    out = []
    for k in range(3):
        counts = ctx.dense_integrate(_arg(_points(name, k), on_device), POSES[k], k)
        out.append((counts, ctx.carve_last(), CR.sort_download(ctx.dense_download(), w)))
    return out


@BOTH
@pytest.mark.parametrize("name", ["odd", "tiny"])
def test_streams_equal_the_restatement_and_repeat(fmx_mod, name, on_device):
    want, got, again = _stream_ref(name), _stream_run(fmx_mod, name, on_device), _stream_run(fmx_mod, name, on_device)
    for k in range(3):
        assert got[k][0] == want[k][0] and got[k][1] == want[k][1], k
        assert CR.same(got[k][2], want[k][2]) is None, (k, CR.same(got[k][2], want[k][2]))
        assert got[k][:2] == again[k][:2] and CR.same(got[k][2], again[k][2]) is None, k
    assert want[2][1][0]["misses"] > 0 and want[2][1][0]["exempt"] > 0 and want[2][2]["misses"].max() > 1


# ------------------------------------------------------------------ 6. roll and clear
@BOTH
def test_roll_keeps_and_hands_over_misses_and_clear_zeroes_them(fmx_mod, on_device):
    ctx, ref = _pair(fmx_mod, 0.5, 1 << 14, geo=_geo("odd"), margin=1)
    for k in range(2):
        _integrate(ctx, ref, _points("odd", k), POSES[k], k, on_device)
    before = _check(ctx, ref)
    centre, half = POSES[1][:, 3], (24, 24, 24)
    inside = {k: m for k, m in zip(before["key"].tolist(), before["misses"].tolist())}
    got = CR.sort_download(ctx.roll_evict(centre, half), 0.5)
    want = ref.evict(centre, half)
    assert CR.same(got, want) is None and len(want["key"]) > 0 and want["misses"].sum() > 0
    after = _check(ctx, ref)
    assert 0 < len(after["key"]) < len(before["key"]) and after["misses"].sum() > 0
    assert all(inside[k] == m for k, m in zip(after["key"].tolist(), after["misses"].tolist()))  # kept: bit for bit
    assert all(inside[k] == m for k, m in zip(want["key"].tolist(), want["misses"].tolist()))
    # a later carve on the rebuilt table, stand-alone and integrating
    assert ctx.carve_rays(_arg(_points("odd", 0), on_device), POSES[0]) == ref.carve_rays(_points("odd", 0), POSES[0])
    _check(ctx, ref)
    _integrate(ctx, ref, _points("odd", 2), POSES[2], 2, on_device)
    _check(ctx, ref)
    ctx.dense_clear()
    ref.clear()
    assert len(ctx.dense_download()["misses"]) == 0
    _integrate(ctx, ref, _points("odd", 1), POSES[1], 7, on_device)  # the same slots again: no stale count
    assert (_check(ctx, ref)["misses"] == 0).all()
    _integrate(ctx, ref, _points("odd", 0), POSES[0], 8, on_device)
    assert _check(ctx, ref)["misses"].sum() > 0


N_REG, W_REG, CAP_REG = 12, 0.5, 1 << 16
REG_CARVE = dict(margin=1, ray_stride=4, max_norm_squared=400.0, every=2)


@functools.lru_cache(maxsize=None)
def _reg_stream():
    world = synth.World()
    out = []
    for k in range(N_REG):
        s = synth.make_scan_skewed("tiny", k, world=world)[0].numpy()
        s.setflags(write=False)
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def _reg_run(dense, carve, roll):
    """One N_REG-scan register_scan stream.  Returns the poses, the per-scan (dense_last,
    carve_last), the key-sorted download and the drained spill (None with the map off)."""
    from form_amd import fmx
    scans = _reg_stream()
    ctx = _ctx(fmx, synth.GEOMETRIES["tiny"], window=(4, 3))
    if dense:
        ctx.dense_configure(True, W_REG, CAP_REG)
    if roll:
        ctx.roll_configure(True, (24, 24, 24), 0.25, True)
    if carve:
        ctx.carve_configure(**REG_CARVE)
    held = [_arg(s, True) for s in scans]
    poses, lasts = [], []
    for k in range(N_REG):
        ctx.register_scan(held[k])
        poses.append(ctx.current_pose().copy())
        lasts.append((ctx.dense_last(), ctx.carve_last()) if dense else None)
    down = CR.sort_download(ctx.dense_download(misses=True), W_REG) if dense else None
    spill = CR.sort_by_owner(ctx.roll_drain(misses=True)) if dense else None
    prof = list(ctx.profile_read())
    ctx.close()
    return poses, lasts, down, spill, prof


def test_register_path_carves_and_spills_misses(fmx_mod):
    scans = _reg_stream()
    poses, lasts, down, spill, _ = _reg_run(True, True, True)
    ref = CR.CarveRef(W_REG, CAP_REG)
    ref.roll_configure(True, (24, 24, 24), 0.25, True)
    ref.carve_configure(**REG_CARVE)
    for k in range(N_REG):
        _, integrated, counts = ref.register(k, scans[k], poses[k], poses[k - 1] if k else None)
        assert lasts[k][0] == (counts, integrated) and integrated == 1, k
        assert lasts[k][1] == ref.carve_last and ref.carve_last[1] == (1 if k % 2 == 0 else 0), k
    assert len(ref.rolls) >= 1 and ref.carve_last == (CR.no_counts(), 0)
    assert CR.same(down, ref.sorted()) is None, CR.same(down, ref.sorted())
    want = ref.drain()
    assert CR.same_owner_sorted(spill, want) is None and len(want["hits"]) > 0
    assert down["misses"].sum() > 0 and want["misses"].sum() > 0


# ------------------------------------------------------------------ 7. off means off
def test_never_configured_reads_as_before(fmx_mod):
    ctx = _ctx(fmx_mod, _geo("odd"))
    ctx.dense_configure(True, 0.5, 1 << 14)
    ctx.profile(True)
    for k in range(2):
        ctx.dense_integrate(_points("odd", k), POSES[k], k)
    assert ctx.carve_last() == (CR.no_counts(), 0)
    plain, ex = ctx.dense_download(), ctx.dense_download(misses=True)
    assert sorted(plain) == ["hits", "index", "points", "scan"] and sorted(ex) == sorted(list(plain) + ["misses"])
    assert R.same(R.sort_download(plain, 0.5), R.sort_download(ex, 0.5)) is None
    assert len(ex["misses"]) == len(plain["hits"]) > 0 and (ex["misses"] == 0).all() and ex["misses"].dtype == np.uint32
    assert len(ctx.dense_download(1, 0.0)["hits"]) == len(plain["hits"])  # misses read 0: every filter passes
    ev = ctx.roll_evict(POSES[1][:, 3], (10, 10, 10), misses=True)
    assert len(ev["misses"]) == len(ev["hits"]) > 0 and (ev["misses"] == 0).all()
    prof = ctx.profile_read()
    assert list(prof)[-1] == "dense" and "carve" not in prof
    assert _status(fmx_mod, lambda: ctx.carve_rays(_points("odd", 0), POSES[0])) == STATE
    ctx.carve_configure(enable=False)  # configured, never enabled: still nothing allocated or launched
    ctx.dense_integrate(_points("odd", 2), POSES[2], 2)
    assert ctx.carve_last() == (CR.no_counts(), 0)
    assert _status(fmx_mod, lambda: ctx.carve_rays(_points("odd", 0), POSES[0])) == STATE
    prof = ctx.profile_read()
    assert list(prof)[-2:] == ["dense", "carve"] and prof["carve"]["launches"] == 0
    ctx.carve_configure(margin=1)
    ctx.dense_integrate(_points("odd", 0), POSES[0], 3)
    assert ctx.profile_read()["carve"]["launches"] == 2  # mark + rays
    ctx.carve_rays(_points("odd", 0), POSES[0])
    assert ctx.profile_read()["carve"]["launches"] == 3  # rays alone


def test_estimation_is_untouched(fmx_mod):
    on, off = _reg_run(True, True, True), _reg_run(False, False, False)
    assert len(on[0]) == N_REG == 12 and "carve" in on[4] and "carve" not in off[4]
    for k in range(N_REG):
        assert np.array_equal(on[0][k].view(np.uint64), off[0][k].view(np.uint64)), k
    assert on[0][-1][:, 3].any()


# ------------------------------------------------------------------ FORM
def test_form_dense_carve_round_trip(fmx_mod):
    import types
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    scans = _reg_stream()[:5]
    g = fmx_mod.FORM()
    g.set_lidar_params(lidar)
    g.set_dense_carve()
    with pytest.raises(ValueError):
        g.initialize()  # needs set_dense_map
    f = fmx_mod.FORM()
    f.set_lidar_params(lidar)
    f.set_dense_carve(True, max_range_m=20.0, margin=1, ray_stride=4)
    f.set_dense_map(True, voxel_width=0.5, max_voxels=1 << 15)
    assert sorted(f.dense_map()) == ["hits", "index", "misses", "points", "scan"] and len(f.dense_map()["misses"]) == 0
    f.initialize()
    ref = CR.CarveRef(0.5, 1 << 15)
    ref.carve_configure(True, 400.0, 1, 4, 1)
    for k in range(5):
        f.add_lidar(scans[k][:, :3])
        ref.integrate(scans[k], f.pose()[:3], k)
        assert f._est.carve_last() == ref.carve_last, k
    d = f.dense_map()
    assert sorted(d) == ["hits", "index", "misses", "points", "scan"] and d["misses"].dtype == np.uint32
    assert CR.same(CR.sort_download(d, 0.5), ref.sorted()) is None and d["misses"].sum() > 0
    some = f.dense_map(2, 0.25)
    assert CR.same(CR.sort_download(some, 0.5), ref.sorted(2, 0.25)) is None and 0 < len(some["hits"]) < len(d["hits"])


# ------------------------------------------------------------------ 8. errors
def test_status_codes_and_too_small_a_capacity(fmx_mod):
    fmx, L = fmx_mod, fmx_mod.lib()
    ctx = _ctx(fmx, _geo("odd"))
    p0 = _points("odd", 0)
    assert _status(fmx, lambda: ctx.carve_configure()) == STATE  # before fmx_dense_configure
    assert _status(fmx, lambda: ctx.carve_rays(p0, POSES[0])) == STATE
    assert _status(fmx, lambda: ctx.dense_download(misses=True)) == STATE
    ctx.dense_configure(True, 0.5, 1 << 14)
    assert L.fmx_carve_configure(ctx.h, None) == INVAL
    for gate in (np.nan, -1.0, -np.inf):
        assert _status(fmx, lambda: ctx.carve_configure(max_norm_squared=gate)) == INVAL, gate
    assert _status(fmx, lambda: ctx.carve_rays(p0, POSES[0])) == STATE  # a refused configuration enabled nothing
    ctx.carve_configure(margin=1, ray_stride=0, every=0)  # 0 = 1
    for k in range(2):
        ctx.dense_integrate(_points("odd", k), POSES[k], k)
        assert ctx.carve_last()[1] == 1
    bad = POSES[0].copy()
    bad[1, 3] = np.inf
    assert _status(fmx, lambda: ctx.carve_rays(p0, bad)) == INVAL
    cnt = fmx._CarveCounts()
    pose = np.ascontiguousarray(POSES[0]).reshape(12)
    assert L.fmx_carve_rays(ctx.h, None, C.c_size_t(5), C.c_int(0), fmx._p(pose), C.byref(cnt)) == INVAL
    assert L.fmx_carve_rays(ctx.h, None, C.c_size_t(0), C.c_int(0), fmx._p(pose), C.byref(cnt)) == 0 and cnt.rays == 0
    assert L.fmx_carve_last(ctx.h, None, None) == 0
    # a filling call with too small a capacity: FMX_E_SIZE and nothing written
    before = CR.sort_download(ctx.dense_download(), 0.5)
    m = len(before["hits"])
    A, out = ctx._voxel_arrays(m, True)
    for v in out.values():
        v.fill(7)
    n = C.c_uint32(m - 1)
    assert L.fmx_carve_download(ctx.h, C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), C.byref(A), C.byref(n)) == SIZE
    assert n.value == m - 1 and all((v == 7).all() for v in out.values())
    centre, half = np.ascontiguousarray(POSES[1][:, 3]), np.array([10, 10, 10], np.uint32)
    evicted = ctx.roll_count(centre, half)[1]
    n = C.c_uint32(evicted - 1)
    assert evicted > 1
    assert L.fmx_carve_evict(ctx.h, fmx._p(centre), fmx._p(half), C.byref(A), C.byref(n)) == SIZE
    assert all((v == 7).all() for v in out.values())
    assert CR.same(CR.sort_download(ctx.dense_download(), 0.5), before) is None  # the map is untouched
    assert L.fmx_carve_download(ctx.h, C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), C.byref(A), None) == INVAL
    # only misses asked for: a filling call all the same
    only = fmx._VoxelArrays()
    only.misses = out["misses"].ctypes.data
    n = C.c_uint32(m)
    assert L.fmx_carve_download(ctx.h, C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), C.byref(only), C.byref(n)) == 0
    assert n.value == m and sorted(out["misses"].tolist()) == sorted(before["misses"].tolist())
    assert (out["hits"] == 7).all()
    # the drain: nothing spilled is a count of 0 either way
    n = C.c_uint32(0)
    assert L.fmx_carve_drain(ctx.h, C.byref(A), C.byref(n)) == 0 and n.value == 0
    # reconfiguring the dense map drops the arrays and turns carving off
    fresh = _ctx(fmx, _geo("odd"))
    fresh.dense_configure(True, 0.5, 1 << 12)
    fresh.carve_configure()
    fresh.dense_configure(True, 0.5, 1 << 13)
    assert _status(fmx, lambda: fresh.carve_rays(p0, POSES[0])) == STATE
    fresh.dense_integrate(p0, POSES[0], 0)
    assert fresh.carve_last() == (CR.no_counts(), 0)

"""Unorganized clouds on the device: fmx_organize against the numpy restatement
(tests/organize_ref.py; equality, which tests/test_organize_cpu.py shows to be a condition
of the inputs), fmx_deskew_cells against fmx_deskew and the per-point restatement, and
fmx_register_cloud against fmx_register_scan of the organized scan, bit for bit."""
import functools
import types

import numpy as np
import pytest
import torch

import deskew_ref as D
import organize_ref as G
from form_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = {"odd": (5, 200), "tiny": (16, 256), "wide": (8, 4096)}
XI_BIG = np.array([0.02, -0.015, 0.1, 1.5, 0.1, -0.05])


def _geo(name):
    r, c = SHAPES[name]
    return synth.ScanGeometry(r, c, 15.0, 0.01, 0.02)


def _ctx(fmx, geo, window=None, **over):
    p = synth.default_params(geo)
    kw = dict(over)
    if window:
        kw.update(max_num_recent_scans=window[0], max_num_keyscans=window[1])
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p), **kw))


@functools.lru_cache(maxsize=None)
def _jit(name, seed):
    r, c = SHAPES[name]
    return G.jittered_cloud(r, c, seed=seed)


@functools.lru_cache(maxsize=None)
def _ref(name, seed, mode, with_fraction=True):
    r, c = SHAPES[name]
    J = _jit(name, seed)
    out = G.organize(J["xyzw"], J["ring"], r, c, J["fraction"] if with_fraction else None,
                     elevation=J["elevation"] if mode == "elevation" else None, **J["cfg"])
    for a in out[:3]:
        if a is not None:
            a.setflags(write=False)
    return out


def _cloud_args(J, on_device, with_fraction=True):
    a = [np.array(J["xyzw"]), np.array(J["ring"]), np.array(J["fraction"]) if with_fraction else None]
    if not on_device:
        return a
    return [torch.from_numpy(a[0]).to("cuda:0"), torch.from_numpy(a[1].view(np.int16)).to("cuda:0"),
            None if a[2] is None else torch.from_numpy(a[2]).to("cuda:0")]


def _np(t, dtype=None):
    if t is None:
        return None
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return a if dtype is None else a.astype(dtype)


def _assert_same(got, ref):
    scan, index, plane, counts = got
    assert counts == ref[3]
    assert np.array_equal(_np(scan).view(np.uint32), ref[0].view(np.uint32))
    assert np.array_equal(_np(index, np.uint32), ref[1])
    if ref[2] is None:
        assert plane is None
    else:
        assert np.array_equal(_np(plane).view(np.uint32), ref[2].view(np.uint32))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", ["ring", "elevation"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_organize_matches_restatement(fmx_mod, name, mode, on_device):
    ctx = _ctx(fmx_mod, _geo(name))
    J = _jit(name, 11)
    ctx.organize_configure(True, elevation=J["elevation"] if mode == "elevation" else None, **J["cfg"])
    # two different clouds back to back, then the first again: a key table that was not
    # put back shows in the second result, counters that were not in the third
    for seed in (11, 12, 11):
        got = ctx.organize(*_cloud_args(_jit(name, seed), on_device))
        _assert_same(got, _ref(name, seed, mode))
    assert _ref(name, 11, mode)[3] != _ref(name, 12, mode)[3]
    got = ctx.organize(*_cloud_args(J, on_device, with_fraction=False))
    _assert_same(got, _ref(name, 11, mode, False))


@pytest.mark.parametrize("mode", ["ring", "elevation"])
@pytest.mark.parametrize("config", ["tiny", "wide"])
def test_round_trip_on_the_device(fmx_mod, config, mode):
    geo = synth.GEOMETRIES[config]
    ctx = _ctx(fmx_mod, geo)
    ctx.organize_configure(True, elevation=synth.elevation_table(geo) if mode == "elevation" else None)
    scan = synth.make_scan(config, 3)[0].numpy()
    xyzw, ring, frac = synth.to_cloud(scan, geo, 9)
    got, index, plane, counts = ctx.organize(xyzw, ring, frac)
    assert np.array_equal(got.view(np.uint32), scan.view(np.uint32))
    assert counts == dict(placed=len(xyzw), displaced=0, off_grid=0, invalid=0)
    filled = scan[:, :3].any(1)
    assert np.array_equal(index != G.EMPTY, filled)
    assert np.array_equal(xyzw[index[filled]], scan[filled])


# ------------------------------------------------------------------ per-point deskew
@functools.lru_cache(maxsize=None)
def _skewed(name):
    geo = _geo(name)
    scan = synth.raycast_skewed(synth.World(), lambda s: synth.trajectory_pose(3 + s), geo, 77).numpy()
    scan.setflags(write=False)
    return scan, geo


def _column_fractions(geo):
    return (np.arange(geo.cols, dtype=np.float64) / geo.cols).astype(np.float32)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_deskew_cells_equals_the_column_kernel(fmx_mod, name, on_device):
    scan, geo = _skewed(name)
    tab = _column_fractions(geo)
    ctx = _ctx(fmx_mod, geo)
    ctx.deskew_configure(True, column_fraction=tab)
    per_point = np.tile(tab, geo.rows)
    if on_device:
        d = torch.from_numpy(np.array(scan)).to("cuda:0")
        want = ctx.deskew(d, XI_BIG).cpu().numpy()
        got = ctx.deskew_cells(d, torch.from_numpy(per_point).to("cuda:0"), XI_BIG).cpu().numpy()
        zero = ctx.deskew_cells(d, torch.from_numpy(per_point).to("cuda:0"), np.zeros(6)).cpu().numpy()
    else:
        want = ctx.deskew(np.array(scan), XI_BIG)
        got = ctx.deskew_cells(np.array(scan), per_point, XI_BIG)
        zero = ctx.deskew_cells(np.array(scan), per_point, np.zeros(6))
    assert (want[:, :3] != scan[:, :3]).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(zero.view(np.uint32), scan.view(np.uint32))  # a zero twist reproduces the input


@functools.lru_cache(maxsize=None)
def _cells_ref(name):
    import oracle_py
    scan, geo = _skewed(name)
    r, c = np.divmod(np.arange(geo.rows * geo.cols), geo.cols)
    frac = np.clip((c + 0.3 * r / geo.rows) / geo.cols, 0.0, 1.0).astype(np.float32)
    out = G.deskew_cells(oracle_py, scan, frac, XI_BIG)
    out.setflags(write=False)
    frac.setflags(write=False)
    return frac, out


@pytest.mark.parametrize("name", list(SHAPES))
def test_deskew_cells_matches_restatement(fmx_mod, name):
    scan, geo = _skewed(name)
    frac, ref = _cells_ref(name)
    ctx = _ctx(fmx_mod, geo)
    got = ctx.deskew_cells(np.array(scan), np.array(frac), XI_BIG)
    u = D.ulp_diff(got[:, :3], ref[:, :3])
    differ = int((u > 0).sum())
    print(f"max ulp {u.max()}, coordinates differing {differ} of {u.size}")
    assert u.max() <= 1
    assert differ <= 1e-4 * u.size
    drop = ~scan[:, :3].any(1)
    assert drop.any()
    assert not got[drop].any()   # dropouts stay exactly 0
    assert not got[:, 3].any()   # so does the pad
    # the fractions down the column matter: not what the column kernel gives
    ctx.deskew_configure(True, column_fraction=_column_fractions(geo))
    assert not np.array_equal(got, ctx.deskew(np.array(scan), XI_BIG))


# ------------------------------------------------------------------ registration
@functools.lru_cache(maxsize=None)
def _stream(n):
    world = synth.World()
    out = []
    for k in range(n):
        s = synth.make_scan_skewed("tiny", k, world=world)[0].numpy()
        s.setflags(write=False)
        out.append(s)
    return out


def _same_state(a, b, k):
    assert np.array_equal(a.current_pose(), b.current_pose()), k
    fa, fb = a.extract_download(), b.extract_download()
    for key in ("planar_index", "point_index", "planar", "point"):
        assert np.array_equal(fa[key], fb[key]), (k, key)
    assert a.last_stats() == b.last_stats(), k


@pytest.mark.parametrize("deskew", [False, True], ids=["plain", "deskewed"])
@pytest.mark.parametrize("mode", ["ring", "elevation"])
def test_register_cloud_equals_register_scan(fmx_mod, mode, deskew):
    n = 12
    geo = synth.GEOMETRIES["tiny"]
    scans = _stream(n)
    org, cld = _ctx(fmx_mod, geo, window=(4, 3)), _ctx(fmx_mod, geo, window=(4, 3))
    xi0 = np.array([0.0, 0.0, 0.01, 0.15, 0.0, 0.0])
    if deskew:  # the column table on one side, the same values per point on the other
        org.deskew_configure(True, initial_twist=xi0, column_fraction=_column_fractions(geo))
        cld.deskew_configure(True, initial_twist=xi0)
    cld.organize_configure(True, elevation=synth.elevation_table(geo) if mode == "elevation" else None)
    for k in range(n):
        xyzw, ring, frac = synth.to_cloud(scans[k], geo, 100 + k)
        a = org.register_scan(torch.from_numpy(np.array(scans[k])).to("cuda:0"))
        on_device = k % 2 == 1  # host and device clouds in turn
        args = _cloud_args(dict(xyzw=xyzw, ring=ring, fraction=frac), on_device)
        b = cld.register_cloud(*args)
        assert a == b[:2], k
        assert b[2] == dict(placed=len(xyzw), displaced=0, off_grid=0, invalid=0), k
        _same_state(org, cld, k)
        (xa, sa), (xb, sb) = org.deskew_last(), cld.deskew_last()
        assert sa == sb == ((1 if k < 2 else 2) if deskew else 0) and np.array_equal(xa, xb), k
    if deskew:
        assert cld.current_pose()[:, 3].any()


def test_error_paths(fmx_mod):
    geo = synth.GEOMETRIES["tiny"]
    ctx = _ctx(fmx_mod, geo)
    scan = synth.make_scan("tiny", 0)[0].numpy()
    xyzw, ring, frac = synth.to_cloud(scan, geo, 1)
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.organize(xyzw, ring)  # not configured
    assert e.value.status == 5  # FMX_E_STATE
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.register_cloud(xyzw, ring)
    assert e.value.status == 5
    tab = synth.elevation_table(geo).copy()
    for bad in (tab[::-1][3], np.nan, np.inf):  # not monotonic / not finite
        t = tab.copy()
        t[5] = bad
        with pytest.raises(fmx_mod.FmxError) as e:
            ctx.organize_configure(True, elevation=t)
        assert e.value.status == 1  # FMX_E_INVAL
    t = tab.copy()
    t[6] = t[5]  # monotonic, not strictly
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.organize_configure(True, elevation=t)
    assert e.value.status == 1
    for kw in (dict(ring_to_row=[0, geo.rows]), dict(azimuth_offset=np.nan)):
        with pytest.raises(fmx_mod.FmxError) as e:
            ctx.organize_configure(True, **kw)
        assert e.value.status == 1
    ctx.organize_configure(False)  # configured, not enabled
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.organize(xyzw, ring)
    assert e.value.status == 5
    ctx.organize_configure(True)
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.organize(xyzw, None)  # ring mode without rings
    assert e.value.status == 1
    # an empty cloud: an all-zero scan
    got, index, plane, counts = ctx.organize(np.zeros((0, 4), np.float32))
    assert not got.any() and got.shape == (geo.rows * geo.cols, 4)
    assert (index == G.EMPTY).all() and plane is None
    assert counts == dict(placed=0, displaced=0, off_grid=0, invalid=0)
    # ... and the table is as it was: a cloud after the rejected calls organizes as usual
    got = ctx.organize(xyzw, ring)[0]
    assert np.array_equal(got.view(np.uint32), scan.view(np.uint32))
    # a ring table: rows upside down, the last ring dropped
    r2r = np.arange(geo.rows)[::-1].copy()
    r2r[-1] = -1
    ctx.organize_configure(True, ring_to_row=r2r)
    got, _, _, counts = ctx.organize(xyzw, ring)
    want = scan.reshape(geo.rows, geo.cols, 4)[::-1].copy()
    want[0] = 0
    assert np.array_equal(got, want.reshape(-1, 4))
    assert counts["off_grid"] == int((ring == geo.rows - 1).sum()) > 0
    # configure after a registration is refused
    ctx.register_cloud(xyzw, ring)
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.organize_configure(True)
    assert e.value.status == 5


def test_unused_stage_changes_nothing(fmx_mod):
    n = 6
    geo = synth.GEOMETRIES["tiny"]
    scans = [torch.from_numpy(np.array(s)).to("cuda:0") for s in _stream(n)]
    plain, unused = _ctx(fmx_mod, geo), _ctx(fmx_mod, geo)
    unused.organize_configure(True, elevation=synth.elevation_table(geo), azimuth_offset=0.2, clockwise=True)
    plain.profile(True)
    for k in range(n):
        plain.register_scan(scans[k])
        if k + 1 < n:
            unused.next_scan(scans[k + 1])
        unused.register_scan(scans[k])
        assert np.array_equal(plain.current_pose(), unused.current_pose()), k
        fa, fb = plain.extract_download(), unused.extract_download()
        for key in ("planar_index", "point_index", "planar", "point"):
            assert np.array_equal(fa[key], fb[key]), (k, key)
        assert unused.last_stats()["pipelined"] == (1 if k > 0 else 0)
    prof = plain.profile_read()
    assert prof["organize"]["launches"] == 0 and prof["extract_rows"]["launches"] > 0
    assert list(prof)[-2:] == ["deskew", "organize"]  # appended: the earlier ids keep their index


def test_profile_counts_both_launches(fmx_mod):
    ctx = _ctx(fmx_mod, _geo("tiny"))
    J = _jit("tiny", 11)
    ctx.organize_configure(True, **J["cfg"])
    ctx.profile(True)
    ctx.organize(*_cloud_args(J, True))
    p = ctx.profile_read()["organize"]
    n, cells = len(J["xyzw"]), 16 * 256
    assert p["launches"] == 2
    assert p["bytes"] == n * (16 + 2 + 4 + 8) + cells * (8 + 16 + 16 + 4 + 4)


def test_form_add_lidar_takes_clouds(fmx_mod):
    geo = synth.GEOMETRIES["tiny"]
    lidar = types.SimpleNamespace(min_range=1.0, max_range=100.0, num_rows=geo.rows, num_columns=geo.cols, rate=10.0)
    world = synth.World()
    a, b = fmx_mod.FORM(), fmx_mod.FORM()
    b.set_organize(True)
    for f in (a, b):
        f.set_lidar_params(lidar)
        f.initialize()
    for k in range(4):
        scan = synth.make_scan("tiny", k, world=world)[0].numpy()
        xyzw, ring, frac = synth.to_cloud(scan, geo, 50 + k)
        fa = a.add_lidar(types.SimpleNamespace(points=scan[:, :3].astype(np.float64)))
        cloud = np.concatenate([xyzw[:, :3].astype(np.float64), ring[:, None].astype(np.float64),
                                frac[:, None].astype(np.float64) * 0.1], 1)  # (N, 5): x, y, z, ring, time (s)
        assert len(cloud) < geo.rows * geo.cols
        fb = b.add_lidar(types.SimpleNamespace(points=cloud))
        assert np.array_equal(a.pose(), b.pose()), k
        assert np.array_equal(fa["planar"], fb["planar"]) and np.array_equal(fa["point"], fb["point"])

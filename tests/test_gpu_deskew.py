"""Scan deskewing on the device: the stand-alone kernel against the numpy restatement
(tests/deskew_ref.py), and fmx_register_scan with deskewing on against the oracle fed the
same deskewed scans — sequential, pipelined, with caller twists, and switched off."""
import functools

import numpy as np
import pytest
import torch

import deskew_ref as D
from form_amd import metrics, synth

pytestmark = pytest.mark.gpu

XI_BIG = np.array([0.02, -0.015, 0.1, 1.5, 0.1, -0.05])  # rotation + translation
XI_TRANS = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.05])    # no rotation: expmap's small-angle branch
SHAPES = {"tiny": (16, 256), "wide": (8, 4096), "odd": (5, 200)}  # odd: cols % 64 != 0, odd rows


def _geo(name):
    if name in synth.GEOMETRIES:
        return synth.GEOMETRIES[name]
    r, c = SHAPES[name]
    return synth.ScanGeometry(r, c, 15.0, 0.01, 0.02)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(skewed scan (N, 4) float32 with dropouts, geometry) of a stand-alone shape."""
    geo = _geo(name)
    assert (geo.rows, geo.cols) == SHAPES[name]
    scan = synth.raycast_skewed(synth.World(), lambda s: synth.trajectory_pose(3 + s), geo, 77).numpy()
    scan.setflags(write=False)
    return scan, geo


@functools.lru_cache(maxsize=None)
def _ref(name, which, table):
    import oracle_py
    scan, geo = _case(name)
    xi = {"big": XI_BIG, "trans": XI_TRANS}[which]
    tab = None if table is None else _table(geo.cols, table)
    out = D.deskew(oracle_py, scan, geo.rows, geo.cols, xi, tab)
    out.setflags(write=False)
    return out


def _table(cols, kind):
    if kind == "reversed":
        return (np.arange(cols, dtype=np.float64) / cols)[::-1].astype(np.float32)
    return np.full(cols, 0.5, np.float32)


def _ctx(fmx, geo, single=False, window=None, **over):
    p = synth.default_params(geo)
    kw = dict(over)
    if window:
        kw.update(max_num_recent_scans=window[0], max_num_keyscans=window[1])
    return fmx.Context(fmx.EstimatorParams(extraction=fmx.KeypointExtractionParams(**p), disable_smoothing=single, **kw))


def _run(ctx, scan, xi, on_device):
    if on_device:
        return ctx.deskew(torch.from_numpy(np.array(scan)).to("cuda:0"), xi).cpu().numpy()
    return ctx.deskew(np.array(scan), xi)


def _check_against(got, ref, scan):
    u = D.ulp_diff(got[:, :3], ref[:, :3])
    differ = int((u > 0).sum())
    print(f"max ulp {u.max()}, coordinates differing {differ} of {u.size}")
    assert u.max() <= 1
    assert differ <= 1e-4 * u.size
    drop = ~scan[:, :3].any(1)
    assert drop.any()
    assert not got[drop].any()        # dropouts stay exactly 0
    assert not got[:, 3].any()        # so does the pad


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_deskew_matches_restatement(fmx_mod, name, on_device):
    scan, geo = _case(name)
    ctx = _ctx(fmx_mod, geo)
    for which, xi in (("big", XI_BIG), ("trans", XI_TRANS)):
        got = _run(ctx, scan, xi, on_device)
        _check_against(got, _ref(name, which, None), scan)
        assert (got[:, :3] != scan[:, :3]).any()
    # a zero twist reproduces the input bit for bit
    got = _run(ctx, scan, np.zeros(6), on_device)
    assert np.array_equal(got.view(np.uint32), scan.view(np.uint32))


@pytest.mark.parametrize("name", list(SHAPES))
def test_deskew_column_tables(fmx_mod, name):
    scan, geo = _case(name)
    ctx = _ctx(fmx_mod, geo)
    ctx.deskew_configure(True, column_fraction=_table(geo.cols, "reversed"))
    _check_against(_run(ctx, scan, XI_BIG, True), _ref(name, "big", "reversed"), scan)
    assert not np.array_equal(_ref(name, "big", "reversed"), _ref(name, "big", None))
    ctx.deskew_configure(True, column_fraction=_table(geo.cols, "half"))
    got = _run(ctx, scan, XI_BIG, False)
    assert np.array_equal(got.view(np.uint32), scan.view(np.uint32))  # every column at mid-sweep: identity
    ctx.deskew_configure(True)  # back to c / cols
    _check_against(_run(ctx, scan, XI_BIG, True), _ref(name, "big", None), scan)


def test_deskew_rejects_bad_arguments(fmx_mod):
    scan, geo = _case("tiny")
    ctx = _ctx(fmx_mod, geo)
    for bad in (1.5, -0.01, np.nan, np.inf):
        t = _table(geo.cols, "half").copy()
        t[geo.cols // 3] = bad
        with pytest.raises(fmx_mod.FmxError) as e:
            ctx.deskew_configure(True, column_fraction=t)
        assert e.value.status == 1  # FMX_E_INVAL
    d = torch.from_numpy(np.array(scan)).to("cuda:0")
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.deskew(d, XI_BIG, out=d)  # aliased
    assert e.value.status == 1
    h = np.array(scan)
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.deskew(h, XI_BIG, out=h)
    assert e.value.status == 1
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.deskew(h[:-1], XI_BIG)  # not rows * cols points
    assert e.value.status == 2  # FMX_E_SIZE
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.deskew_set_twist(XI_BIG)  # deskewing not enabled
    assert e.value.status == 5  # FMX_E_STATE
    # the rejected calls left nothing behind
    assert np.array_equal(_run(ctx, scan, np.zeros(6), True), scan)


def test_device_deskew_restores_planes(fmx_mod, oracle):
    from test_deskew_cpu import PLANE_XI, plane_case
    scan, Tmid, world, geo = plane_case(oracle)
    ctx = _ctx(fmx_mod, geo)
    raw = D.room_plane_distance(world, D.to_world(Tmid, scan[:, :3])).max()
    got = _run(ctx, scan, PLANE_XI, True)
    fixed = D.room_plane_distance(world, D.to_world(Tmid, got[:, :3])).max()
    print(f"max plane distance: raw {raw:.3g} m, deskewed on the device {fixed:.3g} m")
    assert fixed < 1e-4
    assert raw > 0.1


# ------------------------------------------------------------------ registration
def _inv(T):
    o = np.zeros((3, 4))
    o[:, :3] = T[:, :3].T
    o[:, 3] = -T[:, :3].T @ T[:, 3]
    return o


def _gt_twist(oracle, k):
    """Log(T(k)^-1 T(k+1)) of the synthetic trajectory."""
    return oracle.logmap(oracle.compose(_inv(synth.trajectory_pose(k)), synth.trajectory_pose(k + 1)))


@functools.lru_cache(maxsize=None)
def _skewed_stream(config, n):
    world = synth.World()
    out = []
    for k in range(n):
        s = synth.make_scan_skewed(config, k, world=world)[0].numpy()
        s.setflags(write=False)
        out.append(s)
    return out


def _oracle_est(oracle, geo, single, window=None):
    prm = oracle.default_params(synth.default_params(geo))
    prm.disable_smoothing = int(single)
    if window:
        prm.max_num_recent_scans, prm.max_num_keyscans = window
    return oracle.Estimator(prm)


@pytest.mark.parametrize("single", [False, True], ids=["smoothing", "single_pose"])
def test_deskewed_stream_matches_oracle(fmx_mod, oracle, single):
    """After each scan the oracle registers the scan fmx_deskew gives with the twist
    fmx_deskew_last reports: the poses agree to the stream tolerance, so the registration
    deskewed with exactly that twist."""
    n = 12
    geo = synth.GEOMETRIES["small"]
    scans = _skewed_stream("small", n)
    ctx = _ctx(fmx_mod, geo, single)
    ctx.deskew_configure(True, initial_twist=_gt_twist(oracle, 0))
    oest = _oracle_est(oracle, geo, single)
    poses, srcs = [], []
    for k in range(n):
        ctx.register_scan(np.array(scans[k]))
        xi, src = ctx.deskew_last()
        srcs.append(src)
        To, _, _ = oest.register_scan(ctx.deskew(np.array(scans[k]), xi))
        T = ctx.current_pose()
        assert np.abs(T - To).max() < 1e-6, k
        if k < 2:
            assert np.array_equal(xi, _gt_twist(oracle, 0))
        elif single:  # poses never move afterwards: the twist is that of the poses read back
            want = oracle.logmap(oracle.compose(_inv(poses[k - 2]), poses[k - 1]))
            assert np.abs(xi - want).max() < 1e-12, k
        poses.append(T)
    assert srcs == [1, 1] + [2] * (n - 2)


@pytest.mark.parametrize("host", [False, True], ids=["device", "pageable_host"])
def test_pipelined_deskew_equals_sequential(fmx_mod, host):
    """fmx_next_scan with deskewing on: the announced scan's twist needs the final poses
    of the scan before it, so its extraction is queued at the end of that registration —
    same twist, features and poses as the sequential path, bit for bit (a short window:
    keyscan marginalizations are in play)."""
    n = 14
    geo = synth.GEOMETRIES["tiny"]
    raw = _skewed_stream("tiny", n)
    scans = [np.array(s) if host else torch.from_numpy(np.array(s)).to("cuda:0") for s in raw]
    seq, pip = _ctx(fmx_mod, geo, window=(4, 3)), _ctx(fmx_mod, geo, window=(4, 3))
    xi0 = np.array([0.0, 0.0, 0.01, 0.15, 0.0, 0.0])
    for c in (seq, pip):
        c.deskew_configure(True, initial_twist=xi0)
    for k in range(n):
        seq.register_scan(scans[k])
        if k + 1 < n:
            pip.next_scan(scans[k + 1])
        pip.register_scan(scans[k])
        assert np.array_equal(seq.current_pose(), pip.current_pose()), k
        a, b = seq.extract_download(), pip.extract_download()
        for key in ("planar_index", "point_index", "planar", "point"):
            assert np.array_equal(a[key], b[key]), (k, key)
        (xa, sa), (xb, sb) = seq.deskew_last(), pip.deskew_last()
        assert sa == sb == (1 if k < 2 else 2) and np.array_equal(xa, xb), k
        assert seq.last_stats()["pipelined"] == 0
        assert pip.last_stats()["pipelined"] == (1 if k > 0 else 0)
    # back to back (nothing between the calls): the queued extraction is then usually still
    # running when its registration starts, which does its host work first
    b2b = _ctx(fmx_mod, geo, window=(4, 3))
    b2b.deskew_configure(True, initial_twist=xi0)
    for k in range(n):
        if k + 1 < n:
            b2b.next_scan(scans[k + 1])
        b2b.register_scan(scans[k])
    assert np.array_equal(b2b.current_pose(), seq.current_pose())
    assert np.array_equal(b2b.deskew_last()[0], seq.deskew_last()[0])
    assert b2b.last_stats()["pipelined"] == 1
    a, b = seq.extract_download(), b2b.extract_download()
    for key in ("planar_index", "point_index", "planar", "point"):
        assert np.array_equal(a[key], b[key]), key
    # the scans handed in were never written
    for s, r in zip(scans, raw):
        assert np.array_equal(s if host else s.cpu().numpy(), r)


def test_caller_twist_overrides(fmx_mod, oracle):
    """fmx_deskew_set_twist before each scan: reported back with source 3, and the poses
    are those of the oracle fed scans deskewed with those twists.  A second context that
    also announces its scans must drop each queued extraction (it used another twist) and
    say so; its results stay bit-identical."""
    n = 6
    geo = synth.GEOMETRIES["small"]
    scans = _skewed_stream("small", n)
    dev = [torch.from_numpy(np.array(s)).to("cuda:0") for s in scans]
    ctx, pip = _ctx(fmx_mod, geo), _ctx(fmx_mod, geo)
    ctx.deskew_configure(True)
    pip.deskew_configure(True)
    oest = _oracle_est(oracle, geo, False)
    for k in range(n):
        xi = _gt_twist(oracle, k)
        ctx.deskew_set_twist(xi)
        ctx.register_scan(np.array(scans[k]))
        got, src = ctx.deskew_last()
        assert src == 3 and np.array_equal(got, xi)
        To, _, _ = oest.register_scan(ctx.deskew(np.array(scans[k]), xi))
        assert np.abs(ctx.current_pose() - To).max() < 1e-6, k
        # announced, queued with the constant-velocity twist, then overridden
        pip.deskew_set_twist(xi)
        if k + 1 < n:
            pip.next_scan(dev[k + 1])
        pip.register_scan(dev[k])
        assert pip.last_stats()["pipelined"] == 0
        assert pip.deskew_last()[1] == 3
        assert np.array_equal(pip.current_pose(), ctx.current_pose()), k
    # without a new twist the next scan falls back to constant velocity
    ctx.register_scan(np.array(scans[n - 1]))
    assert ctx.deskew_last()[1] == 2


def test_disabled_deskew_is_bit_identical(fmx_mod):
    n = 6
    geo = synth.GEOMETRIES["tiny"]
    scans = [torch.from_numpy(np.array(s)).to("cuda:0") for s in _skewed_stream("tiny", n)]
    plain, off = _ctx(fmx_mod, geo), _ctx(fmx_mod, geo)
    off.deskew_configure(False, initial_twist=XI_BIG, column_fraction=_table(geo.cols, "reversed"))
    for k in range(n):
        plain.register_scan(scans[k])
        if k + 1 < n:
            off.next_scan(scans[k + 1])
        off.register_scan(scans[k])
        assert np.array_equal(plain.current_pose(), off.current_pose()), k
        a, b = plain.extract_download(), off.extract_download()
        for key in ("planar_index", "point_index", "planar", "point"):
            assert np.array_equal(a[key], b[key]), (k, key)
        xi, src = off.deskew_last()
        assert src == 0 and not xi.any()
        assert off.last_stats()["pipelined"] == (1 if k > 0 else 0)
    assert "deskew" in plain.profile_read()


def test_configure_after_registration_is_refused(fmx_mod):
    geo = synth.GEOMETRIES["tiny"]
    ctx = _ctx(fmx_mod, geo)
    ctx.deskew_configure(True)
    ctx.deskew_configure(True, initial_twist=XI_TRANS)  # still before the first scan: fine
    ctx.register_scan(np.array(_skewed_stream("tiny", 1)[0]))
    with pytest.raises(fmx_mod.FmxError) as e:
        ctx.deskew_configure(True)
    assert e.value.status == 5  # FMX_E_STATE
    assert ctx.deskew_last()[1] == 1


def test_deskew_improves_ate(fmx_mod, oracle):
    """C2, 30 skewed scans generated on the device, ground truth the mid-sweep poses.
    The CPU oracle gave 9.5 mm with and 15.7 mm without deskewing on such a stream (ratio
    0.60; profiles/deskew_ate.json holds the figures re-measured with exactly these
    inputs, by tools/deskew_cost.py --ate); the GPU path tracks the oracle to 1e-6."""
    n = 30
    geo = synth.GEOMETRIES["c2"]
    world = synth.World()
    scans = [synth.make_scan_skewed("c2", k, device="cuda:0", world=world)[0] for k in range(n)]
    gt = [synth.trajectory_pose(k + 0.5) for k in range(n)]
    ate = {}
    for on in (False, True):
        ctx = _ctx(fmx_mod, geo)
        if on:
            ctx.deskew_configure(True, initial_twist=_gt_twist(oracle, 0))
        est = []
        for k in range(n):
            ctx.register_scan(scans[k])
            est.append(ctx.current_pose())
        ate[on] = metrics.ate_rmse(est, gt) * 1e3
    print(f"ATE: deskew off {ate[False]:.2f} mm, on {ate[True]:.2f} mm, ratio {ate[True] / ate[False]:.3f}")
    assert ate[True] <= 0.75 * ate[False]

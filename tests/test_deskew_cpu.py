"""Scan deskewing, the parts that need no GPU: the skewed ray caster, the numpy
restatement of the kernel (tests/deskew_ref.py) and the C ABI's null-context checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import deskew_ref as D
from form_amd import synth


@pytest.mark.parametrize("config", ["tiny", "small"])
def test_raycast_skewed_constant_pose_equals_raycast(config):
    geo = synth.GEOMETRIES[config]
    world = synth.World()
    for k in (0, 3):
        T = synth.trajectory_pose(k)
        a = synth.raycast(world, T, geo, synth.SEED + 7919 * (k + 1))
        b = synth.raycast_skewed(world, lambda s: T, geo, synth.SEED + 7919 * (k + 1))
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a, b) and np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))


def test_make_scan_skewed_shares_the_dropout_stream():
    """Same noise / dropout stream as make_scan: the same rays drop out."""
    world = synth.World()
    a = synth.make_scan("tiny", 2, world=world)[0].numpy()
    b, T, geo = synth.make_scan_skewed("tiny", 2, world=world)
    assert np.array_equal(T, synth.trajectory_pose(2.5))
    za, zb = ~a[:, :3].any(1), ~b.numpy()[:, :3].any(1)
    assert (za != zb).mean() < 0.01  # only rays whose hit crosses max_range may differ
    assert not np.array_equal(a, b.numpy())


PLANE_XI = np.array([0.004, -0.003, 0.02, 0.3, 0.02, -0.01])


def plane_case(oracle):
    """An empty room swept with a constant twist: (skewed scan, mid-sweep pose, world,
    geometry).  Noise and dropouts off, so every point lies on a room plane."""
    g = synth.GEOMETRIES["small"]
    geo = synth.ScanGeometry(g.rows, g.cols, g.elev_deg, 0.0, 0.0, g.max_range)
    world = synth.World(n_boxes=0, n_cyl=0)
    T0 = synth.trajectory_pose(5)
    scan = synth.raycast_skewed(world, lambda s: D.se3(oracle, T0, s * PLANE_XI), geo, 1)
    return scan.numpy(), D.se3(oracle, T0, 0.5 * PLANE_XI), world, geo


def test_restatement_restores_planes(oracle):
    scan, Tmid, world, geo = plane_case(oracle)
    assert scan[:, :3].any(1).all()
    raw = D.room_plane_distance(world, D.to_world(Tmid, scan[:, :3])).max()
    dsk = D.deskew(oracle, scan, geo.rows, geo.cols, PLANE_XI)
    fixed = D.room_plane_distance(world, D.to_world(Tmid, dsk[:, :3])).max()
    wrong = D.room_plane_distance(world, D.to_world(Tmid, D.deskew(oracle, scan, geo.rows, geo.cols, -PLANE_XI)[:, :3])).max()
    print(f"max plane distance: raw {raw:.3g} m, deskewed {fixed:.3g} m, sign flipped {wrong:.3g} m")
    assert fixed < 1e-4  # the fp32 ulp at 100 m is 7.6e-6
    assert raw > 0.1
    assert wrong > raw


def test_restatement_identity_and_dropouts(oracle):
    scan, _, geo = synth.make_scan_skewed("tiny", 1)
    scan = scan.numpy()
    assert np.array_equal(D.deskew(oracle, scan, geo.rows, geo.cols, np.zeros(6)), scan)
    assert np.array_equal(D.deskew(oracle, scan, geo.rows, geo.cols, PLANE_XI, np.full(geo.cols, 0.5)), scan)
    out = D.deskew(oracle, scan, geo.rows, geo.cols, PLANE_XI)
    drop = ~scan[:, :3].any(1)
    assert drop.any() and not out[drop].any() and not out[:, 3].any()
    assert (out[~drop, :3] != scan[~drop, :3]).any(1).mean() > 0.9


def test_deskew_null_context_is_rejected():
    from form_amd import fmx
    L = fmx.lib()
    xi = (C.c_double * 6)()
    src = C.c_int(0)
    buf = (C.c_float * 16)()
    out = (C.c_float * 16)()
    p = fmx._DeskewParams()
    assert L.fmx_deskew_configure(None, C.byref(p)) == 1  # FMX_E_INVAL
    assert L.fmx_deskew_set_twist(None, xi) == 1
    assert L.fmx_deskew_last(None, xi, C.byref(src)) == 1
    assert L.fmx_deskew(None, buf, C.c_size_t(4), C.c_int(0), xi, out, C.c_int(0)) == 1


def test_set_deskew_is_not_a_pipeline_key():
    from form_amd import fmx
    f = fmx.FORM()
    before = dict(f.get_params())
    f.set_deskew(True, initial_twist=[0, 0, 0.01, 0.15, 0, 0])
    assert f.get_params() == before == fmx.FORM.default_params()
    with pytest.raises(KeyError):
        f.set_params({"deskew": True})

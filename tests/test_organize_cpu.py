"""The cloud organizer's specification on the host: the numpy restatement
(tests/organize_ref.py) round-trips synthetic scans and resolves collisions as
include/fmx/fmx.h says; the conditions under which the device tests may ask for equality
hold for the jittered cloud; the new entry points reject a NULL context."""
import ctypes as C

import numpy as np
import pytest

import organize_ref as G
from form_amd import synth

SHAPES = [(5, 200), (16, 256), (8, 4096)]  # odd rows and cols % 64 != 0; tiny; the wide path


@pytest.mark.parametrize("mode", ["ring", "elevation"])
@pytest.mark.parametrize("config", ["tiny", "small", "c2", "wide"])
def test_round_trip(config, mode):
    geo = synth.GEOMETRIES[config]
    world = synth.World()
    for k in (0, 3):
        scan = synth.make_scan(config, k, world=world)[0].numpy()
        xyzw, ring, frac = synth.to_cloud(scan, geo, seed=k + 1)
        assert len(xyzw) == int(scan[:, :3].any(1).sum()) < len(scan)
        assert not np.array_equal(xyzw, scan[scan[:, :3].any(1)])  # shuffled
        elev = synth.elevation_table(geo) if mode == "elevation" else None
        got, index, plane, counts = G.organize(xyzw, ring, geo.rows, geo.cols, frac, elevation=elev)
        assert np.array_equal(got.view(np.uint32), scan.view(np.uint32))
        assert counts == dict(placed=len(xyzw), displaced=0, off_grid=0, invalid=0)
        filled = index != G.EMPTY
        assert np.array_equal(filled, scan[:, :3].any(1))
        cols = np.arange(geo.rows * geo.cols) % geo.cols
        assert np.array_equal(plane[filled], (cols[filled] / geo.cols).astype(np.float32))
        assert not plane[~filled].any()


@pytest.mark.parametrize("seed", [11, 12])  # 12: the second cloud of the device test
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_jittered_cloud_meets_the_equality_conditions(shape, seed):
    rows, cols = shape
    J = G.jittered_cloud(rows, cols, seed=seed)
    xyzw, ring, frac, tab, cfg = J["xyzw"], J["ring"], J["fraction"], J["elevation"], J["cfg"]
    n = len(xyzw)
    row, col, valid, on, dcol, drow = G.cells_of(xyzw, ring, rows, cols, elevation=tab, **cfg)
    assert 0 < (~valid).sum() < 20
    # far enough from every cell boundary that no fp64 atan2 can change a cell
    col_margin, row_margin = 0.5 - dcol[valid].max(), 0.5 - drow[valid].max()
    print(f"{rows} x {cols}: {n} points, margins {col_margin:.3f} columns, {row_margin:.3f} spacings")
    assert col_margin >= 0.05 and row_margin >= 0.1
    assert on[valid].all()
    real = valid & (ring < rows)
    assert np.array_equal(row[real], ring[real])  # elevation mode finds every point's ring
    for elev in (None, tab):
        scan, index, plane, counts = G.organize(xyzw, ring, rows, cols, frac, elevation=elev, **cfg)
        assert sum(counts.values()) == n
        assert counts["invalid"] == int((~valid).sum())
        assert counts["off_grid"] == (2 if elev is None else 0)  # the two rings the sensor does not have
        assert counts["displaced"] > 0.1 * n
        empty = index == G.EMPTY
        assert 0.15 < empty.mean() < 0.35  # integers(0, 4): a quarter of the cells get no point
        assert not scan[empty].any() and not plane[empty].any()
        assert np.array_equal(scan[~empty, :3], xyzw[index[~empty], :3]) and not scan[:, 3].any()
        assert np.array_equal(plane[~empty], frac[index[~empty]])
        # a winner with an exact duplicate: the lower index has the cell
        eligible = G.cells_of(xyzw, ring, rows, cols, elevation=elev, **cfg)[3]
        bits = np.ascontiguousarray(xyzw[:, :3]).view(np.dtype((np.void, 12))).reshape(-1)
        _, inv, cnt = np.unique(bits, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        first = np.full(len(cnt), n)
        np.minimum.at(first, inv[eligible], np.flatnonzero(eligible))
        winners = index[~empty].astype(np.int64)
        assert (cnt[inv[winners]] > 1).sum() > 0.02 * len(winners)
        assert np.array_equal(first[inv[winners]], winners)


def test_restatement_keeps_the_nearest_then_the_first():
    # one cell, three ranges, the nearest twice: index 1 wins over its later copy
    xyzw = np.array([[5, 0, 0, 0], [2, 0, 0, 0], [9, 0, 0, 0], [2, 0, 0, 0]], np.float32)
    ring = np.zeros(4, np.uint16)
    scan, index, plane, counts = G.organize(xyzw, ring, 2, 8, np.array([0.1, 0.2, 0.3, 0.4], np.float32))
    assert index[0] == 1 and (index[1:] == G.EMPTY).all()
    assert plane[0] == np.float32(0.2)
    assert counts == dict(placed=1, displaced=3, off_grid=0, invalid=0)
    # a ring table: ring 1 -> row 0, ring 0 dropped, ring 2 past the table
    _, index, _, counts = G.organize(xyzw, np.array([0, 1, 2, 1], np.uint16), 2, 8, ring_to_row=[-1, 0])
    assert index[0] == 1 and counts == dict(placed=1, displaced=1, off_grid=2, invalid=0)


def test_to_cloud_with_cell_fractions():
    scan, _, geo = synth.make_scan("tiny", 1)
    cellf = np.linspace(0, 1, geo.rows * geo.cols).astype(np.float32)
    a = synth.to_cloud(scan, geo, 5, cellf)
    b = synth.to_cloud(scan.numpy(), geo, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # seeded
    cell = a[1].astype(np.int64) * geo.cols + np.round(b[2].astype(np.float64) * geo.cols).astype(np.int64)
    assert np.array_equal(a[2], cellf[cell])
    assert a[1].dtype == np.uint16 and a[2].dtype == np.float32 and a[0].dtype == np.float32


def test_per_point_restatement_equals_the_per_column_one(oracle):
    import deskew_ref as D
    scan, _, geo = synth.make_scan_skewed("tiny", 1)
    scan = scan.numpy()
    xi = np.array([0.02, -0.015, 0.1, 1.5, 0.1, -0.05])
    tab = (np.arange(geo.cols) / geo.cols).astype(np.float32)
    tab[7] = 0.5  # a column that is copied
    want = D.deskew(oracle, scan, geo.rows, geo.cols, xi, tab)
    got = G.deskew_cells(oracle, scan, np.tile(tab, geo.rows), xi)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[:, :3] != scan[:, :3]).any()
    assert np.array_equal(G.deskew_cells(oracle, scan, np.tile(tab, geo.rows), np.zeros(6)), scan)


def test_organize_null_context_is_rejected():
    from form_amd import fmx
    L = fmx.lib()
    xi = (C.c_double * 6)()
    buf = (C.c_float * 16)()
    out = (C.c_float * 16)()
    fr = (C.c_float * 4)()
    p = fmx._OrganizeParams()
    cl = fmx._Cloud()
    assert L.fmx_organize_configure(None, C.byref(p)) == 1  # FMX_E_INVAL
    assert L.fmx_organize(None, C.byref(cl), None, C.c_int(0), None, None, None) == 1
    assert L.fmx_register_cloud(None, C.byref(cl), None, None) == 1
    assert L.fmx_deskew_cells(None, buf, C.c_size_t(4), C.c_int(0), fr, xi, out, C.c_int(0)) == 1


def test_set_organize_is_not_a_pipeline_key():
    from form_amd import fmx
    f = fmx.FORM()
    before = dict(f.get_params())
    f.set_organize(True, elevation=np.linspace(0.2, -0.2, 64), azimuth_offset=0.1, clockwise=True)
    assert f.get_params() == before == fmx.FORM.default_params()
    with pytest.raises(KeyError):
        f.set_params({"organize": True})

"""The carve restatement (tests/carve_ref.py) against itself: the voxel walk's invariants on
random and special rays, and the dynamic-object scenario that tests/test_gpu_carve.py runs on
the device.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import carve_ref as CR
import dense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_path(o, e, w):
    path = CR.walk(o, e, w)
    a = tuple(int(np.floor(np.float64(o[k]) / np.float64(w))) for k in range(3))
    b = tuple(int(np.floor(np.float64(e[k]) / np.float64(w))) for k in range(3))
    S = sum(abs(b[k] - a[k]) for k in range(3))
    assert path[0] == a and path[-1] == b and len(path) == S + 1
    for u, v in zip(path, path[1:]):
        assert sorted(abs(v[k] - u[k]) for k in range(3)) == [0, 0, 1]
    return path


def _box_meets_segment(v, o, e, w, slack=1e-9):
    """Slab test: the segment o + t (e - o), t in [0, 1], against the voxel's box grown by slack."""
    t0, t1 = 0.0, 1.0
    for k in range(3):
        lo, hi = v[k] * w - slack, (v[k] + 1) * w + slack
        d = e[k] - o[k]
        if d == 0.0:
            if not (lo <= o[k] <= hi):
                return False
            continue
        ta, tb = (lo - o[k]) / d, (hi - o[k]) / d
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return t0 <= t1


def test_random_rays_walk_from_a_to_b_through_voxels_the_segment_meets():
    g = np.random.default_rng(7)
    for i in range(400):
        w = float(g.choice([0.05, 0.2, 0.5, 1.0, 3.0]))
        o = g.normal(0, 5, 3)
        e = o + g.normal(0, 1, 3) * g.choice([0.01, 1.0, 10.0, 40.0])
        path = _check_path(o, e, w)
        for v in path:  # (random doubles: in general position)
            assert _box_meets_segment(v, o, e, w), (i, v)


def test_special_rays():
    lengths = {}
    for name, o, p in CR.SPECIAL:
        e = CR.special_end(o, p)
        assert np.array_equal(e, np.array(o) + np.array(p)), name  # exact by construction
        lengths[name] = len(_check_path(o, e, 1.0)) - 1
    assert lengths["same-voxel"] == 0 and lengths["+x"] == 5 and lengths["-z"] == 6
    assert lengths["tie"] == lengths["tie-mirror"] == 9 and lengths["face"] == 4 + 1 + 1
    # the exact tie takes x, y, z in turn
    path = CR.walk((0.5, 0.5, 0.5), (3.5, 3.5, 3.5), 1.0)
    axes = [[abs(v[k] - u[k]) for k in range(3)].index(1) for u, v in zip(path, path[1:])]
    assert axes == [0, 1, 2] * 3
    path = CR.walk((0.5, 0.5, 0.5), (-2.5, -2.5, -2.5), 1.0)
    axes = [[abs(v[k] - u[k]) for k in range(3)].index(1) for u, v in zip(path, path[1:])]
    assert axes == [0, 1, 2] * 3 and path[-1] == (-3, -3, -3)
    # an end exactly on a face belongs to the voxel it opens
    assert CR.walk((0.5, 0.25, 0.75), (4.0, 1.25, 1.25), 1.0)[-1] == (4, 1, 1)
    # axis-aligned: the two idle axes never move
    assert CR.walk((0.5, 0.5, 0.5), (-4.5, 0.5, 0.5), 1.0) == [(-k, 0, 0) for k in range(6)]
    # the long ray of the GPU test
    assert len(CR.walk((0.005, 0.005, 0.005), (20.005, 12.005, 8.005), 0.01)) == 4001


def test_examined_leaves_the_margin_alone():
    path = CR.walk((0.5, 0.5, 0.5), (5.5, 0.5, 0.5), 1.0)
    assert CR.examined(path, 0) == path[:-1] and CR.examined(path, 2) == path[:3]
    assert CR.examined(path, 5) == [] and CR.examined(path, 99) == []


def test_miss_filter_is_the_integer_rule():
    assert CR.miss_fraction(None) == (0, 0) and CR.miss_fraction(0.5) == (32768, 65536)
    assert CR.takes(4, 2, 1, *CR.miss_fraction(0.5)) and not CR.takes(4, 3, 1, *CR.miss_fraction(0.5))
    assert CR.takes(4, 1 << 31, 1, 0, 0) and not CR.takes(1, 0, 2, 0, 0) and CR.takes(3, 0, 0, *CR.miss_fraction(0.0))


def test_host_parts_under_the_sanitizers():
    """tests/cpp/test_carve_host (built by __graft_entry__.build(), tests/cpp/carve_host.mk):
    the parameter check, the origin's range rule and the spill's misses, with ASan and UBSan
    linked into the stand-alone program."""
    path = os.path.join(ROOT, "tests", "cpp", "test_carve_host")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f carve_host.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "carve host ok" in r.stdout, r.stdout + r.stderr[-3000:]


def scenario():
    ref = CR.CarveRef(CR.SCN_W, CR.SCN_CAP, 1.0, 1e4)
    ref.carve_configure(True, 0.0, 1, 1, 1)
    lasts = []
    for k in range(CR.SCN_SCANS):
        assert ref.integrate(CR.scenario_scan(k), np.eye(3, 4), k) is not None
        lasts.append(ref.carve_last)
    return ref, lasts


def test_dynamic_object_scenario():
    ref, lasts = scenario()
    obj = set(CR.scenario_object_keys(ref))
    assert len(obj) == 4
    for k, v in ref.vox.items():
        if k in obj:
            assert ref.misses.get(k, 0) >= 3, k
        else:  # the wall
            assert ref.misses.get(k, 0) == 0, k
    assert all(c[1] == 1 and c[0]["rays"] == 121 for c in lasts)
    assert lasts[0][0]["misses"] == 0 and lasts[0][0]["exempt"] > 0 and lasts[2][0]["misses"] > 0
    everything, kept = ref.sorted(), ref.sorted(1, 0.5)
    assert set(everything["key"].tolist()) - set(kept["key"].tolist()) == obj
    assert len(kept["key"]) == len(everything["key"]) - 4 and (kept["misses"] == 0).all()

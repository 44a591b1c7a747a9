"""Probing the dense voxel map without a device: the restatement (tests/probe_ref.py) against
the carve restatement's walk, an independent recomputation of the entering tau and a brute
force first hit; the dynamic-object scenario on the restatement alone; the header / library /
ctypes surface of the fmx_probe_* block; the host-only parts under the sanitizers."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import carve_ref as CR
import dense_ref as R
import probe_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SYMBOLS = ["fmx_probe_points", "fmx_probe_rays"]
I34 = np.eye(3, 4)


def _tau_alone(o, e, w, u, v):
    """The tau of the step from voxel u to its neighbour v, from the definition alone: the
    plane between them on the axis that moves, ((double)(plane index) * w - o_k) / d_k."""
    k = [abs(v[j] - u[j]) for j in range(3)].index(1)
    plane = max(u[k], v[k])  # stepping up crosses the upper face of u, down its lower face: both max(u, v)
    return (float(plane) * float(w) - float(o[k])) / (float(e[k]) - float(o[k]))


def _check_walk(o, e, w):
    path, tin = PR.walk_tau(o, e, w)
    assert path == CR.walk(o, e, w)
    assert len(tin) == len(path) and tin[0] == 0.0 and math.copysign(1.0, tin[0]) == 1.0
    for s in range(1, len(path)):
        want = _tau_alone(o, e, w, path[s - 1], path[s])
        assert np.float64(tin[s]).view(np.uint64) == np.float64(want).view(np.uint64), (s, tin[s], want)
    assert all(0.0 <= x <= 1.0 for x in tin) and tin == sorted(tin)  # entered in order along the segment
    return path, tin


def test_walk_is_the_carves_with_the_entering_tau_on_special_rays():
    for name, o, p in CR.SPECIAL:
        path, tin = _check_walk(o, CR.special_end(o, p), 1.0)
        if name == "same-voxel":
            assert len(path) == 1 and tin == [0.0]
        if name == "tie":
            assert tin[1:] == [1 / 6] * 3 + [0.5] * 3 + [5 / 6] * 3
        if name == "+x":
            assert tin == [0.0, 0.1, 0.3, 0.5, 0.7, 0.9]


def test_walk_is_the_carves_with_the_entering_tau_on_random_segments():
    g = np.random.default_rng(11)
    for _ in range(300):
        w = float(g.choice([0.05, 0.2, 0.5, 1.0, 3.0]))
        o = g.normal(0, 5, 3)
        e = o + g.normal(0, 1, 3) * g.choice([0.01, 1.0, 10.0, 40.0])
        _check_walk(o, e, w)


def test_first_hit_equals_a_brute_force_scan_of_the_path():
    g = np.random.default_rng(5)
    for trial in range(200):
        o = g.normal(0, 3, 3)
        e = o + g.normal(0, 6, 3)
        path, tin = PR.walk_tau(o, e, 1.0)
        ref = PR.ProbeRef(1.0, 4096, 1e-12, 1e12)
        T = CR.special_pose(o)
        on = [v for v in path if g.random() < 0.2]
        weak = set(v for v in on if g.random() < 0.3)  # one hit only: not solid under min_hits = 2
        if on:
            pts = CR.voxel_centres(on + [v for v in on if v not in weak], 1.0)
            ref.integrate(pts, I34, trial)
        p = np.zeros((1, 4), np.float32)
        p[0, :3] = (e - o).astype(np.float32)
        end = R.classify(p, T, 1.0, 1e-12, 1e12)[1][0]
        path, tin = PR.walk_tau(o, end, 1.0)  # (the fp32 point's own end)
        for skip, min_hits in ((0, 1), (1, 1), (0, 2), (3, 2), (len(path), 1)):
            solid = [s for s in range(len(path)) if s >= skip and R.pack_key(*path[s]) in ref.vox and
                     ref.vox[R.pack_key(*path[s])][0] >= min_hits]
            got = ref.probe_rays(p, T, min_hits, None, skip)
            if solid:
                s = solid[0]
                assert got["state"][0] == PR.SOLID and got["step"][0] == s and got["t"][0] == tin[s]
                assert got["counts"] == dict(hit=1, clear=0, out_of_range=0, invalid=0, steps=s - skip + 1)
                assert R.pack_key(*path[s]) == int(R.key_of_points(got["points"], 1.0)[0])
                assert got["hits"][0] == ref.vox[R.pack_key(*path[s])][0] and got["scan"][0] == trial
            else:
                assert got["state"][0] == PR.ABSENT and got["step"][0] == PR.NO_STEP and got["t"][0] == PR.INF
                assert got["counts"] == dict(hit=0, clear=1, out_of_range=0, invalid=0, steps=max(len(path) - skip, 0))
                assert not got["points"].any() and got["hits"][0] == 0 and got["scan"][0] == 0


def test_point_classes_and_lookup():
    ref = PR.ProbeRef(0.5, 4096, 1.0, 1e4)
    pts = np.array([[2.1, 0.3, 0.2, 0], [2.2, 0.3, 0.2, 0], [9.0, 9.0, 9.0, 0]], np.float32)
    ref.integrate(pts, I34, 77)
    q = np.array([[2.3, 0.4, 0.1, 0], [0.2, 0.1, 0.1, 0], [np.nan, 1, 1, 0], [0, 0, 0, 5], [1, np.inf, 1, 0],
                  [3e5, 1, 1, 0], [6e5, 1, 1, 0], [9.1, 9.2, 9.3, 0]], np.float32)
    got = ref.probe_points(q, I34)
    # 0.2, 0.1, 0.1 is inside the dense gate's minimum: the gate plays no part (absent, not gated)
    assert got["state"].tolist() == [2, 0, 4, 4, 4, 0, 3, 2]
    assert got["counts"] == dict(absent=2, filtered=0, solid=2, out_of_range=1, invalid=3)
    assert got["hits"].tolist() == [2, 0, 0, 0, 0, 0, 0, 1] and got["index"].tolist() == [0, 0, 0, 0, 0, 0, 0, 2]
    assert got["scan"].tolist() == [77, 0, 0, 0, 0, 0, 0, 77]
    assert np.array_equal(got["points"][0], pts[0, :3].astype(np.float64)) and not got["points"][1:7].any()
    two = ref.probe_points(q, I34, 2)
    assert two["state"].tolist() == [2, 0, 4, 4, 4, 0, 3, 1] and two["hits"].tolist() == got["hits"].tolist()
    assert two["counts"] == dict(absent=2, filtered=1, solid=1, out_of_range=1, invalid=3)
    with pytest.raises(ValueError):
        ref.probe_rays(q, CR.special_pose((0.5 * 1048575.0, 0, 0)))


def test_dynamic_object_scenario():
    ref = PR.scenario()
    before = (dict(ref.misses), {k: list(v[:3]) for k, v in ref.vox.items()})
    rays = CR.scenario_scan(CR.SCN_SCANS - 1)
    PR.check_scenario(lambda ratio: ref.probe_rays(rays, I34, 1, ratio))
    look = ref.probe_points(rays, I34, 1, 0.5)
    assert (look["state"] == PR.SOLID).all()  # the last scan's points are the wall's
    box = ref.probe_points(CR.scenario_scan(0)[PR.scenario_middle()], I34, 1, 0.5)
    assert (box["state"] == PR.FILTERED).all() and (box["misses"] >= 3).all()
    assert before == (dict(ref.misses), {k: list(v[:3]) for k, v in ref.vox.items()})  # read only


def _header():
    return open(os.path.join(ROOT, "include", "fmx", "fmx.h")).read()


def test_header_and_library_surface(tmp_path):
    """Fails without the feature: the header declares exactly the fmx_probe_* block, libfmx.so
    exports it, and the ctypes structs have the layout a compiler gives the header's."""
    hdr = _header()
    declared = sorted(s for s in set(re.findall(r"\b(fmx_[a-z_]+)\s*\(", hdr)) if s.startswith("fmx_probe_"))
    assert declared == PROBE_SYMBOLS
    from form_amd import fmx
    L = fmx.lib()
    assert all(hasattr(L, s) for s in PROBE_SYMBOLS)
    assert set(PROBE_SYMBOLS) <= set(fmx.EXPORTED)
    assert re.search(r"#define FMX_ABI_VERSION 1\b", hdr)
    cxx = shutil.which("g++")
    assert cxx, "the layout probe needs g++"
    src = tmp_path / "probe.cpp"
    pc = ["absent", "filtered", "solid", "out_of_range", "invalid"]
    rc = ["hit", "clear", "out_of_range", "invalid", "steps"]
    offs = [f"offsetof(fmx_probe_point_counts, {f})" for f in pc] + [f"offsetof(fmx_probe_ray_counts, {f})" for f in rc]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "fmx/fmx.h"\nint main() {\n'
                   '  const size_t v[] = {sizeof(fmx_probe_point_counts), sizeof(fmx_probe_ray_counts), '
                   + ", ".join(offs) + ',\n    FMX_PROBE_ABSENT, FMX_PROBE_FILTERED, FMX_PROBE_SOLID, '
                   'FMX_PROBE_OUT_OF_RANGE, FMX_PROBE_INVALID, FMX_PROBE_NO_STEP};\n'
                   '  for (size_t x : v) std::printf("%zu ", x);\n}\n')
    exe = tmp_path / "probe"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P, Q = fmx._ProbePointCounts, fmx._ProbeRayCounts
    assert got == [C.sizeof(P), C.sizeof(Q)] + [getattr(P, f).offset for f in pc] + [getattr(Q, f).offset for f in rc] + \
        [fmx.PROBE_ABSENT, fmx.PROBE_FILTERED, fmx.PROBE_SOLID, fmx.PROBE_OUT_OF_RANGE, fmx.PROBE_INVALID,
         fmx.PROBE_NO_STEP]
    assert [f for f, _ in P._fields_] == pc and [f for f, _ in Q._fields_] == rc
    assert (PR.ABSENT, PR.FILTERED, PR.SOLID, PR.OUT_OF_RANGE, PR.INVALID, PR.NO_STEP) == tuple(got[-6:])


def test_null_context_is_rejected():
    from form_amd import fmx
    L = fmx.lib()
    pts, pose = np.ones((2, 4), np.float32), np.ascontiguousarray(I34).reshape(12)
    state, step, t = np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2)
    pc, rc = fmx._ProbePointCounts(), fmx._ProbeRayCounts()
    f = (C.c_uint32(1), C.c_uint32(0), C.c_uint32(0))
    assert L.fmx_probe_points(None, fmx._p(pts), C.c_size_t(2), C.c_int(0), fmx._p(pose), *f, fmx._p(state), None,
                              C.byref(pc)) == 1  # FMX_E_INVAL
    assert L.fmx_probe_rays(None, fmx._p(pts), C.c_size_t(2), C.c_int(0), fmx._p(pose), *f, C.c_uint32(0), fmx._p(state),
                            fmx._p(step), fmx._p(t), None, C.byref(rc)) == 1
    assert L.fmx_probe_points(None, None, C.c_size_t(0), C.c_int(0), None, *f, None, None, None) == 1


def test_form_wrappers_need_the_dense_map():
    from form_amd import fmx
    f = fmx.FORM()
    for call in (f.dense_lookup, f.dense_cast):
        with pytest.raises(RuntimeError):
            call(np.ones((1, 3), np.float32))  # the dense map is off


def test_host_parts_under_the_sanitizers():
    """tests/cpp/test_probe_host (built by __graft_entry__.build(), tests/cpp/probe_host.mk):
    the argument checks, the origin rule and the tag resolution, with ASan and UBSan linked
    into the stand-alone program."""
    path = os.path.join(ROOT, "tests", "cpp", "test_probe_host")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f probe_host.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "probe host ok" in r.stdout, r.stdout + r.stderr[-3000:]

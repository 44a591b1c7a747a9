"""The nearest solid voxel of the dense map without a device: the restatement
(tests/nearest_ref.py) against an independent brute force over all voxels of a random map (the
radius-search guarantee), the tie and shell cases on the restatement alone, the header /
library / ctypes surface of fmx_nearest_voxels, and the host-only parts under the sanitizers."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dense_ref as R
import nearest_ref as NR
import probe_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)


def _pts(rows):
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return p


def _ref(w, reps, cap=4096):
    """A restatement whose representatives are the fp32 points `reps`, one integration each
    (so that none merges into another's voxel unnoticed)."""
    ref = NR.NearestRef(w, cap, *GATE)
    for k, r in enumerate(reps):
        assert ref.integrate(_pts([r]), I34, k)["added"] == 1
    return ref


def _all_voxels_nearest(ref, wp, r2, min_hits=1):
    """Independent of the cube: the smallest (d2, key) over every solid voxel of the map."""
    best = None
    for key, v in ref.vox.items():
        if v[0] < min_hits:
            continue
        e = [float(v[3][k]) - wp[k] for k in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        if d2 <= r2 and (best is None or (d2, key) < best):
            best = (d2, key)
    return best


@pytest.mark.parametrize("w", [1.0, 0.2])
def test_radius_search_equals_a_brute_force_over_all_voxels(w):
    g = np.random.default_rng(17)
    ref = NR.NearestRef(w, 4096, *GATE)
    cloud = _pts(g.uniform(-6 * w, 6 * w, (400, 3)))
    ref.integrate(cloud[:250], I34, 0)
    ref.integrate(cloud, I34, 1)  # the first 250 voxels: two hits or more
    q = _pts(g.uniform(-8 * w, 8 * w, (120, 3)))
    for r in (0.3 * w, 0.999 * w, w, 1.7 * w, 2.5 * w):
        reach = math.floor(r / w) + 1
        for min_hits in (1, 2):
            got = ref.nearest_voxels(q, I34, reach, r, min_hits)
            found = 0
            for i in range(len(q)):
                wp = [float(q[i, k]) for k in range(3)]  # the identity pose: exact
                want = _all_voxels_nearest(ref, wp, r * r, min_hits)
                if want is None:
                    assert got["state"][i] == PR.ABSENT and got["dist2"][i] == NR.INF, (r, i)
                    continue
                found += 1
                assert got["state"][i] == PR.SOLID and got["dist2"][i] == want[0], (r, i)
                assert int(R.key_of_points(got["points"][i], w)[0]) == want[1], (r, i)
            assert got["counts"]["found"] == found and got["counts"]["none"] == len(q) - found
            assert found > 0 or r < 0.5 * w
    # a reach too small for the radius is not a radius search: some answer must differ
    short = ref.nearest_voxels(q, I34, 1, 2.5 * w)
    full = ref.nearest_voxels(q, I34, 3, 2.5 * w)
    assert short["counts"]["found"] < full["counts"]["found"]


def test_a_nearer_voxel_in_a_farther_shell():
    ref = _ref(1.0, [(0.999, 1.7, 0.5), (2.0, 0.5, 0.5)])
    q = _pts([(0.999, 0.5, 0.5)])
    one, two = ref.nearest_voxels(q, I34, 1), ref.nearest_voxels(q, I34, 2)
    assert one["state"][0] == two["state"][0] == PR.SOLID
    assert one["index"][0] == 0 and one["scan"][0] == 0 and two["scan"][0] == 1
    assert two["dist2"][0] < one["dist2"][0] and 1.0 < two["dist2"][0] < 1.0041
    # the mirror: the best well inside shell 1, a decoy in shell 3
    ref = _ref(1.0, [(1.25, 0.5, 0.5), (3.5, 0.5, 0.5)])
    q = _pts([(0.5, 0.5, 0.5)])
    for reach in (1, 2, 3, 8):
        got = ref.nearest_voxels(q, I34, reach)
        assert got["scan"][0] == 0 and got["dist2"][0] == 0.5625, reach


def test_ties_go_to_the_smaller_key():
    ref = _ref(1.0, [(1.0, 1.75, 1.75), (0.5, 1.25, 2.25)])
    q = _pts([(0.25, 0.25, 0.25)])
    assert R.pack_key(0, 1, 2) < R.pack_key(1, 1, 1)
    got = ref.nearest_voxels(q, I34, 2)
    assert got["dist2"][0] == 81 / 16 and got["scan"][0] == 1  # cell (0, 1, 2): shell 2, visited later
    assert ref.nearest_voxels(q, I34, 1)["scan"][0] == 0       # shell 1 alone: cell (1, 1, 1)
    # inside one shell: two mirror images about the query
    ref = _ref(1.0, [(1.75, 0.5, 0.5), (-0.75, 0.5, 0.5)])
    got = ref.nearest_voxels(_pts([(0.5, 0.5, 0.5)]), I34, 1)
    assert got["dist2"][0] == 1.5625 and got["scan"][0] == 1  # cell (-1, 0, 0) has the smaller key


def test_limit_filter_classes_and_bounds():
    ref = NR.NearestRef(1.0, 4096, *GATE)
    ref.integrate(_pts([(1.5, 0.5, 0.5), (1.75, 0.25, 0.5), (0.5, 2.5, 0.5)]), I34, 0)  # two hits, one hit
    assert ref.voxels == 2
    q = _pts([(0.5, 0.5, 0.5), (np.nan, 0, 0), (0, 0, 0), (3e6, 0, 0)])
    got = ref.nearest_voxels(q, I34, 2)
    assert got["state"].tolist() == [PR.SOLID, PR.INVALID, PR.INVALID, PR.OUT_OF_RANGE]
    assert got["counts"] == dict(found=1, none=0, out_of_range=1, invalid=2) and got["lookups_bounds"] == (1, 125)
    assert got["hits"][0] == 2 and got["dist2"][0] == 1.0 and got["dist2"][1:].tolist() == [NR.INF] * 3
    assert ref.nearest_voxels(q, I34, 2, min_hits=3)["state"][0] == PR.ABSENT
    ref.integrate(_pts([(0.5, 2.25, 0.5)] * 3), I34, 1)  # the farther voxel: four hits now
    far = ref.nearest_voxels(q, I34, 2, min_hits=3)
    assert far["dist2"][0] == 4.0 and far["hits"][0] == 4 and far["scan"][0] == 0  # the nearer one is filtered
    for md2, state in ((np.nextafter(1.0, 0.0), PR.ABSENT), (1.0, PR.SOLID), (np.nextafter(1.0, 2.0), PR.SOLID)):
        assert ref.nearest_voxels(q[:1], I34, 1, max_dist2=md2)["state"][0] == state
    assert ref.nearest_voxels(_pts([(1.5, 0.5, 0.5)]), I34, 0, max_dist2=0.0)["dist2"][0] == 0.0
    assert ref.nearest_voxels(q[:1], I34, 0)["state"][0] == PR.ABSENT  # reach 0: the own voxel alone
    # the domain's edge: part of the cube cannot be stored
    edge = _pts([(float((1 << 20) - 2) + 0.5, 0.5, 0.5)])
    assert ref.nearest_voxels(edge, I34, 2)["lookups_bounds"] == (1, 3 * 5 * 5)
    for bad in (dict(reach=9), dict(max_dist2=-1.0), dict(max_dist2=float("nan"))):
        with pytest.raises(ValueError):
            ref.nearest_voxels(q, I34, **bad)


def test_fitness_restated():
    from form_amd import fmx
    st = np.array([PR.SOLID, PR.ABSENT, PR.INVALID, PR.SOLID, PR.OUT_OF_RANGE, PR.SOLID], np.uint8)
    d2 = np.array([0.25, NR.INF, NR.INF, 1e-30, NR.INF, 0.5])
    want = dict(n_valid=4, n_found=3, fitness=0.75, rmse=math.sqrt(math.fsum([0.25, 1e-30, 0.5]) / 3))
    assert fmx.fitness_of(st, d2) == want == NR.fitness(dict(state=st, dist2=d2))
    none = fmx.fitness_of(st[2:3], d2[2:3])
    assert none == dict(n_valid=0, n_found=0, fitness=0.0, rmse=0.0) == NR.fitness(dict(state=st[2:3], dist2=d2[2:3]))


def test_header_and_library_surface(tmp_path):
    """Fails without the feature: the header declares fmx_nearest_voxels, libfmx.so exports it,
    and the ctypes struct has the layout a compiler gives the header's."""
    hdr = open(os.path.join(ROOT, "include", "fmx", "fmx.h")).read()
    declared = sorted(s for s in set(re.findall(r"\b(fmx_[a-z_]+)\s*\(", hdr)) if s.startswith("fmx_nearest_"))
    assert declared == ["fmx_nearest_voxels"]
    from form_amd import fmx
    assert hasattr(fmx.lib(), "fmx_nearest_voxels") and "fmx_nearest_voxels" in fmx.EXPORTED
    assert re.search(r"#define FMX_ABI_VERSION 1\b", hdr)
    cxx = shutil.which("g++")
    assert cxx, "the layout probe needs g++"
    names = ["found", "none", "out_of_range", "invalid", "lookups"]
    src = tmp_path / "nearest.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "fmx/fmx.h"\nint main() {\n'
                   '  const size_t v[] = {sizeof(fmx_nearest_counts), '
                   + ", ".join(f"offsetof(fmx_nearest_counts, {f})" for f in names) + ', FMX_NEAREST_MAX_REACH};\n'
                   '  for (size_t x : v) std::printf("%zu ", x);\n}\n')
    exe = tmp_path / "nearest"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    N = fmx._NearestCounts
    assert got == [C.sizeof(N)] + [getattr(N, f).offset for f in names] + [fmx.NEAREST_MAX_REACH]
    assert [f for f, _ in N._fields_] == names and NR.MAX_REACH == fmx.NEAREST_MAX_REACH


def test_null_context_is_rejected():
    from form_amd import fmx
    L = fmx.lib()
    pts, pose = np.ones((2, 4), np.float32), np.ascontiguousarray(I34).reshape(12)
    state, d2, cnt = np.zeros(2, np.uint8), np.zeros(2), fmx._NearestCounts()
    f = (C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), C.c_uint32(1), C.c_double(1.0))
    assert L.fmx_nearest_voxels(None, fmx._p(pts), C.c_size_t(2), C.c_int(0), fmx._p(pose), *f, fmx._p(state), fmx._p(d2),
                                None, C.byref(cnt)) == 1  # FMX_E_INVAL
    assert L.fmx_nearest_voxels(None, None, C.c_size_t(0), C.c_int(0), None, *f, None, None, None, None) == 1


def test_form_wrappers_need_the_dense_map():
    from form_amd import fmx
    f = fmx.FORM()
    for call in (f.dense_nearest, f.dense_fitness):
        with pytest.raises(RuntimeError):
            call(np.ones((1, 3), np.float32), 0.5)  # the dense map is off


def test_host_parts_under_the_sanitizers():
    """tests/cpp/test_nearest_host (built by __graft_entry__.build(), tests/cpp/nearest_host.mk):
    the argument checks, the offset list and the cube's cell count, with ASan and UBSan linked
    into the stand-alone program."""
    path = os.path.join(ROOT, "tests", "cpp", "test_nearest_host")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f nearest_host.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "nearest host ok" in r.stdout, r.stdout + r.stderr[-3000:]

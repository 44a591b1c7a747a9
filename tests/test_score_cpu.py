"""Scoring many candidate poses against the dense map without a device: the header / library /
ctypes surface of fmx_score_poses and fmx_score_plan, the plan against its restatement, the
restatement (tests/score_ref.py) against a brute force over every voxel of a small map, the
ranking rule and the ranking fixture's design, the candidate grid, and the host-only parts
under the sanitizers."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import nearest_ref as NR
import probe_ref as PR
import score_cases as SC
import score_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
INVAL = 1


def _pts(rows):
    p = np.zeros((len(rows), 4), np.float32)
    p[:, :3] = np.asarray(rows, np.float32).reshape(-1, 3)
    return p


def test_header_and_library_surface(tmp_path):
    """Fails without the feature: a C caller names both entry points, the record's size and
    FMX_SCORE_MAX_POSES; libfmx.so exports the symbols; the ctypes struct and the numpy dtype
    have the layout a compiler gives the header's."""
    hdr = open(os.path.join(ROOT, "include", "fmx", "fmx.h")).read()
    declared = sorted(s for s in set(re.findall(r"\b(fmx_[a-z_]+)\s*\(", hdr)) if s.startswith("fmx_score_"))
    assert declared == ["fmx_score_plan", "fmx_score_poses"]
    from form_amd import fmx
    L = fmx.lib()
    assert all(hasattr(L, s) and s in fmx.EXPORTED for s in declared)
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "the C caller needs a C compiler"
    fields = [f for f, _ in fmx._PoseScore._fields_]
    assert fields == ["found", "none", "out_of_range", "invalid", "sum_d2", "lookups"] == list(fmx.SCORE_FIELDS)
    probe = ["sizeof(fmx_pose_score)", "FMX_SCORE_MAX_POSES"] + [f"offsetof(fmx_pose_score, {f})" for f in fields]
    src = tmp_path / "score.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmx/fmx.h"\n#ifndef SIZES\n'
                   "fmx_status (*poses)(fmx_ctx*, const float*, size_t, int, const double*, uint32_t, const fmx_align_params*,"
                   " fmx_pose_score*) = fmx_score_poses;\n"
                   "fmx_status (*plan)(uint64_t, uint32_t, uint32_t, uint32_t*) = fmx_score_plan;\n"
                   "#else\nint main(void) {\n  const size_t v[] = {" + ", ".join(probe) + "};\n"
                   '  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);\n  return 0;\n}\n#endif\n')
    inc = ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    # the caller of both functions compiles against the header (the library's symbols are checked above)
    subprocess.run([cc, *inc, "-c", str(src), "-o", str(tmp_path / "score.o")], check=True)
    exe = tmp_path / "score"
    subprocess.run([cc, *inc, "-DSIZES", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [32, 65536] + [getattr(fmx._PoseScore, f).offset for f in fields]
    assert got == want and C.sizeof(fmx._PoseScore) == 32 == fmx.SCORE_DTYPE.itemsize
    assert [fmx.SCORE_DTYPE.fields[f][1] for f in fields] == want[2:]
    assert fmx.SCORE_MAX_POSES == 65536 == SR.MAX_POSES


def test_null_context_and_null_plan_are_rejected():
    from form_amd import fmx
    L = fmx.lib()
    pts, poses = np.ones((2, 4), np.float32), np.ascontiguousarray(I34).reshape(1, 12)
    prm, rec = fmx._AlignParams(1, 0, 0, 1, 1.0, 0.1, 1), np.full(1, 7, fmx.SCORE_DTYPE)
    before = rec.tobytes()
    assert L.fmx_score_poses(None, fmx._p(pts), C.c_size_t(2), C.c_int(0), fmx._p(poses), C.c_uint32(1), C.byref(prm),
                             fmx._p(rec)) == INVAL
    assert rec.tobytes() == before
    assert L.fmx_score_plan(C.c_uint64(5), C.c_uint32(1), C.c_uint32(1), None) == INVAL


def test_form_wrappers_need_the_dense_map():
    from form_amd import fmx
    with pytest.raises(RuntimeError):
        fmx.FORM().dense_score(np.ones((1, 3), np.float32), [I34], 0.5)  # the dense map is off
    with pytest.raises(RuntimeError):
        fmx.FORM().dense_relocalize(np.ones((1, 3), np.float32), 0.5, [I34])


def test_plan_equals_its_restatement():
    from form_amd import fmx
    L = fmx.lib()
    base = fmx.score_plan(1, 1, 1)
    tile, chunk, cap = base["tile"], base["chunk"], base["cap"]
    assert (tile, chunk, cap) == (SR.TILE, SR.CHUNK_POSES, SR.CAP)
    ns = [0, 1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 3 * tile + 5, 64 * tile + 1, 4096 * 64, 1 << 24,
          (1 << 28) + 3, (1 << 32) - 1]
    for n in ns:
        for stride in (0, 1, 3, 64):
            for k in (0, 1, chunk, chunk + 1, 65536):
                got, want = fmx.score_plan(n, stride, k), SR.score_plan(n, stride, k)
                assert got == want, (n, stride, k, got, want)
                assert got["kept"] == len(range(0, n, max(stride, 1)))
                assert got["chunk"] >= 1 and (got["chunks"] == 0) == (got["kept"] == 0 or k == 0)
    assert fmx.score_plan(1 << 24, 1, 100)["chunk"] == (32 << 20) // 32 // ((1 << 24) // tile) < chunk
    out = np.full(6, 9, np.uint32)
    assert L.fmx_score_plan(C.c_uint64(5), C.c_uint32(1), C.c_uint32(65537), fmx._p(out)) == INVAL
    assert L.fmx_score_plan(C.c_uint64(1 << 32), C.c_uint32(1), C.c_uint32(1), fmx._p(out)) == INVAL
    assert (out == 9).all()
    with pytest.raises(ValueError):
        SR.score_plan(5, 1, 65537)
    with pytest.raises(ValueError):
        SR.score_plan(1 << 32, 1, 1)


def _brute(ref, sub, T, radius, min_hits=1):
    """Counts and the exact sum over every voxel of the map, without the cube."""
    cnt, d2s = dict.fromkeys(SR.CLASSES, 0), []
    Tl = np.asarray(T, np.float64).reshape(3, 4).tolist()
    for p in sub:
        cls, wp, _ = PR.classify_point(p, Tl, ref.w)
        if cls is not None:
            cnt["invalid" if cls == PR.INVALID else "out_of_range"] += 1
            continue
        best = None
        for key, v in ref.vox.items():
            if not ref._solid(key, min_hits, 0, 0):
                continue
            q = v[3]
            e0, e1, e2 = float(q[0]) - wp[0], float(q[1]) - wp[1], float(q[2]) - wp[2]
            d2 = (e0 * e0 + e1 * e1) + e2 * e2
            if d2 <= radius * radius and (best is None or (d2, key) < best):
                best = (d2, key)
        cnt["found" if best else "none"] += 1
        if best:
            d2s.append(best[0])
    return cnt, math.fsum(d2s)


def test_the_restatement_equals_a_brute_force_over_all_voxels():
    g = np.random.default_rng(5)
    ref = NR.NearestRef(0.5, 2048, *GATE)
    ref.integrate(_pts(g.uniform(-2.0, 2.0, (150, 3))), I34, 0)
    ref.integrate(_pts(g.uniform(-2.0, 2.0, (60, 3))), I34, 1)  # some voxels with two hits
    q = _pts(g.uniform(-2.5, 2.5, (41, 3)))
    q[7, 1], q[20, :3] = np.nan, 0.0
    poses = [I34, np.hstack([np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), [[0.3], [-0.2], [0.1]]]),
             np.hstack([np.eye(3), [[1e9], [0.0], [0.0]]])]
    found = {1: 0, 2: 0}
    for radius in (0.3, 0.75, 1.2):
        reach = math.floor(radius / 0.5) + 1  # an exact radius search
        for stride in (1, 3):
            for min_hits in (1, 2):
                got = SR.score_poses(ref, q, poses, stride, reach=reach, max_dist=radius, min_hits=min_hits)
                for k, T in enumerate(poses):
                    cnt, total = _brute(ref, q[::stride], T, radius, min_hits)
                    assert {c: int(got[c][k]) for c in SR.CLASSES} == cnt and got["sum_d2"][k] == total, (radius, stride, k)
                    assert sum(cnt.values()) == len(q[::stride])
                found[min_hits] += int(got["found"][0])
                assert got["out_of_range"][2] == len(q[::stride]) - 2 // stride  # (the invalid two are off the stride of 3)
                assert got["sum_d2"][2] == 0.0 and got["lookups_lo"][0] <= got["lookups_hi"][0]
    assert found[1] > found[2] > 0  # the filter bites, and leaves something


def test_rank_scores_orders_by_found_then_sum_then_index():
    from form_amd import fmx
    s = dict(found=np.array([3, 5, 5, 5, 0, 5], np.uint32), sum_d2=np.array([0.5, 2.0, 1.0, 1.0, 0.0, 0.25]))
    assert list(fmx.rank_scores(s)) == SR.rank_scores(s) == [5, 2, 3, 1, 0, 4]
    g = np.random.default_rng(3)
    s = dict(found=g.integers(0, 4, 200).astype(np.uint32), sum_d2=g.integers(0, 3, 200) * 0.5)
    assert list(fmx.rank_scores(s)) == SR.rank_scores(s)
    assert list(fmx.rank_scores(dict(found=np.zeros(0, np.uint32), sum_d2=np.zeros(0)))) == []


def test_the_ranking_fixture_realizes_its_design():
    """On the restatement, so that the GPU test cannot pass by a tie: the truth ranks first with
    a strictly larger `found` than every other candidate, and finds every point."""
    world, scan, cands, truth = SC.ranking_fixture()
    ref = NR.NearestRef(SC.WIDTH, SC.CAPACITY, *GATE)
    counts = ref.integrate(world, I34, 0)
    assert counts["added"] == len(world) and counts["merged"] == 0  # every point is a representative
    reach = math.floor(SC.RADIUS / SC.WIDTH) + 1
    s = SR.score_poses(ref, scan, cands, 1, reach=reach, max_dist=SC.RADIUS)
    rank = SR.rank_scores(s)
    assert rank[0] == truth != 0 and s["found"][truth] == len(scan)
    others = np.delete(s["found"], truth)
    assert (others < s["found"][truth]).all() and others.max() > 0  # beaten, not absent
    assert s["sum_d2"][truth] < 1e-9 * len(scan)


def test_pose_grid_nesting_centre_and_limit():
    from form_amd import fmx
    Tc = np.hstack([np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), [[1.0], [2.0], [3.0]]])
    g = fmx.pose_grid(Tc, (1.0, 0.5, 0.0), (0.5, 0.5, 1.0), 0.2, 0.1)
    assert g.shape == (5 * 5 * 3 * 1, 3, 4)
    centre = [k for k in range(len(g)) if g[k].tobytes() == Tc.tobytes()]
    assert centre == [len(g) // 2]  # the centre, bit for bit, once
    # nesting, outermost first: yaw, x, y, z
    assert np.array_equal(g[0, :, 3], [0.0, 1.5, 3.0]) and np.array_equal(g[1, :, 3], [0.0, 2.0, 3.0])
    assert np.array_equal(g[3, :, 3], [0.5, 1.5, 3.0]) and np.array_equal(g[0, :, :3], g[14, :, :3])
    assert not np.array_equal(g[14, :, :3], g[15, :, :3])
    c, s = math.cos(-0.2), math.sin(-0.2)
    assert np.allclose(g[0, :, :3], np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ Tc[:, :3], rtol=0, atol=1e-15)
    assert fmx.pose_grid(np.eye(4), (0, 0, 0), (1, 1, 1)).shape == (1, 3, 4)
    assert len(fmx.pose_grid(I34, (12.7, 12.7, 0), (0.1, 0.1, 1))) == 255 * 255  # 65025: within the limit
    with pytest.raises(ValueError):
        fmx.pose_grid(I34, (12.8, 12.8, 0), (0.1, 0.1, 1))  # 257 x 257
    with pytest.raises(ValueError):
        fmx.pose_grid(I34, (math.inf, 0, 0), (1, 1, 1))


def test_host_parts_under_the_sanitizers():
    """tests/cpp/test_score_host (built by __graft_entry__.build(), tests/cpp/score_host.mk): the
    argument checks, the plan and the ranking rule, with ASan and UBSan linked into the
    stand-alone program.  Nothing is loaded into Python under a sanitizer."""
    path = os.path.join(ROOT, "tests", "cpp", "test_score_host")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f score_host.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "score host ok" in r.stdout, r.stdout + r.stderr[-3000:]

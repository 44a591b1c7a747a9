"""Refining many candidate poses against the dense map without a device: the header / library /
ctypes surface of fmx_refine_systems, fmx_refine_poses and fmx_refine_plan, the plan against its
restatement, the host-only parts under the sanitizers, and the restated lockstep loop
(tests/refine_ref.py) on the two zero-residual fixtures from the starts the GPU loop test uses."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import align_ref as AR
import nearest_ref as NR
import normals_ref as MR
import plane_ref as PL
import refine_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = np.eye(3, 4)
GATE = (1e-12, 1e12)
INVAL = 1

SYSTEM_FIELDS = ["S", "found", "none", "out_of_range", "invalid", "unoriented", "reserved", "lookups"]
RESULT_FIELDS = ["iters", "converged", "singular", "reserved", "last_step", "error", "found", "none", "out_of_range",
                 "invalid", "unoriented", "reserved2", "lookups"]


def test_header_and_library_surface(tmp_path):
    """Fails without the feature: a C caller names the three entry points, both records' sizes
    and FMX_REFINE_MAX_POSES; libfmx.so exports the symbols; the ctypes structs and the numpy
    dtypes have the layout a compiler gives the header's."""
    hdr = open(os.path.join(ROOT, "include", "fmx", "fmx.h")).read()
    declared = sorted(s for s in set(re.findall(r"\b(fmx_[a-z_]+)\s*\(", hdr)) if s.startswith("fmx_refine_"))
    assert declared == ["fmx_refine_plan", "fmx_refine_poses", "fmx_refine_systems"]
    from form_amd import fmx
    L = fmx.lib()
    assert all(hasattr(L, s) and s in fmx.EXPORTED for s in declared)
    assert L.fmx_abi_version() == 1
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "the C caller needs a C compiler"
    assert [f for f, _ in fmx._RefineSystem._fields_] == SYSTEM_FIELDS
    assert [f for f, _ in fmx._RefineResult._fields_] == RESULT_FIELDS
    probe = (["sizeof(fmx_refine_system)", "sizeof(fmx_refine_result)", "FMX_REFINE_MAX_POSES"] +
             [f"offsetof(fmx_refine_system, {f})" for f in SYSTEM_FIELDS] +
             [f"offsetof(fmx_refine_result, {f})" for f in RESULT_FIELDS])
    src = tmp_path / "refine.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmx/fmx.h"\n#ifndef SIZES\n'
                   "fmx_status (*systems)(fmx_ctx*, const float*, size_t, int, const double*, uint32_t, const fmx_align_params*,"
                   " int, fmx_refine_system*) = fmx_refine_systems;\n"
                   "fmx_status (*poses)(fmx_ctx*, const float*, size_t, int, const double*, uint32_t, const fmx_align_params*,"
                   " int, uint32_t, double, double*, fmx_refine_result*) = fmx_refine_poses;\n"
                   "fmx_status (*plan)(uint64_t, uint32_t, uint32_t, uint32_t*) = fmx_refine_plan;\n"
                   "#else\nint main(void) {\n  const size_t v[] = {" + ", ".join(probe) + "};\n"
                   '  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);\n  return 0;\n}\n#endif\n')
    inc = ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    subprocess.run([cc, *inc, "-c", str(src), "-o", str(tmp_path / "refine.o")], check=True)
    exe = tmp_path / "refine"
    subprocess.run([cc, *inc, "-DSIZES", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = ([264, 64, 65536] + [getattr(fmx._RefineSystem, f).offset for f in SYSTEM_FIELDS] +
            [getattr(fmx._RefineResult, f).offset for f in RESULT_FIELDS])
    assert got == want
    assert C.sizeof(fmx._RefineSystem) == 264 == fmx.REFINE_SYSTEM_DTYPE.itemsize
    assert C.sizeof(fmx._RefineResult) == 64 == fmx.REFINE_RESULT_DTYPE.itemsize
    names = ["system" if f == "S" else f for f in SYSTEM_FIELDS]
    assert list(fmx.REFINE_SYSTEM_DTYPE.names) == names and list(fmx.REFINE_RESULT_DTYPE.names) == RESULT_FIELDS
    assert [fmx.REFINE_SYSTEM_DTYPE.fields[f][1] for f in names] == want[3:3 + len(names)]
    assert [fmx.REFINE_RESULT_DTYPE.fields[f][1] for f in RESULT_FIELDS] == want[3 + len(names):]
    assert fmx.REFINE_SYSTEM_DTYPE["system"].shape == (29,)
    assert fmx.REFINE_MAX_POSES == 65536 == RR.MAX_POSES


def test_null_context_and_null_plan_are_rejected():
    from form_amd import fmx
    L = fmx.lib()
    pts, poses = np.ones((2, 4), np.float32), np.ascontiguousarray(I34).reshape(1, 12)
    prm = fmx._AlignParams(1, 0, 0, 1, 1.0, 0.1, 1)
    rec, out, res = np.full(1, 7, fmx.REFINE_SYSTEM_DTYPE), np.full(12, 7.0), np.full(1, 7, fmx.REFINE_RESULT_DTYPE)
    before = rec.tobytes(), out.tobytes(), res.tobytes()
    for plane in (0, 1):
        assert L.fmx_refine_systems(None, fmx._p(pts), C.c_size_t(2), C.c_int(0), fmx._p(poses), C.c_uint32(1), C.byref(prm),
                                    C.c_int(plane), fmx._p(rec)) == INVAL
        assert L.fmx_refine_poses(None, fmx._p(pts), C.c_size_t(2), C.c_int(0), fmx._p(poses), C.c_uint32(1), C.byref(prm),
                                  C.c_int(plane), C.c_uint32(3), C.c_double(1e-6), fmx._p(out), fmx._p(res)) == INVAL
    assert (rec.tobytes(), out.tobytes(), res.tobytes()) == before
    assert L.fmx_refine_plan(C.c_uint64(5), C.c_uint32(1), C.c_uint32(1), None) == INVAL


def test_form_wrappers_need_the_dense_map():
    from form_amd import fmx
    with pytest.raises(RuntimeError):
        fmx.FORM().dense_localize_many(np.ones((1, 3), np.float32), 0.5, [I34])  # the dense map is off
    with pytest.raises(RuntimeError):
        fmx.FORM().dense_relocalize(np.ones((1, 3), np.float32), 0.5, [I34], batched=True)


def test_plan_equals_its_restatement():
    from form_amd import fmx
    L = fmx.lib()
    base = fmx.refine_plan(1, 1, 1)
    tile, chunk, cap = base["tile"], base["chunk"], base["cap"]
    assert (tile, chunk, cap) == (RR.TILE, RR.CHUNK_POSES, RR.CAP) and tile % 256 == 0
    ns = [0, 1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 3 * tile + 5, 8 * tile, 8 * tile + 1, 64 * tile + 1,
          4096 * 64, 1 << 24, (1 << 28) + 3, (1 << 32) - 1]
    for n in ns:
        for stride in (0, 1, 3, 64):
            for k in (0, 1, chunk, chunk + 1, 65536):
                got, want = fmx.refine_plan(n, stride, k), RR.refine_plan(n, stride, k)
                assert got == want, (n, stride, k, got, want)
                assert got["kept"] == len(range(0, n, max(stride, 1)))
                assert got["chunk"] >= 1 and (got["chunks"] == 0) == (got["kept"] == 0 or k == 0)
    assert fmx.refine_plan(1 << 24, 1, 100)["chunk"] == (32 << 20) // 256 // ((1 << 24) // tile) < chunk
    out = np.full(6, 9, np.uint32)
    assert L.fmx_refine_plan(C.c_uint64(5), C.c_uint32(1), C.c_uint32(65537), fmx._p(out)) == INVAL
    assert L.fmx_refine_plan(C.c_uint64(1 << 32), C.c_uint32(1), C.c_uint32(1), fmx._p(out)) == INVAL
    assert (out == 9).all()
    with pytest.raises(ValueError):
        RR.refine_plan(5, 1, 65537)
    with pytest.raises(ValueError):
        RR.refine_plan(1 << 32, 1, 1)


def test_host_parts_under_the_sanitizers():
    """tests/cpp/test_refine_host (built by __graft_entry__.build(), tests/cpp/refine_host.mk): the
    argument checks, the plan and the lockstep loop against align_loop_as, with ASan and UBSan
    linked into the stand-alone program.  Nothing is loaded into Python under a sanitizer."""
    path = os.path.join(ROOT, "tests", "cpp", "test_refine_host")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f refine_host.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "refine host ok" in r.stdout, r.stdout + r.stderr[-3000:]


def _starts(xi):
    return [AR.expmap([s * x for x in xi]) for s in (1.0, 0.5, 0.0)]


def _loop_on(ref, p, starts, threshold, normal_at=None):
    def systems_at(poses):
        got = RR.systems(ref, p, poses, sigma=0.1, normal_at=normal_at, reach=1)
        return [(got["system"][k], {c: int(got[c][k]) for c in RR.CLASSES}) for k in range(len(poses))]

    return RR.refine_poses(systems_at, starts, 30, threshold), systems_at


@pytest.mark.parametrize("form", ["point", "plane"])
def test_the_restated_loop_converges_from_every_start_of_the_gpu_test(form):
    """The precondition tests/test_gpu_refine.py's loop test relies on, on the CPU: from Exp(s
    ZERO_XI), s in {1, 0.5, 0}, the restated lockstep loop converges to the identity under the
    fixture's own threshold; each pose's record is what the one-pose loop (align_ref.align)
    gives, and the batches shrink as poses finish."""
    if form == "point":
        p, _ = AR.zero_residual_cloud()
        ref, normal_at, xi, thr = NR.NearestRef(AR.ZERO_W, 2048, *GATE), None, AR.ZERO_XI, AR.ZERO_THRESHOLD
        assert ref.integrate(p, I34, 0)["merged"] == 0
    else:
        p, _ = PL.zero_residual_cloud()
        ref, xi, thr = NR.NearestRef(1.0, 2048, *GATE), PL.ZERO_XI, PL.ZERO_THRESHOLD
        assert ref.integrate(p, I34, 0)["merged"] == 0
        normal_at = PL.by_owner_of(ref, MR.build(ref, **PL.ZERO_BUILD))
    starts = _starts(xi)
    assert np.array_equal(starts[2], I34)
    got, systems_at = _loop_on(ref, p, starts, thr, normal_at)
    for k in range(3):
        assert got["converged"][k] and not got["singular"][k] and got["last_step"][k] < thr, k
        assert np.abs(got["pose"][k] - I34).max() < 1e-6, k
        alone = AR.align(lambda T: systems_at([T])[0], starts[k], 30, thr)
        assert alone["iters"] == got["iters"][k] and alone["pose"].tobytes() == got["pose"][k].tobytes()
        assert alone["last_step"] == got["last_step"][k] and alone["error"] == got["error"][k]
        assert alone["counts"] == got["counts"][k]
    assert got["iters"][2] == 1 and got["last_step"][2] == 0.0  # the identity is the solution: one evaluation
    assert got["rounds"][0] == 3 and got["rounds"] == sorted(got["rounds"], reverse=True) and len(got["rounds"]) == max(got["iters"])
    # max_iters = 0 and 1, and a pose with nothing in reach among the others
    none = RR.refine_poses(systems_at, starts, 0, thr)
    assert none["rounds"] == [] and all(a.tobytes() == b.tobytes() for a, b in zip(none["pose"], starts))
    lost = starts[0].copy()
    lost[:, 3] += 500.0
    mixed = RR.refine_poses(systems_at, [starts[0], lost, starts[1]], 30, thr)
    assert mixed["singular"] == [False, True, False] and mixed["iters"][1] == 1 and mixed["pose"][1].tobytes() == lost.tobytes()
    for j, k in ((0, 0), (2, 1)):
        assert mixed["pose"][j].tobytes() == got["pose"][k].tobytes() and mixed["iters"][j] == got["iters"][k]

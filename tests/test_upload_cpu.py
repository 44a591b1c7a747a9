"""Loading voxels back into the dense voxel map without a device: the restatement
(tests/upload_ref.py) against an independent recomputation that groups the entries by voxel;
the integration count kept apart from the owner numbering; the header / library / ctypes
surface of fmx_upload_voxels; the host-only parts under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import carve_ref as CR
import dense_ref as R
import upload_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I34 = np.eye(3, 4)


def _entries(g, n, w, dup=0.4):
    """n random entries: duplicates of earlier voxels, invalid and out-of-range ones among them."""
    p = g.normal(0, 6, (n, 3))
    for i in range(1, n):
        if g.random() < dup:
            p[i] = (np.floor(p[g.integers(0, i)] / w) + g.random(3) * 0.98 + 0.01) * w  # another point of that voxel
    scan = g.choice(np.array([0, 3, 1 << 33, (1 << 64) - 1], np.uint64), n)
    index = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    hits = g.integers(0, 5, n).astype(np.uint32)  # some 0: invalid
    misses = g.integers(0, 4, n).astype(np.uint32)
    bad = g.choice(n, max(n // 10, 1), replace=False)
    for j, i in enumerate(bad):
        p[i, j % 3] = (np.nan, np.inf, -np.inf, 1e9, -1e9)[j % 5]
    return p, scan, index, hits, misses


def _grouped(before, p, scan, index, hits, misses, w):
    """The map after the upload from the definition alone: the entries grouped by voxel with
    numpy (no pass in input order).  before: key -> (hits, misses, scan, index, point)."""
    fin = np.isfinite(p).all(1)
    dead = (hits == 0) if hits is not None else np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        c = np.floor(p / w)
    inr = (np.abs(c) < 1048575.0).all(1)
    valid = fin & ~dead & inr
    counts = dict(invalid=int((~fin | dead).sum()), out_of_range=int((fin & ~dead & ~inr).sum()))
    after = {k: list(v) for k, v in before.items()}
    cv = c[valid].astype(np.int64)
    pos = np.flatnonzero(valid)
    uniq, inv = np.unique(cv, axis=0, return_inverse=True) if len(cv) else (cv, np.zeros(0, np.int64))
    inv = inv.reshape(-1)
    added = 0
    for u in range(len(uniq)):
        members = pos[inv == u]
        key = R.pack_key(*[int(x) for x in uniq[u]])
        h = int(sum(int(hits[i]) if hits is not None else 1 for i in members)) & UR.M32
        m = int(sum(int(misses[i]) if misses is not None else 0 for i in members)) & UR.M32
        if key in after:
            after[key][0] = (after[key][0] + h) & UR.M32
            after[key][1] = (after[key][1] + m) & UR.M32
        else:
            f = int(members.min())
            after[key] = [h, m, int(scan[f]) if scan is not None else 0, int(index[f]) if index is not None else 0, p[f].copy()]
            added += 1
    counts.update(added=added, merged=int(valid.sum()) - added)
    return after, counts


def _state(ref):
    return {k: (v[0], ref.misses.get(k, 0), ref.seq_scan[v[1]], v[2], v[3]) for k, v in ref.vox.items()}


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert tuple(a[k][:4]) == tuple(b[k][:4]), (k, a[k], b[k])
        assert np.array_equal(np.asarray(a[k][4]).view(np.uint64), np.asarray(b[k][4]).view(np.uint64)), k


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_grouped_recomputation(seed):
    g = np.random.default_rng(seed)
    w = float(g.choice([0.2, 0.5, 1.0]))
    ref = UR.UploadRef(w, 1 << 12, 1e-6, 1e12)
    ref.carve_configure(True, 0.0, 1, 1, 1)
    pts = np.zeros((60, 4), np.float32)
    pts[:, :3] = g.normal(0, 6, (60, 3))
    ref.integrate(pts, I34, 77)  # resident voxels, some of which the entries hit
    for call in range(3):
        p, scan, index, hits, misses = _entries(g, int(g.integers(1, 300)), w)
        opt = [a if g.random() < 0.7 else None for a in (scan, index, hits, misses)]
        before = _state(ref)
        want, counts = _grouped(before, p, *opt, w)
        assert ref.upload(p, *opt) == counts
        _same_state(_state(ref), want)
        assert sum(counts.values()) == len(p) and ref.integrations == 1
    assert ref.voxels == len(ref.vox)


def test_world_origin_is_valid_and_the_first_position_wins():
    ref = UR.UploadRef(1.0, 64)
    p = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [-0.0, 5.5, 0.0]])
    got = ref.upload(p, scan=[9, 8, 7, 1 << 40], index=[5, 6, 7, 0xFFFFFFFF], hits=[2, 3, 4, 1])
    assert got == dict(added=2, merged=2, out_of_range=0, invalid=0)
    v = ref.vox[R.pack_key(0, 0, 0)]
    assert v[0] == 9 and ref.seq_scan[v[1]] == 9 and v[2] == 5 and np.array_equal(v[3], [0.0, 0.0, 0.0])
    d = ref.sorted()
    assert d["scan"].tolist() == [9, 1 << 40] and d["index"].tolist() == [5, 0xFFFFFFFF] and d["hits"].tolist() == [9, 1]
    # a resident voxel keeps its representative whatever comes
    again = ref.upload(p[1:2], scan=[123], index=[1], hits=[10])
    assert again == dict(added=0, merged=1, out_of_range=0, invalid=0)
    assert ref.sorted()["scan"].tolist() == [9, 1 << 40] and ref.sorted()["hits"].tolist() == [19, 1]


def test_capacity_misses_and_no_entries():
    ref = UR.UploadRef(1.0, 4)
    with pytest.raises(ValueError):
        ref.upload(np.ones((1, 3)), misses=[1])  # carving never enabled
    with pytest.raises(ValueError):
        ref.upload(np.zeros((0, 3)), misses=[])
    p = np.arange(15, dtype=np.float64).reshape(5, 3)
    assert ref.upload(p) is None and ref.voxels == 0 and ref.seq_scan == []  # 0 + 5 > 4
    assert ref.upload(p[:4]) == dict(added=4, merged=0, out_of_range=0, invalid=0)
    assert ref.upload(p[:1]) is None  # 4 + 1 > 4, though it would merge: the integration's rule
    assert ref.upload(np.zeros((0, 3))) == dict(added=0, merged=0, out_of_range=0, invalid=0)
    ref.carve_configure(True)
    ref.carve_configure(False)  # the array stays
    ref.clear()
    assert ref.upload(p[:2], misses=[3, 0]) == dict(added=2, merged=0, out_of_range=0, invalid=0)
    assert ref.sorted()["misses"].tolist() == [3, 0]


def test_an_upload_is_not_an_integration():
    """The carve's `every` counts integrations, not owner numbers."""
    ref, plain = UR.UploadRef(0.5, 1 << 12), CR.CarveRef(0.5, 1 << 12)
    for r in (ref, plain):
        r.carve_configure(True, 0.0, 1, 1, 2)
    scans = [CR.scenario_scan(k) for k in range(3)]
    assert ref.integrate(scans[0], I34, 0) == plain.integrate(scans[0], I34, 0)
    assert ref.carve_last == plain.carve_last and ref.carve_last[1] == 1
    ref.upload(np.array([[100.25, 0.25, 0.25], [101.25, 0.25, 0.25]]), scan=[5, 6])
    assert ref.integrations == 1 and len(ref.seq_scan) == 3
    for k in (1, 2):  # integration 1 does not carve, integration 2 does: as without the upload
        assert ref.integrate(scans[k], I34, k) == plain.integrate(scans[k], I34, k)
        assert ref.carve_last == plain.carve_last and ref.carve_last[1] == (k + 1) % 2
    assert ref.integrations == 3
    far = {R.pack_key(200, 0, 0), R.pack_key(202, 0, 0)}
    got = {k: v for k, v in _state(ref).items() if k not in far}
    _same_state(got, {k: (v[0], plain.misses.get(k, 0), plain.seq_scan[v[1]], v[2], v[3]) for k, v in plain.vox.items()})
    assert sorted(_state(ref)) == sorted(set(got) | far)
    ref.clear()
    assert ref.integrations == 0 and ref.seq_scan == [] and ref.voxels == 0


def _header():
    return open(os.path.join(ROOT, "include", "fmx", "fmx.h")).read()


def test_header_and_library_surface(tmp_path):
    """Fails without the feature: the header declares fmx_upload_voxels, libfmx.so exports it,
    and the ctypes structs have the layout a compiler gives the header's."""
    hdr = _header()
    assert "fmx_upload_voxels" in set(re.findall(r"\b(fmx_[a-z_]+)\s*\(", hdr))
    from form_amd import fmx
    L = fmx.lib()
    assert hasattr(L, "fmx_upload_voxels") and "fmx_upload_voxels" in fmx.EXPORTED
    assert re.search(r"#define FMX_ABI_VERSION 1\b", hdr)
    cxx = shutil.which("g++")
    assert cxx, "the layout probe needs g++"
    vi = ["xyz", "scan", "index", "hits", "misses"]
    uc = ["added", "merged", "out_of_range", "invalid"]
    offs = [f"offsetof(fmx_voxel_input, {f})" for f in vi] + [f"offsetof(fmx_upload_counts, {f})" for f in uc]
    src = tmp_path / "upload.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "fmx/fmx.h"\nint main() {\n'
                   '  const size_t v[] = {sizeof(fmx_voxel_input), sizeof(fmx_upload_counts), ' + ", ".join(offs) + '};\n'
                   '  for (size_t x : v) std::printf("%zu ", x);\n}\n')
    exe = tmp_path / "upload"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    V, U = fmx._VoxelInput, fmx._UploadCounts
    assert got == [C.sizeof(V), C.sizeof(U)] + [getattr(V, f).offset for f in vi] + [getattr(U, f).offset for f in uc]
    assert [f for f, _ in V._fields_] == vi and [f for f, _ in U._fields_] == uc
    assert tuple(uc) == UR.COUNT_NAMES


def test_null_context_is_rejected():
    from form_amd import fmx
    L = fmx.lib()
    A, cnt = fmx._VoxelInput(), fmx._UploadCounts()
    assert L.fmx_upload_voxels(None, C.byref(A), C.c_uint32(0), C.byref(cnt)) == 1  # FMX_E_INVAL
    assert L.fmx_upload_voxels(None, None, C.c_uint32(0), None) == 1


def test_form_wrappers_need_the_dense_map(tmp_path):
    from form_amd import fmx
    f = fmx.FORM()
    empty = dict(points=np.zeros((0, 3)), scan=np.zeros(0, np.uint64), index=np.zeros(0, np.uint32),
                 hits=np.zeros(0, np.uint32))
    for call in (lambda: f.dense_restore(empty), lambda: f.dense_save(tmp_path / "m.npz"),
                 lambda: f.dense_load(tmp_path / "m.npz")):
        with pytest.raises(RuntimeError):
            call()  # the dense map is off


def test_host_parts_under_the_sanitizers():
    """tests/cpp/test_upload_host (built by __graft_entry__.build(), tests/cpp/upload_host.mk):
    the argument checks, the entry classes and the owner numbers, with ASan and UBSan linked
    into the stand-alone program."""
    path = os.path.join(ROOT, "tests", "cpp", "test_upload_host")
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build() (make -C tests/cpp -f upload_host.mk)")
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "upload host ok" in r.stdout, r.stdout + r.stderr[-3000:]

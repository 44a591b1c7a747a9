"""The dense voxel map without a device: the numpy restatement (tests/dense_ref.py) against
a deliberately naive per-point loop, its invariants, the header / library / ctypes surface
of the fmx_dense_* block, and the wrappers' behaviour without a GPU."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dense_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_SYMBOLS = ["fmx_dense_clear", "fmx_dense_configure", "fmx_dense_download", "fmx_dense_integrate",
                 "fmx_dense_last", "fmx_dense_stats"]


def _scan_5x40(seed):
    """5 x 40 points around the sensor: ranges 0.3 .. 130 m (both sides of the default gate),
    a few dropouts, a NaN, an infinity."""
    g = np.random.default_rng(seed)
    n = 5 * 40
    az = np.repeat(np.arange(40) * (2 * np.pi / 40), 5) + g.normal(0, 1e-3, n)
    el = np.tile(np.linspace(-0.3, 0.3, 5), 40)
    r = g.choice([0.3, 0.9, 2.0, 5.0, 5.02, 20.0, 99.0, 130.0], n) + g.normal(0, 1e-3, n)
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = r * np.cos(el) * np.cos(az)
    p[:, 1] = r * np.cos(el) * np.sin(az)
    p[:, 2] = r * np.sin(el)
    p[g.choice(n, 9, replace=False), :3] = 0.0
    p[17, 1] = np.nan
    p[101, 2] = -np.inf
    return p


def _pose(yaw, pitch, t):
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    T = np.zeros((3, 4))
    T[:, :3] = Rz @ Ry
    T[:, 3] = t
    return T


class Naive:
    """One point at a time, Python scalars: nothing shared with the restatement but the
    statement of the semantics."""

    def __init__(self, w, min2, max2):
        self.w, self.min2, self.max2 = w, min2, max2
        self.vox = {}
        self.seq = 0
        self.scans = []

    def integrate(self, pts, T, scan_idx):
        f32 = np.float32
        cnt = dict(added=0, merged=0, gated=0, out_of_range=0, invalid=0)
        for i in range(len(pts)):
            x, y, z = f32(pts[i, 0]), f32(pts[i, 1]), f32(pts[i, 2])
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)) or (x == 0 and y == 0 and z == 0):
                cnt["invalid"] += 1
                continue
            r2 = float(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z)))
            if not (r2 > self.min2 and r2 < self.max2):
                cnt["gated"] += 1
                continue
            xd, yd, zd = float(x), float(y), float(z)
            wp = [((float(T[k, 0]) * xd + float(T[k, 1]) * yd) + float(T[k, 2]) * zd) + float(T[k, 3]) for k in range(3)]
            c = [math.floor(v / self.w) for v in wp]
            if not all(abs(v) < (1 << 20) - 1 for v in c):
                cnt["out_of_range"] += 1
                continue
            key = R.pack_key(*c)
            if key in self.vox:
                v = self.vox[key]
                v[0] += 1
                cnt["merged"] += 1  # (a later point of the opening scan included)
            else:
                self.vox[key] = [1, self.seq, i, wp]
                cnt["added"] += 1
        self.seq += 1
        self.scans.append(scan_idx)
        return cnt

    def sorted(self):
        ks = sorted(self.vox)
        return dict(key=np.array(ks, np.uint64), points=np.array([self.vox[k][3] for k in ks], np.float64).reshape(-1, 3),
                    scan=np.array([self.scans[self.vox[k][1]] for k in ks], np.uint64),
                    index=np.array([self.vox[k][2] for k in ks], np.uint32),
                    hits=np.array([self.vox[k][0] for k in ks], np.uint32))


POSES = [_pose(0.3, 0.1, (-3.0, 2.0, -0.5)), _pose(-1.1, -0.2, (1.5, -40.0, 0.25)), _pose(2.5, 0.05, (0.0, 0.0, 0.0))]


@pytest.mark.parametrize("w", [0.5, 4.0])
def test_restatement_equals_naive_loop(w):
    ref, nav = R.DenseRef(w, 1 << 12), Naive(w, 1.0, 1e4)
    for k, T in enumerate(POSES):
        pts = _scan_5x40(k)
        a, b = ref.integrate(pts, T, (1 << 33) + k), nav.integrate(pts, T, (1 << 33) + k)
        assert a == b, k
        assert a["invalid"] >= 9 and a["gated"] > 0 and a["added"] > 0
    assert R.same(ref.sorted(), nav.sorted()) is None
    assert (ref.sorted()["hits"] > 1).any() and len(set(ref.sorted()["scan"].tolist())) > 1


def test_invariants():
    ref = R.DenseRef(0.5, 1 << 12)
    total = 0
    for k, T in enumerate(POSES):
        pts = _scan_5x40(k)
        c = ref.integrate(pts, T, k)
        assert sum(c.values()) == len(pts)
        total += c["added"] + c["merged"]
        assert int(ref.sorted()["hits"].sum()) == total
        assert ref.voxels == len(ref.sorted()["key"])
    # the same scan again: no voxel is added, every valid point merges, nothing stored moves
    before = ref.sorted()
    c = ref.integrate(_scan_5x40(2), POSES[2], 99)
    assert c["added"] == 0 and c["merged"] > 0
    after = ref.sorted()
    for f in ("key", "points", "scan", "index"):
        assert np.array_equal(before[f], after[f])
    assert int(after["hits"].sum()) == total + c["merged"]
    # min_hits filters, 0 is 1; the capacity rule refuses without changing anything
    assert len(ref.sorted(2)["key"]) < len(after["key"]) and len(ref.sorted(0)["key"]) == len(after["key"])
    small = R.DenseRef(0.5, 150)
    assert small.integrate(_scan_5x40(0), POSES[0]) is None and small.voxels == 0 and small.seq_scan == []
    # a download in any order sorts back to the map
    o = np.random.default_rng(1).permutation(len(after["key"]))
    d = {f: after[f][o] for f in ("points", "scan", "index", "hits")}
    assert R.same(R.sort_download(d, 0.5), after) is None


def test_keys_floor_and_home_slot():
    I = np.eye(3, 4)
    p = np.zeros((4, 4), np.float32)
    p[:, 0] = [-0.25, -0.2, 0.2, 0.25]
    p[:, 1] = 3.0
    cls, world, key = R.classify(p, I, 0.25, 1.0, 1e4)
    assert (cls == 0).all()
    assert [int(k) >> 42 for k in key] == [R.BIAS - 1, R.BIAS - 1, R.BIAS, R.BIAS + 1]  # floor, not truncation
    assert np.array_equal(R.key_of_points(world, 0.25), key)
    assert R.slots_for(1024) == 2048 and R.slots_for(1025) == 4096 and R.slots_for(1) == 2
    assert R.mix64(0) == 0 and R.mix64(1) != R.mix64(2) and R.mix64((1 << 64) + 5) == R.mix64(5)
    assert all(0 <= R.home_slot(k, 2048) < 2048 for k in key)
    assert int(key.max()) < R.EMPTY_KEY


def _header():
    return open(os.path.join(ROOT, "include", "fmx", "fmx.h")).read()


def test_header_and_library_surface(tmp_path):
    """Fails without the feature: the header declares the fmx_dense_* block, libfmx.so
    exports it, and the ctypes structs have the sizes a compiler gives the header's."""
    hdr = _header()
    declared = sorted(s for s in set(re.findall(r"\b(fmx_[a-z_]+)\s*\(", hdr)) if s.startswith("fmx_dense_"))
    assert declared == DENSE_SYMBOLS
    from form_amd import fmx
    L = fmx.lib()
    assert all(hasattr(L, s) for s in DENSE_SYMBOLS)
    assert set(DENSE_SYMBOLS) <= set(fmx.EXPORTED)
    assert re.search(r"#define FMX_ABI_VERSION 1\b", hdr)
    cxx = shutil.which("g++")
    assert cxx, "the layout probe needs g++"
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "fmx/fmx.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu %zu\\n", sizeof(fmx_dense_params), '
                   'sizeof(fmx_dense_counts), offsetof(fmx_dense_params, max_voxels), '
                   'offsetof(fmx_dense_params, every), offsetof(fmx_dense_counts, invalid)); }\n')
    exe = tmp_path / "probe"
    subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(fmx._DenseParams), C.sizeof(fmx._DenseCounts), fmx._DenseParams.max_voxels.offset,
                   fmx._DenseParams.every.offset, fmx._DenseCounts.invalid.offset]
    assert [f for f, _ in fmx._DenseCounts._fields_] == ["added", "merged", "gated", "out_of_range", "invalid"]


def test_null_context_is_rejected():
    from form_amd import fmx
    L = fmx.lib()
    p = fmx._DenseParams()
    n = C.c_uint32(0)
    assert L.fmx_dense_configure(None, C.byref(p)) == 1  # FMX_E_INVAL
    assert L.fmx_dense_integrate(None, None, C.c_size_t(0), C.c_int(0), None, C.c_uint64(0), None) == 1
    assert L.fmx_dense_last(None, None, None) == 1
    assert L.fmx_dense_stats(None, None) == 1
    assert L.fmx_dense_download(None, C.c_uint32(1), None, None, None, None, C.byref(n)) == 1
    assert L.fmx_dense_clear(None) == 1


def test_wrappers_without_a_device_raise():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from form_amd import fmx
    with pytest.raises(fmx.FmxError):
        fmx.Context().dense_configure(True, 0.2, 1024)
    f = fmx.FORM()
    f.set_dense_map(True, voxel_width=0.2, max_voxels=1024)
    with pytest.raises(fmx.FmxError):
        f.initialize()
    d = f.dense_map()  # no estimator: an empty map, no crash
    assert d["points"].shape == (0, 3) and len(d["hits"]) == 0

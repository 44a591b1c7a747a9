"""Rolling the dense voxel map without a device: the numpy restatement (tests/roll_ref.py)
against a deliberately naive per-voxel loop, its invariants, the header / library / ctypes
surface of the fmx_roll_* block, and the wrappers' behaviour without a GPU."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dense_ref as R
import roll_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLL_SYMBOLS = ["fmx_roll_configure", "fmx_roll_count", "fmx_roll_drain", "fmx_roll_evict", "fmx_roll_stats"]


def _scan_5x40(seed):
    """5 x 40 points around the sensor: ranges 0.3 .. 130 m (both sides of the default gate),
    a few dropouts, a NaN, an infinity (test_dense_cpu.py's scans, restated)."""
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


POSES = [_pose(0.3, 0.1, (-3.0, 2.0, -0.5)), _pose(-1.1, -0.2, (1.5, -40.0, 0.25)), _pose(2.5, 0.05, (0.0, 0.0, 0.0))]


def _filled(w, cls=RR.RollRef):
    ref = cls(w, 1 << 12)
    for k, T in enumerate(POSES):
        ref.integrate(_scan_5x40(k), T, (1 << 33) + k)
    return ref


def _naive_outside(ref, centre, half):
    """One voxel at a time, Python integers: the keys of the voxels outside the box."""
    cc = [math.floor(float(centre[k]) / ref.w) for k in range(3)]
    out = []
    for key in ref.vox:
        v = [((key >> 42) & 0x1FFFFF) - (1 << 20), ((key >> 21) & 0x1FFFFF) - (1 << 20), (key & 0x1FFFFF) - (1 << 20)]
        if not all(abs(v[k] - cc[k]) <= half[k] for k in range(3)):
            out.append(key)
    return sorted(out)


@pytest.mark.parametrize("w,half", [(0.5, (20, 30, 4)), (4.0, (3, 3, 1)), (0.5, (0, 0, 0)), (0.5, (1 << 21,) * 3)])
def test_restatement_equals_naive_loop(w, half):
    ref = _filled(w)
    before = ref.sorted()
    centre = POSES[0][:, 3]
    want_out = _naive_outside(ref, centre, half)
    n_in, n_out = ref.count(centre, half)
    assert n_out == len(want_out) and n_in + n_out == len(before["key"])  # a partition
    assert R.same(ref.sorted(), before) is None  # counting changes nothing
    ev = ref.evict(centre, half)
    assert ev["key"].tolist() == want_out
    after = ref.sorted()
    assert ref.voxels == n_in == len(after["key"])
    assert sorted(ev["key"].tolist() + after["key"].tolist()) == before["key"].tolist()
    # kept and evicted voxels carry exactly what the map held for them
    pos = {int(k): i for i, k in enumerate(before["key"])}
    for part in (ev, after):
        ix = np.array([pos[int(k)] for k in part["key"]], np.int64)
        assert R.same(part, {f: before[f][ix] for f in before}) is None
    if half == (0, 0, 0):
        cc = RR.centre_voxel(centre, w)
        assert after["key"].tolist() in ([], [R.pack_key(*cc)])
    if half == (1 << 21,) * 3:
        assert n_out == 0
    else:
        assert n_out > 0
    assert len(ref.seq_scan) == 3  # the integration counter is unchanged


def test_half_zero_keeps_only_the_centre_voxel():
    ref = _filled(0.5)
    some = ref.sorted()
    k = len(some["key"]) // 2
    ev = ref.evict(some["points"][k], (0, 0, 0))
    left = ref.sorted()
    assert left["key"].tolist() == [int(some["key"][k])] and len(ev["key"]) == len(some["key"]) - 1
    assert np.array_equal(left["points"].view(np.uint64), some["points"][k:k + 1].view(np.uint64))


def test_reintegration_opens_evicted_voxels_under_the_new_seq():
    ref = _filled(0.5)
    before = ref.sorted()
    ev = ref.evict(POSES[0][:, 3], (20, 30, 4))
    kept = ref.sorted()
    c = ref.integrate(_scan_5x40(1), POSES[1], 77)  # scan 1 again, as integration 3
    after = ref.sorted()
    back = np.isin(after["key"], ev["key"])
    assert c["added"] == int(back.sum()) > 0
    assert (after["scan"][back] == 77).all()  # new owner ...
    assert set(after["key"][back].tolist()) <= set(before["key"].tolist())
    once = RR.RollRef(0.5, 1 << 12)
    once.integrate(_scan_5x40(1), POSES[1], 77)
    alone = {int(k): int(h) for k, h in zip(once.sorted()["key"], once.sorted()["hits"])}
    assert all(int(h) == alone[int(k)] for k, h in zip(after["key"][back], after["hits"][back]))  # ... hits from it on
    still = np.isin(after["key"], kept["key"])
    for f in ("points", "scan", "index"):
        assert np.array_equal(after[f][still], kept[f])  # kept voxels keep their owner
    assert ref.voxels == len(kept["key"]) + c["added"]


def test_centre_floor_not_truncation():
    assert RR.centre_voxel((-0.1, -0.25, 0.25), 0.25) == [-1, -1, 1]  # negative; exactly on a face
    assert RR.centre_voxel((np.nextafter(0.25, 0.0), -np.nextafter(0.25, 0.0), 0.0), 0.25) == [0, -1, 0]
    L = float((1 << 20) - 2)
    assert RR.centre_voxel((L, -L, 0.0), 1.0) == [(1 << 20) - 2, -(1 << 20) + 2, 0]
    assert RR.centre_voxel((L + 1, 0.0, 0.0), 1.0) is None and RR.centre_voxel((0.0, -L - 0.5, 0.0), 1.0) is None
    assert RR.centre_voxel((np.nan, 0.0, 0.0), 1.0) is None and RR.centre_voxel((0.0, np.inf, 0.0), 1.0) is None
    # the box edge: cc +- half kept, cc +- (half + 1) evicted, also across 0
    keys = [R.pack_key(x, -3, 5) for x in (-5, -4, -1, 0, 2, 3)]
    assert RR.inside(keys, (-1, -3, 5), (3, 0, 0)).tolist() == [False, True, True, True, True, False]
    with pytest.raises(ValueError):
        _filled(0.5).count((0.0, 0.0, 0.0), ((1 << 21) + 1, 0, 0))


def test_register_trigger():
    """The register path's rule on hand-made poses: the first look records, a step rolls
    and records, a refusal by capacity rolls whatever the step."""
    def pose(x):
        return _pose(0.0, 0.0, (x, 0.0, 0.0))

    ref = RR.RollRef(0.5, 1 << 12)
    ref.roll_configure(True, (10, 10, 10), 1.0)
    pts = [_scan_5x40(k) for k in range(3)]
    xs = [0.0, 0.5, 0.75, 1.5, 1.75, 2.4, 2.5]
    rolled = []
    for j, x in enumerate(xs):
        roll, integrated, c = ref.register(j, pts[j % 3], pose(x), pose(xs[j - 1]) if j else None)
        assert integrated == 1 and sum(c.values()) == 200
        if roll:
            rolled.append(j)
            assert roll == ref.rolls[-1][1:] and roll[0] == ref.voxels - c["added"]
    # centre 0.0 recorded at scan 1; |1.5 - 0| >= 1 seen at scan 4; |2.5 - 1.5| >= 1 never seen (no scan 7)
    assert rolled == [4] and ref.stats()["rolls"] == 1 and ref.stats()["last_scan"] == 4
    assert ref.stats()["spilled"] == ref.stats()["evicted"] == ref.rolls[0][2] > 0
    d = ref.drain()
    assert len(d["hits"]) == ref.rolls[0][2] and ref.stats()["spilled"] == 0
    assert np.array_equal(np.lexsort((d["index"], d["scan"])), np.arange(len(d["hits"])))
    # capacity: a huge step, a map too small for another scan
    big = RR.RollRef(0.5, 1 << 12)
    big.integrate(pts[0], pose(0.0), 0)
    cap = big.voxels + 199
    small = RR.RollRef(0.5, cap)
    small.roll_configure(True, (4, 4, 4), 1e9, spill=False)
    out = [small.register(j, pts[j % 3], pose(0.1 * j), pose(0.1 * (j - 1)) if j else None) for j in range(3)]
    assert [o[1] for o in out] == [1, -1, 1]  # scan 1 only records the centre and is refused; scan 2 rolls
    assert out[2][0] is not None and out[2][0][1] > 0 and small.stats()["spilled"] == 0
    off = RR.RollRef(0.5, cap)
    assert [off.register(j, pts[j % 3], pose(0.1 * j), None)[1] for j in range(3)] == [1, -1, -1]


def _header():
    return open(os.path.join(ROOT, "include", "fmx", "fmx.h")).read()


def test_header_and_library_surface(tmp_path):
    """Fails without the feature: the header declares the fmx_roll_* block, libfmx.so exports
    it, and the ctypes struct has the layout a compiler gives the header's."""
    hdr = _header()
    declared = sorted(s for s in set(re.findall(r"\b(fmx_[a-z_]+)\s*\(", hdr)) if s.startswith("fmx_roll_"))
    assert declared == ROLL_SYMBOLS
    from form_amd import fmx
    L = fmx.lib()
    assert all(hasattr(L, s) for s in ROLL_SYMBOLS)
    assert set(ROLL_SYMBOLS) <= set(fmx.EXPORTED)
    assert re.search(r"#define FMX_ABI_VERSION 1\b", hdr)
    assert "never pruned" not in hdr
    cxx = shutil.which("g++")
    assert cxx, "the layout probe needs g++"
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "fmx/fmx.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu %zu\\n", sizeof(fmx_roll_params), '
                   'offsetof(fmx_roll_params, enable), offsetof(fmx_roll_params, half), '
                   'offsetof(fmx_roll_params, step), offsetof(fmx_roll_params, spill)); }\n')
    exe = tmp_path / "probe"
    subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = fmx._RollParams
    assert got == [C.sizeof(P), P.enable.offset, P.half.offset, P.step.offset, P.spill.offset]
    assert [f for f, _ in P._fields_] == ["enable", "half", "step", "spill"]


def test_null_context_is_rejected():
    from form_amd import fmx
    L = fmx.lib()
    p = fmx._RollParams()
    n = C.c_uint32(0)
    c = np.zeros(3)
    h = np.zeros(3, np.uint32)
    out = np.zeros(6, np.uint64)
    assert L.fmx_roll_configure(None, C.byref(p)) == 1  # FMX_E_INVAL
    assert L.fmx_roll_count(None, fmx._p(c), fmx._p(h), fmx._p(out)) == 1
    assert L.fmx_roll_evict(None, fmx._p(c), fmx._p(h), None, None, None, None, C.byref(n)) == 1
    assert L.fmx_roll_drain(None, None, None, None, None, C.byref(n)) == 1
    assert L.fmx_roll_stats(None, fmx._p(out)) == 1


def test_wrappers_without_a_device_raise():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from form_amd import fmx
    for call in (lambda c: c.roll_configure(True, (10, 10, 10), 1.0), lambda c: c.roll_count((0, 0, 0), (1, 1, 1)),
                 lambda c: c.roll_evict((0, 0, 0), (1, 1, 1)), lambda c: c.roll_drain(), lambda c: c.roll_stats()):
        with pytest.raises(fmx.FmxError):
            call(fmx.Context())
    f = fmx.FORM()
    f.set_dense_map(True, voxel_width=0.2, max_voxels=1024)
    f.set_dense_roll(True, 50.0, 2.0)
    with pytest.raises(fmx.FmxError):
        f.initialize()
    d = f.dense_evicted()  # no estimator: nothing evicted, no crash
    assert d["points"].shape == (0, 3) and len(d["hits"]) == 0
    assert d["scan"].dtype == np.uint64 and d["index"].dtype == np.uint32 and d["hits"].dtype == np.uint32

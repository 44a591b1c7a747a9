"""Probing the dense voxel map restated in plain Python (include/fmx/fmx.h, fmx_probe_points;
DESIGN.md §Dense map, Probing) over tests/carve_ref.py, tests/roll_ref.py and
tests/dense_ref.py, none of which it changes: the point classes without the gate, the filter,
the lookup, and the first-hit segment cast with its own walk, which also returns the tau at
which each voxel of the path is entered.  Every fp64 operation is one Python float operation
(IEEE double, one rounding), in the order the header states, so the tests compare with
equality, doubles as bits."""
import math

import numpy as np

import carve_ref as CR
import dense_ref as R
import roll_ref as RR  # noqa: F401  (the restatement's base classes live there)

INF = float("inf")
ABSENT, FILTERED, SOLID, OUT_OF_RANGE, INVALID = range(5)
NO_STEP = 0xFFFFFFFF
VOXEL_FIELDS = ("points", "scan", "index", "hits", "misses")


def walk_tau(o, e, w):
    """(path, tin): the voxels v_0 = a ... v_S = b of the segment from o to e at width w as
    int triples, and for each the tau of the step that entered it (0.0 for v_0)."""
    o, e, w = [float(v) for v in o], [float(v) for v in e], float(w)
    a = [int(math.floor(o[k] / w)) for k in range(3)]
    b = [int(math.floor(e[k] / w)) for k in range(3)]
    d = [e[k] - o[k] for k in range(3)]
    s = [1 if b[k] > a[k] else -1 for k in range(3)]
    cur = list(a)
    tau = [INF, INF, INF]
    for k in range(3):
        if cur[k] != b[k]:
            tau[k] = (float(cur[k] + (1 if s[k] > 0 else 0)) * w - o[k]) / d[k]
    path, tin = [tuple(cur)], [0.0]
    S = abs(b[0] - a[0]) + abs(b[1] - a[1]) + abs(b[2] - a[2])
    for _ in range(S):
        k = min(range(3), key=lambda j: (tau[j], j))  # the smallest tau, the lowest k among equal ones
        tin.append(tau[k])
        cur[k] += s[k]
        tau[k] = INF if cur[k] == b[k] else (float(cur[k] + (1 if s[k] > 0 else 0)) * w - o[k]) / d[k]
        path.append(tuple(cur))
    return path, tin


def classify_point(p, T, w):
    """(class, world point, voxel) of one fp32 point: INVALID, OUT_OF_RANGE, or None (a voxel)."""
    x, y, z = float(p[0]), float(p[1]), float(p[2])
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)) or (x == 0.0 and y == 0.0 and z == 0.0):
        return INVALID, None, None
    wp = [((T[k][0] * x + T[k][1] * y) + T[k][2] * z) + T[k][3] for k in range(3)]
    v = []
    for k in range(3):
        q = wp[k] / w
        if not math.isfinite(q) or not abs(float(math.floor(q))) < R.LIMIT:
            return OUT_OF_RANGE, wp, None
        v.append(int(math.floor(q)))
    return None, wp, tuple(v)


def first_hit(path, skip, solid):
    """The first s >= skip with solid(path[s]), or None; and the voxels examined on the way."""
    for s in range(int(skip), len(path)):
        if solid(path[s]):
            return s, s - int(skip) + 1
    return None, max(len(path) - int(skip), 0)


class ProbeRef(CR.CarveRef):
    """CarveRef with the two read-only probes."""

    def _solid(self, key, min_hits, num, den):
        v = self.vox.get(key)
        return v is not None and CR.takes(v[0], self.misses.get(key, 0), min_hits, num, den)

    def _blank(self, n):
        return dict(state=np.zeros(n, np.uint8), points=np.zeros((n, 3)), scan=np.zeros(n, np.uint64),
                    index=np.zeros(n, np.uint32), hits=np.zeros(n, np.uint32), misses=np.zeros(n, np.uint32))

    def _report(self, out, i, key):
        v = self.vox[key]
        out["points"][i] = v[3]
        out["scan"][i] = self.seq_scan[v[1]]
        out["index"][i], out["hits"][i], out["misses"][i] = v[2], v[0], self.misses.get(key, 0)

    def probe_points(self, xyzw, pose34, min_hits=1, max_miss_ratio=None):
        num, den = CR.miss_fraction(max_miss_ratio)
        p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(pose34, np.float64).reshape(3, 4).tolist()
        out = self._blank(len(p))
        names = ("absent", "filtered", "solid", "out_of_range", "invalid")
        counts = dict.fromkeys(names, 0)
        for i in range(len(p)):
            cls, _, v = classify_point(p[i], T, self.w)
            if cls is None:
                key = R.pack_key(*v)
                cls = ABSENT
                if key in self.vox:
                    cls = SOLID if self._solid(key, min_hits, num, den) else FILTERED
                    self._report(out, i, key)
            out["state"][i] = cls
            counts[names[cls]] += 1
        out["counts"] = counts
        return out

    def probe_rays(self, xyzw, pose34, min_hits=1, max_miss_ratio=None, skip=0):
        """Raises ValueError("FMX_E_RANGE") when the origin's voxel is out of range."""
        num, den = CR.miss_fraction(max_miss_ratio)
        p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(pose34, np.float64).reshape(3, 4)
        if CR.origin_voxel(T, self.w) is None:
            raise ValueError("FMX_E_RANGE")
        o, T = T[:, 3].tolist(), T.tolist()
        out = self._blank(len(p))
        out["step"], out["t"] = np.full(len(p), NO_STEP, np.uint32), np.full(len(p), INF)
        counts = dict(hit=0, clear=0, out_of_range=0, invalid=0, steps=0)
        for i in range(len(p)):
            cls, e, _ = classify_point(p[i], T, self.w)
            if cls is not None:
                out["state"][i] = cls
                counts["invalid" if cls == INVALID else "out_of_range"] += 1
                continue
            path, tin = walk_tau(o, e, self.w)
            s, examined = first_hit(path, skip, lambda v: self._solid(R.pack_key(*v), min_hits, num, den))
            counts["steps"] += examined
            if s is None:
                counts["clear"] += 1
                continue
            counts["hit"] += 1
            out["state"][i], out["step"][i], out["t"][i] = SOLID, s, tin[s]
            self._report(out, i, R.pack_key(*path[s]))
        out["counts"] = counts
        return out


def same(a, b, fields=None):
    """Equality of two probe results (dicts of arrays and a counts dict), doubles compared as
    bits; the first field that differs, or None."""
    for f in sorted(set(a) | set(b)) if fields is None else fields:
        if f == "counts":
            if a[f] != b[f]:
                return f
            continue
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), np.ascontiguousarray(y, np.float64).view(np.uint64)
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            return f
    return None


# ---------------------------------------------------------------- the dynamic-object scenario
# (tests/carve_ref.py's: tests/test_probe_cpu.py casts through it on the restatement alone,
# tests/test_gpu_probe.py on the device.)
def scenario():
    ref = ProbeRef(CR.SCN_W, CR.SCN_CAP, 1.0, 1e4)
    ref.carve_configure(True, 0.0, 1, 1, 1)
    for k in range(CR.SCN_SCANS):
        assert ref.integrate(CR.scenario_scan(k), np.eye(3, 4), k) is not None
    return ref


def scenario_middle():
    """The indices of the middle 5 x 5 rays of the 11 x 11 fan."""
    return [a * 11 + b for a in range(3, 8) for b in range(3, 8)]


def check_scenario(cast):
    """cast(max_miss_ratio) -> a probe_rays result of the last scan's rays from the origin."""
    mid = scenario_middle()
    seen, kept = cast(None), cast(0.5)
    for got in (seen, kept):
        assert (got["state"] == SOLID).all() and got["counts"]["hit"] == 121
    xv = lambda got: np.floor(got["points"][:, 0] / CR.SCN_W).astype(int)  # noqa: E731
    assert (xv(seen)[mid] == 8).all() and (xv(kept) == 20).all()  # the box; the wall behind it, for every ray
    assert (seen["misses"][mid] >= 3).all() and (kept["misses"] == 0).all()
    assert (seen["t"][mid] < kept["t"][mid]).all() and (seen["step"][mid] < kept["step"][mid]).all()
    assert kept["counts"]["steps"] > seen["counts"]["steps"]

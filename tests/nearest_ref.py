"""The nearest solid voxel of the dense map restated in plain Python (include/fmx/fmx.h,
fmx_nearest_voxels; DESIGN.md §Dense map, Nearest) over tests/probe_ref.py, which it does not
change: a brute-force loop over the whole cube of cells around the point's own voxel, with no
shell order and no early stop, so it is the definition.  Every fp64 operation is one Python
float operation (IEEE double, one rounding), in the order the header states, so the tests
compare with equality, doubles as bits."""
import math

import numpy as np

import carve_ref as CR
import dense_ref as R
import probe_ref as PR

INF = float("inf")
MAX_REACH = 8
LIM = (1 << 20) - 1  # a storable coordinate: |c| < LIM
CLASSES = ("found", "none", "out_of_range", "invalid")


def storable(v):
    return all(abs(c) < LIM for c in v)


class NearestRef(PR.ProbeRef):
    """ProbeRef with nearest_voxels()."""

    def nearest_voxels(self, xyzw, pose34, reach=1, max_dist=None, min_hits=1, max_miss_ratio=None, max_dist2=None):
        """max_dist2 overrides max_dist * max_dist.  The result's counts hold the four classes;
        `lookups_bounds` is (valid in-range points, storable cube cells of those points), which
        the device's `lookups` lies between."""
        num, den = CR.miss_fraction(max_miss_ratio)
        if max_dist2 is None:
            md = INF if max_dist is None else float(max_dist)
            max_dist2 = md * md
        max_dist2, reach = float(max_dist2), int(reach)
        if reach > MAX_REACH or not max_dist2 >= 0.0:
            raise ValueError("FMX_E_INVAL")
        p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(pose34, np.float64).reshape(3, 4).tolist()
        out = self._blank(len(p))
        out["dist2"] = np.full(len(p), INF)
        counts = dict.fromkeys(CLASSES, 0)
        points, cells = 0, 0
        span = range(-reach, reach + 1)
        for i in range(len(p)):
            cls, wp, c = PR.classify_point(p[i], T, self.w)
            if cls is not None:
                out["state"][i] = cls
                counts["invalid" if cls == PR.INVALID else "out_of_range"] += 1
                continue
            points += 1
            best = None  # (d2, key)
            for dx in span:
                for dy in span:
                    for dz in span:
                        v = (c[0] + dx, c[1] + dy, c[2] + dz)
                        if not storable(v):
                            continue
                        cells += 1
                        key = R.pack_key(*v)
                        if not self._solid(key, min_hits, num, den):
                            continue
                        q = self.vox[key][3]
                        e0, e1, e2 = float(q[0]) - wp[0], float(q[1]) - wp[1], float(q[2]) - wp[2]
                        d2 = (e0 * e0 + e1 * e1) + e2 * e2
                        if d2 <= max_dist2 and (best is None or (d2, key) < best):
                            best = (d2, key)
            if best is None:
                out["state"][i] = PR.ABSENT
                counts["none"] += 1
                continue
            out["state"][i], out["dist2"][i] = PR.SOLID, best[0]
            counts["found"] += 1
            self._report(out, i, best[1])
        out["counts"] = counts
        out["lookups_bounds"] = (points, cells)
        return out


def same(got, want, fields=None):
    """Equality of a device result and the restatement's (or of two of either), doubles as
    bits, the class counts equal and `lookups`, where one side has it, within the other's
    bounds; the first thing that differs, or None."""
    a, b = dict(got), dict(want)
    ca, cb = dict(a.pop("counts")), dict(b.pop("counts"))
    ba, bb = a.pop("lookups_bounds", None), b.pop("lookups_bounds", None)
    la, lb = ca.pop("lookups", None), cb.pop("lookups", None)
    if ca != cb:
        return "counts"
    for look, bounds in ((la, bb), (lb, ba)):
        if look is not None and bounds is not None and not bounds[0] <= look <= bounds[1]:
            return "lookups"
    if la is not None and lb is not None and la != lb:
        return "lookups"
    return PR.same(a, b, fields)


def fitness(result):
    """FORM.dense_fitness's figures from a nearest_voxels result, restated."""
    st, d2 = result["state"], result["dist2"]
    found = [i for i in range(len(st)) if st[i] == PR.SOLID]
    n_valid = len(found) + sum(1 for s in st if s == PR.ABSENT)
    total = math.fsum(float(d2[i]) for i in found)
    return dict(n_valid=n_valid, n_found=len(found), fitness=len(found) / n_valid if n_valid else 0.0,
                rmse=math.sqrt(total / len(found)) if found else 0.0)

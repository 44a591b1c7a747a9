"""Carving the dense voxel map restated in plain Python (include/fmx/fmx.h, fmx_carve_configure;
DESIGN.md §Dense map, Carving) over tests/dense_ref.py and tests/roll_ref.py: which points
cast a ray, the voxel walk from the sensor to the return, the examined voxels, the exemption
of the integration's own voxels and the miss filter of a download.  Every fp64 operation is
one Python float operation (IEEE double, one rounding), in the order the header states, so
the tests compare with equality."""
import math

import numpy as np

import dense_ref as R
import roll_ref as RR

INF = float("inf")


def miss_fraction(max_miss_ratio):
    """form_amd.fmx.miss_fraction restated: the ratio in 1/65536ths, rounded to nearest."""
    if max_miss_ratio is None:
        return 0, 0
    return int(min(math.floor(float(max_miss_ratio) * 65536.0 + 0.5), float((1 << 32) - 1))), 1 << 16


def takes(hits, misses, min_hits=1, num=0, den=0):
    """A download's rule, in integers."""
    if int(hits) < max(int(min_hits), 1):
        return False
    return den == 0 or int(misses) * int(den) <= int(hits) * int(num)


def origin_voxel(pose34, w):
    """a = floor(o / w) of the pose's translation as three ints, or None when out of range."""
    return RR.centre_voxel(np.asarray(pose34, np.float64).reshape(3, 4)[:, 3], w)


def walk(o, e, w):
    """The path v_0 = a ... v_S = b of the ray from o to e through voxels of width w, as a
    list of int triples.  o, e: three floats each."""
    o, e, w = [float(v) for v in o], [float(v) for v in e], float(w)
    a = [int(math.floor(o[k] / w)) for k in range(3)]
    b = [int(math.floor(e[k] / w)) for k in range(3)]
    d = [e[k] - o[k] for k in range(3)]
    s = [1 if b[k] > a[k] else -1 for k in range(3)]
    cur = list(a)

    def tau(k):
        if cur[k] == b[k]:
            return INF
        g = float(cur[k] + (1 if s[k] > 0 else 0)) * w
        return (g - o[k]) / d[k]

    t = [tau(0), tau(1), tau(2)]
    path = [tuple(cur)]
    for _ in range(sum(abs(b[k] - a[k]) for k in range(3))):
        k = 0  # the smallest tau, the lowest k among equal ones
        if t[1] < t[k]:
            k = 1
        if t[2] < t[k]:
            k = 2
        cur[k] += s[k]
        t[k] = tau(k)
        path.append(tuple(cur))
    return path


def examined(path, margin):
    """v_s with 0 <= s <= S - 1 - margin."""
    S = len(path) - 1
    return path[:max(S - int(margin), 0)]


def ray_indices(xyzw, pose34, w, min2, max2, carve_max2, stride):
    """(indices of the points that cast a ray, cls, world, key) of one launch."""
    p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
    cls, world, key = R.classify(p, pose34, w, min2, max2)
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        r2 = ((x * x + y * y) + z * z).astype(np.float64)  # the same fp32 r2, widened
        ok = (cls == 0) & (r2 < np.float64(carve_max2)) & (np.arange(len(p)) % max(int(stride), 1) == 0)
    return np.flatnonzero(ok), cls, world, key


def no_counts():
    return dict(rays=0, steps=0, misses=0, exempt=0)


class CarveRef(RR.RollRef):
    """RollRef with per-voxel miss counts."""

    def __init__(self, voxel_width, max_voxels, min2=1.0, max2=1e4, every=1):
        self.misses = {}  # key -> misses (absent: 0)
        super().__init__(voxel_width, max_voxels, min2, max2, every)
        self.carve_configure(False)
        self.carve_last = (no_counts(), 0)

    def clear(self):
        super().clear()
        self.misses = {}

    def carve_configure(self, enable=True, max_norm_squared=0.0, margin=1, ray_stride=1, every=1):
        self.carve_on = bool(enable)
        self.carve_max2 = float(max_norm_squared) if max_norm_squared != 0.0 else self.max2
        self.margin, self.stride, self.carve_every = int(margin), max(int(ray_stride), 1), max(int(every), 1)

    # ---- the rays of one launch; exempt: a set of keys, or None
    def _cast(self, xyzw, pose34, exempt):
        c = no_counts()
        T = np.ascontiguousarray(pose34, np.float64).reshape(3, 4)
        if origin_voxel(T, self.w) is None:
            return c
        idx, _, world, _ = ray_indices(xyzw, T, self.w, self.min2, self.max2, self.carve_max2, self.stride)
        o = T[:, 3].tolist()
        for i in idx.tolist():
            c["rays"] += 1
            for v in examined(walk(o, world[i].tolist(), self.w), self.margin):
                c["steps"] += 1
                k = R.pack_key(*v)
                if k not in self.vox:
                    continue
                if exempt is not None and k in exempt:
                    c["exempt"] += 1
                else:
                    self.misses[k] = self.misses.get(k, 0) + 1
                    c["misses"] += 1
        return c

    def carve_rays(self, xyzw, pose34):
        """fmx_carve_rays: stand-alone, nothing exempt."""
        return self._cast(xyzw, pose34, None)

    def integrate(self, xyzw, pose34, scan_idx=0):
        seq = len(self.seq_scan)
        counts = super().integrate(xyzw, pose34, scan_idx)
        self.carve_last = (no_counts(), 0)
        if counts is None or not self.carve_on or seq % self.carve_every:
            return counts
        cls, _, key = R.classify(xyzw, pose34, self.w, self.min2, self.max2)
        own = set(key[cls == 0].tolist())  # every voxel a point of this integration fell into
        self.carve_last = (self._cast(xyzw, pose34, own), 1)
        return counts

    # ---- downloads
    def sorted(self, min_hits=1, max_miss_ratio=None):
        num, den = miss_fraction(max_miss_ratio)
        d = super().sorted(min_hits)
        m = np.array([self.misses.get(k, 0) for k in d["key"].tolist()], np.uint32)
        keep = np.array([takes(h, x, min_hits, num, den) for h, x in zip(d["hits"].tolist(), m.tolist())], bool)
        out = {f: v[keep] for f, v in d.items()}
        out["misses"] = m[keep]
        return out

    def evict(self, centre, half):
        _, out = self._split(centre, half)
        m = np.array([self.misses.pop(k, 0) for k in out], np.uint32)
        ev = super().evict(centre, half)
        ev["misses"] = m
        return ev

    def drain(self):
        if not self.spilled:
            d = dict(RR.empty(), misses=np.zeros(0, np.uint32))
        else:
            d = {f: np.concatenate([e[f] for e in self.spilled]) for f in RR._F + ("misses",)}
        self.spilled = []
        return sort_by_owner(d)


def sort_by_owner(d):
    o = np.lexsort((np.asarray(d["index"]), np.asarray(d["scan"])))
    out = RR.sort_by_owner(d)
    out["misses"] = np.asarray(d["misses"], np.uint32)[o]
    return out


def sort_download(d, voxel_width):
    """A download with misses by key."""
    key = R.key_of_points(d["points"], voxel_width)
    o = np.argsort(key, kind="stable")
    out = R.sort_download(d, voxel_width)
    out["misses"] = np.asarray(d["misses"], np.uint32)[o]
    return out


def same(a, b):
    """R.same and the misses; the first field that differs, or None."""
    f = R.same(a, b)
    if f is not None:
        return f
    x, y = np.asarray(a["misses"]), np.asarray(b["misses"])
    return None if x.shape == y.shape and np.array_equal(x, y) else "misses"


def same_owner_sorted(a, b):
    f = RR.same_owner_sorted(a, b)
    if f is not None:
        return f
    x, y = np.asarray(a["misses"]), np.asarray(b["misses"])
    return None if x.shape == y.shape and np.array_equal(x, y) else "misses"


# ---------------------------------------------------------------- the dynamic-object scenario
# (tests/test_carve_cpu.py checks it on the restatement alone, tests/test_gpu_carve.py runs
# it on the device.)  A sensor at the origin looks along +x at a wall at x = 10.25 through an
# 11 x 11 fan of rays.  In scans 0 and 1 a box stands in front of it at x = 4.25 and takes
# the middle 5 x 5 rays; in scans 2 .. 5 it is gone and those rays reach the wall.
SCN_W, SCN_CAP, SCN_SCANS = 0.5, 1 << 12, 6


def scenario_scan(k):
    ys = (np.arange(11) - 5) * 0.19  # (no coordinate on a voxel face but y = 0, z = 0)
    pts = []
    for y in ys:
        for z in ys:
            box = k < 2 and abs(y) <= 0.45 and abs(z) <= 0.45
            x = 4.25 if box else 10.25
            pts.append((x, y * x / 10.25, z * x / 10.25, 0.0))  # on the ray to (10.25, y, z)
    return np.array(pts, np.float32)


def scenario_object_keys(ref):
    """The keys of the box's voxels (x voxel 8 at width 0.5)."""
    return [k for k in ref.vox if ((k >> 42) & 0x1FFFFF) - R.BIAS == 8]


# ---------------------------------------------------------------- special rays
# (name, origin o, point p in the sensor frame): the pose is [I | o], so the end is e = p + o
# in fp64, one rounding.  Every number below is a dyadic rational: o, p and e are exact.
# Voxel width 1.0.
_H = (0.5, 0.5, 0.5)
SPECIAL = [("+x", _H, (5.0, 0.0, 0.0)), ("-x", _H, (-5.0, 0.0, 0.0)), ("+y", _H, (0.0, 4.0, 0.0)),
           ("-y", _H, (0.0, -4.0, 0.0)), ("+z", _H, (0.0, 0.0, 6.0)), ("-z", _H, (0.0, 0.0, -6.0)),
           ("tie", _H, (3.0, 3.0, 3.0)),          # tau_x = tau_y = tau_z at every step
           ("tie-mirror", _H, (-3.0, -3.0, -3.0)),
           ("face", (0.5, 0.25, 0.75), (3.5, 1.0, 0.5)),      # e_x = 4.0, on a voxel face
           ("straddle", (-1.25, -0.5, 0.25), (3.0, 1.25, -1.0)),  # o and e on both sides of 0
           ("same-voxel", _H, (0.25, 0.125, -0.25)),  # a == b, S = 0
           ("general", (0.125, -2.75, 1.375), (6.5, 3.25, -4.125))]
SPECIAL_GATE = (0.01, 1e12)  # the dense gate of the special-ray maps


def special_pose(o):
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3)
    T[:, 3] = o
    return T


def special_point(p):
    return np.array([[p[0], p[1], p[2], 0.0]], np.float32)


def special_end(o, p):
    """e as the integration computes it."""
    return R.classify(special_point(p), special_pose(o), 1.0, *SPECIAL_GATE)[1][0]


def voxel_centres(voxels, w):
    """One point at the centre of each voxel (to be integrated at the identity pose)."""
    out = np.zeros((len(voxels), 4), np.float32)
    out[:, :3] = (np.array(voxels, np.float64).reshape(-1, 3) + 0.5) * w
    return out

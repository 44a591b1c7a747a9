"""Rolling the dense voxel map restated in numpy (include/fmx/fmx.h, fmx_roll_evict; DESIGN.md
§Dense map, Rolling) over tests/dense_ref.py's DenseRef: the centre voxel, the inside /
outside decision on the stored keys in integers, the eviction, and the register path's
trigger restated from the poses the registrations ended with.  The tests compare with
equality."""
import numpy as np

import dense_ref as R

HALF_MAX = 1 << 21
_F = ("key", "points", "scan", "index", "hits")


def centre_voxel(centre, voxel_width):
    """floor(c / w) in fp64 as three ints, or None unless every |cc| < 2^20 - 1 (a NaN or an
    infinity fails the comparison)."""
    with np.errstate(all="ignore"):
        c = np.floor(np.asarray(centre, np.float64).reshape(3) / np.float64(voxel_width))
        if not (np.abs(c) < R.LIMIT).all():
            return None
    return [int(v) for v in c]


def unpack_keys(keys):
    """(n, 3) int64 voxel coordinates of packed keys."""
    k = np.asarray(keys, np.uint64).reshape(-1)
    m = np.uint64((1 << 21) - 1)
    v = np.stack([(k >> np.uint64(42)) & m, (k >> np.uint64(21)) & m, k & m], 1)
    return v.astype(np.int64) - R.BIAS


def inside(keys, cc, half):
    """Per key: |v - cc| <= half on all three axes, in 64-bit integers."""
    d = np.abs(unpack_keys(keys) - np.array(cc, np.int64)[None, :])
    return (d <= np.array([int(h) for h in half], np.int64)[None, :]).all(1)


def empty():
    return dict(key=np.zeros(0, np.uint64), points=np.zeros((0, 3)), scan=np.zeros(0, np.uint64),
                index=np.zeros(0, np.uint32), hits=np.zeros(0, np.uint32))


def sort_by_owner(d):
    """Evicted voxels (a drain) by (scan, index), which names a representative uniquely."""
    o = np.lexsort((np.asarray(d["index"]), np.asarray(d["scan"])))
    return dict(points=np.asarray(d["points"], np.float64).reshape(-1, 3)[o], scan=np.asarray(d["scan"], np.uint64)[o],
                index=np.asarray(d["index"], np.uint32)[o], hits=np.asarray(d["hits"], np.uint32)[o])


def same_owner_sorted(a, b):
    for f in ("points", "scan", "index", "hits"):
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if f == "points":
            x, y = x.view(np.uint64), y.view(np.uint64)
        if x.shape != y.shape or not np.array_equal(x, y):
            return f
    return None


class RollRef(R.DenseRef):
    """DenseRef with eviction and the register path's rolling."""

    def __init__(self, voxel_width, max_voxels, min2=1.0, max2=1e4, every=1):
        super().__init__(voxel_width, max_voxels, min2, max2)
        self.every = max(int(every), 1)
        self.spilled = []  # key-sorted dicts, one per roll (scan already resolved)
        self.rolls = []    # (scan, kept, evicted) of every register-path roll
        self.roll_configure(False)

    def clear(self):
        super().clear()
        self.centre = None  # (the spill stays)

    def roll_configure(self, enable, half=(0, 0, 0), step=0.0, spill=True):
        self.roll_on, self.half, self.step, self.spill = bool(enable), [int(h) for h in half], float(step), bool(spill)
        self.centre = None

    # ---- stand-alone
    def _split(self, centre, half):
        cc = centre_voxel(centre, self.w)
        if cc is None or any(int(h) > HALF_MAX for h in half):
            raise ValueError("FMX_E_INVAL")
        ks = np.array(sorted(self.vox), np.uint64)
        m = inside(ks, cc, half)
        return ks[m].tolist(), ks[~m].tolist()

    def count(self, centre, half):
        i, o = self._split(centre, half)
        return len(i), len(o)

    def evict(self, centre, half):
        """Removes the voxels outside the box; returns them key-sorted, scans resolved."""
        _, out = self._split(centre, half)
        if not out:
            return empty()
        ev = dict(key=np.array(out, np.uint64),
                  points=np.array([self.vox[k][3] for k in out], np.float64).reshape(-1, 3),
                  scan=np.array([self.seq_scan[self.vox[k][1]] for k in out], np.uint64),
                  index=np.array([self.vox[k][2] for k in out], np.uint32),
                  hits=np.array([self.vox[k][0] for k in out], np.uint32))
        for k in out:
            del self.vox[k]
        return ev

    # ---- register path
    def before_scan(self, j, n, prev_pose):
        """The roll opportunity at the start of scan j's registration (j >= 1): prev_pose is
        scan j - 1's final pose, n the scan's points.  Returns (kept, evicted) of a roll, or None."""
        if not self.roll_on or j < 1:
            return None
        p = np.asarray(prev_pose, np.float64).reshape(-1, 4)[:3, 3].copy()
        if self.centre is None:
            self.centre = p
            return None
        moved = max(float(np.abs(np.float64(p[k]) - np.float64(self.centre[k]))) for k in range(3))
        due = j % self.every == 0
        if not (moved >= self.step) and not (due and self.voxels + n > self.max_voxels):
            return None
        if centre_voxel(p, self.w) is None:
            return None
        ev = self.evict(p, self.half)
        if self.spill and len(ev["key"]):
            self.spilled.append(ev)
        self.centre = p
        self.rolls.append((int(j), self.voxels, len(ev["key"])))
        return self.voxels, len(ev["key"])

    def register(self, j, xyzw, pose, prev_pose):
        """Scan j as the register path treats it: the roll opportunity, then the integration
        when due.  Returns (roll or None, integrated, counts or None)."""
        n = len(np.asarray(xyzw).reshape(-1, 4))
        roll = self.before_scan(j, n, prev_pose)
        if j % self.every:
            return roll, 0, None
        c = self.integrate(xyzw, pose, j)
        return roll, (1 if c is not None else -1), c

    def drain(self):
        """The spill, sorted by (scan, index); empties it."""
        if not self.spilled:
            d = empty()
        else:
            d = {f: np.concatenate([e[f] for e in self.spilled]) for f in _F}
        self.spilled = []
        return sort_by_owner(d)

    def stats(self):
        last = self.rolls[-1] if self.rolls else (0, 0, 0)
        return dict(rolls=len(self.rolls), evicted=sum(r[2] for r in self.rolls),
                    spilled=sum(len(e["key"]) for e in self.spilled), last_kept=last[1], last_evicted=last[2],
                    last_scan=last[0])

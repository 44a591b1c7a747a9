"""The dense voxel map restated in numpy (include/fmx/fmx.h, fmx_dense_integrate; DESIGN.md
§Dense map): classification, world point, voxel key and the first-wins / hits bookkeeping
over a sequence of integrations.  Every fp32 and fp64 operation is one numpy ufunc call on
arrays of that type, in the order the header states, so each rounds once where the kernel's
does (no contraction): the tests compare with equality."""
import numpy as np

BIAS = 1 << 20
LIMIT = float((1 << 20) - 1)  # valid voxel coordinates: |c| < LIMIT
EMPTY_KEY = (1 << 64) - 1
_M64 = (1 << 64) - 1


def classify(xyzw, pose34, voxel_width, min2, max2):
    """Per point: cls (0 valid, 1 invalid, 2 gated, 3 out of range), world (n, 3) float64,
    key (n,) uint64 (meaningful where cls == 0)."""
    p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
    T = np.ascontiguousarray(pose34, np.float64).reshape(3, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        invalid = ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z)) | ((x == 0) & (y == 0) & (z == 0))
        r2 = ((x * x + y * y) + z * z).astype(np.float64)  # fp32, then widened
        gated = ~invalid & ~((r2 > min2) & (r2 < max2))
        xd, yd, zd = x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)
        world = np.stack([((T[k, 0] * xd + T[k, 1] * yd) + T[k, 2] * zd) + T[k, 3] for k in range(3)], 1)
        c = np.floor(world / np.float64(voxel_width))
        inr = (np.abs(c) < LIMIT).all(1)
    oor = ~invalid & ~gated & ~inr
    cls = np.where(invalid, 1, np.where(gated, 2, np.where(oor, 3, 0))).astype(np.int32)
    ci = np.where((cls == 0)[:, None], c, 0.0).astype(np.int64) + BIAS
    key = (ci[:, 0].astype(np.uint64) << np.uint64(42)) | (ci[:, 1].astype(np.uint64) << np.uint64(21)) | \
        ci[:, 2].astype(np.uint64)
    return cls, world, key


def key_of_points(xyz, voxel_width):
    """The voxel keys of stored world points (all in range)."""
    c = np.floor(np.asarray(xyz, np.float64).reshape(-1, 3) / np.float64(voxel_width)).astype(np.int64) + BIAS
    return (c[:, 0].astype(np.uint64) << np.uint64(42)) | (c[:, 1].astype(np.uint64) << np.uint64(21)) | \
        c[:, 2].astype(np.uint64)


def pack_key(cx, cy, cz):
    return ((cx + BIAS) << 42) | ((cy + BIAS) << 21) | (cz + BIAS)


def mix64(k):
    """The splitmix64 finalizer (fmx_device.hpp)."""
    k &= _M64
    k ^= k >> 30
    k = (k * 0xBF58476D1CE4E5B9) & _M64
    k ^= k >> 27
    k = (k * 0x94D049BB133111EB) & _M64
    k ^= k >> 31
    return k


def home_slot(key, slots):
    return mix64(int(key)) & (slots - 1)


def slots_for(max_voxels):
    s = 2
    while s < 2 * max_voxels:
        s <<= 1
    return s


class DenseRef:
    """The map's state over a sequence of integrations."""

    def __init__(self, voxel_width, max_voxels, min2=1.0, max2=1e4):
        self.w, self.max_voxels, self.min2, self.max2 = float(voxel_width), int(max_voxels), float(min2), float(max2)
        self.clear()

    def clear(self):
        self.vox = {}  # key -> [hits, seq, index, world (3,)]
        self.seq_scan = []

    @property
    def voxels(self):
        return len(self.vox)

    def fits(self, n):
        return self.voxels + n <= self.max_voxels

    def integrate(self, xyzw, pose34, scan_idx=0):
        """The counts dict, or None (nothing changed) when the capacity rule refuses."""
        p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
        if not self.fits(len(p)):
            return None
        cls, world, key = classify(p, pose34, self.w, self.min2, self.max2)
        seq = len(self.seq_scan)
        self.seq_scan.append(int(scan_idx))
        ok = np.flatnonzero(cls == 0)
        uk, first, cnt = np.unique(key[ok], return_index=True, return_counts=True)  # first: lowest index
        added = 0
        for k, f, c in zip(uk.tolist(), first.tolist(), cnt.tolist()):
            v = self.vox.get(k)
            if v is None:
                i = int(ok[f])
                self.vox[k] = [c, seq, i, world[i].copy()]
                added += 1
            else:
                v[0] += c
        return dict(added=added, merged=len(ok) - added, gated=int((cls == 2).sum()),
                    out_of_range=int((cls == 3).sum()), invalid=int((cls == 1).sum()))

    def sorted(self, min_hits=1):
        """key, points, scan, index, hits of the voxels with hits >= min_hits, by key."""
        mh = max(int(min_hits), 1)
        ks = sorted(k for k, v in self.vox.items() if v[0] >= mh)
        return dict(key=np.array(ks, np.uint64),
                    points=np.array([self.vox[k][3] for k in ks], np.float64).reshape(-1, 3),
                    scan=np.array([self.seq_scan[self.vox[k][1]] for k in ks], np.uint64),
                    index=np.array([self.vox[k][2] for k in ks], np.uint32),
                    hits=np.array([self.vox[k][0] for k in ks], np.uint32))


def sort_download(d, voxel_width):
    """A download (Context.dense_download) by key, the keys recomputed from its points."""
    key = key_of_points(d["points"], voxel_width)
    o = np.argsort(key, kind="stable")
    return dict(key=key[o], points=np.asarray(d["points"], np.float64).reshape(-1, 3)[o],
                scan=np.asarray(d["scan"], np.uint64)[o], index=np.asarray(d["index"], np.uint32)[o],
                hits=np.asarray(d["hits"], np.uint32)[o])


def same(a, b):
    """Equality of two key-sorted maps, doubles compared as bits; returns the first field
    that differs, or None."""
    for f in ("key", "points", "scan", "index", "hits"):
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if f == "points":
            x, y = x.view(np.uint64), y.view(np.uint64)
        if x.shape != y.shape or not np.array_equal(x, y):
            return f
    return None

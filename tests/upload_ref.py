"""Loading voxels back into the dense voxel map restated in plain Python (include/fmx/fmx.h,
fmx_upload_voxels; DESIGN.md §Dense map, Restoring) over tests/probe_ref.py, tests/carve_ref.py,
tests/roll_ref.py and tests/dense_ref.py, none of which it changes: the entry classes, the
voxel of an entry, resident-wins, first-position-wins among the entries of one call, the
sums, and the integration count kept apart from the owner numbering.  The tests compare with
equality, doubles as bits."""
import numpy as np

import carve_ref as CR
import dense_ref as R
import probe_ref as PR

M32 = (1 << 32) - 1
COUNT_NAMES = ("added", "merged", "out_of_range", "invalid")


def classify_entries(xyz, hits, voxel_width):
    """Per entry: cls (0 valid, 1 invalid, 3 out of range) and key (meaningful where cls == 0).
    No pose, no gate; a point of exactly (0, 0, 0) is valid."""
    p = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    invalid = ~np.isfinite(p).all(1)
    if hits is not None:
        invalid |= np.asarray(hits, np.uint32).reshape(-1) == 0
    with np.errstate(all="ignore"):
        c = np.floor(p / np.float64(voxel_width))
        inr = (np.abs(c) < R.LIMIT).all(1)  # in fp64, before the cast (a NaN or an infinity fails)
    cls = np.where(invalid, 1, np.where(inr, 0, 3)).astype(np.int32)
    ci = np.where((cls == 0)[:, None], c, 0.0).astype(np.int64) + R.BIAS
    key = (ci[:, 0].astype(np.uint64) << np.uint64(42)) | (ci[:, 1].astype(np.uint64) << np.uint64(21)) | \
        ci[:, 2].astype(np.uint64)
    return cls, key


class UploadRef(PR.ProbeRef):
    """ProbeRef with upload().  seq_scan is the owner table (a voxel's v[1] indexes it): an
    integration appends its scan_idx, an upload one entry per distinct scan value it brings;
    `integrations` is the number fmx_dense_stats reports and the carve's `every` counts."""

    def __init__(self, voxel_width, max_voxels, min2=1.0, max2=1e4, every=1):
        self.integrations = 0
        self.carve_have = False
        super().__init__(voxel_width, max_voxels, min2, max2, every)

    def clear(self):
        super().clear()
        self.integrations = 0

    def carve_configure(self, enable=True, *a, **kw):
        super().carve_configure(enable, *a, **kw)
        self.carve_have = self.carve_have or bool(enable)  # the miss array, once there, stays

    def integrate(self, xyzw, pose34, scan_idx=0):
        """CarveRef.integrate with the integration's own number in place of the owner number."""
        number = self.integrations
        counts = R.DenseRef.integrate(self, xyzw, pose34, scan_idx)
        self.carve_last = (CR.no_counts(), 0)
        if counts is None:
            return None
        self.integrations += 1
        if not self.carve_on or number % self.carve_every:
            return counts
        cls, _, key = R.classify(xyzw, pose34, self.w, self.min2, self.max2)
        self.carve_last = (self._cast(xyzw, pose34, set(key[cls == 0].tolist())), 1)
        return counts

    def upload(self, points, scan=None, index=None, hits=None, misses=None):
        """The counts dict; None (nothing changed) when the capacity rule refuses;
        ValueError("FMX_E_STATE") for misses on a map that never enabled carving."""
        p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        n = len(p)
        if misses is not None and not self.carve_have:
            raise ValueError("FMX_E_STATE")
        if n == 0:
            return dict.fromkeys(COUNT_NAMES, 0)
        if not self.fits(n):
            return None
        col = lambda a, dt: None if a is None else np.asarray(a, dt).reshape(-1)  # noqa: E731
        scan, index, hits, misses = col(scan, np.uint64), col(index, np.uint32), col(hits, np.uint32), col(misses, np.uint32)
        cls, key = classify_entries(p, hits, self.w)
        owner = {}  # scan value -> its place in seq_scan (which place cannot be observed)
        for s in sorted(set(scan.tolist())) if scan is not None else [0]:
            owner[s] = len(self.seq_scan)
            self.seq_scan.append(int(s))
        added = 0
        for i in range(n):  # in input order: the lowest position opens an absent voxel
            if cls[i] != 0:
                continue
            k = int(key[i])
            h = int(hits[i]) if hits is not None else 1
            m = int(misses[i]) if misses is not None else 0
            v = self.vox.get(k)
            if v is None:
                s = int(scan[i]) if scan is not None else 0
                self.vox[k] = [h, owner[s], int(index[i]) if index is not None else 0, p[i].copy()]
                added += 1
            else:
                v[0] = (v[0] + h) & M32
            if m or k in self.misses:
                self.misses[k] = (self.misses.get(k, 0) + m) & M32
        valid = int((cls == 0).sum())
        return dict(added=added, merged=valid - added, out_of_range=int((cls == 3).sum()), invalid=int((cls == 1).sum()))

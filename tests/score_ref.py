"""Scoring many candidate poses of a scan against the dense map restated in plain Python
(include/fmx/fmx.h, fmx_score_poses and fmx_score_plan; DESIGN.md §Dense map, Scoring) over
tests/nearest_ref.py, which it does not change: per pose NearestRef.nearest_voxels on the kept
points, the four counts from that, the found points' dist2 summed with math.fsum (the exact
sum rounded once: the device's fixed-order sum is held against it within a tolerance, every
other figure with equality).  Also form_amd.fmx.rank_scores and the plan, restated."""
import math

import numpy as np

import align_ref as AR
import probe_ref as PR

CLASSES = ("found", "none", "out_of_range", "invalid")
MAX_POSES = 65536
TILE, CAP, CHUNK_POSES, PARTIAL_BYTES, RECORD = 256, 2048, 16384, 32 << 20, 32


def poses_of(poses):
    return np.ascontiguousarray(poses, np.float64).reshape(-1, 3, 4)


def score_poses(ref, xyzw, poses, stride=1, **search):
    """ref: a NearestRef; search: nearest_voxels' reach, max_dist / max_dist2, min_hits,
    max_miss_ratio.  A dict of (K,) arrays: the four counts, sum_d2, and lookups_lo /
    lookups_hi, nearest_voxels' bounds on the device's `lookups`.  A pose that repeats an earlier
    one bit for bit takes its record: the call is a function of the pose alone."""
    p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
    P = poses_of(poses)
    if len(P) > MAX_POSES:
        raise ValueError("FMX_E_INVAL")
    sub = p[AR.kept(len(p), stride)]
    out = {k: np.zeros(len(P), np.uint32) for k in CLASSES}
    out.update(sum_d2=np.zeros(len(P)), lookups_lo=np.zeros(len(P), np.uint64), lookups_hi=np.zeros(len(P), np.uint64))
    seen = {}
    for k in range(len(P)):
        if not np.isfinite(P[k]).all():
            raise ValueError("FMX_E_INVAL")
        rec = seen.get(P[k].tobytes())
        if rec is None:
            got = ref.nearest_voxels(sub, P[k], **search)
            found = got["state"] == PR.SOLID
            rec = (got["counts"], math.fsum(float(d) for d in got["dist2"][found]), got["lookups_bounds"])
            seen[P[k].tobytes()] = rec
        for c in CLASSES:
            out[c][k] = rec[0][c]
        out["sum_d2"][k] = rec[1]
        out["lookups_lo"][k], out["lookups_hi"][k] = rec[2]
    return out


def rank_scores(scores):
    """found descending, then sum_d2 ascending, then the index ascending."""
    return sorted(range(len(scores["found"])), key=lambda k: (-int(scores["found"][k]), float(scores["sum_d2"][k]), k))


def score_plan(n_points, stride, n_poses):
    """fmx_score_plan's six figures; ValueError where it refuses."""
    if n_poses > MAX_POSES or n_points >= 1 << 32:
        raise ValueError("FMX_E_INVAL")
    every = max(int(stride), 1)
    kept = (n_points + every - 1) // every
    tiles = (kept + TILE - 1) // TILE
    chunk = max(1, min(CHUNK_POSES, PARTIAL_BYTES // RECORD // max(tiles, 1)))
    return dict(kept=kept, tile=TILE, tiles=tiles, chunk=chunk, chunks=(n_poses + chunk - 1) // chunk if kept else 0, cap=CAP)

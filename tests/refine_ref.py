"""Refining many candidate poses of a scan against the dense map restated in plain Python
(include/fmx/fmx.h, fmx_refine_systems, fmx_refine_poses and fmx_refine_plan; DESIGN.md §Dense
map, Refining) over tests/nearest_ref.py, tests/align_ref.py and tests/plane_ref.py, which it
does not change: per pose align_ref.system_from (plane_ref.system_from in the plane form) on the
kept points, the sums by math.fsum (the exact sums rounded once: the device's fixed-order sums
are held against them within a tolerance, the counts with equality).  Also the lockstep
Gauss-Newton loop over align_ref.gn_step, and the plan."""
import numpy as np

import align_ref as AR
import plane_ref as PL

CLASSES = ("found", "none", "out_of_range", "invalid", "unoriented")
MAX_POSES = 65536
TILE, CAP, CHUNK_POSES, PARTIAL_BYTES, RECORD = 256, 2048, 16384, 32 << 20, 256


def poses_of(poses):
    return np.ascontiguousarray(poses, np.float64).reshape(-1, 3, 4)


def system_from(ref, xyzw, pose34, sigma=1.0, stride=1, normal_at=None, **search):
    """One pose: (the 29 doubles, the five counts, the bounds on `lookups`).  normal_at: None for
    the point form (unoriented 0), else plane_ref's {(scan, index): normal}."""
    if normal_at is None:
        S, cnt, bounds = AR.system_from(ref.nearest_voxels, xyzw, pose34, sigma, stride, **search)
        cnt = dict(cnt, unoriented=0)
    else:
        S, cnt, bounds = PL.system_from(ref.nearest_voxels, normal_at, xyzw, pose34, sigma, stride, **search)
    return S, {c: cnt[c] for c in CLASSES}, bounds


def counts_of(ref, xyzw, pose34, stride=1, normal_at=None, **search):
    return system_from(ref, xyzw, pose34, 1.0, stride, normal_at, **search)[1]


def systems(ref, xyzw, poses, sigma=1.0, stride=1, normal_at=None, **search):
    """ref: a NearestRef; search: nearest_voxels' reach, max_dist / max_dist2, min_hits,
    max_miss_ratio.  A dict of arrays: system (K, 29), the five counts (K,), lookups_lo /
    lookups_hi.  A pose that repeats an earlier one bit for bit takes its record: the call is a
    function of the pose alone."""
    P = poses_of(poses)
    if len(P) > MAX_POSES:
        raise ValueError("FMX_E_INVAL")
    out = {k: np.zeros(len(P), np.uint32) for k in CLASSES}
    out.update(system=np.zeros((len(P), 29)), lookups_lo=np.zeros(len(P), np.uint64), lookups_hi=np.zeros(len(P), np.uint64))
    seen = {}
    for k in range(len(P)):
        if not np.isfinite(P[k]).all():
            raise ValueError("FMX_E_INVAL")
        rec = seen.get(P[k].tobytes())
        if rec is None:
            rec = seen[P[k].tobytes()] = system_from(ref, xyzw, P[k], sigma, stride, normal_at, **search)
        out["system"][k] = rec[0]
        for c in CLASSES:
            out[c][k] = rec[1][c]
        out["lookups_lo"][k], out["lookups_hi"][k] = rec[2]
    return out


def refine_poses(systems_at, poses_init, max_iters=30, threshold=1e-6):
    """fmx_refine_poses' lockstep loop.  systems_at(list of (3, 4) poses) -> a list of (S,
    counts), called once per round with the poses still running, in list order.  A dict of
    per-pose lists: pose, iters, converged, singular, last_step, error, counts, and `rounds`, the
    number of poses each call was given."""
    P = poses_of(poses_init)
    K = len(P)
    T = [P[k].copy() for k in range(K)]
    out = dict(iters=[0] * K, converged=[False] * K, singular=[False] * K, last_step=[0.0] * K, error=[0.0] * K,
               counts=[None] * K, rounds=[])
    active = list(range(K)) if max_iters else []
    while active:
        recs = systems_at([T[k] for k in active])
        out["rounds"].append(len(active))
        left = []
        for k, (S, cnt) in zip(active, recs):
            out["iters"][k] += 1
            out["error"][k], out["counts"][k] = float(S[28]), cnt
            step = AR.gn_step(S, T[k])
            if step is None:
                out["singular"][k], out["converged"][k], T[k] = True, False, P[k].copy()
                continue
            T[k], out["last_step"][k] = step
            out["converged"][k] = out["last_step"][k] < threshold
            if not out["converged"][k] and out["iters"][k] < max_iters:
                left.append(k)
        active = left
    out["pose"] = T
    return out


def refine_plan(n_points, stride, n_poses):
    """fmx_refine_plan's six figures; ValueError where it refuses."""
    if n_poses > MAX_POSES or n_points >= 1 << 32:
        raise ValueError("FMX_E_INVAL")
    every = max(int(stride), 1)
    kept = (n_points + every - 1) // every
    tiles = (kept + TILE - 1) // TILE
    chunk = max(1, min(CHUNK_POSES, PARTIAL_BYTES // RECORD // max(tiles, 1)))
    return dict(kept=kept, tile=TILE, tiles=tiles, chunk=chunk, chunks=(n_poses + chunk - 1) // chunk if kept else 0, cap=CAP)

"""Point-to-plane alignment against the dense map's normals restated (include/fmx/fmx.h,
fmx_plane_system and fmx_plane_align; DESIGN.md §Dense map, Plane alignment) on top of
tests/align_ref.py, which it does not change: given the points, the pose, a nearest result
and each winner's normal it builds the one row per oriented winner in numpy fp64, one rounding
per written operation, and sums the 29 entries with math.fsum.  The loop is align_ref.align."""
import math

import numpy as np

import align_ref as AR
import probe_ref as PR

CLASSES = ("found", "none", "out_of_range", "invalid", "unoriented")


def rows(xyzw, pose34, state, q, normals, sigma):
    """(F, 7) whitened rows [H * inv, -r * inv] of the F found points whose winner has a normal;
    normals: (N, 3), all zeros where the winner is not oriented."""
    p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    T = np.ascontiguousarray(pose34, np.float64).reshape(3, 4)
    n = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    use = (np.asarray(state) == PR.SOLID) & n.any(axis=1)
    p, q, n = p[use], np.ascontiguousarray(q, np.float64).reshape(-1, 3)[use], n[use]
    inv = 1.0 / float(sigma)
    w = [((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)]
    r = (n[:, 0] * (w[0] - q[:, 0]) + n[:, 1] * (w[1] - q[:, 1])) + n[:, 2] * (w[2] - q[:, 2])
    m = [(T[0, a] * n[:, 0] + T[1, a] * n[:, 1]) + T[2, a] * n[:, 2] for a in range(3)]  # R^T n
    out = np.zeros((len(p), 7))
    out[:, 0] = (m[2] * p[:, 1] - m[1] * p[:, 2]) * inv
    out[:, 1] = (m[0] * p[:, 2] - m[2] * p[:, 0]) * inv
    out[:, 2] = (m[1] * p[:, 0] - m[0] * p[:, 1]) * inv
    out[:, 3], out[:, 4], out[:, 5] = m[0] * inv, m[1] * inv, m[2] * inv
    out[:, 6] = -r * inv
    return out


def system(xyzw, pose34, state, q, normals, sigma):
    """The 29 doubles of fmx_plane_system over the given points (already strided)."""
    v = rows(xyzw, pose34, state, q, normals, sigma)
    S = np.zeros(29)
    for r in range(7):
        for c in range(r, 7):
            S[AR.pack_index(r, c)] = math.fsum((v[:, r] * v[:, c]).tolist())
    S[28] = 0.5 * S[27]
    return S


def counts_of(state, normals, n, stride):
    st = np.asarray(state)
    has = np.asarray(normals).reshape(-1, 3).any(axis=1)
    c = AR.counts_of(st, n, stride)
    c["unoriented"] = int(((st == PR.SOLID) & ~has).sum())
    c["found"] -= c["unoriented"]
    return c


def normals_of(result, normal_at):
    """(N, 3) normals of a nearest result's winners; normal_at: {(scan, index): (3,) normal} (the
    owner names a voxel uniquely in the tests' maps), an owner it lacks, or all zeros, meaning
    no normal."""
    out = np.zeros((len(result["state"]), 3))
    for i in np.flatnonzero(np.asarray(result["state"]) == PR.SOLID):
        n = normal_at.get((int(result["scan"][i]), int(result["index"][i])))
        if n is not None:
            out[i] = n
    return out


def system_from(nearest, normal_at, xyzw, pose34, sigma=1.0, stride=1, **kw):
    """nearest(points, pose34, **kw) -> a nearest result; the system, the six counts and the
    result's lookups_bounds over the points i % stride == 0."""
    p = np.ascontiguousarray(xyzw, np.float32).reshape(-1, 4)
    sub = p[AR.kept(len(p), stride)]
    got = nearest(sub, pose34, **kw)
    nrm = normals_of(got, normal_at)
    return system(sub, pose34, got["state"], got["points"], nrm, sigma), counts_of(got["state"], nrm, len(p), stride), \
        got.get("lookups_bounds")


def by_owner(scan, index, normals):
    """{(scan, index): normal} of a normals download."""
    return {(int(s), int(i)): np.asarray(n, np.float64) for s, i, n in zip(scan, index, normals)}


def by_owner_of(ref, built, fp32=True):
    """... of normals_ref.build(ref)'s records, rounded to fp32 as the device stores them."""
    out = {}
    for key, rec in built.items():
        v = ref.vox[key]
        n = np.asarray(rec["normal"], np.float64)
        out[(int(ref.seq_scan[v[1]]), int(v[2]))] = n.astype(np.float32).astype(np.float64) if fp32 else n
    return out


# ---- the zero-residual problem of tests/test_normals_cpu.py and tests/test_gpu_plane.py
ZERO_THRESHOLD = 1e-6
ZERO_XI = (0.004, -0.003, 0.005, 0.03, -0.02, 0.025)  # the initial pose is Exp(ZERO_XI)
# the build of its map: only a voxel whose neighbours all lie in its own plane is oriented (a
# border voxel that sees a second plane has a flatness far above this)
ZERO_BUILD = dict(reach=1, min_support=5, max_flatness=1e-6)


def zero_residual_cloud(seed=5):
    """Three exact planes x = 0.5, y = 0.5, z = 0.5 at voxel width 1: a 7 x 7 patch of voxels on
    each, one fp32 point per voxel at least 0.25 inside its cell in the plane, and Exp(ZERO_XI):
    a scan that is the map itself, seen from a pose a few centimetres and milliradians off.  The
    covariance of an exact axis plane has a zero row: the normal is the axis exactly."""
    g = np.random.default_rng(seed)
    rows_ = []
    for a in range(3):
        for i in range(7):
            for j in range(7):
                p = [i + 1.5 + g.uniform(-0.25, 0.25), j + 1.5 + g.uniform(-0.25, 0.25)]
                p.insert(a, 0.5)
                rows_.append(p)
    p = np.zeros((len(rows_), 4), np.float32)
    p[:, :3] = np.asarray(rows_, np.float32)
    return p, AR.expmap(ZERO_XI)
